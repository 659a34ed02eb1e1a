// hashgan_amd -- the relevant-row histogram: k_hist's pass over the pairs with the label match (metric.py:17-19) folded in.
//
// Per query and distance d the pass counts the rows at distance d twice over: those that share a label with the query and
// those that do not.  Hash-lookup evaluation reads everything from that table -- ball sizes, hits inside the ball, the recall
// denominator -- for every radius at once, with no ranking and no lists.
//
// k_hist's structure (lane = query, unit = segment x 64 queries, rows through scalar-load batches with the software prefetch),
// and still ONE LDS atomic per pair: the lane's column has two counters per distance,
//     h[(d * 2 + match) * 64 + lane],
// so bank = lane % 32 as before.  The row's label words ride in the same scalar batch as its code words (no per-pair gather);
// the query's label words stay in registers (<= 128 classes).  Wider label rows are walked two words at a time, once per batch:
// the lane reloads its two query words per batch (not per pair) and folds the batch's matches into a bit mask.
// Output part[s][d * 2 + match][q], q fastest; k_hist_rel_reduce sums the segments and forms all = irrelevant + relevant.
// Counters are u32 and a segment has < 2^32 rows: exact for any segment length.
#pragma once
#include "hg_kernels.hpp"

namespace hg {

// Rows per scalar-load batch: the current and the prefetched batch (code words + label words as dwords) stay within ~80 SGPRs.
constexpr int rel_batch_rows(int nw, int lwc) {
    int r = 40 / (nw + 2 * lwc), p = 1;
    while (p * 2 <= r) p *= 2;
    return p > 16 ? 16 : (p < 2 ? 2 : p);
}

// LWT = 64-bit label words per row (1 or 2: kept in registers), 0 = any width (g.LW words, walked two at a time per batch)
template <int NW, int LWT>
__global__ __launch_bounds__(256) void k_hist_rel(const u32* __restrict__ qc, const u64* __restrict__ qlab,
                                                  const u32* __restrict__ db, const u64* __restrict__ dblab,
                                                  u32* __restrict__ part, const Geo g) {
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const int lb = logical_block(g.nBlk);
    if (lb < 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const i64 unit = (i64)lb * g.wpb + wave;
    if (unit >= g.nUnits) return;
    const int s = (int)(unit / g.nQT);
    const int qt = (int)(unit - (i64)s * g.nQT);
    const int q = qt * 64 + lane;
    const bool live = q < g.Q;
    constexpr int LWC = LWT > 0 ? LWT : 2;
    const int LW = LWT > 0 ? LWT : g.LW;

    u32 qw[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) qw[w] = live ? qc[(i64)q * NW + w] : 0u;
    u64 ql[LWC];
#pragma unroll
    for (int w = 0; w < LWC; ++w) ql[w] = (LWT > 0 && live) ? qlab[(i64)q * LWT + w] : 0ull;
    const u64* __restrict__ qlrow = qlab + (i64)(live ? q : 0) * LW;      // (LWT = 0: reloaded per batch)

    u32* h = lds + wave * g.NB * 128;                  // [NB][2][64]: a lane only ever touches its own column
    for (int i = 0; i < 2 * g.NB; ++i) h[i * 64 + lane] = 0u;

    // LWT = 0: bit j of the result = row j of the `rows` rows at pl shares a label with the lane's query
    auto wide_mask = [&](const u64* __restrict__ pl, const int rows) -> u32 {
        u32 mm = 0;
        for (int w0 = 0; w0 < LW; w0 += 2) {
            const bool two = w0 + 1 < LW;
            const u64 a0 = live ? qlrow[w0] : 0ull;
            const u64 a1 = live && two ? qlrow[w0 + 1] : 0ull;
            for (int j = 0; j < rows; ++j) {
                const u64* __restrict__ r = pl + (i64)j * LW + w0;       // wave-uniform: scalar loads
                u64 x = r[0] & a0;
                if (two) x |= r[1] & a1;
                mm |= (x != 0ull ? 1u : 0u) << j;
            }
        }
        return mm;
    };

    const i64 lo = (i64)s * g.L;
    const i64 hi = lo + g.L < g.N ? lo + g.L : g.N;
    const u32* __restrict__ p = db + lo * NW;
    const u64* __restrict__ pl = dblab + lo * LW;
    i64 n = lo;
    constexpr int B = rel_batch_rows(NW, LWC);
    constexpr int LB = LWT > 0 ? B * LWT : 1;          // label words of a batch kept in scalars
    // k_hist's software prefetch: the next batch's scalar loads go out right after the first row of the current one
    if (n + B <= hi) {
        u32 c[B * NW];
        u64 l[LB];
#pragma unroll
        for (int i = 0; i < B * NW; ++i) c[i] = p[i];
#pragma unroll
        for (int i = 0; i < LB; ++i) l[i] = LWT > 0 ? pl[i] : 0ull;
        for (; n + B <= hi; n += B, p += B * NW, pl += (i64)B * LW) {
            const bool more = n + 2 * B <= hi;
            u32 mm = 0;
            if constexpr (LWT == 0) mm = wide_mask(pl, B);
            auto row = [&](const int j) {
                u32 d = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) d += __builtin_popcount(qw[w] ^ c[j * NW + w]);
                u32 m;
                if constexpr (LWT > 0) {
                    u64 x = 0;
#pragma unroll
                    for (int w = 0; w < LWT; ++w) x |= l[j * LWT + w] & ql[w];
                    m = x != 0ull ? 1u : 0u;
                } else {
                    m = (mm >> j) & 1u;
                }
                atomicAdd(&h[(d * 2 + m) * 64 + lane], 1u);
            };
            row(0);
            __builtin_amdgcn_sched_barrier(0);
            u32 cn[B * NW];
            u64 ln[LB];
            if (more) {
#pragma unroll
                for (int i = 0; i < B * NW; ++i) cn[i] = p[B * NW + i];
#pragma unroll
                for (int i = 0; i < LB; ++i) ln[i] = LWT > 0 ? pl[B * LWT + i] : 0ull;
            } else {
#pragma unroll
                for (int i = 0; i < B * NW; ++i) cn[i] = 0u;
#pragma unroll
                for (int i = 0; i < LB; ++i) ln[i] = 0ull;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 1; j < B; ++j) row(j);
#pragma unroll
            for (int i = 0; i < B * NW; ++i) c[i] = cn[i];
#pragma unroll
            for (int i = 0; i < LB; ++i) l[i] = ln[i];
        }
    }
    for (; n < hi; ++n, p += NW, pl += LW) {           // ragged tail of the segment
        const u32 d = hamming<NW>(qw, p);
        u32 m;
        if constexpr (LWT > 0) {
            u64 x = 0;
#pragma unroll
            for (int w = 0; w < LWT; ++w) x |= pl[w] & ql[w];
            m = x != 0ull ? 1u : 0u;
        } else {
            m = wide_mask(pl, 1) & 1u;
        }
        atomicAdd(&h[(d * 2 + m) * 64 + lane], 1u);
    }
    u32* __restrict__ out = part + (i64)s * 2 * g.NB * g.Qpad + q;
    for (int i = 0; i < 2 * g.NB; ++i) out[(i64)i * g.Qpad] = h[i * 64 + lane];
}

// all[d][q] = sum over segments of both counters, rel[d][q] = of the relevant one
static __global__ __launch_bounds__(256) void k_hist_rel_reduce(const u32* __restrict__ part, u32* __restrict__ all,
                                                                u32* __restrict__ rel, const Geo g) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 plane = (i64)g.NB * g.Qpad;
    if (i >= plane) return;
    const i64 d = i / g.Qpad, q = i - d * g.Qpad;
    const u32* __restrict__ src = part + 2 * d * g.Qpad + q;
    u32 a0 = 0, a1 = 0;
    for (int s = 0; s < g.S; ++s) {
        a0 += src[(i64)s * 2 * plane];
        a1 += src[(i64)s * 2 * plane + g.Qpad];
    }
    all[i] = a0 + a1;
    rel[i] = a1;
}

}  // namespace hg

// hashgan_amd -- the distance-by-grade histogram: k_hist_rel's pass over the pairs with the GRADE of the pair (labels the row shares
// with the query, hg_graded.hpp) in place of the match bit.
//
// Per query, distance d and grade g the pass counts the rows at distance d that share exactly g labels with the query: J[d][g][q].
// Tie-aware graded metrics -- expected DCG@k and ACG@k over the orders inside the Hamming tie groups, and their exact extremes --
// are functions of that table alone (extra_metrics.tie_graded_from_tables); hg_rel_hist's table is J collapsed to g = 0 / g > 0,
// hg_grade_hist's is J summed over d, and neither gives the joint table back.
//
// k_hist_rel's structure (lane = query, unit = segment x 64 queries, rows and their label words through scalar-load batches with the
// software prefetch, the query's code and label words in registers up to 128 classes) and still ONE LDS atomic per pair: the lane's
// column has G counters per distance,
//     h[(d * G + g) * 64 + lane],
// so bank = lane % 32 as before.  G = 1 + min(most labels on a query, most labels on a database row) bounds every pair's grade
// (k_label_max; the popcounts are taken under the same mask of the last label word as the grades, so a grade never leaves the column).
// Wider label rows are walked two words at a time, once per batch: the lane reloads its two query words per batch (not per pair)
// and adds up one popcount per row of the batch.
//
// A wavefront's column is NB * G * 256 bytes, which outgrows the 160 KiB of a workgroup when NB * G > 640.  The distance range is then
// cut into `bands` of bw = 640 / G distances: a block serves one (unit, band), computes d and g of every row of its segment and counts
// the pairs whose d lies in [band * bw, band * bw + bw).  Every band writes planes of its own, so the table is the same for any band count.
// Output part[s][d * G + g][q], q fastest; k_hist_joint_reduce sums the segments.  Counters are u32 and a segment has < 2^32 rows: exact
// for any segment length.
#pragma once
#include "hg_hist_rel.hpp"

namespace hg {

constexpr int HJ_LDS_CELLS = 640;      // (distance, grade) cells of one wavefront's column that fit 160 KiB: 640 * 256 B

struct JointArgs {
    int G;              // grades 0 .. G - 1
    int bands, bw;      // distance bands, distances per band (bands = 1: bw = NB)
    u64 lastmask;       // the classes of the last label word
};

// out[0] = most labels on a query, out[1] = most labels on a database row (both zeroed by the caller): one thread per row, a
// butterfly per wavefront, one integer atomicMax per wavefront -- order-independent.  Threads [0, Qpad) take the queries, threads
// [Qpad, Qpad + N) the database rows: a wavefront never holds rows of both tables.
static __global__ __launch_bounds__(256) void k_label_max(const u64* __restrict__ qlab, const u64* __restrict__ dblab, const i64 Q,
                                                          const i64 Qpad, const i64 N, const int LW, const u64 lastmask,
                                                          u32* __restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 r = i - Qpad;
    const u64* __restrict__ row = i < Q ? qlab + i * LW : (r >= 0 && r < N ? dblab + r * LW : nullptr);
    u32 x = 0;
    if (row)
        for (int w = 0; w < LW; ++w) x += (u32)__popcll(w == LW - 1 ? row[w] & lastmask : row[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 y = (u32)__shfl_xor((int)x, d, 64);
        x = x > y ? x : y;
    }
    if ((threadIdx.x & 63) == 0 && x > 0) atomicMax(&out[i < Qpad ? 0 : 1], x);
}

// LWT = 64-bit label words per row (1 or 2: kept in registers), 0 = any width (g.LW words, walked two at a time per batch)
// g.nBlk counts (unit block, band) pairs, band fastest; dynamic LDS: wpb * min(NB, bw) * G * 256 bytes.
template <int NW, int LWT>
__global__ __launch_bounds__(256) void k_hist_joint(const u32* __restrict__ qc, const u64* __restrict__ qlab,
                                                    const u32* __restrict__ db, const u64* __restrict__ dblab,
                                                    u32* __restrict__ part, const Geo g, const JointArgs ja) {
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const int lb = logical_block(g.nBlk);
    if (lb < 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ub = lb / ja.bands;
    const int band = lb - ub * ja.bands;
    const i64 unit = (i64)ub * g.wpb + wave;
    if (unit >= g.nUnits) return;
    const int s = (int)(unit / g.nQT);
    const int qt = (int)(unit - (i64)s * g.nQT);
    const int q = qt * 64 + lane;
    const bool live = q < g.Q;
    constexpr int LWC = LWT > 0 ? LWT : 2;
    const int LW = LWT > 0 ? LWT : g.LW;
    const u32 G = (u32)ja.G;
    const int d0 = band * ja.bw;                       // the band's distances: [d0, d0 + nd)
    const int nd = g.NB - d0 < ja.bw ? g.NB - d0 : ja.bw;
    const u32 first = (u32)d0 * G, cells = (u32)nd * G;     // ... are the cells [first, first + cells) of the whole column

    u32 qw[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) qw[w] = live ? qc[(i64)q * NW + w] : 0u;
    u64 ql[LWC];
#pragma unroll
    for (int w = 0; w < LWC; ++w) ql[w] = (LWT > 0 && live) ? qlab[(i64)q * LWT + w] : 0ull;
    if constexpr (LWT > 0) ql[LWT - 1] &= ja.lastmask;
    const u64* __restrict__ qlrow = qlab + (i64)(live ? q : 0) * LW;      // (LWT = 0: reloaded per batch)

    u32* h = lds + wave * ja.bw * ja.G * 64;           // [nd][G][64]: a lane only ever touches its own column
    for (u32 i = 0; i < cells; ++i) h[i * 64 + lane] = 0u;
    // the band's planes of this segment's block (the address is formed here: a per-lane value, so the scalars behind it are free in the loop)
    u32* __restrict__ out = part + ((i64)s * g.NB * G + first) * g.Qpad + q;

    // one pair: a cell outside the band is another block's (gr < G, so the cell lies in the band iff d does; unsigned compare: a cell
    // before the band wraps)
    auto count = [&](const u32 d, const u32 gr) {
        const u32 cell = d * G + gr - first;
        if (cell < cells) atomicAdd(&h[cell * 64 + lane], 1u);
    };
    constexpr int B = rel_batch_rows(NW, LWC);
    // LWT = 0: gr[j] = grade of row j of the B rows at pl against the lane's query
    auto wide_grades = [&](const u64* __restrict__ pl, u32 (&gr)[B]) {
#pragma unroll
        for (int j = 0; j < B; ++j) gr[j] = 0u;
        for (int w0 = 0; w0 < LW; w0 += 2) {
            const bool two = w0 + 1 < LW;
            u64 a0 = live ? qlrow[w0] : 0ull;
            u64 a1 = live && two ? qlrow[w0 + 1] : 0ull;
            if (w0 == LW - 1) a0 &= ja.lastmask;
            if (w0 + 1 == LW - 1) a1 &= ja.lastmask;
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const u64* __restrict__ r = pl + (i64)j * LW + w0;       // wave-uniform: scalar loads
                gr[j] += (u32)__popcll(r[0] & a0);
                if (two) gr[j] += (u32)__popcll(r[1] & a1);
            }
        }
    };
    // ... and of one row (the segment's ragged tail)
    auto wide_grade = [&](const u64* __restrict__ r) -> u32 {
        u32 x = 0;
        for (int w = 0; w < LW; ++w) {
            u64 a = live ? qlrow[w] : 0ull;
            if (w == LW - 1) a &= ja.lastmask;
            x += (u32)__popcll(r[w] & a);
        }
        return x;
    };

    const i64 lo = (i64)s * g.L;
    const i64 hi = lo + g.L < g.N ? lo + g.L : g.N;
    const u32* __restrict__ p = db + lo * NW;
    const u64* __restrict__ pl = dblab + lo * LW;
    const u32* const pend = db + hi * NW;              // (the code pointer counts the rows: one scalar pair less than an index beside it)
    constexpr int LB = LWT > 0 ? B * LWT : 1;          // label words of a batch kept in scalars
    // k_hist's software prefetch: the next batch's scalar loads go out right after the first row of the current one
    if (p + B * NW <= pend) {
        u32 c[B * NW];
        u64 l[LB];
#pragma unroll
        for (int i = 0; i < B * NW; ++i) c[i] = p[i];
#pragma unroll
        for (int i = 0; i < LB; ++i) l[i] = LWT > 0 ? pl[i] : 0ull;
        for (; p + B * NW <= pend; p += B * NW, pl += (i64)B * LW) {
            const bool more = p + 2 * B * NW <= pend;
            u32 gr[B];
            if constexpr (LWT == 0) wide_grades(pl, gr);
            auto row = [&](const int j) {
                u32 d = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) d += __builtin_popcount(qw[w] ^ c[j * NW + w]);
                u32 x;
                if constexpr (LWT > 0) {
                    x = 0;
#pragma unroll
                    for (int w = 0; w < LWT; ++w) x += (u32)__popcll(l[j * LWT + w] & ql[w]);
                } else {
                    x = gr[j];
                }
                count(d, x);
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
    for (; p < pend; p += NW, pl += LW) {           // ragged tail of the segment
        const u32 d = hamming<NW>(qw, p);
        u32 x;
        if constexpr (LWT > 0) {
            x = 0;
#pragma unroll
            for (int w = 0; w < LWT; ++w) x += (u32)__popcll(pl[w] & ql[w]);
        } else {
            x = wide_grade(pl);
        }
        count(d, x);
    }
    for (u32 i = 0; i < cells; ++i) out[(i64)i * g.Qpad] = h[i * 64 + lane];
}

// tab[d * G + g][q] = sum over the segments
static __global__ __launch_bounds__(256) void k_hist_joint_reduce(const u32* __restrict__ part, u32* __restrict__ tab,
                                                                  const i64 plane, const int S) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    u32 acc = 0;
    for (int s = 0; s < S; ++s) acc += part[(i64)s * plane + i];
    tab[i] = acc;
}

}  // namespace hg

// hashgan_amd -- graded relevance for multi-label retrieval: the grade of a (query, row) pair is the number of labels they
// share, popcount(qlab & dblab).  Two passes:
//
// k_graded        along the ranked lists the last ranking left on the device (out_idx), one workgroup per query: per cut-off k
//                 of an ascending list ks, S_k = sum of the grades of the first k ranks, hits_k = ranks with grade > 0,
//                 dcg_k = sum gain[g_i] * disc[i], wsum_k = sum over the ranks with g_i > 0 of S_i / i.  ACG, NDCG's numerator and
//                 WAP at every k come from those four [Q][nk] tables; nothing of size Q x R leaves the device (unless the grade
//                 bytes themselves are asked for).
// k_grade_hist    over the Q x N label pairs, no codes and no ranking: rows per (grade, query).  The ideal ordering NDCG
//                 divides by is "all rows sorted by grade", so IDCG at any k follows from this table on the host in O(Q C).
//
// k_graded's summation order is fixed by ks alone: the list is walked in chunks of 256 ranks that never straddle a cut-off
// (a chunk ends at the next k or after 256 ranks, whichever comes first; the lanes past the end hold zeros), the grades are
// scanned across the wavefront (shuffles) and across the four wavefronts (LDS), each lane forms its two float64 terms
// -- gain[g] * disc[i], one rounded product, and S_i / i, one rounded division --, a wavefront sums them by a butterfly of
// shuffles (every lane ends with the same bits: the additions pair the same operands), the four wavefront sums are added in
// wavefront order and the chunk's sum joins the running total.  No float atomic, no order that depends on timing.
//
// k_grade_hist has k_hist_rel's structure (hg_hist_rel.hpp): lane = query, unit = segment x 64 queries, the rows' label words
// through scalar-load batches with the software prefetch, the query's label words in registers up to 128 classes and walked two
// at a time beyond; the lane's LDS column is h[g * 64 + lane], one ds_add_u32 per pair (a lane only touches its own column, so a
// read-modify-write would do -- the atomic without return is the leaner code: one LDS instruction and no wait for a result).
// Bits past class C - 1 of the query's last label word are masked off once, so a grade never exceeds C and never leaves the column.
// Output part[s][g][q], q fastest; k_grade_hist_reduce sums the segments.  Counters are u32: exact for any segment length.
#pragma once
#include "hg_kernels.hpp"

namespace hg {

constexpr int GR_THREADS = 256;        // k_graded's block: four wavefronts, one chunk of the list per step
constexpr int GR_MAX_K = 64;           // cut-offs per pass
constexpr int GR_MAX_C = 255;          // a grade is a byte

struct GradedArgs {
    const u32* idx;                    // [Q][R] ranked row indices (IDX_NONE / anything outside the table: grade 0, never followed)
    const u64* dblab; const u64* qlab; // label words, LW per row
    const i64* ks;                     // [nk] ascending cut-offs, 1 <= k <= R
    const double* gain;                // [C + 1]
    const double* disc;                // [ks[nk - 1]], disc[i] for rank i + 1
    i64* gsum; i64* hits;              // [Q][nk]
    double* dcg; double* wsum;         // [Q][nk]
    u8* grades;                        // [Q][R], or null
    i64 R, N;
    int nk, LW;
    u64 lastmask;                      // the classes of the last label word
    const u8* plane; i64 Rp;           // PLANE: the grade bytes [Q][Rp] of the whole database's lists (hg_list_merge.hpp) instead of idx / dblab / qlab
};

__device__ __forceinline__ u32 grade_of(const GradedArgs& a, const u64* __restrict__ ql, const u32 gi) {
    if ((i64)gi >= a.N) return 0u;     // (IDX_NONE included: N < 2^32 - 1)
    const u64* __restrict__ dl = a.dblab + (i64)gi * a.LW;
    u32 g = 0;
    for (int w = 0; w < a.LW; ++w) {
        u64 m = ql[w];                 // wave-uniform: scalar loads
        if (w == a.LW - 1) m &= a.lastmask;
        g += (u32)__popcll(dl[w] & m);
    }
    return g;
}

__device__ __forceinline__ u32 wave_scan_u32(u32 v, const int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// PLANE: the grade of rank i is plane[q][i], a shard's merged grade plane, not gathered through idx.  Everything after the grade is
// the same code, so the sums have the bits the gather gives on one context with the whole database.
template <bool PLANE>
__global__ __launch_bounds__(GR_THREADS) void k_graded(const GradedArgs a) {
    __shared__ u32 sg[GR_THREADS / 64], sh[GR_THREADS / 64];
    __shared__ double sd[GR_THREADS / 64], sw[GR_THREADS / 64];
    const int q = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32* __restrict__ idx = a.idx + (i64)q * a.R;
    const u64* __restrict__ ql = a.qlab + (i64)q * a.LW;
    u8* __restrict__ gr = a.grades ? a.grades + (i64)q * a.R : nullptr;
    const u8* __restrict__ pg = PLANE ? a.plane + (i64)q * a.Rp : nullptr;

    i64 S = 0, H = 0;                  // running totals, the same in every thread
    double dcg = 0.0, ws = 0.0;
    i64 pos = 0;
    for (int j = 0; j < a.nk;) {
        const i64 kj = a.ks[j];
        const i64 end = pos + GR_THREADS < kj ? pos + GR_THREADS : kj;
        const i64 i = pos + tid;
        const bool act = i < end;
        u32 g = 0u;
        if constexpr (PLANE) g = act ? (u32)pg[i] : 0u;
        else g = act ? grade_of(a, ql, idx[i]) : 0u;
        if (act && gr) gr[i] = (u8)g;
        const u32 incl = wave_scan_u32(g, lane);
        const u32 wh = (u32)__popcll(__ballot(g > 0u));
        const double t1 = wave_sum_f64(act ? __dmul_rn(a.gain[g], a.disc[i]) : 0.0);
        if (lane == 63) sg[wave] = incl;
        if (lane == 0) { sh[wave] = wh; sd[wave] = t1; }
        __syncthreads();
        u32 before = 0, tot = 0, th = 0;
        double td = 0.0;
#pragma unroll
        for (int w = 0; w < GR_THREADS / 64; ++w) {
            const u32 x = sg[w];
            before += w < wave ? x : 0u;
            tot += x;
            th += sh[w];
            td += sd[w];
        }
        const i64 Si = S + (i64)(before + incl);
        const double t2 = wave_sum_f64(g > 0u ? (double)Si / (double)(i + 1) : 0.0);
        if (lane == 0) sw[wave] = t2;
        __syncthreads();               // (sg / sh / sd are written again only after this barrier, sw only after the next one)
        double tw = 0.0;
#pragma unroll
        for (int w = 0; w < GR_THREADS / 64; ++w) tw += sw[w];
        S += tot; H += th; dcg += td; ws += tw;
        pos = end;
        if (pos == kj) {
            if (tid == 0) {
                const i64 o = (i64)q * a.nk + j;
                a.gsum[o] = S; a.hits[o] = H; a.dcg[o] = dcg; a.wsum[o] = ws;
            }
            ++j;
        }
    }
    if (gr)                            // the grade bytes of the ranks past the last cut-off
        for (i64 i = pos + tid; i < a.R; i += GR_THREADS) gr[i] = PLANE ? pg[i] : (u8)grade_of(a, ql, idx[i]);
}

// Rows per scalar-load batch: the current and the prefetched batch of label words stay within 64 SGPRs.
constexpr int grade_batch_rows(int lwt) { return lwt == 1 ? 16 : 8; }

// LWT = 64-bit label words per row (1 or 2: kept in registers), 0 = any width (g.LW words, walked two at a time per batch)
// G = C + 1 bins; dynamic LDS: wpb * G * 256 bytes.
template <int LWT>
__global__ __launch_bounds__(256) void k_grade_hist(const u64* __restrict__ qlab, const u64* __restrict__ dblab,
                                                    u32* __restrict__ part, const Geo g, const int G, const u64 lastmask) {
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
    const int LW = LWT > 0 ? LWT : g.LW;

    u32* h = lds + wave * G * 64;                      // [G][64]: a lane only ever touches its own column
    for (int i = 0; i < G; ++i) h[i * 64 + lane] = 0u;

    const i64 lo = (i64)s * g.L;
    const i64 hi = lo + g.L < g.N ? lo + g.L : g.N;
    const u64* __restrict__ pl = dblab + lo * LW;
    i64 n = lo;
    if constexpr (LWT > 0) {
        u64 ql[LWT];
#pragma unroll
        for (int w = 0; w < LWT; ++w) ql[w] = live ? qlab[(i64)q * LWT + w] : 0ull;
        ql[LWT - 1] &= lastmask;
        constexpr int B = grade_batch_rows(LWT);
        constexpr int LB = B * LWT;
        auto grade = [&](const u64* l) -> u32 {
            u32 x = 0;
#pragma unroll
            for (int w = 0; w < LWT; ++w) x += (u32)__popcll(l[w] & ql[w]);
            return x;
        };
        // k_hist's software prefetch: the next batch's scalar loads go out right after the first row of the current one
        if (n + B <= hi) {
            u64 l[LB];
#pragma unroll
            for (int i = 0; i < LB; ++i) l[i] = pl[i];
            for (; n + B <= hi; n += B, pl += LB) {
                const bool more = n + 2 * B <= hi;
                atomicAdd(&h[grade(l) * 64 + lane], 1u);
                __builtin_amdgcn_sched_barrier(0);
                u64 ln[LB];
                if (more) {
#pragma unroll
                    for (int i = 0; i < LB; ++i) ln[i] = pl[LB + i];
                } else {
#pragma unroll
                    for (int i = 0; i < LB; ++i) ln[i] = 0ull;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 1; j < B; ++j) atomicAdd(&h[grade(l + j * LWT) * 64 + lane], 1u);
#pragma unroll
                for (int i = 0; i < LB; ++i) l[i] = ln[i];
            }
        }
        for (; n < hi; ++n, pl += LWT) {               // ragged tail of the segment
            u32 x = 0;
#pragma unroll
            for (int w = 0; w < LWT; ++w) x += (u32)__popcll(pl[w] & ql[w]);
            atomicAdd(&h[x * 64 + lane], 1u);
        }
    } else {
        // wide label rows: per batch the lane reloads its query words two at a time and adds up the batch's grades
        constexpr int B = 8;
        const u64* __restrict__ qlrow = qlab + (i64)(live ? q : 0) * LW;
        for (; n < hi; n += B, pl += (i64)B * LW) {
            const int rows = hi - n < B ? (int)(hi - n) : B;
            u32 gr[B];
#pragma unroll
            for (int j = 0; j < B; ++j) gr[j] = 0u;
            for (int w0 = 0; w0 < LW; w0 += 2) {
                const bool two = w0 + 1 < LW;
                u64 a0 = live ? qlrow[w0] : 0ull;
                u64 a1 = live && two ? qlrow[w0 + 1] : 0ull;
                if (w0 == LW - 1) a0 &= lastmask;
                if (w0 + 1 == LW - 1) a1 &= lastmask;
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    if (j < rows) {
                        const u64* __restrict__ r = pl + (i64)j * LW + w0;       // wave-uniform: scalar loads
                        gr[j] += (u32)__popcll(r[0] & a0);
                        if (two) gr[j] += (u32)__popcll(r[1] & a1);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < B; ++j)
                if (j < rows) atomicAdd(&h[gr[j] * 64 + lane], 1u);
        }
    }
    u32* __restrict__ out = part + (i64)s * G * g.Qpad + q;
    for (int i = 0; i < G; ++i) out[(i64)i * g.Qpad] = h[i * 64 + lane];
}

// hist[g][q] = sum over the segments
static __global__ __launch_bounds__(256) void k_grade_hist_reduce(const u32* __restrict__ part, u32* __restrict__ hist,
                                                                  const i64 plane, const int S) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    u32 acc = 0;
    for (int s = 0; s < S; ++s) acc += part[(i64)s * plane + i];
    hist[i] = acc;
}

}  // namespace hg

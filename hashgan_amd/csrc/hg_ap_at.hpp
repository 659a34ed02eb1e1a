// hashgan_amd -- AP@R and the hits among the top R at many cut-offs R_0 < R_1 < ... from ONE ranking (hg_ap_at).
//
// The canonical order is total, so the top R_j is a prefix of the top R_max and the match bitmap one ranking at R_max left on the
// device holds every cut-off's row.  px[k] * imatch[k] (metric.py:20-22) does not depend on R, and np.sum adds 8192-element chunks
// left to right (hg_kernels.hpp, K6): every cut-off beyond a full chunk shares that chunk's sum, only the last, partial chunk of a
// cut-off needs a summation tree of its own.  ap[q][j] has the bits k_ap gives for R = R_j: the element values of ap_eval2 (the
// Markstein step against RN(1 / k)) or of ap_eval (a division, without the table), the same eight strided accumulators per leaf with
// the xor tree and the sequential tail, the same left + right node additions, the same chunk accumulation, the same total / rel.
//
// k_ap_at, one workgroup of NT threads (NT / 64 wavefronts) per query, chunk by chunk:
//   1  the chunk's 128 words come from global memory once, their popcount prefix is built once (two wavefronts);
//   2  the evaluations ("tasks") of the chunk: the full 8192-element tree when a cut-off ends at the chunk's end or beyond it, and
//      the tree of R_j - chunk base elements for every cut-off that ends inside the chunk.  NT / 64 tasks at a time:
//        a  their leaves, eight to a wavefront step (eight lanes per leaf), dealt round robin over all wavefronts -- a long and a short
//           tree side by side keep every wavefront busy -- each leaf sum into the task's 2 KB of tree scratch;
//        b  wavefront w walks the tree of task w level by level (wavefront-level synchronisation only) and its lane 0 writes
//           ap[q][j] = (sum of the full chunks before + this sum) / rel, rel[q][j] from the same prefix counts.
//   3  the full tree's sum joins the running total that every later cut-off starts from.
// Float64 throughout, no atomics; a task's additions are a function of the query's row and R_j alone: not of Q, not of the other
// cut-offs, not of NT.
#pragma once
#include "hg_kernels.hpp"

namespace hg {

constexpr int AA_MAX_R = 64;           // cut-offs per pass

struct ApAtArgs {
    const u64* mbits;                  // [Q][RW] the ranking's match bitmap, global rank order
    i64 RW;
    const i64* Rs;                     // [nR] strictly ascending, 1 <= R_j <= the ranking's R
    const ApShape* shapes;             // [0] the full chunk; [1 + j] the last chunk of cut-off j, R_j mod AP_CHUNK elements (unused when 0)
    const double* recip;               // RN(1 / k), k <= R_max + AP_RECIP_SLACK, or null: divide
    double* ap;                        // [Q][nR]
    u32* rel;                          // [Q][nR]
    int nR;
};

// One leaf [ls, ls + ll) of the chunk at rank cb by the eight lanes of a group (j: the lane inside it); every lane of the wavefront
// calls this (ll = 0: no leaf), lane 0 of a group returns the leaf's sum.  ap_eval2's leaf, wpre complete for all 128 words.
__device__ __forceinline__ double aa_leaf_recip(const u64* cw, const u32* wpre, const u32 before, const i64 cb, const int ls, const int ll,
                                                const int j, const double* __restrict__ recip) {
    const u32* cw32 = (const u32*)cw;
    const int body = ll - (ll % 8);
    const int wi = ls >> 6;
    u32 P = before + wpre[wi] + (u32)__popcll(cw[wi] & ((1ull << (ls & 63)) - 1ull));      // matches before the leaf (ls is a multiple of 8)
    const u32 lmask = (2u << j) - 1u;
    const int wd = ls >> 5, bs = ls & 31;
    const double* __restrict__ rp = recip + (cb + ls + j + 1);
    double b = (double)(cb + ls + j + 1);
    double r = 0.0;
    for (int i4 = 0; __any(32 * i4 < body); ++i4) {        // 32 elements of the leaf = 4 of the lane's per step
        const u32 lo = cw32[wd + i4], hi = cw32[wd + i4 + 1];
        u32 W = __builtin_amdgcn_alignbit(hi, lo, (u32)bs);
        const int nb = body - 32 * i4;
        W = nb >= 32 ? W : nb <= 0 ? 0u : W & ((1u << nb) - 1u);
        const double ys[4] = {rp[0], rp[8], rp[16], rp[24]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 byte = (W >> (8 * k)) & 0xFFu;
            const u32 cnt = P + (u32)__builtin_popcount(byte & lmask);
            P += (u32)__builtin_popcount(byte);
            const u32 bit = (byte >> j) & 1u;
            const double a = (double)(cnt * bit);
            const double q = a * ys[k];
            r += __builtin_fma(__builtin_fma(-q, b, a), ys[k], q);
            b += 8.0;
        }
        rp += 32;
    }
    r += ap_dpp_mov<0xB1>(r);                              // lane ^ 1, lane ^ 2, the other quad of the eight: ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
    r += ap_dpp_mov<0x4E>(r);
    r += ap_dpp_mov<0x141>(r);
    // tail: element body + j of the leaf for j < ll - body, added by lane 0 in order
    const int tw = (ls + body) >> 5, tb = (ls + body) & 31;
    const u32 byte = __builtin_amdgcn_alignbit(cw32[tw + 1], cw32[tw], (u32)tb) & ((1u << (ll - body)) - 1u);
    const u32 cnt = P + (u32)__builtin_popcount(byte & lmask);
    const u32 bit = (byte >> j) & 1u;
    const double a = (double)(cnt * bit);
    const double bt = (double)(cb + ls + body + j + 1);
    const double y = recip[cb + ls + body + j + 1];
    const double q = a * y;
    const double v = __builtin_fma(__builtin_fma(-q, bt, a), y, q);      // +0.0 where there is no element
    double res = r;                                        // (ll < 8: r is 0.0)
    res += v;
    res += ap_dpp_mov<0x101>(v);                           // row_shl:1 .. 7: the values of lanes j + 1 .. j + 7
    res += ap_dpp_mov<0x102>(v);
    res += ap_dpp_mov<0x103>(v);
    res += ap_dpp_mov<0x104>(v);
    res += ap_dpp_mov<0x105>(v);
    res += ap_dpp_mov<0x106>(v);
    res += ap_dpp_mov<0x107>(v);
    return res;
}

// The same leaf with ap_eval's element values: one correctly rounded division each (no table: lists beyond 2^20, option ap_recip = 0).
__device__ __forceinline__ double aa_leaf_div(const u64* cw, const u32* wpre, const u32 before, const i64 cb, const int ls, const int ll,
                                              const int j) {
    auto val = [&](const int e) -> double {
        const u64 word = cw[e >> 6];
        const int bpos = e & 63;
        if (!((word >> bpos) & 1ull)) return 0.0;
        const u32 cnt = before + wpre[e >> 6] + (u32)__popcll(word & ((2ull << bpos) - 1ull));
        return (double)cnt / (double)(cb + e + 1);
    };
    const int body = ll - (ll % 8);
    double r = 0.0;
    if (ll >= 8)
        for (int e = ls + j; e < ls + body; e += 8) r += val(e);
    r += __shfl_xor(r, 1);
    r += __shfl_xor(r, 2);
    r += __shfl_xor(r, 4);
    double res = ll >= 8 ? r : 0.0;
    if (j == 0)
        for (int e = ls + (ll >= 8 ? body : 0); e < ls + ll; ++e) res += val(e);
    return res;
}

template <int NT>
static __global__ __launch_bounds__(NT) void k_ap_at(const ApAtArgs a) {
    static_assert(NT >= AP_CHUNK / 64 && NT % 64 == 0 && NT <= 512, "one thread per word of a chunk, at most eight wavefronts");
    constexpr int NWV = NT / 64;
    constexpr int CWORDS = AP_CHUNK / 64;
    __shared__ __attribute__((aligned(8))) u64 cw[CWORDS + 2];         // (+2: a leaf's masked window may read one dword past the chunk)
    __shared__ __attribute__((aligned(8))) double tree[NWV][2 * AP_LEAF];   // per task of a batch: leaf sums, then the internal nodes
    __shared__ i64 sRs[AA_MAX_R];
    __shared__ u32 wpre[CWORDS + 1];                                   // matches in the chunk's words before word w
    __shared__ double s_full;                                          // the full tree's sum of this chunk
    __shared__ u32 s_w0;
    const int tid = (int)threadIdx.x, lane = tid & 63, j8 = tid & 7;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = (int)blockIdx.x, nR = a.nR;
    const u64* __restrict__ row = a.mbits + (i64)q * a.RW;
    double* __restrict__ ap_q = a.ap + (i64)q * nR;
    u32* __restrict__ rel_q = a.rel + (i64)q * nR;
    if (tid < nR) sRs[tid] = a.Rs[tid];
    if (tid < 2) cw[CWORDS + tid] = 0ull;
    __syncthreads();

    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    u32 before = 0;                    // matches before the chunk                     (the same in every thread)
    double total = 0.0;                // sum of the full chunks before this one       (the same in every thread)
    int jlo = 0;                       // first cut-off that ends in this chunk or later
    for (i64 c = 0; jlo < nR; ++c) {
        const i64 cb = c * AP_CHUNK;
        // 1: the chunk's words and their popcount prefix (two wavefronts, 64 words each)
        if (tid < CWORDS) {
            const i64 w = (cb >> 6) + tid;
            const u64 word = (w < a.RW) ? row[w] : 0ull;
            cw[tid] = word;
            u32 incl = (u32)__popcll(word);
            incl += (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false);
            incl += (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false);
            incl += (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false);
            incl += (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false);
            incl += (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, false);
            incl += (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xC, 0xF, false);
            if (tid == 63) s_w0 = incl;
            wpre[tid + 1] = incl;
            if (tid == 0) wpre[0] = 0u;
        }
        __syncthreads();
        if (tid >= 64 && tid < CWORDS) wpre[tid + 1] += s_w0;
        __syncthreads();
        const u32 chunk_cnt = wpre[CWORDS];

        // the chunk's tasks: [0] the full tree if a cut-off ends at the chunk's end or beyond it, then the cut-offs jlo .. jp - 1 inside it
        int jhi = jlo;
        while (jhi < nR && sRs[jhi] <= cb + AP_CHUNK) ++jhi;
        const bool ends_full = jhi > jlo && sRs[jhi - 1] == cb + AP_CHUNK;
        const int full = (jhi < nR || ends_full) ? 1 : 0;
        const int jp = jhi - (ends_full ? 1 : 0);
        const int ntask = full + (jp - jlo);
        auto shape_of = [&](const int t) -> const ApShape* { return (full && t == 0) ? a.shapes : a.shapes + 1 + (jlo + t - full); };
        double total_next = total;
        for (int t0 = 0; t0 < ntask; t0 += NWV) {
            const int nb = ntask - t0 < NWV ? ntask - t0 : NWV;
            // the tree tables of this wavefront's task, requested before anything waits
            const ApShape* __restrict__ shw = shape_of(t0 + (wave < nb ? wave : 0));
            const int nn = shw->n_nodes, nlv = shw->n_leaves, max_h = shw->max_h;
            int tl[2] = {0, 0}, tr[2] = {0, 0}, th[2] = {0, 0};
            if (wave < nb) {
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (lane + 64 * k < nn) { tl[k] = shw->nl[lane + 64 * k]; tr[k] = shw->nr[lane + 64 * k]; th[k] = shw->nh[lane + 64 * k]; }
            }
            // 2a: the batch's leaves, eight per wavefront step, steps dealt over all wavefronts
            int first[NWV + 1];
            first[0] = 0;
#pragma unroll
            for (int k = 0; k < NWV; ++k) first[k + 1] = first[k] + (k < nb ? (shape_of(t0 + k)->n_leaves + 7) / 8 : 0);
            for (int it = wave; it < first[NWV]; it += NWV) {
                int kt = 0;
#pragma unroll
                for (int k = 1; k < NWV; ++k) kt = it >= first[k] ? k : kt;       // (empty slots k >= nb repeat first[nb]: it < first[nb] stops before them)
                if (kt >= nb) kt = nb - 1;
                int base = 0;
#pragma unroll
                for (int k = 0; k < NWV; ++k) base = k == kt ? first[k] : base;
                const ApShape* __restrict__ sh = shape_of(t0 + kt);
                const int leaf = (it - base) * 8 + (lane >> 3);
                const bool act = leaf < sh->n_leaves;
                const int ls = act ? sh->leaf_start[leaf] : 0, ll = act ? sh->leaf_len[leaf] : 0;
                const double res = a.recip ? aa_leaf_recip(cw, wpre, before, cb, ls, ll, j8, a.recip) : aa_leaf_div(cw, wpre, before, cb, ls, ll, j8);
                if (act && j8 == 0) tree[kt][leaf] = res;
            }
            __syncthreads();
            // 2b: wavefront w walks the tree of task t0 + w; every addition is left + right as in NumPy's recursion
            if (wave < nb) {
                double* tw = tree[wave];
                for (int hgt = 1; hgt <= max_h; ++hgt) {
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        if (lane + 64 * k < nn && th[k] == hgt) tw[nlv + lane + 64 * k] = tw[tl[k]] + tw[tr[k]];
                    wave_lds_sync();
                }
                if (lane == 0) {
                    const double chunk_sum = tw[nlv + nn - 1];         // the root is the last node (or the only leaf)
                    const int t = t0 + wave;
                    if (full && t == 0) {
                        s_full = chunk_sum;
                    } else {
                        const int j = jlo + t - full;
                        const int n = (int)(sRs[j] - cb);              // 1 .. AP_CHUNK - 1
                        const u32 r = before + wpre[n >> 6] + ((n & 63) ? (u32)__popcll(cw[n >> 6] & ((1ull << (n & 63)) - 1ull)) : 0u);
                        const double tot = (c == 0) ? chunk_sum : total + chunk_sum;
                        rel_q[j] = r;
                        ap_q[j] = r ? tot / (double)r : nan;
                    }
                }
            }
            __syncthreads();
            if (full && t0 == 0) {                                     // 3: what every later cut-off starts from
                total_next = (c == 0) ? s_full : total + s_full;
                if (ends_full && tid == 0) {
                    const u32 r = before + chunk_cnt;
                    rel_q[jhi - 1] = r;
                    ap_q[jhi - 1] = r ? total_next / (double)r : nan;
                }
            }
        }
        total = total_next;
        before += chunk_cnt;
        jlo = jhi;
    }
}

}  // namespace hg

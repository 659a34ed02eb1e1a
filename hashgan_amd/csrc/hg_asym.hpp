// hashgan_amd -- the asymmetric ranking's kernels (hg_topr_asym / hg_map_asym; DESIGN.md section 8, "Asymmetric ranking").
//
// Real-valued queries against a database stored as packed codes: s(q, n) = the float32 fma chain of hg_map_real over k ascending with
// x_nk = +1.0f where bit k of row n's code is set, else -1.0f.  The database's 32-bit code words ARE its rows; the kernels here give the
// real-valued pipeline (hg_real.hip) its two hot stages from them -- and, for the paths that are not worth a second form, plain float rows:
//
//   k_asym_image16      the filter's 16-bit A-fragment image (k_expand_dbf_bf16's layout) straight from the codes: +-1 is exact in IEEE
//                       half and in bfloat16 alike, and every row's norm^2 is exactly b, so nothing is measured and nothing downloaded
//   k_asym_rescore      k_real_rescore's job from the codes: a kept row is NW code words and a label word (8 + 8 bytes at 64 bits) instead
//                       of a 4 * bpad-byte float row gathered through LDS
//   k_asym_expand_rows  f32 [rows][KP] of +-1.0 (pad features 0) for the kernels that read float rows (no cut, vector fallbacks, real_mfma < 2)
#pragma once
#include "hg_kernels.hpp"
#include "hg_real_kernels.hpp"

namespace hg {

// Chunk (group G, MFMA m, k-half hh, row r) = 16 bytes at (((G * (KP/16) + m) * 2 + hh) * 16 + r) * 16 holding the 16-bit features
// 16 m + 8 hh .. + 7 of row 16 G + r: one thread per chunk, its eight features one byte of a code word.  Pad rows (>= N) and pad
// features (>= b) are zero.  (rstride > 1: image row i is table row i * rstride -- the sample passes' images.)
template <bool HALF>
static __global__ __launch_bounds__(256) void k_asym_image16(const u32* __restrict__ db, uint4* __restrict__ img, const i64 N, const i64 n16, const int KP,
                                                             const int NW, const int b, const i64 rstride) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const int per_row = KP / 8;
    if (i >= n16 * per_row) return;
    const i64 row = i / per_row;
    const int c = (int)(i - row * per_row), m = c >> 1, hh = c & 1;
    const int k0 = 16 * m + 8 * hh;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row < N && k0 < b) {
        const int w = k0 >> 5;
        const u32 bits = w < NW ? db[row * rstride * NW + w] >> (k0 & 31) : 0u;
        constexpr u32 ONE = HALF ? 0x3C00u : 0x3F80u;        // +1.0 in IEEE half / bfloat16; -1.0 sets bit 15
        u32 h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = k0 + j < b ? (ONE | ((bits >> j) & 1u ? 0u : 0x8000u)) : 0u;
        v.x = h[0] | (h[1] << 16); v.y = h[2] | (h[3] << 16);
        v.z = h[4] | (h[5] << 16); v.w = h[6] | (h[7] << 16);
    }
    img[(((row >> 4) * (KP / 16) + m) * 2 + hh) * 16 + (row & 15)] = v;
}

// out[i][k] = bit k of code row i * rstride ? +1.0f : -1.0f for k < b, 0.0f for b <= k < KP; rows i < rows.  One thread per four features.
static __global__ __launch_bounds__(256) void k_asym_expand_rows(const u32* __restrict__ db, float4* __restrict__ out, const i64 rows, const int KP,
                                                                 const int NW, const int b, const i64 rstride) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const int per_row = KP / 4;
    if (i >= rows * per_row) return;
    const i64 row = i / per_row;
    const int k0 = 4 * (int)(i - row * per_row);
    const int w = k0 >> 5;
    const u32 bits = k0 < b && w < NW ? db[row * rstride * NW + w] >> (k0 & 31) : 0u;
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = k0 + j < b ? ((bits >> j) & 1u ? 1.0f : -1.0f) : 0.0f;
    out[i] = float4{e[0], e[1], e[2], e[3]};
}

// One step of the chain per feature, k ascending: fmaf(q_k, +-1.0f, acc) -- the very operation k_real_rescore applies to a float row of +-1.0.
// The query's features sit in the lanes of qv (feature L0 + j of this 64-feature piece in lane L0 + j): a step's q_k is a v_readlane.
// (The features are the same for every row and round, and a compiler that sees it reads all of them into scalar registers ahead of the
// chain, or of the loop: more than a wavefront has next to the kernel's pointers.  The empty statement ties the register to the
// accumulator every 16 steps: the lane reads of a piece cannot start before the piece in front of it is done, so 16 are live at most.)
template <int L0> __device__ __forceinline__ float asym_word(u32 qv, const u32 bits, float acc) {      // a whole word: 32 features
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        asm volatile("" : "+v"(qv), "+v"(acc));
#pragma unroll
        for (int j = 16 * h; j < 16 * h + 16; ++j)
            acc = __builtin_fmaf(__uint_as_float((u32)__builtin_amdgcn_readlane((int)qv, L0 + j)), (bits >> j) & 1u ? 1.0f : -1.0f, acc);
    }
    return acc;
}
template <int L0> __device__ __forceinline__ float asym_tail(u32 qv, const u32 bits, const int n, float acc) {      // the last word's n < 32 features
    asm volatile("" : "+v"(qv), "+v"(acc));
    for (int j = 0; j < n; ++j)
        acc = __builtin_fmaf(__uint_as_float((u32)__builtin_amdgcn_readlane((int)qv, L0 + j)), (bits >> j) & 1u ? 1.0f : -1.0f, acc);
    return acc;
}

// Rescore from codes: wavefront = (group of SG consecutive slices, query); lane = one kept row -- k_real_rescore's mapping, its
// records {~mono(s) | match << 31 | idx} compacted to the front of their slices, its counts (sl_cnt_out [S][Qpad], cnt_by_query [Q][S]),
// its prefetch of the next round's row numbers.  A lane loads its row's NW code words (NWT = 1: one dword, 2: one 8-byte load, 0: NW
// taken at run time, a loop) and its first label word; the query's features are wave-uniform: loaded once, 64 to a vector register, a
// feature per lane, and read back lane by lane as the scalar operand of each step.  No LDS: what bounds the resident wavefronts is
// registers alone.
template <int NWT, int SG>
__global__ __launch_bounds__(256) void k_asym_rescore(const float* __restrict__ qf, const u32* __restrict__ db, const u32* sl_cnt,
                                                      const u32* __restrict__ krows, u64* __restrict__ cand, u32 cap, i64 crow, const float* __restrict__ thr,
                                                      u32* sl_cnt_out, u32* __restrict__ cnt_by_query, const u64* __restrict__ dblab, const u64* __restrict__ qlab,
                                                      const int embed_match, const int KP, const int nw_rt, const int b, const Geo g) {      // (sl_cnt_out may be sl_cnt)
    const int NW = NWT ? NWT : nw_rt;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const i64 unit = (i64)blockIdx.x * WPB + wave;
    const int nG = (g.S + SG - 1) / SG;
    if (unit >= (i64)nG * g.Q) return;
    const int sg = __builtin_amdgcn_readfirstlane((int)(unit / g.Q));
    const int q = __builtin_amdgcn_readfirstlane((int)(unit - (i64)sg * g.Q));
    const int s0 = sg * SG;
    // The slices' counters live in LANES, not in scalar registers (2 SG + 1 of them, live across the whole loop next to a dozen pointers
    // and whatever the chain reads ahead: k_real_rescore's scalar registers spill at SG >= 3): lane x < SG of `prev` holds pre[x], the
    // records in front of slice s0 + x in the group's concatenated slices; lane x of `keptv` the records of slice s0 + x that score above
    // the cut, so far.  A scalar use is a v_readlane, and the loops over the slices stay rolled so that only one is live at a time.
    const u32 mycnt = lane < SG && s0 + lane < g.S ? sl_cnt[(i64)(s0 + lane) * g.Qpad + q] : 0u;
    u32 prev = 0, total = 0;
#pragma unroll
    for (int x = 0; x < SG; ++x) {
        prev = lane == x ? total : prev;
        total += (u32)__builtin_amdgcn_readlane((int)mycnt, x);
    }
    // (up to 64 bits one register, 64 features; beyond, a register per code word, its 32 features in lanes 0 .. 31)
    constexpr int NQV = NWT ? 1 : 8, QPER = NWT ? 64 : 32;
    u32 qv[NQV];
#pragma unroll
    for (int t = 0; t < NQV; ++t) qv[t] = lane < QPER && QPER * t + lane < KP ? __float_as_uint(qf[(i64)q * KP + QPER * t + lane]) : 0u;
    const float cutq = thr[q];
    u64* __restrict__ rows = cand + (i64)q * crow + (i64)s0 * cap;                  // the records it leaves, slice by slice
    const u32* __restrict__ kept_rows = krows + (i64)q * crow + (i64)s0 * cap;      // the row numbers the filter kept, the same slices
    u32 keptv = 0;
    const u64 below = (1ull << lane) - 1ull;
    const int full = b >> 5, rest = b & 31;                  // whole code words of features, and the last word's
    // record i of the group's concatenated slices -> (slice k, offset): the last slice whose first record is at or before i (pre ascends)
    auto locate = [&](const u32 pv, const u32 i, int& k, u32& off) {
        k = 0;
        off = i;
#pragma unroll 1
        for (int x = 1; x < SG; ++x) {
            const u32 p = (u32)__builtin_amdgcn_readlane((int)pv, x);
            if (i >= p) { k = x; off = i - p; }
        }
    };
    u32 idx_next = g.idx_base;
    {
        int k0; u32 off0;
        locate(prev, (u32)lane, k0, off0);
        if ((u32)lane < total) idx_next = kept_rows[(i64)k0 * cap + off0];
    }
    for (u32 base = 0; base < total; base += 64) {
        const u32 i = base + lane;
        const bool valid = i < total;
        // (everything the rounds share is the same in every round, and a compiler that sees it keeps it all in scalar registers across the
        // loop: made opaque per round, the lane reads and the query's loads stay inside it)
        u32 pv = prev;
        asm volatile("" : "+v"(pv));
        int k; u32 off;
        locate(pv, i, k, off);
        const u32 idx = idx_next;                                               // (idle lanes: the first row, a valid one)
        idx_next = g.idx_base;
        if (i + 64 < total) {
            int kn; u32 offn;
            locate(pv, i + 64, kn, offn);
            idx_next = kept_rows[(i64)kn * cap + offn];
        }
        const u32 local = idx - g.idx_base;
        const u64 lab0 = dblab[(i64)local * g.LW];
        float acc = 0.0f;
        if constexpr (NWT == 1) {
            const u32 w0 = db[local];
            acc = full ? asym_word<0>(qv[0], w0, acc) : asym_tail<0>(qv[0], w0, rest, acc);
        } else if constexpr (NWT == 2) {
            const uint2 w = *(const uint2*)(db + (i64)local * 2);             // (rows of two words are 8-byte aligned)
            acc = asym_word<0>(qv[0], w.x, acc);
            acc = full == 2 ? asym_word<32>(qv[0], w.y, acc) : asym_tail<32>(qv[0], w.y, rest, acc);
        } else {
            const u32* __restrict__ code = db + (i64)local * NW;
#pragma unroll 1
            for (int w = 0; w <= full; ++w) {                // (everything about w is wave-uniform)
                const int n = w < full ? 32 : rest;
                if (!n) break;
                u32 qs = qv[0];
#pragma unroll
                for (int t = 1; t < NQV; ++t) qs = w == t ? qv[t] : qs;
                const u32 bits = code[w];
                acc = n == 32 ? asym_word<0>(qs, bits, acc) : asym_tail<0>(qs, bits, n, acc);
            }
        }
        // Only rows that score above the cut stay (the filter's margin let others through): they move to the front of
        // their slice, in index order -- every read of this round is done, and a record never moves to the right.
        const float ipv = acc + 0.0f;
        const bool pass = valid && !(ipv <= cutq);
        const u64 bal = __ballot(pass);
        u64 mine = 0;
        u32 before = 0;
#pragma unroll 1
        for (int x = 0; x < SG; ++x) {
            const u64 m = __ballot(valid && k == x);
            const u32 kx = (u32)__builtin_amdgcn_readlane((int)keptv, x);
            if (k == x) { mine = m; before = kx; }
            keptv += lane == x ? (u32)__popcll(bal & m) : 0u;
        }
        if (pass) {
            u64 any = lab0 & qlab[(i64)q * g.LW];
            for (int w = 1; w < g.LW; ++w) any |= dblab[(i64)local * g.LW + w] & qlab[(i64)q * g.LW + w];
            // (embed_match = 0: the records go to kernels that order by the whole 64 bits -- every row a record, > 128 features)
            rows[(i64)k * cap + before + (u32)__popcll(bal & mine & below)] = ((u64)(~mono_key(ipv)) << 32) | (u64)(idx | (any && embed_match ? 0x80000000u : 0u));
        }
    }
    if (lane < SG && s0 + lane < g.S) {
        sl_cnt_out[(i64)(s0 + lane) * g.Qpad + q] = keptv;
        cnt_by_query[(i64)q * g.S + s0 + lane] = keptv;
    }
}

}  // namespace hg

// hashgan_amd -- the quantised ranking's kernels (hg_topr_pq / hg_map_pq; DESIGN.md section 8, "Quantised databases").
//
// Real-valued queries against a database stored as product-quantisation codes: M disjoint subspaces of dsub features, K <= 256 codewords
// each.  A row decodes by pure gather, x[n][k] = books[k / dsub][codes[n][k / dsub]][k % dsub], so s(q, n) is hg_map_real's float32 fma
// chain over k ascending on the decoded row, bit for bit (AQD, the asymmetric quantiser distance).  The kernels here give the real-valued
// pipeline (hg_real.hip) its two hot stages from codes u8 [N][MP] (MP = M rounded up to 4, pad bytes 0) and codebooks f32 [M][K][dsub]:
//
//   k_pq_image16      the filter's 16-bit A-fragment image (k_expand_dbf_bf16's layout and conversion) with every feature looked up
//   k_pq_rescore      k_asym_rescore's job with the operand looked up in the codebooks, read through the vector cache
//   k_pq_expand_rows  f32 [rows][KP] decoded rows (pad features 0) for the kernels that read float rows (no cut, vector fallbacks,
//                     real_mfma < 2, the staged sample beyond 128 features)
#pragma once
#include "hg_kernels.hpp"
#include "hg_real_kernels.hpp"
#include "hg_real_bf.hpp"

namespace hg {

struct PqTab {
    const u8* codes;        // [N][MP]
    const float* books;     // [M][K][dsub]
    int M, K, dsub, MP;
};

__device__ __forceinline__ float pq_feature(const PqTab& t, const i64 trow, const int k) {
    const int m = k / t.dsub, j = k - m * t.dsub;
    const u32 code = t.codes[trow * t.MP + m];
    return t.books[((i64)m * t.K + code) * t.dsub + j];
}

// Chunk (group G, MFMA m, k-half hh, row r) = 16 bytes at (((G * (KP/16) + m) * 2 + hh) * 16 + r) * 16 holding the 16-bit features
// 16 m + 8 hh .. + 7 of row 16 G + r: one thread per chunk, each feature a codebook float through k_expand_dbf_bf16's conversion.  Pad
// rows (>= N) and pad features (>= b) are zero.  (rstride > 1: image row i is table row i * rstride -- the sample passes' images.)
template <bool HALF>
static __global__ __launch_bounds__(256) void k_pq_image16(const PqTab t, uint4* __restrict__ img, const i64 N, const i64 n16, const int KP, const int b,
                                                           const i64 rstride) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const int per_row = KP / 8;
    if (i >= n16 * per_row) return;
    const i64 row = i / per_row;
    const int c = (int)(i - row * per_row), m = c >> 1, hh = c & 1;
    const int k0 = 16 * m + 8 * hh;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row < N && k0 < b) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = k0 + j < b ? pq_feature(t, row * rstride, k0 + j) : 0.0f;
        v.x = pack_h2<HALF>(f[0], f[1]); v.y = pack_h2<HALF>(f[2], f[3]);
        v.z = pack_h2<HALF>(f[4], f[5]); v.w = pack_h2<HALF>(f[6], f[7]);
    }
    img[(((row >> 4) * (KP / 16) + m) * 2 + hh) * 16 + (row & 15)] = v;
}

// out[i][k] = feature k of table row i * rstride for k < b, 0.0f for b <= k < KP; rows i < rows.  One thread per four features.
static __global__ __launch_bounds__(256) void k_pq_expand_rows(const PqTab t, float4* __restrict__ out, const i64 rows, const int KP, const int b,
                                                               const i64 rstride) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const int per_row = KP / 4;
    if (i >= rows * per_row) return;
    const i64 row = i / per_row;
    const int k0 = 4 * (int)(i - row * per_row);
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = k0 + j < b ? pq_feature(t, row * rstride, k0 + j) : 0.0f;
    out[i] = float4{e[0], e[1], e[2], e[3]};
}

// k_pq_rescore's arguments.
struct PqRescoreArgs {
    const float* qf;
    PqTab t;
    const u32* sl_cnt;          // [S][Qpad]: the filter's counts
    const u32* krows;
    u64* cand;
    u32 cap;
    i64 crow;
    const float* thr;
    u32* sl_cnt_out;            // (may be sl_cnt)
    u32* cnt_by_query;
    const u64* dblab;
    const u64* qlab;
    int embed_match, KP;
    Geo g;
};

// Rescore from PQ codes: wavefront = (group of SG consecutive slices, query); lane = one kept row -- k_asym_rescore's mapping, records
// {~mono(s) | match << 31 | idx}, compaction, counts (sl_cnt_out [S][Qpad], cnt_by_query [Q][S]) and prefetch of the next round's row
// numbers.  A lane loads its row's code bytes a dword at a time (four subspaces ahead of the chain) and its first label word; the
// query's features are wave-uniform: 64 to a vector register, a feature per lane, read back lane by lane as the scalar operand of each
// step (hg_asym.hpp).  The other operand is the lane's codeword, read from the codebooks through the vector cache (at most 255 KB: they
// stay in the L2, the codewords in use in the L1): G = 4 features per 16-byte read when dsub is a multiple of four (a codeword then
// starts on 16 bytes), one feature per read otherwise; the next read is issued before the steps of the one in hand.
// (A form that staged codebooks of up to 64 KB in LDS -- persistent blocks of 4, 8 or 16 wavefronts -- was measured and removed: DESIGN.md
// section 8, "Quantised databases".)
template <int G, int SG>
__global__ __launch_bounds__(256) void k_pq_rescore(const PqRescoreArgs args) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 below = (1ull << lane) - 1ull;
    const float* __restrict__ qf = args.qf;
    const float* __restrict__ books = args.t.books;
    const u32* __restrict__ codes32 = (const u32*)args.t.codes;
    const int M = args.t.M, K = args.t.K, dsub = args.t.dsub, MPW = args.t.MP >> 2, KP = args.KP;      // (MPW: code dwords per row)
    const u32* sl_cnt = args.sl_cnt;
    u32* sl_cnt_out = args.sl_cnt_out;
    u32* __restrict__ cnt_by_query = args.cnt_by_query;
    const u64* __restrict__ dblab = args.dblab;
    const u64* __restrict__ qlab = args.qlab;
    const u32 cap = args.cap;
    const i64 crow = args.crow;
    const int embed_match = args.embed_match;
    const int gS = args.g.S, gQ = args.g.Q, gLW = args.g.LW;
    const i64 gQpad = args.g.Qpad;
    const u32 idx_base = args.g.idx_base;
    const int nG = (gS + SG - 1) / SG;
    auto book = [&](const u32 a, float (&x)[G]) {            // G floats at float index a of the codebooks
        if constexpr (G == 4) {
            const float4 v = *(const float4*)(books + a);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            x[0] = books[a];
        }
    };
    const i64 unit = (i64)blockIdx.x * WPB + wave;
    if (unit >= (i64)nG * gQ) return;
    const int sg = __builtin_amdgcn_readfirstlane((int)(unit / gQ));
    const int q = __builtin_amdgcn_readfirstlane((int)(unit - (i64)sg * gQ));
    const int s0 = sg * SG;
    // (the slices' counters live in lanes, as in k_asym_rescore: lane x < SG of `prev` holds the records in front of slice s0 + x in the
    // group's concatenated slices, lane x of `keptv` the records of slice s0 + x that score above the cut so far)
    const u32 mycnt = lane < SG && s0 + lane < gS ? sl_cnt[(i64)(s0 + lane) * gQpad + q] : 0u;
    u32 prev = 0, total = 0;
#pragma unroll
    for (int x = 0; x < SG; ++x) {
        prev = lane == x ? total : prev;
        total += (u32)__builtin_amdgcn_readlane((int)mycnt, x);
    }
    u32 qv[4];                                               // the query: 64 features to a register, up to 256
#pragma unroll
    for (int p = 0; p < 4; ++p) qv[p] = 64 * p + lane < KP ? __float_as_uint(qf[(i64)q * KP + 64 * p + lane]) : 0u;
    const float cutq = args.thr[q];
    u64* __restrict__ rows = args.cand + (i64)q * crow + (i64)s0 * cap;                  // the records it leaves, slice by slice
    const u32* __restrict__ kept_rows = args.krows + (i64)q * crow + (i64)s0 * cap;      // the row numbers the filter kept, the same slices
    u32 keptv = 0;
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
    u32 idx_next = idx_base;
    {
        int k0; u32 off0;
        locate(prev, (u32)lane, k0, off0);
        if ((u32)lane < total) idx_next = kept_rows[(i64)k0 * cap + off0];
    }
    for (u32 base = 0; base < total; base += 64) {
        const u32 i = base + lane;
        const bool valid = i < total;
        // (made opaque per round: what the rounds share stays inside the loop instead of in scalar registers across it)
        u32 pv = prev;
        asm volatile("" : "+v"(pv));
        int k; u32 off;
        locate(pv, i, k, off);
        const u32 idx = idx_next;                                               // (idle lanes: the first row, a valid one)
        idx_next = idx_base;
        if (i + 64 < total) {
            int kn; u32 offn;
            locate(pv, i + 64, kn, offn);
            idx_next = kept_rows[(i64)kn * cap + offn];
        }
        const u32 local = idx - idx_base;
        const u64 lab0 = dblab[(i64)local * gLW];
        const u32* __restrict__ code = codes32 + (i64)local * MPW;
        u32 wc = code[0], wn = MPW > 1 ? code[1] : 0u;       // the code dword of the subspace being addressed, and the one behind it
        u32 q0 = qv[0], q1 = qv[1], q2 = qv[2], q3 = qv[3];
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3));
        float acc = 0.0f;
        u32 a_cur = (wc & 0xFFu) * (u32)dsub;                // float index of subspace 0's codeword
        float xn[G];
        book(a_cur, xn);
        int kf = 0;                                          // the feature the chain is at (wave-uniform, like m and j)
        u32 qs = q0;
#pragma unroll 1
        for (int m = 0; m < M; ++m) {
            u32 a_next = a_cur;                              // (behind the last subspace: a valid address, read and not used)
            if (m + 1 < M) {
                const int mm = m + 1;
                if ((mm & 3) == 0) {
                    wc = wn;
                    if (mm + 4 < M) wn = code[(mm >> 2) + 1];
                }
                a_next = ((u32)mm * (u32)K + ((wc >> (8 * (mm & 3))) & 0xFFu)) * (u32)dsub;
            }
#pragma unroll 1
            for (int j = 0; j < dsub; j += G) {
                float x[G];
#pragma unroll
                for (int e = 0; e < G; ++e) x[e] = xn[e];
                book(j + G < dsub ? a_cur + (u32)(j + G) : a_next, xn);
                if ((kf & 63) == 0) { const int p = kf >> 6; qs = p == 0 ? q0 : p == 1 ? q1 : p == 2 ? q2 : q3; }
#pragma unroll
                for (int e = 0; e < G; ++e)                  // (G = 4: kf is a multiple of four, the four features lie in one register)
                    acc = __builtin_fmaf(__uint_as_float((u32)__builtin_amdgcn_readlane((int)qs, (kf + e) & 63)), x[e], acc);
                kf += G;
            }
            a_cur = a_next;
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
            const u64 mk = __ballot(valid && k == x);
            const u32 kx = (u32)__builtin_amdgcn_readlane((int)keptv, x);
            if (k == x) { mine = mk; before = kx; }
            keptv += lane == x ? (u32)__popcll(bal & mk) : 0u;
        }
        if (pass) {
            u64 any = lab0 & qlab[(i64)q * gLW];
            for (int w = 1; w < gLW; ++w) any |= dblab[(i64)local * gLW + w] & qlab[(i64)q * gLW + w];
            // (embed_match = 0: the records go to kernels that order by the whole 64 bits -- every row a record, > 128 features)
            rows[(i64)k * cap + before + (u32)__popcll(bal & mine & below)] = ((u64)(~mono_key(ipv)) << 32) | (u64)(idx | (any && embed_match ? 0x80000000u : 0u));
        }
    }
    if (lane < SG && s0 + lane < gS) {
        sl_cnt_out[(i64)(s0 + lane) * gQpad + q] = keptv;
        cnt_by_query[(i64)q * gS + s0 + lane] = keptv;
    }
}

}  // namespace hg

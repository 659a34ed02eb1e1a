// Re-rank of the Hamming tie groups by the float32 inner product (hg_topr_rerank; DESIGN.md section 3, "Re-ranked ties").
//
// Order of a query's rows: Hamming distance d ascending, inner product s descending, database index ascending -- as ONE 64-bit key
//   key = d << 56 | ~mono(s) << 24 | idx            (d <= 255, idx < 2^24; ascending keys = the order)
// with s the fixed float32 chain of hg_real_kernels.hpp (one fma chain from +0.0 in feature order, then + 0.0).  The exact histogram
// and plan (k_hist, k_plan) give the threshold t of every query, the size hown[d][q] of every group d <= t and its first rank
// posbase[d][q]; M_q = cnt_lt[q] + hown[t][q] records are kept per query, in [base[q], base[q] + M_q) of the chunk's record buffer.
//
//   k_rr_scan      hist[s][d][q] -> its exclusive prefix over the segments s, in place: where segment s starts inside group d of query q
//   k_rr_sizes     M_q
//   k_rr_collect   the pass over all pairs (lane <-> query, rows wave-uniform, as k_hist): a row with d <= t takes the next slot of its
//                  (segment, distance) range -- a counter column in LDS that only its lane touches, so no atomics and the same
//                  slots every run -- and leaves its index there
//   k_rr_score     per record the exact chain over the row's and the query's floats; the record becomes its key
//   k_rr_order     one block per query: all M_q keys sorted in LDS when they fit, else group by group -- in LDS, or, beyond it, by an
//                  LSD radix over the key's 14 nibbles between the record buffer and a second one; the first R leave as idx / dist / score
#pragma once
#include "hg_real_kernels.hpp"

namespace hg {

constexpr int RR_THREADS = 1024;                 // k_rr_order's block
constexpr int RR_LDS_KEYS = 16384;               // keys it sorts in LDS (128 KiB)
constexpr int RR_LDS_BYTES = RR_LDS_KEYS * 8 + 256;   // + the radix passes' wavefront sums
constexpr int RR_IDX_BITS = 24;                  // rows per database: 2^24
constexpr i64 RR_MAX_ROWS = 1ll << RR_IDX_BITS;

struct RerankArgs {
    const int* t;            // [Qpad] threshold distance (k_plan)
    const u32* cnt_lt;       // [Qpad] rows closer than t
    const u32* hown;         // [NB][Qpad] rows per distance
    const u32* posbase;      // [NB][Qpad] first rank of group d (d <= t)
    const u64* base;         // [Q] first record of the query inside its chunk's buffer
    u64* recs;               // the chunk's records
    u64* tmp;                // second buffer of the same size (groups beyond the LDS; else null)
    int q0, nq;              // the chunk's queries
};

static __global__ __launch_bounds__(256) void k_rr_scan(u32* __restrict__ hist, const int* __restrict__ tq, const Geo g) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 plane = (i64)g.NB * g.Qpad;
    if (i >= plane) return;
    const int d = (int)(i / g.Qpad), q = (int)(i - (i64)d * g.Qpad);
    if (q >= g.Q || d > tq[q]) return;
    u32 acc = 0;
    for (int s = 0; s < g.S; ++s) {
        const u32 v = hist[(i64)s * plane + i];
        hist[(i64)s * plane + i] = acc;
        acc += v;
    }
}

static __global__ __launch_bounds__(256) void k_rr_sizes(const int* __restrict__ tq, const u32* __restrict__ cnt_lt, const u32* __restrict__ hown,
                                                         u32* __restrict__ msz, const Geo g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.Q) return;
    const int t = tq[q];
    msz[q] = t < 0 ? 0u : cnt_lt[q] + hown[(i64)t * g.Qpad + q];
}

// g: the histogram pass's geometry with nUnits = S x (query tiles of the chunk), wpb and nBlk of this launch; qt0: the chunk's first tile
template <int NW>
__global__ __launch_bounds__(256) void k_rr_collect(const u32* __restrict__ qc, const u32* __restrict__ db, const u32* __restrict__ hist,
                                                    const RerankArgs a, const int qt0, const int nqt, const Geo g) {
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const int lb = logical_block(g.nBlk);
    if (lb < 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const i64 unit = (i64)lb * g.wpb + wave;
    if (unit >= g.nUnits) return;
    const int s = (int)(unit / nqt);
    const int qt = qt0 + (int)(unit - (i64)s * nqt);
    const int q = qt * 64 + lane;
    const bool live = q >= a.q0 && q < a.q0 + a.nq;

    u32 qw[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) qw[w] = live ? qc[(i64)q * NW + w] : 0u;
    const int t = live ? a.t[q] : -1;
    const u32 mq = t < 0 ? 0u : a.cnt_lt[q] + a.hown[(i64)t * g.Qpad + q];
    u64* __restrict__ out = a.recs + (live ? a.base[q] : 0ull);

    // the lane's column: slot of the next row of this segment at distance d, as a rank inside the query's records
    u32* h = lds + wave * g.NB * 64;
    const u32* __restrict__ hs = hist + (i64)s * g.NB * g.Qpad + q;
    for (int d = 0; d < g.NB; ++d) h[d * 64 + lane] = d <= t ? a.posbase[(i64)d * g.Qpad + q] + hs[(i64)d * g.Qpad] : 0u;

    const i64 lo = (i64)s * g.L;
    const i64 hi = lo + g.L < g.N ? lo + g.L : g.N;
    const u32* __restrict__ p = db + lo * NW;
    constexpr int B = Batch<NW>::rows;
    i64 n = lo;
    for (; n + B <= hi; n += B, p += B * NW) {
        u32 c[B * NW];
#pragma unroll
        for (int i = 0; i < B * NW; ++i) c[i] = p[i];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            u32 d = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) d += __builtin_popcount(qw[w] ^ c[j * NW + w]);
            if ((int)d <= t) {
                const u32 pos = h[d * 64 + lane];
                h[d * 64 + lane] = pos + 1u;
                if (pos < mq) out[pos] = (u64)(u32)(n + j);
            }
        }
    }
    for (; n < hi; ++n, p += NW) {
        const u32 d = hamming<NW>(qw, p);
        if ((int)d <= t) {
            const u32 pos = h[d * 64 + lane];
            h[d * 64 + lane] = pos + 1u;
            if (pos < mq) out[pos] = (u64)(u32)n;
        }
    }
}

// grid (chunk queries, blocks per query); bpad: the float tables' row pitch (a multiple of 16, zero padded)
static __global__ __launch_bounds__(256) void k_rr_score(const float* __restrict__ qf, const float* __restrict__ dbf, const int bpad,
                                                         const RerankArgs a, const Geo g) {
    __shared__ float qs[256];
    const int q = a.q0 + (int)blockIdx.x;
    for (int k = threadIdx.x; k < bpad; k += 256) qs[k] = qf[(i64)q * bpad + k];
    __syncthreads();
    const int t = a.t[q];
    if (t < 0) return;
    const u32 mq = a.cnt_lt[q] + a.hown[(i64)t * g.Qpad + q];
    u64* __restrict__ recs = a.recs + a.base[q];
    // the groups' first ranks, to tell a record's distance from its slot: walked along with the slot (slots ascend per thread)
    int d = 0;
    u32 dend = a.hown[q];                                   // end of group 0
    for (u32 i = blockIdx.y * 256 + threadIdx.x; i < mq; i += gridDim.y * 256) {
        while (i >= dend && d < t) { ++d; dend += a.hown[(i64)d * g.Qpad + q]; }
        u32 idx = (u32)recs[i];
        if ((i64)idx >= g.N) idx = 0u;                       // (cannot happen: every slot was filled; a gather must not leave the table)
        const float4* __restrict__ row = (const float4*)(dbf + (i64)idx * bpad);
        float acc = 0.0f;
        for (int k = 0; k < bpad; k += 4) {
            const float4 x = row[k >> 2];
            acc = __builtin_fmaf(qs[k + 0], x.x, acc);
            acc = __builtin_fmaf(qs[k + 1], x.y, acc);
            acc = __builtin_fmaf(qs[k + 2], x.z, acc);
            acc = __builtin_fmaf(qs[k + 3], x.w, acc);
        }
        const float ip = acc + 0.0f;
        recs[i] = ((u64)(u32)d << 56) | ((u64)(~mono_key(ip)) << RR_IDX_BITS) | (u64)idx;
    }
}

struct RerankOut {
    u32* idx;                // [Q][R]
    u8* dist;
    float* score;
    unsigned long long* counters;   // [0] groups ordered in LDS, [1] groups ordered by the radix passes
};

__device__ __forceinline__ void rr_emit(const RerankOut& o, const i64 slot, const u64 key) {
    o.idx[slot] = (u32)key & (u32)(RR_MAX_ROWS - 1);
    o.dist[slot] = (u8)(key >> 56);
    o.score[slot] = mono_inv(~(u32)(key >> RR_IDX_BITS));
}

// bitonic sort of the m (a power of two) keys in LDS, ascending
__device__ __forceinline__ void rr_bitonic(u64* __restrict__ keys, const int m) {
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < (m >> 1); p += RR_THREADS) {      // one thread per pair (i, i + j)
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i + j;
                const u64 x = keys[i], y = keys[l];
                if (((i & k) == 0) == (x > y)) { keys[i] = y; keys[l] = x; }
            }
            __syncthreads();
        }
    }
}

// n keys from src (global) sorted in LDS, the first nw emitted at rank0 of the query's list
__device__ __forceinline__ void rr_sort_lds(u64* __restrict__ keys, const u64* __restrict__ src, const u32 n, const u32 nw, const RerankOut& o,
                                            const i64 row0, const u32 rank0) {
    int m = 1;
    while ((u32)m < n) m <<= 1;
    for (int i = threadIdx.x; i < m; i += RR_THREADS) keys[i] = (u32)i < n ? src[i] : ~0ull;
    __syncthreads();
    rr_bitonic(keys, m);
    for (u32 i = threadIdx.x; i < nw; i += RR_THREADS) rr_emit(o, row0 + rank0 + i, keys[i]);
    __syncthreads();
}

// LSD radix over the 14 nibbles of key bits [0, 56): thread k owns the k-th run of `per` consecutive keys, counts its nibbles, a block-wide
// exclusive scan over (nibble, thread) places them -- stable, and the same result whatever order the keys arrived in.  Returns the buffer
// that holds the sorted keys (14 passes: the one they started in).
__device__ __forceinline__ u64* rr_sort_radix(u32* cnt, u64* bufA, u64* bufB, const u32 n) {
    u32* wsum = cnt + 16 * RR_THREADS;
    const u32 per = (n + RR_THREADS - 1) / RR_THREADS;
    const u32 lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const u32 hi = lo + per < n ? lo + per : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* src = bufA;
    u64* dst = bufB;
    for (int shift = 0; shift < 56; shift += 4) {
        u32 c[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = 0u;
        for (u32 i = lo; i < hi; ++i) {
            const int dg = (int)(src[i] >> shift) & 15;
#pragma unroll
            for (int k = 0; k < 16; ++k) c[k] += dg == k ? 1u : 0u;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) cnt[k * RR_THREADS + threadIdx.x] = c[k];
        __syncthreads();
        // exclusive scan over the 16 x 1024 counters in (nibble, thread) order: thread k takes entries [16 k, 16 k + 16)
        u32 run[16], sum = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { run[k] = sum; sum += cnt[threadIdx.x * 16 + k]; }
        u32 inc = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u32 before = inc - sum;
        for (int w = 0; w < wave; ++w) before += wsum[w];
#pragma unroll
        for (int k = 0; k < 16; ++k) cnt[threadIdx.x * 16 + k] = before + run[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = cnt[k * RR_THREADS + threadIdx.x];
        for (u32 i = lo; i < hi; ++i) {
            const u64 key = src[i];
            const int dg = (int)(key >> shift) & 15;
            u32 pos = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) { if (dg == k) { pos = c[k]; c[k] += 1u; } }
            if (pos < n) dst[pos] = key;
        }
        __threadfence_block();
        __syncthreads();
        u64* sw = src; src = dst; dst = sw;
    }
    return src;
}

static __global__ __launch_bounds__(RR_THREADS) void k_rr_order(const RerankArgs a, const RerankOut o, const Geo g) {
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    u64* keys = (u64*)lds;
    const int q = a.q0 + (int)blockIdx.x;
    const int t = a.t[q];
    if (t < 0) return;
    const u32 mq = a.cnt_lt[q] + a.hown[(i64)t * g.Qpad + q];
    const u32 R = (u32)g.R;
    u64* recs = a.recs + a.base[q];
    const i64 row0 = (i64)q * g.R;
    if (mq <= (u32)RR_LDS_KEYS) {                           // the whole query at once: the distance leads the key
        rr_sort_lds(keys, recs, mq, mq < R ? mq : R, o, row0, 0u);
        if (threadIdx.x == 0) {
            u32 groups = 0;
            for (int d = 0; d <= t; ++d) groups += a.hown[(i64)d * g.Qpad + q] ? 1u : 0u;
            atomicAdd(&o.counters[0], (unsigned long long)groups);
        }
        return;
    }
    for (int d = 0; d <= t; ++d) {
        const u32 n = a.hown[(i64)d * g.Qpad + q], off = a.posbase[(i64)d * g.Qpad + q];
        if (n == 0u || off >= R) continue;
        const u32 nw = n < R - off ? n : R - off;
        if (n <= (u32)RR_LDS_KEYS) {
            rr_sort_lds(keys, recs + off, n, nw, o, row0, off);
            if (threadIdx.x == 0) atomicAdd(&o.counters[0], 1ull);
        } else {
            const u64* sorted = rr_sort_radix(lds, recs + off, a.tmp + a.base[q] + off, n);
            for (u32 i = threadIdx.x; i < nw; i += RR_THREADS) rr_emit(o, row0 + off + i, sorted[i]);
            if (threadIdx.x == 0) atomicAdd(&o.counters[1], 1ull);
            __syncthreads();
        }
    }
}

}  // namespace hg

// hashgan_amd -- label-free relevance: the ground truth of a query is a set of database rows (its true nearest neighbours in the
// original feature space), not a class label.  Three passes:
//
// k_nbr_sort     one workgroup per query: up to NB_MAX_G row numbers -- a row of the caller's table, or the first G ranks of the ranked
//                index list the last ranking left (a strided slice of out_idx) -- into LDS, a bitonic network on the next power of two,
//                the sorted row out.  0xFFFFFFFF pads a shorter set and, being the largest word, sorts to the end; the valid ids are
//                counted, and a duplicate (two equal neighbours after the sort) or an id >= n_total raises a bit of one flag word.
// k_nbr_match    the match bitmap from the sets: workgroup (query, chunk of NM_CHUNK ranks) keeps the query's sorted set in LDS, a lane
//                takes a rank, follows the ranked index list and searches the set by bisection; 64 slots make a word by __ballot exactly
//                as k_match forms its words, with k_match's guard against stale list words.  A slot past R holds no bit.
// k_nbr_hist     nbr[d][q] = the neighbours of q at Hamming distance d: one workgroup per query, lanes walk the set, gather the row's
//                code words, xor + popcount against the query's words, one ds_add_u32 into the block's column of b + 1 bins; the block
//                writes its own column of the [b + 1][Qpad] table.  A pad slot counts nothing.
//
// Everything is an integer and exact: no float anywhere, and no result depends on an order -- the sorted table is a function of the set,
// a bit of the bitmap of (set, index), a counter of the histogram of the set.
//
// The sort keeps P = 2^ceil(log2 G) words in LDS (64 KiB at the largest set) plus one row of counters: a workgroup may declare all
// 160 KiB of a CU, the launcher raises the dynamic limit past 64 KiB once per device.  A compare-exchange step at stride j touches words
// l and l + j of the lane's pair: consecutive lanes take consecutive l inside a run of j, so the strides >= 32 are free of bank
// conflicts (ds_read_b32 / ds_write_b32 bank = word % 32 within a 32-lane half) and the five strides below 32 of every merge are
// 2-way -- 15 % of the 105 steps' LDS cycles at the largest set, and the kernel runs once per ground truth, not per ranking.
#pragma once
#include "hg_kernels.hpp"

namespace hg {

constexpr int NB_MAX_G = 16384;        // ids per set: 64 KiB of LDS for the sort
constexpr int NB_SORT_THREADS = 1024;  // k_nbr_sort's block for the sets beyond NB_SORT_SMALL words; 256 below
constexpr int NB_SORT_SMALL = 2048;
constexpr int NB_SORT_EXTRA = 64;      // words behind the sort's P: [0] the valid ids
constexpr int NM_THREADS = 256;        // k_nbr_match's block: four wavefronts, four words of the bitmap per step
constexpr int NM_CHUNK = 2048;         // ... and the ranks of one block: the set is staged once per 2048 searches
constexpr int NH_THREADS = 256;        // k_nbr_hist's block
constexpr u32 NB_FLAG_DUP = 1u, NB_FLAG_RANGE = 2u;

struct NbrSortArgs {
    const u32* src;                    // row q at src + q * stride: G ids in any order, IDX_NONE pads
    i64 stride;
    u32* ids;                          // [Q][G] ascending, pads at the end
    u32* count;                        // [Q] valid ids
    u32* flag;                         // one word, zeroed: NB_FLAG_DUP | NB_FLAG_RANGE
    int G, P;                          // P: the power of two >= max(G, 64)
    i64 n_total;
};

// grid Q, 256 or 1024 threads, (P + NB_SORT_EXTRA) * 4 bytes of dynamic LDS
static __global__ __launch_bounds__(NB_SORT_THREADS) void k_nbr_sort(const NbrSortArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 nb_lds[];
    u32* s = nb_lds;
    const int q = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const u32* __restrict__ src = a.src + (i64)q * a.stride;
    for (int i = tid; i < a.P; i += T) s[i] = i < a.G ? src[i] : IDX_NONE;
    if (tid == 0) s[a.P] = 0u;
    __syncthreads();
    const int half = a.P >> 1;
    for (int k = 2; k <= a.P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < half; i += T) {
                const int l = 2 * i - (i & (j - 1));           // pair i of this step: words l and l + j
                const u32 x = s[l], y = s[l + j];
                const bool up = (l & k) == 0;
                if ((x > y) == up) { s[l] = y; s[l + j] = x; }
            }
            __syncthreads();
        }
    }
    // ascending: the valid ids first, then the pads (a.G <= a.P, and the words past G were pads from the start)
    u32 n = 0, bad = 0;
    u32* __restrict__ dst = a.ids + (i64)q * a.G;
    for (int i = tid; i < a.G; i += T) {
        const u32 v = s[i];
        dst[i] = v;
        if (v != IDX_NONE) {
            ++n;
            if ((i64)v >= a.n_total) bad |= NB_FLAG_RANGE;
            if (i + 1 < a.P && s[i + 1] == v) bad |= NB_FLAG_DUP;
        }
    }
    if (n) atomicAdd(&s[a.P], n);
    if (bad) atomicOr(a.flag, bad);
    __syncthreads();
    if (tid == 0) a.count[q] = s[a.P];
}

struct NbrMatchArgs {
    const u32* idx;                    // [Q][R] ranked row indices
    const u32* ids;                    // [Q][G] sorted sets
    const u32* count;                  // [Q]
    u64* mbits;                        // [Q][RW]
    i64 R, RW, N;
    int G, nCB;                        // nCB = ceil(R / NM_CHUNK) blocks per query
    u32 idx_base;
};

// grid Q * nCB, NM_THREADS threads, G * 4 bytes of dynamic LDS
static __global__ __launch_bounds__(NM_THREADS) void k_nbr_match(const NbrMatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 nb_lds[];
    u32* s = nb_lds;
    const int q = (int)(blockIdx.x / (u32)a.nCB);
    const i64 k0 = (i64)(blockIdx.x - (u32)q * (u32)a.nCB) * NM_CHUNK;
    const int tid = (int)threadIdx.x;
    const int n = (int)a.count[q];                         // <= G
    const u32* __restrict__ set = a.ids + (i64)q * a.G;
    for (int i = tid; i < n; i += NM_THREADS) s[i] = set[i];
    __syncthreads();
    const u32* __restrict__ idx = a.idx + (i64)q * a.R;
    const i64 k1 = k0 + NM_CHUNK;                          // (whole words: every wavefront of the block runs the same steps)
    for (i64 k = k0 + tid; k < k1; k += NM_THREADS) {
        bool m = false;
        if (k < a.R) {
            const u32 gi = idx[k];
            // (k_match's guard: a stale word of the list is never taken for a row)
            if (gi != IDX_NONE && (i64)(gi - a.idx_base) < a.N) {
                int lo = 0, hi = n;                        // the first word >= gi
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s[mid] < gi) lo = mid + 1; else hi = mid;
                }
                m = lo < n && s[lo] == gi;
            }
        }
        const u64 word = __ballot(m);
        if ((tid & 63) == 0 && (k >> 6) < a.RW) a.mbits[(i64)q * a.RW + (k >> 6)] = word;
    }
}

struct NbrHistArgs {
    const u32* qc;                     // [Q][NW] query codes
    const u32* db;                     // [N][NW] database codes
    const u32* ids;                    // [Q][G]
    u32* nbr;                          // [NB][Qpad]
    i64 N, Qpad;
    int G, NW, NB;
};

// grid Q, NH_THREADS threads
static __global__ __launch_bounds__(NH_THREADS) void k_nbr_hist(const NbrHistArgs a) {
    __shared__ u32 h[256];             // NB = b + 1 <= 256 bins
    const int q = (int)blockIdx.x;
    const int tid = (int)threadIdx.x;
    h[tid] = 0u;
    u32 qw[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) qw[w] = w < a.NW ? a.qc[(i64)q * a.NW + w] : 0u;
    __syncthreads();
    const u32* __restrict__ set = a.ids + (i64)q * a.G;
    for (int i = tid; i < a.G; i += NH_THREADS) {
        const u32 id = set[i];
        if (id == IDX_NONE || (i64)id >= a.N) continue;    // a pad slot counts nothing
        const u32* __restrict__ row = a.db + (i64)id * a.NW;
        u32 d = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w)
            if (w < a.NW) d += (u32)__builtin_popcount(qw[w] ^ row[w]);
        if (d < (u32)a.NB) atomicAdd(&h[d], 1u);
    }
    __syncthreads();
    if (tid < a.NB) a.nbr[(i64)tid * a.Qpad + q] = h[tid];
}

}  // namespace hg

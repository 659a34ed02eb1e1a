// hashgan_amd -- class votes along the ranked lists: which classes did a query retrieve?  Two passes:
//
// k_votes            along the ranked lists the last ranking left on the device (out_idx), one workgroup per query: per cut-off k of
//                    an ascending list ks and class c, votes[q][j][c] = the ranks i < ks[j] whose row carries label c; from them
//                    top[q][j] = the largest count and pred[q][j] = the smallest class that reaches it (-1 when every count is 0):
//                    the k-nearest-neighbour prediction by majority vote.
// k_vote_confusion   conf[j][a][b] = sum over the queries that carry label a of votes[q][j][b]: the retrieval confusion matrix.
//
// Everything is an integer and exact: no float anywhere, and no result depends on an order.
//
// k_votes walks the list as k_graded does (hg_graded.hpp): chunks of 256 ranks that never straddle a cut-off, a lane per rank, the
// lanes past the chunk's end holding zero words.  A rank gathers its row's LW label words and adds one to counters[class] in LDS for
// every set bit -- one ds_add_u32 without return per label, counters shared by the block.  The counters are running totals, so a
// cut-off costs two barriers, one coalesced store of C counters and one max-reduce of (count, 255 - class) keys, and the chunks between
// two cut-offs need no barrier at all.  The walk is two chunks deep: while chunk n is counted, the label words of chunk n + 1 and the
// indices of chunk n + 2 are in flight -- a block walks its list alone, and at four blocks per CU (the CIFAR evaluation: 1000 queries)
// nothing else hides a chunk's two dependent loads.
// The form without LDS atomics was built and measured against this one (tools/votes_timing.py, profiles/votes_timing.txt; BALLOT = true,
// measurement build only, option "probe_votes"): per wavefront and label word the 64 lanes' words are ORed by a butterfly of shuffles,
// and for each set bit c of the OR lane c of an accumulator register adds popcount(ballot(bit c of the lane's word)), so 64 rows of one
// class cost one ballot instead of 64 adds on one address.  It is the slower one wherever the label gather does not bound the pass
// (C3 and the CIFAR evaluation; equal at C2): the twelve dependent cross-lane steps of the OR and the ballot -> popcount -> add chain per
// class are latency a wavefront with three neighbours on its SIMD cannot hide, while the adds leave the lane at once.  With every row
// of a chunk in one class -- 64 adds on one address, the adds' worst case -- the ballots win at the CIFAR evaluation, but that worst
// case is still faster than the ballots are on ordinary labels there.
// On a shard's partial lists the same walk writes the shard's vote table for the exchange (OWN = true, below; hg_list_merge.hpp).
// An index >= N (IDX_NONE included) votes for nothing and is never followed; bits past class C - 1 of the last label word are masked
// off before anything is counted, so they never index a counter.
//
// k_vote_confusion: block (a, j, s) walks the queries of segment s; a wavefront takes every fourth query of it, reads the query's
// label word with bit a through a scalar load (wave-uniform), and where the bit is set its lanes add the row votes[q][j][.] -- lane l
// the classes l, l + 64, ... -- into int64 registers, eight queries in flight.  The four wavefronts' sums meet in LDS and one integer
// atomic per (segment, a, b) with a non-zero sum goes to conf, which the host has zeroed: integer adds commute, the result is exact.
#pragma once
#include "hg_kernels.hpp"

namespace hg {

constexpr int VT_THREADS = 256;        // k_votes' block: four wavefronts, one chunk of the list per step
constexpr int VT_MAX_K = 64;           // cut-offs per pass
constexpr int VT_MAX_C = 255;          // classes (the limit of the other label-count metrics)
constexpr int VT_WORDS = 4;            // label words of VT_MAX_C classes
constexpr int VC_SEG = 512;            // k_vote_confusion: queries per block
constexpr int VC_BATCH = 8;            // ... and a wavefront's queries in flight

struct VotesArgs {
    const u32* idx;                    // [Q][R] ranked row indices (IDX_NONE / anything outside the table: no vote, never followed)
    const u64* dblab;                  // label words, LW per row
    const i64* ks;                     // [nk] ascending cut-offs, 1 <= k <= R
    u32* votes;                        // [Q][nk][C]
    int* pred;                         // [Q][nk]
    u32* top;                          // [Q][nk]
    i64 R, N;
    int nk, LW, C;
    u64 lastmask;                      // the classes of the last label word
    u32 idx_base; i64 Qpad;            // OWN: the first row of this shard's table; the pitch of the vote table's planes
};

__device__ __forceinline__ u64 wave_or_u64(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Ranks [pos, end) of the list, counted towards cut-off j: at most VT_THREADS of them, ending at ks[j] at the latest.  j = nk: past the
// last cut-off (no ranks).
struct VtChunk { i64 pos, end; int j; };
// (ks: the cut-offs in LDS -- the kernel stores to global memory, so a global read of them inside the loop is a vector load, and waiting
// for it waits for the chunks in flight too)
__device__ __forceinline__ VtChunk vt_chunk(const i64* ks, const int nk, const i64 pos, const int j) {
    VtChunk c{pos, pos, j};
    if (j < nk) {
        const i64 kj = ks[j];
        c.end = pos + VT_THREADS < kj ? pos + VT_THREADS : kj;
    }
    return c;
}
__device__ __forceinline__ VtChunk vt_next(const i64* ks, const int nk, const VtChunk& c) {
    if (c.j >= nk) return c;
    return vt_chunk(ks, nk, c.end, c.end == ks[c.j] ? c.j + 1 : c.j);
}

// BALLOT: the form without LDS atomics (above; measurement build only) -- sacc holds a row of counters per wavefront instead of row 0 for
// the block, written from the accumulator registers at a cut-off.
// OWN: the pass on a shard's lists for the exchange (hg_list_merge.hpp) -- idx holds global row indices in global rank positions and
// IDX_NONE where a slot is another shard's; a rank counts when idx - idx_base is a row of this table, the slots that count are counted
// themselves in counter C (one ballot per wavefront and chunk), and the C + 1 counters of a cut-off go to the vote table's planes
// votes[j][c][q] (pitch Qpad) instead of votes[q][j][c].  No prediction: that is the merged counts' (k_vote_pick).
template <bool BALLOT, bool OWN = false>
__global__ __launch_bounds__(VT_THREADS) void k_votes(const VotesArgs a) {
    static_assert(!(BALLOT && OWN), "the measurement form counts whole lists only");
    __shared__ u32 sacc[VT_THREADS / 64][VT_WORDS * 64];
    __shared__ u64 skey[VT_THREADS / 64];
    __shared__ i64 ks[VT_MAX_K];
    const int q = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32* __restrict__ idx = a.idx + (i64)q * a.R;
    if (tid < a.nk) ks[tid] = a.ks[tid];

    u32 acc[VT_WORDS] = {0u, 0u, 0u, 0u};                  // BALLOT: this wavefront's running totals, register w of lane l = class 64 w + l
    sacc[0][tid] = 0u;                                     // the block's counters
    __syncthreads();
    // two chunks ahead: m = the label words of the chunk being counted, mn = the next one's, gin = the indices of the one after
    const auto load_idx = [&](const VtChunk& c) -> u32 {
        const i64 i = c.pos + tid;
        return i < c.end ? idx[i] : IDX_NONE;
    };
    const auto load_words = [&](const u32 gi, u64 (&m)[VT_WORDS]) -> bool {
        const u32 li = OWN ? gi - a.idx_base : gi;
        const bool row = (i64)li < a.N && (!OWN || gi != IDX_NONE);      // (IDX_NONE -- a lane past the chunk's end too -- included: N < 2^32 - 1)
        const u64* __restrict__ dl = a.dblab + (i64)(row ? li : 0u) * a.LW;
#pragma unroll
        for (int w = 0; w < VT_WORDS; ++w) m[w] = row && w < a.LW ? dl[w] : 0ull;
        return row;
    };
    VtChunk cur = vt_chunk(ks, a.nk, 0, 0), nxt = vt_next(ks, a.nk, cur);
    u64 m[VT_WORDS], mn[VT_WORDS];
    bool own = load_words(load_idx(cur), m);
    u32 gin = load_idx(nxt);
    while (cur.j < a.nk) {
        const int j = cur.j;
        const bool own_n = load_words(gin, mn);
        if constexpr (OWN) {
            const u32 n = (u32)__popcll(__ballot(own));
            if (lane == 0 && n) atomicAdd(&sacc[0][a.C], n);         // (C <= 255: counter C is no class's)
        }
        const VtChunk nn = vt_next(ks, a.nk, nxt);
        gin = load_idx(nn);
#pragma unroll
        for (int w = 0; w < VT_WORDS; ++w) {
            if (w < a.LW) {                                // (wave-uniform)
                if (w == a.LW - 1) m[w] &= a.lastmask;
                if constexpr (!BALLOT) {
                    for (u64 x = m[w]; x; x &= x - 1ull) atomicAdd(&sacc[0][w * 64 + __builtin_ctzll(x)], 1u);
                    continue;
                }
                const u64 any_v = wave_or_u64(m[w]);       // the classes these 64 rows carry: the same in every lane
                u64 any = (u64)(u32)__builtin_amdgcn_readfirstlane((u32)any_v) |            // (the builtin returns int: no sign extension)
                          (u64)(u32)__builtin_amdgcn_readfirstlane((u32)(any_v >> 32)) << 32;
                while (any) {
                    const int cbit = __builtin_ctzll(any);
                    any &= any - 1ull;
                    const u32 n = (u32)__popcll(__ballot((m[w] >> cbit) & 1ull));
                    acc[w] += lane == cbit ? n : 0u;
                }
            }
        }
        if (cur.end == ks[j]) {
            if constexpr (BALLOT) {
#pragma unroll
                for (int w = 0; w < VT_WORDS; ++w) sacc[wave][w * 64 + lane] = acc[w];
            }
            __syncthreads();
            u32 tot = 0;
            if (tid < a.C + (OWN ? 1 : 0)) {
#pragma unroll
                for (int v = 0; v < (BALLOT ? VT_THREADS / 64 : 1); ++v) tot += sacc[v][tid];
                if constexpr (OWN) a.votes[((i64)j * (a.C + 1) + tid) * a.Qpad + q] = tot;
                else a.votes[((i64)q * a.nk + j) * a.C + tid] = tot;
            }
            // the largest count, the smallest class among equals: max of (count, 255 - class)
            const u64 key = OWN ? 0ull : wave_max_u64(tid < a.C ? (u64)tot << 8 | (u64)(255 - tid) : 0ull);
            if (lane == 0) skey[wave] = key;
            __syncthreads();               // (sacc is written again only after this barrier, skey only after the next cut-off's first one)
            if (tid == 0 && !OWN) {
                u64 best = skey[0];
#pragma unroll
                for (int v = 1; v < VT_THREADS / 64; ++v) best = skey[v] > best ? skey[v] : best;
                const u32 t = (u32)(best >> 8);
                a.top[(i64)q * a.nk + j] = t;
                a.pred[(i64)q * a.nk + j] = t ? 255 - (int)(best & 255ull) : -1;
            }
        }
#pragma unroll
        for (int w = 0; w < VT_WORDS; ++w) m[w] = mn[w];
        own = own_n;
        cur = nxt; nxt = nn;
    }
}

struct ConfArgs {
    const u32* votes;                  // [Q][nk][C]
    const u64* qlab;                   // query label words, LW per query
    unsigned long long* conf;          // [nk][C][C], zeroed
    i64 Q;
    int nk, LW, C;
};

// grid (C, nk, segments of VC_SEG queries), 256 threads
static __global__ __launch_bounds__(256) void k_vote_confusion(const ConfArgs a) {
    __shared__ unsigned long long ssum[4][VT_WORDS * 64];
    const int ca = (int)blockIdx.x, j = (int)blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const i64 q0 = (i64)blockIdx.z * VC_SEG, q1 = q0 + VC_SEG < a.Q ? q0 + VC_SEG : a.Q;
    const u64* __restrict__ ql = a.qlab + (ca >> 6);
    const int sh = ca & 63;
    unsigned long long acc[VT_WORDS] = {0ull, 0ull, 0ull, 0ull};
    for (i64 qb = q0 + wave; qb < q1; qb += 4 * VC_BATCH) {
        u32 v[VC_BATCH][VT_WORDS];
#pragma unroll
        for (int t = 0; t < VC_BATCH; ++t) {
            const i64 q = qb + 4 * t;                      // wave-uniform: the label word comes through a scalar load
            const bool has = q < q1 && ((ql[q * a.LW] >> sh) & 1ull);
            const u32* __restrict__ row = a.votes + ((has ? q : q0) * a.nk + j) * a.C;
#pragma unroll
            for (int w = 0; w < VT_WORDS; ++w) v[t][w] = has && w * 64 + lane < a.C ? row[w * 64 + lane] : 0u;
        }
#pragma unroll
        for (int t = 0; t < VC_BATCH; ++t)
#pragma unroll
            for (int w = 0; w < VT_WORDS; ++w) acc[w] += v[t][w];
    }
#pragma unroll
    for (int w = 0; w < VT_WORDS; ++w) ssum[wave][w * 64 + lane] = acc[w];
    __syncthreads();
    const int cb = (int)threadIdx.x;
    if (cb < a.C) {
        const unsigned long long s = ssum[0][cb] + ssum[1][cb] + ssum[2][cb] + ssum[3][cb];
        if (s) atomicAdd(a.conf + ((i64)j * a.C + ca) * a.C + cb, s);
    }
}

}  // namespace hg

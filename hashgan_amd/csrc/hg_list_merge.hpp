// hashgan_amd -- the list-based side metrics of a database-sharded context: hg_graded's four sums and hg_votes' counts walk the ranked
// lists, and on a shard the lists are partial.  The exact staged sequence (hg_hist -> hg_plan -> hg_select with "staged_lists") leaves a
// shard's members of the global top R in their GLOBAL rank positions: out_idx[q][i] is the global row index where slot i is this
// shard's and IDX_NONE where it is another's, so every slot i < R of a query belongs to exactly one shard.  Two exchange units follow,
// each one contiguous block per shard, equal in size on every rank (the queries are replicated, R and the cut-offs are the call's):
//
//     grade plane   u8  [Q][Rp], then u32 own[Qpad]      Rp = R rounded up to 16 (rows stay 16-byte aligned), Qpad = 64 x query tiles
//                   byte i of row q = popcount(qlab & dblab) of the shard's own row in slot i, the last label word masked as in
//                   grade_of; 0 where the slot is another shard's and in the pad bytes i >= R.  own[q] = the slots i < R of query q
//                   that are this shard's (0 for the pad queries).  Q Rp + 4 Qpad bytes.
//     vote table    u32 [nk][C + 1][Qpad], q fastest like the side tables (hg_side_merge.hpp)
//                   plane (j, c), c < C: the shard's own slots i < ks[j] whose row carries class c; plane (j, C): the shard's own
//                   slots i < ks[j].  4 nk (C + 1) Qpad bytes.
//
// k_list_grades writes a shard's grade plane: one workgroup per query in k_graded's list walk (hg_graded.hpp) -- a lane per rank, the
// query's label words wave-uniform --, the row address dblab + (gi - idx_base) LW guarded by gi - idx_base < N as k_match guards it.
// Four neighbouring lanes' bytes meet in one of them through shuffles and leave as one 32-bit store; own[q] is the sum of the
// wavefronts' ballots.  The vote table is written by k_votes itself (hg_votes.hpp, OWN = true).
//
// k_list_merge_grades merges the Gsh gathered blocks ([Gsh] equal blocks back to back, what an all-gather leaves) into one plane
// [Q][Rp]: a thread reads 16 bytes of every block -- a wavefront 1 KiB of contiguous bytes per block -- and ORs them, since a slot is
// non-zero in at most one block.  Behind the plane's threads one thread per query sums the blocks' own words.  Three flags, set by
// integer atomics whose result does not depend on the order of arrival (flag[0] a bit each, flag[1 + f] the smallest query of flag f
// by atomicMin, 0xFFFFFFFF: none):
//     bit 0  owned-slots          a real query's summed own is not R (a shard's block missing, counted twice, zeroed or stale)
//     bit 1  slot-claimed-twice   a byte i < R of a real query is non-zero in two blocks
//     bit 2  grade-range          a byte i < R of a real query exceeds C -- k_graded indexes gain[g], a table of C + 1 doubles, so a
//                                 fabricated or stale block must never become a merged plane
// The pad bytes i >= R and the pad queries' own words are never checked; the merged plane's pad bytes are written as zeros.
//
// k_list_merge_votes is k_side_merge's sibling (its one column total per query does not fit: here every cut-off has its own total):
// one workgroup per 64-query tile, thread = (plane lane 0..15, four queries), a cell accumulated in 64 bits.  It writes the merged
// counts in hg_votes' own layout [Q][nk][C], which k_vote_pick and k_vote_confusion read.  Two flags, same words as above:
//     bit 0  overflow      a summed cell of a real query does not fit 32 bits
//     bit 1  owned-slots   plane (j, C) of a real query does not sum to ks[j]
// The pad columns q >= Q are read and never checked or stored.
//
// k_vote_pick: one wavefront per (query, cut-off) max-reduces the keys (count, 255 - class) exactly as k_votes does at a cut-off:
// the largest count, the smallest class among equals, -1 when every count is 0.
#pragma once
#include "hg_graded.hpp"
#include "hg_votes.hpp"
#include "hg_side_merge.hpp"

namespace hg {

constexpr int LG_THREADS = 256;        // k_list_grades: four wavefronts, 256 ranks per step
constexpr u32 LIST_NO_QUERY = 0xFFFFFFFFu;

struct ListGradesArgs {
    const u32* idx;                    // [Q][R] global row indices in global rank positions, IDX_NONE: another shard's slot
    const u64* dblab; const u64* qlab; // label words, LW per row; dblab holds the rows [idx_base, idx_base + N)
    u8* plane;                         // [Q][Rp]
    u32* own;                          // [Qpad], zeroed by the host (the pad queries stay 0)
    i64 R, Rp, N;
    u32 idx_base;
    int LW;
    u64 lastmask;                      // the classes of the last label word
};

static __global__ __launch_bounds__(LG_THREADS) void k_list_grades(const ListGradesArgs a) {
    __shared__ u32 sown[LG_THREADS / 64];
    const int q = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32* __restrict__ idx = a.idx + (i64)q * a.R;
    const u64* __restrict__ ql = a.qlab + (i64)q * a.LW;
    u8* __restrict__ row = a.plane + (i64)q * a.Rp;
    u32 mine = 0;                      // this wavefront's owned slots, the same in every lane
    for (i64 i0 = 0; i0 < a.Rp; i0 += LG_THREADS) {
        const i64 i = i0 + tid;
        const u32 gi = i < a.R ? idx[i] : IDX_NONE;
        const u32 li = gi - a.idx_base;
        const bool has = gi != IDX_NONE && (i64)li < a.N;
        u32 g = 0;
        if (has) {
            const u64* __restrict__ dl = a.dblab + (i64)li * a.LW;
            for (int w = 0; w < a.LW; ++w) {
                u64 m = ql[w];         // wave-uniform: scalar loads
                if (w == a.LW - 1) m &= a.lastmask;
                g += (u32)__popcll(dl[w] & m);
            }
        }
        mine += (u32)__popcll(__ballot(has));
        // bytes of the lanes 4n .. 4n + 3 into lane 4n (a lane past the wavefront's end is never used: 64 is a multiple of 4)
        const u32 packed = g | (u32)__shfl_down(g, 1, 64) << 8 | (u32)__shfl_down(g, 2, 64) << 16 | (u32)__shfl_down(g, 3, 64) << 24;
        if ((lane & 3) == 0 && i < a.Rp) *reinterpret_cast<u32*>(row + i) = packed;      // (Rp is a multiple of 16: i + 3 < Rp)
    }
    if (lane == 0) sown[wave] = mine;
    __syncthreads();
    if (tid == 0) a.own[q] = sown[0] + sown[1] + sown[2] + sown[3];
}

// 0x80 in every byte of x that is not zero
__device__ __forceinline__ u32 nonzero_bytes(const u32 x) { return (x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u; }

struct ListMergeGradesArgs {
    const u8* blocks;                  // [Gsh] blocks of Q Rp + 4 Qpad bytes
    u8* dst;                           // [Q][Rp]
    u32* flag;                         // [4], see above ({0, none, none, none} before the launch)
    i64 Q, Qpad, R, Rp;
    int Gsh, C;
};

__device__ __forceinline__ void list_flag(u32* flag, const int f, const i64 q) {
    atomicOr(&flag[0], 1u << f);
    atomicMin(&flag[1 + f], (u32)q);
}

static __global__ __launch_bounds__(256) void k_list_merge_grades(const ListMergeGradesArgs a) {
    const i64 vrow = a.Rp >> 4, nvec = a.Q * vrow;
    const i64 block = a.Q * a.Rp + 4 * a.Qpad;
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t < nvec) {
        const i64 q = t / vrow, col = (t - q * vrow) << 4;
        u32 acc[4] = {0u, 0u, 0u, 0u}, m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                        // the bytes i < R of each word: the pad bytes are masked off as they arrive
            const i64 left = a.R - (col + 4 * k);
            m[k] = left >= 4 ? ~0u : left <= 0 ? 0u : (1u << (8 * (int)left)) - 1u;
        }
        u32 twice = 0;
        for (int r = 0; r < a.Gsh; ++r) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.blocks + (i64)r * block + (t << 4));
            const u32 w[4] = {v.x & m[0], v.y & m[1], v.z & m[2], v.w & m[3]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                twice |= nonzero_bytes(acc[k]) & nonzero_bytes(w[k]);
                acc[k] |= w[k];
            }
        }
        bool range = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int s = 0; s < 32; s += 8) range |= ((acc[k] >> s) & 255u) > (u32)a.C;
        *reinterpret_cast<uint4*>(a.dst + (t << 4)) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
        if (twice) list_flag(a.flag, 1, q);
        if (range) list_flag(a.flag, 2, q);
    } else if (t - nvec < a.Q) {
        const i64 q = t - nvec;
        u64 s = 0;
        for (int r = 0; r < a.Gsh; ++r) s += reinterpret_cast<const u32*>(a.blocks + (i64)r * block + a.Q * a.Rp)[q];
        if (s != (u64)a.R) list_flag(a.flag, 0, q);
    }
}

struct ListMergeVotesArgs {
    const u32* tabs;                   // [Gsh][nk][C + 1][Qpad]
    u32* dst;                          // [Q][nk][C]
    u32* flag;                         // [4], see above
    const i64* ks;                     // [nk]
    i64 Q, Qpad;
    int nk, C, Gsh;
};

static __global__ __launch_bounds__(SM_THREADS) void k_list_merge_votes(const ListMergeVotesArgs a) {
    const int tid = (int)threadIdx.x, quad = tid & 15, pl = tid >> 4;
    const i64 q0 = (i64)blockIdx.x * 64 + quad * 4;          // (< Qpad: the grid is Qpad / 64)
    const i64 planes = (i64)a.nk * (a.C + 1), block = planes * a.Qpad;
    for (i64 p = pl; p < planes; p += SM_LANES) {
        const int j = (int)(p / (a.C + 1)), c = (int)(p - (i64)j * (a.C + 1));
        const i64 off = p * a.Qpad + q0;
        u64 s[4] = {0, 0, 0, 0};
        for (int r = 0; r < a.Gsh; ++r) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.tabs + (i64)r * block + off);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        }
        const u64 want = c == a.C ? (u64)a.ks[j] : 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const i64 q = q0 + k;
            if (q >= a.Q) continue;
            if (s[k] >> 32) list_flag(a.flag, 0, q);
            if (c == a.C) {
                if (s[k] != want) list_flag(a.flag, 1, q);
            } else {
                a.dst[(q * a.nk + j) * a.C + c] = (u32)s[k];
            }
        }
    }
}

// the cut-offs of a vote pack or merge, handed over by value
struct Cutoffs { i64 v[VT_MAX_K]; };
static __global__ void k_put_cutoffs(const Cutoffs k, i64* __restrict__ dst, const int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = k.v[threadIdx.x];
}

struct VotePickArgs {
    const u32* votes;                  // [Q][nk][C]
    int* pred;                         // [Q][nk]
    u32* top;                          // [Q][nk]
    i64 n;                             // Q nk
    int C;
};

static __global__ __launch_bounds__(256) void k_vote_pick(const VotePickArgs a) {
    const int lane = threadIdx.x & 63;
    const i64 o = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= a.n) return;
    const u32* __restrict__ row = a.votes + o * a.C;
    u64 key = 0;
#pragma unroll
    for (int w = 0; w < VT_WORDS; ++w) {
        const int c = w * 64 + lane;
        const u64 k = c < a.C ? (u64)row[c] << 8 | (u64)(255 - c) : 0ull;
        key = k > key ? k : key;
    }
    key = wave_max_u64(key);
    if (lane == 0) {
        const u32 t = (u32)(key >> 8);
        a.top[o] = t;
        a.pred[o] = t ? 255 - (int)(key & 255ull) : -1;
    }
}

}  // namespace hg

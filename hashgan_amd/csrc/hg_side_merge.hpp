// hashgan_amd -- the order-free side tables of a database-sharded context: hg_rel_hist's, hg_grade_hist's and hg_joint_hist's tables
// are additive over shards, so the whole database's table is the cell-by-cell sum of the shards' tables and everything that reads
// one -- k_tie_ap, the lookup curves, the tie-aware graded reduction, IDCG -- reads the sum with the bits one context would give.
//
// The exchange unit of a table is one contiguous block of u32 planes [planes][Qpad], q fastest (Qpad = 64 x query tiles, equal on
// every rank because the queries are replicated):
//     rel     [2][NB][Qpad]      all, then rel
//     grade   [C + 1][Qpad]
//     joint   [NB][Gc][Qpad]     the shard's own [NB][Gs][Qpad] with zero planes for the grades Gs .. Gc - 1 (a shard's G depends
//                                on its own rows; Gc is the maximum over the shards)
// k_side_pack writes a shard's block, 16 bytes per thread.  k_side_merge sums the Gsh gathered blocks ([Gsh] equal blocks back to
// back, what an all-gather leaves): one workgroup per 64-query tile, thread = (plane lane 0..15, four queries), so a wavefront reads
// four planes x 256 contiguous bytes per block.  A cell is accumulated in 64 bits and stored as u32; a query's column total -- the
// sum over the planes that partition the database's rows: `all` for rel, every plane for grade and joint -- must be n_total.  Two
// flags, both set by integer atomics whose result does not depend on the order of arrival:
//     flag[0] bit 0   a cell of a real query (q < Q) does not fit 32 bits
//     flag[0] bit 1   a real query's column total is not n_total (a shard missing, counted twice or stale)
//     flag[1]         the smallest such query (atomicMin; 0xFFFFFFFF: none)
// The pad columns q >= Q are summed like the others (their low 32 bits) and never checked.
#pragma once
#include "hg_hist_joint.hpp"

namespace hg {

constexpr int SM_THREADS = 256;        // k_side_merge: 16 plane lanes x 16 quads of queries
constexpr int SM_LANES = SM_THREADS / 16;

struct SidePackArgs {
    const u32* src0; const u32* src1;  // the shard's table(s): planes [0, split) come from src0, planes [split, planes) from src1
    u32* dst;                          // [planes][Qpad]
    i64 Qpad, planes, split;
    int Gs, Gc;                        // src0's plane d * Gs + g lands in plane d * Gc + g; g >= Gs: zeros (1, 1: a plain copy)
};

static __global__ __launch_bounds__(256) void k_side_pack(const SidePackArgs a) {
    const i64 quads = a.Qpad >> 2;
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.planes * quads) return;
    const i64 p = i / quads, x = i - p * quads;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (p >= a.split) {
        v = reinterpret_cast<const uint4*>(a.src1 + (p - a.split) * a.Qpad)[x];
    } else {
        const i64 d = p / a.Gc;
        const int g = (int)(p - d * a.Gc);
        if (g < a.Gs) v = reinterpret_cast<const uint4*>(a.src0 + (d * a.Gs + g) * a.Qpad)[x];
    }
    reinterpret_cast<uint4*>(a.dst)[i] = v;
}

struct SideMergeArgs {
    const u32* tabs;                   // [Gsh][planes][Qpad]
    u32* dst;                          // [planes][Qpad]
    u32* flag;                         // [2], see above ({0, 0xFFFFFFFF} before the launch)
    i64 Q, Qpad, planes;
    i64 check_planes;                  // the planes [0, check_planes) add up to a query's column total
    i64 n_total;
    int Gsh;
};

static __global__ __launch_bounds__(SM_THREADS) void k_side_merge(const SideMergeArgs a) {
    __shared__ u64 cs[SM_LANES][64];   // column totals per plane lane
    __shared__ u32 co[SM_LANES][64];   // "a cell beyond 32 bits" per plane lane
    const int tid = (int)threadIdx.x, quad = tid & 15, pl = tid >> 4;
    const i64 q0 = (i64)blockIdx.x * 64 + quad * 4;          // (< Qpad: the grid is Qpad / 64)
    const i64 block = a.planes * a.Qpad;
    u64 col[4] = {0, 0, 0, 0};
    u32 over[4] = {0, 0, 0, 0};
    for (i64 p = pl; p < a.planes; p += SM_LANES) {
        const i64 off = p * a.Qpad + q0;
        u64 s[4] = {0, 0, 0, 0};
        for (int r = 0; r < a.Gsh; ++r) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.tabs + (i64)r * block + off);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        }
        *reinterpret_cast<uint4*>(a.dst + off) = make_uint4((u32)s[0], (u32)s[1], (u32)s[2], (u32)s[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            over[k] |= (u32)(s[k] >> 32);
            if (p < a.check_planes) col[k] += s[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cs[pl][quad * 4 + k] = col[k];
        co[pl][quad * 4 + k] = over[k];
    }
    __syncthreads();
    const i64 q = (i64)blockIdx.x * 64 + tid;
    if (tid >= 64 || q >= a.Q) return;
    u64 total = 0;
    u32 o = 0;
#pragma unroll
    for (int l = 0; l < SM_LANES; ++l) { total += cs[l][tid]; o |= co[l][tid]; }
    if (o) atomicOr(&a.flag[0], 1u);
    if (total != (u64)a.n_total) {
        atomicOr(&a.flag[0], 2u);
        atomicMin(&a.flag[1], (u32)q);
    }
}

}  // namespace hg

// Features and labels that already lie in device memory (hg_set_database_dev / hg_set_queries_dev): one fused pack straight out of
// the caller's arrays, whatever their strides and element type -- no staging copy, no second pass for the float table.
//
// k_pack_dev<DT, VEC>   one wavefront per row, WPB rows per block, the blocks striding over the table (at most 8 per CU: the census
//                       leaves with three atomics per wavefront, and a million rows' worth on one address is a queue of its own).  A
//                       row is read ONCE and gives, from that one read: the packed code words u32 [n][NW] (bit = v > 0, the words
//                       k_pack_sign_f32 writes), the census (bad[0] entries outside {-1, 0, +1}, NaN included; bad[2] zeros; bad[3]
//                       minus ones) and -- fout != null -- the float32 row at pitch bpad, pad columns zero (what hg_map_real streams).
//                       float16 / bfloat16 are widened to float32 exactly before anything looks at the value.
//                         VEC    unit column stride, base and row pitch multiples of 16 bytes (hg_dev::vector_loads_ok): a lane takes
//                                16 bytes -- 4 floats or 8 halves -- so the wavefront covers the whole row (b <= 255) with one load
//                                instruction; the lane whose 16 bytes straddle the row's end reads its elements one by one (nothing is
//                                read beyond the extent the host verified); a code word is OR-ed together across its 8 (4) lanes.
//                         !VEC   any strides, any alignment: a lane per column, 64 columns per ballot, like k_pack_sign_f32.
//                       Same predicates on the same values: both paths write identical bytes (tests/test_dev_input_gpu.py).
//                       codes == null: the float rows only (the second pass of keep_floats = 2), no census.
// k_pack_labels_dev<DT> the same shape for labels: int64 / int32 / uint8 (bool) / float32, bit = v != 0, bad[1] counts entries that
//                       are not exactly 0 or 1 (0.5, NaN).  u64 [n][LW] as k_pack_labels_i64 writes.  A lane per column: label rows
//                       are short, and 64 consecutive elements per instruction are coalesced for every element size.
// Stores are plain vector stores; no inline assembly.
#pragma once
#include "hg_ctx.hpp"
#include "hg_dev_desc.hpp"

namespace hg {

static_assert(HG_MAX_BITS < 256, "k_pack_dev's 16-byte path covers a row with one load per lane: 64 lanes x 4 floats");

// raw element -> float32, exactly
template <int DT> struct DevFeat;
template <> struct DevFeat<HG_F32> {
    typedef u32 E;
    static __device__ __forceinline__ float widen(u32 bits) { return __uint_as_float(bits); }
};
template <> struct DevFeat<HG_F16> {
    typedef unsigned short E;
    static __device__ __forceinline__ float widen(u32 bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
};
template <> struct DevFeat<HG_BF16> {
    typedef unsigned short E;
    static __device__ __forceinline__ float widen(u32 bits) { return __uint_as_float(bits << 16); }
};

struct DevCensus {
    u32 bad = 0, zero = 0, neg = 0;
    __device__ __forceinline__ void see(float v) {
        bad += !(v == 1.0f || v == -1.0f || v == 0.0f);
        zero += v == 0.0f;
        neg += v == -1.0f;
    }
};
static __device__ __forceinline__ u32 wave_sum(u32 x) {
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

template <int DT, bool VEC>
static __global__ __launch_bounds__(256) void k_pack_dev(const void* __restrict__ src, const i64 rs, const i64 cs, const i64 n, const int b,
                                                         const int NW, u32* __restrict__ codes, float* __restrict__ fout, const int bpad,
                                                         unsigned long long* __restrict__ bad) {
    typedef typename DevFeat<DT>::E E;
    const int lane = threadIdx.x & 63;
    const bool pack = codes != nullptr;
    DevCensus cs3;
    for (i64 r = (i64)blockIdx.x * WPB + (threadIdx.x >> 6); r < n; r += (i64)gridDim.x * WPB) {
        const E* __restrict__ row = (const E*)src + r * rs;
        if (VEC) {
            constexpr int V = 16 / (int)sizeof(E);         // elements per lane: 4 floats, 8 halves
            constexpr int G = 32 / V;                      // lanes per code word: 8, 4
            const int col0 = lane * V;
            float v[V];
            if (col0 + V <= b) {
                const uint4 q = *reinterpret_cast<const uint4*>(row + col0);
                const u32 w[4] = {q.x, q.y, q.z, q.w};
                if (sizeof(E) == 4) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = DevFeat<DT>::widen(w[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[(2 * k) % V] = DevFeat<DT>::widen(w[k] & 0xFFFFu);
                        v[(2 * k + 1) % V] = DevFeat<DT>::widen(w[k] >> 16);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = col0 + k < b ? DevFeat<DT>::widen(row[col0 + k]) : 0.0f;
            }
            if (pack) {
                u32 bits = 0;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    if (col0 + k < b) {
                        cs3.see(v[k]);
                        bits |= (u32)(v[k] > 0.0f) << k;
                    }
                }
                u32 part = bits << (V * (lane & (G - 1)));
#pragma unroll
                for (int m = 1; m < G; m <<= 1) part |= __shfl_xor(part, m);
                if ((lane & (G - 1)) == 0 && lane / G < NW) codes[r * NW + lane / G] = part;
            }
            if (fout && col0 < bpad) {                    // (bpad is a multiple of 16: a lane's columns are all inside or all outside)
                float4* __restrict__ dst = reinterpret_cast<float4*>(fout + r * bpad + col0);
#pragma unroll
                for (int k = 0; k < V; k += 4) dst[k / 4] = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
            }
        } else {
            for (int c0 = 0; c0 < b; c0 += 64) {           // (these slabs also cover the pad columns: ceil64(b) >= ceil16(b))
                const int col = c0 + lane;
                const bool valid = col < b;
                const float v = valid ? DevFeat<DT>::widen(row[(i64)col * cs]) : 0.0f;
                if (pack) {
                    if (valid) cs3.see(v);
                    const u64 word = __ballot(valid && v > 0.0f);
                    const int w = c0 >> 5;
                    if (lane == 0) {
                        codes[r * NW + w] = (u32)word;
                        if (w + 1 < NW) codes[r * NW + w + 1] = (u32)(word >> 32);
                    }
                }
                if (fout && col < bpad) fout[r * bpad + col] = v;
            }
        }
    }
    if (!pack) return;
    // bad[0]: entries outside {-1, 0, +1}; bad[2]: zeros; bad[3]: minus ones (bad[1] belongs to the labels)
    const u32 nbad = wave_sum(cs3.bad), nzero = wave_sum(cs3.zero), nneg = wave_sum(cs3.neg);
    if (lane == 0) {
        if (nbad) atomicAdd(bad, (unsigned long long)nbad);
        if (nzero) atomicAdd(bad + 2, (unsigned long long)nzero);
        if (nneg) atomicAdd(bad + 3, (unsigned long long)nneg);
    }
}

// raw label element -> (nonzero, neither 0 nor 1)
template <int DT> struct DevLab;
template <> struct DevLab<HG_I64> { typedef long long E; };
template <> struct DevLab<HG_I32> { typedef int E; };
template <> struct DevLab<HG_U8> { typedef unsigned char E; };
template <> struct DevLab<HG_F32> { typedef float E; };           // (NaN != 0: the bit is set, and it counts as bad)

template <int DT>
static __global__ __launch_bounds__(256) void k_pack_labels_dev(const void* __restrict__ src, const i64 rs, const i64 cs, const i64 n, const int C,
                                                                const int LW, u64* __restrict__ out, unsigned long long* __restrict__ bad) {
    typedef typename DevLab<DT>::E E;
    const int lane = threadIdx.x & 63;
    u32 nbad = 0;
    for (i64 r = (i64)blockIdx.x * WPB + (threadIdx.x >> 6); r < n; r += (i64)gridDim.x * WPB) {
        const E* __restrict__ row = (const E*)src + r * rs;
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int col = c0 + lane;
            const E v = col < C ? row[(i64)col * cs] : (E)0;
            nbad += !(v == (E)0 || v == (E)1);
            const u64 word = __ballot(v != (E)0);
            if (lane == 0) out[r * LW + (c0 >> 6)] = word;
        }
    }
    nbad = wave_sum(nbad);
    if (lane == 0 && nbad) atomicAdd(bad + 1, (unsigned long long)nbad);
}

}  // namespace hg

// ---- launchers ------------------------------------------------------------------------------------------------------------
// Blocks stride over the rows; 8 blocks of 4 wavefronts fill a CU's wavefront slots.
inline int dev_pack_grid(const hg_ctx* c, i64 n) {
    const i64 want = (n + WPB - 1) / WPB, cap = (i64)c->n_cu * 8;
    return (int)(want < cap ? want : cap);
}

template <int DT>
static int launch_pack_dev_t(hg_ctx* c, const hg_dev_array& f, u32* codes, float* fout, int bpad) {
    const dim3 grid(dev_pack_grid(c, f.rows)), block(256);
    unsigned long long* bad = c->badcnt.as<unsigned long long>();
    c->t_begin(KI_PACK);
    if (hg_dev::vector_loads_ok(f))
        hipLaunchKernelGGL((k_pack_dev<DT, true>), grid, block, 0, c->stream, f.ptr, (i64)f.row_stride, (i64)f.col_stride, (i64)f.rows,
                           c->b, c->NW, codes, fout, bpad, bad);
    else
        hipLaunchKernelGGL((k_pack_dev<DT, false>), grid, block, 0, c->stream, f.ptr, (i64)f.row_stride, (i64)f.col_stride, (i64)f.rows,
                           c->b, c->NW, codes, fout, bpad, bad);
    c->t_end();
    return c->check_launch("k_pack_dev");
}
// codes == null: the float rows only; fout == null: codes and census only
static int launch_pack_dev(hg_ctx* c, const hg_dev_array& f, u32* codes, float* fout, int bpad) {
    switch (f.dtype) {
        case HG_F32: return launch_pack_dev_t<HG_F32>(c, f, codes, fout, bpad);
        case HG_F16: return launch_pack_dev_t<HG_F16>(c, f, codes, fout, bpad);
        case HG_BF16: return launch_pack_dev_t<HG_BF16>(c, f, codes, fout, bpad);
        default: return fail(HG_ERR_ARG, "k_pack_dev: feature dtype %d", f.dtype);
    }
}

template <int DT>
static int launch_pack_labels_dev_t(hg_ctx* c, const hg_dev_array& l, u64* out) {
    c->t_begin(KI_PACK);
    hipLaunchKernelGGL((k_pack_labels_dev<DT>), dim3(dev_pack_grid(c, l.rows)), dim3(256), 0, c->stream, l.ptr, (i64)l.row_stride,
                       (i64)l.col_stride, (i64)l.rows, c->C, c->LW, out, c->badcnt.as<unsigned long long>());
    c->t_end();
    return c->check_launch("k_pack_labels_dev");
}
static int launch_pack_labels_dev(hg_ctx* c, const hg_dev_array& l, u64* out) {
    switch (l.dtype) {
        case HG_I64: return launch_pack_labels_dev_t<HG_I64>(c, l, out);
        case HG_I32: return launch_pack_labels_dev_t<HG_I32>(c, l, out);
        case HG_U8: return launch_pack_labels_dev_t<HG_U8>(c, l, out);
        case HG_F32: return launch_pack_labels_dev_t<HG_F32>(c, l, out);
        default: return fail(HG_ERR_ARG, "k_pack_labels_dev: label dtype %d", l.dtype);
    }
}

// Results into the caller's DEVICE memory (hg_export): one streaming copy-convert per item out of the context's result buffers into an
// array laid out as the caller's framework made it, whatever its strides and element type -- no staging copy, no host pass.
//
// k_export<CLS, D, VEC>   no LDS, no atomics; every destination element is written exactly once.  Blocks stride over the work (at most
//                         8 per CU, like k_pack_dev).  CLS names what is read, D what is written:
//                           XC_U32  u32 [Q][pitch]          ranked indices, scores (their bits), hit counts     -> i64 (zero-extended) | u32 (the bits)
//                           XC_U8   u8 [Q][pitch]           distances, grades                                   -> u8 | u32 (widened)
//                           XC_BIT  u64 [Q][pitch words]    the match bitmap, rank r = bit r of the query's row -> u8 0 / 1
//                           XC_F64  f64 [Q][pitch]          APs                                                 -> u64 (the bits) | float (correctly rounded)
//                           VEC    unit column stride, base and row pitch multiples of 16 bytes (hg_dev::vector_stores_ok): a lane produces
//                                  16 destination bytes -- 2 i64, 4 32-bit elements or 16 bytes -- and stores them with one instruction, so a
//                                  wavefront writes 1 KiB of consecutive addresses.  Its source elements are loaded one by one (a source row is
//                                  only element-aligned when R is odd), bytes four at a time where their address allows: no load reaches beyond
//                                  the lane's own elements, so none leaves the source's Q x R.  16 match bits become 16 bytes in registers.
//                                  The lane whose 16 bytes straddle the end of a row (k no multiple of the vector) writes its elements one
//                                  by one: nothing beyond the extent the host verified is touched.
//                           !VEC   any strides, any alignment: a lane per element.
//                         Same conversions on the same values: both paths write identical bytes (tests/test_dev_output_gpu.py).
// Stores are plain vector stores; no inline assembly.
#pragma once
#include "hg_ctx.hpp"
#include "hg_dev_desc.hpp"

namespace hg {

enum ExportClass { XC_U32 = 0, XC_U8, XC_BIT, XC_F64 };

template <int CLS> struct ExportSrc;
template <> struct ExportSrc<XC_U32> { typedef u32 E; };
template <> struct ExportSrc<XC_U8> { typedef u8 E; };
template <> struct ExportSrc<XC_BIT> { typedef u64 E; };
template <> struct ExportSrc<XC_F64> { typedef u64 E; };

// one source value -> one destination element
template <int CLS, class D> struct ExportCvt {
    static __device__ __forceinline__ D of(typename ExportSrc<CLS>::E v) { return (D)v; }               // zero-extension, or the same bits
};
template <> struct ExportCvt<XC_F64, float> {
    static __device__ __forceinline__ float of(u64 v) { return (float)__longlong_as_double((long long)v); }   // round to nearest even; NaN stays NaN
};

// element (q, r) of the source
template <int CLS>
static __device__ __forceinline__ typename ExportSrc<CLS>::E export_load(const typename ExportSrc<CLS>::E* __restrict__ src, i64 pitch, i64 q, i64 r) {
    if constexpr (CLS == XC_BIT) return (src[q * pitch + (r >> 6)] >> (r & 63)) & 1ull;
    else return src[q * pitch + r];
}

// 4 bits -> 4 bytes of 0 / 1 (bit i in byte i)
static __device__ __forceinline__ u32 export_spread4(u32 x) {
    return (x & 1u) | ((x & 2u) << 7) | ((x & 4u) << 14) | ((x & 8u) << 21);
}

template <int CLS, class D, bool VEC>
static __global__ __launch_bounds__(256) void k_export(const void* __restrict__ src_, const i64 pitch, D* __restrict__ dst, const i64 rs, const i64 cs,
                                                       const i64 Q, const i64 k) {
    typedef typename ExportSrc<CLS>::E E;
    const E* __restrict__ src = (const E*)src_;
    const i64 step = (i64)gridDim.x * blockDim.x;
    if (VEC) {
        constexpr int V = 16 / (int)sizeof(D);             // elements per lane: 2, 4 or 16
        const i64 nv = (k + V - 1) / V;                    // vectors per row, the last one possibly short
        for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < Q * nv; v += step) {
            const i64 q = v / nv, col0 = (v - q * nv) * V;
            D* __restrict__ out = dst + q * rs + col0;     // (cs == 1; a multiple of 16 bytes from the aligned base)
            if (col0 + V <= k) {
                union { uint4 q4; D e[V]; u32 w[4]; } pk;
                if constexpr (CLS == XC_BIT) {             // 16 bits of one bitmap word (col0 is a multiple of 16)
                    const u32 bits = (u32)(src[q * pitch + (col0 >> 6)] >> (col0 & 63)) & 0xFFFFu;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pk.w[j] = export_spread4((bits >> (4 * j)) & 15u);
                } else if constexpr (CLS == XC_U8) {
                    const u8* __restrict__ s = (const u8*)src + q * pitch + col0;
                    constexpr int NWD = V / 4;             // source dwords: 4 (u8 -> u8) or 1 (u8 -> u32)
                    u32 w[NWD];
                    if (((uintptr_t)s & 3) == 0) {
#pragma unroll
                        for (int j = 0; j < NWD; ++j) w[j] = reinterpret_cast<const u32*>(s)[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < NWD; ++j) w[j] = (u32)s[4 * j] | ((u32)s[4 * j + 1] << 8) | ((u32)s[4 * j + 2] << 16) | ((u32)s[4 * j + 3] << 24);
                    }
#pragma unroll
                    for (int j = 0; j < V; ++j) pk.e[j] = (D)((w[j / 4] >> (8 * (j % 4))) & 0xFFu);
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) pk.e[j] = ExportCvt<CLS, D>::of(src[q * pitch + col0 + j]);
                }
                *reinterpret_cast<uint4*>(out) = pk.q4;
            } else {
                for (i64 r = col0; r < k; ++r) out[r - col0] = ExportCvt<CLS, D>::of(export_load<CLS>(src, pitch, q, r));
            }
        }
    } else {
        for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < Q * k; e += step) {
            const i64 q = e / k, r = e - q * k;
            dst[q * rs + r * cs] = ExportCvt<CLS, D>::of(export_load<CLS>(src, pitch, q, r));
        }
    }
}

}  // namespace hg

// ---- launcher -------------------------------------------------------------------------------------------------------------
// One item, validated by hg_export: `src` [Q][pitch] of class `cls` into `d`.  *vec: the 16-byte path was taken.
template <int CLS, class D>
static int launch_export_t(hg_ctx* c, const void* src, i64 pitch, const hg_dev_array& d, bool* vec) {
    const i64 Q = d.rows, k = d.cols;
    const int V = 16 / (int)sizeof(D);
    *vec = hg_dev::vector_stores_ok(d) && k > 1;           // (a column of Q elements -- AP, HITS -- goes element-wise)
    const i64 work = *vec ? Q * ((k + V - 1) / V) : Q * k;
    const i64 want = (work + 255) / 256, cap = (i64)c->n_cu * 8;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(256);
    c->t_begin(KI_EXPORT);
    if (*vec)
        hipLaunchKernelGGL((k_export<CLS, D, true>), grid, block, 0, c->stream, src, pitch, (D*)const_cast<void*>(d.ptr), (i64)d.row_stride,
                           (i64)d.col_stride, Q, k);
    else
        hipLaunchKernelGGL((k_export<CLS, D, false>), grid, block, 0, c->stream, src, pitch, (D*)const_cast<void*>(d.ptr), (i64)d.row_stride,
                           (i64)d.col_stride, Q, k);
    c->t_end();
    return c->check_launch("k_export");
}

static int launch_export(hg_ctx* c, int cls, const void* src, i64 pitch, const hg_dev_array& d, bool* vec) {
    switch (cls) {
        case XC_U32:
            if (d.dtype == HG_I64) return launch_export_t<XC_U32, u64>(c, src, pitch, d, vec);
            return launch_export_t<XC_U32, u32>(c, src, pitch, d, vec);                    // int32, float32: the same 32 bits
        case XC_U8:
            if (d.dtype == HG_U8) return launch_export_t<XC_U8, u8>(c, src, pitch, d, vec);
            return launch_export_t<XC_U8, u32>(c, src, pitch, d, vec);
        case XC_BIT: return launch_export_t<XC_BIT, u8>(c, src, pitch, d, vec);
        case XC_F64:
            if (d.dtype == HG_F64) return launch_export_t<XC_F64, u64>(c, src, pitch, d, vec);
            return launch_export_t<XC_F64, float>(c, src, pitch, d, vec);
        default: return fail(HG_ERR_ARG, "k_export: class %d", cls);
    }
}

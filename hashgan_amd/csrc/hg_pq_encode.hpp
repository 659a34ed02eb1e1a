// hashgan_amd -- the exact product-quantisation encoder's kernels (hg_pq_encode / hg_pq_encode_dev / hg_set_database_pq_f32; DESIGN.md
// section 8, "Quantised databases").
//
// Codebooks f32 [M][K][dsub], a feature row x (b = M * dsub <= 255, K <= 256).  The code of subspace m, all in IEEE float64, every
// operation rounded once, no fused multiply-add, features and codewords ascending, a strict `<`:
//     d_k = 0.0;  for j = 0 .. dsub-1:  t = (double)x[m*dsub+j] - (double)w[m][k][j];  d_k = d_k + t*t
//     code = the lowest k with d_k minimal:  best = 0; for k = 1 .. K-1: if (d_k < d_best) best = k
//     err(row) = 0.0; for m = 0 .. M-1: err += d_best(m)
// A non-finite feature makes every d_k of its subspace +inf or NaN, so the strict `<` leaves code 0; such rows are counted.
//
//   k_pq_books_f64   the codebooks widened to float64 once per call (a few hundred KB at most), so that the chain's codeword operand needs no
//                    conversion inside the loops.
//   k_pq_encode<D>   one wavefront = 64 consecutive rows over all M subspaces, lane = row, one wavefront per block.  Per subspace the
//                    wavefront brings its rows' subvectors into LDS as float32 (element by element through the caller's
//                    strides and element type: whatever of a row's cache lines one subspace leaves unused the next ones take from the
//                    cache), widened exactly from float16 / bfloat16.  The codeword operand is wave-uniform: read from the float64
//                    copy through the constant address space, i.e. by scalar loads into scalar registers, which the float64 vector
//                    instructions take as an operand directly.  That leaves three float64 vector instructions per (row, codeword,
//                    feature) -- subtract, multiply, add -- and one compare and three selects per codeword.
//                      D = 1 .. 16   the register path: the row's subvector is widened into 2 D vector registers once per subspace.
//                      D = 0         the generic path, any dsub up to 255: the subvector stays in LDS, padded with zeros to whole
//                                    groups of four features (so are the float64 codewords: adding +0.0 changes no bit), float32
//                                    [dp / 4][64][4]; a lane reads a group with one 16-byte read and widens it -- a fourth
//                                    float64-rate instruction per step; sixteen features per wait (the loop is unrolled by four).
//                    A wavefront alone is bound by the latency of its scalar loads and waits: the launcher
//                    gives a launch as many rows as the work buffers allow.
//                    Rows >= N of a tail wavefront compute on zeros and write nothing.  Stores are plain vector stores; the count of
//                    rows with a non-finite feature leaves with one vector atomic per wavefront that has any.
#pragma once
#include "hg_kernels.hpp"
#include "hg_dev_in.hpp"

namespace hg {

constexpr int PQE_PITCH = 65;          // register path: words between two features' columns in LDS (lanes that stage one row's features hit different banks)
constexpr int PQE_MAX_REG = 16;        // the register path's largest dsub

// wd [M][K][dp] = (double)w [M][K][dsub], features dsub .. dp - 1 zero (dp = dsub: a plain copy).  A zero feature on both sides adds
// t * t = +0.0 to a sum that is never -0.0: the generic path's padding to whole groups of four changes no bit.
static __global__ __launch_bounds__(256) void k_pq_books_f64(const float* __restrict__ w, double* __restrict__ wd, const int n, const int dsub, const int dp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int cw = i / dp, j = i - cw * dp;
    wd[i] = j < dsub ? (double)w[cw * dsub + j] : 0.0;
}

struct PqEncArgs {
    const void* src;            // element (r, c) at src + (r * rs + c * cs) * itemsize(dtype)
    i64 rs, cs;
    int dtype;                  // HG_F32, HG_F16, HG_BF16
    i64 n;                      // rows of this launch (< 2^31)
    const double* wd;           // f64 [M][K][dp]
    int M, K, dsub;
    int dp;                     // features per codeword in wd: dsub (register path) or dsub rounded up to 4 (generic path)
    u8* codes;                  // [n][M]
    double* err;                // [n]
    unsigned long long* bad;    // += rows with a non-finite feature
};

static __device__ __forceinline__ float pqe_load(const void* src, const i64 e, const int dtype) {
    if (dtype == HG_F32) return ((const float*)src)[e];
    const u32 bits = ((const unsigned short*)src)[e];
    return dtype == HG_F16 ? DevFeat<HG_F16>::widen(bits) : DevFeat<HG_BF16>::widen(bits);
}
static __device__ __forceinline__ bool pqe_nonfinite(const float f) { return !(__builtin_fabsf(f) < INFINITY); }

typedef const __attribute__((address_space(4))) double* PqeBook;     // wave-uniform reads: scalar loads

template <int D>
static __global__ __launch_bounds__(64) void k_pq_encode(const PqEncArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float pqe_x[];           // D > 0: [D][PQE_PITCH]; D = 0: [dp / 4][64][4]
    const int lane = threadIdx.x;
    const int M = a.M, K = a.K, dsub = D ? D : a.dsub, dp = D ? D : a.dp;
    const i64 row0 = (i64)blockIdx.x * 64, row = row0 + lane;
    const int rows = (int)(a.n - row0 < 64 ? a.n - row0 : 64);
    const PqeBook wd = (PqeBook)(uintptr_t)a.wd;
    double err = 0.0;
    bool nonfinite = false;
    for (int m = 0; m < M; ++m) {
        __syncthreads();                                     // (the last subspace's reads are done)
        for (int e = lane; e < 64 * dp; e += 64) {
            const int r = e / dp, j = e - r * dp;
            const float v = r < rows && j < dsub ? pqe_load(a.src, (row0 + r) * a.rs + (i64)(m * dsub + j) * a.cs, a.dtype) : 0.0f;
            pqe_x[D ? j * PQE_PITCH + r : ((j >> 2) * 64 + r) * 4 + (j & 3)] = v;
        }
        __syncthreads();
        const PqeBook wm = wd + (i64)m * K * dp;
        int best = 0;
        double dbest = 0.0;
        if constexpr (D > 0) {
            double x[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float f = pqe_x[j * PQE_PITCH + lane];
                nonfinite |= pqe_nonfinite(f);
                x[j] = (double)f;
            }
#pragma unroll 2
            for (int k = 0; k < K; ++k) {
                double d = 0.0;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double t = x[j] - wm[k * D + j];
                    d = d + t * t;
                }
                const bool take = k == 0 || d < dbest;
                best = take ? k : best;
                dbest = take ? d : dbest;
            }
        } else {
            const float4* __restrict__ x4 = reinterpret_cast<const float4*>(pqe_x) + lane;
            const int groups = dp >> 2;
            for (int g = 0; g < groups; ++g) {
                const float4 f = x4[g * 64];
                nonfinite = nonfinite || pqe_nonfinite(f.x) || pqe_nonfinite(f.y) || pqe_nonfinite(f.z) || pqe_nonfinite(f.w);
            }
            for (int k = 0; k < K; ++k) {
                const PqeBook wk = wm + k * dp;
                double d = 0.0;
#pragma unroll 4
                for (int g = 0; g < groups; ++g) {
                    const float4 f = x4[g * 64];
                    const double t0 = (double)f.x - wk[4 * g], t1 = (double)f.y - wk[4 * g + 1];
                    const double t2 = (double)f.z - wk[4 * g + 2], t3 = (double)f.w - wk[4 * g + 3];
                    d = d + t0 * t0;
                    d = d + t1 * t1;
                    d = d + t2 * t2;
                    d = d + t3 * t3;
                }
                const bool take = k == 0 || d < dbest;
                best = take ? k : best;
                dbest = take ? d : dbest;
            }
        }
        err += dbest;
        if (lane < rows) a.codes[row * M + m] = (u8)best;
    }
    if (lane < rows) a.err[row] = err;
    const u64 nf = __ballot(nonfinite && lane < rows);
    if (lane == 0 && nf) atomicAdd(a.bad, (unsigned long long)__popcll(nf));
}

}  // namespace hg

// libhashgan_amd.so -- the exact product-quantisation encoder (hg_pq_encode, hg_pq_encode_dev) and the loader that goes from float
// features to a quantised context (hg_set_database_pq_f32): hg_pq_encode.hpp has the contract and the kernels, DESIGN.md section 8,
// "Quantised databases", the measurements.  The encoder reads and writes nothing of the context but work buffers, the census counter
// and two statistics: tables, ranked lists, PQ tables, generations and hg_map_begin's licence stay as they were.
#include "hg_ctx.hpp"
#include "hg_pq_encode.hpp"
#include <algorithm>

namespace {

// What both encoders check of the codebooks' shape and values before anything is launched.
int check_books(const char* who, const float* books, int M, int K, int dsub) {
    if (M < 1) return fail(HG_ERR_ARG, "%s: M=%d subspaces (need >= 1)", who, M);
    if (K < 1 || K > 256) return fail(HG_ERR_ARG, "%s: K=%d codewords outside 1..256", who, K);
    if (dsub < 1) return fail(HG_ERR_ARG, "%s: dsub=%d features per subspace (need >= 1)", who, dsub);
    if ((i64)M * dsub > HG_MAX_BITS) return fail(HG_ERR_ARG, "%s: M * dsub = %lld features, more than %d", who, (long long)M * dsub, HG_MAX_BITS);
    if (!books) return fail(HG_ERR_ARG, "%s: null codebooks", who);
    const size_t n = (size_t)M * K * dsub;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(books[i]))
            return fail(HG_ERR_ARG, "%s: codebook entry [%d][%d][%d] is not finite", who, (int)(i / dsub / K), (int)(i / dsub % K), (int)(i % dsub));
    return HG_OK;
}

// Rows per launch: option "pq_encode_chunk_rows", or what keeps the work buffers at 256 MB -- of float32 features on their way up
// (host), of codes and errors on their way back (device features stay where they are) -- in whole wavefronts.  A launch is one
// wavefront per 64 rows and a wavefront's chain is long, so a launch wants many times the GPU's 8192 wavefront slots' worth of rows
// where the table has them: a chunk of 64 MB (4096 wavefronts at b = 64, 1028 at b = 255) was measured at half the rate and less.
i64 chunk_rows(const hg_ctx* c, int b, int M, bool host) {
    if (c->opt.pq_encode_chunk_rows > 0) return c->opt.pq_encode_chunk_rows;
    const i64 r = ((i64)256 << 20) / (host ? 4 * (i64)b : (i64)M + 8);
    return r / 64 * 64;
}

template <int D> int launch_encode_t(hg_ctx* c, const PqEncArgs& a) {
    const size_t lds = D ? (size_t)D * PQE_PITCH * 4 : (size_t)a.dp * 64 * 4;         // (dp <= 256: at most 64 KB)
    c->t_begin(KI_PQ_ENCODE);
    hipLaunchKernelGGL(k_pq_encode<D>, dim3((unsigned)((a.n + 63) / 64)), dim3(64), lds, c->stream, a);
    c->t_end();
    return c->check_launch("k_pq_encode");
}
// features per codeword of the float64 copy: the generic path reads whole groups of four
int books_pitch(int dsub) { return dsub <= PQE_MAX_REG ? dsub : (dsub + 3) / 4 * 4; }
int launch_encode(hg_ctx* c, const PqEncArgs& a) {
    switch (a.dsub) {
        case 1: return launch_encode_t<1>(c, a);    case 2: return launch_encode_t<2>(c, a);    case 3: return launch_encode_t<3>(c, a);
        case 4: return launch_encode_t<4>(c, a);    case 5: return launch_encode_t<5>(c, a);    case 6: return launch_encode_t<6>(c, a);
        case 7: return launch_encode_t<7>(c, a);    case 8: return launch_encode_t<8>(c, a);    case 9: return launch_encode_t<9>(c, a);
        case 10: return launch_encode_t<10>(c, a);  case 11: return launch_encode_t<11>(c, a);  case 12: return launch_encode_t<12>(c, a);
        case 13: return launch_encode_t<13>(c, a);  case 14: return launch_encode_t<14>(c, a);  case 15: return launch_encode_t<15>(c, a);
        case 16: return launch_encode_t<16>(c, a);
        default: return launch_encode_t<0>(c, a);
    }
}
static_assert(PQE_MAX_REG == 16, "launch_encode lists the register path's instances");

// The encoder proper, everything validated: rows [0, N) of `host` (float32 [N][b], through the work buffer pqe_in chunk by chunk) or of
// the device array `dev`; codes, err (optional) and the count of non-finite rows come back to the host, complete on return.
int encode_rows(hg_ctx* c, const float* host, const hg_dev_array* dev, i64 N, const float* books, int M, int K, int dsub, uint8_t* host_codes,
                double* host_err, int64_t* bad_rows) {
    const int b = M * dsub, dp = books_pitch(dsub), nw = M * K * dsub, nwd = M * K * dp;
    const i64 chunk = std::min<i64>(chunk_rows(c, b, M, host != nullptr), N);
    const FirstReservations fr;
    HG_TRY(c->pqe_books.reserve((size_t)nw * 4));
    HG_TRY(c->pqe_books64.reserve((size_t)nwd * 8));
    HG_TRY(c->pqe_codes.reserve((size_t)chunk * M));
    HG_TRY(c->pqe_err.reserve((size_t)chunk * 8));
    HG_TRY(c->badcnt.reserve(32));
    if (host) HG_TRY(c->pqe_in.reserve((size_t)chunk * b * 4));
    fr.keep(c);
    if (dev) HG_TRY(wait_for_producer(c, dev->stream));
    HG_HIP(hipMemsetAsync(c->badcnt.p, 0, 32, c->stream));
    HG_HIP(hipMemcpyAsync(c->pqe_books.p, books, (size_t)nw * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pq_books_f64, dim3(grid_for(nwd)), dim3(256), 0, c->stream, c->pqe_books.as<float>(), c->pqe_books64.as<double>(), nwd, dsub, dp);
    HG_TRY(c->check_launch("k_pq_books_f64"));
    PqEncArgs a{};
    a.wd = c->pqe_books64.as<double>();
    a.M = M; a.K = K; a.dsub = dsub; a.dp = dp;
    a.codes = c->pqe_codes.as<u8>();
    a.err = c->pqe_err.as<double>();
    a.bad = c->badcnt.as<unsigned long long>();
    for (i64 r0 = 0; r0 < N; r0 += chunk) {                // (one stream: a chunk's upload follows the kernel that read the last one, its kernel the downloads)
        const i64 n = std::min(chunk, N - r0);
        if (host) {
            HG_HIP(hipMemcpyAsync(c->pqe_in.p, host + r0 * b, (size_t)n * b * 4, hipMemcpyHostToDevice, c->stream));
            a.src = c->pqe_in.p; a.rs = b; a.cs = 1; a.dtype = HG_F32;
        } else {
            a.src = (const char*)dev->ptr + r0 * dev->row_stride * hg_dev::itemsize(dev->dtype);
            a.rs = dev->row_stride; a.cs = dev->col_stride; a.dtype = dev->dtype;
        }
        a.n = n;
        HG_TRY(launch_encode(c, a));
        HG_HIP(hipMemcpyAsync(host_codes + r0 * M, c->pqe_codes.p, (size_t)n * M, hipMemcpyDeviceToHost, c->stream));
        if (host_err) HG_HIP(hipMemcpyAsync(host_err + r0, c->pqe_err.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    unsigned long long bad = 0;
    HG_HIP(hipMemcpyAsync(&bad, c->badcnt.p, 8, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    *bad_rows = (int64_t)bad;
    c->pq_encode_calls++;
    c->pq_encoded_rows += N;
    return HG_OK;
}

int encode_host(hg_ctx* c, const char* who, const float* host_x, int64_t N, const float* books, int M, int K, int dsub, uint8_t* host_codes,
                double* host_err, int64_t* bad_rows) {
    if (!c) return fail(HG_ERR_ARG, "%s: null context", who);
    if (N < 1 || !host_x || !host_codes || !bad_rows) return fail(HG_ERR_ARG, "%s: need N >= 1, features, a place for the codes and bad_rows", who);
    HG_TRY(check_books(who, books, M, K, dsub));
    if (N >= 0x80000000ll) return fail(HG_ERR_ARG, "%s: N=%lld rows (need < 2^31)", who, (long long)N);
    HG_TRY(c->use());
    return encode_rows(c, host_x, nullptr, N, books, M, K, dsub, host_codes, host_err, bad_rows);
}

}  // namespace

extern "C" {

int hg_pq_encode(hg_ctx* c, const float* host_features, int64_t N, const float* host_books, int M, int K, int dsub, uint8_t* host_codes,
                 double* host_err, int64_t* bad_rows) {
    return encode_host(c, "hg_pq_encode", host_features, N, host_books, M, K, dsub, host_codes, host_err, bad_rows);
}

int hg_pq_encode_dev(hg_ctx* c, const hg_dev_array* f, const float* host_books, int M, int K, int dsub, uint8_t* host_codes, double* host_err,
                     int64_t* bad_rows) {
    const char* who = "hg_pq_encode_dev";
    if (!c) return fail(HG_ERR_ARG, "%s: null context", who);
    if (!f || !host_codes || !bad_rows) return fail(HG_ERR_ARG, "%s: need a feature descriptor, a place for the codes and bad_rows", who);
    HG_TRY(check_books(who, host_books, M, K, dsub));
    if (!f->ptr) return fail(HG_ERR_ARG, "%s: null data pointer", who);
    if (!hg_dev::feature_dtype(f->dtype))
        return fail(HG_ERR_ARG, "%s: feature dtype %d (%s) is not float32, float16 or bfloat16", who, f->dtype, hg_dev::dtype_name(f->dtype));
    if (f->row_stride < 1 || f->col_stride < 1)
        return fail(HG_ERR_ARG, "%s: feature strides (%lld, %lld) must both be >= 1 (in elements)", who, (long long)f->row_stride, (long long)f->col_stride);
    if (f->rows < 1 || f->rows >= 0x80000000ll) return fail(HG_ERR_ARG, "%s: N=%lld rows outside 1..2^31 - 1", who, (long long)f->rows);
    if (f->cols != (int64_t)M * dsub)
        return fail(HG_ERR_ARG, "%s: features have %lld columns, the codebooks M * dsub = %d", who, (long long)f->cols, M * dsub);
    int64_t extent = 0;
    if (!hg_dev::extent_bytes(*f, &extent)) return fail(HG_ERR_ARG, "%s: the array's extent in bytes does not fit 63 bits", who);
    HG_TRY(c->use());
    HG_TRY(check_dev_pointer(c, who, "features", *f, extent));
    return encode_rows(c, nullptr, f, f->rows, host_books, M, K, dsub, host_codes, host_err, bad_rows);
}

// Encode on the GPU, then the existing loader on the codes brought back (N x M bytes): the context ends up exactly as
// hg_set_database_pq leaves it for those codes.  What that loader refuses of the arguments it shares is refused here before any work.
int hg_set_database_pq_f32(hg_ctx* c, const float* host_features, const float* host_books, const int64_t* host_labels, int64_t N, int M, int K,
                           int dsub, int C, int64_t idx_base, int64_t n_total, int64_t* bad_codes, int64_t* bad_labels, int64_t* bad_rows) {
    const char* who = "hg_set_database_pq_f32";
    if (!c) return fail(HG_ERR_ARG, "%s: null context", who);
    if (N < 1 || !host_features || !host_labels) return fail(HG_ERR_ARG, "%s: need N >= 1 and data", who);
    if (C < 1) return fail(HG_ERR_ARG, "%s: C=%d", who, C);
    if (idx_base != 0 || n_total != N)
        return fail(HG_ERR_ARG, "%s: one shard only (idx_base=%lld, n_total=%lld for N=%lld rows)", who, (long long)idx_base, (long long)n_total, (long long)N);
    std::vector<uint8_t> codes;
    int64_t bad = 0;
    HG_TRY(check_books(who, host_books, M, K, dsub));
    if (N >= 0x80000000ll) return fail(HG_ERR_ARG, "%s: N=%lld rows (need < 2^31)", who, (long long)N);
    try { codes.resize((size_t)N * M); }
    catch (const std::exception& e) { return fail(HG_ERR_NOMEM, "%s: %s", who, e.what()); }
    HG_TRY(encode_host(c, who, host_features, N, host_books, M, K, dsub, codes.data(), nullptr, &bad));
    if (bad_rows) *bad_rows = bad;
    if (bad) return fail(HG_ERR_ARG, "%s: %lld rows have a non-finite feature; nothing was loaded", who, (long long)bad);
    return hg_set_database_pq(c, codes.data(), host_books, host_labels, N, M, K, dsub, C, idx_base, n_total, bad_codes, bad_labels);
}

}  // extern "C"

int preload_pq_encode() {   // (hg_preload: see preload_seq)
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_pq_encode<8>)));
    return HG_OK;
}

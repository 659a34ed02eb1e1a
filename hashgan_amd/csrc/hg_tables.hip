// libhashgan_amd.so -- the table loaders (see hg_ctx.hpp for the map of the translation units).  Every loader is four steps: validate (a refused
// call leaves the context as it was), drop the stage (begin_database_load / begin_query_load: a load that fails from here on leaves a context that
// answers HG_ERR_STATE), fill the tables, commit (database_loaded / queries_loaded: they alone set the stage, the float residency and c->bpad).
#include "hg_ctx.hpp"
#include "hg_host_pack.hpp"
#include "hg_dev_in.hpp"

#include <exception>
#include <thread>

// hg_set_queries: dst_a[i] = src_a[(i / dw) * sw + i % dw] (packed code rows: the unused upper half of an odd row's last 64-bit word is dropped),
// dst_b[j] = src_b[j] (label words) -- sources in pinned host memory
static __global__ __launch_bounds__(256) void k_copy_in(const u32* __restrict__ src_a, u32* __restrict__ dst_a, const i64 na, const int sw, const int dw,
                                                        const u32* __restrict__ src_b, u32* __restrict__ dst_b, const i64 nb) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < na) { const i64 r = i / dw; dst_a[i] = src_a[r * sw + (i - r * dw)]; }
    else if (i - na < nb) dst_b[i - na] = src_b[i - na];
}

namespace {
// What a database load is asked to hold: `rows` rows of b-bit codes and C classes, rows [idx_base, idx_base + rows) of n_total.
struct TableShape { i64 rows; int b, C; i64 idx_base, n_total; int NW() const { return (b + 31) / 32; } int LW() const { return (C + 63) / 64; } };

// Where a load goes: the packed codes and label words, the float table, the census of the features.
struct TableDst { DevBuf& codes; DevBuf& labels; DevBuf& feats; i64 (&census)[3]; };
TableDst database_dst(hg_ctx* c) { return {c->db, c->dblab, c->from_floats.rows, c->census_db}; }
TableDst queries_dst(hg_ctx* c) { return {c->qc, c->qlab, c->qf, c->census_q}; }

// Does the float table follow the packed one to the GPU (the values of option keep_floats)?
enum class Floats { NEVER = 0, ALWAYS = 1, UNLESS_PM1 = 2 };   // UNLESS_PM1: iff the features are no +-1 code
// the query table is small: its floats follow whenever the database's are there (the inner-product ranking needs both) --
// or the caller asks for them (option keep_query_floats: the asymmetric ranking needs the queries' alone)
Floats query_floats(const hg_ctx* c) { return c->from_floats.rows_valid || c->opt.keep_query_floats ? Floats::ALWAYS : Floats::NEVER; }

struct Packed {                        // what a packer hands back (rc != HG_OK: nothing else counts; floats: the float table is resident in TableDst::feats)
    int rc = HG_OK; bool floats = false; i64 bad_codes = 0, bad_labels = 0;
    Packed(int rc_) : rc(rc_) {}       // (what HG_TRY / HG_HIP / fail return)
    Packed(bool f, i64 bc, i64 bl) : floats(f), bad_codes(bc), bad_labels(bl) {}
};
Packed packed(const TableDst& d, bool floats, i64 nonbinary, i64 bad_labels, i64 zeros, i64 minus_ones) {
    d.census[0] = nonbinary; d.census[1] = zeros; d.census[2] = minus_ones;
    return Packed(floats, nonbinary, bad_labels);
}
void report_bad(const Packed& p, int64_t* bad_codes, int64_t* bad_labels) {
    if (bad_codes) *bad_codes = (int64_t)p.bad_codes;
    if (bad_labels) *bad_labels = (int64_t)p.bad_labels;
}

int check_database_shape(const char* who, const TableShape& s, bool have_data) {
    if (s.rows < 1 || !have_data) return fail(HG_ERR_ARG, "%s: need N >= 1 and data", who);
    if (s.b < 1 || s.b > HG_MAX_BITS) return fail(HG_ERR_ARG, "%s: b=%d outside 1..%d", who, s.b, HG_MAX_BITS);
    if (s.C < 1) return fail(HG_ERR_ARG, "%s: C=%d", who, s.C);
    if (s.idx_base < 0 || s.n_total < s.rows || s.idx_base + s.rows > s.n_total || s.n_total >= 0xFFFFFFFFll)
        return fail(HG_ERR_ARG, "%s: shard [%lld, %lld) does not fit a database of %lld rows (< 2^32 - 1)", who,
                    (long long)s.idx_base, (long long)(s.idx_base + s.rows), (long long)s.n_total);
    return HG_OK;
}
int check_query_rows(const char* who, i64 Q, bool have_data) {
    if (Q < 1 || !have_data) return fail(HG_ERR_ARG, "%s: need Q >= 1 and data", who);
    if (Q > 0x7FFFFFC0ll) return fail(HG_ERR_ARG, "%s: Q too large", who);
    return HG_OK;
}

// A validated database load starts: no tables until database_loaded (queries must be set again after it: b, C may change).
void begin_database_load(hg_ctx* c, const TableShape& s) {
    c->stage = ST_NONE;
    c->from_pq.forget_tables();                        // (hg_set_database_pq loads its own behind this)
    c->N = s.rows; c->b = s.b; c->C = s.C; c->n_total = s.n_total;
    c->NW = s.NW(); c->NB = s.b + 1; c->LW = s.LW();
    c->idx_base = (u32)s.idx_base;
}
// What a successful load of the database ends with: everything derived from the old tables is invalid, earlier lost bets say nothing
// about the new one.  floats: from_floats.rows holds the table as loaded (c->bpad: its row pitch; 0 without it).
void database_loaded(hg_ctx* c, bool floats) {
    c->from_floats.rows_valid = floats;
    c->bpad = floats ? pad16(c->b) : 0;
    c->stage = ST_DB;
    c->dbx_valid = c->dbx3_valid = c->dbx4_valid = c->dbx8_valid = false;
    c->forget_rows();
    c->bet_consecutive_fail = c->shard_bet_fail = 0;
    c->cap_boost = c->real_cap_boost = 1;
    c->crowd_probed = false;
    c->cfg_epoch++;
    c->db_gen++;
}

// A new query table of the SAME size on an unchanged database and configuration keeps hg_map_begin's licence to enqueue blind:
// every buffer of the step is sized by Q, nothing about the bet depends on what the queries are (its verdict is checked on the
// GPU either way), so a caller that hands over batch after batch keeps two steps in flight.
void queries_replaced(hg_ctx* c, bool carry) {
    c->cfg_epoch++;
    c->q_gen++;
    if (carry) c->map_warm_cfg = c->cfg_epoch;
}
// A validated query load starts: the database stays, no queries until queries_loaded.  -> the licence carries over (nothing before the commit changes its terms)
bool begin_query_load(hg_ctx* c, i64 Q) {
    const bool carry = (c->stage & ST_Q) && c->Q == Q && c->map_warm_R >= 0 && c->map_warm_cfg == c->cfg_epoch;
    c->stage = ST_DB;
    c->Q = Q;
    return carry;
}
// ... and ends.  floats: qf holds the queries' float table (without it c->bpad stays what the database's commit made it).
void queries_loaded(hg_ctx* c, bool carry, bool floats) {
    c->stage = ST_DB | ST_Q;
    c->qx_valid = false;
    c->qf_resident = floats;
    if (floats) c->bpad = pad16(c->b);
    queries_replaced(c, carry);
}

// The pinned block packed rows are staged in, grown to cb bytes of codes and lbytes of label words (64-byte aligned).
struct PackedStaging { u32* codes; u64* labels; };
int packed_staging(hg_ctx* c, size_t cb, size_t lbytes, PackedStaging* out) {
    const size_t off = (cb + 63) & ~(size_t)63;
    if (c->hpk_cap < off + lbytes) HG_TRY(c->sync());  // (uploads out of the old block)
    HG_HIP(pin_grow(&c->hpk, &c->hpk_cap, off + lbytes));
    *out = {(u32*)c->hpk, (u64*)((char*)c->hpk + off)};
    return HG_OK;
}

// Upload packed uint64 codes as dense uint32 [n][NW] (NW = ceil(b/32)): when NW is
// odd the unused high half of the last uint64 word is dropped by a strided copy.
int upload_codes(hg_ctx* c, DevBuf& dst, const uint64_t* host, i64 n, int W, int NW) {
    HG_TRY(dst.reserve((size_t)n * NW * 4 + 64 * 4));  // +64 words: scalar loads may read past a ragged tail
    if (NW == 2 * W) {
        HG_HIP(hipMemcpyAsync(dst.p, host, (size_t)n * NW * 4, hipMemcpyHostToDevice, c->stream));
    } else {
        HG_HIP(hipMemcpy2DAsync(dst.p, (size_t)NW * 4, host, (size_t)W * 8, (size_t)NW * 4, (size_t)n,
                                hipMemcpyHostToDevice, c->stream));
    }
    return HG_OK;
}

// float32 features + int64 labels -> packed device tables, packed ON THE GPU (k_pack_sign_f32 / k_pack_labels_i64)
Packed pack_on_device(hg_ctx* c, const float* x, const int64_t* lab, i64 n, const TableDst& d) {
    const int b = c->b, C = c->C, NW = c->NW, LW = c->LW;
    // the float table stays resident, zero-padded to a multiple of 16 features: the real-valued
    // ranking (hg_map_real) streams it, and padding keeps its rows 64-byte aligned
    const int bpad = pad16(b);
    const size_t fb = (size_t)n * bpad * 4, lb = (size_t)n * C * 8;
    HG_TRY(d.feats.reserve(fb + 256));
    HG_TRY(c->stage_in.reserve(lb));
    HG_TRY(c->badcnt.reserve(32));
    HG_TRY(d.codes.reserve((size_t)n * NW * 4 + 64 * 4));
    HG_TRY(d.labels.reserve((size_t)n * LW * 8));
    HG_HIP(hipMemsetAsync(c->badcnt.p, 0, 32, c->stream));
    if (bpad != b) HG_HIP(hipMemsetAsync(d.feats.p, 0, fb, c->stream));
    HG_HIP(hipMemcpy2DAsync(d.feats.p, (size_t)bpad * 4, x, (size_t)b * 4, (size_t)b * 4, (size_t)n, hipMemcpyHostToDevice, c->stream));
    c->t_begin(KI_PACK);
    hipLaunchKernelGGL(k_pack_sign_f32, dim3(grid_for(n, WPB)), dim3(256), 0, c->stream, d.feats.as<float>(), (i64)bpad,
                       d.codes.as<u32>(), n, b, NW, c->badcnt.as<unsigned long long>());
    c->t_end();
    HG_TRY(c->check_launch("k_pack_sign_f32"));
    HG_HIP(hipMemcpyAsync(c->stage_in.p, lab, lb, hipMemcpyHostToDevice, c->stream));
    c->t_begin(KI_PACK);
    hipLaunchKernelGGL(k_pack_labels_i64, dim3(grid_for(n, WPB)), dim3(256), 0, c->stream, c->stage_in.as<long long>(),
                       d.labels.as<u64>(), n, C, LW, c->badcnt.as<unsigned long long>());
    c->t_end();
    HG_TRY(c->check_launch("k_pack_labels_i64"));
    unsigned long long bad[4] = {0, 0, 0, 0};
    HG_HIP(hipMemcpyAsync(bad, c->badcnt.p, 32, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    return packed(d, true, (i64)bad[0], (i64)bad[1], (i64)bad[2], (i64)bad[3]);
}

// A big float table (256 MB at 1M x 64) on its way to the GPU: the runtime stages a pageable source at ~25 GB/s.  Host
// threads copy 16 MB chunks (rows padded on the way) into four pinned buffers instead, each chunk's DMA runs while the next
// is copied.  Enqueues on `stream`; which_pool: the host pool that copies (1 while pool 0 packs).
constexpr int NSL = 4;
constexpr size_t CH = (size_t)16 << 20;
int ensure_fstage(hg_ctx* c) {
    if (c->fstage) return HG_OK;
    HG_HIP(pin_alloc(&c->fstage, CH * NSL, &c->fstage_cap));
    for (int k = 0; k < NSL; ++k) HG_HIP(hipEventCreateWithFlags(&c->fstage_ev[k], hipEventDisableTiming));
    return HG_OK;
}
int ensure_stream2(hg_ctx* c) {
    if (!c->stream2) HG_TRY(stream_create(c->device, &c->stream2));
    if (!c->stream2_ev) HG_HIP(hipEventCreateWithFlags(&c->stream2_ev, hipEventDisableTiming));
    return HG_OK;
}
int stage_floats(hg_ctx* c, const float* x, i64 n, int b, int bpad, DevBuf& feats, hipStream_t stream, int which_pool) {
    HG_TRY(ensure_fstage(c));
    const i64 rows_per = (i64)(CH / ((size_t)bpad * 4));
    int slot = 0;
    bool used[NSL] = {false, false, false, false};
    try {
        for (i64 r0 = 0; r0 < n; r0 += rows_per, slot = (slot + 1) % NSL) {
            const i64 r1 = r0 + rows_per < n ? r0 + rows_per : n;
            if (used[slot]) HG_HIP(hipEventSynchronize(c->fstage_ev[slot]));
            float* st = (float*)((char*)c->fstage + (size_t)slot * CH);
            host_copy_rows(x, r0, r1, b, bpad, st, 0, which_pool);
            HG_HIP(hipMemcpyAsync((char*)feats.p + (size_t)r0 * bpad * 4, st, (size_t)(r1 - r0) * bpad * 4, hipMemcpyHostToDevice, stream));
            HG_HIP(hipEventRecord(c->fstage_ev[slot], stream));
            used[slot] = true;
        }
    } catch (const std::exception& e) {
        return fail(HG_ERR_NOMEM, "host-side staging of the float table failed: %s", e.what());
    }
    return HG_OK;
}

// The same hand-over with the packing done by host threads BEFORE the upload (hg_host_pack.hpp): 16 MB instead of 339 MB
// cross PCIe at C2.  The float table follows only when somebody will rank by inner product (`floats`).
Packed pack_on_host(hg_ctx* c, const float* x, const int64_t* lab, i64 n, const TableDst& d, Floats floats) {
    const int b = c->b, C = c->C, NW = c->NW, LW = c->LW;
    const size_t cb = (size_t)n * NW * 4, lbytes = (size_t)n * LW * 8;
    PackedStaging h;
    HG_TRY(packed_staging(c, cb, lbytes, &h));
    HostPackCensus cs;
    HG_TRY(d.codes.reserve(cb + 64 * 4));
    HG_TRY(d.labels.reserve(lbytes));
    // the packed rows cross PCIe while the host threads still pack the rest: the calling thread ships every finished
    // prefix (a quarter of a big table at a time), the workers claim row ranges in ascending order
    i64 shipped = 0;
    hipError_t ship_err = hipSuccess;
    const i64 piece = n >= (1 << 18) ? (n + 3) / 4 : n;
    auto ship = [&](long long rows_done) {
        if (rows_done < n && rows_done - shipped < piece) return;
        if (rows_done <= shipped || ship_err != hipSuccess) return;
        hipError_t e = hipMemcpyAsync((char*)d.codes.p + (size_t)shipped * NW * 4, (const char*)h.codes + (size_t)shipped * NW * 4,
                                      (size_t)(rows_done - shipped) * NW * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync((char*)d.labels.p + (size_t)shipped * LW * 8, (const char*)h.labels + (size_t)shipped * LW * 8,
                               (size_t)(rows_done - shipped) * LW * 8, hipMemcpyHostToDevice, c->stream);
        ship_err = e;
        shipped = rows_done;
    };
    // Will the float table follow?  ALWAYS: yes; UNLESS_PM1: only if the features are no +-1 code -- and a single entry
    // that is neither -1 nor +1 among the first rows settles that before the census is in (tanh outputs: the first entry).
    // Then a second thread stages and ships the floats (its own small pool, its own stream) WHILE the packing pool works.
    const int bpad = pad16(b);
    const size_t fb = (size_t)n * bpad * 4;
    bool early = false;
    if (x && floats != Floats::NEVER && fb >= ((size_t)8 << 20)) {
        early = floats == Floats::ALWAYS;
        const i64 probe = (i64)std::min<i64>(n, 64) * b;
        for (i64 k = 0; k < probe && !early; ++k) early = !(x[k] == 1.0f || x[k] == -1.0f);
    }
    int stage_rc = HG_OK;
    std::string stage_msg;                               // (the error text is thread-local: carried over by hand)
    std::thread stager;
    if (early) {
        HG_TRY(ensure_stream2(c));
        HG_TRY(d.feats.reserve(fb + 256));
        try {
            HostTimer t_thr(HP_THREAD);                  // ("thread": starting the staging thread)
            stager = std::thread([&] {
                if (hipSetDevice(c->device) != hipSuccess) { stage_rc = HG_ERR_HIP; stage_msg = "hipSetDevice failed in the staging thread"; return; }
                stage_rc = stage_floats(c, x, n, b, bpad, d.feats, c->stream2, 1);
                if (stage_rc != HG_OK) stage_msg = g_err;
            });
        } catch (const std::exception&) {
            early = false;                               // no second thread to be had: the floats follow the packing
        }
    }
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{stager};
    try {
        HostTimer t_pack(HP_PACK);                       // ("pack": the packing pool's pass over the arrays, prefixes shipped meanwhile)
        host_pack_ship(x, lab, n, b, C, h.codes, h.labels, &cs, 0,
                       +[](void* f, long long rows) { (*static_cast<decltype(ship)*>(f))(rows); }, &ship);
    } catch (const std::exception& e) {               // no exception crosses the C ABI (thread creation can fail)
        return fail(HG_ERR_NOMEM, "host-side packing failed: %s", e.what());
    }
    if (ship_err != hipSuccess) return fail(HG_ERR_HIP, "upload of the packed tables failed: %s", hipGetErrorString(ship_err));
    const bool pm1 = cs.nonbinary == 0 && cs.zeros == 0;
    const bool up = floats == Floats::ALWAYS || (floats == Floats::UNLESS_PM1 && !pm1);
    if (stager.joinable()) stager.join();
    if (early) {
        if (stage_rc != HG_OK) return fail(stage_rc, "%s", stage_msg.c_str());
        HG_HIP(hipEventRecord(c->stream2_ev, c->stream2));
        HG_HIP(hipStreamWaitEvent(c->stream, c->stream2_ev, 0));
    }
    if (up && !early) {
        HG_TRY(d.feats.reserve(fb + 256));
        if (fb >= ((size_t)8 << 20)) {
            HG_TRY(stage_floats(c, x, n, b, bpad, d.feats, c->stream, 0));
        } else {
            if (bpad != b) HG_HIP(hipMemsetAsync(d.feats.p, 0, fb, c->stream));
            HG_HIP(hipMemcpy2DAsync(d.feats.p, (size_t)bpad * 4, x, (size_t)b * 4, (size_t)b * 4, (size_t)n, hipMemcpyHostToDevice, c->stream));
        }
    }
    HG_TRY(c->sync());                                 // the pinned staging is reused by the next call
    return packed(d, up, cs.nonbinary, cs.bad_labels, cs.zeros, cs.minus_ones);
}

int check_dev_arrays(hg_ctx* c, const char* who, const hg_dev_array* f, const hg_dev_array* l, int64_t max_rows, int want_b, int want_C) {
    char msg[256];
    int64_t fb = 0, lb = 0;
    if (hg_dev::check_pair(f, l, HG_MAX_BITS, max_rows, want_b, want_C, &fb, &lb, msg, sizeof msg)) return fail(HG_ERR_ARG, "%s: %s", who, msg);
    HG_TRY(check_dev_pointer(c, who, "features", *f, fb));
    return check_dev_pointer(c, who, "labels", *l, lb);
}

// Device arrays -> packed device tables (+ the float table: `floats`, UNLESS_PM1 by the census).  Everything here was validated by check_dev_arrays.
Packed pack_from_device(hg_ctx* c, const hg_dev_array& f, const hg_dev_array& l, const TableDst& d, Floats floats) {
    const i64 n = f.rows;
    const int bpad = pad16(c->b);
    const size_t fb = (size_t)n * bpad * 4;
    const bool first_pass = floats == Floats::ALWAYS;  // the floats leave with the codes, from one read of the caller's rows
    HG_TRY(c->badcnt.reserve(32));
    HG_TRY(d.codes.reserve((size_t)n * c->NW * 4 + 64 * 4));
    HG_TRY(d.labels.reserve((size_t)n * c->LW * 8));
    if (first_pass) HG_TRY(d.feats.reserve(fb + 256));
    HG_TRY(wait_for_producer(c, f.stream));
    if (l.stream != f.stream) HG_TRY(wait_for_producer(c, l.stream));
    HG_HIP(hipMemsetAsync(c->badcnt.p, 0, 32, c->stream));
    HG_TRY(launch_pack_dev(c, f, d.codes.as<u32>(), first_pass ? d.feats.as<float>() : nullptr, bpad));
    HG_TRY(launch_pack_labels_dev(c, l, d.labels.as<u64>()));
    unsigned long long bad[4] = {0, 0, 0, 0};
    HG_HIP(hipMemcpyAsync(bad, c->badcnt.p, 32, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    const bool pm1 = bad[0] == 0 && bad[2] == 0;
    const bool up = first_pass || (floats == Floats::UNLESS_PM1 && !pm1);
    if (up && !first_pass) {                           // the census asked for the floats: a second pass over the caller's memory
        HG_TRY(d.feats.reserve(fb + 256));
        HG_TRY(launch_pack_dev(c, f, nullptr, d.feats.as<float>(), bpad));
        HG_TRY(c->sync());
    }
    return packed(d, up, (i64)bad[0], (i64)bad[1], (i64)bad[2], (i64)bad[3]);
}

// The codebook pass of hg_set_database_pq.  scan(), per codeword: finite?  its sign pattern (PW words), its census (entries outside {-1, 0, +1}; zeros; minus ones), its norm^2 in float64.
// fold(), once the rows' codes are counted (used[m][k]): the decoded table's census, and xmax2 >= every row's norm^2 -- the sum over the subspaces of the largest norm^2 among the codewords that occur, rounded up.
struct PqBooks {
    int M, K, dsub, PW;
    std::vector<u32> pat;
    std::vector<i64> census;
    std::vector<double> norm;
    int scan(const float* books) {
        const size_t ncw = (size_t)M * K;
        try { pat.assign(ncw * PW, 0u); census.assign(ncw * 3, 0); norm.assign(ncw, 0.0); }
        catch (const std::exception& e) { return fail(HG_ERR_NOMEM, "hg_set_database_pq: %s", e.what()); }
        for (size_t w = 0; w < ncw; ++w) {
            const float* cw = books + w * dsub;
            for (int j = 0; j < dsub; ++j) {
                const float f = cw[j];
                if (!std::isfinite(f))
                    return fail(HG_ERR_ARG, "hg_set_database_pq: codebook entry [%d][%d][%d] is not finite", (int)(w / K), (int)(w % K), j);
                pat[w * PW + (j >> 5)] |= (u32)(f > 0.0f) << (j & 31);
                census[w * 3 + 0] += !(f == 1.0f || f == -1.0f || f == 0.0f);
                census[w * 3 + 1] += f == 0.0f;
                census[w * 3 + 2] += f == -1.0f;
                norm[w] += (double)f * (double)f;
            }
        }
        return HG_OK;
    }
    float fold(const std::vector<long long>& used, i64 (&table_census)[3]) const {
        double bound = 0.0;
        for (int m = 0; m < M; ++m) {
            double mx = 0.0;
            for (int k = 0; k < K; ++k) {
                const size_t w = (size_t)m * K + k;
                const i64 n = used[w];
                if (!n) continue;
                for (int e = 0; e < 3; ++e) table_census[e] += n * census[w * 3 + e];
                if (norm[w] > mx) mx = norm[w];
            }
            bound += mx;
        }
        float xmax2 = (float)bound;
        if ((double)xmax2 < bound) xmax2 = std::nextafterf(xmax2, INFINITY);
        return xmax2;
    }
};
}  // namespace

// hg_preload: the staging blocks, the second stream and the packing pools' threads now; and this unit's code object (see preload_seq)
int preload_tables(hg_ctx* c) {
    HG_TRY(ensure_stream2(c));
    HG_TRY(ensure_fstage(c));
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_copy_in)));
    host_pack_warm();
    return HG_OK;
}

extern "C" {

int hg_pack_sign_f32(const float* x, int64_t n, int b, uint64_t* out) {
    if (!x || !out || n < 0 || b < 1) return fail(HG_ERR_ARG, "hg_pack_sign_f32: bad argument");
    const int W = (b + 63) / 64;
    for (int64_t i = 0; i < n; ++i) {
        const float* row = x + i * b;
        for (int w = 0; w < W; ++w) {
            uint64_t v = 0;
            const int hi = b - w * 64 < 64 ? b - w * 64 : 64;
            for (int j = 0; j < hi; ++j) v |= (uint64_t)(row[w * 64 + j] > 0.0f) << j;
            out[i * W + w] = v;
        }
    }
    return HG_OK;
}

int hg_set_database(hg_ctx* c, const uint64_t* codes, const uint64_t* labels, int64_t N, int b, int C,
                    int64_t idx_base, int64_t n_total) {
    if (!c) return fail(HG_ERR_ARG, "hg_set_database: null context");
    const TableShape s{N, b, C, idx_base, n_total};
    HG_TRY(check_database_shape("hg_set_database", s, codes && labels));
    HG_TRY(c->use());
    begin_database_load(c, s);
    HG_TRY(upload_codes(c, c->db, codes, N, (b + 63) / 64, c->NW));
    HG_TRY(c->dblab.reserve((size_t)N * c->LW * 8));
    HG_HIP(hipMemcpyAsync(c->dblab.p, labels, (size_t)N * c->LW * 8, hipMemcpyHostToDevice, c->stream));
    HG_TRY(c->sync());
    database_loaded(c, false);                         // packed input: no float table for the real-valued path
    return HG_OK;
}

int hg_set_database_f32(hg_ctx* c, const float* host_x, const int64_t* host_labels, int64_t N, int b, int C,
                        int64_t idx_base, int64_t n_total, int64_t* bad_codes, int64_t* bad_labels) {
    if (!c) return fail(HG_ERR_ARG, "hg_set_database_f32: null context");
    const TableShape s{N, b, C, idx_base, n_total};
    HG_TRY(check_database_shape("hg_set_database_f32", s, host_x && host_labels));
    HG_TRY(c->use());
    begin_database_load(c, s);
    const Packed p = c->opt.host_pack ? pack_on_host(c, host_x, host_labels, N, database_dst(c), (Floats)c->opt.keep_floats)
                                      : pack_on_device(c, host_x, host_labels, N, database_dst(c));
    HG_TRY(p.rc);
    database_loaded(c, p.floats);
    report_bad(p, bad_codes, bad_labels);
    return HG_OK;
}

// Product-quantisation codes u8 [N][M], codebooks f32 [M][K][dsub], labels int64 [N][C] (hg_pq.hpp).  The context ends up as
// hg_set_database_f32 leaves it for the decoded table under keep_floats = 0, plus the PQ tables in from_pq.  The sign codes come from
// per-codeword sign patterns (dsub bits each, computed once) that host threads OR into the rows' words -- the same pool, the same pinned
// staging and the same uploads as pack_on_host; the one pass over the codes also checks every byte against K, counts how often each
// codeword occurs (the census of the decoded table; which codewords bound the rows' norm) -- no N x b floats anywhere.
int hg_set_database_pq(hg_ctx* c, const uint8_t* host_codes, const float* host_books, const int64_t* host_labels, int64_t N, int M, int K,
                       int dsub, int C, int64_t idx_base, int64_t n_total, int64_t* bad_codes, int64_t* bad_labels) {
    if (!c) return fail(HG_ERR_ARG, "hg_set_database_pq: null context");
    if (M < 1) return fail(HG_ERR_ARG, "hg_set_database_pq: M=%d subspaces (need >= 1)", M);
    if (K < 1 || K > 256) return fail(HG_ERR_ARG, "hg_set_database_pq: K=%d codewords outside 1..256", K);
    if (dsub < 1) return fail(HG_ERR_ARG, "hg_set_database_pq: dsub=%d features per subspace (need >= 1)", dsub);
    if ((i64)M * dsub > HG_MAX_BITS) return fail(HG_ERR_ARG, "hg_set_database_pq: M * dsub = %lld features, more than %d", (long long)M * dsub, HG_MAX_BITS);
    if (idx_base != 0 || n_total != N) return fail(HG_ERR_ARG, "hg_set_database_pq: one shard only (idx_base=%lld, n_total=%lld for N=%lld rows)",
                                                    (long long)idx_base, (long long)n_total, (long long)N);
    if (N >= 0xFFFFFFFFll) return fail(HG_ERR_ARG, "hg_set_database_pq: N=%lld rows (need < 2^32 - 1)", (long long)N);
    const TableShape s{N, M * dsub, C, idx_base, n_total};
    HG_TRY(check_database_shape("hg_set_database_pq", s, host_codes && host_books && host_labels));
    PqBooks books{M, K, dsub, (dsub + 31) / 32};
    HG_TRY(books.scan(host_books));
    HG_TRY(c->use());
    const int b = s.b, NW = s.NW(), LW = s.LW();
    const size_t cb = (size_t)N * NW * 4, lbytes = (size_t)N * LW * 8, ncw = (size_t)M * K;
    PackedStaging h;
    HG_TRY(packed_staging(c, cb, lbytes, &h));
    HostPackCensus cs;
    std::vector<long long> used;
    HostPqScan scan;
    try {
        HostTimer t_pack(HP_PACK);
        used.assign(ncw, 0);
        host_pack(nullptr, host_labels, N, b, C, nullptr, h.labels, &cs, 0);
        host_pq_sign(host_codes, N, M, K, dsub, books.pat.data(), books.PW, h.codes, NW, used.data(), &scan, 0);
    } catch (const std::exception& e) {               // no exception crosses the C ABI
        return fail(HG_ERR_NOMEM, "hg_set_database_pq: host-side packing failed: %s", e.what());
    }
    if (scan.bad_row >= 0)
        return fail(HG_ERR_ARG, "hg_set_database_pq: code byte %d at row %lld, subspace %d is not below K=%d", scan.bad_code, (long long)scan.bad_row, scan.bad_m, K);
    i64 census[3] = {0, 0, 0};
    const float xmax2 = books.fold(used, census);
    // upload: the packed tables (what hg_set_database_f32 sets for the decoded table, no float table), then the PQ tables
    begin_database_load(c, s);
    HG_TRY(c->db.reserve(cb + 64 * 4));
    HG_TRY(c->dblab.reserve(lbytes));
    HG_HIP(hipMemcpyAsync(c->db.p, h.codes, cb, hipMemcpyHostToDevice, c->stream));
    HG_HIP(hipMemcpyAsync(c->dblab.p, h.labels, lbytes, hipMemcpyHostToDevice, c->stream));
    RowSource& src = c->from_pq;
    const int MP = (M + 3) / 4 * 4;
    HG_TRY(src.pq_codes.reserve((size_t)N * MP + 64));
    HG_TRY(src.pq_books.reserve(ncw * dsub * 4 + 64));
    if (MP == M) {
        HG_HIP(hipMemcpyAsync(src.pq_codes.p, host_codes, (size_t)N * M, hipMemcpyHostToDevice, c->stream));
    } else {
        HG_HIP(hipMemsetAsync(src.pq_codes.p, 0, (size_t)N * MP, c->stream));
        HG_HIP(hipMemcpy2DAsync(src.pq_codes.p, (size_t)MP, host_codes, (size_t)M, (size_t)M, (size_t)N, hipMemcpyHostToDevice, c->stream));
    }
    HG_HIP(hipMemcpyAsync(src.pq_books.p, host_books, ncw * dsub * 4, hipMemcpyHostToDevice, c->stream));
    HG_TRY(c->sync());                                 // the pinned staging and the caller's arrays are free again
    database_loaded(c, false);
    src.pq_M = M; src.pq_K = K; src.pq_dsub = dsub; src.pq_MP = MP;
    src.pq_xmax2 = xmax2;
    src.pq_valid = true;
    report_bad(packed(database_dst(c), false, census[0], cs.bad_labels, census[1], census[2]), bad_codes, bad_labels);
    return HG_OK;
}

// ---- features and labels in DEVICE memory (hg_dev_in.hpp: the kernels; hg_dev_desc.hpp: the descriptor arithmetic) ----
// Is a.ptr device memory of the context's GPU, and does the array's extent lie inside its allocation?  Asked of the runtime
// before anything is launched: a pointer it does not know comes back as HG_ERR_ARG, never as a fault.
int check_dev_pointer(hg_ctx* c, const char* who, const char* what, const hg_dev_array& a, int64_t extent) {
    hipPointerAttribute_t at{};
    hipError_t e = hipPointerGetAttributes(&at, a.ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();                       // (not a launch failure: leave nothing for check_launch to find)
        return fail(HG_ERR_ARG, "%s: the %s pointer %p is not known to the HIP runtime (%s)", who, what, a.ptr, hipGetErrorString(e));
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged)
        return fail(HG_ERR_ARG, "%s: the %s pointer %p is not plain device memory (host, managed or unregistered memory)", who, what, a.ptr);
    if (at.device != c->device)
        return fail(HG_ERR_ARG, "%s: the %s lie on device %d, the context runs on device %d", who, what, at.device, c->device);
    void* base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)a.ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(HG_ERR_ARG, "%s: no allocation found around the %s pointer %p (%s)", who, what, a.ptr, hipGetErrorString(e));
    }
    if (!hg_dev::inside(a.ptr, extent, base, size))
        return fail(HG_ERR_ARG, "%s: the %s span %lld bytes from %p, the allocation ends %lld bytes from there", who, what, (long long)extent,
                    a.ptr, (long long)((const char*)base + size - (const char*)a.ptr));
    return HG_OK;
}

// The context's stream behind whatever the producer has enqueued so far on `s` (NULL: the null stream)
int wait_for_producer(hg_ctx* c, void* s) {
    if ((hipStream_t)s == c->stream) return HG_OK;
    hipEvent_t ev = c->get_event();
    if (!ev) return fail(HG_ERR_HIP, "hipEventCreate failed");
    hipError_t e = hipEventRecord(ev, (hipStream_t)s);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
    c->pool.push_back(ev);                             // (the wait is enqueued: the event may be recorded again)
    HG_HIP(e);
    return HG_OK;
}

int hg_set_database_dev(hg_ctx* c, const hg_dev_array* features, const hg_dev_array* labels, int64_t idx_base, int64_t n_total,
                        int64_t* bad_codes, int64_t* bad_labels) {
    if (!c) return fail(HG_ERR_ARG, "hg_set_database_dev: null context");
    HG_TRY(c->use());
    HG_TRY(check_dev_arrays(c, "hg_set_database_dev", features, labels, 0xFFFFFFFEll, 0, 0));
    const TableShape s{features->rows, (int)features->cols, (int)labels->cols, idx_base, n_total};
    HG_TRY(check_database_shape("hg_set_database_dev", s, true));
    begin_database_load(c, s);
    const Packed p = pack_from_device(c, *features, *labels, database_dst(c), (Floats)c->opt.keep_floats);
    HG_TRY(p.rc);
    database_loaded(c, p.floats);
    report_bad(p, bad_codes, bad_labels);
    return HG_OK;
}

int hg_set_queries(hg_ctx* c, const uint64_t* codes, const uint64_t* labels, int64_t Q) {
    HG_TRY(need(c, ST_DB, "hg_set_queries", "hg_set_database"));
    HG_TRY(check_query_rows("hg_set_queries", Q, codes && labels));
    const bool carry = begin_query_load(c, Q);
    // through a pinned block of the context's own (two, alternating), copied from there by the stream: the call returns without
    // waiting for whatever the stream still holds -- a step of hg_map_begin on the previous batch -- and the caller's arrays
    // are free the moment it does
    const int W = (c->b + 63) / 64;
    const size_t cb = (size_t)Q * W * 8, lb = (size_t)Q * c->LW * 8;
    hg_ctx::QStage& qs = c->qstage[c->qstage_next];
    c->qstage_next ^= 1;
    if (qs.used) HG_HIP(hipEventSynchronize(qs.ev));   // (the copy out of this block two loads ago)
    HG_HIP(pin_grow(&qs.pin, &qs.cap, cb + lb));
    if (!qs.ev) HG_HIP(hipEventCreateWithFlags(&qs.ev, hipEventDisableTiming));
    memcpy(qs.pin, codes, cb);
    memcpy((char*)qs.pin + cb, labels, lb);
    HG_TRY(c->qc.reserve((size_t)Q * c->NW * 4 + 64 * 4));
    HG_TRY(c->qlab.reserve(lb));
    // fetched by a KERNEL out of the pinned block (it is device-addressable: loads over the link), like k_copy_out the other way: a
    // copy-engine transfer of these 160 KB sits ~20 us on the stream behind a cross-queue barrier -- per step, for a caller that hands
    // over a new batch per step (a small table only: a big one is the copy engines' work)
    if (cb + lb <= ((size_t)4 << 20)) {
        const i64 nc = (i64)Q * c->NW, nl = (i64)Q * c->LW * 2;
        hipLaunchKernelGGL(k_copy_in, dim3(grid_for(nc + nl)), dim3(256), 0, c->stream, (const u32*)qs.pin, c->qc.as<u32>(), nc, 2 * W, c->NW,
                           (const u32*)((const char*)qs.pin + cb), c->qlab.as<u32>(), nl);
        HG_TRY(c->check_launch("k_copy_in"));
    } else {
        HG_TRY(upload_codes(c, c->qc, (const uint64_t*)qs.pin, Q, W, c->NW));
        HG_HIP(hipMemcpyAsync(c->qlab.p, (const char*)qs.pin + cb, lb, hipMemcpyHostToDevice, c->stream));
    }
    HG_HIP(hipEventRecord(qs.ev, c->stream));
    qs.used = true;
    queries_loaded(c, carry, false);                     // packed input: no float table
    return HG_OK;
}

int hg_set_queries_f32(hg_ctx* c, const float* host_x, const int64_t* host_labels, int64_t Q, int64_t* bad_codes,
                       int64_t* bad_labels) {
    HG_TRY(need(c, ST_DB, "hg_set_queries_f32", "hg_set_database"));
    HG_TRY(check_query_rows("hg_set_queries_f32", Q, host_x && host_labels));
    const bool carry = begin_query_load(c, Q);
    const Packed p = c->opt.host_pack ? pack_on_host(c, host_x, host_labels, Q, queries_dst(c), query_floats(c))
                                      : pack_on_device(c, host_x, host_labels, Q, queries_dst(c));
    HG_TRY(p.rc);
    queries_loaded(c, carry, p.floats);
    report_bad(p, bad_codes, bad_labels);
    return HG_OK;
}

int hg_set_queries_dev(hg_ctx* c, const hg_dev_array* features, const hg_dev_array* labels, int64_t* bad_codes, int64_t* bad_labels) {
    HG_TRY(need(c, ST_DB, "hg_set_queries_dev", "hg_set_database"));
    HG_TRY(check_dev_arrays(c, "hg_set_queries_dev", features, labels, 0x7FFFFFC0ll, c->b, c->C));
    HG_TRY(check_query_rows("hg_set_queries_dev", features->rows, true));
    const bool carry = begin_query_load(c, features->rows);
    const Packed p = pack_from_device(c, *features, *labels, queries_dst(c), query_floats(c));
    HG_TRY(p.rc);
    queries_loaded(c, carry, p.floats);
    report_bad(p, bad_codes, bad_labels);
    return HG_OK;
}

// packed tables back to the host (tests; also lets a caller keep the packed form)
int hg_get_packed(hg_ctx* c, int which, uint32_t* host_codes, uint64_t* host_labels) {
    HG_TRY(need(c, which ? (ST_DB | ST_Q) : ST_DB, "hg_get_packed", "hg_set_database / hg_set_queries"));
    const i64 n = which ? c->Q : c->N;
    const TableDst t = which ? queries_dst(c) : database_dst(c);
    if (host_codes) HG_HIP(hipMemcpyAsync(host_codes, t.codes.p, (size_t)n * c->NW * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_labels) HG_HIP(hipMemcpyAsync(host_labels, t.labels.p, (size_t)n * c->LW * 8, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

}  // extern "C"

// libhashgan_amd.so -- real-valued (float32 inner product) ranking, what main.py:157,164 feeds lib/metric.py:13-14:
// sampled cut -> bf16 filter on the matrix cores -> exact float32 rescoring -> LDS ranking.
//
// One call is a ladder of attempts (run_real -> real_call -> real_ladder -> real_attempt).  An attempt builds one RealReq and passes it down by
// const reference; what it leaves behind is c->real (RealState), assigned afresh when the attempt begins.
//
// The database's rows come from a RowSource that travels with the call (RealReq::src): run_real picks the context's from_floats (the loaded
// float table), run_asym (hg_topr_asym, hg_map_asym) from_codes (the packed codes read as +-1, hg_asym.hpp), run_pq (hg_topr_pq, hg_map_pq)
// from_pq (product-quantisation codes and codebooks, hg_pq.hpp), and a requery child runs on its parent's.  What differs between the kinds
// -- float rows, 16-bit images, the filter's norm word, the rescore, the rows of the staged sample -- is the section "the row source" below;
// nothing outside it reads RowSource::kind.
#include "hg_ctx.hpp"
#include "hg_real_kernels.hpp"
#include "hg_real_mx.hpp"
#include "hg_real_bf.hpp"
#include "hg_asym.hpp"
#include "hg_pq.hpp"
#include <type_traits>

constexpr double REAL_FIRST_SIGMA = 5.0;        // depth of the first cut in deviations of the sampled count: one query in ~3e5 loses it and is ranked again on its
                                              // own (real_requery_lost).  10k x 1M x 64, R = 5000: 6 -> 5.92 ms per call, 5 -> 5.81, 4 -> 5.86, 3.5 -> 6.01 (the
                                              // rescore's time follows its rounds, not its rows: the shallower cut mostly helps the rank stage)
constexpr i64 REAL_SAMPLE_HITS = 64;          // the real-valued bet samples so that this many of a query's top R rows are in the sample (tools/real_sample_sweep.py: 32 .. 256 measured)
constexpr i64 REAL_SECOND_SAMPLE = 4;         // the second, counting sample expects four times REAL_SAMPLE_HITS of a query's top R rows: 256
constexpr i64 REAL_FIRST_HITS_BRACKET = 24;   // ... and the first sample, when a second one follows, this many (10k x 1M x 64, R = 5000, call: 64 -> 4.86 ms, 48 -> 4.76, 32 -> 4.72,
                                              // 24 -> 4.68, 16 -> 4.65, 12 -> 4.70, 8 -> 4.80 -- below 16 the bins of the second sample no longer reach the cut; 6: lists beyond the LDS)
constexpr i64 REAL_SEG_BYTES = 512 * 1024;    // bytes of feature rows per segment of the real-valued pair passes
constexpr int REAL_MX_QPB = WPB * 32 * RMX_QT;   // queries per block of the float32 MFMA pair passes (k_real_select_mx, k_real_sample_mx)

namespace {
// ---- run-time values as template arguments ----
// f(std::true_type{}) or f(std::false_type{}); nest two for two flags
template <class F> int with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// f(std::integral_constant<int, KP>{}) for KP = c->bpad, the padded feature count, up to the MAXKP (128 or 256) the callee's kernels take
template <int MAXKP, class F> int with_features(const hg_ctx* c, F&& f) {
#define HG_KP(kp) case kp: if constexpr (kp <= MAXKP) return f(std::integral_constant<int, kp>{}); break;
    switch (c->bpad) {
        HG_KP(16) HG_KP(32) HG_KP(48) HG_KP(64) HG_KP(80) HG_KP(96) HG_KP(112) HG_KP(128)
        HG_KP(144) HG_KP(160) HG_KP(176) HG_KP(192) HG_KP(208) HG_KP(224) HG_KP(240) HG_KP(256)
    }
#undef HG_KP
    return fail(HG_ERR_ARG, "real-valued ranking supports up to %d features (have %d)", MAXKP, c->b);
}
// f(std::integral_constant<int, SG>{}) for the slices per wavefront the rescore kernels are built for (rescore_slices_per_wave picks among them;
// a build with -DHG_RS_FORCE=n has that one alone)
template <class F> int with_slices(int SG, F&& f) {
#define HG_SG(sg) case sg: return f(std::integral_constant<int, sg>{});
#ifdef HG_RS_FORCE
    switch (SG) { HG_SG(HG_RS_FORCE) }
#else
    switch (SG) { HG_SG(8) HG_SG(6) HG_SG(4) HG_SG(3) HG_SG(2) HG_SG(1) }
#endif
#undef HG_SG
    return fail(HG_ERR_ARG, "real-valued ranking: no rescore kernel for %d slices per wavefront", SG);
}

// ---- launch geometry ----
inline int seg_pairs(const Geo& g) { return (g.S + 1) / 2; }
// Geo of a (segment pair) x (query block) launch over `rows` rows: about `segs` segments of a multiple of 16 rows (0: the segments of g0),
// blocks of `qpb` queries
Geo pair_geometry(const Geo& g0, i64 rows, int segs, int qpb) {
    Geo g = g0;
    g.N = rows;
    if (segs) {
        const i64 L = ((rows + segs - 1) / segs + 15) / 16 * 16;
        g.L = L;
        g.S = (int)((rows + L - 1) / L);
    }
    g.nQT = (g.Q + qpb - 1) / qpb;
    g.nUnits = (i64)seg_pairs(g) * g.nQT;
    g.wpb = WPB;
    g.nBlk = (int)g.nUnits;
    return g;
}
// the call's geometry (make_geometry: a unit = one segment x 64 queries, WPB units per block) with segments of L rows
void cut_segments(Geo& g, i64 L) {
    g.L = L;
    g.S = (int)((g.N + L - 1) / L);
    g.nUnits = (i64)g.S * g.nQT;
    g.nBlk = (int)((g.nUnits + WPB - 1) / WPB);
}

// ---- the row source (RealReq::src): what the FLOATS, the CODES and the PQ kind do differently, and the only readers of RowSource::kind ----
PqTab pq_tab(const RowSource& s) { return PqTab{s.pq_codes.as<u8>(), s.pq_books.as<float>(), s.pq_M, s.pq_K, s.pq_dsub, s.pq_MP}; }
// `rows` float rows [rows][bpad] of every stride-th database row from the codes (+-1.0) or the PQ tables (decoded), pad features 0
void expand_rows(hg_ctx* c, const RowSource& s, DevBuf& dst, i64 rows, i64 stride) {
    const dim3 grid(grid_for(rows * (c->bpad / 4)));
    if (s.kind == RowSource::PQ)
        hipLaunchKernelGGL(k_pq_expand_rows, grid, dim3(256), 0, c->stream, pq_tab(s), dst.as<float4>(), rows, c->bpad, c->b, stride);
    else
        hipLaunchKernelGGL(k_asym_expand_rows, grid, dim3(256), 0, c->stream, c->db.as<u32>(), dst.as<float4>(), rows, c->bpad, c->NW, c->b, stride);
}
// The database's float rows [N][bpad]: the loaded table; from the codes or the PQ tables, rows expanded into the source's work buffer on
// first need per database (k_asym_expand_rows, k_pq_expand_rows; stats "asym_float_rows" / "pq_float_rows" say that a call came here)
int float_rows(hg_ctx* c, const RealReq& r, const float** rows) {
    RowSource& s = *r.src;
    if (s.kind != RowSource::FLOATS) {
        const bool pq = s.kind == RowSource::PQ;
        s.rows_read = 1;
        if (!s.rows_valid) {
            HG_TRY(s.rows.reserve((size_t)c->N * c->bpad * 4 + 256));
            c->t_begin(pq ? KI_PQ_EXPAND : KI_ASYM_EXPAND);
            expand_rows(c, s, s.rows, (i64)c->N, 1);
            c->t_end();
            HG_TRY(c->check_launch(pq ? "k_pq_expand_rows" : "k_asym_expand_rows"));
            s.rows_valid = true;
        }
    }
    *rows = s.rows.as<float>();
    return HG_OK;
}
// 16-bit image (IEEE half or bfloat16: the source's img_half) of every stride-th database row, `rows` of them padded to rows16, in MFMA fragment order
void expand_image16(hg_ctx* c, const RealReq& r, DevBuf& dst, i64 rows, i64 rows16, int KP, i64 stride) {
    const RowSource& s = *r.src;
    const dim3 grid(grid_for(rows16 * (KP / 8)));
    with_bool(s.img_half, [&](auto half) {
        if (s.kind == RowSource::CODES)
            hipLaunchKernelGGL(k_asym_image16<half>, grid, dim3(256), 0, c->stream, c->db.as<u32>(), dst.as<uint4>(), rows, rows16, KP, c->NW, c->b, stride);
        else if (s.kind == RowSource::PQ)
            hipLaunchKernelGGL(k_pq_image16<half>, grid, dim3(256), 0, c->stream, pq_tab(s), dst.as<uint4>(), rows, rows16, KP, c->b, stride);
        else
            hipLaunchKernelGGL(k_expand_dbf_bf16<half>, grid, dim3(256), 0, c->stream, s.rows.as<float>(), dst.as<uint4>(), rows, rows16, KP, stride);
        return HG_OK;
    });
}
// The smallest float32 that is >= x (x >= 0, or +inf): in integer arithmetic, whatever rounding and subnormal modes the host runs in.  A value
// below the smallest subnormal becomes that subnormal, one beyond the largest finite float +inf -- which makes the filter keep every row.
float float_at_least(double x) {
    if (!(x > 0.0)) return 0.0f;
    u64 d;
    memcpy(&d, &x, 8);
    const int e = (int)(d >> 52) - 1023;                 // x = (1 + frac / 2^52) 2^e (a subnormal double: e = -1023, far below every float)
    const u64 frac = d & ((1ull << 52) - 1);
    u32 f;
    if (e > 127) f = 0x7F800000u;
    else if (e >= -126) f = (((u32)(e + 127) << 23) | (u32)(frac >> 29)) + ((frac & ((1ull << 29) - 1)) ? 1u : 0u);   // (a carry runs into the exponent, up to +inf)
    else {
        const int sh = -97 - e;                          // x / 2^-149 = (2^52 + frac) >> sh, rounded up: the subnormal's significand (2^23: the smallest normal)
        const u64 full = frac | (1ull << 52);
        f = sh >= 64 ? 1u : (u32)(full >> sh) + ((full & ((1ull << sh) - 1)) ? 1u : 0u);
    }
    float r;
    memcpy(&r, &f, 4);
    return r;
}
// The filter's 16-bit image of the database, built on first use, and with it the largest row norm^2 (xmax2: k_real_thr2's margin) and the
// choice between IEEE half and bfloat16 -- once per database.  FLOATS: k_row_norm_max in double, one 8-byte download and a wait, rounded up
// to the float the margin reads.  CODES: +-1 is exact
// in either format and every row's norm^2 is exactly b -- the host writes that itself, a fill on the stream: no kernel, no download, no wait.
// PQ: the loader's bound on every row's norm^2 (the largest codeword that occurs, subspace by subspace: k_real_thr2's margin holds for any
// value >= the true maximum), written the same way.
int ensure_filter_image(hg_ctx* c, const RealReq& r) {
    RowSource& s = *r.src;
    if (s.img_valid) return HG_OK;
    const bool pq = s.kind == RowSource::PQ;
    const bool codes = s.kind != RowSource::FLOATS;         // (no float table: the host knows the norm word)
    const int KP = c->bpad;
    const i64 n16 = (c->N + 15) / 16 * 16;
    HG_TRY(s.img.reserve((size_t)n16 * KP * 2));
    HG_TRY(s.xmax2.reserve(8));                             // (the float the margin reads; FLOATS: first the double k_row_norm_max leaves)
    float xm = pq ? s.pq_xmax2 : (float)c->b;
    if (!codes) {
        double x2 = 0.0;
        HG_HIP(hipMemsetAsync(s.xmax2.p, 0, 8, c->stream));
        c->t_begin(KI_PACK);
        hipLaunchKernelGGL(k_row_norm_max, dim3(grid_for(c->N)), dim3(256), 0, c->stream, s.rows.as<float>(), (i64)c->N, KP, s.xmax2.as<u64>());
        HG_HIP(hipMemcpyAsync(&x2, s.xmax2.p, 8, hipMemcpyDeviceToHost, c->stream));
        HG_TRY(c->sync());
        xm = float_at_least(x2);
    }
    u32 xbits;
    memcpy(&xbits, &xm, 4);
    HG_HIP(hipMemsetD32Async((hipDeviceptr_t)s.xmax2.p, (int)xbits, 1, c->stream));
    if (codes) c->t_begin(pq ? KI_PQ_IMAGE : KI_ASYM_IMAGE);
    // IEEE half (three more significant bits: a margin an eighth of bfloat16's) when no feature can overflow it (every |x_k| <= the row's
    // norm < 2^15) and the rows are not tiny either: half's error has an absolute floor -- subnormals, flushed or not -- that outgrows the
    // relative term once norms fall below ~0.1; bfloat16 has float32's exponents and no such floor
    s.img_half = c->opt.real_mfma == 2 && xm >= 1.0f && xm < 1073741824.0f;         // 1 <= largest row norm^2 < 2^30 (inf and the NaN marker fail the test)
    expand_image16(c, r, s.img, c->N, n16, KP, 1);
    c->t_end();
    HG_TRY(c->check_launch(pq ? "k_pq_image16" : codes ? "k_asym_image16" : "k_expand_dbf_bf16"));
    s.img_valid = true;
    return HG_OK;
}
// The exact scores of the rows the filter kept: wavefront = (SG slices, query), `waves` of them.  FLOATS: k_real_rescore gathers the kept
// rows' float rows through LDS.  CODES: k_asym_rescore reads their code words instead (no LDS), the word count a template argument up to two.
// PQ: k_pq_rescore looks the operand up in the codebooks through the vector cache (no LDS), four features per read where dsub is a
// multiple of four.
template <int KP> int launch_rescore(hg_ctx* c, const RealReq& r, int SG, i64 waves) {
    const Geo& g = c->geo;
    const bool codes = r.src->kind == RowSource::CODES, pq = r.src->kind == RowSource::PQ;
    const float* rows = nullptr;
    if (!codes && !pq) HG_TRY(float_rows(c, r, &rows));
    c->t_begin(pq ? KI_PQ_RESCORE : codes ? KI_ASYM_RESCORE : KI_REAL_RESCORE);
    HG_TRY(with_slices(SG, [&](auto sg) {
        if (pq) {
            const RowSource& s = *r.src;
            return with_bool(s.pq_dsub % 4 == 0, [&](auto wide) {
                const PqRescoreArgs a{c->qf.as<float>(), pq_tab(s), c->sl_cnt.as<u32>(), c->krows.as<u32>(), c->cand.as<u64>(), c->cap, c->crow, c->thr.as<float>(),
                                      c->sl_cnt.as<u32>(), c->cntq.as<u32>(), c->dblab.as<u64>(), c->qlab.as<u64>(), r.no_cut ? 0 : 1, KP, g};
                hipLaunchKernelGGL((k_pq_rescore<(wide ? 4 : 1), sg>), dim3(grid_for(waves, WPB)), dim3(256), 0, c->stream, a);
                return HG_OK;
            });
        }
        auto from_codes = [&](auto nwt) {
            hipLaunchKernelGGL((k_asym_rescore<nwt, sg>), dim3(grid_for(waves, WPB)), dim3(256), 0, c->stream, c->qf.as<float>(), c->db.as<u32>(),
                               c->sl_cnt.as<u32>(), c->krows.as<u32>(), c->cand.as<u64>(), c->cap, c->crow, c->thr.as<float>(), c->sl_cnt.as<u32>(),
                               c->cntq.as<u32>(), c->dblab.as<u64>(), c->qlab.as<u64>(), r.no_cut ? 0 : 1, KP, c->NW, c->b, g);
            return HG_OK;
        };
        if (codes)       // (the code words: one, two, or NW at run time)
            return c->NW == 1 ? from_codes(std::integral_constant<int, 1>{}) : c->NW == 2 ? from_codes(std::integral_constant<int, 2>{}) : from_codes(std::integral_constant<int, 0>{});
        hipLaunchKernelGGL((k_real_rescore<(KP <= 128 ? KP : 0), sg>), dim3(grid_for(waves, WPB)), dim3(256), rescore_lds_bytes(), c->stream, c->qf.as<float>(),
                           rows, c->sl_cnt.as<u32>(), c->krows.as<u32>(), c->cand.as<u64>(), c->cap, c->crow, c->thr.as<float>(),
                           c->sl_cnt.as<u32>(), c->cntq.as<u32>(), c->dblab.as<u64>(), c->qlab.as<u64>(), r.no_cut ? 0 : 1, KP, g);
        return HG_OK;
    }));
    c->t_end();
    return c->check_launch(pq ? "k_pq_rescore" : codes ? "k_asym_rescore" : "k_real_rescore");
}
// Float rows for the staged sample beyond 128 features (k_real_sample_any), inside its timing slot, which this opens and the caller closes:
// every *stride-th row of the table -- or, from the codes or the PQ tables, the M sampled rows alone expanded into the sample's own per-call
// buffer (a few MB, like the 16-bit sample images; *stride becomes 1), so that a bet on more than 128 features never asks for the whole
// database as floats
int sampled_rows(hg_ctx* c, const RealReq& r, i64 M, i64* stride, const float** rows) {
    if (r.src->kind != RowSource::FLOATS) {
        HG_TRY(c->sampx.reserve((size_t)M * c->bpad * 4 + 256));
        c->t_begin(KI_REAL_SAMPLE);
        expand_rows(c, *r.src, c->sampx, M, *stride);
        *rows = c->sampx.as<float>();
        *stride = 1;
        return HG_OK;
    }
    HG_TRY(float_rows(c, r, rows));
    c->t_begin(KI_REAL_SAMPLE);
    return HG_OK;
}

// ---- pair passes ----
// the sample's scores feed only the cut: with the 16-bit filter behind it the sample runs in the same arithmetic ("real_mfma" 1 keeps the exact chains)
bool sample_in_16bit(const hg_ctx* c) { return c->bpad <= 128 && c->opt.real_mfma == 2 && c->opt.real_sample_half && c->geo.L % 16 == 0; }

template <int BP> int real_launch_sample(hg_ctx* c, const RealReq& r, i64 M, i64 stride) {
    const Geo& g = c->geo;
    const i64 units = (M + 63) / 64 * g.nQT;
    const float* dbf;
    HG_TRY(float_rows(c, r, &dbf));
    c->t_begin(KI_REAL_SAMPLE);
    hipLaunchKernelGGL(k_real_sample<BP>, dim3(grid_for(units, WPB)), dim3(256), (size_t)WPB * 64 * 65 * 4, c->stream,
                       c->qf.as<float>(), dbf, c->samp.as<float>(), M, stride, g);
    c->t_end();
    return c->check_launch("k_real_sample");
}
// (one query per lane: the call's own geometry, a unit = one segment x 64 queries)
template <int BP> int real_launch_select(hg_ctx* c, const RealReq& r) {
    const Geo& g = c->geo;
    RealSelArgs a{c->thr.as<float>(), c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->cap, c->crow};
    const float* dbf;
    HG_TRY(float_rows(c, r, &dbf));
    c->t_begin(KI_REAL_SELECT);
    hipLaunchKernelGGL((k_real_select<BP, 1>), dim3(padded_grid(g.nBlk)), dim3(256), 0, c->stream, c->qf.as<float>(),
                       dbf, a, c->cand.as<u64>(), g);
    c->t_end();
    return c->check_launch("k_real_select");
}
// real-valued select on the matrix cores: blocks = (pair of segments) x (256 queries)
template <int KP> int real_launch_select_mx(hg_ctx* c, const RealReq& r) {
    RowSource& s = *r.src;
    if (!s.rowsx_valid) {
        const i64 n16 = (c->N + 15) / 16 * 16;
        HG_TRY(s.rowsx.reserve((size_t)n16 * KP * 4));
        const i64 items = n16 * (KP / 4);
        const float* dbf;
        HG_TRY(float_rows(c, r, &dbf));
        c->t_begin(KI_PACK);
        hipLaunchKernelGGL(k_expand_dbf, dim3(grid_for(items)), dim3(256), 0, c->stream, dbf, s.rowsx.as<float4>(),
                           (i64)c->N, n16, KP, (i64)1);
        c->t_end();
        HG_TRY(c->check_launch("k_expand_dbf"));
        s.rowsx_valid = true;
    }
    const Geo g = pair_geometry(c->geo, c->geo.N, 0, REAL_MX_QPB);
    RealSelArgs a{c->thr.as<float>(), c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->cap, c->crow};
    c->t_begin(KI_REAL_SELECT);
    hipLaunchKernelGGL((k_real_select_mx<KP>), dim3(padded_grid(g.nBlk)), dim3(256), 0, c->stream,
                       c->qf.as<float>(), s.rowsx.as<u8>(), a, c->cand.as<u64>(), g);
    c->t_end();
    return c->check_launch("k_real_select_mx");
}
// Slices per wavefront of the rescoring pass.  The kernel's time follows its ROUNDS of 64 rows and its wavefronts, hardly its rows
// (10k x 1M x 64, R = 5000, 17 rows per slice: 1 slice 4.04 ms, 2 2.41, 3 2.06, 4 2.12, 5 2.05, 6 1.90, 7 1.92, 8 2.07, 11 2.20), so
// the count that fills its rounds best: expected rounds of a wavefront (`per_slice` rows expected in a slice, Poisson-ish) plus half
// a round of fixed cost, a little more per round the more slices the lane-to-slice search walks, per slice
int rescore_slices_per_wave(double per_slice) {
#ifdef HG_RS_FORCE
    (void)per_slice;
    return HG_RS_FORCE;
#else
    int SG = 1;
    double best = 1e300;
    for (const int sg : {1, 2, 3, 4, 6, 8}) {
        if (per_slice >= 64.0 && sg > 2) break;          // (slices of full rounds: nothing to pack, keep the rows' L2 footprint small)
        const double m = per_slice * sg, sd = std::sqrt(m > 1.0 ? m : 1.0);
        double rounds = 1.0;
        for (int k = 1; k <= 64; ++k) {
            const double p = 0.5 * std::erfc((64.0 * k - m) / sd * 0.7071067811865476);
            rounds += p;
            if (p < 1e-6) break;
        }
        const double cost = (0.5 + rounds * (1.0 + 0.03 * sg)) / sg;
        if (cost < best) { best = cost; SG = sg; }
    }
    return SG;
#endif
}
// filter + rescore (hg_real_bf.hpp): bf16 pair pass with a rigorous margin, then the exact chain for the survivors
template <int KP> int real_launch_select_bf(hg_ctx* c, const RealReq& r) {
    constexpr int QT = KP <= 128 ? 2 : 1;
    HG_TRY(ensure_filter_image(c, r));
    const RowSource& s = *r.src;
    c->real.half = s.img_half;
    const Geo& g = c->geo;
    HG_TRY(c->thr2.reserve((size_t)g.Qpad * 4));
    c->t_begin(KI_REAL_GUESS);
    hipLaunchKernelGGL(k_real_thr2, dim3(grid_for(g.Q)), dim3(256), 0, c->stream, c->qf.as<float>(), c->thr.as<float>(),
                       s.xmax2.as<u32>(), c->thr2.as<float>(), g.Q, KP, s.img_half ? 1.0 / 1024.0 : 1.0 / 256.0, s.img_half ? 1.0 / 16384.0 : 0.0);
    c->t_end();
    HG_TRY(c->check_launch("k_real_thr2"));
    const Geo gs = pair_geometry(g, g.N, 0, WPB * 32 * QT);
    RealSelArgs a{c->thr.as<float>(), c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->cap, c->crow};
    HG_TRY(c->krows.reserve((size_t)g.Q * c->crow * 4));     // the kept rows' numbers: the filter writes, the rescore reads
    // (a wavefront's 64 record rows within 4 GB: 32-bit cursors -- every bet; beyond, e.g. every row a record of a 10M-row database, 64-bit ones)
    // (a 32-bit cursor keeps counting past a full slice -- by up to a segment's rows -- so that the hits it dropped are known: the
    // furthest it can get is the wavefront's 64 record rows plus one segment)
    // (test hook "real_far_cursors": the 64-bit cursors at any size)
    const bool far_rows = c->real_far_cursors != 0 || (64ull * (unsigned long long)c->crow + (unsigned long long)g.L) * 4ull >= (1ull << 32);
    c->t_begin(KI_REAL_SELECT);
    HG_TRY(with_bool(s.img_half, [&](auto half) { return with_bool(far_rows, [&](auto far_) {
        if (real_bf_lds_bytes(KP) > 64 * 1024)
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_real_select_bf<KP, QT, half, far_>), hipFuncAttributeMaxDynamicSharedMemorySize, real_bf_lds_bytes(KP)));
        hipLaunchKernelGGL((k_real_select_bf<KP, QT, half, far_>), dim3(padded_grid(gs.nBlk)), dim3(256), real_bf_lds_bytes(KP), c->stream,
                           c->qf.as<float>(), s.img.as<u8>(), c->thr2.as<float>(), a, c->krows.as<u32>(), gs);
        return HG_OK;
    }); }));
    c->t_end();
    HG_TRY(c->check_launch("k_real_select_bf"));
    // (the rows a query is expected to keep -- the rank its cut was guessed at, scaled back from the sample; every row without a cut -- over its slices)
    const int SG = rescore_slices_per_wave(1.03 * r.expect / (double)g.S);
    const i64 waves = (i64)((g.S + SG - 1) / SG) * g.Q;
    HG_TRY(c->cntq.reserve((size_t)g.Q * g.S * 4));
    return launch_rescore<KP>(c, r, SG, waves);
}
// sample pass on the float32 MFMA: image of the M sampled rows (rebuilt per call: a few MB), ~32 segments (16 pairs)
template <int KP> int real_launch_sample_mx(hg_ctx* c, const RealReq& r, i64 M, i64 stride, i64 mstride) {
    const i64 m16 = (M + 15) / 16 * 16;
    HG_TRY(c->sampx.reserve((size_t)m16 * KP * 4));
    const float* dbf;
    HG_TRY(float_rows(c, r, &dbf));
    c->t_begin(KI_REAL_SAMPLE);
    hipLaunchKernelGGL(k_expand_dbf, dim3(grid_for(m16 * (KP / 4))), dim3(256), 0, c->stream, dbf, c->sampx.as<float4>(),
                       M, m16, KP, stride);
    const Geo g = pair_geometry(c->geo, M, 32, REAL_MX_QPB);
    hipLaunchKernelGGL((k_real_sample_mx<KP>), dim3(padded_grid(g.nBlk)), dim3(256), 0, c->stream, c->qf.as<float>(), c->sampx.as<u8>(),
                       c->samp.as<float>(), mstride, g);
    c->t_end();
    return c->check_launch("k_real_sample_mx");
}
// sample pass in the filter's 16-bit arithmetic (k_real_sample_h): the sampled rows' image rebuilt per call (1.6 MB at 10k x 1M), ~32 segments
template <int KP> int real_launch_sample_h(hg_ctx* c, const RealReq& r, i64 M, i64 stride, i64 mstride) {
    HG_TRY(ensure_filter_image(c, r));                   // (decides half / bfloat16 for this database)
    const i64 m16 = (M + 15) / 16 * 16;
    HG_TRY(c->sampx.reserve((size_t)m16 * KP * 2));
    c->t_begin(KI_REAL_SAMPLE);
    expand_image16(c, r, c->sampx, M, m16, KP, stride);
    const Geo g = pair_geometry(c->geo, M, 32, WPB * 64);
    with_bool(r.src->img_half, [&](auto half) { return with_bool(r.samp16, [&](auto o16) {
        hipLaunchKernelGGL((k_real_sample_h<KP, half, o16>), dim3(padded_grid(g.nBlk)), dim3(256), 0, c->stream, c->qf.as<float>(),
                           c->sampx.as<u8>(), c->samp.as<float>(), mstride, g);
        return HG_OK;
    }); });
    c->t_end();
    return c->check_launch("k_real_sample_h");
}
// the second, counting sample (k_real_sample_count + k_real_guess2): thr[q] moves up to the deepest cut a four times larger sample supports
template <int KP> int real_launch_sample_count(hg_ctx* c, const RealReq& r, i64 M2, i64 stride2, u32 need2) {
    const Geo& g0 = c->geo;
    const i64 m16 = (M2 + 15) / 16 * 16;
    HG_TRY(c->sampx.reserve((size_t)m16 * KP * 2));     // (sized for this pass before the first one ran: place_cut)
    c->t_begin(KI_REAL_SAMPLE);
    expand_image16(c, r, c->sampx, M2, m16, KP, stride2);
    const Geo g = pair_geometry(g0, M2, 64, WPB * 64);   // ~64 segments (32 pairs; 16 .. 256 segments measured: 32 and up the same)
    const int nSP = seg_pairs(g);
    HG_TRY(c->hist2.reserve((size_t)nSP * g.Qpad * RC_BINS * 4 + (size_t)WPB * 64 * RC_BINS * 4));      // [segment pair][Qpad][bin], every word written (+ a block's overhang past Qpad)
    constexpr int lds = real_count_lds_bytes(KP);
    HG_TRY(with_bool(r.src->img_half, [&](auto half) {
        if (lds > 64 * 1024) HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_real_sample_count<KP, half>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL((k_real_sample_count<KP, half>), dim3(padded_grid(g.nBlk)), dim3(256), lds, c->stream, c->qf.as<float>(), c->sampx.as<u8>(),
                           c->thr.as<float>(), c->hist2.as<u32>(), g);
        return HG_OK;
    }));
    c->t_end();
    HG_TRY(c->check_launch("k_real_sample_count"));
    c->t_begin(KI_REAL_GUESS);
    hipLaunchKernelGGL(k_real_guess2, dim3(grid_for(g0.Q, 8)), dim3(256), 0, c->stream, c->hist2.as<u32>(), c->thr.as<float>(), g0.Q, (i64)g0.Qpad, nSP, need2);
    c->t_end();
    return c->check_launch("k_real_guess2");
}
// scores of every stride-th row (M of them) into samp[q][mstride]
int real_sample(hg_ctx* c, const RealReq& r, i64 M, i64 stride, i64 mstride) {
    if (sample_in_16bit(c)) return with_features<128>(c, [&](auto kp) { return real_launch_sample_h<kp>(c, r, M, stride, mstride); });
    if (c->bpad <= 128 && c->opt.real_mfma) return with_features<128>(c, [&](auto kp) { return real_launch_sample_mx<kp>(c, r, M, stride, mstride); });
    if (c->bpad > 128) {                                 // k_real_sample keeps the query in registers: the staged form beyond
        const Geo& g = c->geo;
        const i64 units = (M + 63) / 64 * g.nQT;
        const size_t lds = (size_t)WPB * (64 * 65 * 4 + 16 * 128);
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_real_sample_any), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const float* dbf = nullptr;
        HG_TRY(sampled_rows(c, r, M, &stride, &dbf));      // (opens the sample's timing slot)
        hipLaunchKernelGGL(k_real_sample_any, dim3(grid_for(units, WPB)), dim3(256), lds, c->stream, c->qf.as<float>(), dbf,
                           c->samp.as<float>(), M, stride, c->bpad, g);
        c->t_end();
        return c->check_launch("k_real_sample_any");
    }
    // (the vector kernels write samp[q][M] densely: the caller passes mstride = M)
    return with_features<128>(c, [&](auto kp) { return real_launch_sample<kp / 2>(c, r, M, stride); });
}
// the pair pass over the whole database; *filtered = it left unscored candidates that k_real_rescore completed
int real_select(hg_ctx* c, const RealReq& r, bool* filtered) {
    *filtered = false;
    // without a cut (every row a record: R = N, or after lost bets) a filter filters nothing and every pair would be rescored:
    // the exact float32 MFMA pass gives the scores at once (C1: 4.6 -> 4.0 ms per call)
    const bool filter = c->opt.real_mfma == 2 && !(r.no_cut && c->bpad <= 128);
    if ((filter || c->bpad > 128) && c->geo.L % 16 == 0) {   // (the only pass for > 128 features)
        HG_TRY(with_features<256>(c, [&](auto kp) { return real_launch_select_bf<kp>(c, r); }));
        *filtered = true;
        return HG_OK;
    }
    if (c->opt.real_mfma && c->geo.L % 16 == 0) return with_features<128>(c, [&](auto kp) { return real_launch_select_mx<kp>(c, r); });
    return with_features<128>(c, [&](auto kp) { return real_launch_select<kp / 2>(c, r); });
}

// ---- one attempt, stage by stage: geometry -> cut (or none) -> select -> one of three rank tails ----
void real_geometry(hg_ctx* c, const RealReq& r) {
    make_geometry(c);
    Geo& g = c->geo;
    {   // Float rows are 4*bpad bytes (32x a 64-bit code): keep a segment's rows within ~512 KB so the few
        // segments an XCD works on at a time stay in its 4 MiB L2 while all query tiles pass over them.
        i64 L = (i64)REAL_SEG_BYTES / ((i64)c->bpad * 4);
        L = L / 16 * 16;
        if (L < 64) L = 64;
        if (g.L > L) cut_segments(g, L);
    }
    if (r.no_cut && c->bpad <= 128 && c->opt.real_mfma && c->opt.real_whole_rounds > 0) {
        // Every row a record through k_real_select_mx: blocks = (pairs of segments) x (256 queries), four wavefronts each, up to
        // three resident per CU (two beyond 64 features).  The plain geometry gave the CIFAR evaluation (1000 x 54 000) 376 blocks
        // for 256 CUs -- half the CUs with two, half with one; cut the database so that the blocks fill whole rounds instead.
        const i64 nQB = (g.Q + REAL_MX_QPB - 1) / REAL_MX_QPB;
        const i64 per_cu = c->bpad <= 64 ? std::min<i64>(c->opt.real_whole_rounds, 3) : std::min<i64>(c->opt.real_whole_rounds, 2);
        const i64 slots = (i64)c->n_cu * per_cu;
        i64 k = (seg_pairs(g) * nQB + slots - 1) / slots;          // rounds the plain geometry touches
        if (k < 1) k = 1;
        const i64 nSP = slots * k / nQB;
        if (nSP >= 1) {
            i64 L = (g.N + 2 * nSP - 1) / (2 * nSP);
            L = (L + 15) / 16 * 16;
            if (L < 64) L = 64;
            if (L <= g.L) cut_segments(g, L);
        }
    }
}
// The bet: sample so that about 64 of a query's top R rows are in it; guess the cut `sigma` deviations deep (thr[q]).  With a second,
// counting sample behind it (256 expected hits) the first one only has to bracket the cut from below: half the rows do
// (REAL_FIRST_HITS_BRACKET).  Then the slices' capacity.  What the stage learns for the ones after it goes into the request.
int place_cut(hg_ctx* c, RealReq& r) {
    const Geo& g = c->geo;
    const i64 R = r.R;
    const bool can16 = sample_in_16bit(c);
    const i64 stride2 = (i64)((double)R / (double)(REAL_SAMPLE_HITS * REAL_SECOND_SAMPLE));
    i64 stride = (i64)((double)R / (double)REAL_FIRST_HITS_BRACKET);
    const bool second = can16 && c->opt.real_second_sample && stride2 >= 1 && stride >= 2 * stride2 && (c->N + stride - 1) / stride <= RG_MMAX;
    if (!second) stride = (i64)((double)R / (double)REAL_SAMPLE_HITS);
    if (stride < 1) stride = 1;
    const i64 M = (c->N + stride - 1) / stride;
    const double fr = (double)R * (double)M / (double)c->N;
    const u32 rank_s = (u32)std::ceil(fr + r.sigma * std::sqrt(fr)) + 1u;
    // samp[q][mstride]: the matrix-core sample pass stores 16 samples at a time (rows 64-byte aligned), the vector kernels M densely
    const i64 mstride = c->bpad <= 128 && c->opt.real_mfma ? (M + 15) / 16 * 16 : M;
    HG_TRY(c->samp.reserve((size_t)g.Q * mstride * 4));
    // 16-bit sample scores when both ends take them: k_real_sample_h writes, k_real_guess_lds reads
    r.samp16 = M <= RG_MMAX && can16;
    // ... and then the second, counting sample tightens the cut (k_real_sample_count)
    const i64 M2 = second ? (c->N + stride2 - 1) / stride2 : 0;
    if (second) HG_TRY(c->sampx.reserve((size_t)((M2 + 15) / 16 * 16) * c->bpad * 2));      // (before the first pass reads it: no move between the two)
    HG_TRY(real_sample(c, r, M, stride, mstride));
    c->t_begin(KI_REAL_GUESS);
    if (M <= RG_MMAX) with_bool(r.samp16, [&](auto s16) {
        hipLaunchKernelGGL(k_real_guess_lds<s16>, dim3(g.Q), dim3(1024), 0, c->stream, c->samp.as<float>(), M, mstride, rank_s, c->thr.as<float>());
        return HG_OK;
    });
    else hipLaunchKernelGGL(k_real_guess, dim3(g.Q), dim3(256), 0, c->stream, c->samp.as<float>(), M, mstride, rank_s, c->thr.as<float>());
    c->t_end();
    HG_TRY(c->check_launch("k_real_guess"));
    if (second) {
        const double fr2 = (double)R * (double)M2 / (double)c->N;
        const u32 need2 = (u32)std::ceil(fr2 + r.sigma * std::sqrt(fr2)) + 1u;
        HG_TRY(with_features<128>(c, [&](auto kp) { return real_launch_sample_count<kp>(c, r, M2, stride2, need2); }));
        r.expect = (double)R * (1.0 + r.sigma / std::sqrt(fr2 > 1.0 ? fr2 : 1.0));
    }
    const double mean = r.budget * (double)R / (double)g.S;
    u32 cap = (u32)std::ceil(mean + 6.0 * std::sqrt(mean) + 16.0);
    cap = (cap + 15u) & ~15u;                         // a multiple of the compact records' ring (16) and flush piece (8)
    const u32 whole = (u32)((g.L + 15) & ~15ll);      // (a slice never needs more than its segment's rows)
    c->cap = cap < whole ? cap : whole;
    return HG_OK;
}
// no bet: every row becomes a record (thr = -inf), slices are whole segments
int take_every_row(hg_ctx* c) {
    HG_HIP(hipMemsetD32Async((hipDeviceptr_t)c->thr.p, (int)0xFF800000u, (size_t)c->geo.Q, c->stream));     // (a fill on the stream: no host vector, no wait)
    c->cap = (u32)c->geo.L;
    return HG_OK;
}
// Behind a kernel that ranks in LDS and leaves the match bits: the usual case needs nothing more, so AP and the download of {flag, AP,
// hit counts} ride behind the kernel and the call synchronises ONCE (round 5: verdict, wait, AP, wait, two copies, wait); when the flag
// says otherwise the APs are simply not used.  Leaves the stage at the select: the caller adds what the flag allows.
int ap_behind_then_flag(hg_ctx* c, const RealReq& r, int* flag) {
    if (r.with_ap) {
        c->stage = ST_DB | ST_Q | ST_SELECT | ST_MATCH;
        HG_TRY(do_ap(c));
        HG_TRY(stage_ap_download(c));
    }
    HG_TRY(wait_verdict(c, r.with_ap, flag));
    c->stage = ST_DB | ST_Q | ST_SELECT;
    return HG_OK;
}
// a bet whose records fit the LDS of one workgroup: copy + select + counting passes + ranked list in one kernel.  *ranked = false:
// some query's records exceed the LDS, the global-memory passes rank them all
int rank_in_lds(hg_ctx* c, const RealReq& r, int* lost, bool* ranked) {
    const Geo& g = c->geo;
    constexpr int NA = 14336;
    HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_real_rank_lds<NA>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)real_rank_lds_bytes<NA>()));
    c->t_begin(KI_RADIX);
    hipLaunchKernelGGL(k_real_rank_lds<NA>, dim3(g.Q), dim3(1024), real_rank_lds_bytes<NA>(), c->stream, c->cand.as<u64>(), c->crow, c->cap,
                       c->cntq.as<u32>(), c->failq.as<u32>(), c->thr.as<float>(), r.skip_lists ? nullptr : c->out_idx.as<u32>(), r.skip_lists ? nullptr : c->scores.as<float>(),
                       c->dblab.as<u64>(), c->qlab.as<u64>(), c->mbits.as<u64>(), c->RW, c->err.as<int>(), c->qbad.as<u32>(), g);
    c->t_end();
    HG_TRY(c->check_launch("k_real_rank_lds"));
    int flag = 0;
    HG_TRY(ap_behind_then_flag(c, r, &flag));            // (a lost bet's APs are not used)
    *ranked = !(flag & 2);
    if (!*ranked) {
        HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
        return HG_OK;
    }
    c->real.lds_ranked = true;
    c->real.lists_made = !r.skip_lists;
    *lost = flag & 1;
    if (*lost) return HG_OK;
    c->stage |= ST_MATCH;                                // the rank kernel left the match bits too
    if (r.with_ap) { c->stage |= ST_AP; c->ap_staged = true; }
    return HG_OK;
}
// every row a record (R = N on a CIFAR-sized database): split by score range into LDS-sized groups, order each group
// in LDS (k_real_group_split / k_real_group_sort) -- two trips of the records through memory instead of the radix
// passes' four, 3.1 -> 0.85 ms at C1; piled-up scores come back as bit 2 of the flag (*ranked = false).  (A bet's list beyond the
// LDS -- 19 000 records in 489 short slices at R = 10 000 -- stays with the radix passes: 3.9 ms against 5.7 this way.)
int rank_by_groups(hg_ctx* c, const RealReq& r, int* lost, bool* ranked) {
    const Geo& g = c->geo;
    HG_TRY(c->gtab.reserve((size_t)g.Q * (RG_MAXG + 1) * 4));
    // (a group spans at least RG_CAP / 2 of cumulative count -- the largest bucket is at most RG_CAP / 2: at most 2 n / RG_CAP + 1 groups)
    const int maxg = (int)std::min<i64>(RG_MAXG, 2 * c->crow / RG_CAP + 2);
    // (per launch like everywhere else: the attribute is per DEVICE, and a process may hold contexts on several)
    HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_real_group_sort), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)real_group_sort_lds()));
    c->t_begin(KI_RADIX);
    hipLaunchKernelGGL(k_real_group_split, dim3(g.Q), dim3(1024), real_group_split_lds(g.S), c->stream, c->cand.as<u64>(), c->crow, c->cap,
                       c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->tot.as<u32>(), c->sortA.as<u64>(), c->gtab.as<u32>(), c->crow, c->err.as<int>(), maxg, g);
    c->t_end();
    HG_TRY(c->check_launch("k_real_group_split"));
    // the sort writes the ranked lists and the match bits itself (k_real_finish and k_match are for the radix passes)
    HG_HIP(hipMemsetAsync(c->mbits.p, 0, (size_t)g.Q * c->RW * 8, c->stream));
    HG_HIP(hipMemsetAsync(c->qbad.p, 0, (size_t)g.Qpad * 4, c->stream));
    const GroupOut go{r.skip_lists ? nullptr : c->out_idx.as<u32>(), r.skip_lists ? nullptr : c->scores.as<float>(), c->mbits.as<u32>(), c->dblab.as<u64>(), c->qlab.as<u64>(), c->RW, g.R, g.LW, g.idx_base};
    c->t_begin(KI_RADIX);
    hipLaunchKernelGGL(k_real_group_sort, dim3(g.Q, maxg), dim3(1024), real_group_sort_lds(), c->stream, c->sortA.as<u64>(), c->gtab.as<u32>(),
                       go, c->crow, c->err.as<int>());
    c->t_end();
    HG_TRY(c->check_launch("k_real_group_sort"));
    int flag = 0;
    HG_TRY(ap_behind_then_flag(c, r, &flag));            // (a piled-up query's APs are not used -- the bitmaps they are read from are zeroed, defined memory)
    *ranked = !(flag & 4);
    if (!*ranked) {
        HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
        return HG_OK;
    }
    c->real.grouped = true;
    c->real.lists_made = !r.skip_lists;
    *lost = flag;
    c->stage |= ST_MATCH;
    if (r.with_ap) { c->stage |= ST_AP; c->ap_staged = flag == 0; }
    return HG_OK;
}
// the global-memory passes: four radix passes between two sort buffers, k_real_finish, and the labels gathered through the ranked
// idx list (k_match) -- so the lists are written whoever asked
int rank_by_radix(hg_ctx* c, const RealReq& r, size_t rows, int* lost) {
    const Geo& g = c->geo;
    const size_t slots = (size_t)g.Q * g.R;
    HG_TRY(c->sortB.reserve(rows));
    HG_TRY(c->out_idx.reserve(slots * 4)); HG_TRY(c->scores.reserve(slots * 4));
    c->real.lists_made = true;
    const int nwav = c->crow >= 16384 ? 16 : 4;
    const size_t lds = (size_t)(nwav + 1) * 256 * 4;
    const u64* in = c->cand.as<u64>();
    u64* bufs[2] = {c->sortA.as<u64>(), c->sortB.as<u64>()};
    for (int pass = 0; pass < 4; ++pass) {
        RadixArgs ra{c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->tot.as<u32>(), c->cap, c->crow, c->crow, pass == 0, 32 + 8 * pass};
        u64* out = bufs[pass & 1];
        c->t_begin(KI_RADIX);
        if (nwav == 16) hipLaunchKernelGGL(k_radix_pass<16>, dim3(g.Q), dim3(1024), lds, c->stream, in, out, ra, g);
        else hipLaunchKernelGGL(k_radix_pass<4>, dim3(g.Q), dim3(256), lds, c->stream, in, out, ra, g);
        c->t_end();
        HG_TRY(c->check_launch("k_radix_pass"));
        in = out;
    }
    c->t_begin(KI_REAL_FINISH);
    const i64 nKB = grid_for(g.R);
    if (nKB * g.Q > 0x7FFFFFFFll) return fail(HG_ERR_ARG, "real-valued ranking: Q*R too large for one launch");
    hipLaunchKernelGGL(k_real_finish, dim3((unsigned)(nKB * g.Q)), dim3(256), 0, c->stream, in, c->crow, c->tot.as<u32>(),
                       c->out_idx.as<u32>(), c->scores.as<float>(), c->err.as<int>(), c->qbad.as<u32>(), (int)nKB,
                       c->real.filtered ? c->thr.as<float>() : nullptr, g);
    c->t_end();
    HG_TRY(c->check_launch("k_real_finish"));
    c->stage = ST_DB | ST_Q | ST_SELECT;
    HG_TRY(do_match(c));                               // label gather through the ranked idx list
    if (r.with_ap) HG_TRY(do_ap(c));
    return read_plan_flag(c, lost);
}

// ---- real-valued ranking: sample -> guess -> select (filter + rescore) -> rank in LDS, group by group, or by radix passes ----
// one attempt; *lost = some query came up short of R records or overflowed a slice (bet mode only)
int real_attempt(hg_ctx* c, RowSource& src, int64_t R, bool bet, double sigma, double budget, bool with_ap, int* lost) {
    RealState fresh;
    fresh.attempts = c->real.attempts + 1;
    c->real = fresh;
    RealReq req;
    req.src = &src; req.R = R; req.bet = bet; req.sigma = sigma; req.budget = budget; req.with_ap = with_ap;
    req.no_cut = !bet;
    req.expect = bet ? (double)R * (1.0 + sigma / std::sqrt((double)REAL_SAMPLE_HITS)) : (double)c->N;      // (a second sample lowers it: place_cut)
    // hg_map_real wants match bits and APs: the kernels that rank in LDS skip the idx / score lists then (Q x R x 8 bytes of stores: 0.4 GB at
    // 10k x R = 5000 and at the CIFAR evaluation alike); the global-memory passes gather the labels THROUGH the idx list and always write it
    // -- and only they reserve the lists then (and the second sort buffer: 0.43 GB each at the CIFAR evaluation, where a recycled context's
    // first call at the shape meets hipMalloc for whatever the block cache cannot serve)
    req.skip_lists = with_ap && !c->opt.real_map_lists && !c->is_sub;
    real_geometry(c, req);
    HG_TRY(set_R(c, R, 1, 0));
    const Geo& g = c->geo;
    const size_t qb = (size_t)g.Qpad * 4;
    HG_TRY(c->thr.reserve(qb)); HG_TRY(c->sl_cnt.reserve((size_t)g.S * qb)); HG_TRY(c->failq.reserve(qb));
    HG_TRY(c->tot.reserve(qb)); HG_TRY(c->err.reserve(16)); HG_TRY(c->qbad.reserve(qb));
    HG_HIP(hipMemsetAsync(c->failq.p, 0, qb, c->stream));
    HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
    if (bet) HG_TRY(place_cut(c, req)); else HG_TRY(take_every_row(c));
    c->crow = (i64)g.S * c->cap;
    // the record rows; the global-memory ranking passes (a query whose records exceed the LDS, the exhaustive mode) need two
    // more buffers of that size -- a widened bet (real_ladder) only goes as far as the rows alone stay moderate
    const size_t rows = (size_t)g.Q * c->crow * 8;
    const bool beyond_global = rows * 3 > (size_t)200 << 30;
    if (bet && rows > (size_t)64 << 30) { *lost = 1; return HG_OK; }
    if (!bet && beyond_global)
        return fail(HG_ERR_NOMEM, "real-valued ranking: %zu GB of records needed (Q=%d, %lld per query)", rows * 3 >> 30, g.Q, (long long)c->crow);
    HG_TRY(c->cand.reserve(rows));
    HG_TRY(real_select(c, req, &c->real.filtered));
    HG_TRY(c->mbits.reserve((size_t)g.Q * c->RW * 8));
    if (!req.skip_lists) { HG_TRY(c->out_idx.reserve((size_t)g.Q * g.R * 4)); HG_TRY(c->scores.reserve((size_t)g.Q * g.R * 4)); }
    bool ranked = false;
    if (c->real.filtered && bet && c->opt.real_sort_lds && g.S <= RK_SMAX && R <= RK_RMAX) {
        HG_TRY(rank_in_lds(c, req, lost, &ranked));
        if (ranked) return HG_OK;
    }
    if (beyond_global) { *lost = 1; return HG_OK; }      // (a bet: without one the call has failed above)
    HG_TRY(c->sortA.reserve(rows));
    if (c->opt.real_groups && g.S <= 8192 && !bet && c->crow <= (i64)RG_MAXG * RG_CAP) {
        HG_TRY(rank_by_groups(c, req, lost, &ranked));
        if (ranked) return HG_OK;
    }
    return rank_by_radix(c, req, rows, lost);
}

int real_call(hg_ctx* c, RowSource& src, int64_t R, bool with_ap);

// A few queries lost the first bet (their cut kept fewer than R rows, or their rows crowd into one slice): those alone run again,
// on a child context that borrows the database's tables and runs on the parent's row source, with the usual escalation; their lists and match bits go back into the
// parent's rows and the parent evaluates all queries.  The whole call is redone only when many queries lost (real_ladder).  Because a
// lost query now costs a fraction of a millisecond instead of the call, the first cut can sit shallower (REAL_FIRST_SIGMA).
int real_requery_lost(hg_ctx* c, RowSource& src, int64_t R, bool with_ap, bool* handled) {
    *handled = false;
    if (c->is_sub || !c->real.lds_ranked || !c->real.filtered) return HG_OK;
    const Geo g = c->geo;
    std::vector<u32> bad((size_t)g.Q);
    HG_HIP(hipMemcpyAsync(bad.data(), c->qbad.p, (size_t)g.Q * 4, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    std::vector<u32> lost;
    for (int q = 0; q < g.Q; ++q) if (bad[(size_t)q]) lost.push_back((u32)q);
    const i64 nF = (i64)lost.size();
    if (nF == 0 || nF * 16 > g.Q) return HG_OK;
    hg_ctx* s = requery_child(c, nF);
    s->real_cap_boost = c->real_cap_boost;
    HG_TRY(c->flist.reserve((size_t)nF * 4));
    HG_HIP(hipMemcpyAsync(c->flist.p, lost.data(), (size_t)nF * 4, hipMemcpyHostToDevice, c->stream));
    HG_TRY(s->qf.reserve((size_t)nF * c->bpad * 4 + 256));
    HG_TRY(s->qlab.reserve((size_t)nF * c->LW * 8));
    auto move = [&](const void* from, void* to, i64 rowbytes, int gather) {
        hipLaunchKernelGGL(k_move_rows, dim3((unsigned)nF), dim3(256), 0, c->stream, (const u8*)from, (u8*)to,
                           c->flist.as<u32>(), rowbytes, gather);
    };
    move(c->qf.p, s->qf.p, (i64)c->bpad * 4, 1);
    move(c->qlab.p, s->qlab.p, (i64)c->LW * 8, 1);
    HG_TRY(c->check_launch("k_move_rows"));
    s->qf_resident = true;
    s->stage = ST_DB | ST_Q;
    HG_TRY(real_call(s, src, R, false));               // (the same stream, strictly in sequence: an image the child builds is the source's)
    if (s->RW != c->RW) return fail(HG_ERR_HIP, "real-valued ranking: internal error, the requeried lists have another width");
    move(s->mbits.p, c->mbits.p, c->RW * 8, 0);
    if (c->real.lists_made) {
        move(s->out_idx.p, c->out_idx.p, R * 4, 0);
        move(s->scores.p, c->scores.p, R * 4, 0);
    }
    HG_TRY(c->check_launch("k_move_rows"));
    HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
    c->stage = ST_DB | ST_Q | ST_SELECT | ST_MATCH;
    if (with_ap) HG_TRY(do_ap(c));
    HG_TRY(c->sync());                               // `lost` (the H2D source) must outlive the copy
    c->real_requeried += nF;
    *handled = true;
    return HG_OK;
}

// The attempts of one call, until one holds: the bet on a sampled cut; its few lost queries alone; deeper cuts with wider slices;
// every row a record.
int real_ladder(hg_ctx* c, RowSource& src, int64_t R, bool with_ap) {
    int lost = 0;
    if (R * 8 <= c->N && c->N >= 65536) {              // bet on a sampled cut; retry once deeper, then give up betting
        const double boost0 = (double)c->real_cap_boost;
        HG_TRY(real_attempt(c, src, R, true, c->is_sub ? 6.0 : REAL_FIRST_SIGMA, 3.0 * boost0, with_ap, &lost));
        if (!lost) return HG_OK;
        bool handled = false;
        HG_TRY(real_requery_lost(c, src, R, with_ap, &handled));
        if (handled) return HG_OK;
        // a deeper cut with twice the budget; then -- features that follow the labels in a database stored class by class
        // put a query's top rows into a tenth of its slices -- eight and sixty-four times the slices' capacity, kept for
        // the next calls on this database (the exhaustive mode below writes EVERY pair down: 80 GB at 10k x 1M)
        for (int attempt = 0; attempt < 3; ++attempt) {
            if (attempt > 0) {
                if (c->cap >= (u32)((c->geo.L + 15) & ~15ll)) break;      // a slice already holds its segment
                c->real_cap_boost = c->real_cap_boost * 8 > 4096 ? 4096 : c->real_cap_boost * 8;
            }
            HG_TRY(real_attempt(c, src, R, true, 16.0, 6.0 * (double)c->real_cap_boost, with_ap, &lost));
            if (!lost) {
                if (attempt > 0 && c->real_cap_boost < 4096) c->real_cap_boost *= 2;     // (the budget that held: 6 = 2 x 3; a held plain retry changes nothing)
                return HG_OK;
            }
        }
        c->real_cap_boost = (i64)boost0;
    }
    HG_TRY(real_attempt(c, src, R, false, 0.0, 0.0, with_ap, &lost));
    if (lost) return fail(HG_ERR_HIP, "real-valued ranking: internal error, exhaustive pass came up short");
    return HG_OK;
}

// a call on the row source `src`, whose tables the caller has checked
int real_call(hg_ctx* c, RowSource& src, int64_t R, bool with_ap) {
    if (c->n_total != c->N) return fail(HG_ERR_STATE, "real-valued ranking is single-shard");
    if (R < 1 || R > c->N) return fail(HG_ERR_ARG, "R=%lld outside 1..N (N=%lld rows in the database)", (long long)R, (long long)c->N);
    if (c->N > 0x7FFFFFFFll) return fail(HG_ERR_ARG, "real-valued ranking takes up to 2^31 - 1 rows (have %lld)", (long long)c->N);   // (bit 31 of a record's index half is its match bit)
    c->real_lists = false;                             // from here on the list buffers are this call's: nothing to hand out unless it succeeds
    c->real.attempts = 0;
    if (with_ap && !c->is_sub) HG_TRY(ensure_out_block(c));      // verdict, APs and hit counts side by side: one download
    HG_TRY(real_ladder(c, src, R, with_ap));
    c->real_lists = c->real.lists_made;
    return HG_OK;
}

int run_real(hg_ctx* c, int64_t R, bool with_ap) {
    if (!c->bpad || !c->from_floats.rows.p || !c->qf.p || !c->from_floats.rows_valid || !c->qf_resident)
        return fail(HG_ERR_STATE, "real-valued ranking needs the float features on the GPU: load them with hg_set_database_f32 / "
                                  "hg_set_queries_f32 (option keep_floats = 1 if the database is a +-1 code)");
    return real_call(c, c->from_floats, R, with_ap);
}

// The asymmetric call: the same ladder on the database's CODES (any loader left them in c->db) and the queries' floats; what it leaves is
// what run_real leaves.
int run_asym(hg_ctx* c, int64_t R, bool with_ap) {
    c->real_lists = false;                             // a refused call leaves no lists either
    c->lists_valid = false;                            // ... and the call writes out_idx: a Hamming ranking's lists end here (hg_get_topr refuses)
    if (!c->bpad || !c->qf.p || !c->qf_resident || !c->db.p)
        return fail(HG_ERR_STATE, "asymmetric ranking needs the queries' float features on the GPU: set option keep_query_floats = 1, then load "
                                  "them with hg_set_queries_f32 / hg_set_queries_dev");
    c->from_codes.rows_read = 0;
    HG_TRY(real_call(c, c->from_codes, R, with_ap));
    c->asym_calls++;
    return HG_OK;
}

// The quantised call: the same ladder on the PQ tables hg_set_database_pq loaded and the queries' floats; what it leaves is what run_real
// leaves.
int run_pq(hg_ctx* c, int64_t R, bool with_ap) {
    c->real_lists = false;                             // a refused call leaves no lists either
    c->lists_valid = false;                            // ... and the call writes out_idx: a Hamming ranking's lists end here (hg_get_topr refuses)
    if (!c->from_pq.pq_valid)
        return fail(HG_ERR_STATE, "quantised ranking needs the database's PQ codes and codebooks: load them with hg_set_database_pq "
                                  "(any other database loader forgets them)");
    if (!c->bpad || !c->qf.p || !c->qf_resident)
        return fail(HG_ERR_STATE, "quantised ranking needs the queries' float features on the GPU: set option keep_query_floats = 1, then load "
                                  "them with hg_set_queries_f32 / hg_set_queries_dev");
    c->from_pq.rows_read = 0;
    HG_TRY(real_call(c, c->from_pq, R, with_ap));
    c->pq_calls++;
    return HG_OK;
}

}  // namespace

extern "C" {

int hg_topr_pq(hg_ctx* c, int64_t R) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_topr_pq", "hg_set_database_pq + hg_set_queries_f32 (option keep_query_floats = 1)"));
    return run_pq(c, R, false);
}

int hg_map_pq(hg_ctx* c, int64_t R, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_map_pq", "hg_set_database_pq + hg_set_queries_f32 (option keep_query_floats = 1)"));
    HG_TRY(run_pq(c, R, true));
    return hg_get_ap(c, host_ap, host_rel);
}

int hg_topr_real(hg_ctx* c, int64_t R) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_topr_real", "hg_set_database_f32 + hg_set_queries_f32"));
    return run_real(c, R, false);
}

int hg_map_real(hg_ctx* c, int64_t R, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_map_real", "hg_set_database_f32 + hg_set_queries_f32"));
    HG_TRY(run_real(c, R, true));
    return hg_get_ap(c, host_ap, host_rel);
}

int hg_topr_asym(hg_ctx* c, int64_t R) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_topr_asym", "a database load + hg_set_queries_f32 (option keep_query_floats = 1)"));
    return run_asym(c, R, false);
}

int hg_map_asym(hg_ctx* c, int64_t R, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_map_asym", "a database load + hg_set_queries_f32 (option keep_query_floats = 1)"));
    HG_TRY(run_asym(c, R, true));
    return hg_get_ap(c, host_ap, host_rel);
}

}  // extern "C"

// hg_preload: the runtime loads a translation unit's code object when one of its kernels is first needed (milliseconds);
// asking for a kernel's attributes does that now
int preload_real() {
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_real_thr2)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_asym_image16<true>)));      // (the same code object: the asymmetric kernels' names for a reader)
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_asym_rescore<2, 6>)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_asym_expand_rows)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_pq_image16<true>)));        // (... and the quantised kernels')
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_pq_rescore<4, 6>)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_pq_expand_rows)));
    return HG_OK;
}

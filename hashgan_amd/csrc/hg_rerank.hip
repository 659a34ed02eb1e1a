// libhashgan_amd.so -- the re-ranked Hamming ranking (hg_topr_rerank, hg_map_rerank, hg_get_rerank_scores): Hamming distance first,
// the float32 inner product inside equal distances, the database index last (hg_rerank.hpp; DESIGN.md section 3, "Re-ranked ties").
// A ranking like hg_topr: it owns the step state and leaves idx / dist lists, the match bitmap and -- its own -- the score list.
#include "hg_ctx.hpp"
#include "hg_rerank.hpp"

namespace {

template <int NW> int launch_collect_t(hg_ctx* c, const RerankArgs& a, int qt0, int nqt) {
    Geo g = c->geo;                                    // the histogram pass's segments: hist[s][d][q] holds their prefixes
    g.nUnits = (i64)g.S * nqt;
    // LDS: one u32 slot column per lane: wpb * NB * 64 * 4 bytes (<= 160 KiB per workgroup), as k_hist
    int wpb = WPB;
    while (wpb > 1 && (size_t)wpb * g.NB * 256 > 160u * 1024u) wpb >>= 1;
    g.wpb = wpb;
    g.nBlk = (int)((g.nUnits + wpb - 1) / wpb);
    const size_t lds = (size_t)wpb * g.NB * 256;
    static std::atomic<unsigned long long> lds_allowed{0};
    if (lds > 64 * 1024 && !(lds_allowed.load() >> (c->device & 63) & 1ull)) {
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rr_collect<NW>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_allowed.fetch_or(1ull << (c->device & 63));
    }
    c->t_begin(KI_RR_COLLECT);
    hipLaunchKernelGGL(k_rr_collect<NW>, dim3(padded_grid(g.nBlk)), dim3(64 * wpb), lds, c->stream, c->qc.as<u32>(), c->db.as<u32>(),
                       c->hist.as<u32>(), a, qt0, nqt, g);
    c->t_end();
    return c->check_launch("k_rr_collect");
}
int launch_collect(hg_ctx* c, const RerankArgs& a, int qt0, int nqt) { HG_DISPATCH_NW(launch_collect_t, c, a, qt0, nqt) }

int run_rerank(hg_ctx* c, int64_t R, bool with_ap) {
    if (!c->bpad || !c->from_floats.rows.p || !c->qf.p || !c->from_floats.rows_valid || !c->qf_resident)
        return fail(HG_ERR_STATE, "real-valued ranking needs the float features on the GPU: load them with hg_set_database_f32 / "
                                  "hg_set_queries_f32 (option keep_floats = 1 if the database is a +-1 code)");
    if (c->idx_base != 0 || c->N != c->n_total)
        return fail(HG_ERR_STATE, "hg_topr_rerank: the context holds rows [%lld, %lld) of %lld: the re-rank needs the whole database in one context",
                    (long long)c->idx_base, (long long)(c->idx_base + c->N), (long long)c->n_total);
    if (R < 1 || R > c->N) return fail(HG_ERR_ARG, "R=%lld outside 1..N (N=%lld rows in the database)", (long long)R, (long long)c->N);
    if (c->b > HG_MAX_BITS || c->bpad > 256) return fail(HG_ERR_ARG, "hg_topr_rerank: b=%d bits (at most %d)", c->b, HG_MAX_BITS);
    if (c->N > RR_MAX_ROWS) return fail(HG_ERR_ARG, "hg_topr_rerank takes up to 2^%d rows (have %lld): a record's key keeps %d bits for the index", RR_IDX_BITS, (long long)c->N, RR_IDX_BITS);
    c->real_lists = false;
    c->lists_valid = false;
    c->want_lists = true;
    c->rr_records = c->rr_chunks = c->rr_groups_lds = c->rr_groups_global = 0;
    // exact histogram (per segment, vector ALU) and plan: t, cnt_lt, posbase; hown[d][q] is the size of group d
    HG_TRY(rerank_hist_plan(c, R));
    const Geo g = c->geo;
    c->stage = ST_DB | ST_Q;                           // (the per-segment histograms become prefixes: no ST_HIST for a later hg_plan)
    c->t_begin(KI_RR_SCAN);
    hipLaunchKernelGGL(k_rr_scan, dim3(grid_for((i64)g.NB * g.Qpad)), dim3(256), 0, c->stream, c->hist.as<u32>(), c->t.as<int>(), g);
    c->t_end();
    HG_TRY(c->check_launch("k_rr_scan"));
    HG_TRY(c->rr_base.reserve((size_t)g.Qpad * 8 + 16));
    HG_TRY(c->rr_msz.reserve((size_t)g.Qpad * 4));
    hipLaunchKernelGGL(k_rr_sizes, dim3(grid_for(g.Q)), dim3(256), 0, c->stream, c->t.as<int>(), c->cnt_lt.as<u32>(), c->hown.as<u32>(), c->rr_msz.as<u32>(), g);
    HG_TRY(c->check_launch("k_rr_sizes"));
    // the one synchronisation: the M_q come home, the host cuts the queries into chunks whose records fit the budget
    std::vector<u32> msz((size_t)g.Q);
    int plan_err = 0;
    HG_HIP(hipMemcpyAsync(msz.data(), c->rr_msz.p, (size_t)g.Q * 4, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(hipMemcpyAsync(&plan_err, c->err.p, 4, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    if (plan_err) return fail(HG_ERR_HIP, "hg_topr_rerank: internal error, the plan found fewer than R rows");
    const u64 budget = (u64)(c->opt.dense_budget_mb > 0 ? c->opt.dense_budget_mb : 1) << 20;
    struct Chunk { int q0, nq; u64 recs; };
    std::vector<Chunk> chunks;
    std::vector<u64> base((size_t)g.Q);
    u64 total = 0, largest = 0;
    bool beyond_lds = false;
    for (int q = 0; q < g.Q; ++q) {
        const u64 m = msz[q];
        total += m;
        if (m > (u64)RR_LDS_KEYS) beyond_lds = true;      // (a group of it may need the second buffer)
        if (chunks.empty() || (chunks.back().recs + m) * 16 > budget) chunks.push_back(Chunk{q, 0, 0});   // (a query beyond the budget: a chunk of one)
        base[q] = chunks.back().recs;
        chunks.back().nq += 1;
        chunks.back().recs += m;
        if (chunks.back().recs > largest) largest = chunks.back().recs;
    }
    const size_t slots = (size_t)g.Q * g.R;
    HG_TRY(c->rr_recs.reserve((size_t)largest * 8));
    if (beyond_lds) HG_TRY(c->rr_tmp.reserve((size_t)largest * 8));
    HG_TRY(c->rr_cnt.reserve(16));
    HG_TRY(c->out_idx.reserve(slots * 4));
    HG_TRY(c->out_dist.reserve(slots));
    HG_TRY(c->rr_scores.reserve(slots * 4));
    HG_TRY(c->mbits.reserve((size_t)g.Q * c->RW * 8));
    HG_HIP(hipMemcpyAsync(c->rr_base.p, base.data(), (size_t)g.Q * 8, hipMemcpyHostToDevice, c->stream));
    HG_HIP(hipMemsetAsync(c->rr_cnt.p, 0, 16, c->stream));
    static std::atomic<unsigned long long> lds_allowed{0};
    if (!(lds_allowed.load() >> (c->device & 63) & 1ull)) {
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rr_order), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_allowed.fetch_or(1ull << (c->device & 63));
    }
    const RerankOut o{c->out_idx.as<u32>(), c->out_dist.as<u8>(), c->rr_scores.as<float>(), c->rr_cnt.as<unsigned long long>()};
    for (const Chunk& ch : chunks) {
        RerankArgs a{c->t.as<int>(), c->cnt_lt.as<u32>(), c->hown.as<u32>(), c->posbase.as<u32>(), c->rr_base.as<u64>(),
                     c->rr_recs.as<u64>(), beyond_lds ? c->rr_tmp.as<u64>() : nullptr, ch.q0, ch.nq};
        const int qt0 = ch.q0 / 64, qt1 = (ch.q0 + ch.nq - 1) / 64;
        HG_TRY(launch_collect(c, a, qt0, qt1 - qt0 + 1));
        // blocks per query of the scoring pass: enough to fill the device at few queries, one per 2048 records at most
        u64 mmax = 0;
        for (int q = ch.q0; q < ch.q0 + ch.nq; ++q) if (msz[q] > mmax) mmax = msz[q];
        i64 per = (i64)((mmax + 2047) / 2048), fill = ((i64)c->n_cu * 8 + ch.nq - 1) / ch.nq;
        if (per > fill) per = fill;
        if (per < 1) per = 1;
        if (per > 65535) per = 65535;
        c->t_begin(KI_RR_SCORE);
        hipLaunchKernelGGL(k_rr_score, dim3((unsigned)ch.nq, (unsigned)per), dim3(256), 0, c->stream, c->qf.as<float>(), c->from_floats.rows.as<float>(), c->bpad, a, g);
        c->t_end();
        HG_TRY(c->check_launch("k_rr_score"));
        c->t_begin(KI_RR_ORDER);
        hipLaunchKernelGGL(k_rr_order, dim3((unsigned)ch.nq), dim3(RR_THREADS), RR_LDS_BYTES, c->stream, a, o, g);
        c->t_end();
        HG_TRY(c->check_launch("k_rr_order"));
    }
    c->optimistic = false;
    c->crow = R;
    c->cap = 0;
    c->rec8 = false;
    c->ap_fused = false;
    c->ranked_local = false;
    c->last_select = SEL_NONE;
    c->last_rank = RK_NONE;
    c->lists_valid = true;
    c->stage = ST_DB | ST_Q | ST_SELECT;
    HG_TRY(do_match(c));                               // label gather through the ranked idx list (any class count)
    if (with_ap) HG_TRY(do_ap(c));
    unsigned long long counters[2] = {0, 0};
    HG_HIP(hipMemcpyAsync(counters, c->rr_cnt.p, 16, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());                                 // (base goes out of scope; the counters come home)
    c->rr_records = (i64)total;
    c->rr_chunks = (i64)chunks.size();
    c->rr_groups_lds = (i64)counters[0];
    c->rr_groups_global = (i64)counters[1];
    c->rr.finish(c, g.Q, g.Q, R);
    return HG_OK;
}

}  // namespace

extern "C" {

int hg_topr_rerank(hg_ctx* c, int64_t R) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_topr_rerank", "hg_set_database_f32 + hg_set_queries_f32"));
    return run_rerank(c, R, false);
}

int hg_map_rerank(hg_ctx* c, int64_t R, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_map_rerank", "hg_set_database_f32 + hg_set_queries_f32"));
    HG_TRY(run_rerank(c, R, true));
    return hg_get_ap(c, host_ap, host_rel);
}

int hg_get_rerank_scores(hg_ctx* c, float* host_scores) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_rerank_scores", "hg_topr_rerank / hg_map_rerank"));
    if (!(c->stage & ST_SELECT) || !c->rr.current(c))
        return fail(HG_ERR_STATE, "hg_get_rerank_scores: the last ranking was not a re-rank (hg_topr_rerank / hg_map_rerank on the tables loaded now)");
    if (!host_scores) return fail(HG_ERR_ARG, "hg_get_rerank_scores: null pointer");
    HG_HIP(hipMemcpyAsync(host_scores, c->rr_scores.p, (size_t)c->rr.Q * c->rr.dim * 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

}  // extern "C"

int preload_rerank() {   // (hg_preload: see preload_seq)
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_rr_order)));
    return HG_OK;
}

// libhashgan_amd.so -- the Hamming sequences: segment geometry, histogram -> plan -> select -> rank, in their staged
// (sharded) and one-shot forms (lib/metric.py:13-19 as a counting selection).
#include "hg_ctx.hpp"
#include "hg_select_mx.hpp"
#include "hg_select_mx3.hpp"
#include "hg_select_mx4.hpp"
#include "hg_hist_mx.hpp"

// Segment geometry of the pair passes: ~target_units wavefront-sized units.
constexpr i64 SAMPLE_RATIO = 2;      // the sampled pass works on segments this many times longer than the select pass's (= per segment pair)

Geo full_geometry(const hg_ctx* c) {
    Geo g = c->geo;
    g.Q = (int)c->Q;
    g.nQT = (int)((c->Q + 63) / 64);
    g.Qpad = g.nQT * 64;
    g.NW = c->NW; g.NB = c->NB; g.LW = c->LW;
    g.N = c->N; g.R = c->R; g.idx_base = c->idx_base;
    i64 S = (c->opt.target_units + g.nQT - 1) / g.nQT;
    // few queries: more segments than fill the GPU twice only make every query's record row longer to walk
    // (Q = 64, N = 10M: 12500 slices per query cost the rank stage 3.4 ms; 2048 cost 0.1)
    if (S > c->opt.max_segments) S = c->opt.max_segments;
    const i64 maxS = (c->N + c->opt.min_segment - 1) / c->opt.min_segment;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    i64 L = (c->N + S - 1) / S;
    const i64 lq = (c->opt.select_packed >= 3 && c->NW <= 2) ? 96 : 32;   // k_select_mx walks segments in 32-row tiles, k_select_mx3 in 48-row supertiles
    L = (L + lq - 1) / lq * lq;
    if (L < lq) L = lq;
    S = (c->N + L - 1) / L;
    if (S < 1) S = 1;
    if (c->opt.optimistic && c->opt.select_mfma && S >= 4) {
        // k_select_mx runs (S / 2) x ceil(Q / 256 or 512) equal blocks, 4 or 2 resident per CU: pick the S near the
        // target that fills a whole number of such rounds, so the last round is not a nearly empty one
        const bool qt2 = c->NW <= 4;                                // mirrors launch_select_mx_t
        const bool mx3 = c->opt.select_packed == 3 && c->NW <= 4;   // k_select_mx3 / k_select_mx4: blocks of 8 wavefronts x 64 queries, two per CU
        const int mx3_wpb = c->NW <= 2 ? M3Pack::WPB : M4Pack::WPB;
        const i64 qblk = mx3 ? 64 * mx3_wpb : qt2 ? 256 : 512;
        const i64 nQB = (c->Q + qblk - 1) / qblk;
        const i64 slots = (i64)c->n_cu * (mx3 ? 16 / mx3_wpb : qt2 ? 4 : 2);
        i64 k = (S / 2 * nQB + slots / 2) / slots;
        if (k < 1) k = 1;
        // k_rank_lean takes at most 256 slices per query.  A target beyond that (few queries: C3's 2100 ask for 496 segments)
        // is cut to the whole rounds that 256 segments fill, when that is at least one: C3 396 -> 198 segments, one round of
        // blocks instead of two, k_rank_lean instead of k_rank_cnt: 0.277 -> 0.200 ms per step
        if (mx3 && c->opt.rank_lds >= 2 && S > 256 && 128 * nQB >= slots) {
            k = 128 * nQB / slots;
            L = (c->N + 255) / 256;
            L = (L + lq - 1) / lq * lq;
            S = (c->N + L - 1) / L;                // <= 256; the search below lands on the even count that fills k rounds
        }
        i64 S2 = 2 * (slots * k / nQB);
        if (S2 > maxS) S2 = maxS / 2 * 2;
        for (; S2 >= 4; S2 -= 2) {                 // rounding L up to 16 rows can drop segments: land on an even count
            i64 L2 = (c->N + S2 - 1) / S2;
            L2 = (L2 + lq - 1) / lq * lq;
            const i64 Sr = (c->N + L2 - 1) / L2;
            if (Sr * 4 < S * 3) break;             // too far from the target: keep the plain choice
            if (Sr % 2 == 0 && Sr * 4 <= S * 5 && (Sr / 2) * nQB <= slots * k) { S = Sr; L = L2; break; }
        }
    }
    g.S = (int)S; g.L = L;
    g.nUnits = (i64)g.S * g.nQT;
    g.hist_stride = 1;
    g.hcap = 0;
    g.wpb = WPB;
    g.nBlk = (int)((g.nUnits + WPB - 1) / WPB);
    return g;
}

// The sampled pass only needs the shard total: use 2x longer segments so the per-segment
// histogram array (and its reduction) shrinks with the work.
Geo hist_geometry(const hg_ctx* c) {
    Geo g = c->geo;
    if (g.hist_stride > 1 || c->hist_pairs) {
        const i64 L = g.L * (c->hist_pairs ? 2 : SAMPLE_RATIO);
        g.L = L;
        g.S = (int)((g.N + L - 1) / L);
        g.nUnits = (i64)g.S * g.nQT;
    }
    return g;
}

// histogram on the matrix cores: blocks = (pair of segments) x (256 queries); stride in tiles of 16 rows
bool hist_mx_applies(const hg_ctx* c, int stride, bool pairs_ok) {
    if (!c->opt.hist_mfma || !c->opt.select_mfma || c->NW > 8 || c->is_sub) return false;
    {   // long segments (>= 65536 visited rows per pair) need one dword counter per query tile: with long codes the four
        // wavefronts' columns then exceed the CU's LDS -- the vector kernel, which shrinks its block, takes those
        const Geo& g = c->geo;
        const i64 tiles_per_half = ((g.L + 15) / 16 + stride - 1) / stride;
        const bool pack16 = 2 * tiles_per_half * 16 < 65536;
        if ((size_t)WPB * (pack16 ? 1 : 2) * g.NB * 32 * 4 > 160u * 1024u) return false;
    }
    return stride > 1 ? SAMPLE_RATIO == 2 : pairs_ok;
}

// The record pass of the current sequence: which kernel takes it (the launchers live in hg_pairs_valu.hip / hg_pairs_mx.hip).
// one-byte records {match, dist} (no index): only the matrix-core kernels of the bet produce them, and only when nobody wants the lists
static bool select_takes_mx(const hg_ctx* c) { return c->optimistic && c->opt.select_mfma && c->cap < (1u << MX_POS_BITS); }
static bool records_are_bytes(const hg_ctx* c) {
    return select_takes_mx(c) && c->opt.compact_records && !c->want_lists && c->LW <= 2 && c->cap % 16 == 0 && c->crow * 64 < (1ll << 31);
}
// the record rows of the coming select: Q x crow slots of one byte or eight.  (Until round 6 eight bytes were reserved either way:
// 2 GB at C2 for 0.25 GB of records -- and 14.9 GB once a class-sorted database had widened the slices, a hipMalloc that took
// between 0.4 ms and 3.5 s.)
static int reserve_records(hg_ctx* c) {
    return c->cand.reserve((size_t)c->geo.Q * (size_t)c->crow * (records_are_bytes(c) ? 1 : 8) + 64);
}

static int launch_select(hg_ctx* c, const StepReq& req) {
    const int NW = c->NW;
    const int* cut = cut_of(c, req);
    const int lw = c->LW <= 2 ? c->LW : 0;           // > 128 classes: match bits come from k_match
    const bool mx = select_takes_mx(c);
    c->rec8 = records_are_bytes(c);
    if (!c->optimistic && c->R * 4 >= c->n_total) { c->last_select = SEL_DENSE; return launch_select_dense(c, lw); }   // dense regime: most pairs are selected
    // three rows per accumulator + batched drain: codes of <= 64 bits, one-byte records (<= 128 classes).  (For <= 32 bits the
    // second k-half of every MFMA is empty, and it still beat round 2's two-rows-per-accumulator kernel: 0.69 vs 0.85 ms at b = 32.)
    if (NW <= 2 && c->opt.select_packed == 3 && c->rec8 && c->geo.L % M3_ROWS == 0 && (lw == 1 || lw == 2)) { c->last_select = SEL_MX3; return launch_select_mx3(c, lw, cut); }
    // codes of 65..128 bits: two rows per accumulator (8-bit fields) and the same drain
    if ((NW == 3 || NW == 4) && c->opt.select_packed == 3 && c->rec8 && c->geo.L % M4_ROWS == 0 && (lw == 1 || lw == 2)) { c->last_select = SEL_MX4; return launch_select_mx4(c, lw, cut); }
    if (mx) { c->last_select = SEL_MX; return launch_select_mx(c, lw, cut); }
    c->last_select = SEL_VALU;
    return launch_select_valu(c, lw, c->optimistic);
}

// rows k_hist visits with batch stride `stride` (mirrors its loop)
template <int NW> i64 sampled_rows_t(Geo g, int stride, int ratio) {
    g.hist_stride = stride;
    {
        const i64 L = g.L * ratio;                  // mirrors hist_geometry()
        g.L = L;
        g.S = (int)((g.N + L - 1) / L);
    }
    constexpr int B = Batch<NW>::rows;
    i64 total = 0;
    for (int s = 0; s < g.S; ++s) {
        const i64 lo = (i64)s * g.L, hi = lo + g.L < g.N ? lo + g.L : g.N;
        const i64 nb = (hi - lo) / B;
        total += (nb + stride - 1) / stride * B;
    }
    return total;
}
i64 sampled_rows(hg_ctx* c, int stride) {
    if (hist_mx_applies(c, stride, false)) return hist_mx_sampled_rows(c->geo, stride);
    switch (c->NW) {
        case 1: return sampled_rows_t<1>(c->geo, stride, (int)SAMPLE_RATIO);
        case 2: return sampled_rows_t<2>(c->geo, stride, (int)SAMPLE_RATIO);
        case 3: return sampled_rows_t<3>(c->geo, stride, (int)SAMPLE_RATIO);
        case 4: return sampled_rows_t<4>(c->geo, stride, (int)SAMPLE_RATIO);
        case 5: return sampled_rows_t<5>(c->geo, stride, (int)SAMPLE_RATIO);
        case 6: return sampled_rows_t<6>(c->geo, stride, (int)SAMPLE_RATIO);
        case 7: return sampled_rows_t<7>(c->geo, stride, (int)SAMPLE_RATIO);
        default: return sampled_rows_t<8>(c->geo, stride, (int)SAMPLE_RATIO);
    }
}


// =============================================================================
extern "C" {

// Compile-time A/B switch (tools/ab_build.sh): 0 = the one-shot bet's guess walks the segment pairs' planes itself, as it did before
// k_hist_i8 summed them on its way out.
#ifndef HG_GUESS_TOTALS
#define HG_GUESS_TOTALS 1
#endif

// tot_out (the one-shot bet's sampled pass): where k_hist_i8 takes the pass on a whole-database context it also leaves the planes'
// totals over the segment pairs in c->hist_tot -- *tot_out, which the caller hands to k_guess_direct (that kernel reads them and
// stores zeros over them again); nullptr where another kernel takes the pass.
static int do_hist(hg_ctx* c, int stride, bool reduce = true, bool pairs_ok = false, int hcap = 0, u64** tot_out = nullptr) {
    make_geometry(c);
    c->geo.hist_stride = stride;
    const bool mx = hist_mx_applies(c, stride, pairs_ok);
    c->geo.hcap = mx && !reduce && stride > 1 ? hcap : 0;
    c->hist_pairs = mx && stride == 1;                 // full pass per segment pair: the plan's per-segment steps follow suit
    const Geo& g = c->geo;
    const size_t plane = (size_t)g.NB * g.Qpad * 4;
    HG_TRY(c->hist.reserve(plane * g.S));
    u64* tot = nullptr;
    if (tot_out) *tot_out = nullptr;
    if (HG_GUESS_TOTALS && tot_out && mx && hist_i8_applies(c) && c->N == c->n_total && !c->is_sub) {
        const int dn = g.hcap > 0 && g.hcap < g.NB ? g.hcap : g.NB;
        const size_t cap0 = c->hist_tot.cap;
        HG_TRY(c->hist_tot.reserve((size_t)((dn + 1) / 2) * g.Qpad * 8));   // two planes to a 64-bit word
        // a new allocation (the block cache may hand the grown table the very block it gave back: same address, the bytes beyond
        // the old table never cleared), or a pass that no guess followed: never in the steady state
        if (c->hist_tot_zero != c->hist_tot.p || c->hist_tot.cap != cap0)
            HG_HIP(hipMemsetAsync(c->hist_tot.p, 0, c->hist_tot.cap, c->stream));
        c->hist_tot_zero = nullptr;                    // until the guess that clears it is enqueued
        *tot_out = tot = c->hist_tot.as<u64>();
    }
    HG_TRY(c->hown.reserve(plane + TAIL_WORDS * 4));
    if (reduce) {   // tail of the exported histogram: [0] overflow flag, [1] rows this pass visited
        const u32 visited = (u32)(stride == 1 ? g.N : sampled_rows(c, stride));
        // written by a kernel: ordered with the kernels that read it, no pageable staging memory to keep alive
        hipLaunchKernelGGL(k_set_tail, dim3(1), dim3(64), 0, c->stream, (u32*)(c->hown.as<char>() + plane), visited);
        HG_TRY(c->check_launch("k_set_tail"));
    }
    HG_TRY(mx ? launch_hist_mx(c, tot) : launch_hist(c));
    if (!reduce) { c->stage = ST_DB | ST_Q; return HG_OK; }      // the caller reads the per-segment histograms itself
    const Geo gh = hist_geometry(c);
    c->t_begin(KI_HIST_REDUCE);
    hipLaunchKernelGGL(k_hist_reduce, dim3(grid_for((i64)g.NB * g.Qpad)), dim3(256), 0, c->stream,
                       c->hist.as<u32>(), c->hown.as<u32>(), gh);
    c->t_end();
    HG_TRY(c->check_launch("k_hist_reduce"));
    c->stage = ST_DB | ST_Q | (stride == 1 ? ST_HIST : 0);
    return HG_OK;
}

int hg_hist(hg_ctx* c) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_hist", "hg_set_database + hg_set_queries"));
    HG_TRY(do_hist(c, 1));
    return c->stage_end();
}

int hg_hist_buffer(hg_ctx* c, void** dev_ptr, int64_t* nbytes) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_hist_buffer", "hg_hist / hg_sample_hist / hg_select_candidates"));
    if (!c->hown.p) return fail(HG_ERR_STATE, "hg_hist_buffer: no histogram computed yet");
    if (dev_ptr) *dev_ptr = c->hown.p;
    if (nbytes) *nbytes = ((int64_t)c->geo.NB * c->geo.Qpad + TAIL_WORDS) * 4;
    return HG_OK;
}

extern "C++" int set_R(hg_ctx* c, int64_t R, int G, int rank) {
    if (G < 1 || rank < 0 || rank >= G) return fail(HG_ERR_ARG, "rank %d of %d", rank, G);
    if (R < 1 || R > c->n_total)
        return fail(HG_ERR_ARG, "R=%lld outside 1..N (N=%lld rows in the database)", (long long)R, (long long)c->n_total);
    c->R = R; c->G = G; c->rank = rank;
    c->lists_changed();                                // every ranking comes through here: hg_graded's tables were the previous lists'
    c->bitmap_changed();                               // ... and hg_ap_at's the previous bitmap's
    c->mbits_merged = c->mbits_in_ws_b = false;
    c->match_source = 0;                               // ... and its bits are the labels' again (hg_match_neighbours)
    c->rr.begin();                                     // ... and a re-rank's score list goes with its lists
    c->geo.R = R;
    c->RW = (R + 63) / 64;
    return HG_OK;
}

// k_plan on c->hown (full histogram, or the records' histogram in optimistic mode)
static int launch_plan(hg_ctx* c, const uint32_t* dev_hist_all) {
    const Geo& g = c->geo;
    const size_t qb = (size_t)g.Qpad * 4;
    HG_TRY(c->posbase.reserve((size_t)g.NB * qb));
    HG_TRY(c->t.reserve(qb)); HG_TRY(c->cnt_lt.reserve(qb)); HG_TRY(c->quota.reserve(qb));
    HG_TRY(c->tie_before.reserve(qb)); HG_TRY(c->n_lt.reserve(qb)); HG_TRY(c->err.reserve(16));
    HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
    Plan pl{c->t.as<int>(), c->cnt_lt.as<u32>(), c->quota.as<u32>(), c->tie_before.as<u32>(), c->n_lt.as<u32>(),
            c->posbase.as<u32>(), c->err.as<int>()};
    c->t_begin(KI_PLAN);
    hipLaunchKernelGGL(k_plan, dim3(grid_for(g.Q)), dim3(256), 0, c->stream, c->hown.as<u32>(),
                       (const u32*)dev_hist_all, c->G, c->rank, pl, g);
    c->t_end();
    return c->check_launch("k_plan");
}

// exact plan: threshold from the full histogram, then the exact record-row layout
static int do_plan(hg_ctx* c, int64_t R, const uint32_t* dev_hist_all, int G, int rank) {
    if (G > 1 && !dev_hist_all) return fail(HG_ERR_ARG, "hg_plan: G > 1 needs the gathered histograms");
    HG_TRY(set_R(c, R, G, rank));
    const Geo& g = c->geo;
    const size_t qb = (size_t)g.Qpad * 4;
    HG_TRY(launch_plan(c, dev_hist_all));
    HG_TRY(c->seglt.reserve((size_t)g.S * qb)); HG_TRY(c->segtie.reserve((size_t)g.S * qb));
    HG_TRY(c->sl_start.reserve((size_t)g.S * qb)); HG_TRY(c->sl_tie.reserve((size_t)g.S * qb));
    HG_TRY(c->sl_cnt.reserve((size_t)g.S * qb)); HG_TRY(c->tot.reserve(qb)); HG_TRY(c->failq.reserve(qb));
    HG_TRY(c->sstar.reserve(qb));
    const Geo gp = hist_geometry(c);                   // per segment -- or per segment pair after k_hist_mx (then only sstar is used)
    const int ratio = (int)(gp.L / g.L);
    c->t_begin(KI_SEG_COUNTS);
    hipLaunchKernelGGL(k_seg_counts, dim3(grid_for((i64)gp.S * g.Qpad)), dim3(256), 0, c->stream, c->hist.as<u32>(),
                       c->t.as<int>(), c->seglt.as<u32>(), c->segtie.as<u32>(), gp);
    c->t_end();
    HG_TRY(c->check_launch("k_seg_counts"));
    c->t_begin(KI_SEG_LAYOUT);
    hipLaunchKernelGGL(k_seg_layout, dim3(grid_for(g.Qpad)), dim3(256), 0, c->stream, c->seglt.as<u32>(),
                       c->segtie.as<u32>(), c->quota.as<u32>(), c->tie_before.as<u32>(), c->sl_start.as<u32>(),
                       c->sl_tie.as<u32>(), c->tot.as<u32>(), c->sstar.as<int>(), ratio, gp);
    c->t_end();
    HG_TRY(c->check_launch("k_seg_layout"));
    c->optimistic = false;
    c->crow = R;
    c->cap = 0;
    c->stage = ST_DB | ST_Q | ST_HIST | ST_PLAN;
    return HG_OK;
}

// the re-rank's first two steps (hg_rerank.hip): the exact histogram per segment on the vector ALU, then threshold and group starts
extern "C++" int rerank_hist_plan(hg_ctx* c, int64_t R) {
    HG_TRY(do_hist(c, 1));
    HG_TRY(set_R(c, R, 1, 0));
    return launch_plan(c, nullptr);
}

static int plan_overrun(hg_ctx* c) {                  // k_plan's verdict on an exact sequence
    c->stage = ST_DB | ST_Q | ST_HIST;
    return fail(HG_ERR_ARG, "R=%lld exceeds the rows present in the gathered histograms", (long long)c->R);
}
static int check_plan_flag(hg_ctx* c) {
    int err = 0;
    HG_TRY(read_plan_flag(c, &err));
    return err ? plan_overrun(c) : HG_OK;
}

int hg_plan(hg_ctx* c, int64_t R, const uint32_t* dev_hist_all, int G, int rank) {
    HG_TRY(need(c, ST_HIST, "hg_plan", "hg_hist"));
    // a one-shot exact call may have left histograms per segment PAIR (k_hist_mx); the staged select lays its slices out
    // per segment
    if (c->hist_pairs) return fail(HG_ERR_STATE, "hg_plan called before hg_hist (the last histogram pass belonged to a one-shot call)");
    HG_TRY(do_plan(c, R, dev_hist_all, G, rank));
    // the device flag says "R exceeds the rows in the gathered histograms"; R <= n_total was checked on
    // the host already, so an unsynchronised caller loses nothing by skipping the read-back
    return c->opt.stage_sync ? check_plan_flag(c) : HG_OK;
}

// The buffers a ranking writes: the match bitmap, and the idx / dist lists where they are written (a token 16 bytes where not).
// fill: the lists' slots start as IDX_NONE / 0xFF -- the ones that are another shard's, or past this shard's own records.
enum ListFill { FILL_NONE, FILL_IDX, FILL_BOTH };
static int reserve_lists(hg_ctx* c, bool lists, ListFill fill) {
    const Geo& g = c->geo;
    const size_t slots = (size_t)g.Q * g.R;
    HG_TRY(c->mbits.reserve((size_t)g.Q * c->RW * 8));
    HG_TRY(c->out_idx.reserve(lists ? slots * 4 : 16));
    HG_TRY(c->out_dist.reserve(lists ? slots : 16));
    if (lists && fill != FILL_NONE) HG_HIP(hipMemsetAsync(c->out_idx.p, 0xFF, slots * 4, c->stream));
    if (lists && fill == FILL_BOTH) HG_HIP(hipMemsetAsync(c->out_dist.p, 0xFF, slots, c->stream));
    return HG_OK;
}

// record pass + ordering (+ gather-based label match when labels are too wide for the record pass)
static int do_select(hg_ctx* c, const StepReq& req) {
    const bool lists = lists_needed(c);
    HG_TRY(reserve_records(c));
    HG_TRY(reserve_lists(c, lists, c->G > 1 ? FILL_BOTH : FILL_NONE));
    HG_TRY(launch_select(c, req));
    // one block per query: verify (optimistic) + plan + order.  Exact single-shard rows hold precisely the top R, so the same counting plan reproduces t and the bucket starts.
    HG_TRY(c->optimistic || c->G == 1 ? launch_rank(c, RANK_WHOLE, req) : launch_order(c));
    c->lists_valid = lists;
    c->stage = (c->stage & (ST_DB | ST_Q | ST_HIST | ST_PLAN)) | ST_PLAN | ST_SELECT;
    if (c->LW <= 2) c->stage |= ST_MATCH;                 // match bits came with the records
    else HG_TRY(do_match(c));
    return HG_OK;
}

int hg_select(hg_ctx* c) {
    HG_TRY(need(c, ST_PLAN, "hg_select", "hg_plan"));
    c->want_lists = c->opt.staged_lists != 0;
    HG_TRY(do_select(c, StepReq{}));
    return c->stage_end();
}

// ---- staged optimistic sequence (multi-shard): sample -> [gather] -> guess -> candidates ->
// [gather] -> rank.  Mirrors the one-shot bet, with the two histogram exchanges made explicit.
// Sampling stride of the bet, in row batches.  One row batch in 24: a fixed 4 % of a pass (with the
// matrix-core select the sampling pass is a visible share of the step; 16 -> 24 trades 0.05 ms of it for
// ~3 % more surplus records).  The
// guess's safety margin is relative to sqrt(sampled hits), so a small R only means relatively more
// surplus records (R = 100: ~3.5 R of them) -- still far cheaper than a full histogram pass.
// Capacity of a (segment, query) slice of the bet: the budgeted mean + 6 sigma, never more than the segment's rows, and
// the record rows of all queries together stay below 64 GB ("cap_boost" may ask for more than is sensible).
static u32 slice_capacity(const hg_ctx* c, double mean) {
    const Geo& g = c->geo;
    u32 cap = (u32)std::ceil(mean + 6.0 * std::sqrt(mean) + 16.0);
    cap = (cap + 15u) & ~15u;                      // a multiple of the compact records' ring (16) and flush piece (8)
    const u32 whole = (u32)((g.L + 15) & ~15ll);
    if (cap > whole) cap = whole;
    while (cap > 64u && (double)g.Q * (double)g.S * (double)cap * 8.0 > 64e9) cap = (cap / 2u + 15u) & ~15u;
    return cap;
}
// what every guess writes: the cut, the slices' bookkeeping, the queries whose slices overflowed
static int reserve_guess(hg_ctx* c) {
    const Geo& g = c->geo;
    const size_t qb = (size_t)g.Qpad * 4;
    HG_TRY(c->tguess.reserve(qb)); HG_TRY(c->sl_start.reserve((size_t)g.S * qb)); HG_TRY(c->sl_tie.reserve((size_t)g.S * qb));
    HG_TRY(c->sl_cnt.reserve((size_t)g.S * qb)); HG_TRY(c->tot.reserve(qb)); HG_TRY(c->failq.reserve(qb));
    return c->sstar.reserve(qb);
}
// the guess is in force: slices budgeted for `mean` records each
static void adopt_guess(hg_ctx* c, double mean) {
    c->optimistic = true;
    c->cap = slice_capacity(c, mean);
    c->crow = (i64)c->geo.S * c->cap;
    c->stage = ST_DB | ST_Q | ST_PLAN;
}
// a guessed cut keeps at most ~2.6 R rows over ALL shards; a shard's share is proportional to its size,
// with the same 6-sigma headroom per slice as the one-shot bet
static double staged_mean(const hg_ctx* c, int64_t R) {
    const double share = (double)c->N / (double)c->n_total;
    return 0.1 * (double)c->opt.cand_budget_x10 * (double)c->cap_boost * (double)R * share / (double)c->geo.S;
}

static int auto_stride(hg_ctx* c, int64_t R) {
    (void)R;
    return c->opt.sample_stride > 0 ? (int)c->opt.sample_stride : 24;
}

int hg_bet_eligible(hg_ctx* c, int64_t R, int world, int* eligible) {
    if (!c || !eligible || world < 1) return fail(HG_ERR_ARG, "hg_bet_eligible: bad argument");
    // only quantities every rank shares: options, R, the size of the whole database, the world size -- and the count of
    // consecutive SHARDED bets lost, which only hg_merge_ranked / hg_rank / hg_bet_verdict touch, with a verdict that is
    // computed from gathered data and therefore the same on every rank (one-shot calls keep their own counter)
    const int stride = auto_stride(c, R);
    const i64 per_shard = c->n_total / world;
    *eligible = c->opt.optimistic && c->shard_bet_fail < 2 && stride >= 2 && R * 8 <= c->n_total && per_shard >= 65536;
    return HG_OK;
}

int hg_sample_hist(hg_ctx* c, int64_t R) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_sample_hist", "hg_set_database + hg_set_queries"));
    const int stride = auto_stride(c, R);
    if (stride < 2) return fail(HG_ERR_ARG, "hg_sample_hist: R=%lld is too small to sample for", (long long)R);
    if (c->beyond.p) HG_HIP(hipMemsetAsync(c->beyond.p, 0, 4, c->stream));      // (a new bet: "cut_beyond_planes" is about this one)
    HG_TRY(do_hist(c, stride));
    return c->stage_end();
}

int hg_guess(hg_ctx* c, int64_t R, const uint32_t* dev_hist_all, int G, int rank) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_guess", "hg_sample_hist"));
    if (G > 1 && !dev_hist_all) return fail(HG_ERR_ARG, "hg_guess: G > 1 needs the gathered sample histograms");
    HG_TRY(set_R(c, R, G, rank));
    const Geo& g = c->geo;
    HG_TRY(reserve_guess(c));
    HG_HIP(hipMemsetAsync(c->failq.p, 0, (size_t)g.Qpad * 4, c->stream));
    c->t_begin(KI_GUESS);
    const Geo gh = hist_geometry(c);                   // the sampled pass ran on coarser segments
    hipLaunchKernelGGL(k_guess, dim3(grid_for(g.Q)), dim3(256), 0, c->stream, c->hown.as<u32>(), (const u32*)dev_hist_all, G,
                       rank, c->hist.as<u32>(), gh.S, (int)(gh.L / g.L), (double)c->opt.guess_sigma, (i64)c->n_total,
                       c->tguess.as<int>(), c->sstar.as<int>(), g);
    c->t_end();
    HG_TRY(c->check_launch("k_guess"));
    adopt_guess(c, staged_mean(c, R));
    return c->stage_end();
}

int hg_select_candidates(hg_ctx* c) {
    HG_TRY(need(c, ST_PLAN, "hg_select_candidates", "hg_guess"));
    if (!c->optimistic) return fail(HG_ERR_STATE, "hg_select_candidates: no guess in force (use hg_select after hg_plan)");
    const Geo& g = c->geo;
    c->want_lists = c->opt.staged_lists != 0 || c->LW > 2;  // decides the record format (hg_rank places them)
    HG_TRY(reserve_records(c));
    HG_TRY(launch_select(c, StepReq{}));
    const size_t plane = (size_t)g.NB * g.Qpad * 4;
    HG_HIP(hipMemsetAsync(c->hown.as<char>() + plane, 0, TAIL_WORDS * 4, c->stream));
    HG_TRY(launch_rank(c, RANK_COUNT, StepReq{}));                // per-wave and shard histograms of the records
    return c->stage_end();
}

// Sharded bet, AP only: select, then rank THIS shard's records locally (rank kernels' mode 3).  What leaves the
// shard is its per-distance record counts (hg_hist_buffer) and its match bitmap in local rank order
// (hg_match_buffer); hg_merge_ranked stitches the global bitmap from the gathered pairs.  One exchange and one
// pass over the records fewer than hg_select_candidates + hg_rank.
int hg_select_ranked(hg_ctx* c) {
    HG_TRY(need(c, ST_PLAN, "hg_select_ranked", "hg_guess"));
    if (!c->optimistic) return fail(HG_ERR_STATE, "hg_select_ranked: no guess in force");
    const Geo& g = c->geo;
    // > 128 classes: the record pass leaves the match bit 0 (launch_select_nw instantiates LW = 0); the local bitmap
    // then comes from k_match gathering the labels through the LOCAL ranked index list, so that list is kept
    const bool wide = c->LW > 2;
    c->want_lists = wide;
    HG_TRY(reserve_records(c));
    HG_TRY(reserve_lists(c, wide, FILL_IDX));          // slots past the shard's own records: IDX_NONE
    HG_TRY(c->err.reserve(16));
    HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
    HG_TRY(launch_select(c, StepReq{}));
    const size_t plane = (size_t)g.NB * g.Qpad * 4;
    HG_HIP(hipMemsetAsync(c->hown.as<char>() + plane, 0, TAIL_WORDS * 4, c->stream));
    HG_TRY(launch_rank(c, RANK_LOCAL, StepReq{}));
    c->lists_valid = false;
    c->ranked_local = true;
    c->stage = ST_DB | ST_Q | ST_PLAN | ST_SELECT;
    if (wide) HG_TRY(do_match(c));                    // metric.py:17-19 through the local list
    c->want_lists = false;
    c->stage = ST_DB | ST_Q | ST_PLAN | ST_MATCH;     // hg_match_buffer hands out the LOCAL bitmap until the merge
    return c->stage_end();
}

static int merge_ranked_range(hg_ctx* c, const uint32_t* dev_hist_all, const uint64_t* dev_bits_all, int G, i64 q0, i64 nq, const char* who,
                              const MergeSrc* routed = nullptr) {
    HG_TRY(need(c, ST_MATCH, who, "hg_select_ranked"));
    if (!c->ranked_local) return fail(HG_ERR_STATE, "%s: hg_select_ranked has not run", who);
    if (G < 1 || G > 64 || (G > 1 && (!dev_hist_all || !dev_bits_all)))
        return fail(HG_ERR_ARG, "%s: bad argument (1 <= G <= 64, gathered buffers for G > 1)", who);
    const Geo& g = c->geo;
    if (q0 < 0 || nq < 0 || q0 + nq > g.Q) return fail(HG_ERR_ARG, "%s: queries [%lld, %lld) of %d", who, (long long)q0, (long long)(q0 + nq), g.Q);
    HG_TRY(c->mbits2.reserve((size_t)g.Q * c->RW * 8));
    HG_TRY(c->qbad.reserve((size_t)g.Qpad * 4));
    const u32* hall = G > 1 || routed ? (const u32*)dev_hist_all : c->hown.as<u32>();
    const u64* ball = G > 1 || routed ? (const u64*)dev_bits_all : c->mbits.as<u64>();
    const size_t rows_lds = (size_t)WPB * G * c->RW * 8;       // the G local bitmap rows of a block's four queries
    const size_t cnt_lds = (size_t)WPB * G * g.NB * 4;         // their per-distance counts: at most 4 * 64 * 256 * 4 = 256 KiB ...
    const int use_lds = rows_lds + cnt_lds <= 64 * 1024;
    const size_t merge_lds = (use_lds ? rows_lds : 0) + cnt_lds;
    if (merge_lds > 160 * 1024)                                // ... which only many shards of long codes reach
        return fail(HG_ERR_ARG, "hg_merge_ranked: G=%d shards of %d-bit codes need %zu bytes of LDS per block (160 KiB available): "
                                "use the staged sequence (hg_select_candidates / hg_rank)", G, c->b, merge_lds);
    if (merge_lds > 64 * 1024)
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_merge_ranked), hipFuncAttributeMaxDynamicSharedMemorySize, (int)merge_lds));
    c->t_begin(KI_MERGE);
    if (nq > 0)
    {   // all-gathered whole tables by default; `routed`: the owner's blocks of an all-to-all (hg_merge_ap_owned)
        const MergeSrc whole{(i64)g.NB * g.Qpad + TAIL_WORDS, g.Qpad, (i64)g.NB * g.Qpad, (i64)g.Q * c->RW, 0};
        hipLaunchKernelGGL(k_merge_ranked, dim3(grid_for(nq, WPB)), dim3(256), merge_lds, c->stream, hall, ball, G,
                           c->RW, c->mbits2.as<u64>(), c->err.as<int>(), c->qbad.as<u32>(), use_lds, g, (int)q0, (int)(q0 + nq), routed ? *routed : whole);
    }
    c->t_end();
    HG_TRY(c->check_launch("k_merge_ranked"));
    std::swap(c->mbits, c->mbits2);                    // the global bitmap is what hg_ap and hg_get_match see
    c->ranked_local = false;
    c->bitmap_changed();
    c->mbits_merged = q0 == 0 && nq == g.Q;
    c->G = G;
    return HG_OK;
}

// The verdict of a sharded bet is known (computed from gathered data: the same on every rank): count it.  A lost bet sends the
// caller back to the tables.  Returns `lost`; what else a win or a loss means is the entry point's.
static bool count_verdict(hg_ctx* c, int lost) {
    c->bet_runs++;
    if (lost) { c->bet_fallbacks++; c->shard_bet_fail++; c->stage = ST_DB | ST_Q; }
    else c->shard_bet_fail = 0;
    return lost != 0;
}
// option "defer_verdict": the caller goes on as if the bet held (match bits, exchange, AP) and asks hg_bet_verdict at the end,
// together with its final download: no host round trip in the middle of the step
static void defer_verdict(hg_ctx* c, int* bet_lost) { *bet_lost = -1; c->verdict_pending = true; c->verdict_known = false; }

int hg_merge_ranked(hg_ctx* c, const uint32_t* dev_hist_all, const uint64_t* dev_bits_all, int G, int* bet_lost) {
    if (!bet_lost) return fail(HG_ERR_ARG, "hg_merge_ranked: null argument");
    HG_TRY(merge_ranked_range(c, dev_hist_all, dev_bits_all, G, 0, c ? c->geo.Q : 0, "hg_merge_ranked"));
    if (c->opt.defer_verdict) {
        defer_verdict(c, bet_lost);
        c->stage = ST_DB | ST_Q | ST_PLAN | ST_SELECT | ST_MATCH;
        return c->stage_end();
    }
    HG_TRY(read_plan_flag(c, bet_lost));
    if (!count_verdict(c, *bet_lost)) c->stage = ST_DB | ST_Q | ST_PLAN | ST_SELECT | ST_MATCH;
    return HG_OK;
}

// hg_rank's placement stands (the bet held, or its verdict is deferred): the lists and match bits are the context's
static int adopt_ranking(hg_ctx* c) {
    c->lists_valid = c->want_lists;
    c->stage = ST_DB | ST_Q | ST_PLAN | ST_SELECT;
    if (c->LW <= 2) c->stage |= ST_MATCH;
    else HG_TRY(do_match(c));
    return HG_OK;
}

int hg_rank(hg_ctx* c, const uint32_t* dev_hist_all, int G, int rank, int* bet_lost) {
    HG_TRY(need(c, ST_PLAN, "hg_rank", "hg_select_candidates"));
    if (!c->optimistic) return fail(HG_ERR_STATE, "hg_rank: no guess in force");
    if (!bet_lost || G < 1 || (G > 1 && !dev_hist_all)) return fail(HG_ERR_ARG, "hg_rank: bad argument");
    c->G = G; c->rank = rank;
    c->want_lists = c->opt.staged_lists != 0 || c->LW > 2;
    HG_TRY(reserve_lists(c, c->want_lists, G > 1 ? FILL_BOTH : FILL_NONE));
    HG_TRY(launch_plan(c, dev_hist_all));
    HG_TRY(launch_rank(c, RANK_PLACE, StepReq{}));                // placement with the shared plan
    if (c->opt.defer_verdict) {
        defer_verdict(c, bet_lost);
        HG_TRY(adopt_ranking(c));
        return c->stage_end();
    }
    HG_TRY(read_plan_flag(c, bet_lost));
    if (count_verdict(c, *bet_lost)) return HG_OK;
    HG_TRY(adopt_ranking(c));
    return c->sync();
}

int hg_bet_verdict(hg_ctx* c, int* bet_lost) {
    if (!c || !bet_lost) return fail(HG_ERR_ARG, "hg_bet_verdict: null argument");
    if (!c->verdict_pending) return fail(HG_ERR_STATE, "hg_bet_verdict: no deferred hg_rank outstanding");
    c->verdict_pending = false;
    int flag = 0;
    if (c->verdict_known) flag = c->verdict_flag;      // came over with hg_get_ap's download
    else HG_TRY(read_plan_flag(c, &flag));
    c->verdict_known = false;
    *bet_lost = flag;
    if (count_verdict(c, flag)) c->lists_valid = false;
    return HG_OK;
}

// What follows the merge of this rank's queries [q0, q0 + nq): their AP (k_ap's block index is the query), then {AP, hits} and the
// verdict packed into `part`, `width` queries wide.
static int ap_pack_part(hg_ctx* c, i64 q0, i64 nq, i64 width, void** dev_part, int64_t* nbytes) {
    const Geo& g = c->geo;
    c->stage = ST_DB | ST_Q | ST_PLAN | ST_SELECT | ST_MATCH;
    HG_TRY(c->ap.reserve((size_t)g.Q * 8));
    HG_TRY(c->rel.reserve((size_t)g.Q * 4));
    HG_TRY(do_ap_range(c, q0, nq));
    if (!(q0 == 0 && nq == g.Q)) c->stage &= ~(unsigned)ST_MATCH;   // the merged bitmap holds rows [q0, q0 + nq) only: hg_get_match has nothing whole to hand out
    const size_t pb = (size_t)(width + 1) * 16;
    HG_TRY(c->part.reserve(pb));
    hipLaunchKernelGGL(k_pack_part, dim3(grid_for(width + 1)), dim3(256), 0, c->stream, c->ap.as<double>(), c->rel.as<u32>(),
                       c->err.as<int>(), q0, nq, width, c->part.as<double>());
    HG_TRY(c->check_launch("k_pack_part"));
    *dev_part = c->part.p; *nbytes = (int64_t)pb;
    return c->stage_end();
}

// The sharded bet with the per-query stages SPLIT over the ranks: after the all-gather of record counts and local bitmaps
// every rank merges and evaluates only its own queries [q0, q0 + nq) (instead of all Q on every rank), packs {AP, hits}
// and its verdict into `part`; one small all-gather later hg_unpack_parts gives every rank all of it.
int hg_merge_ap_part(hg_ctx* c, const uint32_t* dev_hist_all, const uint64_t* dev_bits_all, int G, int64_t q0, int64_t nq,
                     int64_t width, void** dev_part, int64_t* nbytes) {
    if (!c || !dev_part || !nbytes || width < nq || width < 1) return fail(HG_ERR_ARG, "hg_merge_ap_part: bad argument");
    HG_TRY(merge_ranked_range(c, dev_hist_all, dev_bits_all, G, q0, nq, "hg_merge_ap_part"));
    return ap_pack_part(c, q0, nq, width, dev_part, nbytes);
}

int hg_unpack_parts(hg_ctx* c, const void* dev_parts_all, int G, int64_t width, double* host_ap, int64_t* host_rel, int* bet_lost) {
    if (!c || !dev_parts_all || G < 1 || width < 1 || !host_ap || !host_rel || !bet_lost) return fail(HG_ERR_ARG, "hg_unpack_parts: bad argument");
    HG_TRY(c->use());
    const i64 Q = c->geo.Q;
    const size_t pb = (size_t)(width + 1) * 16, total = pb * (size_t)G;
    HG_TRY(ensure_pin(c, total));
    HG_HIP(hipMemcpyAsync(c->pin, dev_parts_all, total, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    int flag = 0;
    i64 done = 0;
    for (int r = 0; r < G; ++r) {
        const double* p = (const double*)((const char*)c->pin + (size_t)r * pb);
        const i64 n = (i64)p[2 * width + 1];
        if (n < 0 || n > width || done + n > Q) return fail(HG_ERR_ARG, "hg_unpack_parts: rank %d reports %lld queries (width %lld, %lld of %lld placed)",
                                                            r, (long long)n, (long long)width, (long long)done, (long long)Q);
        flag |= p[2 * width] != 0.0;
        for (i64 i = 0; i < n; ++i) { host_ap[done + i] = p[2 * i]; host_rel[done + i] = (int64_t)p[2 * i + 1]; }
        done += n;
    }
    if (done != Q) return fail(HG_ERR_ARG, "hg_unpack_parts: the parts cover %lld of %lld queries", (long long)done, (long long)Q);
    *bet_lost = flag;
    c->verdict_pending = false;
    c->verdict_known = false;
    if (count_verdict(c, flag)) c->lists_valid = false;
    return HG_OK;
}

// ---- the sharded bet with its exchanges routed by query owner (all-to-all instead of all-gather): see k_pack_sample_owner ----
static int owners_for(hg_ctx* c, int G, Owners* w, const char* who) {
    if (G < 1 || G > 64) return fail(HG_ERR_ARG, "%s: 1 <= G <= 64", who);
    *w = make_owners(c->geo.Q, G);
    return HG_OK;
}
static int sample_planes(const hg_ctx* c) { const int NB = c->geo.NB; return NB / 2 + 2 < NB ? NB / 2 + 2 : NB; }   // what a guess can need (enqueue_optimistic)

int hg_pack_sample_by_owner(hg_ctx* c, int G, void** dev_ptr, int64_t* nbytes_per_peer) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_pack_sample_by_owner", "hg_sample_hist"));
    if (!dev_ptr || !nbytes_per_peer || !c->hown.p) return fail(HG_ERR_ARG, "hg_pack_sample_by_owner: bad argument (hg_sample_hist first)");
    Owners w;
    HG_TRY(owners_for(c, G, &w, "hg_pack_sample_by_owner"));
    const Geo& g = c->geo;
    const int HC = sample_planes(c);
    const i64 blk = 4 + (i64)HC * w.width;
    HG_TRY(c->obuf[0].reserve((size_t)G * blk * 4));
    hipLaunchKernelGGL(k_pack_sample_owner, dim3(grid_for((i64)G * HC * w.width)), dim3(256), 0, c->stream, c->hown.as<u32>(), w, HC,
                       c->obuf[0].as<u32>(), g);
    HG_TRY(c->check_launch("k_pack_sample_owner"));
    *dev_ptr = c->obuf[0].p;
    *nbytes_per_peer = blk * 4;
    return c->stage_end();
}

int hg_guess_owned(hg_ctx* c, int64_t R, const void* dev_recv, int G, int rank, void** dev_ptr, int64_t* nbytes_per_peer) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_guess_owned", "hg_sample_hist"));
    if (!dev_recv || !dev_ptr || !nbytes_per_peer) return fail(HG_ERR_ARG, "hg_guess_owned: null argument");
    Owners w;
    HG_TRY(owners_for(c, G, &w, "hg_guess_owned"));
    HG_TRY(set_R(c, R, G, rank));
    const Geo& g = c->geo;
    HG_TRY(c->obuf[1].reserve((size_t)G * w.width * 16));
    c->t_begin(KI_GUESS);
    hipLaunchKernelGGL(k_guess_owner, dim3(grid_for(w.width)), dim3(256), 0, c->stream, (const u32*)dev_recv, w, sample_planes(c),
                       owner_nq(w, rank), (double)c->opt.guess_sigma, (i64)c->n_total, c->obuf[1].as<u32>(), g);
    c->t_end();
    HG_TRY(c->check_launch("k_guess_owner"));
    *dev_ptr = c->obuf[1].p;
    *nbytes_per_peer = (int64_t)w.width * 16;
    return c->stage_end();
}

int hg_guess_finish(hg_ctx* c, int64_t R, const void* dev_answers, int G, int rank) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_guess_finish", "hg_sample_hist"));
    if (!dev_answers) return fail(HG_ERR_ARG, "hg_guess_finish: null argument");
    Owners w;
    HG_TRY(owners_for(c, G, &w, "hg_guess_finish"));
    HG_TRY(set_R(c, R, G, rank));
    const Geo& g = c->geo;
    HG_TRY(reserve_guess(c));
    HG_HIP(hipMemsetAsync(c->failq.p, 0, (size_t)g.Qpad * 4, c->stream));
    HG_TRY(c->beyond.reserve(4));
    HG_HIP(hipMemsetAsync(c->beyond.p, 0, 4, c->stream));
    const Geo gh = hist_geometry(c);                   // the sampled pass ran on coarser segments
    c->t_begin(KI_GUESS);
    hipLaunchKernelGGL(k_guess_finish, dim3(grid_for(g.Q)), dim3(256), 0, c->stream, (const u32*)dev_answers, w, c->hist.as<u32>(), gh.S,
                       (int)(gh.L / g.L), c->tguess.as<int>(), c->sstar.as<int>(), c->beyond.as<u32>(), g);
    c->t_end();
    HG_TRY(c->check_launch("k_guess_finish"));
    adopt_guess(c, staged_mean(c, R));
    return c->stage_end();
}

int hg_pack_ranked_by_owner(hg_ctx* c, int G, void** dev_ptr, int64_t* nbytes_per_peer) {
    HG_TRY(need(c, ST_MATCH, "hg_pack_ranked_by_owner", "hg_select_ranked"));
    if (!c->ranked_local) return fail(HG_ERR_STATE, "hg_pack_ranked_by_owner: hg_select_ranked has not run");
    if (!dev_ptr || !nbytes_per_peer) return fail(HG_ERR_ARG, "hg_pack_ranked_by_owner: null argument");
    Owners w;
    HG_TRY(owners_for(c, G, &w, "hg_pack_ranked_by_owner"));
    const Geo& g = c->geo;
    const i64 cw = ((i64)g.NB * w.width + 1) & ~1ll;
    const i64 blk32 = cw + TAIL_WORDS + 2 * (i64)w.width * c->RW;
    HG_TRY(c->obuf[0].reserve((size_t)G * blk32 * 4));
    const i64 items = (i64)G * (cw + TAIL_WORDS) + (i64)G * w.width * c->RW;
    hipLaunchKernelGGL(k_pack_ranked_owner, dim3(grid_for(items)), dim3(256), 0, c->stream, c->hown.as<u32>(), c->mbits.as<u64>(), w, c->RW, cw,
                       c->obuf[0].as<u32>(), g);
    HG_TRY(c->check_launch("k_pack_ranked_owner"));
    *dev_ptr = c->obuf[0].p;
    *nbytes_per_peer = blk32 * 4;
    return c->stage_end();
}

int hg_merge_ap_owned(hg_ctx* c, const void* dev_recv, int G, int rank, void** dev_part, int64_t* nbytes) {
    if (!c || !dev_recv || !dev_part || !nbytes) return fail(HG_ERR_ARG, "hg_merge_ap_owned: null argument");
    Owners w;
    HG_TRY(owners_for(c, G, &w, "hg_merge_ap_owned"));
    if (rank < 0 || rank >= G) return fail(HG_ERR_ARG, "hg_merge_ap_owned: rank %d of %d", rank, G);
    const Geo& g = c->geo;
    const i64 cw = ((i64)g.NB * w.width + 1) & ~1ll;
    const i64 blk32 = cw + TAIL_WORDS + 2 * (i64)w.width * c->RW;
    const i64 q0 = owner_q0(w, rank), nq = owner_nq(w, rank);
    const MergeSrc ms{blk32, w.width, cw, blk32 / 2, (int)q0};
    const u32* hall = (const u32*)dev_recv;
    const u64* ball = (const u64*)(hall + cw + TAIL_WORDS);
    HG_TRY(merge_ranked_range(c, hall, ball, G, q0, nq, "hg_merge_ap_owned", &ms));
    return ap_pack_part(c, q0, nq, w.width, dev_part, nbytes);
}

// ---- one-shot forms: every stage enqueued back to back, one synchronisation ----
// Optimistic bet (single shard, R << N): instead of a full histogram pass, sample
// every stride-th row batch, guess the threshold a few sigma high, select a
// superset with it, then verify: the records' exact histogram must contain R rows
// and no slice may have overflowed.  The verified result is identical to the
// exact path's; a failed bet reruns the exact path.
static bool optimistic_eligible(hg_ctx* c, int64_t R, int* stride_out) {
    if (!c->opt.optimistic || c->bet_consecutive_fail >= 2) return false;
    if (R * 8 > c->N || c->N < 65536) return false;
    make_geometry(c);
    const int stride = auto_stride(c, R);
    if (stride < 2) return false;
    *stride_out = stride;
    return true;
}

// R = N on one shard (the reference's CIFAR-10 setting): every row is a member of every ranked list, so nothing
// has to be selected or written down -- the ranking kernel walks the shard's rows directly, computing each row's
// distance and match bit from the codes and labels in both of its passes (counting, then stable placement).
static int enqueue_all_rows(hg_ctx* c, int64_t R, const StepReq& req, StepReq::Rows rows) {
    make_geometry(c);
    HG_TRY(set_R(c, R, 1, 0));
    const Geo& g = c->geo;
    const size_t qb = (size_t)g.Qpad * 4;
    HG_TRY(c->err.reserve(16)); HG_TRY(c->failq.reserve(qb)); HG_TRY(c->tot.reserve(qb)); HG_TRY(c->sl_cnt.reserve(qb));
    HG_TRY(c->cand.reserve(64));
    HG_TRY(reserve_lists(c, c->want_lists, FILL_NONE));
    HG_HIP(hipMemsetAsync(c->err.p, 0, 4, c->stream));
    c->optimistic = false;
    c->crow = R;
    c->cap = 0;
    c->rec8 = false;
    c->last_select = SEL_NONE;                         // no record pass at all
    StepReq walk = req;
    walk.rows = rows;
    HG_TRY(launch_rank(c, RANK_WHOLE, walk));
    c->lists_valid = c->want_lists;
    c->stage = ST_DB | ST_Q | ST_PLAN | ST_SELECT | ST_MATCH;
    return HG_OK;
}

static int enqueue_exact(hg_ctx* c, int64_t R, const StepReq& req) {
    // N/8 < R <= N through the byte matrix (k_dense_bytes + k_rank_dense: R = N/2 of N = 1M 68.8 -> 16.3 ms, C1 0.35 -> 0.19 ms)
    if (R * 8 > c->N && c->opt.all_rows_shortcut && rank_dense_fits(c)) return enqueue_all_rows(c, R, req, StepReq::BYTES);
    if (c->N == c->n_total && R == c->N && c->opt.all_rows_shortcut && c->LW <= 2 && c->NW <= 8)
        return enqueue_all_rows(c, R, req, StepReq::DIRECT);   // one-shot calls are single-shard; codes / label sets the byte matrix does not take: k_rank_fused walks the rows
    HG_TRY(do_hist(c, 1));
    HG_TRY(do_plan(c, R, nullptr, 1, 0));
    return do_select(c, req);
}

// The exact sequence with its second pass on the matrix cores (one shard, R << N): full histogram -> plan (exact
// threshold t, and sstar = the last segment whose ties at t are still inside the quota) -> k_select_mx with T = t,
// fixed-capacity slices -> the bet's rank stage, which cuts the ties at the quota.  Nothing is guessed, so the only way
// this can fail is a slice overflowing its capacity (clustered rows): *err then, and the caller runs enqueue_exact.
static bool exact_mx_applies(const hg_ctx* c, int64_t R) {
    return c->opt.select_mfma && c->N == c->n_total && R * 8 <= c->N && c->N >= 65536 && !c->is_sub;
}
static int enqueue_exact_mx(hg_ctx* c, int64_t R, const StepReq& req) {
    HG_TRY(do_hist(c, 1, true, true));                 // per segment pair on the matrix cores where that applies
    HG_TRY(do_plan(c, R, nullptr, 1, 0));              // c->t, c->sstar; leaves optimistic = false, crow = R
    const Geo& g = c->geo;
    // in all the slices hold R records + the ties of one segment beyond the quota, but unevenly: segments up to sstar carry
    // ALL their rows at distance t (the cut bucket is typically the fullest), later ones none -- budget like the bet does
    // (not adopt_guess: this capacity has never had slice_capacity's two clamps -- to the segment's rows, to 64 GB of record rows --
    // and keeps its own arithmetic: no cap_boost, the stage stays do_plan's)
    const double mean = 0.1 * (double)c->opt.cand_budget_x10 * (double)R / (double)g.S;
    u32 cap = (u32)std::ceil(mean + 6.0 * std::sqrt(mean) + 16.0);
    cap = (cap + 15u) & ~15u;
    c->optimistic = true;
    c->cap = cap;
    c->crow = (i64)g.S * cap;
    HG_HIP(hipMemsetAsync(c->failq.p, 0, (size_t)g.Qpad * 4, c->stream));
    StepReq exact = req;
    exact.exact_cut = true;
    return do_select(c, exact);
}

static int enqueue_optimistic(hg_ctx* c, int64_t R, int stride, const StepReq& req) {
    // the guess stops at the cut, far below b/2 when R <= N/8 on any data whose queries resemble the database: the
    // sampled pass writes only those planes (130 -> 68 MB per launch at C2).  A cut beyond them reads as a thin
    // sample -- everything is taken, the slices overflow, the exact sequence answers.
    u64* tot = nullptr;                                // the planes' totals over the segment pairs, where k_hist_i8 took the pass
    HG_TRY(do_hist(c, stride, false, false, c->NB / 2 + 2, &tot));
    HG_TRY(set_R(c, R, 1, 0));
    const Geo& g = c->geo;
    HG_TRY(reserve_guess(c));
    HG_TRY(c->err.reserve(16));
    // first bet on this database: the guess kernel also measures how the near rows crowd (err[2], err[3]) -- see below
    const bool probe = c->opt.crowd_probe && !c->crowd_probed && c->cap_boost == 1 && !c->capturing && !c->is_sub;
    u32* crowd = probe ? c->err.as<u32>() + 2 : nullptr;
    if (probe) HG_HIP(hipMemsetAsync(crowd, 0, 8, c->stream));
    c->t_begin(KI_GUESS);
    const Geo gh = hist_geometry(c);                   // the sampled pass ran on coarser segments
    {   // lanes per query by the number of sampled segments each has to sum
        const int ratio = (int)(gh.L / g.L);
        const u32 srows = (u32)sampled_rows(c, stride);
        double sigma = (double)req.guess_sigma;
        if (c->handicap_next && !c->capturing) { sigma = -(double)c->handicap_next; c->handicap_next = 0; }   // (test hook: this bet is meant to lose)
#define HG_GUESS(P)                                                                                                     \
        hipLaunchKernelGGL(k_guess_direct<P>, dim3(grid_for(g.Qpad, WPB * (64 / P))), dim3(256), 0, c->stream,          \
                           c->hist.as<u32>(), gh.S, ratio, sigma, (i64)c->n_total, srows,                \
                           c->tguess.as<int>(), c->sstar.as<int>(), c->failq.as<u32>(), c->err.as<int>(), crowd, tot, g)
        // (more lanes per query shorten a lane's share of a plane but scatter a wavefront's loads over more lines: with 64
        // lanes for every query that the chip has room for, Q = 1000 went 0.068 -> 0.090 ms, C3 0.032 -> 0.061)
        if (gh.S <= 64) HG_GUESS(4);
        else if (gh.S <= 512) HG_GUESS(16);
        else HG_GUESS(64);
#undef HG_GUESS
    }
    c->t_end();
    HG_TRY(c->check_launch("k_guess_direct"));
    if (tot) c->hist_tot_zero = tot;                   // the guess stored zeros over every total it was handed
    if (probe) {
        // One host round trip, once per database: sum over the queries of (fullest sampled segment) * segments / (their total)
        // is ~2 for rows in random order (the maximum of ~50 small Poisson counts) and ~the number of classes for a database
        // stored class by class, whose slices then need that many times the mean -- widen them NOW instead of losing the
        // first two bets (round 3: first call 6.6 ms at C2, two lost bets per new context).
        u32 cr[2] = {0u, 0u};
        HG_HIP(hipMemcpyAsync(cr, crowd, 8, hipMemcpyDeviceToHost, c->stream));
        HG_TRY(c->sync());
        c->crowd_probed = true;
        const double ratio = cr[1] ? (double)cr[0] * (double)gh.S / (double)cr[1] : 0.0;
        c->crowd_x100 = (i64)(ratio * 100.0);
        if (ratio > 4.0) {
            i64 boost = 2;
            while ((double)boost < ratio && boost < 64) boost *= 2;
            c->cap_boost = boost;
            c->cfg_epoch++;
        }
    }
    // slice capacity: a guessed cut typically keeps 1.3-3 R rows (the guess overshoots by at most one
    // distance bucket, and cumulative counts grow ~2x per bucket in the tail where the cut lies; clustered
    // codes grow faster) -- budget 4 R per query over the S segments plus 6 sigma per slice.  HBM is
    // plentiful (2.5 GB at C2); an overflow only costs the exact rerun.
    adopt_guess(c, 0.1 * (double)req.cand_budget_x10 * (double)c->cap_boost * (double)R / (double)g.S);
    StepReq guessed = req;
    guessed.err_zeroed = true;                         // k_guess_direct cleared the lost-bet flag: launch_rank need not
    return do_select(c, guessed);
}

// Lost bets are per query (a short superset, an overflowed slice).  When only a few queries lost,
// rerun just those through the exact sequence in a child context that borrows the database
// tables, and patch their results into place.  *handled = false: too many, caller reruns all.
static int rerun_lost_queries(hg_ctx* c, int64_t R, bool lists, bool with_ap, bool* handled) {
    *handled = false;
    const Geo g = c->geo;
    std::vector<u32> bad((size_t)g.Q);
    HG_HIP(hipMemcpyAsync(bad.data(), c->qbad.p, (size_t)g.Q * 4, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    std::vector<u32> lost;
    for (int q = 0; q < g.Q; ++q) if (bad[(size_t)q]) lost.push_back((u32)q);
    const i64 nF = (i64)lost.size();
    if (nF == 0 || nF * 8 > g.Q) return HG_OK;
    hg_ctx* s = requery_child(c, nF);
    s->opt.optimistic = 0;
    // a handful of queries: the per-segment bookkeeping (k_hist_reduce, k_seg_layout walk S segments per query) costs more than
    // the pair passes themselves -- 2048 segments: 0.8 ms of a 1 ms rerun; 256 keep every CU busy and cost 0.1
    s->opt.max_segments = 256;
    HG_TRY(c->flist.reserve((size_t)nF * 4));
    HG_HIP(hipMemcpyAsync(c->flist.p, lost.data(), (size_t)nF * 4, hipMemcpyHostToDevice, c->stream));
    HG_TRY(s->qc.reserve((size_t)nF * c->NW * 4 + 64 * 4));
    HG_TRY(s->qlab.reserve((size_t)nF * c->LW * 8));
    auto move = [&](const void* src, void* dst, i64 rowbytes, int gather) {
        hipLaunchKernelGGL(k_move_rows, dim3((unsigned)nF), dim3(256), 0, c->stream, (const u8*)src, (u8*)dst,
                           c->flist.as<u32>(), rowbytes, gather);
    };
    move(c->qc.p, s->qc.p, (i64)c->NW * 4, 1);
    move(c->qlab.p, s->qlab.p, (i64)c->LW * 8, 1);
    HG_TRY(c->check_launch("k_move_rows"));
    s->stage = ST_DB | ST_Q;
    s->want_lists = lists;
    HG_TRY(enqueue_exact(s, R, StepReq{}));
    if (with_ap) HG_TRY(do_ap(s));
    move(s->mbits.p, c->mbits.p, c->RW * 8, 0);
    if (with_ap) {
        move(s->ap.p, c->ap.p, 8, 0);
        move(s->rel.p, c->rel.p, 4, 0);
    }
    if (lists) {
        move(s->out_idx.p, c->out_idx.p, R * 4, 0);
        move(s->out_dist.p, c->out_dist.p, R, 0);
    }
    HG_TRY(c->check_launch("k_move_rows"));
    HG_TRY(c->sync());                               // `lost` (the H2D source) must outlive the copy
    c->bet_requeried += nF;
    *handled = true;
    return HG_OK;
}

// The bet's sequence for hg_map, enqueued on the stream: sampled histogram -> guess -> select -> verify + order ->
// AP -> flag, AP and hit counts into pinned memory.  Pure enqueue (no synchronisation, no allocation once the
// buffers are warm), so it can run under stream capture.
// The verdict word, the APs and the hit counts into pinned memory behind everything enqueued so far (hg_get_ap then copies from there):
// one synchronisation for the whole call instead of a pageable 4-byte download, a wait, and hg_get_ap's own copies and wait.
// The step's results into pinned host memory by a KERNEL (the host block is device-addressable: stores go over the link as posted
// writes): a hipMemcpyAsync of these ~120 KB runs on a copy engine behind a cross-queue barrier and holds the stream ~20 us -- the
// gap between one step's last kernel and the next step's first (hg_map_begin) -- where this launch costs a few.
static __global__ __launch_bounds__(256) void k_copy_out(const uint4* __restrict__ src, uint4* __restrict__ dst, const u32 n16, const u32 tail_dwords) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n16) dst[i] = src[i];
    if (i < tail_dwords) ((u32*)(dst + n16))[i] = ((const u32*)(src + n16))[i];
}

// the copy-engine form: {verdict, leftover count}, APs and hit counts wherever the three live
static int download_results(hg_ctx* c, char* pb) {    // pb: [flag: 16 B][ap Q x 8][rel Q x 4]
    const size_t Q = (size_t)c->geo.Q;
    HG_HIP(hipMemcpyAsync(pb, c->err.p, 8, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(hipMemcpyAsync(pb + 16, c->ap.p, Q * 8, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(hipMemcpyAsync(pb + 16 + Q * 8, c->rel.p, Q * 4, hipMemcpyDeviceToHost, c->stream));
    return HG_OK;
}

extern "C++" int stage_ap_download(hg_ctx* c, void* dst) {      // dst: a pinned block of its own (hg_map_begin), else (nullptr) the context's
    const size_t Q = (size_t)c->geo.Q;
    if (!dst) HG_TRY(ensure_pin(c, Q * 12 + 16));
    char* pb = (char*)(dst ? dst : c->pin);    // [flag: 16 B][ap Q x 8][rel Q x 4]
    const char* base = (const char*)c->outblk.p;
    if (base && c->outblk_q == (i64)Q && c->err.p == base && c->ap.p == base + 16 && c->rel.p == base + 16 + Q * 8) {
        const size_t bytes = 16 + Q * 12;      // the three are views of one block (ensure_out_block)
        static const bool by_engine = getenv("HG_COPY_ENGINE_DOWNLOAD") != nullptr;       // (A/B: the copy-engine form)
        if (by_engine || c->capturing) {
            HG_HIP(hipMemcpyAsync(pb, base, bytes, hipMemcpyDeviceToHost, c->stream));
            return HG_OK;
        }
        const u32 n16 = (u32)(bytes / 16), tail = (u32)((bytes % 16) / 4);
        hipLaunchKernelGGL(k_copy_out, dim3((n16 + 255) / 256 + (n16 % 256 == 0 && tail ? 1 : 0)), dim3(256), 0, c->stream, (const uint4*)base, (uint4*)pb, n16, tail);
        return c->check_launch("k_copy_out");
    }
    return download_results(c, pb);
}

extern "C++" int wait_verdict(hg_ctx* c, bool staged, int* flag) {
    if (!staged) return read_plan_flag(c, flag);
    HG_TRY(c->sync());
    *flag = *(const int*)c->pin;
    return HG_OK;
}

// One attempt at a step, enqueued: the sequence of its kind, then -- for hg_map -- the APs (unless a rank kernel's epilogue left
// them) and their way home.  Pure enqueue for a bet whose buffers are warm, so a bet can run under stream capture.
enum Attempt { AT_BET, AT_EXACT_MX, AT_EXACT };
static int enqueue_attempt(hg_ctx* c, Attempt kind, int64_t R, int stride, const StepReq& req, bool with_ap) {
    c->t_step_begin();
    HG_TRY(kind == AT_BET ? enqueue_optimistic(c, R, stride, req) : kind == AT_EXACT_MX ? enqueue_exact_mx(c, R, req) : enqueue_exact(c, R, req));
    if (with_ap) {
        if (c->ap_fused) { c->ap_staged = false; c->stage |= ST_AP; }     // the rank kernel's epilogue left the APs (leftovers: finish_leftovers)
        else HG_TRY(do_ap(c));
        if (kind == AT_EXACT) c->ap_fused = false;     // (no leftovers on this path: nothing for finish_leftovers)
        HG_TRY(stage_ap_download(c, req.dst));         // [flag, leftover count: 16 B][ap Q x 8][rel Q x 4]; C1 (R = N through the byte matrix): 0.17 -> 0.14 ms per call
    }
    c->t_step_end();
    return HG_OK;
}
// the bet as the options ask for it
static StepReq bet_request(const hg_ctx* c, bool fuse_ap, void* dst = nullptr) {
    StepReq req;
    req.fuse_ap = fuse_ap;
    req.guess_sigma = c->opt.guess_sigma;
    req.cand_budget_x10 = c->opt.cand_budget_x10;
    req.dst = dst;
    return req;
}

static int capture_step(hg_ctx* c, int64_t R, int stride, const StepReq& req) {
    c->drop_graph();
    const unsigned long long epoch0 = g_alloc_epoch.load();
    HG_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    c->capturing = true;
    const int rc = enqueue_attempt(c, AT_BET, R, stride, req, true);
    c->capturing = false;
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &gr);
    if (rc != HG_OK || e != hipSuccess || !gr || g_alloc_epoch != epoch0) {
        if (gr) (void)hipGraphDestroy(gr);
        c->drop_graph();
        (void)hipGetLastError();
        if (rc != HG_OK) return rc;
        return fail(HG_ERR_HIP, "step capture failed: %s", e != hipSuccess ? hipGetErrorString(e) : "a buffer moved during capture");
    }
    hipGraphExec_t ex = nullptr;
    const hipError_t e2 = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
    if (e2 != hipSuccess) {
        (void)hipGraphDestroy(gr);
        c->drop_graph();
        return fail(HG_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e2));
    }
    auto& sg = c->sg;
    sg.graph = gr; sg.exec = ex;
    sg.epoch = g_alloc_epoch; sg.cfg = c->cfg_epoch; sg.R = R; sg.timing = c->timing;
    sg.left = *c;                                      // (the context's StepState)
    c->graph_captures++;
    return HG_OK;
}

// After the synchronisation of a fused step (k_rank_cnt ranked AND evaluated): the queries it declined -- pin[1] of them,
// flagged in bigq; a list spanning more than 16 distances, a record beyond its counters -- get the general rank kernel and
// k_ap now, and the results come over again.  Rare by construction (none on any BASELINE workload), so the common step
// carries neither launch.
static int finish_leftovers(hg_ctx* c, int* flag) {
    if (!c->ap_fused) return HG_OK;
    const u32 nleft = ((const u32*)c->pin)[1];
    if ((nleft != 0) != c->leftovers_expected) { c->leftovers_expected = nleft != 0; c->cfg_epoch++; }
    if (!nleft) return HG_OK;
    c->rank_leftovers += nleft;
    c->last_leftovers_inline = c->leftovers_inline;
    if (c->leftovers_inline) { c->leftovers_inline = false; return HG_OK; }     // k_rank_dense<slices> ranked them within the step
    HG_TRY(launch_rank_leftovers(c));
    HG_TRY(do_ap_range(c, 0, c->geo.Q, c->bigq.as<u32>()));
    HG_TRY(download_results(c, (char*)c->pin));
    return wait_verdict(c, true, flag);
}

// What follows every enqueued attempt of a one-shot call: wait, read the verdict (the bet was lost, a slice overflowed, R
// exceeds the rows), and for hg_map rank what a fused step left over; ap_staged: the pinned block holds the call's results.
static int await_attempt(hg_ctx* c, bool with_ap, int* flag) {
    HG_TRY(wait_verdict(c, with_ap, flag));
    if (with_ap) {
        HG_TRY(finish_leftovers(c, flag));
        c->ap_staged = *flag == 0;
    }
    return HG_OK;
}
static int run_attempt(hg_ctx* c, Attempt kind, int64_t R, int stride, const StepReq& req, bool with_ap, int* flag) {
    static const bool trace = getenv("HG_STEP_TRACE") != nullptr;        // debugging: where a slow step spent its time
    const auto tp0 = std::chrono::steady_clock::now();
    HG_TRY(enqueue_attempt(c, kind, R, stride, req, with_ap));
    const auto tp1 = std::chrono::steady_clock::now();
    HG_TRY(await_attempt(c, with_ap, flag));
    if (trace) {
        const auto tp2 = std::chrono::steady_clock::now();
        const double e = std::chrono::duration<double, std::milli>(tp1 - tp0).count(), w = std::chrono::duration<double, std::milli>(tp2 - tp1).count();
        if (e + w > 2.0) fprintf(stderr, "[hg] slow step: enqueue %.3f ms, wait %.3f ms (t_seq %lld, pending events %zu, pool %zu)\n", e, w, (long long)c->t_seq, c->pending.size(), c->pool.size());
    }
    return HG_OK;
}

// hg_map's first bet as a captured step (option "step_graph"): the second sighting of the same step (same tables, options, R,
// timing level; no buffer moved since) captures it, later ones replay it.  *launched = false: the caller runs it eagerly.
static int replay_bet(hg_ctx* c, int64_t R, int stride, const StepReq& req, bool* launched, int* flag) {
    auto& sg = c->sg;
    *launched = false;
    const auto current = [&] { return sg.exec && sg.epoch == g_alloc_epoch && sg.cfg == c->cfg_epoch && sg.R == R && sg.timing == c->timing; };
    const bool seen = sg.seen_epoch == g_alloc_epoch && sg.seen_cfg == c->cfg_epoch && sg.seen_R == R && sg.seen_timing == c->timing;
    if (!current() && seen && capture_step(c, R, stride, req) != HG_OK) c->opt.step_graph = 0;      // not fatal: stay eager from now on
    if (!current()) return HG_OK;
    HG_HIP(hipGraphLaunch(sg.exec, c->stream));
    HG_TRY(set_R(c, R, 1, 0));
    static_cast<StepState&>(*c) = sg.left;             // what the captured enqueue left behind on the host side
    c->graph_replays++;
    *launched = true;
    HG_TRY(await_attempt(c, true, flag));
    c->t_collect_graph();
    return HG_OK;
}

// The escalation ladder of a one-shot call: the bet -> (few queries lost: those alone, exactly) -> wider bets -> the exact
// threshold with the matrix-core select -> the exact sequence.
static int run_oneshot(hg_ctx* c, int64_t R, bool lists, bool with_ap) {
    c->real_lists = false;
    int stride = 0;
    if (R < 1 || R > c->n_total)
        return fail(HG_ERR_ARG, "R=%lld outside 1..N (N=%lld rows in the database)", (long long)R, (long long)c->n_total);
    c->want_lists = lists;
    if (with_ap && !c->is_sub) HG_TRY(ensure_out_block(c));
    int flag = 0;
    if (optimistic_eligible(c, R, &stride)) {
        const StepReq req = bet_request(c, with_ap);
        c->bet_runs++;
        if (with_ap) HG_TRY(ensure_pin(c, (size_t)c->Q * 12 + 16));
        bool launched = false;
        // event-record nodes inside a graph turned out slow and unreliable on ROCm 7.2 (a replayed step took 1.9 ms
        // instead of 1.55, elapsed times came back for one replay in twenty): with kernel timing on, steps stay eager
        if (with_ap && c->opt.step_graph && !lists && !c->is_sub && c->timing == 0) HG_TRY(replay_bet(c, R, stride, req, &launched, &flag));
        if (!launched) {
            HG_TRY(run_attempt(c, AT_BET, R, stride, req, with_ap, &flag));
            auto& sg = c->sg;
            if (with_ap) { sg.seen_epoch = g_alloc_epoch; sg.seen_cfg = c->cfg_epoch; sg.seen_R = R; sg.seen_timing = c->timing; }
        }
        if (!flag) { c->bet_consecutive_fail = 0; return HG_OK; }
        bool handled = false;                      // some queries lost their bet
        HG_TRY(rerun_lost_queries(c, R, lists, with_ap, &handled));
        if (handled) { c->bet_consecutive_fail = 0; return HG_OK; }
        // many queries lost.  Before paying for the exact two-pass sequence (3x the bet at C2), bet once more with
        // twice the safety margin and twice the record budget -- the verification is what makes either bet exact.
        // Still lost: the hits crowd into few segments (a database stored class by class: ten classes put ten times the
        // mean into a query's slices), which no margin on the CUT cures -- escalate the slices' capacity (x8, x64, until a
        // slice would hold its whole segment) and remember what worked for the next calls on this database.
        if (c->opt.second_bet) {
            StepReq wide = req;
            wide.guess_sigma = 2 * req.guess_sigma + 2;
            wide.cand_budget_x10 = 2 * req.cand_budget_x10;
            const i64 boost0 = c->cap_boost;
            for (int attempt = 0; attempt < 3; ++attempt) {
                if (attempt > 0) {
                    if (c->cap >= (u32)((c->geo.L + 15) & ~15ll)) break;               // a slice already holds a segment
                    if ((double)c->geo.Q * (double)c->crow * 8.0 * 8.0 > 64e9) break;  // the record rows would not fit comfortably
                    c->cap_boost = c->cap_boost * 8 > 4096 ? 4096 : c->cap_boost * 8;
                }
                c->bet_rebets++;
                const int rc = run_attempt(c, AT_BET, R, stride, wide, with_ap, &flag);
                if (rc != HG_OK) { c->cap_boost = boost0; return rc; }
                // held with twice the budget of a first bet at this boost: the next call's first bet gets that budget
                // (a class-sorted database of tight clusters lost every first bet at x8 and won every second one)
                // -- only when a WIDENED attempt was the one that held: a held plain second bet (attempt 0) says the margin was
                // short this once, not that the slices are too small, and must not ratchet every later first bet's budget up
                auto keep = [&] {
                    if (attempt > 0 && c->cap_boost < 4096) c->cap_boost *= 2;
                    c->bet_consecutive_fail = 0;
                    c->cfg_epoch++;
                };
                if (!flag) { keep(); return HG_OK; }
                handled = false;
                HG_TRY(rerun_lost_queries(c, R, lists, with_ap, &handled));
                if (handled) { keep(); return HG_OK; }
            }
            c->cap_boost = boost0;                 // nothing helped: do not keep paying for big slices
        }
        c->bet_fallbacks++;                        // still too many: exact path for all
        c->bet_consecutive_fail++;
    }
    if (exact_mx_applies(c, R)) {
        // (hg_map: the AP from the rank kernel's epilogue, as in the bet it shares the rank stage with -- and what that kernel
        // declines is counted in "rank_leftovers" and ranked by finish_leftovers, the same way)
        StepReq mx;
        mx.fuse_ap = with_ap && !lists;
        HG_TRY(run_attempt(c, AT_EXACT_MX, R, 0, mx, with_ap, &flag));
        if (!flag) return HG_OK;                   // (else a slice overflowed: the vector-ALU select with exact-sized slices)
    }
    StepReq exact;
    exact.fuse_ap = with_ap && !lists;
    HG_TRY(run_attempt(c, AT_EXACT, R, 0, exact, with_ap, &flag));
    return flag ? plan_overrun(c) : HG_OK;
}

int hg_topr(hg_ctx* c, int64_t R) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_topr", "hg_set_database + hg_set_queries"));
    return run_oneshot(c, R, true, false);
}

int hg_map(hg_ctx* c, int64_t R, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_map", "hg_set_database + hg_set_queries"));
    const i64 fails0 = c->bet_fallbacks + c->bet_requeried + c->bet_rebets, left0 = c->rank_leftovers;
    c->last_leftovers_inline = false;
    HG_TRY(run_oneshot(c, R, false, true));
    HG_TRY(hg_get_ap(c, host_ap, host_rel));
    // what hg_map_begin may enqueue without looking back: this very step, when it just won its bet outright
    // (queries the fused rank kernel declines are fine when the step ranks them itself within the stream: leftovers_inline)
    if (c->optimistic && c->bet_fallbacks + c->bet_requeried + c->bet_rebets == fails0 && (c->rank_leftovers == left0 || c->last_leftovers_inline) && !c->is_sub) {
        c->map_warm_cfg = c->cfg_epoch; c->map_warm_epoch = g_alloc_epoch; c->map_warm_R = R;
        // slot 1's stream now, once per context (a stream costs milliseconds to create -- not inside a caller's pipeline)
        if (c->opt.step_streams >= 2 && c->own_stream && !c->stream_b) HG_TRY(stream_create(c->device, &c->stream_b));
    } else {
        c->map_warm_R = -1;
    }
    return HG_OK;
}

// hg_map in two halves, for a caller that evaluates batch after batch: hg_map_begin enqueues a step (kernels and the download of
// its verdict, APs and hit counts into a pinned block of its own) and returns; hg_map_end waits for the OLDEST step in flight and
// hands its results over.  Two steps may be in flight, so the GPU starts step i + 1 the moment step i ends -- the host's wake-up,
// its copies and its next enqueue (~40 us per step at C2) no longer sit between them.  A step is only enqueued blind when the
// last synchronous hg_map with the same tables, options and R won its bet outright; otherwise hg_map_begin runs the whole call
// itself (and keeps the results for hg_map_end).  A blind step that loses its bet is run again, synchronously, by hg_map_end:
// results are those of hg_map in every case.
// Two-stream form (step_streams = 2): the tables a blind step reads and a step would otherwise (re)build on first use -- the
// query image after hg_set_queries kept the licence, the AP tables -- are built on the context's stream BEFORE the step, so a step
// on stream_b never writes them and a fork point taken after this sees them.  *enqueued: something was.
static int prepare_shared(hg_ctx* c, int64_t R, bool* enqueued) {
    *enqueued = false;
    if (c->opt.select_mfma && !c->qx_valid) { HG_TRY(ensure_mx_images(c, false)); *enqueued = true; }
    const bool recip = c->opt.ap_recip && R <= (1ll << 20);
    if (c->shapes_for_R != R || (recip && c->recip_for_R != R)) {
        HG_TRY(set_R(c, R, 1, 0));
        bool use_recip = false;
        HG_TRY(ensure_ap_tables(c, &use_recip));
        *enqueued = true;
    }
    return HG_OK;
}

// A blind step of slot 1 on stream_b, in the workspace ws_b.  Its stream first waits for everything on the context's stream
// except a blind slot-0 step in flight (that one writes only the context's own workspace): ev_pre, recorded just before it, when
// nothing else was enqueued since; else the stream's tail.  stream_b itself holds nothing else: its previous step was waited for
// by hg_map_end, so the workspace is free.
static int enqueue_bet_on_b(hg_ctx* c, hg_ctx::MapSlot& m, int64_t R, int stride, bool tail_fork) {
    if (!c->stream_b) HG_TRY(stream_create(c->device, &c->stream_b));
    if (!c->ev_pre) HG_HIP(hipEventCreateWithFlags(&c->ev_pre, hipEventDisableTiming));
    if (!c->ev_fork) HG_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    if (tail_fork || !c->pre_valid) {
        HG_HIP(hipEventRecord(c->ev_fork, c->stream));
        HG_HIP(hipStreamWaitEvent(c->stream_b, c->ev_fork, 0));
    } else {
        HG_HIP(hipStreamWaitEvent(c->stream_b, c->ev_pre, 0));
    }
    c->b_open = false;
    const FirstReservations first;                     // (ws_b's: the context's own workspace is untouched)
    c->swap_step();
    int rc = ensure_out_block(c);                      // (ws_b's own err / ap / rel views; on first use)
    if (rc == HG_OK) rc = enqueue_attempt(c, AT_BET, R, stride, bet_request(c, true, m.pin), true);
    if (rc == HG_OK && hipEventRecord(m.ev, c->stream) != hipSuccess) rc = fail(HG_ERR_HIP, "hg_map_begin: hipEventRecord failed");
    c->swap_step();
    if (rc != HG_OK) { (void)hipStreamSynchronize(c->stream_b); return rc; }
    c->b_ev = m.ev;
    c->b_open = true;
    first.keep(c);
    c->map_overlapped++;
    return HG_OK;
}

int hg_map_begin(hg_ctx* c, int64_t R) {
    if (!c) return fail(HG_ERR_ARG, "hg_map_begin: null context");
    if ((c->stage & (ST_DB | ST_Q)) != (ST_DB | ST_Q)) return fail(HG_ERR_STATE, "hg_map_begin called before hg_set_database + hg_set_queries");
    HG_HIP(hipSetDevice(c->device));                   // (not use(): a blind step does not wait for the other slot's)
    if (c->ms_n == 2) return fail(HG_ERR_STATE, "hg_map_begin: two steps are in flight already (hg_map_end takes the oldest)");
    const int slot = (c->ms_head + c->ms_n) & 1;
    hg_ctx::MapSlot& m = c->mslot[slot];
    m.R = R; m.Q = c->Q;
    m.q_gen = c->q_gen; m.db_gen = c->db_gen;
    int stride = 0;
    bool blind = c->map_warm_R == R && c->map_warm_cfg == c->cfg_epoch && c->map_warm_epoch == g_alloc_epoch && !c->is_sub;
    if (blind) {
        c->real_lists = false;
        c->want_lists = false;
        HG_TRY(ensure_out_block(c));
        blind = optimistic_eligible(c, R, &stride) && c->map_warm_epoch == g_alloc_epoch;
    }
    if (blind) {
        const size_t need_b = (size_t)c->Q * 12 + 16;
        HG_HIP(pin_grow(&m.pin, &m.cap, need_b));
        if (!m.ev) HG_HIP(hipEventCreateWithFlags(&m.ev, hipEventDisableTiming));
        c->bet_runs++;
        // two streams unless the caller owns the stream (hg_set_stream) or per-kernel timing is on (its events assume one stream)
        const bool two = c->opt.step_streams >= 2 && c->own_stream && c->timing == 0 && !c->capturing;
        bool prepped = false;
        if (two) HG_TRY(prepare_shared(c, R, &prepped));
        c->bitmap_changed();                           // (a ranking that does not come through set_R)
        c->mbits_in_ws_b = two && slot == 1;
        if (two && slot == 1) {
            HG_TRY(enqueue_bet_on_b(c, m, R, stride, prepped));
        } else {
            if (two) {                                 // the fork point of a slot-1 step enqueued while this one is in flight
                if (!c->ev_pre) HG_HIP(hipEventCreateWithFlags(&c->ev_pre, hipEventDisableTiming));
                HG_HIP(hipEventRecord(c->ev_pre, c->stream));
            }
            c->pre_valid = two;                        // (one stream: this step may build a shared table -- no fork point before it)
            HG_TRY(enqueue_attempt(c, AT_BET, R, stride, bet_request(c, true, m.pin), true));
            HG_HIP(hipEventRecord(m.ev, c->stream));
        }
        m.inline_ok = c->leftovers_inline;               // the step ranks what its fused kernel declines within the stream
        c->leftovers_inline = false;
        c->ap_staged = false;
        m.async = true;
        c->map_async_steps++;
    } else {
        m.ap.resize((size_t)c->Q); m.rel.resize((size_t)c->Q);
        HG_TRY(hg_map(c, R, m.ap.data(), m.rel.data()));
        m.async = false;
    }
    ++c->ms_n;
    return HG_OK;
}

int hg_map_end(hg_ctx* c, double* host_ap, int64_t* host_rel) {
    if (!c) return fail(HG_ERR_ARG, "hg_map_end: null context");
    HG_HIP(hipSetDevice(c->device));                   // (not use(): nothing is enqueued unless the step lost -- hg_map then joins)
    if (!c->ms_n) return fail(HG_ERR_STATE, "hg_map_end: no step in flight (hg_map_begin first)");
    hg_ctx::MapSlot& m = c->mslot[c->ms_head];
    c->ms_head ^= 1; --c->ms_n;                           // (taken off the queue whatever happens below)
    const size_t Q = (size_t)m.Q;
    if (!m.async) {
        if (host_ap) memcpy(host_ap, m.ap.data(), Q * 8);
        if (host_rel) memcpy(host_rel, m.rel.data(), Q * 8);
        return HG_OK;
    }
    HG_HIP(hipEventSynchronize(m.ev));
    const u32* w = (const u32*)m.pin;                      // [verdict][queries the fused rank kernel declined] ...
    if (w[0] == 0 && (w[1] == 0 || m.inline_ok)) {         // (won: the results are this step's whatever the tables hold by now)
        const char* pb = (const char*)m.pin;
        if (host_ap) memcpy(host_ap, pb + 16, Q * 8);
        if (host_rel) {
            const u32* r = (const u32*)(pb + 16 + Q * 8);
            for (size_t q = 0; q < Q; ++q) host_rel[q] = r[q];
        }
        return HG_OK;
    }
    // the bet was lost (or queries were left over): the synchronous call sorts that out -- reruns, deeper bets, wider slices -- on
    // the same tables; a younger step in flight keeps its own verdict in its own block
    c->map_warm_R = -1;
    if (m.q_gen != c->q_gen || m.db_gen != c->db_gen || (i64)Q != c->Q)
        return fail(HG_ERR_STATE, "hg_map_end: the %s replaced while a step that lost its bet was in flight: its tables are gone, "
                                  "load them again and call hg_map", m.db_gen != c->db_gen ? "database was" : "queries were");
    c->map_async_redone++;
    return hg_map(c, m.R, host_ap, host_rel);
}

}  // extern "C"

// hg_preload: the runtime loads a translation unit's code object when one of its kernels is first needed (milliseconds);
// asking for a kernel's attributes does that now
int preload_seq() {
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_copy_out)));
    return HG_OK;
}

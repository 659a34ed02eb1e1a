// libhashgan_amd.so -- the rank stage of the Hamming sequences: verify + plan + order of a step's rows.
// choose_rank decides which kernel meets them (a RankChoice: nothing launched, reserved or written); launch_rank runs the
// choice -- the common prologue, one launcher per kernel, then the general kernel where the first one declines queries.
#include "hg_ctx.hpp"
#include "hg_rank_cnt.hpp"
#include "hg_rank_lean.hpp"
#include "hg_rank_dense.hpp"

// Every record of a bet lies within its query's cut (the guess; the exact threshold of enqueue_exact_mx), and a list
// reaching further down than the 16 (32) distances the LDS rank kernels place leaves them anyway: byte counters for the 18 (34)
// distances up to the cut are all they need (round 3: b/2 + 2 of them -- 8.7 KB of LDS at b = 64, 16.9 KB at b = 128); a
// query with a record below them goes to k_rank_fused.  0: a counter for every distance (short codes), and no cut to read.
static int cut_counters(const Geo& g) { return rank_cnt_maxb(g.NB) + 2 < g.NB ? rank_cnt_maxb(g.NB) + 2 : 0; }
static int nbits_for(int NB) { int nbits = 1; while ((1 << nbits) < NB) ++nbits; return nbits; }

// What the rank stage decides for one step.
struct RankChoice {
    RankKernel first = RK_FUSED;   // ranks first (RK_FUSED: the general kernel alone; RK_NONE: byte rows that k_rank_dense does not take)
    i64 recs = 0;                  // k_rank_lean / k_rank_cnt: record capacity of the LDS arrays (RankLdsArgs::lds_recs)
    int psp = 0, nbc = 0;          // k_rank_lean: pieces of every slice fetched up front; both: distances that have counters (cut_counters)
    int lds = 0;                   // dynamic LDS bytes of `first` (k_rank_dense<slices>: sl_lds)
    bool ap_epilogue = false;      // the AP is asked of first's epilogue (k_rank_dense's two forms give it only with the reciprocals)
    bool then_general = false;     // k_rank_fused follows on the queries `first` declined (bigq)
    int nwav = 4, bits_lds = 0;    // k_rank_fused: wavefronts per query; its bitmap fits the LDS
    int sl_rows = 0, sl_lds = 0;   // k_rank_dense<slices>, first or inline: counter rows, LDS bytes
    bool inline_slices = false;    // ... ranks within the step what a fused k_rank_lean / k_rank_cnt declined
    bool gbm = false;              // k_rank_dense on the byte matrix: the R-bit bitmap in global memory; else kparts blocks per query, each
    int kparts = 1; i64 rw_part = 0;   // keeping rw_part words of it in LDS (rw_part = 0: one block, all of it)
};

// k_rank_fused's shape: wavefronts per query by the records per query (~ 3R of a bet, R exact) -- or 16 when only a handful of
// blocks has work (the leftovers of a fused step: what counts is one block's latency)
static void general_shape(const hg_ctx* c, bool few_blocks, RankChoice& ch) {
    ch.nwav = (c->optimistic ? 3 * c->R : c->R) >= 16384 || (few_blocks && c->R >= 1024) ? 16 : 4;
    ch.bits_lds = ((size_t)(ch.nwav + 1) * c->geo.NB + 8 + 2 * (size_t)c->RW) * 4 <= 64 * 1024;
}

// The choice, from the context as the select left it (R, the slices' capacity, the record format, the segment count), the
// options, the mode and the request.  None of it has to be known before the select runs: the select writes one record layout
// per format (one byte or eight) whichever kernel reads it.  What does anticipate the choice is the geometry: full_geometry
// keeps a bet at <= 256 segments where k_rank_lean may take it.  Launches nothing, reserves nothing, writes nothing.
static RankChoice choose_rank(const hg_ctx* c, int mode, const StepReq& req) {
    const Geo& g = c->geo;
    const int lds_cu = 160 * 1024;
    RankChoice ch;
    // AP from the first kernel's epilogue: hg_map asks for it, the step ranks whole lists, and nobody wants them written out
    const bool ap_wanted = req.fuse_ap && c->opt.fuse_ap && mode == RANK_WHOLE && !lists_needed(c);
    if (req.rows == StepReq::BYTES && mode == RANK_WHOLE) {
        // the dense regime through the byte matrix (hg_rank_dense.hpp): the counter columns always fit a block's LDS for codes of <= 126 bits
        // (c->NB, not g.NB: rank_dense_fits asks before the step's geometry is made)
        ch.first = c->opt.rank_dense && c->LW <= 2 && c->NW <= 4 && c->b <= 126 && c->N == c->n_total && !c->is_sub ? RK_DENSE : RK_NONE;
        if (ch.first == RK_NONE) return ch;
        // Where the R-bit bitmap lives.  LDS while two blocks still share a CU, and the AP then leaves from the epilogue (C1: 0.12 ms
        // for ranking + AP).  A bitmap that leaves room for one block only: in global memory while the members are few (R < N/4:
        // the atomic ORs of the matching members cost ~3.6 ms per 10^9; two to four blocks per CU), else in LDS with one block per CU --
        // and k_ap afterwards either way (an epilogue on four wavefronts per CU is a latency chain: 62 chunks at R = 500k, 0.3 ms per query).
        // Q = 10k, N = 1M, b = 64, ranking + AP: R = 130k 7.4 ms global / 11.5 LDS; 200k 9.7 / 12.0; 500k 22.7 / 13.7.
        const int tot_lds = rank_dense_layout(c->NB, c->RW, false).total, tot_gbm = rank_dense_layout(c->NB, c->RW, true).total;
        const int blocks_lds = (c->RW * 8 + 4096 < lds_cu && tot_lds <= lds_cu) ? lds_cu / tot_lds : 0;
        // A bitmap beyond one block's LDS with R >= N/4: K blocks per query, each ranks everything and keeps its K-th of the ranks in LDS
        // (R = N = 1M: two blocks per query, 2 x 10 ms, against 37 ms of atomic ORs on a bitmap in global memory)
        if (blocks_lds == 0 && g.R * 4 >= c->N && c->opt.rank_dense_gbm != 1) {
            const i64 room = lds_cu - tot_gbm - 4096;
            ch.kparts = (int)((c->RW * 8 + room - 1) / room);
            if (ch.kparts >= 2 && ch.kparts <= 8) ch.rw_part = (c->RW + ch.kparts - 1) / ch.kparts; else ch.kparts = 1;
        }
        ch.gbm = ch.rw_part ? false
               : c->opt.rank_dense_gbm >= 0 ? c->opt.rank_dense_gbm != 0 || blocks_lds == 0 : (blocks_lds == 0 || (blocks_lds < 2 && g.R * 4 < c->N));
        ch.lds = ch.gbm ? tot_gbm : ch.rw_part ? rank_dense_layout(c->NB, ch.rw_part, false).total : tot_lds;
        ch.ap_epilogue = !ch.gbm && !ch.rw_part && blocks_lds >= 2 && ap_wanted;
        return ch;
    }
    general_shape(c, false, ch);
    // Only a bet's records, whole (one shard) or ranked locally (RANK_LOCAL), meet an LDS-resident kernel: exact rows, and the
    // count and place phases around the shards' exchange, are k_rank_fused's.
    if (!c->optimistic || mode == RANK_COUNT || mode == RANK_PLACE) return ch;
    ch.nbc = cut_counters(g);
    const double share = (double)c->N / (double)(c->n_total > 0 ? c->n_total : 1);
    // k_rank_dense<slices>: the bet's cut never exceeds b/2 + 1 -- enqueue_optimistic's sampled pass stops there --, so b/2 + 2 counter rows cover its records
    ch.sl_rows = (!req.exact_cut && g.NB / 2 + 2 < g.NB) ? g.NB / 2 + 2 : g.NB;
    ch.sl_lds = rank_dense_layout(ch.sl_rows + 1, c->RW, false).total;
    const bool slices_fit = c->rec8 && !c->want_lists && g.S <= RD_THREADS && ch.sl_rows <= 126 && ch.sl_lds <= lds_cu;
    // The last fused step on this context had queries its rank kernel declined (one of C5's 10 000 spans more distances than
    // k_rank_lean places): rank the flagged ones right behind it, in the same stream -- a launch of mostly returning blocks --
    // instead of a second host round trip (k_rank_fused + k_ap + three downloads: 0.08 ms of C5's 1.27).
    ch.inline_slices = ap_wanted && c->leftovers_expected && c->opt.inline_leftovers && slices_fit;
    // the lean counting sort (k_rank_lean): the whole record row in one coalesced read, piecewise compaction, chunks in registers
    if (c->opt.rank_lds >= 2 && c->rec8 && !c->want_lists && g.S <= 256 && (c->cap & 15u) == 0 && c->cap <= 1024 && g.R <= 60000) {
        const int nbc_eff = ch.nbc ? ch.nbc : (g.NB < 128 ? g.NB : 128);
        // room for every piece of the row when that fits HG_RANK_WAVES blocks per CU; else for the usual list (2.2 R + padding)
        const i64 all = (i64)g.S * c->cap;
        // pieces of a slice fetched up front: what it holds but for a 4-sigma exception, when the select keeps ~0.7 of the budgeted
        // mean (cap = mean + 6 sqrt(mean) + 16, inverted); at most what four loads per thread cover
        const double mb = std::pow(std::sqrt((double)c->cap > 7.0 ? (double)c->cap - 7.0 : 0.0) - 3.0, 2.0), est = 0.7 * mb;
        int psp = (int)std::ceil((est + 4.0 * std::sqrt(est) + 1.0) / 16.0);
        if (psp > (int)(c->cap >> 4)) psp = (int)(c->cap >> 4);
        if (psp > RL_MAX_PIECES / g.S) psp = RL_MAX_PIECES / g.S;
        if (psp < 1) psp = 1;
        const i64 room = ((lds_cu / HG_RANK_WAVES) & ~511ll) - rank_lean_layout(g.NB, c->RW, g.S, 0, ch.nbc).total;
        i64 rb = all <= room ? all : room & ~15ll;
        const i64 least = ((i64)(2.2 * (double)c->R * share) + 256 + 16 * (i64)g.S + 15) & ~15ll;
        if (rb < least && least <= all) rb = least;
        if (rb > all) rb = all;
        if (rb > 16 * RL_MAX_PIECES) rb = 16 * RL_MAX_PIECES;      // a thread keeps at most four pieces of its query's list
        const RankLeanLds L = rank_lean_layout(g.NB, c->RW, g.S, (int)rb, ch.nbc);
        if (nbc_eff <= 63 && L.total <= 64 * 1024 && rb >= 16 && (rb >= least || rb == all)) {
            ch.first = RK_LEAN; ch.recs = rb; ch.psp = psp; ch.lds = L.total;
            ch.ap_epilogue = ap_wanted; ch.then_general = !ap_wanted;
            return ch;
        }
    }
    // long lists of a bet (beyond k_rank_lean's LDS): k_rank_dense's two passes over the query's record slices, thread = part of a slice
    if (mode == RANK_WHOLE && c->opt.rank_slices > 0 && g.R >= c->opt.rank_slices && slices_fit) {
        ch.first = RK_SLICES;
        ch.ap_epilogue = ap_wanted && lds_cu / ch.sl_lds >= 2;
        ch.inline_slices = false;
        return ch;
    }
    // per-thread counting sort (k_rank_cnt): byte counters for every distance + a tile of the records, <= 64 KiB per
    // block; lists longer than a tile are ranked tile by tile
    if (c->opt.rank_lds >= 1) {
        const int lists = lists_needed(c) ? 1 : 0;
        i64 r2 = (i64)(2.5 * (double)c->R * share) + 256;         // a tile of the records: the usual list (1.3 - 2 R) in one
        if (r2 < 4096) r2 = 4096;                                  // (small R: the guess's margin is relatively larger)
        r2 = r2 / 64 * 64;
        RankCntLds L = rank_cnt_layout(g.NB, c->RW, g.S, (int)r2, lists, ch.nbc);
        {   // one block more per CU when trimming the record tile by a few percent (never below 2.2 R) makes it fit
            const int per_cu = (int)(lds_cu / ((L.total + 511) & ~511));
            const i64 want = (lds_cu / (per_cu + 1)) & ~511ll;
            const i64 r3 = (r2 - (L.total - want)) / 64 * 64;
            // (the kernel is compiled for HG_RANK_WAVES wavefronts per SIMD = blocks per CU: more LDS room than that buys nothing)
            if (per_cu + 1 <= HG_RANK_WAVES && L.total > want && r3 >= (i64)(2.2 * (double)c->R * share) + 256 && r3 >= 4096 && !lists) {
                r2 = r3;
                L = rank_cnt_layout(g.NB, c->RW, g.S, (int)r2, 0, ch.nbc);
            }
        }
        while (L.total > 64 * 1024 && r2 > 64) { r2 -= 64; L = rank_cnt_layout(g.NB, c->RW, g.S, (int)r2, lists, ch.nbc); }
        if (L.total <= 64 * 1024 && r2 >= 4096) {
            // hg_map's bet: the AP leaves with the ranking (the bitmap is in LDS), and the general kernel is NOT launched behind it --
            // the step's download carries the number of queries this kernel declined (err[1]); the host launches it only then
            ch.first = RK_CNT; ch.recs = r2; ch.lds = L.total;
            ch.ap_epilogue = ap_wanted; ch.then_general = !ap_wanted;
            return ch;
        }
    }
    return ch;
}

bool rank_dense_fits(const hg_ctx* c) { return choose_rank(c, RANK_WHOLE, StepReq{false, StepReq::BYTES}).first == RK_DENSE; }
// the tables an AP epilogue reads, where one is asked for: the summation trees, and the reciprocals (*use_recip) for lists of <= 2^20
static int ap_epilogue_tables(hg_ctx* c, const RankChoice& ch, bool* use_recip) {
    *use_recip = false;
    return ch.ap_epilogue ? ensure_ap_tables(c, use_recip) : HG_OK;
}
static int reserve_rank_out(hg_ctx* c, int mode, int nwav) {
    HG_TRY(c->err.reserve(16));
    HG_TRY(c->qbad.reserve((size_t)c->geo.Qpad * 4));
    if (mode != RANK_WHOLE) HG_TRY(c->hwq.reserve((size_t)c->geo.Q * nwav * c->geo.NB * 4));
#ifdef HG_RANK_PROFILE
    HG_TRY(c->hwq.reserve((size_t)4096 * 16 * 4 + (size_t)c->geo.Q * nwav * c->geo.NB * 4));
#endif
    return HG_OK;
}

static void launch_dense_bytes(hg_ctx* c, u8* D, i64 Npad, int q0, int nq) {
    const int qper = 64;
    const dim3 grid((unsigned)(Npad / 1024), (unsigned)((nq + qper - 1) / qper));
    const u32 padbyte = (u32)c->b;                     // the distance of the rows past N (k_rank_dense: padrow)
#define HG_DENSE_BYTES(NW_, LW_)                                                                                                      \
    hipLaunchKernelGGL((k_dense_bytes<NW_, LW_>), grid, dim3(256), 0, c->stream, c->qc.as<u32>(), c->qlab.as<u64>(), c->db.as<u32>(), \
                       c->dblab.as<u64>(), D, c->N, Npad, q0, nq, qper, padbyte)
    const int key = c->NW * 2 + (c->LW <= 1 ? 0 : 1);
    switch (key) {
        case 2: HG_DENSE_BYTES(1, 1); break;
        case 3: HG_DENSE_BYTES(1, 2); break;
        case 4: HG_DENSE_BYTES(2, 1); break;
        case 5: HG_DENSE_BYTES(2, 2); break;
        case 6: HG_DENSE_BYTES(3, 1); break;
        case 7: HG_DENSE_BYTES(3, 2); break;
        case 8: HG_DENSE_BYTES(4, 1); break;
        default: HG_DENSE_BYTES(4, 2); break;
    }
#undef HG_DENSE_BYTES
}

// k_dense_bytes + k_rank_dense, chunk of queries by chunk: no records, no verdict of a bet -- none of launch_rank's prologue
static int launch_rank_dense(hg_ctx* c, const RankChoice& ch) {
    const Geo& g = c->geo;
    HG_TRY(c->err.reserve(16));
    HG_TRY(c->qbad.reserve((size_t)g.Qpad * 4));
    const i64 Npad = rank_dense_pieces(c->N) * RD_THREADS * 16;
    i64 qchunk = (c->opt.dense_budget_mb << 20) / Npad;
    if (qchunk < 1) qchunk = 1;
    if (qchunk > g.Q) qchunk = g.Q;
    // (the byte matrix is a budget, not a need: when the device cannot give that much, fewer queries per chunk do)
    for (;;) {
        const int rc = c->dbytes.reserve((size_t)qchunk * Npad);
        if (rc == HG_OK) break;
        if (qchunk == 1) return rc;
        (void)hipGetLastError();
        qchunk = (qchunk + 1) / 2;
    }
    bool fused = false;                                // the AP from the epilogue: only with the reciprocals
    HG_TRY(ap_epilogue_tables(c, ch, &fused));
    if (ch.gbm) HG_HIP(hipMemsetAsync(c->mbits.p, 0, (size_t)g.Q * c->RW * 8, c->stream));
    for (i64 q0 = 0; q0 < g.Q; q0 += qchunk) {
        const int nq = (int)(q0 + qchunk < g.Q ? qchunk : g.Q - q0);
        c->t_begin(KI_SELECT);
        launch_dense_bytes(c, c->dbytes.as<u8>(), Npad, (int)q0, nq);
        c->t_end();
        HG_TRY(c->check_launch("k_dense_bytes"));
        RankDenseArgs da{c->dbytes.as<u8>(), Npad, (int)q0, c->err.as<int>(), c->qbad.as<u32>(), c->RW,
                         fused ? c->shapes.as<ApShape>() : nullptr, fused ? c->ap_recip.as<double>() : nullptr, c->ap.as<double>(), c->rel.as<u32>(),
                         nullptr, nullptr, nullptr, 0u, 0, ch.rw_part, nullptr, g.NB};
        c->t_begin(KI_RANK_FUSED);
#define HG_RANK_DENSE(LISTS_, GBM_)                                                                                                              \
    do {                                                                                                                                         \
        if (q0 == 0) HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rank_dense<LISTS_, GBM_, false>), hipFuncAttributeMaxDynamicSharedMemorySize, ch.lds)); \
        hipLaunchKernelGGL((k_rank_dense<LISTS_, GBM_, false>), dim3(nq, ch.kparts), dim3(RD_THREADS), (size_t)ch.lds, c->stream, da, c->out_idx.as<u32>(),  \
                           c->out_dist.as<u8>(), c->mbits.as<u32>(), g);                                                                         \
    } while (0)
        if (c->want_lists) { if (ch.gbm) HG_RANK_DENSE(true, true); else HG_RANK_DENSE(true, false); }
        else { if (ch.gbm) HG_RANK_DENSE(false, true); else HG_RANK_DENSE(false, false); }
#undef HG_RANK_DENSE
        c->t_end();
        HG_TRY(c->check_launch("k_rank_dense"));
    }
    c->last_rank = RK_DENSE;
    c->ap_fused = fused;
    return HG_OK;
}

// k_rank_dense<slices> (hg_rank_dense.hpp) over the bet's one-byte records: the whole launch (long lists), or only the queries
// flagged in `only` (what a fused k_rank_lean / k_rank_cnt declined -- a handful of blocks, behind a launch whose AP tables
// and reciprocals are in place: rank_lds_done), with the AP from the epilogue
static int launch_rank_slices(hg_ctx* c, const RankChoice& ch, const u32* only) {
    const Geo& g = c->geo;
    bool fused = only != nullptr;
    if (!only) { HG_TRY(ap_epilogue_tables(c, ch, &fused)); c->ap_fused = fused; }
    RankDenseArgs da{nullptr, 0, 0, c->err.as<int>(), c->qbad.as<u32>(), c->RW,
                     fused ? c->shapes.as<ApShape>() : nullptr, fused ? c->ap_recip.as<double>() : nullptr, c->ap.as<double>(), c->rel.as<u32>(),
                     c->cand.as<u8>(), c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->cap, c->crow, 0, only, ch.sl_rows};
    HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rank_dense<false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, ch.sl_lds));
    c->t_begin(only ? KI_RANK_FUSED : KI_RANK_LDS);
    hipLaunchKernelGGL((k_rank_dense<false, false, true>), dim3(g.Q), dim3(RD_THREADS), (size_t)ch.sl_lds, c->stream, da, c->out_idx.as<u32>(),
                       c->out_dist.as<u8>(), c->mbits.as<u32>(), g);
    c->t_end();
    return c->check_launch("k_rank_dense<slices>");
}

// The arguments k_rank_lean and k_rank_cnt share, after the reservations they need (bigq; the AP tables where the epilogue is
// asked for); want_lists, rec8 and spec_pieces are the caller's to set.
static int rank_lds_args(hg_ctx* c, int mode, const StepReq& req, const RankChoice& ch, RankLdsArgs* la, bool* use_recip) {
    HG_TRY(c->bigq.reserve((size_t)c->geo.Qpad * 4));
    HG_TRY(ap_epilogue_tables(c, ch, use_recip));
    const bool ap = ch.ap_epilogue;
    *la = RankLdsArgs{c->sl_cnt.as<u32>(), c->failq.as<u32>(), c->err.as<int>(), c->qbad.as<u32>(), c->bigq.as<u32>(),
                      c->cap, c->crow, 0, 1, c->RW, (int)ch.recs, mode, c->hwq.as<u32>(), c->hown.as<u32>(),
                      c->t.as<int>(), c->cnt_lt.as<u32>(), c->quota.as<u32>(), c->tie_before.as<u32>(), c->posbase.as<u32>(), ch.nbc,
                      ap ? c->shapes.as<ApShape>() : nullptr, ap && *use_recip ? c->ap_recip.as<double>() : nullptr,
                      c->ap.as<double>(), c->rel.as<u32>(), ap ? c->err.as<u32>() + 1 : nullptr, ch.nbc ? cut_of(c, req) : nullptr, 0};
    return HG_OK;
}
// ... and what their launch leaves on the host.  A fused one with one-byte records may rank its leftovers within the step;
// with eight-byte records (k_rank_cnt only) leftovers_inline stays what the step before left, as it always has.
static int rank_lds_done(hg_ctx* c, const RankChoice& ch, bool use_recip) {
    c->last_lds_recs = ch.recs;
    c->ap_fused = ch.ap_epilogue;
    if (!ch.ap_epilogue || !c->rec8) return HG_OK;
    c->leftovers_inline = ch.inline_slices && use_recip;
    return c->leftovers_inline ? launch_rank_slices(c, ch, c->bigq.as<u32>()) : HG_OK;
}

static int launch_rank_lean(hg_ctx* c, int mode, const StepReq& req, const RankChoice& ch) {
    RankLdsArgs la;
    bool use_recip = false;
    HG_TRY(rank_lds_args(c, mode, req, ch, &la, &use_recip));
    la.spec_pieces = ch.psp;
    c->t_begin(KI_RANK_LDS);
    hipLaunchKernelGGL(k_rank_lean, dim3(padded_grid(c->geo.Q)), dim3(256), (size_t)ch.lds, c->stream, c->cand.as<u8>(), la, c->mbits.as<u32>(), c->geo);
    c->t_end();
    HG_TRY(c->check_launch("k_rank_lean"));
    return rank_lds_done(c, ch, use_recip);
}

static int launch_rank_cnt(hg_ctx* c, int mode, const StepReq& req, const RankChoice& ch) {
    RankLdsArgs la;
    bool use_recip = false;
    HG_TRY(rank_lds_args(c, mode, req, ch, &la, &use_recip));
    la.want_lists = lists_needed(c) ? 1 : 0;
    la.rec8 = c->rec8 ? 1 : 0;
    c->t_begin(KI_RANK_LDS);
    hipLaunchKernelGGL(k_rank_cnt, dim3(c->geo.Q), dim3(256), (size_t)ch.lds, c->stream, c->cand.as<u64>(), la, c->out_idx.as<u32>(),
                       c->out_dist.as<u8>(), c->mbits.as<u32>(), c->geo);
    c->t_end();
    HG_TRY(c->check_launch("k_rank_cnt"));
    return rank_lds_done(c, ch, use_recip);
}

// k_rank_fused in one of its modes, on every query or on those flagged in `only`
static int launch_rank_general(hg_ctx* c, int mode, const StepReq& req, const RankChoice& ch, const u32* only) {
    const Geo& g = c->geo;
    RankArgs ra{c->sl_cnt.as<u32>(), c->tot.as<u32>(), c->failq.as<u32>(), c->err.as<int>(), c->qbad.as<u32>(),
                mode, c->hwq.as<u32>(), c->hown.as<u32>(), c->t.as<int>(), c->cnt_lt.as<u32>(), c->quota.as<u32>(),
                c->tie_before.as<u32>(), c->posbase.as<u32>(),
                c->optimistic ? c->cap : 256u, c->crow, c->optimistic ? 0 : 1, lists_needed(c) ? 1 : 0, ch.bits_lds, c->RW, only,
                req.rows == StepReq::DIRECT ? 1 : 0, c->rec8 ? 1 : 0, c->db.as<u32>(), c->dblab.as<u64>(), c->qc.as<u32>(), c->qlab.as<u64>()};
    const size_t lds_bytes = ((size_t)(ch.nwav + 1) * g.NB + 8 + (ch.bits_lds ? 2 * (size_t)c->RW : 0)) * 4;
    c->t_begin(mode == RANK_COUNT ? KI_CAND_HIST : KI_RANK_FUSED);
    if (ch.nwav == 16)
        hipLaunchKernelGGL(k_rank_fused<16>, dim3(g.Q), dim3(1024), lds_bytes, c->stream, c->cand.as<u64>(), ra,
                           c->out_idx.as<u32>(), c->out_dist.as<u8>(), c->mbits.as<u32>(), nbits_for(g.NB), g);
    else
        hipLaunchKernelGGL(k_rank_fused<4>, dim3(g.Q), dim3(256), lds_bytes, c->stream, c->cand.as<u64>(), ra,
                           c->out_idx.as<u32>(), c->out_dist.as<u8>(), c->mbits.as<u32>(), nbits_for(g.NB), g);
    c->t_end();
    return c->check_launch("k_rank_fused");
}

int launch_rank(hg_ctx* c, RankMode mode, const StepReq& req) {
    const Geo& g = c->geo;
    const RankChoice ch = choose_rank(c, mode, req);
    if (ch.first == RK_NONE) return fail(HG_ERR_STATE, "launch_rank: the byte matrix does not take these tables");
    if (ch.first == RK_DENSE) return launch_rank_dense(c, ch);
    // the prologue every other kernel shares: a bitmap beyond k_rank_fused's LDS is ORed into global memory, the verdict
    // word of a bet (unless the guess kernel cleared it) or the exact rows' overflow flags start from zero
    if (mode != RANK_COUNT && !ch.bits_lds) HG_HIP(hipMemsetAsync(c->mbits.p, 0, (size_t)g.Q * c->RW * 8, c->stream));
    HG_TRY(reserve_rank_out(c, mode, ch.nwav));
    if (mode == RANK_WHOLE) {
        if (c->optimistic) { if (!req.err_zeroed) HG_HIP(hipMemsetAsync(c->err.p, 0, 8, c->stream)); }
        else HG_HIP(hipMemsetAsync(c->failq.p, 0, (size_t)g.Qpad * 4, c->stream));
    }
    c->ap_fused = false; c->last_rank = ch.first;
    switch (ch.first) {
        case RK_LEAN: HG_TRY(launch_rank_lean(c, mode, req, ch)); break;
        case RK_CNT: HG_TRY(launch_rank_cnt(c, mode, req, ch)); break;
        case RK_SLICES: return launch_rank_slices(c, ch, nullptr);
        default: return launch_rank_general(c, mode, req, ch, nullptr);
    }
    return ch.then_general ? launch_rank_general(c, mode, req, ch, c->bigq.as<u32>()) : HG_OK;
}

// The second half of a fused step: k_rank_lean / k_rank_cnt has run (with its AP epilogue) and flagged in bigq the queries it declined;
// rank just those with the general kernel.  No memset (the verdict word and the bitmap are the step's); "rank_variant" stays the step's.
int launch_rank_leftovers(hg_ctx* c) {
    RankChoice ch;
    general_shape(c, true, ch);
    HG_TRY(reserve_rank_out(c, RANK_WHOLE, ch.nwav));
    c->ap_fused = false;
    return launch_rank_general(c, RANK_WHOLE, StepReq{}, ch, c->bigq.as<u32>());
}

// k_order: the exact sequence's placement on several shards, with the plan k_plan made from the gathered histograms
int launch_order(hg_ctx* c) {
    const Geo& g = c->geo;
    const size_t lds_words = (size_t)g.NB + 2 * (size_t)c->RW;
    const int bits_lds = WPB * lds_words * 4 <= 64 * 1024;
    if (!bits_lds) HG_HIP(hipMemsetAsync(c->mbits.p, 0, (size_t)g.Q * c->RW * 8, c->stream));
    OrdArgs oa{c->t.as<int>(), c->cnt_lt.as<u32>(), c->quota.as<u32>(), c->tie_before.as<u32>(), c->posbase.as<u32>(),
               c->tot.as<u32>(), c->crow, lists_needed(c) ? 1 : 0, bits_lds, c->RW};
    c->t_begin(KI_ORDER);
    hipLaunchKernelGGL(k_order, dim3(grid_for(g.Q, WPB)), dim3(256),
                       (size_t)WPB * (g.NB + (bits_lds ? 2 * (size_t)c->RW : 0)) * 4, c->stream, c->cand.as<u64>(), oa,
                       c->out_idx.as<u32>(), c->out_dist.as<u8>(), c->mbits.as<u32>(), nbits_for(g.NB), g);
    c->t_end();
    return c->check_launch("k_order");
}

int preload_rank() {   // (hg_preload: see preload_seq)
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_rank_fused<4>)));
    return HG_OK;
}

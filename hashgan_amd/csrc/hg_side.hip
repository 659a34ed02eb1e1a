// libhashgan_amd.so -- the side metrics: passes next to the ranking that read the tables, the ranked lists or the match bitmap and write
// buffers of their own.  None touches the step state -- stage, geometry, hist / hown, lists, match bits, hg_ap's results -- so a plan, a
// select or a step in flight goes on as if the call had not happened.  Each keeps one SideResult (hg_ctx.hpp; DESIGN.md, "Side metrics: the host side").
#include "hg_ctx.hpp"
#include "hg_hist_rel.hpp"
#include "hg_graded.hpp"
#include "hg_tie_ap.hpp"
#include "hg_ap_at.hpp"
#include "hg_hist_joint.hpp"
#include "hg_votes.hpp"
#include "hg_side_merge.hpp"
#include "hg_list_merge.hpp"
#include "hg_neighbours.hpp"

// the classes of the last label word
static u64 lastmask(int C) { return C % 64 ? (1ull << (C % 64)) - 1ull : ~0ull; }

// Cut-offs handed over by the caller: `n` of them (1..max_n), strictly ascending within 1..bound.
static int check_cutoffs(const char* who, const char* name, const int64_t* host, int n, int max_n, i64 bound, const char* bound_name) {
    if (!host) return fail(HG_ERR_ARG, "%s: null pointer (%s)", who, name);
    if (n < 1 || n > max_n) return fail(HG_ERR_ARG, "%s: %d cut-offs in %s (1..%d)", who, n, name, max_n);
    for (int j = 0; j < n; ++j)
        if (host[j] < 1 || host[j] > bound || (j > 0 && host[j] <= host[j - 1]))
            return fail(HG_ERR_ARG, "%s: %s must be strictly ascending within 1..%lld (%s); %s[%d]=%lld", who, name, (long long)bound, bound_name, name, j, (long long)host[j]);
    return HG_OK;
}

static bool is_shard(const hg_ctx* c) { return !(c->idx_base == 0 && c->N == c->n_total); }
static int whole_database(const hg_ctx* c, const char* who, const char* why) {
    if (!is_shard(c)) return HG_OK;
    return fail(HG_ERR_STATE, "%s: the context holds rows [%lld, %lld) of %lld: %s", who, (long long)c->idx_base, (long long)(c->idx_base + c->N), (long long)c->n_total, why);
}

template <int LWT> static int launch_grade_hist_t(hg_ctx* c, Geo g, int G) {
    // LDS: wpb * G * 64 * 4 bytes (C = 255: two wavefronts, 128 KiB)
    int wpb = WPB;
    while (wpb > 1 && (size_t)wpb * G * 256 > 160u * 1024u) wpb >>= 1;
    g.wpb = wpb;
    g.nBlk = (int)((g.nUnits + wpb - 1) / wpb);
    const size_t lds = (size_t)wpb * G * 256;
    static std::atomic<unsigned long long> lds_allowed{0};
    if (lds > 64 * 1024 && !(lds_allowed.load() >> (c->device & 63) & 1ull)) {
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_grade_hist<LWT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_allowed.fetch_or(1ull << (c->device & 63));
    }
    c->t_begin(KI_GRADE_HIST);
    hipLaunchKernelGGL((k_grade_hist<LWT>), dim3(padded_grid(g.nBlk)), dim3(64 * wpb), lds, c->stream, c->qlab.as<u64>(),
                       c->dblab.as<u64>(), c->gh_part.as<u32>(), g, G, lastmask(c->C));
    c->t_end();
    return c->check_launch("k_grade_hist");
}

// the distance-by-grade histogram: G counters per distance of the band in the lane's column
template <int NW, int LWT> static int launch_hist_joint_t(hg_ctx* c, Geo g, const JointArgs& ja) {
    // LDS: wpb * bw * G * 64 * 4 bytes; a band holds at most HJ_LDS_CELLS cells, so one wavefront always fits 160 KiB
    const size_t column = (size_t)ja.bw * ja.G * 256;
    int wpb = WPB;
    while (wpb > 1 && (size_t)wpb * column > 160u * 1024u) wpb >>= 1;
    g.wpb = wpb;
    g.nBlk = (int)((g.nUnits + wpb - 1) / wpb) * ja.bands;
    const size_t lds = (size_t)wpb * column;
    static std::atomic<unsigned long long> lds_allowed{0};
    if (lds > 64 * 1024 && !(lds_allowed.load() >> (c->device & 63) & 1ull)) {
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hist_joint<NW, LWT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_allowed.fetch_or(1ull << (c->device & 63));
    }
    c->t_begin(KI_HIST_JOINT);
    hipLaunchKernelGGL((k_hist_joint<NW, LWT>), dim3(padded_grid(g.nBlk)), dim3(64 * wpb), lds, c->stream, c->qc.as<u32>(),
                       c->qlab.as<u64>(), c->db.as<u32>(), c->dblab.as<u64>(), c->jh_part.as<u32>(), g, ja);
    c->t_end();
    return c->check_launch("k_hist_joint");
}
template <int NW> static int hist_joint_nw(hg_ctx* c, const Geo& g, const JointArgs& ja) {
    switch (c->LW) {
        case 1: return launch_hist_joint_t<NW, 1>(c, g, ja);
        case 2: return launch_hist_joint_t<NW, 2>(c, g, ja);
        default: return launch_hist_joint_t<NW, 0>(c, g, ja);
    }
}
static int launch_hist_joint(hg_ctx* c, const Geo& g, const JointArgs& ja) { HG_DISPATCH_NW(hist_joint_nw, c, g, ja) }

// One of the three additive tables (hg_side_merge.hpp), seen from hg_pack_side_table and hg_merge_side_table: the shard's own result and
// buffers, the merged ones, the planes of a block and how many of them add up to a query's column total.
struct SideTable {
    const char* name; const char* pass;
    SideResult* own; SideResult* merged;
    DevBuf* src0; DevBuf* src1; DevBuf* dst;
    i64 planes, split, check_planes, dim;
    int Gs, Gc;
};
static int side_table(hg_ctx* c, const char* who, int which, int Gc, bool packing, SideTable* t) {
    const i64 NB = c->NB;
    switch (which) {
        case HG_SIDE_REL:
            *t = SideTable{"rel", "hg_rel_hist", &c->rh, &c->mrh, &c->rh_all, &c->rh_rel, &c->mg_rel, 2 * NB, NB, NB, NB, 1, 1};
            return HG_OK;
        case HG_SIDE_GRADE:
            if (c->C > GR_MAX_C) return fail(HG_ERR_ARG, "%s: C=%d classes (a grade is a byte: at most %d)", who, c->C, GR_MAX_C);
            *t = SideTable{"grade", "hg_grade_hist", &c->gh, &c->mgh, &c->gh_tab, nullptr, &c->mg_grade, c->C + 1, c->C + 1, c->C + 1, c->C + 1, 1, 1};
            return HG_OK;
        case HG_SIDE_JOINT: {
            if (c->C > GR_MAX_C) return fail(HG_ERR_ARG, "%s: C=%d classes (a grade is a byte: at most %d)", who, c->C, GR_MAX_C);
            if (Gc < 1 || Gc > c->C + 1) return fail(HG_ERR_ARG, "%s: Gc=%d grades (1..C + 1 = %d)", who, Gc, c->C + 1);
            const int Gs = packing && c->jh.current(c) ? (int)(c->jh.dim / NB) : Gc;
            *t = SideTable{"joint", "hg_joint_hist", &c->jh, &c->mjh, &c->jh_tab, nullptr, &c->mg_joint, NB * Gc, NB * Gc, NB * Gc, NB * Gc, Gs, Gc};
            return HG_OK;
        }
        default: return fail(HG_ERR_ARG, "%s: which=%d (HG_SIDE_REL, HG_SIDE_GRADE or HG_SIDE_JOINT)", who, which);
    }
}

// The sizes of the two list exchange units (hg_list_merge.hpp) for the ranking and tables held now.
struct ListGeo { i64 Q, Qpad, R, Rp; };
static ListGeo list_geometry(const hg_ctx* c) {
    const Geo g = full_geometry(c);
    return ListGeo{g.Q, g.Qpad, c->geo.R, (c->geo.R + 15) / 16 * 16};
}
// the cut-offs into lm_tab as a kernel argument: no host array has to outlive the call, so the pack need not synchronise
static int put_cutoffs(hg_ctx* c, const int64_t* host_ks, int nk) {
    Cutoffs k{};
    for (int j = 0; j < nk; ++j) k.v[j] = host_ks[j];
    hipLaunchKernelGGL(k_put_cutoffs, dim3(1), dim3(64), 0, c->stream, k, c->lm_tab.as<i64>(), nk);
    return c->check_launch("k_put_cutoffs");
}
static int list_kind(hg_ctx* c, const char* who, int which) {
    if (which != HG_LIST_GRADES && which != HG_LIST_VOTES) return fail(HG_ERR_ARG, "%s: which=%d (HG_LIST_GRADES or HG_LIST_VOTES)", who, which);
    if (c->C > GR_MAX_C) return fail(HG_ERR_ARG, "%s: C=%d classes (at most %d)", who, c->C, GR_MAX_C);
    return HG_OK;
}

// Neighbour sets (hg_neighbours.hpp): k_nbr_sort on row q = src + q * stride of Q rows into nb_ids / nb_cnt, then its flag word back to
// the host (one synchronisation).  *flag: NB_FLAG_DUP | NB_FLAG_RANGE.
static int sort_neighbours(hg_ctx* c, const u32* src, i64 stride, i64 Q, int G, u32* flag) {
    int P = 64;
    while (P < G) P <<= 1;
    const size_t lds = (size_t)(P + NB_SORT_EXTRA) * 4;
    static std::atomic<unsigned long long> lds_allowed{0};
    if (lds > 64 * 1024 && !(lds_allowed.load() >> (c->device & 63) & 1ull)) {
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nbr_sort), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_allowed.fetch_or(1ull << (c->device & 63));
    }
    HG_HIP(hipMemsetAsync(c->nb_flag.p, 0, 4, c->stream));
    NbrSortArgs a;
    a.src = src; a.stride = stride;
    a.ids = c->nb_ids.as<u32>(); a.count = c->nb_cnt.as<u32>(); a.flag = c->nb_flag.as<u32>();
    a.G = G; a.P = P; a.n_total = c->n_total;
    c->t_begin(KI_NBR_SORT);
    if (Q > 0) hipLaunchKernelGGL(k_nbr_sort, dim3((unsigned)Q), dim3(P <= NB_SORT_SMALL ? 256 : NB_SORT_THREADS), lds, c->stream, a);
    c->t_end();
    HG_TRY(c->check_launch("k_nbr_sort"));
    HG_HIP(hipMemcpyAsync(flag, c->nb_flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}
// the set's buffers for Q sets of G ids (first reservations: no buffer of a blind step moves)
static int reserve_neighbours(hg_ctx* c, i64 Q, int G, bool staged) {
    const FirstReservations first;
    HG_TRY(c->nb_ids.reserve((size_t)(Q > 0 ? Q : 1) * G * 4));
    HG_TRY(c->nb_cnt.reserve((size_t)(Q > 0 ? Q : 1) * 4));
    HG_TRY(c->nb_flag.reserve(16));
    if (staged) HG_TRY(c->nb_stage.reserve((size_t)(Q > 0 ? Q : 1) * G * 4));
    first.keep(c);
    return HG_OK;
}
// the ranked index lists hg_votes accepts on a whole-database context
static bool lists_on_device(const hg_ctx* c) { return (c->stage & ST_SELECT) && (c->lists_valid || c->real_lists); }

extern "C" {

// The relevant-row histogram (hg_hist_rel.hpp): one pass over the pairs leaves all[d][q] (rows at distance d) and rel[d][q] (those
// that share a label with the query), in the full pass's geometry (do_hist(c, 1)).
int hg_rel_hist(hg_ctx* c) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_rel_hist", "hg_set_database + hg_set_queries"));
    const Geo g = full_geometry(c);
    c->rh.begin();
    const FirstReservations first;
    const size_t plane = (size_t)g.NB * g.Qpad * 4;
    HG_TRY(c->rh_part.reserve(2 * plane * g.S));
    HG_TRY(c->rh_all.reserve(plane));
    HG_TRY(c->rh_rel.reserve(plane));
    first.keep(c);
    HG_TRY(launch_hist_rel(c, g));
    c->last_rel_hist = 1;
    c->t_begin(KI_HIST_REL_REDUCE);
    hipLaunchKernelGGL(k_hist_rel_reduce, dim3(grid_for((i64)g.NB * g.Qpad)), dim3(256), 0, c->stream, c->rh_part.as<u32>(),
                       c->rh_all.as<u32>(), c->rh_rel.as<u32>(), g);
    c->t_end();
    HG_TRY(c->check_launch("k_hist_rel_reduce"));
    c->rh.finish(c, g.Q, g.Qpad, g.NB);
    return c->stage_end();
}

// Graded relevance along the ranked lists (hg_graded.hpp): per query and cut-off k of `host_ks`, the sum of the grades, the ranks with a
// grade, the discounted gain and the sum WAP averages, from the idx lists the last ranking left in out_idx -- hg_topr, a staged
// select with lists, hg_topr_real.  The host tables are copied before the call returns (it synchronises whatever "stage_sync" says).
int hg_graded(hg_ctx* c, const int64_t* host_ks, int nk, const double* host_gain, const double* host_disc, int keep_grades) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_graded", "hg_set_database + hg_set_queries"));
    c->gr.begin();
    // a shard: the merged grade plane of the whole database's lists (hg_merge_list_table) stands in for the gather through out_idx
    const bool plane_fed = is_shard(c) && c->mlg.current(c);
    if (!plane_fed) HG_TRY(whole_database(c, "hg_graded", "graded sums need the whole database in one context (lists of a shard are partial)"));
    if (!plane_fed && (!(c->stage & ST_SELECT) || !(c->lists_valid || c->real_lists)))
        return fail(HG_ERR_STATE, "hg_graded: no ranked lists on the device (hg_map and hg_map_real write none): call hg_topr / hg_topr_real first");
    if (c->C > GR_MAX_C) return fail(HG_ERR_ARG, "hg_graded: C=%d classes (a grade is a byte: at most %d)", c->C, GR_MAX_C);
    if (!host_gain || !host_disc) return fail(HG_ERR_ARG, "hg_graded: null pointer");
    const i64 Q = plane_fed ? c->mlg.Q : c->geo.Q, R = plane_fed ? c->mlg.dim : c->geo.R;
    HG_TRY(check_cutoffs("hg_graded", "ks", host_ks, nk, GR_MAX_K, R, "R"));
    const i64 kmax = host_ks[nk - 1];
    const size_t o_gain = GR_MAX_K * 8, o_disc = o_gain + (size_t)(c->C + 1) * 8, tab = o_disc + (size_t)kmax * 8;
    const size_t plane = (size_t)Q * nk * 8;
    const FirstReservations first;
    HG_TRY(c->gr_tab.reserve(tab));
    HG_TRY(c->gr_out.reserve(4 * plane));
    if (keep_grades) HG_TRY(c->gr_grades.reserve((size_t)Q * R));
    first.keep(c);
    char* t = c->gr_tab.as<char>();
    HG_HIP(hipMemcpyAsync(t, host_ks, (size_t)nk * 8, hipMemcpyHostToDevice, c->stream));
    HG_HIP(hipMemcpyAsync(t + o_gain, host_gain, (size_t)(c->C + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HG_HIP(hipMemcpyAsync(t + o_disc, host_disc, (size_t)kmax * 8, hipMemcpyHostToDevice, c->stream));
    char* o = c->gr_out.as<char>();
    GradedArgs a;
    a.idx = c->out_idx.as<u32>(); a.dblab = c->dblab.as<u64>(); a.qlab = c->qlab.as<u64>();
    a.ks = (const i64*)t; a.gain = (const double*)(t + o_gain); a.disc = (const double*)(t + o_disc);
    a.gsum = (i64*)o; a.hits = (i64*)(o + plane); a.dcg = (double*)(o + 2 * plane); a.wsum = (double*)(o + 3 * plane);
    a.grades = keep_grades ? c->gr_grades.as<u8>() : nullptr;
    a.R = R; a.N = c->N; a.nk = nk; a.LW = c->LW;
    a.lastmask = lastmask(c->C);
    a.plane = plane_fed ? c->lm_grades.as<u8>() : nullptr; a.Rp = plane_fed ? c->mlg.Qpad : 0;
    c->t_begin(KI_GRADED);
    if (plane_fed) hipLaunchKernelGGL(k_graded<true>, dim3((unsigned)Q), dim3(GR_THREADS), 0, c->stream, a);
    else hipLaunchKernelGGL(k_graded<false>, dim3((unsigned)Q), dim3(GR_THREADS), 0, c->stream, a);
    c->t_end();
    HG_TRY(c->check_launch("k_graded"));
    HG_TRY(c->sync());                                 // (the host tables are the caller's)
    c->gr_kept = keep_grades != 0; c->gr_R = R;
    c->gr.finish(c, Q, Q, nk);
    return HG_OK;
}

// The grade histogram of this shard (hg_graded.hpp): rows per (grade, query) in one pass over the label pairs, in the full pass's
// geometry like hg_rel_hist.
int hg_grade_hist(hg_ctx* c) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_grade_hist", "hg_set_database + hg_set_queries"));
    if (c->C > GR_MAX_C) return fail(HG_ERR_ARG, "hg_grade_hist: C=%d classes (a grade is a byte: at most %d)", c->C, GR_MAX_C);
    const Geo g = full_geometry(c);
    c->gh.begin();
    const int G = c->C + 1;
    const FirstReservations first;
    const i64 plane = (i64)G * g.Qpad;
    HG_TRY(c->gh_part.reserve((size_t)plane * 4 * g.S));
    HG_TRY(c->gh_tab.reserve((size_t)plane * 4));
    first.keep(c);
    switch (c->LW) {
        case 1: HG_TRY(launch_grade_hist_t<1>(c, g, G)); break;
        case 2: HG_TRY(launch_grade_hist_t<2>(c, g, G)); break;
        default: HG_TRY(launch_grade_hist_t<0>(c, g, G)); break;
    }
    c->t_begin(KI_GRADE_HIST_REDUCE);
    hipLaunchKernelGGL(k_grade_hist_reduce, dim3(grid_for(plane)), dim3(256), 0, c->stream, c->gh_part.as<u32>(), c->gh_tab.as<u32>(), plane, g.S);
    c->t_end();
    HG_TRY(c->check_launch("k_grade_hist_reduce"));
    c->gh.finish(c, g.Q, g.Qpad, G);
    return c->stage_end();
}

// The distance-by-grade histogram of this shard (hg_hist_joint.hpp): rows per (distance, grade, query) in one pass over the pairs.
// G = 1 + min(most labels on a query, most labels on a database row) comes from a max-reduce over the two label tables (one
// synchronisation: the host sizes the buffers and the LDS column by it).  A geometry of its own, cut from the full pass's: the bands
// multiply the grid, so the segments are divided by them -- c->geo is not touched.
int hg_joint_hist(hg_ctx* c) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_joint_hist", "hg_set_database + hg_set_queries"));
    if (c->C > GR_MAX_C) return fail(HG_ERR_ARG, "hg_joint_hist: C=%d classes (a grade is a byte: at most %d)", c->C, GR_MAX_C);
    Geo g = full_geometry(c);
    c->jh.begin();
    const FirstReservations first;
    HG_TRY(c->jh_max.reserve(8));
    HG_HIP(hipMemsetAsync(c->jh_max.p, 0, 8, c->stream));
    c->t_begin(KI_LABEL_MAX);
    hipLaunchKernelGGL(k_label_max, dim3(grid_for((i64)g.Qpad + c->N)), dim3(256), 0, c->stream, c->qlab.as<u64>(), c->dblab.as<u64>(),
                       c->Q, (i64)g.Qpad, c->N, c->LW, lastmask(c->C), c->jh_max.as<u32>());
    c->t_end();
    HG_TRY(c->check_launch("k_label_max"));
    u32 most[2] = {0, 0};
    HG_HIP(hipMemcpyAsync(most, c->jh_max.p, 8, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    JointArgs ja;
    ja.G = 1 + (int)(most[0] < most[1] ? most[0] : most[1]);
    if (ja.G > c->C + 1) return fail(HG_ERR_HIP, "hg_joint_hist: %d grades from %d classes", ja.G, c->C);   // (the popcounts are masked: cannot happen)
    ja.bw = g.NB * ja.G <= HJ_LDS_CELLS ? g.NB : HJ_LDS_CELLS / ja.G;      // (G <= 256: a band has at least two distances)
    ja.bands = (g.NB + ja.bw - 1) / ja.bw;
    ja.lastmask = lastmask(c->C);
    if (ja.bands > 1) {                                // S x bands ~ the full pass's S
        const i64 S = (g.S + ja.bands / 2) / ja.bands > 1 ? (g.S + ja.bands / 2) / ja.bands : 1;
        g.L = ((c->N + S - 1) / S + 31) / 32 * 32;
        g.S = (int)((c->N + g.L - 1) / g.L);
        g.nUnits = (i64)g.S * g.nQT;
    }
    const i64 plane = (i64)g.NB * ja.G * g.Qpad;
    HG_TRY(c->jh_part.reserve((size_t)plane * 4 * g.S));
    HG_TRY(c->jh_tab.reserve((size_t)plane * 4));
    first.keep(c);
    HG_TRY(launch_hist_joint(c, g, ja));
    c->jh_G = ja.G; c->jh_bands = ja.bands;
    c->t_begin(KI_HIST_JOINT_REDUCE);
    hipLaunchKernelGGL(k_hist_joint_reduce, dim3(grid_for(plane)), dim3(256), 0, c->stream, c->jh_part.as<u32>(), c->jh_tab.as<u32>(), plane, g.S);
    c->t_end();
    HG_TRY(c->check_launch("k_hist_joint_reduce"));
    c->jh.finish(c, g.Q, g.Qpad, (i64)g.NB * ja.G);
    return c->stage_end();
}

// Tie-aware AP at the cut-offs `host_Rs` (hg_tie_ap.hpp): expectation, hit probability, minimum and maximum of AP@R over the orders
// inside the tie groups, from hg_rel_hist's two tables alone.  Runs that pass when the tables of the current generations are not
// there and reuses them otherwise.  The host array is copied before the call returns (it synchronises whatever "stage_sync" says).
int hg_tie_ap(hg_ctx* c, const int64_t* host_Rs, int nR) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_tie_ap", "hg_set_database + hg_set_queries"));
    c->ta.begin();
    // a shard: the merged table of the whole database (hg_merge_side_table) stands in for the shard's own, the cut-offs reach n_total
    const bool shard = !(c->idx_base == 0 && c->N == c->n_total);
    if (shard && !c->mrh.current(c))
        HG_TRY(whole_database(c, "hg_tie_ap", "the cut at R needs the tables of the whole database: merge the shards' (hg_pack_side_table, hg_merge_side_table) first"));
    HG_TRY(check_cutoffs("hg_tie_ap", "Rs", host_Rs, nR, TA_MAX_R, shard ? c->n_total : c->N, shard ? "n_total" : "N"));
    if (c->NB > TA_THREADS) return fail(HG_ERR_ARG, "hg_tie_ap: b=%d bits (at most %d)", c->b, TA_THREADS - 1);
    if (!shard && !c->rh.current(c)) HG_TRY(hg_rel_hist(c));
    const SideResult& tab = shard ? c->mrh : c->rh;
    const i64 Q = tab.Q;
    const size_t plane = (size_t)Q * nR * 8;
    const FirstReservations first;
    HG_TRY(c->ta_tab.reserve(TA_MAX_R * 8));
    HG_TRY(c->ta_out.reserve(7 * plane));
    first.keep(c);
    HG_HIP(hipMemcpyAsync(c->ta_tab.p, host_Rs, (size_t)nR * 8, hipMemcpyHostToDevice, c->stream));
    char* o = c->ta_out.as<char>();
    TieApArgs a;
    a.all = shard ? c->mg_rel.as<u32>() : c->rh_all.as<u32>();
    a.rel = shard ? c->mg_rel.as<u32>() + tab.dim * tab.Qpad : c->rh_rel.as<u32>();
    a.Rs = c->ta_tab.as<i64>();
    a.ap_exp = (double*)o; a.p_hit = (double*)(o + plane); a.ap_min = (double*)(o + 2 * plane); a.ap_max = (double*)(o + 3 * plane);
    a.rel_exp = (double*)(o + 4 * plane); a.rel_lo = (i64*)(o + 5 * plane); a.rel_hi = (i64*)(o + 6 * plane);
    a.Qpad = tab.Qpad; a.NB = (int)tab.dim; a.nR = nR;
    c->t_begin(KI_TIE_AP);
    hipLaunchKernelGGL(k_tie_ap, dim3((unsigned)Q, (unsigned)nR), dim3(TA_THREADS), 0, c->stream, a);
    c->t_end();
    HG_TRY(c->check_launch("k_tie_ap"));
    HG_TRY(c->sync());                                 // (the host array is the caller's)
    c->ta.finish(c, Q, Q, nR);
    return HG_OK;
}

// AP@R and the hits among the top R at the cut-offs `host_Rs` from the match bitmap the last ranking left, in one pass per query
// (hg_ap_at.hpp).  Tables of its own -- the one-R AP tables stay the ranking's; the host array is copied before the call returns
// (it synchronises whatever "stage_sync" says).
int hg_ap_at(hg_ctx* c, const int64_t* host_Rs, int nR) {
    HG_TRY(need(c, ST_MATCH, "hg_ap_at", "a ranking that leaves the whole match bitmap (hg_topr, hg_topr_real, hg_map, hg_match, a merge of all queries)"));
    c->aa.begin();
    if (c->ranked_local) return fail(HG_ERR_STATE, "hg_ap_at: the match bitmap is in this shard's local rank order (hg_select_ranked): merge it first");
    if (c->G > 1 && !c->mbits_merged)
        return fail(HG_ERR_STATE, "hg_ap_at: the match bitmap holds this shard's rows only (%d shards): merge it first (hg_merge_match, hg_merge_ranked)", c->G);
    if (c->mbits_in_ws_b) return fail(HG_ERR_STATE, "hg_ap_at: the last ranking was a step of hg_map_begin in its own workspace: rank with hg_topr / hg_map first");
    const i64 Q = c->geo.Q, R = c->geo.R;
    HG_TRY(check_cutoffs("hg_ap_at", "Rs", host_Rs, nR, AA_MAX_R, R, "R of the last ranking"));
    const i64 Rmax = host_Rs[nR - 1];
    // host image of the tables: the cut-offs, the full chunk's tree, one tree per cut-off for its last chunk
    const size_t o_shapes = AA_MAX_R * 8, tab = o_shapes + sizeof(ApShape) * (size_t)(1 + nR);
    std::vector<char> img(tab, 0);
    memcpy(img.data(), host_Rs, (size_t)nR * 8);
    ApShape* sh = reinterpret_cast<ApShape*>(img.data() + o_shapes);
    build_shape(AP_CHUNK, sh[0]);
    for (int j = 0; j < nR; ++j) build_shape((int)(host_Rs[j] % AP_CHUNK), sh[1 + j]);
    const size_t n = (size_t)Q * nR;
    const FirstReservations first;
    HG_TRY(c->aa_tab.reserve(tab));
    HG_TRY(c->aa_out.reserve(n * 12));
    // reciprocals of the ranks (ensure_ap_tables' rule: lists beyond 2^20 divide): the ranking's table if it is there, else one of its own
    const bool use_recip = c->opt.ap_recip && Rmax <= (1ll << 20);
    const double* recip = nullptr;
    if (use_recip && c->recip_for_R == R && c->ap_recip.p) {
        recip = c->ap_recip.as<double>();
    } else if (use_recip) {
        if (c->aa_recip_n < Rmax) {
            HG_TRY(c->aa_recip.reserve((size_t)(Rmax + 1 + AP_RECIP_SLACK) * 8));
            hipLaunchKernelGGL(k_recip_table, dim3(grid_for(Rmax + 1 + AP_RECIP_SLACK)), dim3(256), 0, c->stream, c->aa_recip.as<double>(), Rmax + AP_RECIP_SLACK);
            HG_TRY(c->check_launch("k_recip_table"));
            c->aa_recip_n = Rmax;
        }
        recip = c->aa_recip.as<double>();
    }
    first.keep(c);
    HG_HIP(hipMemcpyAsync(c->aa_tab.p, img.data(), tab, hipMemcpyHostToDevice, c->stream));
    ApAtArgs a;
    a.mbits = c->mbits.as<u64>(); a.RW = c->RW;
    a.Rs = c->aa_tab.as<i64>(); a.shapes = (const ApShape*)(c->aa_tab.as<char>() + o_shapes);
    a.recip = recip;
    a.ap = c->aa_out.as<double>(); a.rel = (u32*)(c->aa_out.as<char>() + n * 8);
    a.nR = nR;
    // few queries with long lists: four times the threads per query (do_ap_range's rule, on the longest list)
    const bool wide = Q * 2 < (i64)c->n_cu * 8 && Rmax > 2 * AP_CHUNK && c->opt.ap_wide;
    c->t_begin(KI_AP_AT);
    if (Q > 0 && wide) hipLaunchKernelGGL(k_ap_at<512>, dim3((unsigned)Q), dim3(512), 0, c->stream, a);
    else if (Q > 0) hipLaunchKernelGGL(k_ap_at<AP_THREADS>, dim3((unsigned)Q), dim3(AP_THREADS), 0, c->stream, a);
    c->t_end();
    HG_TRY(c->check_launch("k_ap_at"));
    HG_TRY(c->sync());                                 // (the host image goes out of scope)
    c->aa.finish(c, Q, Q, nR);
    return HG_OK;
}

// Class votes along the ranked lists (hg_votes.hpp): per query and cut-off k of `host_ks`, how many of the first k ranks carry each class,
// the largest count and the smallest class that reaches it; and per cut-off the confusion matrix over the queries' own labels.  The lists
// are hg_graded's: whatever the last ranking left in out_idx.  The host array is copied before the call returns (it synchronises
// whatever "stage_sync" says).
int hg_votes(hg_ctx* c, const int64_t* host_ks, int nk) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_votes", "hg_set_database + hg_set_queries"));
    c->vt.begin();
    // a shard: the merged vote counts of the whole database's lists (hg_merge_list_table) stand in for the walk along out_idx
    const bool merged_fed = is_shard(c) && c->mlv.current(c);
    if (!merged_fed) HG_TRY(whole_database(c, "hg_votes", "class votes need the whole database in one context (lists of a shard are partial)"));
    if (!merged_fed && (!(c->stage & ST_SELECT) || !(c->lists_valid || c->real_lists)))
        return fail(HG_ERR_STATE, "hg_votes: no ranked lists on the device (hg_map and hg_map_real write none): call hg_topr / hg_topr_real first");
    if (c->C > VT_MAX_C) return fail(HG_ERR_ARG, "hg_votes: C=%d classes (at most %d)", c->C, VT_MAX_C);
    const i64 Q = merged_fed ? c->mlv.Q : c->geo.Q, R = c->geo.R;
    HG_TRY(check_cutoffs("hg_votes", "ks", host_ks, nk, VT_MAX_K, R, "R"));
    if (merged_fed && (nk != (int)c->mlv.dim || memcmp(host_ks, c->mlv_ks, (size_t)nk * 8)))
        return fail(HG_ERR_ARG, "hg_votes: on a shard ks must be the %d cut-offs the vote tables were merged at (hg_merge_list_table)", (int)c->mlv.dim);
    const size_t n = (size_t)Q * nk, conf_bytes = (size_t)nk * c->C * c->C * 8;
    const FirstReservations first;
    HG_TRY(c->vt_tab.reserve(VT_MAX_K * 8));
    HG_TRY(c->vt_votes.reserve(n * c->C * 4));
    HG_TRY(c->vt_pred.reserve(n * 8));
    HG_TRY(c->vt_conf.reserve(conf_bytes));
    first.keep(c);
    HG_HIP(hipMemcpyAsync(c->vt_tab.p, host_ks, (size_t)nk * 8, hipMemcpyHostToDevice, c->stream));
    HG_HIP(hipMemsetAsync(c->vt_conf.p, 0, conf_bytes, c->stream));
    VotesArgs a;
    a.idx = c->out_idx.as<u32>(); a.dblab = c->dblab.as<u64>(); a.ks = c->vt_tab.as<i64>();
    a.votes = c->vt_votes.as<u32>(); a.pred = c->vt_pred.as<int>(); a.top = c->vt_pred.as<u32>() + n;
    a.R = R; a.N = c->N; a.nk = nk; a.LW = c->LW; a.C = c->C;
    a.lastmask = lastmask(c->C);
    a.idx_base = 0; a.Qpad = 0;
    if (merged_fed) {
        HG_HIP(hipMemcpyAsync(c->vt_votes.p, c->lm_votes.p, n * c->C * 4, hipMemcpyDeviceToDevice, c->stream));
        VotePickArgs k;
        k.votes = a.votes; k.pred = a.pred; k.top = a.top; k.n = (i64)n; k.C = c->C;
        c->t_begin(KI_VOTE_PICK);
        if (n > 0) hipLaunchKernelGGL(k_vote_pick, dim3(grid_for((i64)n, 4)), dim3(256), 0, c->stream, k);
        c->t_end();
        HG_TRY(c->check_launch("k_vote_pick"));
    } else {
        c->t_begin(KI_VOTES);
#if HG_PROBES
        if (c->opt.probe_votes) hipLaunchKernelGGL(k_votes<true>, dim3((unsigned)Q), dim3(VT_THREADS), 0, c->stream, a);
        else
#endif
        hipLaunchKernelGGL(k_votes<false>, dim3((unsigned)Q), dim3(VT_THREADS), 0, c->stream, a);
        c->t_end();
        HG_TRY(c->check_launch("k_votes"));
    }
    ConfArgs f;
    f.votes = a.votes; f.qlab = c->qlab.as<u64>(); f.conf = c->vt_conf.as<unsigned long long>();
    f.Q = Q; f.nk = nk; f.LW = c->LW; f.C = c->C;
    c->t_begin(KI_VOTE_CONFUSION);
    hipLaunchKernelGGL(k_vote_confusion, dim3((unsigned)c->C, (unsigned)nk, (unsigned)((Q + VC_SEG - 1) / VC_SEG)), dim3(256), 0, c->stream, f);
    c->t_end();
    HG_TRY(c->check_launch("k_vote_confusion"));
    HG_TRY(c->sync());                                 // (the host array is the caller's)
    c->vt.finish(c, Q, Q, nk);
    return HG_OK;
}

// Label-free relevance (hg_neighbours.hpp): NB(q), a set of at most G distinct global row numbers per loaded query, sorted on the device.
// A table of the loaded queries and database like every side result (nb): a reload of either and hg_trim end it, and so does a refused
// call.  A new set also ends the histogram of the previous one (nh).
int hg_set_neighbours(hg_ctx* c, const uint32_t* host_ids, int64_t Q, int G) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_set_neighbours", "hg_set_database + hg_set_queries"));
    c->nb.begin(); c->nh.begin();
    HG_TRY(whole_database(c, "hg_set_neighbours", "neighbour sets need the whole database in one context"));
    if (!host_ids) return fail(HG_ERR_ARG, "hg_set_neighbours: null pointer");
    if (Q != c->Q) return fail(HG_ERR_ARG, "hg_set_neighbours: Q=%lld sets for %lld loaded queries", (long long)Q, (long long)c->Q);
    if (G < 1 || G > NB_MAX_G) return fail(HG_ERR_ARG, "hg_set_neighbours: G=%d ids per set (1..%d)", G, NB_MAX_G);
    HG_TRY(reserve_neighbours(c, Q, G, true));
    if (Q > 0) HG_HIP(hipMemcpyAsync(c->nb_stage.p, host_ids, (size_t)Q * G * 4, hipMemcpyHostToDevice, c->stream));
    u32 flag = 0;
    HG_TRY(sort_neighbours(c, c->nb_stage.as<u32>(), G, Q, G, &flag));    // (synchronises: the host table is the caller's again)
    if (flag)
        return fail(HG_ERR_ARG, "hg_set_neighbours: %s%s%s", flag & NB_FLAG_DUP ? "a set holds the same id twice" : "", flag == (NB_FLAG_DUP | NB_FLAG_RANGE) ? "; " : "",
                    flag & NB_FLAG_RANGE ? "a set holds an id outside the database (0xFFFFFFFF pads a shorter set)" : "");
    c->nb.finish(c, Q, Q, G);
    return HG_OK;
}

// ... the same from the first G ranks of the ranked index lists the last ranking left on the device (hg_votes' precondition): the exact
// float32 top G of hg_topr_real becomes the ground truth without leaving the GPU.  The lists are read only.
int hg_neighbours_from_lists(hg_ctx* c, int G) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_neighbours_from_lists", "hg_set_database + hg_set_queries"));
    c->nb.begin(); c->nh.begin();
    HG_TRY(whole_database(c, "hg_neighbours_from_lists", "neighbour sets need the whole database in one context"));
    if (!lists_on_device(c))
        return fail(HG_ERR_STATE, "hg_neighbours_from_lists: no ranked lists on the device (hg_map and hg_map_real write none): call hg_topr / hg_topr_real first");
    const i64 Q = c->geo.Q, R = c->geo.R;
    if (G < 1 || G > NB_MAX_G || G > R) return fail(HG_ERR_ARG, "hg_neighbours_from_lists: G=%d (1..min(R=%lld, %d))", G, (long long)R, NB_MAX_G);
    HG_TRY(reserve_neighbours(c, Q, G, false));
    u32 flag = 0;
    HG_TRY(sort_neighbours(c, c->out_idx.as<u32>(), R, Q, G, &flag));
    if (flag) return fail(HG_ERR_STATE, "hg_neighbours_from_lists: the first %d ranks of a list hold a repeated or foreign row (flag %u)", G, flag);
    c->nb.finish(c, Q, Q, G);
    return HG_OK;
}

// The match bitmap from the neighbour sets instead of the label words: slot k of query q matches iff idx[q][k] is in NB(q).  Through
// the ranked index lists in global rank order for all queries -- the lists hg_votes accepts on a whole-database context.  Sets the match
// stage, clears the AP stage; hg_ap, hg_ap_at, hg_get_match and hg_export go on unchanged.  The next ranking brings the label bits back.
int hg_match_neighbours(hg_ctx* c) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_match_neighbours", "hg_set_database + hg_set_queries"));
    if (!c->nb.current(c)) return fail(HG_ERR_STATE, "hg_match_neighbours: no neighbour sets of the tables loaded now: call hg_set_neighbours or hg_neighbours_from_lists first");
    HG_TRY(whole_database(c, "hg_match_neighbours", "neighbour sets need the whole database in one context"));
    if (!lists_on_device(c))
        return fail(HG_ERR_STATE, "hg_match_neighbours: no ranked lists on the device (hg_map, hg_map_real and hg_map_begin write none): call hg_topr, hg_topr_real, hg_topr_asym or hg_topr_rerank first");
    if (c->ranked_local) return fail(HG_ERR_STATE, "hg_match_neighbours: the lists are in this shard's local rank order (hg_select_ranked)");
    if (c->G > 1) return fail(HG_ERR_STATE, "hg_match_neighbours: the lists hold one of %d shards' rows", c->G);
    if (c->mbits_in_ws_b || c->ms_n) return fail(HG_ERR_STATE, "hg_match_neighbours: a step of hg_map_begin is in flight or was the last ranking: rank with hg_topr first");
    if (c->verdict_pending) return fail(HG_ERR_STATE, "hg_match_neighbours: the bet's verdict is pending (defer_verdict): ask hg_bet_verdict first");
    const i64 Q = c->geo.Q, R = c->geo.R;
    if (Q != c->nb.Q) return fail(HG_ERR_STATE, "hg_match_neighbours: %lld ranked queries, %lld neighbour sets", (long long)Q, (long long)c->nb.Q);
    const int G = (int)c->nb.dim;
    const i64 nCB = (R + NM_CHUNK - 1) / NM_CHUNK;
    if (nCB * Q > 0x7FFFFFFFll) return fail(HG_ERR_ARG, "hg_match_neighbours: Q*R too large for one launch");
    HG_TRY(c->mbits.reserve((size_t)Q * c->RW * 8));       // (the ranking's own: it is large enough already)
    const size_t lds = (size_t)G * 4;
    static std::atomic<unsigned long long> lds_allowed{0};
    if (lds > 48 * 1024 && !(lds_allowed.load() >> (c->device & 63) & 1ull)) {
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nbr_match), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_allowed.fetch_or(1ull << (c->device & 63));
    }
    NbrMatchArgs a;
    a.idx = c->out_idx.as<u32>(); a.ids = c->nb_ids.as<u32>(); a.count = c->nb_cnt.as<u32>(); a.mbits = c->mbits.as<u64>();
    a.R = R; a.RW = c->RW; a.N = c->N; a.G = G; a.nCB = (int)nCB; a.idx_base = c->idx_base;
    c->t_begin(KI_NBR_MATCH);
    if (Q > 0) hipLaunchKernelGGL(k_nbr_match, dim3((unsigned)(nCB * Q)), dim3(NM_THREADS), lds, c->stream, a);
    c->t_end();
    HG_TRY(c->check_launch("k_nbr_match"));
    c->stage |= ST_MATCH;
    c->stage &= ~(unsigned)ST_AP;
    c->bitmap_changed();
    c->match_source = 1;
    return c->stage_end();
}

// The neighbour distance histogram: nbr[d][q] = the neighbours of q at Hamming distance d, Q x G pairs through the packed codes.  The
// shape and meaning of hg_rel_hist's relevant table; a table of its own (nh), the staged pipeline's state and the other results untouched.
int hg_nbr_hist(hg_ctx* c) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_nbr_hist", "hg_set_database + hg_set_queries"));
    c->nh.begin();
    if (!c->nb.current(c)) return fail(HG_ERR_STATE, "hg_nbr_hist: no neighbour sets of the tables loaded now: call hg_set_neighbours or hg_neighbours_from_lists first");
    const Geo g = full_geometry(c);
    if (g.Q != c->nb.Q) return fail(HG_ERR_STATE, "hg_nbr_hist: %d loaded queries, %lld neighbour sets", g.Q, (long long)c->nb.Q);
    if (g.NB > 256 || g.NW > 8) return fail(HG_ERR_ARG, "hg_nbr_hist: codes of %d words", g.NW);
    const FirstReservations first;
    HG_TRY(c->nh_tab.reserve((size_t)g.NB * g.Qpad * 4));
    first.keep(c);
    NbrHistArgs a;
    a.qc = c->qc.as<u32>(); a.db = c->db.as<u32>(); a.ids = c->nb_ids.as<u32>(); a.nbr = c->nh_tab.as<u32>();
    a.N = c->N; a.Qpad = g.Qpad; a.G = (int)c->nb.dim; a.NW = g.NW; a.NB = g.NB;
    c->t_begin(KI_NBR_HIST);
    if (g.Q > 0) hipLaunchKernelGGL(k_nbr_hist, dim3((unsigned)g.Q), dim3(NH_THREADS), 0, c->stream, a);
    c->t_end();
    HG_TRY(c->check_launch("k_nbr_hist"));
    c->nh.finish(c, g.Q, g.Qpad, g.NB);
    return c->stage_end();
}

// A shard's current table `which` as one block in the exchange layout (hg_side_merge.hpp): u32 [planes][Qpad], for the joint table
// zero-padded in g to the common grade count Gc.  The block is the context's (mg_pack) and holds until the next pack.
int hg_pack_side_table(hg_ctx* c, int which, int Gc, void** dev_ptr, int64_t* nbytes) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_pack_side_table", "hg_set_database + hg_set_queries"));
    if (!dev_ptr || !nbytes) return fail(HG_ERR_ARG, "hg_pack_side_table: null pointer");
    if (which == HG_SIDE_JOINT && c->C <= GR_MAX_C && !c->jh.current(c))        // (before Gc is looked at: without the pass there is no Gs)
        return fail(HG_ERR_STATE, "hg_pack_side_table: no joint table of the tables loaded now: call hg_joint_hist first");
    SideTable t;
    HG_TRY(side_table(c, "hg_pack_side_table", which, which == HG_SIDE_JOINT ? Gc : 1, true, &t));
    if (!t.own->current(c)) return fail(HG_ERR_STATE, "hg_pack_side_table: no %s table of the tables loaded now: call %s first", t.name, t.pass);
    if (t.Gc < t.Gs) return fail(HG_ERR_ARG, "hg_pack_side_table: Gc=%d is less than this shard's %d grades (stat joint_hist_grades)", t.Gc, t.Gs);
    const i64 Qpad = t.own->Qpad, cells = t.planes * Qpad;
    const FirstReservations first;
    HG_TRY(c->mg_pack.reserve((size_t)(cells > 0 ? cells : 1) * 4));
    first.keep(c);
    if (cells > 0) {
        SidePackArgs a;
        a.src0 = t.src0->as<u32>(); a.src1 = t.src1 ? t.src1->as<u32>() : nullptr; a.dst = c->mg_pack.as<u32>();
        a.Qpad = Qpad; a.planes = t.planes; a.split = t.split; a.Gs = t.Gs; a.Gc = t.Gc;
        c->t_begin(KI_SIDE_PACK);
        hipLaunchKernelGGL(k_side_pack, dim3(grid_for(cells / 4)), dim3(256), 0, c->stream, a);
        c->t_end();
        HG_TRY(c->check_launch("k_side_pack"));
    }
    *dev_ptr = c->mg_pack.p;
    *nbytes = cells * 4;
    return c->stage_end();
}

// The Gsh gathered blocks of table `which` summed into the merged table of the whole database, with the two checks of
// hg_side_merge.hpp; the flag words are read before the call returns (it synchronises whatever "stage_sync" says).
int hg_merge_side_table(hg_ctx* c, int which, const void* dev_tabs_all, int Gsh, int Gc) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_merge_side_table", "hg_set_database + hg_set_queries"));
    if (which == HG_SIDE_REL) c->mrh.begin();
    else if (which == HG_SIDE_GRADE) c->mgh.begin();
    else if (which == HG_SIDE_JOINT) c->mjh.begin();
    SideTable t;
    HG_TRY(side_table(c, "hg_merge_side_table", which, which == HG_SIDE_JOINT ? Gc : 1, false, &t));
    if (!dev_tabs_all || ((uintptr_t)dev_tabs_all & 15)) return fail(HG_ERR_ARG, "hg_merge_side_table: dev_tabs_all must be a 16-byte aligned device address");
    if (Gsh < 1 || Gsh > 4096) return fail(HG_ERR_ARG, "hg_merge_side_table: %d shards (1..4096)", Gsh);
    const Geo g = full_geometry(c);
    const i64 cells = t.planes * g.Qpad;
    const FirstReservations first;
    HG_TRY(c->mg_flag.reserve(8));
    HG_TRY(t.dst->reserve((size_t)(cells > 0 ? cells : 1) * 4));
    first.keep(c);
    u32 flag[2] = {0u, 0xFFFFFFFFu};
    if (cells > 0) {
        HG_HIP(hipMemsetAsync(c->mg_flag.p, 0, 4, c->stream));
        HG_HIP(hipMemsetAsync(c->mg_flag.as<char>() + 4, 0xFF, 4, c->stream));
        SideMergeArgs a;
        a.tabs = (const u32*)dev_tabs_all; a.dst = t.dst->as<u32>(); a.flag = c->mg_flag.as<u32>();
        a.Q = g.Q; a.Qpad = g.Qpad; a.planes = t.planes; a.check_planes = t.check_planes; a.n_total = c->n_total; a.Gsh = Gsh;
        c->t_begin(KI_SIDE_MERGE);
        hipLaunchKernelGGL(k_side_merge, dim3((unsigned)g.nQT), dim3(SM_THREADS), 0, c->stream, a);
        c->t_end();
        HG_TRY(c->check_launch("k_side_merge"));
        HG_HIP(hipMemcpyAsync(flag, c->mg_flag.p, 8, hipMemcpyDeviceToHost, c->stream));
    }
    HG_TRY(c->sync());                                 // (the flag words decide the call)
    if (flag[0] & 1u)
        return fail(HG_ERR_STATE, "hg_merge_side_table: a cell of the merged %s table does not fit 32 bits (overflow flag; %d blocks)", t.name, Gsh);
    if (flag[0] & 2u)
        return fail(HG_ERR_STATE, "hg_merge_side_table: the merged %s table's column of query %u does not add up to n_total = %lld rows (column-total flag: "
                    "a shard's block is missing, counted twice or stale; %d blocks)", t.name, flag[1], (long long)c->n_total, Gsh);
    if (which == HG_SIDE_JOINT) c->mjh_G = t.Gc;
    t.merged->finish(c, g.Q, g.Qpad, t.dim);
    return HG_OK;
}

// This shard's part of the whole database's ranked lists as one block in the exchange layout (hg_list_merge.hpp): the grade plane
// u8 [Q][Rp] + u32 own[Qpad], or the vote table u32 [nk][C + 1][Qpad] at the cut-offs `host_ks`.  Needs the lists of the exact staged
// sequence -- global indices in global rank positions.  The block is the context's (lm_pack) and holds until the next pack.
int hg_pack_list_table(hg_ctx* c, int which, const int64_t* host_ks, int nk, void** dev_ptr, int64_t* nbytes) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_pack_list_table", "hg_set_database + hg_set_queries"));
    if (!dev_ptr || !nbytes) return fail(HG_ERR_ARG, "hg_pack_list_table: null pointer");
    HG_TRY(list_kind(c, "hg_pack_list_table", which));
    if (c->real_lists)
        return fail(HG_ERR_STATE, "hg_pack_list_table: the ranked lists are real-valued (hg_topr_real): that ranking splits the queries, every rank holds the whole table");
    if (c->ranked_local)
        return fail(HG_ERR_STATE, "hg_pack_list_table: the last ranking is in this shard's local rank order (hg_select_ranked): rank with hg_plan + hg_select (\"staged_lists\")");
    if (!(c->stage & ST_SELECT) || !c->lists_valid)
        return fail(HG_ERR_STATE, "hg_pack_list_table: no ranked lists in global rank positions on the device: rank with hg_plan + hg_select (\"staged_lists\") or hg_topr first");
    const ListGeo L = list_geometry(c);
    if (which == HG_LIST_VOTES) HG_TRY(check_cutoffs("hg_pack_list_table", "ks", host_ks, nk, VT_MAX_K, L.R, "R"));
    const size_t plane = (size_t)L.Q * L.Rp;
    const size_t bytes = which == HG_LIST_GRADES ? plane + (size_t)L.Qpad * 4 : (size_t)nk * (c->C + 1) * L.Qpad * 4;
    const FirstReservations first;
    HG_TRY(c->lm_pack.reserve(bytes));
    if (which == HG_LIST_VOTES) HG_TRY(c->lm_tab.reserve(VT_MAX_K * 8));
    first.keep(c);
    if (which == HG_LIST_GRADES) {
        HG_HIP(hipMemsetAsync(c->lm_pack.as<char>() + plane, 0, (size_t)L.Qpad * 4, c->stream));      // (own of the pad queries)
        ListGradesArgs a;
        a.idx = c->out_idx.as<u32>(); a.dblab = c->dblab.as<u64>(); a.qlab = c->qlab.as<u64>();
        a.plane = c->lm_pack.as<u8>(); a.own = (u32*)(c->lm_pack.as<char>() + plane);
        a.R = L.R; a.Rp = L.Rp; a.N = c->N; a.idx_base = c->idx_base; a.LW = c->LW;
        a.lastmask = lastmask(c->C);
        c->t_begin(KI_LIST_GRADES);
        if (L.Q > 0) hipLaunchKernelGGL(k_list_grades, dim3((unsigned)L.Q), dim3(LG_THREADS), 0, c->stream, a);
        c->t_end();
        HG_TRY(c->check_launch("k_list_grades"));
    } else {
        HG_TRY(put_cutoffs(c, host_ks, nk));
        HG_HIP(hipMemsetAsync(c->lm_pack.p, 0, bytes, c->stream));                                     // (the pad columns)
        VotesArgs a;
        a.idx = c->out_idx.as<u32>(); a.dblab = c->dblab.as<u64>(); a.ks = c->lm_tab.as<i64>();
        a.votes = c->lm_pack.as<u32>(); a.pred = nullptr; a.top = nullptr;
        a.R = L.R; a.N = c->N; a.nk = nk; a.LW = c->LW; a.C = c->C;
        a.lastmask = lastmask(c->C);
        a.idx_base = c->idx_base; a.Qpad = L.Qpad;
        c->t_begin(KI_VOTES);
        if (L.Q > 0) hipLaunchKernelGGL((k_votes<false, true>), dim3((unsigned)L.Q), dim3(VT_THREADS), 0, c->stream, a);
        c->t_end();
        HG_TRY(c->check_launch("k_votes"));
    }
    *dev_ptr = c->lm_pack.p;
    *nbytes = (int64_t)bytes;
    return c->stage_end();
}

// The Gsh gathered blocks of kind `which` merged into the grade plane / the vote counts of the whole database's lists, with the
// checks of hg_list_merge.hpp; the flag words are read before the call returns (it synchronises whatever "stage_sync" says).
int hg_merge_list_table(hg_ctx* c, int which, const void* dev_blocks_all, int Gsh, const int64_t* host_ks, int nk) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_merge_list_table", "hg_set_database + hg_set_queries"));
    if (which == HG_LIST_GRADES) c->mlg.begin();
    else if (which == HG_LIST_VOTES) c->mlv.begin();
    HG_TRY(list_kind(c, "hg_merge_list_table", which));
    if (!dev_blocks_all || ((uintptr_t)dev_blocks_all & 15)) return fail(HG_ERR_ARG, "hg_merge_list_table: dev_blocks_all must be a 16-byte aligned device address");
    if (Gsh < 1 || Gsh > 4096) return fail(HG_ERR_ARG, "hg_merge_list_table: %d shards (1..4096)", Gsh);
    if (!(c->stage & ST_SELECT) || c->ranked_local || c->real_lists)
        return fail(HG_ERR_STATE, "hg_merge_list_table: no ranking whose lists the blocks could belong to: rank with hg_plan + hg_select or hg_topr first");
    const ListGeo L = list_geometry(c);
    if (which == HG_LIST_VOTES) HG_TRY(check_cutoffs("hg_merge_list_table", "ks", host_ks, nk, VT_MAX_K, L.R, "R"));
    const bool grades = which == HG_LIST_GRADES;
    const size_t out_bytes = grades ? (size_t)L.Q * L.Rp : (size_t)L.Q * nk * c->C * 4;
    const FirstReservations first;
    HG_TRY(c->lm_flag.reserve(16));
    HG_TRY((grades ? c->lm_grades : c->lm_votes).reserve(out_bytes > 0 ? out_bytes : 1));
    if (!grades) HG_TRY(c->lm_tab.reserve(VT_MAX_K * 8));
    first.keep(c);
    u32 flag[4] = {0u, LIST_NO_QUERY, LIST_NO_QUERY, LIST_NO_QUERY};
    if (L.Q > 0) {
        HG_HIP(hipMemsetAsync(c->lm_flag.p, 0, 4, c->stream));
        HG_HIP(hipMemsetAsync(c->lm_flag.as<char>() + 4, 0xFF, 12, c->stream));
        if (grades) {
            ListMergeGradesArgs a;
            a.blocks = (const u8*)dev_blocks_all; a.dst = c->lm_grades.as<u8>(); a.flag = c->lm_flag.as<u32>();
            a.Q = L.Q; a.Qpad = L.Qpad; a.R = L.R; a.Rp = L.Rp; a.Gsh = Gsh; a.C = c->C;
            c->t_begin(KI_LIST_MERGE_GRADES);
            hipLaunchKernelGGL(k_list_merge_grades, dim3(grid_for(L.Q * (L.Rp >> 4) + L.Q)), dim3(256), 0, c->stream, a);
            c->t_end();
            HG_TRY(c->check_launch("k_list_merge_grades"));
        } else {
            HG_TRY(put_cutoffs(c, host_ks, nk));
            ListMergeVotesArgs a;
            a.tabs = (const u32*)dev_blocks_all; a.dst = c->lm_votes.as<u32>(); a.flag = c->lm_flag.as<u32>(); a.ks = c->lm_tab.as<i64>();
            a.Q = L.Q; a.Qpad = L.Qpad; a.nk = nk; a.C = c->C; a.Gsh = Gsh;
            c->t_begin(KI_LIST_MERGE_VOTES);
            hipLaunchKernelGGL(k_list_merge_votes, dim3((unsigned)(L.Qpad / 64)), dim3(SM_THREADS), 0, c->stream, a);
            c->t_end();
            HG_TRY(c->check_launch("k_list_merge_votes"));
        }
        HG_HIP(hipMemcpyAsync(flag, c->lm_flag.p, 16, hipMemcpyDeviceToHost, c->stream));
    }
    HG_TRY(c->sync());                                 // (the flag words decide the call)
    const char* const kind = grades ? "grade plane" : "vote table";
    if (grades) {
        if (flag[0] & 1u)
            return fail(HG_ERR_STATE, "hg_merge_list_table: the blocks' owned slots of query %u do not add up to R = %lld (owned-slots flag: a shard's block is missing, "
                        "counted twice, zeroed or stale; %d blocks)", flag[1], (long long)L.R, Gsh);
        if (flag[0] & 2u)
            return fail(HG_ERR_STATE, "hg_merge_list_table: a slot of query %u is non-zero in two blocks of the %s (slot-claimed-twice flag; %d blocks)", flag[2], kind, Gsh);
        if (flag[0] & 4u)
            return fail(HG_ERR_STATE, "hg_merge_list_table: a grade of query %u in the %s exceeds C = %d (grade-range flag; %d blocks)", flag[3], kind, c->C, Gsh);
        c->mlg.finish(c, L.Q, L.Rp, L.R);
    } else {
        if (flag[0] & 2u)
            return fail(HG_ERR_STATE, "hg_merge_list_table: the blocks' owned slots of query %u do not add up to a cut-off (owned-slots flag: a shard's block is missing, "
                        "counted twice, zeroed or stale; %d blocks)", flag[2], Gsh);
        if (flag[0] & 1u)
            return fail(HG_ERR_STATE, "hg_merge_list_table: a cell of query %u in the merged %s does not fit 32 bits (overflow flag; %d blocks)", flag[1], kind, Gsh);
        memcpy(c->mlv_ks, host_ks, (size_t)nk * 8);
        c->mlv.finish(c, L.Q, L.Q, nk);
    }
    return HG_OK;
}

// ---- getters: the copies on the context's stream, one synchronisation
int hg_get_rel_hist(hg_ctx* c, uint32_t* host_all, uint32_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_rel_hist", "hg_rel_hist"));
    if (!c->rh.current(c)) return fail(HG_ERR_STATE, "hg_get_rel_hist called before hg_rel_hist (on the tables loaded now)");
    if (host_all) HG_TRY(download_pitched(c, host_all, c->rh_all, c->rh.Q, c->rh.Qpad, c->rh.dim));
    if (host_rel) HG_TRY(download_pitched(c, host_rel, c->rh_rel, c->rh.Q, c->rh.Qpad, c->rh.dim));
    return c->sync();
}

int hg_get_graded(hg_ctx* c, int64_t* host_gsum, int64_t* host_hits, double* host_dcg, double* host_wsum) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_graded", "hg_graded"));
    if (!c->gr.current(c)) return fail(HG_ERR_STATE, "hg_get_graded called before hg_graded (on the ranked lists and tables held now)");
    void* const dst[4] = {host_gsum, host_hits, host_dcg, host_wsum};
    HG_TRY(download_planes(c, c->gr_out, (size_t)c->gr.Q * c->gr.dim * 8, dst, 4));
    return c->sync();
}

int hg_get_grades(hg_ctx* c, uint8_t* host_grades) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_grades", "hg_graded"));
    if (!c->gr.current(c) || !c->gr_kept)
        return fail(HG_ERR_STATE, "hg_get_grades: the last hg_graded on these lists did not keep the grade bytes (keep_grades = 0), or there was none");
    if (!host_grades) return fail(HG_ERR_ARG, "hg_get_grades: null pointer");
    HG_HIP(hipMemcpyAsync(host_grades, c->gr_grades.p, (size_t)c->gr.Q * c->gr_R, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_grade_hist(hg_ctx* c, uint32_t* host_hist) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_grade_hist", "hg_grade_hist"));
    if (!c->gh.current(c)) return fail(HG_ERR_STATE, "hg_get_grade_hist called before hg_grade_hist (on the tables loaded now)");
    if (!host_hist) return fail(HG_ERR_ARG, "hg_get_grade_hist: null pointer");
    HG_TRY(download_pitched(c, host_hist, c->gh_tab, c->gh.Q, c->gh.Qpad, c->gh.dim));
    return c->sync();
}

int hg_get_joint_hist(hg_ctx* c, uint32_t* host_hist) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_joint_hist", "hg_joint_hist"));
    if (!c->jh.current(c)) return fail(HG_ERR_STATE, "hg_get_joint_hist called before hg_joint_hist (on the tables loaded now)");
    if (!host_hist) return fail(HG_ERR_ARG, "hg_get_joint_hist: null pointer");
    HG_TRY(download_pitched(c, host_hist, c->jh_tab, c->jh.Q, c->jh.Qpad, c->jh.dim));
    return c->sync();
}

int hg_get_merged_rel_hist(hg_ctx* c, uint32_t* host_all, uint32_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_merged_rel_hist", "hg_merge_side_table"));
    if (!c->mrh.current(c)) return fail(HG_ERR_STATE, "hg_get_merged_rel_hist called before hg_merge_side_table of the rel table (on the tables loaded now)");
    const SideResult& m = c->mrh;
    if (host_all) HG_TRY(download_pitched(c, host_all, c->mg_rel, m.Q, m.Qpad, m.dim));
    if (host_rel)                                      // (the second half of the block)
        HG_HIP(hipMemcpy2DAsync(host_rel, (size_t)m.Q * 4, c->mg_rel.as<u32>() + m.dim * m.Qpad, (size_t)m.Qpad * 4, (size_t)m.Q * 4, (size_t)m.dim,
                                hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_merged_grade_hist(hg_ctx* c, uint32_t* host_hist) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_merged_grade_hist", "hg_merge_side_table"));
    if (!c->mgh.current(c)) return fail(HG_ERR_STATE, "hg_get_merged_grade_hist called before hg_merge_side_table of the grade table (on the tables loaded now)");
    if (!host_hist) return fail(HG_ERR_ARG, "hg_get_merged_grade_hist: null pointer");
    HG_TRY(download_pitched(c, host_hist, c->mg_grade, c->mgh.Q, c->mgh.Qpad, c->mgh.dim));
    return c->sync();
}

int hg_get_merged_joint_hist(hg_ctx* c, uint32_t* host_hist) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_merged_joint_hist", "hg_merge_side_table"));
    if (!c->mjh.current(c)) return fail(HG_ERR_STATE, "hg_get_merged_joint_hist called before hg_merge_side_table of the joint table (on the tables loaded now)");
    if (!host_hist) return fail(HG_ERR_ARG, "hg_get_merged_joint_hist: null pointer");
    HG_TRY(download_pitched(c, host_hist, c->mg_joint, c->mjh.Q, c->mjh.Qpad, c->mjh.dim));
    return c->sync();
}

int hg_get_tie_ap(hg_ctx* c, double* host_ap_exp, double* host_p_hit, double* host_ap_min, double* host_ap_max, double* host_rel_exp,
                  int64_t* host_rel_lo, int64_t* host_rel_hi) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_tie_ap", "hg_tie_ap"));
    if (!c->ta.current(c)) return fail(HG_ERR_STATE, "hg_get_tie_ap called before hg_tie_ap (on the tables loaded now)");
    void* const dst[7] = {host_ap_exp, host_p_hit, host_ap_min, host_ap_max, host_rel_exp, host_rel_lo, host_rel_hi};
    HG_TRY(download_planes(c, c->ta_out, (size_t)c->ta.Q * c->ta.dim * 8, dst, 7));
    return c->sync();
}

int hg_get_ap_at(hg_ctx* c, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_ap_at", "hg_ap_at"));
    if (!c->aa.current(c)) return fail(HG_ERR_STATE, "hg_get_ap_at called before hg_ap_at (on the match bitmap and tables held now)");
    const size_t n = (size_t)c->aa.Q * c->aa.dim;
    std::vector<u32> rel(host_rel ? n : 0);
    if (host_ap) HG_HIP(hipMemcpyAsync(host_ap, c->aa_out.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (host_rel) HG_HIP(hipMemcpyAsync(rel.data(), c->aa_out.as<char>() + n * 8, n * 4, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    widen_u32(host_rel, rel.data(), rel.size());
    return HG_OK;
}

int hg_get_vote_pred(hg_ctx* c, int32_t* host_pred, int64_t* host_top) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_vote_pred", "hg_votes"));
    if (!c->vt.current(c)) return fail(HG_ERR_STATE, "hg_get_vote_pred called before hg_votes (on the ranked lists and tables held now)");
    const size_t n = (size_t)c->vt.Q * c->vt.dim;
    std::vector<u32> top(host_top ? n : 0);
    if (host_pred) HG_HIP(hipMemcpyAsync(host_pred, c->vt_pred.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_top) HG_HIP(hipMemcpyAsync(top.data(), c->vt_pred.as<char>() + n * 4, n * 4, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    widen_u32(host_top, top.data(), top.size());
    return HG_OK;
}

int hg_get_vote_confusion(hg_ctx* c, int64_t* host_conf) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_vote_confusion", "hg_votes"));
    if (!c->vt.current(c)) return fail(HG_ERR_STATE, "hg_get_vote_confusion called before hg_votes (on the ranked lists and tables held now)");
    if (!host_conf) return fail(HG_ERR_ARG, "hg_get_vote_confusion: null pointer");
    HG_HIP(hipMemcpyAsync(host_conf, c->vt_conf.p, (size_t)c->vt.dim * c->C * c->C * 8, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_votes(hg_ctx* c, uint32_t* host_votes) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_votes", "hg_votes"));
    if (!c->vt.current(c)) return fail(HG_ERR_STATE, "hg_get_votes called before hg_votes (on the ranked lists and tables held now)");
    if (!host_votes) return fail(HG_ERR_ARG, "hg_get_votes: null pointer");
    HG_HIP(hipMemcpyAsync(host_votes, c->vt_votes.p, (size_t)c->vt.Q * c->vt.dim * c->C * 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_neighbours(hg_ctx* c, uint32_t* host_ids_sorted, uint32_t* host_count) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_neighbours", "hg_set_neighbours"));
    if (!c->nb.current(c)) return fail(HG_ERR_STATE, "hg_get_neighbours called before hg_set_neighbours / hg_neighbours_from_lists (on the tables loaded now)");
    if (host_ids_sorted) HG_HIP(hipMemcpyAsync(host_ids_sorted, c->nb_ids.p, (size_t)c->nb.Q * c->nb.dim * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_count) HG_HIP(hipMemcpyAsync(host_count, c->nb_cnt.p, (size_t)c->nb.Q * 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_nbr_hist(hg_ctx* c, uint32_t* host_nbr, uint32_t* host_count) {
    HG_TRY(need(c, ST_DB | ST_Q, "hg_get_nbr_hist", "hg_nbr_hist"));
    if (!c->nh.current(c) || !c->nb.current(c)) return fail(HG_ERR_STATE, "hg_get_nbr_hist called before hg_nbr_hist (on the neighbour sets and tables held now)");
    if (host_nbr) HG_TRY(download_pitched(c, host_nbr, c->nh_tab, c->nh.Q, c->nh.Qpad, c->nh.dim));
    if (host_count) HG_HIP(hipMemcpyAsync(host_count, c->nb_cnt.p, (size_t)c->nb.Q * 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

}  // extern "C"

int preload_side() {   // (hg_preload: see preload_seq)
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_tie_ap)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_nbr_sort)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_nbr_match)));
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_nbr_hist)));
    return HG_OK;
}

// libhashgan_amd.so -- context, options / statistics / timing, label match, AP and the downloads (see hg_ctx.hpp
// for the map of the translation units).
#include "hg_ctx.hpp"
#include "hg_dev_out.hpp"

#include <map>
#include <mutex>

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char* const kKernelNames[KI_COUNT] = {"k_hist", "k_hist_reduce", "k_plan", "k_seg_counts", "k_seg_layout", "k_guess",
                                            "k_select", "k_rank_hist", "k_order", "k_rank_fused", "k_match", "k_ap", "k_merge", "k_pack",
                                            "k_real_sample", "k_real_guess", "k_real_select", "k_radix_pass", "k_real_finish", "k_select_mx", "k_rank_cnt", "rccl_allgather", "step_gpu_span", "k_real_rescore",
                                            "k_hist_rel", "k_hist_rel_reduce", "k_graded", "k_grade_hist", "k_grade_hist_reduce", "k_tie_ap", "k_ap_at",
                                            "k_label_max", "k_hist_joint", "k_hist_joint_reduce",
                                            "k_rr_scan", "k_rr_collect", "k_rr_score", "k_rr_order", "k_export", "k_votes", "k_vote_confusion", "k_side_pack", "k_side_merge",
                                            "k_list_grades", "k_list_merge_grades", "k_list_merge_votes", "k_vote_pick", "k_asym_image16", "k_asym_rescore", "k_asym_expand_rows",
                                            "k_nbr_sort", "k_nbr_match", "k_nbr_hist", "k_pq_image16", "k_pq_rescore", "k_pq_expand_rows", "k_pq_encode"};
// Flatten NumPy's pairwise-summation tree for a chunk of n elements (n <= 8192):
// numpy/_core/src/umath/loops_utils.h.src, pairwise_sum: n <= 128 is a leaf,
// otherwise split at n/2 rounded down to a multiple of 8.
void build_shape(int n, ApShape& sh) {
    memset(&sh, 0, sizeof sh);
    sh.n = n;
    struct Rec {
        ApShape& s;
        void go(int off, int len) {
            if (len <= AP_LEAF) {
                s.leaf_start[s.n_leaves] = (unsigned short)off;
                s.leaf_len[s.n_leaves] = (unsigned short)len;
                s.prog[s.n_prog++] = (short)s.n_leaves++;
            } else {
                int n2 = len / 2;
                n2 -= n2 % 8;
                go(off, n2);
                go(off + n2, len - n2);
                s.prog[s.n_prog++] = -1;
            }
        }
    } rec{sh};
    if (n > 0) rec.go(0, n);
    // the same tree as a node table (k_ap evaluates it level by level): replay the postfix program on a stack of ids
    int stack[64], sp = 0, height[2 * AP_LEAF] = {0};
    for (int i = 0; i < sh.n_prog; ++i) {
        const int op = sh.prog[i];
        if (op >= 0) { stack[sp++] = op; continue; }
        const int r = stack[--sp], l = stack[--sp];
        const int k = sh.n_nodes++, id = sh.n_leaves + k;
        sh.nl[k] = (short)l;
        sh.nr[k] = (short)r;
        const int hgt = 1 + (height[l] > height[r] ? height[l] : height[r]);
        sh.nh[k] = (unsigned char)hgt;
        height[id] = hgt;
        if (hgt > sh.max_h) sh.max_h = hgt;
        stack[sp++] = id;
    }
}

std::atomic<unsigned long long> g_alloc_epoch{1};
const char* const kHostPhaseNames[HP_COUNT] = {"init", "devmalloc", "devfree", "hostmalloc", "hostfree", "destroy", "stream", "event", "sync", "pack", "thread"};
std::atomic<long long> g_host_ns[HP_COUNT], g_host_calls[HP_COUNT], g_host_max_ns[HP_COUNT];

// ---- the process-wide cache of device blocks, pinned blocks and streams (hg_ctx.hpp) ----------------------------------
namespace {
struct BlockCache {
    std::mutex m;
    std::multimap<std::pair<int, size_t>, void*> blocks;   // (device, bytes) -> block; pinned blocks: device -1
    size_t dev_bytes = 0, pin_bytes = 0;
    std::multimap<int, hipStream_t> streams;
    long long hits = 0, misses = 0;
    static size_t limit(const char* env, size_t dflt_mb) {
        const char* v = getenv(env);
        return (size_t)(v ? atoll(v) : (long long)dflt_mb) << 20;
    }
    void* take(int device, size_t want, size_t* got) {
        std::lock_guard<std::mutex> lk(m);
        static const bool trace = getenv("HG_CACHE_TRACE") != nullptr;
        auto it = blocks.lower_bound({device, want});
        if (it == blocks.end() || it->first.first != device || it->first.second > 2 * want + ((size_t)1 << 20)) {
            ++misses;
            if (trace) fprintf(stderr, "[hg cache] miss: %s block of %zu bytes (cached: %zu device, %zu pinned bytes in %zu blocks)\n",
                               device < 0 ? "pinned" : "device", want, dev_bytes, pin_bytes, blocks.size());
            return nullptr;
        }
        void* p = it->second;
        *got = it->first.second;
        (device < 0 ? pin_bytes : dev_bytes) -= *got;
        blocks.erase(it);
        ++hits;
        return p;
    }
    static void free_block(int device, void* p) {
        if (device < 0) { HostTimer t_(HP_HOSTFREE); (void)hipHostFree(p); }
        else { HostTimer t_(HP_DEVFREE); (void)hipFree(p); }
    }
    void give(int device, void* p, size_t bytes) {
        static const size_t dev_limit = limit("HG_CACHE_MB", 49152), pin_limit = limit("HG_PIN_CACHE_MB", 512);
        const size_t lim = device < 0 ? pin_limit : dev_limit;
        // (hipFree waits for the device; a cached block must be just as free of readers and writers before anybody else takes it)
        (void)hipDeviceSynchronize();
        if (bytes > lim) { free_block(device, p); return; }
        std::vector<std::pair<int, void*>> evict;
        {
            std::lock_guard<std::mutex> lk(m);
            blocks.insert({{device, bytes}, p});
            size_t& total = device < 0 ? pin_bytes : dev_bytes;
            total += bytes;
            while (total > lim) {                              // the largest block of this kind goes first
                auto hi = blocks.upper_bound({device, ~(size_t)0});
                if (hi == blocks.begin()) break;
                --hi;
                if ((hi->first.first < 0) != (device < 0)) break;
                total -= hi->first.second;
                evict.push_back({hi->first.first, hi->second});
                blocks.erase(hi);
            }
        }
        for (auto& e : evict) free_block(e.first, e.second);
    }
    void release_all() {
        std::vector<std::pair<int, void*>> all;
        std::vector<std::pair<int, hipStream_t>> st;
        {
            std::lock_guard<std::mutex> lk(m);
            for (auto& b : blocks) all.push_back({b.first.first, b.second});
            blocks.clear();
            dev_bytes = pin_bytes = 0;
            for (auto& x : streams) st.push_back({x.first, x.second});
            streams.clear();
        }
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (auto& b : all) { if (b.first >= 0) (void)hipSetDevice(b.first); free_block(b.first, b.second); }
        for (auto& x : st) { (void)hipSetDevice(x.first); (void)hipStreamDestroy(x.second); }
        (void)hipSetDevice(cur);
    }
};
BlockCache& cache() { static BlockCache* c = new BlockCache(); return *c; }      // (never destroyed: contexts may outlive static destructors)
}  // namespace

void* cache_take_dev(int device, size_t want, size_t* got) { return cache().take(device, want, got); }
void cache_give_dev(int device, void* p, size_t bytes) { cache().give(device, p, bytes); }
void* cache_take_pin(size_t want, size_t* got) { return cache().take(-1, want, got); }
void cache_give_pin(void* p, size_t bytes) { cache().give(-1, p, bytes); }
hipStream_t cache_take_stream(int device) {
    BlockCache& c = cache();
    std::lock_guard<std::mutex> lk(c.m);
    auto it = c.streams.find(device);
    if (it == c.streams.end()) return nullptr;
    hipStream_t s = it->second;
    c.streams.erase(it);
    return s;
}
void cache_give_stream(int device, hipStream_t s) {
    BlockCache& c = cache();
    {
        std::lock_guard<std::mutex> lk(c.m);
        if (c.streams.count(device) < 8) { c.streams.insert({device, s}); return; }
    }
    (void)hipStreamDestroy(s);
}
void cache_release_all() { cache().release_all(); }
static long long cache_stat(int which) {
    BlockCache& c = cache();
    std::lock_guard<std::mutex> lk(c.m);
    return which == 0 ? (long long)c.dev_bytes : which == 1 ? (long long)c.pin_bytes : which == 2 ? c.hits : which == 3 ? c.misses : (long long)c.streams.size();
}
int stream_create(int device, hipStream_t* out) {
    *out = cache_take_stream(device);
    if (*out) return HG_OK;
    HG_HIP(host_timed(HP_STREAM, [&] { return hipStreamCreateWithFlags(out, hipStreamNonBlocking); }));
    return HG_OK;
}

int need(hg_ctx* c, unsigned st, const char* who, const char* what) {
    if (!c) return fail(HG_ERR_ARG, "%s: null context", who);
    if ((c->stage & st) != st) return fail(HG_ERR_STATE, "%s called before %s", who, what);
    return c->use();
}

int launch_min_topr(hg_ctx* c, const u32* idx_all, const u8* dist_all, i64 n, int G) {
    c->t_begin(KI_MERGE);
    hipLaunchKernelGGL(k_min_topr, dim3(grid_for(n)), dim3(256), 0, c->stream, idx_all, dist_all, c->out_idx.as<u32>(), c->out_dist.as<u8>(), n, G);
    c->t_end();
    return c->check_launch("k_min_topr");
}

// The plan kernel flags R > (rows in the histograms it saw); read it back with the results.
int read_plan_flag(hg_ctx* c, int* flag) {
    HG_HIP(hipMemcpyAsync(flag, c->err.p, 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

// The verdict words, the APs and the hit counts of a one-shot call live side by side in one device block -- in the layout of the
// pinned staging block -- so that they come home in ONE copy (three blit kernels and their gaps cost a short step 10-15 us: C3 0.214
// -> 0.20 ms).  err, ap and rel become views; whoever reserves more than a view holds later simply gets a buffer of its own again.
int ensure_out_block(hg_ctx* c) {
    const size_t Q = (size_t)c->Q;
    char* base = (char*)c->outblk.p;
    if (base && c->outblk_q == (i64)Q && c->err.p == base && c->ap.p == base + 16 && c->rel.p == base + 16 + Q * 8) return HG_OK;
    HG_TRY(c->sync());                                 // (nothing may still be writing the old buffers)
    HG_TRY(c->outblk.reserve(16 + Q * 12 + 64));
    HG_HIP(hipMemsetAsync(c->outblk.p, 0, 16, c->stream));
    c->err.view(c->outblk, 0, 16);
    c->ap.view(c->outblk, 16, Q * 8);
    c->rel.view(c->outblk, 16 + Q * 8, Q * 4);
    c->outblk_q = (i64)Q;
    return HG_OK;
}

int ensure_pin(hg_ctx* c, size_t need_b) {
    if (c->pin_cap >= need_b) return HG_OK;
    HG_HIP(pin_grow(&c->pin, &c->pin_cap, need_b));
    ++g_alloc_epoch;                                   // captured downloads point into the old block
    return HG_OK;
}

// The child context that reruns a few lost queries exactly (rerun_lost_queries, real_requery_lost), created on first use on the
// parent's stream (ordered with its work).  It takes the parent's problem shape, database tables and options, with the call
// protocol of a plain synchronous call and no timing; each caller then applies its own overrides and loads the nF lost queries.
hg_ctx* requery_child(hg_ctx* c, i64 nF) {
    if (!c->sub) {
        c->sub = new hg_ctx();
        c->sub->is_sub = true;
        c->sub->device = c->device;
        c->sub->stream = c->stream;
    }
    hg_ctx* s = c->sub;
    s->N = c->N; s->b = c->b; s->C = c->C; s->n_total = c->n_total; s->NW = c->NW; s->NB = c->NB; s->LW = c->LW;
    s->idx_base = c->idx_base; s->n_cu = c->n_cu; s->bpad = c->bpad;
    s->opt = c->opt;
    s->opt.stage_sync = 1; s->opt.defer_verdict = 0; s->opt.step_graph = 0; s->opt.step_streams = 2; s->opt.timing_every = 1;
    s->timing = 0;
    s->db.borrow(c->db);
    s->dblab.borrow(c->dblab);
    s->Q = nF;
    return s;
}

// What the context and its requery child hold on the device (stat "device_bytes"; borrowed buffers and views are another's).
static i64 device_bytes(hg_ctx* c) {
    i64 total = 0;
    c->for_each_buf([&](DevBuf& d, BufClass) { if (!d.borrowed) total += (i64)d.cap; });
    return total + (c->sub ? device_bytes(c->sub) : 0);
}

// =============================================================================
extern "C" {

const char* hg_last_error(void) { return g_err.c_str(); }
int hg_version(void) { return 100; }

int hg_device_count(int* count) {
    if (!count) return fail(HG_ERR_ARG, "hg_device_count: null pointer");
    HG_HIP(hipGetDeviceCount(count));
    return HG_OK;
}

int hg_init(int device, hg_ctx** out) {
    if (!out) return fail(HG_ERR_ARG, "hg_init: null pointer");
    *out = nullptr;
    HostTimer t_init(HP_INIT);
    int n = 0;
    HG_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(HG_ERR_ARG, "hg_init: device %d out of range (%d visible)", device, n);
    HG_HIP(hipSetDevice(device));
    // A step is a few milliseconds and ends in one stream synchronisation: spin instead of sleeping on it.
    // (Refused when the device is already initialised, e.g. by torch -- harmless.)
    if (hipSetDeviceFlags(hipDeviceScheduleSpin) != hipSuccess) (void)hipGetLastError();
    hg_ctx* c = new hg_ctx();
    c->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->n_cu = cus;
    const int rc_s = stream_create(device, &c->stream);
    if (rc_s != HG_OK) { delete c; return rc_s; }
    *out = c;
    return HG_OK;
}

int hg_destroy(hg_ctx* c) {
    if (!c) return HG_OK;
    HostTimer t_destroy(HP_DESTROY);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream_b) (void)hipStreamSynchronize(c->stream_b);
    c->t_collect();
    c->drop_graph();
    for (auto e : c->pool) (void)hipEventDestroy(e);
    c->for_each_buf([](DevBuf& d, BufClass) { d.release(); });
    comm_release(c);
    if (c->sub) { hg_ctx* s = c->sub; c->sub = nullptr; (void)hg_destroy(s); }
    pin_free(c->pin, c->pin_cap);
    for (auto& m : c->mslot) { pin_free(m.pin, m.cap); if (m.ev) (void)hipEventDestroy(m.ev); m.pin = nullptr; m.ev = nullptr; }
    pin_free(c->hpk, c->hpk_cap);
    pin_free(c->fstage, c->fstage_cap);
    for (auto& q : c->qstage) { pin_free(q.pin, q.cap); if (q.ev) (void)hipEventDestroy(q.ev); q.pin = nullptr; q.ev = nullptr; }
    if (c->stream2_ev) (void)hipEventDestroy(c->stream2_ev);
    if (c->stream2) { (void)hipStreamSynchronize(c->stream2); cache_give_stream(c->device, c->stream2); }
    for (auto& e : c->fstage_ev) if (e) (void)hipEventDestroy(e);
    if (c->ev_pre) (void)hipEventDestroy(c->ev_pre);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->stream_b) cache_give_stream(c->device, c->stream_b);                              // (synchronised above)
    if (c->stream && c->own_stream && !c->is_sub) cache_give_stream(c->device, c->stream);   // (synchronised above)
    delete c;
    return HG_OK;
}

// ---- results into DEVICE memory (hg_dev_out.hpp: the kernel; hg_dev_desc.hpp: the descriptor arithmetic) ----
namespace {
struct ExportPlan { int cls; const void* src; i64 pitch, Q, R; int64_t bytes; };
}
// Where an item's values lie, by its host getter's rules: class, base, row pitch (in source elements), queries and list length.
// HG_ERR_STATE, naming the call that would provide them, when the context does not hold them.
static int export_source(hg_ctx* c, int what, ExportPlan* p) {
    const bool ranked = (c->stage & ST_SELECT) != 0;
    p->Q = c->geo.Q; p->R = c->geo.R; p->pitch = c->geo.R;
    switch (what) {
        case HG_OUT_IDX:
            if (!ranked || !(c->lists_valid || c->real_lists))
                return fail(HG_ERR_STATE, "hg_export: IDX needs ranked lists, and the last call materialised none (hg_map skips them): call hg_topr, hg_topr_real or hg_topr_rerank");
            p->cls = XC_U32; p->src = c->out_idx.p;
            return HG_OK;
        case HG_OUT_DIST:
            // (real_lists: out_idx is a real-valued ranking's, which writes no distances -- out_dist would be an earlier ranking's)
            if (!ranked || !c->lists_valid || c->real_lists)
                return fail(HG_ERR_STATE, "hg_export: DIST needs the lists of a Hamming ranking: call hg_topr or hg_topr_rerank (hg_map and the real-valued rankings leave no distances)");
            p->cls = XC_U8; p->src = c->out_dist.p;
            return HG_OK;
        case HG_OUT_SCORE:
            p->cls = XC_U32;
            if (ranked && c->rr.current(c)) { p->src = c->rr_scores.p; p->Q = c->rr.Q; p->R = p->pitch = c->rr.dim; return HG_OK; }
            if (ranked && c->real_lists) { p->src = c->scores.p; return HG_OK; }
            return fail(HG_ERR_STATE, "hg_export: SCORE needs the score list of a real-valued ranking or a re-rank: call hg_topr_real or hg_topr_rerank");
        case HG_OUT_MATCH:
            if (!(c->stage & ST_MATCH)) return fail(HG_ERR_STATE, "hg_export: MATCH called before hg_match (or a ranking that leaves the match bitmap)");
            if (c->ranked_local) return fail(HG_ERR_STATE, "hg_export: the match bitmap is in this shard's local rank order (hg_select_ranked): merge it first");
            if (c->G > 1 && !c->mbits_merged)
                return fail(HG_ERR_STATE, "hg_export: the match bitmap holds this shard's rows only (%d shards): merge it first (hg_merge_match, hg_merge_ranked)", c->G);
            if (c->mbits_in_ws_b) return fail(HG_ERR_STATE, "hg_export: the last ranking was a step of hg_map_begin in its own workspace: rank with hg_topr / hg_map first");
            p->cls = XC_BIT; p->src = c->mbits.p; p->pitch = c->RW;
            return HG_OK;
        case HG_OUT_AP: case HG_OUT_HITS:
            if (!(c->stage & ST_AP)) return fail(HG_ERR_STATE, "hg_export: %s called before hg_ap", hg_dev::out_name(what));
            p->cls = what == HG_OUT_AP ? XC_F64 : XC_U32;
            p->src = what == HG_OUT_AP ? c->ap.p : c->rel.p;
            p->R = p->pitch = 1;
            return HG_OK;
        case HG_OUT_GRADES:
            if ((c->stage & (ST_DB | ST_Q)) != (ST_DB | ST_Q) || !c->gr.current(c) || !c->gr_kept)
                return fail(HG_ERR_STATE, "hg_export: GRADES needs the grade bytes of these lists: call hg_graded with keep_grades = 1");
            p->cls = XC_U8; p->src = c->gr_grades.p; p->Q = c->gr.Q; p->R = p->pitch = c->gr_R;
            return HG_OK;
        default: return fail(HG_ERR_ARG, "hg_export: unknown item %d", what);
    }
}

int hg_export(hg_ctx* c, const hg_export_item* items, int n) {
    if (!c) return fail(HG_ERR_ARG, "hg_export: null context");
    if (!items || n < 1 || n > 8) return fail(HG_ERR_ARG, "hg_export: 1..8 items (have %d)", n);
    // results that may still be withdrawn are not handed to another stream
    if (c->ms_n) return fail(HG_ERR_STATE, "hg_export: a step of hg_map_begin is in flight: take it with hg_map_end first");
    if (c->verdict_pending) return fail(HG_ERR_STATE, "hg_export: the bet's verdict is pending (defer_verdict): ask hg_bet_verdict first");
    // every item is judged before anything is enqueued
    ExportPlan plan[8];
    for (int i = 0; i < n; ++i) HG_TRY(export_source(c, items[i].what, &plan[i]));
    HG_TRY(c->use());
    for (int i = 0; i < n; ++i) {
        const hg_dev_array& d = items[i].dst;
        char msg[256];
        if (hg_dev::check_out_item(items[i], plan[i].Q, plan[i].R, c->n_total, &plan[i].bytes, msg, sizeof msg))
            return fail(HG_ERR_ARG, "hg_export: item %d: %s", i, msg);
        HG_TRY(check_dev_pointer(c, "hg_export", hg_dev::out_name(items[i].what), d, plan[i].bytes));
        for (const DevBuf* s : {&c->out_idx, &c->out_dist, &c->scores, &c->rr_scores, &c->mbits, &c->ap, &c->rel, &c->gr_grades})
            if (s->p && hg_dev::ranges_intersect(d.ptr, plan[i].bytes, s->p, (int64_t)s->cap))
                return fail(HG_ERR_ARG, "hg_export: item %d: the destination lies inside a result buffer of this context", i);
        for (int j = 0; j < i; ++j)
            if (hg_dev::ranges_intersect(d.ptr, plan[i].bytes, items[j].dst.ptr, plan[j].bytes))
                return fail(HG_ERR_ARG, "hg_export: the destinations of items %d and %d intersect", j, i);
    }
    // the consumers' streams, each once
    void* consumers[8];
    int nc = 0;
    for (int i = 0; i < n; ++i) {
        void* s = items[i].dst.stream;
        bool seen = (hipStream_t)s == c->stream;
        for (int j = 0; j < nc; ++j) seen = seen || consumers[j] == s;
        if (!seen) consumers[nc++] = s;
    }
    for (int j = 0; j < nc; ++j) HG_TRY(wait_for_producer(c, consumers[j]));       // earlier readers and writers of the destinations finish first
    c->export_bytes = 0; c->export_variant = 0;
    for (int i = 0; i < n; ++i) {
        bool vec = false;
        HG_TRY(launch_export(c, plan[i].cls, plan[i].src, plan[i].pitch, items[i].dst, &vec));
        c->export_variant |= vec ? 1 : 2;
        c->export_bytes += items[i].dst.rows * items[i].dst.cols * hg_dev::itemsize(items[i].dst.dtype);
    }
    if (nc) {                                          // whatever the consumers enqueue from here on sees the data
        hipEvent_t ev = c->get_event();
        if (!ev) return fail(HG_ERR_HIP, "hipEventCreate failed");
        hipError_t e = hipEventRecord(ev, c->stream);
        for (int j = 0; j < nc && e == hipSuccess; ++j) e = hipStreamWaitEvent((hipStream_t)consumers[j], ev, 0);
        c->pool.push_back(ev);                         // (the waits are enqueued: the event may be recorded again)
        HG_HIP(e);
    }
    return c->stage_end();
}

extern "C++" int do_match(hg_ctx* c) {
    const Geo& g = c->geo;
    const i64 nKB = (g.R + 255) / 256;
    const i64 blocks = nKB * g.Q;
    if (blocks > 0x7FFFFFFFll) return fail(HG_ERR_ARG, "hg_match: Q*R too large for one launch");
    c->t_begin(KI_MATCH);
    hipLaunchKernelGGL(k_match, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->out_idx.as<u32>(),
                       c->dblab.as<u64>(), c->qlab.as<u64>(), c->mbits.as<u64>(), c->RW, (int)nKB, g);
    c->t_end();
    HG_TRY(c->check_launch("k_match"));
    c->stage |= ST_MATCH;
    c->stage &= ~(unsigned)ST_AP;
    c->bitmap_changed();
    return HG_OK;
}

// Label-match bits are produced together with the ranking (k_select/k_order) for
// up to 128 classes; this stage exists for wider label sets and for API symmetry.
int hg_match(hg_ctx* c) {
    HG_TRY(need(c, ST_SELECT, "hg_match", "hg_select"));
    if (c->stage & ST_MATCH) return HG_OK;
    HG_TRY(do_match(c));
    return c->stage_end();
}

int hg_match_buffer(hg_ctx* c, void** dev_ptr, int64_t* nbytes) {
    HG_TRY(need(c, ST_MATCH, "hg_match_buffer", "hg_match"));
    if (dev_ptr) *dev_ptr = c->mbits.p;
    if (nbytes) *nbytes = (int64_t)c->geo.Q * c->RW * 8;
    return HG_OK;
}

int hg_merge_match(hg_ctx* c, const uint64_t* dev_bits_all, int G) {
    HG_TRY(need(c, ST_MATCH, "hg_merge_match", "hg_match"));
    if (!dev_bits_all || G < 1) return fail(HG_ERR_ARG, "hg_merge_match: bad argument");
    const i64 n = (i64)c->geo.Q * c->RW;
    c->t_begin(KI_MERGE);
    hipLaunchKernelGGL(k_or_bits, dim3(grid_for(n)), dim3(256), 0, c->stream, (const u64*)dev_bits_all, c->mbits.as<u64>(), n, G);
    c->t_end();
    HG_TRY(c->check_launch("k_or_bits"));
    c->bitmap_changed();                               // (hg_ap_at's tables were the unmerged bitmap's)
    c->mbits_merged = true;
    return c->stage_end();
}

// k_ap's tables for the current R: the flattened summation trees and the reciprocals of the ranks (also read by
// k_rank_cnt's AP epilogue); *use_recip: lists beyond 2^20 divide
extern "C++" int ensure_ap_tables(hg_ctx* c, bool* use_recip_out) {
    const Geo& g = c->geo;
    if (c->shapes_for_R != g.R) {
        std::vector<ApShape> sh(2);
        build_shape(g.R >= AP_CHUNK ? AP_CHUNK : (int)g.R, sh[0]);
        build_shape((int)(g.R % AP_CHUNK), sh[1]);
        HG_TRY(c->shapes.reserve(sizeof(ApShape) * 2));
        HG_HIP(hipMemcpyAsync(c->shapes.p, sh.data(), sizeof(ApShape) * 2, hipMemcpyHostToDevice, c->stream));
        HG_HIP(hipStreamSynchronize(c->stream));   // sh goes out of scope
        c->shapes_for_R = g.R;
    }
    // reciprocals of the ranks 1 .. R (k_ap's division in three multiply-adds); lists beyond 2^20 divide
    const bool use_recip = c->opt.ap_recip && g.R <= (1ll << 20);
    if (use_recip && c->recip_for_R != g.R) {
        // (AP_RECIP_SLACK more: ap_eval2's masked slots past the last rank still load a -- finite -- entry)
        HG_TRY(c->ap_recip.reserve((size_t)(g.R + 1 + AP_RECIP_SLACK) * 8));
        hipLaunchKernelGGL(k_recip_table, dim3(grid_for(g.R + 1 + AP_RECIP_SLACK)), dim3(256), 0, c->stream, c->ap_recip.as<double>(), (i64)g.R + AP_RECIP_SLACK);
        HG_TRY(c->check_launch("k_recip_table"));
        c->recip_for_R = g.R;
    }
    HG_TRY(c->ap.reserve((size_t)g.Q * 8));
    HG_TRY(c->rel.reserve((size_t)g.Q * 4));
    *use_recip_out = use_recip;
    return HG_OK;
}

// only: optional device flags [Q] -- evaluate just the flagged queries
extern "C++" int do_ap_range(hg_ctx* c, i64 q0, i64 nq, const u32* only) {      // k_ap's block index is the query: a range is a pointer offset
    c->ap_staged = false;
    const Geo& g = c->geo;
    bool use_recip = false;
    HG_TRY(ensure_ap_tables(c, &use_recip));
    c->t_begin(KI_AP);
    // few queries with long lists: four times the threads per query (see k_ap)
    const bool wide = nq * 2 < (i64)c->n_cu * 8 && g.R > 2 * AP_CHUNK && c->opt.ap_wide;
    if (nq > 0 && wide)
        hipLaunchKernelGGL(k_ap<512>, dim3((unsigned)nq), dim3(512), 0, c->stream, c->mbits.as<u64>() + (size_t)q0 * c->RW, c->RW, g.R,
                           c->shapes.as<ApShape>(), use_recip ? c->ap_recip.as<double>() : (const double*)nullptr,
                           c->ap.as<double>() + q0, c->rel.as<u32>() + q0, only ? only + q0 : (const u32*)nullptr);
    else if (nq > 0)
        hipLaunchKernelGGL(k_ap<AP_THREADS>, dim3((unsigned)nq), dim3(AP_THREADS), 0, c->stream, c->mbits.as<u64>() + (size_t)q0 * c->RW, c->RW, g.R,
                           c->shapes.as<ApShape>(), use_recip ? c->ap_recip.as<double>() : (const double*)nullptr,
                           c->ap.as<double>() + q0, c->rel.as<u32>() + q0, only ? only + q0 : (const u32*)nullptr);
    c->t_end();
    HG_TRY(c->check_launch("k_ap"));
    c->stage |= ST_AP;
    return HG_OK;
}

int hg_ap(hg_ctx* c) {
    HG_TRY(need(c, ST_MATCH, "hg_ap", "hg_match"));
    HG_TRY(do_ap(c));
    return c->stage_end();
}

int hg_topr_buffers(hg_ctx* c, void** dev_idx, void** dev_dist, int64_t* n_slots) {
    HG_TRY(need(c, ST_SELECT, "hg_topr_buffers", "hg_select"));
    if (!c->lists_valid) return fail(HG_ERR_STATE, "ranked lists were not materialised by the last call (use hg_topr / staged_lists)");
    if (dev_idx) *dev_idx = c->out_idx.p;
    if (dev_dist) *dev_dist = c->out_dist.p;
    if (n_slots) *n_slots = (int64_t)c->geo.Q * c->geo.R;
    return HG_OK;
}

int hg_merge_topr(hg_ctx* c, const uint32_t* dev_idx_all, const uint8_t* dev_dist_all, int G) {
    HG_TRY(need(c, ST_SELECT, "hg_merge_topr", "hg_select"));
    if (!c->lists_valid) return fail(HG_ERR_STATE, "ranked lists were not materialised by the last call");
    if (!dev_idx_all || !dev_dist_all || G < 1) return fail(HG_ERR_ARG, "hg_merge_topr: bad argument");
    const i64 n = (i64)c->geo.Q * c->geo.R;
    c->t_begin(KI_MERGE);
    hipLaunchKernelGGL(k_min_topr, dim3(grid_for(n)), dim3(256), 0, c->stream, (const u32*)dev_idx_all,
                       (const u8*)dev_dist_all, c->out_idx.as<u32>(), c->out_dist.as<u8>(), n, G);
    c->t_end();
    HG_TRY(c->check_launch("k_min_topr"));
    c->lists_changed();
    return c->stage_end();
}

int hg_get_topr_real(hg_ctx* c, uint32_t* host_idx, float* host_scores) {
    HG_TRY(need(c, ST_SELECT, "hg_get_topr_real", "hg_topr_real / hg_map_real"));
    if (!c->real_lists) return fail(HG_ERR_STATE, "hg_get_topr_real: no real-valued ranked lists (the last ranking was not real-valued, or it was an hg_map_real, "
                                                  "which skips them: use hg_topr_real, or option real_map_lists = 1)");
    const size_t slots = (size_t)c->geo.Q * c->geo.R;
    if (host_idx) HG_HIP(hipMemcpyAsync(host_idx, c->out_idx.p, slots * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_scores) HG_HIP(hipMemcpyAsync(host_scores, c->scores.p, slots * 4, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_topr(hg_ctx* c, uint32_t* host_idx, uint8_t* host_dist) {
    HG_TRY(need(c, ST_SELECT, "hg_get_topr", "hg_select"));
    if (!c->lists_valid) return fail(HG_ERR_STATE, "ranked lists were not materialised by the last call (hg_map skips them; use hg_topr)");
    const size_t slots = (size_t)c->geo.Q * c->geo.R;
    if (host_idx) HG_HIP(hipMemcpyAsync(host_idx, c->out_idx.p, slots * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_dist) HG_HIP(hipMemcpyAsync(host_dist, c->out_dist.p, slots, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_get_match(hg_ctx* c, uint8_t* host_imatch) {
    HG_TRY(need(c, ST_MATCH, "hg_get_match", "hg_match"));
    if (!host_imatch) return fail(HG_ERR_ARG, "hg_get_match: null pointer");
    const i64 Q = c->geo.Q, R = c->geo.R, RW = c->RW;
    std::vector<u64> bits((size_t)Q * RW);
    HG_HIP(hipMemcpyAsync(bits.data(), c->mbits.p, bits.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HG_TRY(c->sync());
    for (i64 q = 0; q < Q; ++q)
        for (i64 k = 0; k < R; ++k) host_imatch[q * R + k] = (u8)((bits[q * RW + (k >> 6)] >> (k & 63)) & 1ull);
    return HG_OK;
}

int hg_get_ap(hg_ctx* c, double* host_ap, int64_t* host_rel) {
    HG_TRY(need(c, ST_AP, "hg_get_ap", "hg_ap"));
    const i64 Q = c->geo.Q;
    if (!(c->ap_staged && c->pin)) {                   // (else the one-shot call already brought them over)
        // one batch of copies into pinned memory, one synchronisation; a deferred verdict rides along
        HG_TRY(ensure_pin(c, (size_t)Q * 12 + 16));
        char* pb = (char*)c->pin;
        if (c->verdict_pending) HG_HIP(hipMemcpyAsync(pb, c->err.p, 4, hipMemcpyDeviceToHost, c->stream));
        if (host_ap) HG_HIP(hipMemcpyAsync(pb + 16, c->ap.p, (size_t)Q * 8, hipMemcpyDeviceToHost, c->stream));
        if (host_rel) HG_HIP(hipMemcpyAsync(pb + 16 + (size_t)Q * 8, c->rel.p, (size_t)Q * 4, hipMemcpyDeviceToHost, c->stream));
        HG_TRY(c->sync());
        if (c->verdict_pending) { c->verdict_flag = *(const int*)pb; c->verdict_known = true; }
    }
    const char* pb = (const char*)c->pin;
    if (host_ap) memcpy(host_ap, pb + 16, (size_t)Q * 8);
    if (host_rel) widen_u32(host_rel, pb + 16 + (size_t)Q * 8, (size_t)Q);
    return HG_OK;
}

int hg_get_hist(hg_ctx* c, uint32_t* host_hist) {
    HG_TRY(need(c, ST_HIST, "hg_get_hist", "hg_hist"));
    if (!host_hist) return fail(HG_ERR_ARG, "hg_get_hist: null pointer");
    const Geo& g = c->geo;
    HG_TRY(download_pitched(c, host_hist, c->hown, g.Q, g.Qpad, g.NB));
    return c->sync();
}

// Context-owned device scratch (grows only) and a stream-ordered device-to-device copy: what an in-process
// communicator (virtual shards of one GPU in the tests) needs to do hg_allgather's job without RCCL.
int hg_scratch(hg_ctx* c, int slot, int64_t nbytes, void** dev_ptr) {
    if (!c || !dev_ptr || nbytes < 1 || slot < 0 || slot >= 4) return fail(HG_ERR_ARG, "hg_scratch: bad argument");
    HG_TRY(c->use());
    HG_TRY(c->scratch[slot].reserve((size_t)nbytes));
    *dev_ptr = c->scratch[slot].p;
    return HG_OK;
}

int hg_memcpy_dtod(hg_ctx* c, void* dev_dst, const void* dev_src, int64_t nbytes) {
    if (!c || !dev_dst || !dev_src || nbytes < 0) return fail(HG_ERR_ARG, "hg_memcpy_dtod: bad argument");
    HG_TRY(c->use());
    if (nbytes) HG_HIP(hipMemcpyAsync(dev_dst, dev_src, (size_t)nbytes, hipMemcpyDeviceToDevice, c->stream));
    return c->stage_end();
}

// device <-> host copies of raw device addresses, complete on return (a stand-in communicator that goes through the
// host -- tests/file_comm.py, for multi-process dry runs on one GPU -- is their only user)
int hg_memcpy_dtoh(hg_ctx* c, void* host_dst, const void* dev_src, int64_t nbytes) {
    if (!c || !host_dst || !dev_src || nbytes < 0) return fail(HG_ERR_ARG, "hg_memcpy_dtoh: bad argument");
    HG_TRY(c->use());
    if (nbytes) HG_HIP(hipMemcpyAsync(host_dst, dev_src, (size_t)nbytes, hipMemcpyDeviceToHost, c->stream));
    return c->sync();
}

int hg_memcpy_htod(hg_ctx* c, void* dev_dst, const void* host_src, int64_t nbytes) {
    if (!c || !dev_dst || !host_src || nbytes < 0) return fail(HG_ERR_ARG, "hg_memcpy_htod: bad argument");
    HG_TRY(c->use());
    if (nbytes) HG_HIP(hipMemcpyAsync(dev_dst, host_src, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    return c->sync();
}

int hg_synchronize(hg_ctx* c) {
    if (!c) return fail(HG_ERR_ARG, "hg_synchronize: null context");
    HG_TRY(c->use());
    return c->sync();
}

int hg_set_stream(hg_ctx* c, void* stream) {
    if (!c) return fail(HG_ERR_ARG, "hg_set_stream: null context");
    HG_TRY(c->use());
    HG_TRY(c->sync());                               // drain the old stream first
    c->drop_graph();
    c->cfg_epoch++;
    if (c->stream && c->own_stream) cache_give_stream(c->device, c->stream);
    if (stream) {
        c->stream = (hipStream_t)stream;
        c->own_stream = false;
    } else {
        HG_TRY(stream_create(c->device, &c->stream));
        c->own_stream = true;
    }
    if (c->sub) c->sub->stream = c->stream;
    return HG_OK;
}

// Every configuration key but the three hg_set_option handles first: the Options field it sets and the values it takes -- a flag
// takes any value (nonzero = 1), a ranged key lo .. hi (else the text), select_packed any value as it is.
namespace {
struct OptionKey { const char* key; i64 Options::*field; bool flag; i64 lo, hi; const char* range; };
constexpr i64 kMax = INT64_MAX;
constexpr OptionKey flag(const char* k, i64 Options::*f) { return {k, f, true, 0, 1, nullptr}; }
constexpr OptionKey ranged(const char* k, i64 Options::*f, i64 lo, i64 hi, const char* range) { return {k, f, false, lo, hi, range}; }
const OptionKey kOptionKeys[] = {
    ranged("target_units", &Options::target_units, 1, kMax, "target_units must be >= 1"),
    ranged("min_segment", &Options::min_segment, 16, kMax, "min_segment must be >= 16"),
    ranged("max_segments", &Options::max_segments, 1, kMax, "max_segments must be >= 1"),
    ranged("sample_stride", &Options::sample_stride, 0, 1024, "sample_stride must be 0 (auto) .. 1024"),
    ranged("guess_sigma", &Options::guess_sigma, 0, 64, "guess_sigma must be 0..64"),
    ranged("cand_budget_x10", &Options::cand_budget_x10, 11, 1000, "cand_budget_x10 must be 11..1000"),
    flag("second_bet", &Options::second_bet),
    flag("crowd_probe", &Options::crowd_probe),
    flag("select_mfma", &Options::select_mfma),
    ranged("select_packed", &Options::select_packed, INT64_MIN, kMax, nullptr),
    flag("compact_records", &Options::compact_records),
    ranged("hist_mfma", &Options::hist_mfma, 0, 2, "hist_mfma must be 0, 1 or 2"),
    ranged("rank_lds", &Options::rank_lds, 0, 2, "rank_lds must be 0, 1 or 2"),
    ranged("rank_slices", &Options::rank_slices, 0, kMax, "rank_slices must be >= 0 (the smallest R it takes; 0: off)"),
    ranged("rank_dense", &Options::rank_dense, 0, 2, "rank_dense must be 0 or 1 (2 is accepted and means 1)"),
    ranged("rank_dense_gbm", &Options::rank_dense_gbm, -1, 1, "rank_dense_gbm must be -1, 0 or 1"),
    ranged("dense_budget_mb", &Options::dense_budget_mb, 1, kMax, "dense_budget_mb must be >= 1"),
    flag("all_rows_shortcut", &Options::all_rows_shortcut),
    flag("fuse_ap", &Options::fuse_ap),
    flag("inline_leftovers", &Options::inline_leftovers),
    flag("ap_wide", &Options::ap_wide),
    flag("ap_recip", &Options::ap_recip),
#if HG_PROBES
    ranged("probe_select", &Options::probe_select, INT64_MIN, kMax, nullptr),   // (libhashgan_amd_probe.so only: python -m hashgan_amd.build --probes)
    ranged("probe_votes", &Options::probe_votes, 0, 1, "probe_votes must be 0 or 1"),
#endif
    flag("stage_sync", &Options::stage_sync),
    flag("defer_verdict", &Options::defer_verdict),
    flag("staged_lists", &Options::staged_lists),
    flag("step_graph", &Options::step_graph),
    ranged("step_streams", &Options::step_streams, 1, 2, "step_streams must be 1 or 2"),
    ranged("timing_every", &Options::timing_every, 1, 1024, "timing_every must be 1..1024"),
    flag("host_pack", &Options::host_pack),
    ranged("keep_floats", &Options::keep_floats, 0, 2, "keep_floats must be 0, 1 or 2"),
    ranged("pq_encode_chunk_rows", &Options::pq_encode_chunk_rows, 0, 0x7FFFFFFF, "pq_encode_chunk_rows must be 0 (the default) .. 2^31 - 1"),
    ranged("keep_query_floats", &Options::keep_query_floats, 0, 1, "keep_query_floats must be 0 or 1"),
    ranged("real_mfma", &Options::real_mfma, 0, 2, "real_mfma must be 0, 1 or 2"),
    flag("real_sample_half", &Options::real_sample_half),
    flag("real_second_sample", &Options::real_second_sample),
    flag("real_sort_lds", &Options::real_sort_lds),
    flag("real_groups", &Options::real_groups),
    flag("real_map_lists", &Options::real_map_lists),
    ranged("real_whole_rounds", &Options::real_whole_rounds, 0, 8, "real_whole_rounds must be 0 .. 8"),
};
}  // namespace

int hg_set_option(hg_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return fail(HG_ERR_ARG, "hg_set_option: null argument");
    if (!strcmp(key, "handicap_next_bet")) {           // test hook: not a configuration change (a blind hg_map_begin stays blind -- and loses)
        if (value < 0 || value > 64) return fail(HG_ERR_ARG, "handicap_next_bet must be 0..64");
        c->handicap_next = value;
        return HG_OK;
    }
    if (!strcmp(key, "real_far_cursors")) {            // test hook: the filter's 64-bit-cursor drain at sizes a test can afford (valid at every size; same results)
        if (value < 0 || value > 1) return fail(HG_ERR_ARG, "real_far_cursors must be 0 or 1");
        c->real_far_cursors = value;
        return HG_OK;
    }
    if (!strcmp(key, "optimistic")) {                  // (a fresh start: the latches of lost bets are cleared)
        c->opt.optimistic = value != 0;
        c->bet_consecutive_fail = c->shard_bet_fail = 0;
        c->cfg_epoch++;
        return HG_OK;
    }
    if (!strcmp(key, "cap_boost")) {                   // run state: lost bets escalate it, every load resets it
        if (value < 1 || value > 4096) return fail(HG_ERR_ARG, "cap_boost must be 1..4096");
        // a caller that WIDENS the slices is retrying a lost sharded bet within the same call (sharded.evaluate_shard): that attempt
        // does not count towards hg_bet_eligible's "two calls in a row lost their bets"
        if (value > c->cap_boost && c->shard_bet_fail > 0) c->shard_bet_fail--;
        c->cap_boost = value;
        c->cfg_epoch++;
        return HG_OK;
    }
    for (const OptionKey& k : kOptionKeys) {
        if (strcmp(key, k.key)) continue;
        if (!k.flag && (value < k.lo || value > k.hi)) return fail(HG_ERR_ARG, "%s", k.range);
        c->opt.*k.field = k.flag ? value != 0 : value;
        c->cfg_epoch++;                                // whatever changes: a captured step is rebuilt
        return HG_OK;
    }
    return fail(HG_ERR_ARG, "hg_set_option: unknown key '%s'", key);
}

// Work buffers only grow (a big call leaves gigabytes behind for the next one to reuse); hg_trim
// gives everything but the loaded tables back (the images and AP tables are rebuilt on their next use).
int hg_trim(hg_ctx* c) {
    if (!c) return fail(HG_ERR_ARG, "hg_trim: null context");
    HG_TRY(c->use());
    HG_TRY(c->sync());
    c->for_each_buf([](DevBuf& d, BufClass k) { if (k != BUF_TABLE) d.release(); });
    c->forget_derived();
    c->hist_tot_zero = c->ws_b.hist_tot_zero = nullptr;   // (the plane totals went with the work buffers: a new allocation is cleared before its first pass)
    if (c->sub) { hg_ctx* s = c->sub; c->sub = nullptr; (void)hg_destroy(s); }
    c->stage &= (ST_DB | ST_Q);
    c->lists_valid = false;
    c->real_lists = false;
    cache_release_all();                               // (a caller that trims wants the memory back at the RUNTIME -- another framework in the process -- not in this library's cache)
    return HG_OK;
}

int hg_preload(hg_ctx* c) {
    if (!c) return fail(HG_ERR_ARG, "hg_preload: null context");
    HG_TRY(c->use());
    HG_TRY(preload_tables(c));
    HG_TRY(ensure_pin(c, (size_t)1 << 20));
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_ap<AP_THREADS>)));
    HG_TRY(preload_seq()); HG_TRY(preload_rank()); HG_TRY(preload_side()); HG_TRY(preload_valu()); HG_TRY(preload_mx()); HG_TRY(preload_mx1()); HG_TRY(preload_real()); HG_TRY(preload_rerank()); HG_TRY(preload_pq_encode());
    return HG_OK;
}

int hg_release_cache(void) {
    cache_release_all();
    return HG_OK;
}

int hg_get_stat(hg_ctx* c, const char* key, int64_t* value) {
    if (!c || !key || !value) return fail(HG_ERR_ARG, "hg_get_stat: null argument");
    if (!strcmp(key, "optimistic_runs")) *value = c->bet_runs;
    else if (!strcmp(key, "optimistic_fallbacks")) *value = c->bet_fallbacks;
    else if (!strcmp(key, "optimistic_requeried")) *value = c->bet_requeried;
    else if (!strcmp(key, "optimistic_rebets")) *value = c->bet_rebets;
    else if (!strcmp(key, "rank_leftovers")) *value = c->rank_leftovers;
    else if (!strcmp(key, "select_variant")) *value = c->last_select;
    else if (!strcmp(key, "rank_variant")) *value = c->last_rank;
    else if (!strcmp(key, "hist_variant")) *value = c->last_hist;
    else if (!strcmp(key, "rank_lds_recs")) *value = c->last_lds_recs;
    else if (!strcmp(key, "slice_cap")) *value = c->cap;
    else if (!strcmp(key, "rel_hist_variant")) *value = c->last_rel_hist;
    else if (!strcmp(key, "ap_at_cutoffs")) *value = c->aa.dim;
    else if (!strcmp(key, "votes_cutoffs")) *value = c->vt.dim;
    else if (!strcmp(key, "match_source")) *value = c->match_source;
    else if (!strcmp(key, "joint_hist_grades")) *value = c->jh_G;
    else if (!strcmp(key, "joint_hist_bands")) *value = c->jh_bands;
    else if (!strcmp(key, "merged_joint_grades")) *value = c->mjh_G;
    else if (!strcmp(key, "rel_hist_current")) *value = c->rh.current(c) ? 1 : 0;       // the shard's table of the loaded queries and database is there
    else if (!strcmp(key, "grade_hist_current")) *value = c->gh.current(c) ? 1 : 0;
    else if (!strcmp(key, "joint_hist_current")) *value = c->jh.current(c) ? 1 : 0;
    else if (!strcmp(key, "rerank_records")) *value = c->rr_records;
    else if (!strcmp(key, "rerank_chunks")) *value = c->rr_chunks;
    else if (!strcmp(key, "rerank_groups_lds")) *value = c->rr_groups_lds;
    else if (!strcmp(key, "rerank_groups_global")) *value = c->rr_groups_global;
    else if (!strcmp(key, "export_bytes")) *value = c->export_bytes;
    else if (!strcmp(key, "export_variant")) *value = c->export_variant;
    else if (!strcmp(key, "ap_fused")) *value = c->ap_fused ? 1 : 0;
    else if (!strcmp(key, "cap_boost")) *value = c->cap_boost;
    else if (!strcmp(key, "crowding_x100")) *value = c->crowd_x100;
    else if (!strcmp(key, "real_cap_boost")) *value = c->real_cap_boost;
    else if (!strcmp(key, "last_optimistic")) *value = c->optimistic ? 1 : 0;
    else if (!strcmp(key, "real_attempts")) *value = c->real.attempts;
    else if (!strcmp(key, "real_requeried")) *value = c->real_requeried;
    // how the last real-valued ranking ran: bit 0 = bf16 filter + exact rescoring, bit 1 = ranked by the LDS-resident kernel,
    // bit 2 = record lists beyond the LDS ordered group by group (k_real_group_*), bit 3 = the filter ran in IEEE half (else bfloat16)
    else if (!strcmp(key, "real_path")) *value = (c->real.filtered ? 1 : 0) | (c->real.lds_ranked ? 2 : 0) | (c->real.grouped ? 4 : 0) | (c->real.filtered && c->real.half ? 8 : 0);
    else if (!strcmp(key, "asym_calls")) *value = c->asym_calls;
    else if (!strcmp(key, "asym_float_rows")) *value = c->from_codes.rows_read;
    else if (!strcmp(key, "pq_calls")) *value = c->pq_calls;
    else if (!strcmp(key, "pq_float_rows")) *value = c->from_pq.rows_read;
    else if (!strcmp(key, "pq_encode_calls")) *value = c->pq_encode_calls;
    else if (!strcmp(key, "pq_encoded_rows")) *value = c->pq_encoded_rows;
    else if (!strcmp(key, "device_bytes")) *value = device_bytes(c);
#ifdef HG_RANK_PROFILE
#ifdef HG_RANK_PROFILE                        // (tools/rank_phase_profile.py: where k_rank_cnt left its phase timestamps)
    else if (!strcmp(key, "dbg_hwq_ptr")) *value = (int64_t)(uintptr_t)c->hwq.p;
#endif
#endif
    else if (!strcmp(key, "cache_device_bytes")) *value = cache_stat(0);      // the process-wide block cache (hg_ctx.hpp)
    else if (!strcmp(key, "cache_pinned_bytes")) *value = cache_stat(1);
    else if (!strcmp(key, "cache_hits")) *value = cache_stat(2);
    else if (!strcmp(key, "cache_misses")) *value = cache_stat(3);
    else if (!strcmp(key, "cache_streams")) *value = cache_stat(4);
    else if (!strncmp(key, "host_", 5)) {              // process-wide host-side phase timers (hg_ctx.hpp, HostPhase)
        const char* rest = key + 5;
        int kind = -1;                                 // 0 total us, 1 calls, 2 longest call us
        if (!strncmp(rest, "us_", 3)) { kind = 0; rest += 3; }
        else if (!strncmp(rest, "n_", 2)) { kind = 1; rest += 2; }
        else if (!strncmp(rest, "max_us_", 7)) { kind = 2; rest += 7; }
        int ph = -1;
        for (int i = 0; i < HP_COUNT; ++i) if (!strcmp(rest, kHostPhaseNames[i])) ph = i;
        if (kind < 0 || ph < 0) return fail(HG_ERR_ARG, "hg_get_stat: unknown key '%s'", key);
        *value = kind == 0 ? g_host_ns[ph].load() / 1000 : kind == 1 ? g_host_calls[ph].load() : g_host_max_ns[ph].load() / 1000;
    }
    else if (!strcmp(key, "graph_replays")) *value = c->graph_replays;
    else if (!strcmp(key, "cut_beyond_planes")) {      // a download: asked for after a lost owner-routed bet only
        u32 v = 0;
        if (c->beyond.p) {
            HG_HIP(hipMemcpyAsync(&v, c->beyond.p, 4, hipMemcpyDeviceToHost, c->stream));
            HG_TRY(c->sync());
        }
        *value = v;
    }
    else if (!strcmp(key, "map_async_steps")) *value = c->map_async_steps;
    else if (!strcmp(key, "map_async_redone")) *value = c->map_async_redone;
    else if (!strcmp(key, "map_overlapped_steps")) *value = c->map_overlapped;
    else if (!strcmp(key, "segments")) *value = c->geo.S;
    else if (!strcmp(key, "records_kept")) {
        // records the last bet's select pass left in the slices, over all live queries (a download of the slice counts: a
        // measurement read after the step, never part of one) -- kept / (Q R) is what the guess's margin costs
        const Geo& g = c->geo;
        *value = -1;
        if (c->optimistic && c->sl_cnt.p && c->sl_cnt.cap >= (size_t)g.S * g.Qpad * 4) {
            HG_TRY(c->use());
            HG_TRY(c->sync());
            std::vector<u32> h((size_t)g.S * g.Qpad);
            HG_HIP(hipMemcpy(h.data(), c->sl_cnt.p, h.size() * 4, hipMemcpyDeviceToHost));
            i64 total = 0;
            for (int s = 0; s < g.S; ++s) for (int q = 0; q < g.Q; ++q) total += h[(size_t)s * g.Qpad + q];
            *value = total;
        }
    }
    else return fail(HG_ERR_ARG, "hg_get_stat: unknown key '%s'", key);
    return HG_OK;
}

// What hg_set_database_f32 / hg_set_queries_f32 saw in the float table they were handed: entries outside {-1, 0, +1}, zeros, minus
// ones, and whether the floats are resident on the device -- from which the caller tells +-1 codes (Hamming ranking), {0,1} bits
// and real-valued features (inner-product ranking) apart.
int hg_get_census(hg_ctx* c, int queries, int64_t out[4]) {
    if (!c || !out) return fail(HG_ERR_ARG, "hg_get_census: null argument");
    const i64* cs = queries ? c->census_q : c->census_db;
    out[0] = cs[0]; out[1] = cs[1]; out[2] = cs[2];
    out[3] = (queries ? c->qf_resident : c->from_floats.rows_valid) ? 1 : 0;
    return HG_OK;
}

int hg_timing_enable(hg_ctx* c, int on) {
    if (!c) return fail(HG_ERR_ARG, "hg_timing_enable: null context");
    c->timing = on < 0 ? 0 : (on > 2 ? 2 : on);
    c->t_seq = 0;
    return HG_OK;
}

int hg_timing_reset(hg_ctx* c) {
    if (!c) return fail(HG_ERR_ARG, "hg_timing_reset: null context");
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream_b) (void)hipStreamSynchronize(c->stream_b);
    c->t_collect();
    for (int i = 0; i < KI_COUNT; ++i) { c->t_ms[i] = 0; c->t_n[i] = 0; }
    return HG_OK;
}

int hg_timing_read(hg_ctx* c, int cap, const char** names, double* total_ms, int64_t* launches, int* n) {
    if (!c || !n) return fail(HG_ERR_ARG, "hg_timing_read: null argument");
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream_b) (void)hipStreamSynchronize(c->stream_b);
    c->t_collect();                                    // events recorded since the last read
    int k = 0;
    for (int i = 0; i < KI_COUNT && k < cap; ++i) {
        if (!c->t_n[i]) continue;
        if (names) names[k] = kKernelNames[i];
        if (total_ms) total_ms[k] = c->t_ms[i];
        if (launches) launches[k] = c->t_n[i];
        ++k;
    }
    *n = k;
    return HG_OK;
}

}  // extern "C"

// Host side of libhashgan_amd.so, shared by its translation units: error plumbing, device buffers, the context
// (struct hg_ctx, opaque in include/hashgan_amd.h) and the handful of host functions one unit calls in another.
//
//   hg_core.hip        context, options / statistics / timing, label match, AP, downloads, results into device arrays (hg_export)
//   hg_tables.hip      the table loaders (hg_set_database*, hg_set_queries*, hg_get_packed): one shape check, three packers with one destination and one result record, one commit per table
//   hg_seq.hip         the Hamming sequences: geometry, histogram -> plan -> select -> rank, staged (sharded) and one-shot forms
//   hg_rank.hip        their rank stage: the choice of the kernel (RankChoice), one launcher per kernel, the leftovers of a fused step, k_order
//   hg_side.hip        the side metrics (hg_rel_hist, hg_graded, hg_grade_hist, hg_tie_ap, hg_ap_at, hg_joint_hist, hg_votes, hg_nbr_hist) and their getters: one SideResult each;
//                      the neighbour sets of label-free relevance and the match bitmap from them (hg_set_neighbours, hg_neighbours_from_lists, hg_match_neighbours);
//                      the shards' histogram tables packed and merged into the whole database's (hg_pack_side_table, hg_merge_side_table), and the
//                      grades and votes along a shard's partial lists (hg_pack_list_table, hg_merge_list_table)
//   hg_rerank.hip      the re-ranked Hamming ranking (hg_topr_rerank, hg_map_rerank): distance, then float32 inner product inside equal distances
//   hg_pairs_valu.hip  launchers of the vector-ALU pair passes (k_hist, k_select, k_select_dense)
//   hg_pairs_mx.hip    launchers of the matrix-core pair passes (k_select_mx3 / mx4, k_hist_mx, k_hist_i8) and their images
//   hg_pairs_mx1.hip   launcher of k_select_mx (every code length: the longest compile)
//   hg_real.hip        real-valued (float32 inner product) ranking: a ladder of attempts, each with one RealReq down and one RealState (hg_ctx::real) up;
//                      its asymmetric form (hg_topr_asym, hg_map_asym): the same call on the other RowSource, the database's packed codes read as +-1 (hg_asym.hpp);
//                      its quantised form (hg_topr_pq, hg_map_pq): the same call on a third, product-quantisation codes and codebooks (hg_pq.hpp; loaded by hg_set_database_pq, hg_tables.hip)
//   hg_pq_encode.hip   the exact product-quantisation encoder (hg_pq_encode, hg_pq_encode_dev: hg_pq_encode.hpp) and the loader from float features to a
//                      quantised context (hg_set_database_pq_f32: encode, then hg_set_database_pq on the codes)
//   hg_comm.hip        RCCL collectives (library dlopen'ed on first use)
//
// No torch, no CPU compute path: every entry point either runs HIP kernels or fails.
#pragma once
#include "hg_kernels.hpp"
#pragma GCC visibility push(default)     // the library is built with -fvisibility=hidden: only the C ABI is exported
#include "../../include/hashgan_amd.h"
#pragma GCC visibility pop

#include <rccl/rccl.h>     // types and enums only: the library itself is dlopen'ed by hg_comm_init (573 MB, not every process needs it)
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace hg;

extern thread_local std::string g_err;          // hg_last_error(): per thread
int fail(int code, const char* fmt, ...);       // sets g_err, returns code

#define HG_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? HG_ERR_NOMEM : HG_ERR_HIP, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                          \
    } while (0)

#define HG_TRY(expr)                \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != HG_OK) return rc_; \
    } while (0)


// Bumped whenever a device buffer moves: captured graphs hold raw addresses and die with the epoch they were built in.
extern std::atomic<unsigned long long> g_alloc_epoch;   // bumped by every context's buffers (one MAPs object per thread is supported): atomic

// Host-side cost of the runtime calls a context makes outside its kernels -- creating it, device and pinned allocations and
// their release -- accumulated process-wide (hg_get_stat "host_us_<phase>", "host_n_<phase>", "host_max_us_<phase>"): what a
// caller that builds a context per evaluation (main.py:164 builds a MAPs per evaluation) pays before any kernel runs.
enum HostPhase { HP_INIT = 0, HP_DEVMALLOC, HP_DEVFREE, HP_HOSTMALLOC, HP_HOSTFREE, HP_DESTROY, HP_STREAM, HP_EVENT, HP_SYNC, HP_PACK, HP_THREAD, HP_COUNT };
extern const char* const kHostPhaseNames[HP_COUNT];
extern std::atomic<long long> g_host_ns[HP_COUNT], g_host_calls[HP_COUNT], g_host_max_ns[HP_COUNT];
struct HostTimer {
    int id;
    std::chrono::steady_clock::time_point t0;
    explicit HostTimer(int i) : id(i), t0(std::chrono::steady_clock::now()) {}
    ~HostTimer() {
        const long long ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        g_host_ns[id] += ns;
        g_host_calls[id] += 1;
        long long m = g_host_max_ns[id].load();
        while (ns > m && !g_host_max_ns[id].compare_exchange_weak(m, ns)) {}
    }
};
template <class F> inline auto host_timed(int id, F&& f) { HostTimer t_(id); return f(); }

// HG_EFENCE=1 (debugging): every device buffer ends 64..127 bytes before an UNMAPPED 2 MiB page of its own virtual range
// (hipMemAddressReserve / hipMemMap), so a kernel reading or writing past a buffer -- beyond the 64 bytes of slack the
// kernels are allowed -- faults at once instead of only when hipMalloc happens to place the buffer at the end of a mapping;
// and every new buffer starts out filled with 0xCB, so nothing can rely on fresh memory being zero.  HG_EFENCE=2: the
// fill only, on plain allocations; HG_EFENCE=3: the unmapped page in FRONT of every buffer.  (tools/fuzz_*.py and the gpu
// tests run under all three.)
struct Fence { void* va = nullptr; void* map_at = nullptr; size_t va_size = 0, map_size = 0; hipMemGenericAllocationHandle_t h{}; };
inline int efence_mode() { static const int m = getenv("HG_EFENCE") ? atoi(getenv("HG_EFENCE")) : 0; return m; }
inline bool efence_on() { return efence_mode() != 0; }
inline hipError_t fence_alloc(Fence& f, void** out, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
    if (e != hipSuccess) return e;
    if (gran < ((size_t)2 << 20)) gran = (size_t)2 << 20;
    f.map_size = (bytes + gran - 1) / gran * gran;
    f.va_size = f.map_size + gran;                                   // the last granule stays unmapped
    e = hipMemAddressReserve(&f.va, f.va_size, gran, nullptr, 0);
    if (e != hipSuccess) return e;
    e = hipMemCreate(&f.h, f.map_size, &prop, 0);
    if (e != hipSuccess) return e;
    // HG_EFENCE=3: the unmapped granule comes FIRST and the buffer starts right behind it (reads before a buffer)
    const bool front = efence_mode() == 3;
    f.map_at = (char*)f.va + (front ? gran : 0);
    e = hipMemMap(f.map_at, f.map_size, 0, f.h, 0);
    if (e != hipSuccess) return e;
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    e = hipMemSetAccess(f.map_at, f.map_size, &acc, 1);
    if (e != hipSuccess) return e;
    *out = front ? f.map_at : (char*)f.va + ((f.map_size - bytes) & ~(size_t)63);       // 64-byte aligned, ends < 64 bytes before the fence
    return hipSuccess;
}
inline void fence_free(Fence& f) {
    if (!f.va) return;
    (void)hipDeviceSynchronize();                                    // hipFree waits for the device; unmapping does not
    (void)hipMemUnmap(f.map_at, f.map_size);
    (void)hipMemRelease(f.h);
    // (the virtual range is NOT returned: a later buffer at the same address could meet stale cache lines of this one)
    f = Fence{};
}

// Process-wide cache of what a context allocates and a destroyed (or trimmed) context gives back: device blocks, pinned host
// blocks, streams.  hipMalloc on this stack takes 0.03 - 0.4 ms -- and now and then SECONDS (3.5 s measured for one call among
// a few hundred: tools/new_context_probe.py, profiles/r06_new_context_probe.txt), hipStreamCreate 1.5 - 18 ms, a 64 MB
// hipHostMalloc 9 ms, hg_destroy's frees 3.7 ms: a caller that builds a context per evaluation paid all of that per call.  A
// block goes back to the cache instead of the runtime and the next request of a similar size takes it (best fit, at most twice
// the size asked for); the cache holds at most HG_CACHE_MB (default 49152 -- a class-sorted C2 database's widened record slices alone are 14.9 GB) of device and HG_PIN_CACHE_MB (default 512) of pinned
// memory -- the largest blocks go first when it is full -- and hg_release_cache() empties it.  HG_EFENCE builds bypass it.
void* cache_take_dev(int device, size_t want, size_t* got);           // nullptr: nothing suitable cached
void cache_give_dev(int device, void* p, size_t bytes);              // (frees it if the cache is full)
void* cache_take_pin(size_t want, size_t* got);
void cache_give_pin(void* p, size_t bytes);
hipStream_t cache_take_stream(int device);                           // nullptr: none cached
int stream_create(int device, hipStream_t* out);                    // from the cache, else a new non-blocking stream
void cache_give_stream(int device, hipStream_t s);
void cache_release_all();
inline size_t cache_round(size_t bytes) {                            // sizes a later request can match: 4 KB up to 1 MB, then 1 MB
    const size_t g = bytes < ((size_t)1 << 20) ? 4096 : (size_t)1 << 20;
    return (bytes + g - 1) / g * g;
}
// pinned host block through the cache (*cap = what the block really holds)
inline hipError_t pin_alloc(void** p, size_t want, size_t* cap) {
    *p = cache_take_pin(want, cap);
    if (*p) return hipSuccess;
    const size_t sz = cache_round(want);
    const hipError_t e = host_timed(HP_HOSTMALLOC, [&] { return hipHostMalloc(p, sz, hipHostMallocDefault); });
    if (e == hipSuccess) *cap = sz;
    return e;
}
inline void pin_free(void* p, size_t cap) { if (p) cache_give_pin(p, cap); }
inline hipError_t pin_grow(void** p, size_t* cap, size_t want) {     // a block of at least `want` bytes (a smaller one is given back, its contents with it)
    if (*cap >= want) return hipSuccess;
    pin_free(*p, *cap);
    *p = nullptr; *cap = 0;
    return pin_alloc(p, want, cap);
}

// A device buffer that only ever grows.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    size_t blk = 0;             // bytes of the allocation behind p (0: borrowed, or a fenced one)
    int dev = 0;
    bool borrowed = false;      // points into another context's allocation
    Fence fence;                // HG_EFENCE: the buffer's own virtual range
    void drop() {
        if (p && !borrowed) {
            if (fence.va) { HostTimer t_(HP_DEVFREE); fence_free(fence); }
            else if (blk) cache_give_dev(dev, p, blk);
            else { HostTimer t_(HP_DEVFREE); (void)hipFree(p); }
        }
        blk = 0;
    }
    int reserve(size_t bytes) {
        if (bytes <= cap) return HG_OK;
        drop();
        p = nullptr; cap = 0; borrowed = false;
        // slack: 16-byte wide copies may read past the last row of a table
        if (efence_mode() == 2) {                           // plain allocation, poisoned
            HG_HIP(hipMalloc(&p, bytes + 64));
            HG_HIP(hipMemset(p, 0xCB, bytes + 64));
            HG_HIP(hipDeviceSynchronize());                  // (the fill runs on the null stream; the context's stream does not wait for it)
        } else if (efence_on()) {
            HG_HIP(fence_alloc(fence, &p, bytes + 64));
            HG_HIP(hipMemset(p, 0xCB, bytes + 64));
            HG_HIP(hipDeviceSynchronize());
        } else {
            HG_HIP(hipGetDevice(&dev));
            p = cache_take_dev(dev, bytes + 64, &blk);
            if (!p) {
                const size_t sz = cache_round(bytes + 64);
                HG_HIP(host_timed(HP_DEVMALLOC, [&] { return hipMalloc(&p, sz); }));
                blk = sz;
            }
        }
        cap = bytes;
        ++g_alloc_epoch;
        return HG_OK;
    }
    void borrow(const DevBuf& o) {
        drop();
        if (p != o.p) ++g_alloc_epoch;
        p = o.p; cap = o.cap; borrowed = true;
    }
    // `bytes` at `off` inside another buffer (which must outlive the view)
    void view(const DevBuf& o, size_t off, size_t bytes) {
        drop();
        if (p != (char*)o.p + off) ++g_alloc_epoch;
        p = (char*)o.p + off; cap = bytes; borrowed = true;
    }
    void release() { drop(); if (p) ++g_alloc_epoch; p = nullptr; cap = 0; borrowed = false; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

enum KernelId { KI_HIST = 0, KI_HIST_REDUCE, KI_PLAN, KI_SEG_COUNTS, KI_SEG_LAYOUT, KI_GUESS, KI_SELECT, KI_CAND_HIST,
                KI_ORDER, KI_RANK_FUSED, KI_MATCH, KI_AP, KI_MERGE, KI_PACK, KI_REAL_SAMPLE, KI_REAL_GUESS, KI_REAL_SELECT,
                KI_RADIX, KI_REAL_FINISH, KI_SELECT_MX, KI_RANK_LDS, KI_COMM, KI_STEP, KI_REAL_RESCORE, KI_HIST_REL, KI_HIST_REL_REDUCE,
                KI_GRADED, KI_GRADE_HIST, KI_GRADE_HIST_REDUCE, KI_TIE_AP, KI_AP_AT, KI_LABEL_MAX, KI_HIST_JOINT, KI_HIST_JOINT_REDUCE,
                KI_RR_SCAN, KI_RR_COLLECT, KI_RR_SCORE, KI_RR_ORDER, KI_EXPORT, KI_VOTES, KI_VOTE_CONFUSION, KI_SIDE_PACK, KI_SIDE_MERGE,
                KI_LIST_GRADES, KI_LIST_MERGE_GRADES, KI_LIST_MERGE_VOTES, KI_VOTE_PICK, KI_ASYM_IMAGE, KI_ASYM_RESCORE, KI_ASYM_EXPAND,
                KI_NBR_SORT, KI_NBR_MATCH, KI_NBR_HIST, KI_PQ_IMAGE, KI_PQ_RESCORE, KI_PQ_EXPAND, KI_PQ_ENCODE, KI_COUNT };
enum Stage { ST_NONE = 0, ST_DB = 1, ST_Q = 2, ST_HIST = 4, ST_PLAN = 8, ST_SELECT = 16, ST_MATCH = 32, ST_AP = 64 };
extern const char* const kKernelNames[KI_COUNT];
// the kernel that took the last record pass / the last rank stage (stats "select_variant", "rank_variant"), and what the rank stage is asked for
enum SelectKernel { SEL_NONE = 0, SEL_VALU = 1, SEL_DENSE = 2, SEL_MX = 3, SEL_MX3 = 5, SEL_MX4 = 6 };   // none, k_select, k_select_dense, k_select_mx, k_select_mx3, k_select_mx4
enum RankKernel { RK_NONE = 0, RK_FUSED = 1, RK_CNT = 3, RK_LEAN = 6, RK_DENSE = 7, RK_SLICES = 8 };    // none, k_rank_fused, k_rank_cnt, k_rank_lean, k_rank_dense, k_rank_dense<slices>
enum RankMode : int { RANK_WHOLE = 0, RANK_COUNT = 1, RANK_PLACE = 2, RANK_LOCAL = 3 };   // RankArgs::mode, RankLdsArgs::mode: the whole ranking (one shard); on several
                           // shards the records' histograms before the exchange, then the placement with the shared plan; this shard's records ranked locally (hg_select_ranked)

void build_shape(int n, ApShape& sh);           // NumPy's pairwise-summation tree of an n-element chunk, flattened (hg_core.hip)

struct Pending { int id; hipEvent_t a, b; };

// The engine's options: one field per key of hg_set_option, named after the key, its default the initialiser.  The keys'
// accepted values are in hg_set_option's table (hg_core.hip); DESIGN.md section 9 lists them with the tests that set them.
struct Options {
    // segments of the pair passes
    i64 target_units = 16384;      // wavefront-sized units the pair passes are split into (segment count)
    i64 min_segment = 256;         // shortest segment, rows
    i64 max_segments = 2048;       // cap on the segment count (few queries)
    // the one-shot bet
    i64 optimistic = 1;            // one-shot calls may bet on a sampled threshold (verified, exact fallback)
    i64 sample_stride = 0;         // sampling stride in row batches, 0 = auto
    i64 guess_sigma = 5;           // safety margin of the guess, in standard deviations of the sample count (5: a query loses its bet
                                   // about once in 3 million -- it is then rerun alone; 6 -> 5 keeps ~4 % fewer surplus records)
    i64 cand_budget_x10 = 40;      // optimistic record budget per query, in tenths of R
    i64 second_bet = 1;            // a lost one-shot bet is retried once with a wider margin before the exact sequence
    i64 crowd_probe = 1;           // the first bet on a database measures how its near rows crowd (k_guess_direct's probe)
    // kernels
    i64 select_mfma = 1;           // optimistic select: 1 = matrix-core kernel (k_select_mx), 0 = vector-ALU k_select
    i64 select_packed = 3;         // several distances per MFMA accumulator: 3 = k_select_mx3 (<= 64 bits, three) / k_select_mx4 (65..128 bits, two) with
                                   // the batched drain, for one-byte records; anything else = k_select_mx (one distance per accumulator)
    i64 compact_records = 1;       // one-byte compact records (matrix-core select, no lists wanted)
    i64 hist_mfma = 2;             // histograms (sampled pass; full pass of the one-shot exact sequence) on the matrix cores -- 2: the integer instruction
                                   // delivers the counter address (k_hist_i8, codes of <= 128 bits), 1: fp4 distances (k_hist_mx), 0: vector ALU
    i64 rank_lds = 2;              // the bet's rank stage keeps a query's records in LDS: >= 1 the per-thread counting sort (k_rank_cnt) where it
                                   // applies, 2 its lean form (k_rank_lean) for one-byte records without lists, <= 256 slices, <= 1024 pieces per query
    i64 rank_slices = 7000;        // a bet's one-byte records with R >= this are ranked by k_rank_dense<slices>; 0: off (k_rank_cnt's tiles).
                                   // Q = 10k, N = 1M: R = 5000 0.274 ms against k_rank_lean's 0.139 (fixed costs of the counter columns); R = 8000 0.318 / 0.372; R = 50 000 1.38 / 3.83
    i64 rank_dense = 1;            // N/8 < R <= N on one shard through the byte matrix (k_dense_bytes + k_rank_dense, hg_rank_dense.hpp; codes of <= 126 bits, <= 128 classes); 0: off
    i64 rank_dense_gbm = -1;       // k_rank_dense's bitmap in global memory (1) or LDS (0, where it fits); -1: by the blocks per CU
    i64 dense_budget_mb = 16384;   // the byte matrix D holds at most this much (queries are chunked)
    i64 all_rows_shortcut = 1;     // R = N: skip histogram and plan (every row is a member)
    i64 fuse_ap = 1;               // AP from the rank kernel's epilogue (k_rank_cnt: the bitmap is still in LDS)
    i64 inline_leftovers = 1;      // queries the fused rank kernel declined are ranked within the step's stream
    i64 ap_wide = 1;               // k_ap with 512 threads per query when the queries are few and their lists long (0: always 128)
    i64 ap_recip = 1;              // k_ap divides through the table of reciprocals (bit for bit the division; 0: divide)
    i64 probe_select = 0;          // measurement probes of the matrix-core select kernels (SelArgs::probe; a key of the HG_PROBES build only)
    i64 probe_votes = 0;           // 1: k_votes counts by ballots, the form its LDS adds were measured against (hg_votes.hpp; a key of the HG_PROBES build only)
    // call protocol
    i64 stage_sync = 1;            // staged calls synchronise the stream before returning
    i64 defer_verdict = 0;         // hg_rank does not wait for the bet's verdict; hg_bet_verdict reads it later
    i64 staged_lists = 1;          // staged hg_select materialises the idx/dist lists
    i64 step_graph = 0;            // 1 = hg_map captures and replays its step (see run_oneshot)
    i64 step_streams = 2;          // 2 = hg_map_begin's slot-1 blind steps on stream_b, 1 = every step on the context's stream
    i64 timing_every = 1;          // level-1 timing records its events on every n-th one-shot step only
    // hand-over of float32 / int64 arrays
    i64 host_pack = 1;             // packed on the host by a thread pool before the upload (hg_host_pack.hpp); 0 = upload the raw arrays, pack on the GPU
    i64 keep_floats = 2;           // database float table on the GPU -- 0 never, 1 always, 2 only if it is not a +-1 code
    i64 pq_encode_chunk_rows = 0;  // rows per launch of the PQ encoder (host features: per upload through the work buffer); 0: 256 MB of work buffers
    i64 keep_query_floats = 0;     // 1: the query float table stays on the GPU whether or not the database's is there (the asymmetric ranking: hg_map_asym)
    // real-valued ranking
    i64 real_mfma = 2;             // 2 = bf16 filter on the matrix cores + exact rescoring of the survivors, 1 = exact float32 MFMA pass, 0 = vector ALU
    i64 real_sample_half = 1;      // the sampled cut's scores in the filter's 16-bit arithmetic (k_real_sample_h) instead of exact float32 chains
    i64 real_second_sample = 1;    // a second, counting sample four times as large tightens the sampled cut
    i64 real_sort_lds = 1;         // sort + finish of the filter path in one LDS-resident kernel when the records fit
    i64 real_groups = 1;           // record lists beyond the LDS are split by score range and ordered group by group in LDS (0: the four radix passes)
    i64 real_map_lists = 0;        // hg_map_real also writes the ranked idx / score lists (hg_get_topr_real after it); 0: match bits and APs only, like hg_map
    i64 real_whole_rounds = 3;     // the no-cut float32 MFMA pass (k_real_select_mx) cuts the database so that its blocks fill whole rounds of this many
                                   // per CU; 0: the plain geometry
};

// What a device buffer of the context holds (hg_ctx::for_each_buf): hg_trim keeps the tables and frees the rest.
enum BufClass {
    BUF_TABLE,      // loaded by hg_set_*
    BUF_DERIVED,    // built from the tables or R on first use, valid while a key says so (hg_ctx::forget_derived resets every key)
    BUF_WORK,       // written by a call, reserved again by the next one
};

// The buffers a bet writes: the context's own (hg_ctx inherits them) and a second set (hg_ctx::ws_b) for the slot-1 steps of
// hg_map_begin on the second stream.
struct StepBufs {
    DevBuf hist, hown, posbase, t, tguess, sstar, cnt_lt, quota, tie_before, n_lt, err, sl_start, sl_tie, sl_cnt, tot, failq,
           cand, out_idx, out_dist, mbits, ap, rel, qbad, bigq, hwq;
    DevBuf outblk;             // [verdict 16 B][ap Q x 8][rel Q x 4]: err, ap and rel are views of it (ensure_out_block), so a call's results come home in ONE copy
    i64 outblk_q = -1;         // the Q those views were cut for
    // The one-shot bet's plane totals, two planes to a u64 word, [(planes the sampled pass writes + 1) / 2][Qpad]: k_hist_i8 adds each segment pair's counts, k_guess_direct
    // reads a query's column in one trip and stores zeros over it.  hist_tot_zero is the allocation known to hold zeros behind everything
    // enqueued so far (nullptr: not known -- a fresh allocation, a pass with no guess behind it); the next bet then clears it first.
    DevBuf hist_tot;
    const void* hist_tot_zero = nullptr;
    template <class F> void for_each_step_buf(F&& f) {
        for (DevBuf* d : {&hist_tot, &hist, &hown, &posbase, &t, &tguess, &sstar, &cnt_lt, &quota, &tie_before, &n_lt, &err, &sl_start, &sl_tie,
                          &sl_cnt, &tot, &failq, &cand, &out_idx, &out_dist, &mbits, &ap, &rel, &qbad, &bigq, &hwq})
            f(*d, BUF_WORK);
        f(outblk, BUF_DERIVED);
    }
};

// What the enqueue of a step leaves behind on the host for the entry points after it.  hg_ctx inherits it, and a captured step
// (hg_ctx::StepGraph) keeps the copy its replays restore by one assignment.
struct StepState {
    unsigned stage = ST_NONE;
    Geo geo{};
    i64 RW = 0;
    bool optimistic = false;   // records come from a guessed threshold (fixed-capacity slices)
    bool lists_valid = false;
    bool rec8 = false;         // the record rows hold one-byte compact records (matrix-core select, no lists wanted)
    u32 cap = 0;               // optimistic slice capacity
    i64 crow = 0;              // record-row stride
    // AP from the rank kernel's epilogue (k_rank_cnt: the bitmap is still in LDS) -- one launch less per step, and the general
    // rank kernel for the queries k_rank_cnt declines is launched only when the step's download says there are any
    bool ap_fused = false;     // the last launch_rank left the AP of every query it ranked in c->ap / c->rel, leftovers counted in err[1]
    bool leftovers_inline = false;     // ... and the step ranked those leftovers itself within the stream (rank_lds_done)
    int last_select = SEL_NONE;   // stat "select_variant": a SelectKernel
    int last_rank = RK_NONE;   // stat "rank_variant": a RankKernel
    int last_hist = 0;         // stat "hist_variant": 1 k_hist, 2 k_hist_mx, 3 k_hist_i8; + 4: the matrix-core kernel's counters were dwords (else 16-bit halves)
    i64 last_lds_recs = 0;     // stat "rank_lds_recs": the record capacity handed to the last k_rank_lean / k_rank_cnt launch (RankLdsArgs::lds_recs)
};

// What one enqueue of a step is asked to do.  Built by the entry point and passed down by const reference to the launchers; a
// level that knows more (the guess kernel has cleared the verdict word, the sequence cuts at the exact threshold) hands a copy
// on, so a request ends with its call.  The staged entry points pass the default.
struct StepReq {
    bool fuse_ap = false;      // AP from the rank kernel's epilogue wanted (hg_map), where option "fuse_ap" and the kernel allow it
    enum Rows { RECORDS, BYTES, DIRECT } rows = RECORDS;   // the rank stage's rows: the select's records, the byte matrix (k_dense_bytes
                               // + k_rank_dense), or the database rows themselves (R = N: k_rank_fused computes distance and match bit per row)
    bool exact_cut = false;    // the matrix-core select and the LDS rank kernels cut at the EXACT threshold c->t (hg_hist + k_plan), not the guess c->tguess
    bool err_zeroed = false;   // the guess kernel in front of the rank stage already cleared the verdict word
    i64 guess_sigma = 0;       // the bet's margin and record budget for this attempt (options "guess_sigma", "cand_budget_x10"; a second
    i64 cand_budget_x10 = 0;   // bet widens both)
    void* dst = nullptr;       // pinned block the results go to (hg_map_begin's slot); nullptr: the context's own
};

// What one attempt of the real-valued ranking (hg_real.hip) is asked to do.  Built by real_attempt and passed down by const reference
// to the sample and select stages and their launchers; the stage that places the cut writes what it learns into the attempt's copy
// before the stages after it see it, so a request ends with its attempt.
struct RowSource;
struct RealReq {
    RowSource* src = nullptr;  // the database's rows this call ranks: the context's from_floats, from_codes or from_pq (a requery child: its parent's)
    i64 R = 0;
    bool bet = false;          // cut at a sampled threshold `sigma` deviations deep, slices sized for `budget` x R records per query
    double sigma = 0.0, budget = 0.0;
    bool with_ap = false;      // hg_map_real: APs wanted
    // derived by the attempt for the levels below it
    bool no_cut = false;       // every row a record (thr = -inf)
    double expect = 0.0;       // rows per query the cut is expected to keep (a second sample lowers it; picks the rescore's slices per wavefront)
    bool samp16 = false;       // the sample's scores are 16-bit (k_real_sample_h writes, k_real_guess_lds reads)
    bool skip_lists = false;   // the kernels that rank in LDS leave the idx / score lists out (match bits and APs only)
};

// What an attempt of the real-valued ranking leaves behind on the host: real_attempt begins by assigning a fresh one (keeping the
// count), so nothing survives from an earlier attempt or call.  Stat "real_path" is computed from it.
struct RealState {
    bool filtered = false;     // the select left unscored candidates that k_real_rescore completed (filter + rescore)
    bool lds_ranked = false;   // the LDS-resident rank kernel produced the lists
    bool grouped = false;      // the record lists were ordered group by group (k_real_group_*)
    bool lists_made = false;   // out_idx / scores hold the ranked lists (hg_map_real skips them on the paths that rank in LDS)
    bool half = false;         // the filter ran in IEEE half (else bfloat16): bit 3 of stat "real_path"
    i64 attempts = 0;          // stat "real_attempts": attempts of the last call (1 = the first bet held)
};

// What the real-valued ranking (hg_real.hip) reads and derives from the database's rows.  The context holds one per kind, each with its
// own buffers and keys -- an image built from codes and one built from a float table never meet -- and a call is handed the one it runs
// on (RealReq::src: hg_map_real from_floats, hg_map_asym from_codes, hg_map_pq from_pq); hg_real.hip's row-source section alone looks at the kind.
struct RowSource {
    enum Kind { FLOATS, CODES, PQ } kind;   // the loaded float table (hg_set_database_f32 / _dev with keep_floats) | the packed codes c->db read as +-1 (hg_asym.hpp)
                               // | product-quantisation codes and codebooks (hg_set_database_pq, hg_pq.hpp)
    DevBuf rows;               // f32 [N][bpad].  FLOATS: the table as loaded (BUF_TABLE; rows_valid: it is resident).  CODES, PQ: the rows (pads 0) expanded on first
                               // need per database (k_asym_expand_rows, k_pq_expand_rows) for the paths that read float rows (no cut, vector fallbacks, real_mfma < 2): BUF_WORK
    DevBuf rowsx;              // rows in MFMA A-fragment order (k_real_select_mx)
    DevBuf img, xmax2;         // filter + rescore path (hg_real_bf.hpp): 16-bit image of the rows, their max norm^2 (ensure_filter_image)
    bool rows_valid = false, rowsx_valid = false, img_valid = false;
    bool img_half = false;     // img is in IEEE half instead of bfloat16 (no feature of the database can overflow it)
    i64 rows_read = 0;         // CODES, PQ, stats "asym_float_rows" / "pq_float_rows": the last call read the expanded rows
    // PQ: the tables hg_set_database_pq loaded (BUF_TABLE) -- codes u8 [N][MP], MP = M rounded up to 4 with pad bytes 0, and codebooks f32 [M][K][dsub];
    // pq_xmax2 >= every row's norm^2: the sum over the subspaces of the largest norm^2 among the codewords that occur, rounded up
    DevBuf pq_codes, pq_books;
    int pq_M = 0, pq_K = 0, pq_dsub = 0, pq_MP = 0;
    float pq_xmax2 = 0.0f;
    bool pq_valid = false;     // the PQ tables are the loaded database's (any other database loader ends that)
    void forget_derived() { rowsx_valid = img_valid = false; if (kind != FLOATS) rows_valid = false; }   // a database load, hg_trim: each is rebuilt on its next use
    void forget_tables() { pq_valid = false; pq_codes.release(); pq_books.release(); }
};

// The results of one side metric (hg_side.hip) and what they were computed from: the generations of the two tables, the rows Q, their
// pitch Qpad (where the table is pitched), the second dimension (NB, C + 1, nk, nR or NB * G).  The entry point calls begin() first and finish()
// last, so a refused or failed call leaves none; the getters, and hg_tie_ap for the histogram it reuses, ask current().  DESIGN.md, "Side metrics: the host side".
struct hg_ctx;
struct SideResult {
    bool done = false;
    unsigned long long q_gen = 0, db_gen = 0;
    i64 Q = 0, Qpad = 0, dim = 0;
    void begin() { done = false; }
    inline void finish(const hg_ctx* c, i64 Q_, i64 Qpad_, i64 dim_);
    inline bool current(const hg_ctx* c) const;
};

struct hg_ctx : StepBufs, StepState {
    int device = 0;
    int n_cu = 256;            // compute units of the device
    hipStream_t stream = nullptr;
    bool own_stream = true;    // false: the stream belongs to the caller (hg_set_stream) or to the parent context
    Options opt;

    // problem
    i64 N = 0, Q = 0, R = 0, n_total = 0;
    int b = 0, C = 0, NW = 0, NB = 0, LW = 0;
    u32 idx_base = 0;
    int G = 1, rank = 0;

    bool crowd_probed = false; // the first bet on this database has measured how its near rows crowd (k_guess_direct's probe)
    i64 crowd_x100 = 0;        // stat "crowding_x100": that measure, x 100 (~200: rows in random order; ~100 x classes: stored class by class)
    i64 cap_boost = 1;         // slice capacity multiplier a lost bet escalated to on this database (run_oneshot); 1 after every load
    i64 real_cap_boost = 1;    // the same for the real-valued ranking's slices (real_ladder)
    bool leftovers_expected = false;   // the last fused step on this context left queries to the general kernel
    bool last_leftovers_inline = false;   // ... and the last finished step had ranked its own within the stream (finish_leftovers)

    // run state (what a step leaves behind: StepState)
    bool want_lists = true;
    i64 bet_runs = 0, bet_fallbacks = 0, bet_requeried = 0;   // stats "optimistic_runs", "optimistic_fallbacks", "optimistic_requeried"
    i64 rank_leftovers = 0;    // stat "rank_leftovers": queries of fused steps that k_rank_cnt left to the general rank kernel
    int bet_consecutive_fail = 0;   // one-shot bets lost in a row (this context only)
    int shard_bet_fail = 0;         // sharded bets lost in a row: identical on every rank by construction
    hg_ctx* sub = nullptr;     // child context (shares the database) that reruns single lost queries exactly (requery_child)
    bool is_sub = false;

    // device state (the buffers themselves: for_each_buf)
    bool dbx_valid = false, qx_valid = false, dbx8_valid = false, dbx3_valid = false, dbx4_valid = false;
    bool hist_pairs = false;   // the last FULL histogram pass ran per segment pair (k_hist_mx)
    i64 bet_rebets = 0;        // stat "optimistic_rebets"
    // the side metrics (hg_side.hip): one record per result set, and what is a feature's own next to it
    SideResult rh;             // hg_rel_hist: rh_all / rh_rel [NB][Qpad]
    SideResult gr;             // hg_graded: gr_out's four tables [Q][nk] of the ranked lists it found
    SideResult gh;             // hg_grade_hist: gh_tab [C + 1][Qpad]
    SideResult ta;             // hg_tie_ap: ta_out's seven tables [Q][nR]
    SideResult aa;             // hg_ap_at: aa_out, ap [Q][nR] and rel [Q][nR] of the match bitmap the last ranking left; dim is also stat "ap_at_cutoffs"
    SideResult jh;             // hg_joint_hist: jh_tab [NB * G][Qpad]; dim = NB * G
    SideResult vt;             // hg_votes: vt_votes [Q][nk][C], vt_pred's pred / top [Q][nk], vt_conf [nk][C][C] of the ranked lists it found; dim = nk, also stat "votes_cutoffs"
    SideResult mrh, mgh, mjh;  // hg_merge_side_table: the shards' tables summed into the whole database's -- mg_rel [2][NB][Qpad] (all, then rel; dim = NB),
                               // mg_grade [C + 1][Qpad], mg_joint [NB * Gc][Qpad] (dim = NB * Gc).  Ended by the merge's own refusal or failure, a reload, hg_trim
    SideResult mlg, mlv;       // hg_merge_list_table (hg_list_merge.hpp): the shards' grade planes merged into lm_grades [Q][Rp] (Qpad = Rp, dim = R), their vote tables
                               // into lm_votes [Q][nk][C] (dim = nk, the cut-offs in mlv_ks).  They belong to the ranked lists too: ended like gr and vt (lists_changed), and by their own merge's refusal
    SideResult nb;             // hg_set_neighbours / hg_neighbours_from_lists: nb_ids [Q][G] sorted, nb_cnt [Q]; dim = G.  A table of the loaded queries and database
    SideResult nh;             // hg_nbr_hist: nh_tab [NB][Qpad] of nb's sets (a new set ends it)
    int match_source = 0;      // stat "match_source": the match bitmap came from the labels (0) or from the neighbour sets (1: hg_match_neighbours); every ranking resets it (set_R)
    i64 mlv_ks[64] = {0};      // the cut-offs of the merged vote table: hg_votes on a shard takes these and no others
    int mjh_G = 0;             // stat "merged_joint_grades": the common grade count Gc of the last joint merge that succeeded (0: none yet)
    SideResult rr;             // the last ranking was a re-rank (hg_rerank.hip) of these tables: rr_scores [Q][R]; dim = R.  Not a side metric -- set_R ends it
    i64 rr_records = 0, rr_chunks = 0, rr_groups_lds = 0, rr_groups_global = 0;   // stats "rerank_records" / "rerank_chunks" / "rerank_groups_lds" / "rerank_groups_global" of the last re-rank
    int jh_G = 0, jh_bands = 0;   // stats "joint_hist_grades" / "joint_hist_bands": grades and distance bands of the last hg_joint_hist (0: no pass yet)
    int last_rel_hist = 0;     // stat "rel_hist_variant": 1 k_hist_rel (0: no pass yet)
    bool gr_kept = false; i64 gr_R = 0;   // gr_grades holds the grade bytes [Q][gr_R] of gr's pass
    i64 aa_recip_n = -1;       // aa_recip holds RN(1 / k) for k = 1 .. this (+ AP_RECIP_SLACK)
    i64 export_bytes = 0; int export_variant = 0;   // stats "export_bytes" / "export_variant" of the last hg_export: bytes written; bit 0 a 16-byte-store kernel ran, bit 1 an element-wise one
    void lists_changed() { gr.begin(); vt.begin(); mlg.begin(); mlv.begin(); }   // the ranked lists are no longer the ones hg_graded / hg_votes walked (a merge into them)
    void bitmap_changed() { aa.begin(); }     // the match bitmap is no longer the one hg_ap_at walked (hg_match, the merges, a blind step)
    bool mbits_merged = false; // G > 1: the shards' bitmaps have been merged into mbits for all queries (hg_merge_match, hg_merge_ranked)
    bool mbits_in_ws_b = false;   // the last ranking was a blind step on stream_b: its bitmap is ws_b's, not mbits
    bool verdict_pending = false, verdict_known = false;
    int verdict_flag = 0;
    // pinned landing zone for a one-shot call's results: AP, hit counts and the lost-bet flag come back with the
    // call's single synchronisation instead of three blocking copies into pageable memory afterwards
    void* pin = nullptr;
    size_t pin_cap = 0;
    // hg_map_begin / hg_map_end: up to two steps in flight, each with its own pinned landing block and event
    struct MapSlot {
        void* pin = nullptr; size_t cap = 0; hipEvent_t ev = nullptr;
        bool async = false;            // enqueued only (else: ran synchronously, results in ap / rel)
        bool inline_ok = false;        // the step ranked its fused kernel's leftovers itself
        i64 R = 0, Q = 0;
        unsigned long long q_gen = 0, db_gen = 0;   // the tables the step was enqueued on (hg_map_end redoes a lost step only on those)
        std::vector<double> ap; std::vector<int64_t> rel;
    } mslot[2];
    int ms_head = 0, ms_n = 0;
    // Slot 1's blind steps run on a second stream (option "step_streams" = 2), so that two consecutive steps overlap on the GPU:
    // the tail of one (k_rank_lean, the download) and the sampled pass and guess of the next run beside the other's select.  Such
    // a step writes a workspace of its own -- every buffer a bet writes, swapped in for the enqueue (swap_step) -- and reads
    // the shared tables (database images, query tables, AP tables), which only ever change on the context's stream.
    //   stream_b  waits, before the step, for everything on the context's stream but a blind slot-0 step in flight: ev_pre
    //             (recorded just before that step, while pre_valid) or else ev_fork at the stream's tail;
    //   stream    waits for stream_b's work (b_ev, while b_open) before anything but hg_map_begin / hg_map_end is enqueued (use()).
    StepBufs ws_b;
    hipStream_t stream_b = nullptr;
    hipEvent_t ev_pre = nullptr, ev_fork = nullptr, b_ev = nullptr;
    bool pre_valid = false, b_open = false;
    bool swapped = false;      // ws_b and stream_b are swapped in (a slot-1 step is being enqueued)
    i64 map_overlapped = 0;    // stat "map_overlapped_steps": blind steps enqueued on stream_b
    void swap_step() {
        std::swap(static_cast<StepBufs&>(*this), ws_b);
        std::swap(stream, stream_b);
        swapped = !swapped;
    }
    unsigned long long map_warm_cfg = 0, map_warm_epoch = 0;   // configuration of the last synchronous hg_map that won its bet outright
    i64 map_warm_R = -1;
    i64 map_async_steps = 0, map_async_redone = 0;
    unsigned long long q_gen = 0, db_gen = 0;      // bumped by every (re)load of the query / database tables
    i64 handicap_next = 0;     // test hook "handicap_next_bet": the NEXT bet's guess sits this many deviations BELOW the expected count (it loses), once
    i64 real_far_cursors = 0;  // test hook "real_far_cursors": 1 = k_real_select_bf keeps its 64-bit cursors (FAR) at any size, not only when a wavefront's record rows span 4 GB
    // hg_set_queries stages the packed tables through two alternating pinned blocks and does not wait for the stream: a new batch
    // can be handed over while a step on the previous one is still in flight (hg_map_begin / hg_map_end, batch after batch)
    struct QStage { void* pin = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; } qstage[2];
    int qstage_next = 0;
    bool ap_staged = false;
    bool ranked_local = false; // mbits holds this shard's bitmap in LOCAL rank order (hg_select_ranked)
    // the three row sources of the real-valued ranking: hg_topr_real / hg_map_real run on the first, hg_topr_asym / hg_map_asym on the second,
    // hg_topr_pq / hg_map_pq on the third
    RowSource from_floats{RowSource::FLOATS}, from_codes{RowSource::CODES}, from_pq{RowSource::PQ};
    void forget_rows() { from_floats.forget_derived(); from_codes.forget_derived(); from_pq.forget_derived(); }
    i64 asym_calls = 0;        // stat "asym_calls": asymmetric calls that succeeded (cumulative)
    i64 pq_calls = 0;          // stat "pq_calls": quantised calls that succeeded (cumulative)
    i64 pq_encode_calls = 0, pq_encoded_rows = 0;   // stats "pq_encode_calls" / "pq_encoded_rows": encoder calls that succeeded, the rows they encoded (cumulative)
    i64 real_requeried = 0;       // queries that lost the first real-valued bet and were ranked again on their own (cumulative)
    int bpad = 0;              // feature count padded to a multiple of 16 (0: no float tables loaded)
    i64 census_db[3] = {0, 0, 0}, census_q[3] = {0, 0, 0};
    // hand-over of float32 / int64 arrays (options host_pack, keep_floats)
    hipStream_t stream2 = nullptr;   // the float table's uploads while the packing pool works (pack_on_host)
    hipEvent_t stream2_ev = nullptr;
    size_t fstage_cap = 0;
    void* fstage = nullptr;    // 4 x 16 MB of pinned staging for float tables on their way to the GPU (pack_on_host)
    hipEvent_t fstage_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void* hpk = nullptr;       // pinned staging for the packed tables
    size_t hpk_cap = 0;
    bool qf_resident = false;  // the query float table as loaded is on the GPU (the database's: from_floats.rows_valid)
    RealState real;            // what the last attempt of a real-valued ranking left behind
    bool real_lists = false;   // hg_get_topr_real may hand out out_idx / scores: cleared where run_real begins, set once its ladder has succeeded
    i64 shapes_for_R = -1;
    i64 recip_for_R = -1;      // ap_recip holds RN(1 / k) for k = 1 .. this

    // collectives (RCCL over xGMI), one communicator per context
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;

    // device buffers beyond the step's (StepBufs)
    DevBuf db, dblab, qc, qlab;                 // the packed tables: database codes and label words, query codes and label words
    DevBuf qf;                                  // the queries' float table (hg_set_queries_f32 with the floats kept; the database's: from_floats.rows)
    DevBuf dbx, qx;            // fp4 images of db / qc in MFMA fragment order for k_select_mx (dbx_valid, qx_valid)
    DevBuf dbx8;               // i8 image of the database codes in A-fragment order (k_hist_i8; dbx8_valid)
    DevBuf rh_part, rh_all, rh_rel;   // hg_rel_hist: per-segment counters [S][2 NB][Qpad], the tables all / rel [NB][Qpad] (rh)
    DevBuf gr_tab, gr_out, gr_grades;   // hg_graded: [ks 64 x i64][gain C + 1][disc kmax], the tables gsum / hits / dcg / wsum [Q][nk] each, grade bytes [Q][R]
    DevBuf gh_part, gh_tab;    // hg_grade_hist: per-segment counters [S][C + 1][Qpad], the table [C + 1][Qpad] (gh)
    DevBuf jh_max, jh_part, jh_tab;   // hg_joint_hist: {most labels on a query, on a database row}, per-segment counters [S][NB * G][Qpad], the table [NB * G][Qpad] (jh)
    DevBuf ta_tab, ta_out;     // hg_tie_ap: the cut-offs [64 x i64], the tables ap_exp / p_hit / ap_min / ap_max / rel_exp / rel_lo / rel_hi [Q][nR] each (ta)
    DevBuf aa_tab, aa_out;     // hg_ap_at: [cut-offs 64 x i64][ApShape x (1 + nR)], the tables ap [Q][nR] x 8 and rel [Q][nR] x 4 (aa)
    DevBuf vt_tab, vt_votes, vt_pred, vt_conf;   // hg_votes: the cut-offs [64 x i64], votes [Q][nk][C] x 4, pred [Q][nk] x 4 then top [Q][nk] x 4, conf [nk][C][C] x 8 (vt)
    DevBuf mg_pack, mg_flag;   // hg_pack_side_table's block in the exchange layout (one at a time: the next pack overwrites it); hg_merge_side_table's two flag words
    DevBuf mg_rel, mg_grade, mg_joint;   // the merged tables (mrh, mgh, mjh)
    DevBuf lm_pack, lm_flag, lm_tab;   // hg_pack_list_table's block in the exchange layout (one at a time: the next pack overwrites it); hg_merge_list_table's four flag words; the cut-offs [64 x i64] of the vote pack / merge
    DevBuf lm_grades, lm_votes;   // the merged grade plane and vote counts (mlg, mlv)
    DevBuf nb_ids, nb_cnt, nb_flag, nb_stage;   // neighbour sets: sorted ids [Q][G] (pads at the end), valid ids [Q], k_nbr_sort's flag word, the caller's table on its way to the sort
    DevBuf nh_tab;             // hg_nbr_hist: the table [NB][Qpad] (nh)
    DevBuf aa_recip;           // hg_ap_at's own reciprocals (aa_recip_n) when the ranking's table (ap_recip, recip_for_R) is not there
    DevBuf rr_recs, rr_tmp;    // re-rank: a chunk's records (row index, then the sort key), the radix passes' second buffer (groups beyond the LDS only)
    DevBuf rr_base, rr_msz, rr_cnt, rr_scores;   // re-rank: a query's first record in its chunk [Q] x 8, records per query [Q] x 4, {groups in LDS, groups by radix}, the score lists [Q][R]
    DevBuf dbx3;               // fp4 image for k_select_mx3 (48-row supertiles, three rows per accumulator; dbx3_valid)
    DevBuf dbx4;               // fp4 image for k_select_mx4 (32-row supertiles, two rows per accumulator; codes of 65..128 bits; dbx4_valid)
    DevBuf shapes, ap_recip;   // k_ap's summation trees (shapes_for_R) and reciprocals (recip_for_R)
    DevBuf seglt, segtie;
    DevBuf mbits2;             // hg_merge_ranked's output (swapped with mbits)
    DevBuf part;               // hg_merge_ap_part's output: {AP, hits} of this rank's queries + its verdict
    DevBuf obuf[2];            // owner-routed exchanges: [0] the blocks this rank sends (hg_pack_*_by_owner), [1] its answers as an owner (hg_guess_owned)
    DevBuf beyond;             // one word: hg_guess_finish met a query whose cut lies beyond the planes its owner was sent
    DevBuf stage_in, badcnt;   // pack_on_device: the raw labels, the census counters
    DevBuf flist;              // the lost queries a requery child reruns
    DevBuf dbytes;             // the byte matrix D[q][Npad] of the dense regime (k_dense_bytes)
    DevBuf samp, thr, sortA, sortB, scores, gtab;   // real-valued path
    DevBuf sampx;              // float features of the sampled rows in MFMA A-fragment order (k_real_sample_mx), rebuilt per call
    DevBuf cntq;               // real-valued path: the slices' record counts after the rescore, query-major [Q][S] (k_real_rank_lds reads a query's row in one piece)
    DevBuf krows;              // real-valued path: the rows the filter kept, 4-byte row numbers [Q][S][cap] (k_real_select_bf writes, k_real_rescore reads)
    DevBuf thr2;               // filter + rescore path: lowered cuts
    DevBuf hist2;              // the second sample's counts [Q][RC_BINS] (k_real_sample_count)
    DevBuf pqe_in, pqe_books, pqe_books64, pqe_codes, pqe_err;   // the PQ encoder (hg_pq_encode.hip): a chunk of host features f32 [chunk][b], the codebooks f32 and f64 [M][K][dsub], a chunk's codes u8 [chunk][M] and errors f64 [chunk]
    DevBuf gathered[4], scratch[4], comm_tmp, gath_idx, gath_dist;   // hg_allgather's landing zones, hg_scratch, the collectives' own

    // Every device buffer of the context, each once, with its class: hg_destroy, hg_trim and the stat "device_bytes" walk this.
    template <class F> void for_each_buf(F&& f) {
        for (DevBuf* d : {&db, &dblab, &qc, &qlab, &from_floats.rows, &qf, &from_pq.pq_codes, &from_pq.pq_books}) f(*d, BUF_TABLE);
        for (DevBuf* d : {&dbx, &qx, &dbx8, &dbx3, &dbx4, &shapes, &ap_recip, &aa_recip}) f(*d, BUF_DERIVED);
        for (RowSource* s : {&from_floats, &from_codes, &from_pq}) for (DevBuf* d : {&s->rowsx, &s->img, &s->xmax2}) f(*d, BUF_DERIVED);
        f(from_codes.rows, BUF_WORK);
        f(from_pq.rows, BUF_WORK);
        for (DevBuf* d : {&seglt, &segtie, &mbits2, &part, &obuf[0], &obuf[1], &beyond, &stage_in, &badcnt, &flist, &dbytes, &samp, &thr,
                          &sortA, &sortB, &scores, &gtab, &sampx, &cntq, &krows, &thr2, &hist2, &comm_tmp, &gath_idx, &gath_dist, &rh_part, &rh_all, &rh_rel,
                          &gr_tab, &gr_out, &gr_grades, &gh_part, &gh_tab, &ta_tab, &ta_out, &aa_tab, &aa_out, &jh_max, &jh_part, &jh_tab, &vt_tab, &vt_votes, &vt_pred, &vt_conf,
                          &mg_pack, &mg_flag, &mg_rel, &mg_grade, &mg_joint, &lm_pack, &lm_flag, &lm_tab, &lm_grades, &lm_votes, &rr_recs, &rr_tmp, &rr_base, &rr_msz, &rr_cnt, &rr_scores,
                          &nb_ids, &nb_cnt, &nb_flag, &nb_stage, &nh_tab, &pqe_in, &pqe_books, &pqe_books64, &pqe_codes, &pqe_err})
            f(*d, BUF_WORK);
        for (DevBuf& d : gathered) f(d, BUF_WORK);
        for (DevBuf& d : scratch) f(d, BUF_WORK);
        for_each_step_buf(f);
        ws_b.for_each_step_buf(f);
    }
    // the keys of the BUF_DERIVED buffers: after this each is rebuilt on its next use
    void forget_derived() {
        dbx_valid = qx_valid = dbx8_valid = dbx3_valid = dbx4_valid = false;
        forget_rows();
        for (SideResult* r : {&rh, &gr, &gh, &ta, &aa, &jh, &vt, &mrh, &mgh, &mjh, &mlg, &mlv, &rr, &nb, &nh}) r->begin();   // (hg_trim releases their tables with the other work buffers)
        shapes_for_R = recip_for_R = aa_recip_n = -1;
        outblk_q = ws_b.outblk_q = -1;
    }

    // one-shot step as a hipGraph: the bet's whole sequence (memsets, ~7 kernels, the result download) is captured the
    // second time hg_map sees the same problem and replayed afterwards -- one launch per step instead of ~15 enqueues,
    // so the step time no longer depends on how fast the host can feed the stream
    struct StepGraph {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        unsigned long long epoch = 0, cfg = 0, seen_epoch = 0, seen_cfg = 0;   // key of exec / of the last eager step
        i64 R = -1, seen_R = -1;
        int timing = -1, seen_timing = -1;
        StepState left;                    // what the captured enqueue left behind on the host
        std::vector<Pending> evs;          // event-record nodes inside the graph (kernel timing)
    } sg;
    unsigned long long cfg_epoch = 1;      // bumped by everything that changes what a step enqueues (tables, options, stream)
    bool capturing = false;
    i64 graph_replays = 0, graph_captures = 0;

    // timing
    int timing = 0;            // 0 off, 1 the pair passes only (hist, select), 2 every kernel
    double t_ms[KI_COUNT] = {0};
    i64 t_n[KI_COUNT] = {0};
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;

    // every entry point but hg_map_begin / hg_map_end: whatever it enqueues on the context's stream follows stream_b's work
    int use() {
        HG_HIP(hipSetDevice(device));
        pre_valid = false;
        if (b_open) { HG_HIP(hipStreamWaitEvent(stream, b_ev, 0)); b_open = false; }
        return HG_OK;
    }

    hipEvent_t get_event() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)host_timed(HP_EVENT, [&] { return hipEventCreate(&e); });
        return e;
    }
    bool t_wanted(int id) const {
        // 1: the select pass (the roofline kernel) and the step's span only -- every event pair costs the stream ~2-4 us
        // and only on one step in "timing_every" (the averages are over the sampled launches)
        return timing >= 2 || (timing == 1 && (id == KI_SELECT || id == KI_SELECT_MX || id == KI_STEP) &&
                               (capturing || opt.timing_every <= 1 || t_seq % opt.timing_every == 0));
    }
    i64 t_seq = 0;             // one-shot steps since timing was enabled
    // while a step is being captured the events become event-record nodes of the graph and stay with it
    std::vector<Pending>& t_list() { return capturing ? sg.evs : pending; }
    bool t_open = false;
    void t_begin(int id) {
        t_open = t_wanted(id);
        if (!t_open) return;
        Pending p{id, get_event(), get_event()};
        (void)hipEventRecord(p.a, stream);
        t_list().push_back(p);
    }
    void t_end() {
        if (!t_open) return;
        t_open = false;
        (void)hipEventRecord(t_list().back().b, stream);
    }
    // the whole step's span on the GPU (first enqueue to the last byte of the download): nests around the kernels' pairs
    int step_slot = -1;
    void t_step_begin() {
        step_slot = -1;
        ++t_seq;
        if (!t_wanted(KI_STEP)) return;
        Pending p{KI_STEP, get_event(), get_event()};
        (void)hipEventRecord(p.a, stream);
        step_slot = (int)t_list().size();
        t_list().push_back(p);
    }
    void t_step_end() {
        if (step_slot < 0) return;
        (void)hipEventRecord(t_list()[step_slot].b, stream);
        step_slot = -1;
    }
    void t_collect_graph() {   // after a replay has completed
        for (auto& p : sg.evs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { t_ms[p.id] += ms; t_n[p.id] += 1; }
        }
    }
    void drop_graph() {
        if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
        if (sg.graph) (void)hipGraphDestroy(sg.graph);
        sg.exec = nullptr; sg.graph = nullptr;
        for (auto& p : sg.evs) { pool.push_back(p.a); pool.push_back(p.b); }
        sg.evs.clear();
    }
    void t_collect() {   // after a stream sync
        for (auto& p : pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { t_ms[p.id] += ms; t_n[p.id] += 1; }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
    int sync() {
        HG_HIP(host_timed(HP_SYNC, [&] { return hipStreamSynchronize(stream); }));     // ("sync": waiting for the GPU -- kernels and copies included)
        if (b_open && !swapped) {                      // (stream_b's work that the context's stream has not waited for)
            HG_HIP(host_timed(HP_SYNC, [&] { return hipStreamSynchronize(stream_b); }));
            b_open = false;
        }
        if (pending.size() > 4096) t_collect();       // otherwise the elapsed times are read when somebody asks for them
        return HG_OK;
    }
    // end of a staged call that only enqueued work: synchronise unless the caller orders everything on
    // one stream itself (hg_set_stream + stage_sync = 0, e.g. torch's current stream in sharded mode)
    int stage_end() { return opt.stage_sync ? sync() : HG_OK; }
    int check_launch(const char* what) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(HG_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
        return HG_OK;
    }
};

inline void SideResult::finish(const hg_ctx* c, i64 Q_, i64 Qpad_, i64 dim_) { *this = SideResult{true, c->q_gen, c->db_gen, Q_, Qpad_, dim_}; }
inline bool SideResult::current(const hg_ctx* c) const { return done && q_gen == c->q_gen && db_gen == c->db_gen; }

// hg_map_begin enqueues blind only while no device buffer has moved since the hg_map that gave the licence (map_warm_epoch).  First
// reservations of buffers a blind step never touches (a side metric's tables, the second workspace) move none of those: take one
// of these before such a group and call keep() once all of it succeeded -- not on an early return.
struct FirstReservations {
    const unsigned long long e0 = g_alloc_epoch.load();
    void keep(hg_ctx* c) const { if (c->map_warm_epoch == e0) c->map_warm_epoch = g_alloc_epoch; }
};

// downloads on the context's stream (the caller synchronises): k equal planes into optional host pointers; a [rows][Qpad] table of
// 32-bit words without its padding.  And hit counts widened u32 -> int64.
inline int download_planes(hg_ctx* c, const DevBuf& src, size_t plane, void* const* host, int k) {
    for (int i = 0; i < k; ++i)
        if (host[i]) HG_HIP(hipMemcpyAsync(host[i], src.as<char>() + i * plane, plane, hipMemcpyDeviceToHost, c->stream));
    return HG_OK;
}
inline int download_pitched(hg_ctx* c, void* host, const DevBuf& src, i64 Q, i64 Qpad, i64 rows) {
    HG_HIP(hipMemcpy2DAsync(host, (size_t)Q * 4, src.p, (size_t)Qpad * 4, (size_t)Q * 4, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    return HG_OK;
}
inline void widen_u32(int64_t* dst, const void* src, size_t n) {
    for (size_t i = 0; i < n; ++i) dst[i] = ((const u32*)src)[i];
}

inline int grid_for(i64 n, int per_block = 256) { return (int)((n + per_block - 1) / per_block); }
inline int padded_grid(int nBlk) { return (nBlk + 7) / 8 * 8; }
inline int pad16(int b) { return (b + 15) / 16 * 16; }   // a float table's row pitch: the feature count padded to a multiple of 16 (hg_ctx::bpad)

// ---- across translation units --------------------------------------------------------------------------------------
// hg_core.hip
int need(hg_ctx* c, unsigned st, const char* who, const char* what);     // stage check + hipSetDevice
int ensure_pin(hg_ctx* c, size_t need_b);
int do_match(hg_ctx* c);                         // k_match through the ranked idx list (> 128 classes, real-valued lists)
int ensure_ap_tables(hg_ctx* c, bool* use_recip);   // summation trees + reciprocals for the current R, c->ap / c->rel sized
int do_ap_range(hg_ctx* c, i64 q0, i64 nq, const u32* only = nullptr);      // k_ap on queries [q0, q0 + nq) (only: device flags [Q], just the flagged ones)
inline int do_ap(hg_ctx* c) { return do_ap_range(c, 0, c->geo.Q); }
int ensure_out_block(hg_ctx* c);                   // err / ap / rel as views of one block (before anything of the call is enqueued)
int read_plan_flag(hg_ctx* c, int* flag);        // *err back to the host (synchronises)
int launch_min_topr(hg_ctx* c, const u32* idx_all, const u8* dist_all, i64 n, int G);
hg_ctx* requery_child(hg_ctx* c, i64 nF);       // c->sub, set up to rerun nF lost queries of c
// hg_tables.hip
extern "C" int check_dev_pointer(hg_ctx* c, const char* who, const char* what, const hg_dev_array& a, int64_t extent);   // a.ptr is device memory of the context's GPU and the extent lies inside its allocation (else HG_ERR_ARG)
extern "C" int wait_for_producer(hg_ctx* c, void* s);   // (both defined among the device-array entry points)  the context's stream behind whatever is enqueued so far on the producer's stream s
int preload_tables(hg_ctx* c);                   // hg_preload: the loaders' staging blocks, second stream and packing threads; the unit's code object
// hg_seq.hip
int stage_ap_download(hg_ctx* c, void* dst = nullptr);   // {verdict, AP, hit counts} into pinned host memory behind everything enqueued so far (no synchronisation)
int wait_verdict(hg_ctx* c, bool staged, int* flag);     // waits for the stream; the verdict word from the context's pinned block (staged) or by a download of its own
Geo full_geometry(const hg_ctx* c);               // the full pass's segment geometry for the tables and options held now
inline void make_geometry(hg_ctx* c) { c->geo = full_geometry(c); }
Geo hist_geometry(const hg_ctx* c);
int set_R(hg_ctx* c, int64_t R, int G, int rank);
int rerank_hist_plan(hg_ctx* c, int64_t R);       // full per-segment histogram (k_hist) + k_plan on one shard: c->hist, c->hown, c->t, c->cnt_lt, c->posbase
// hg_rank.hip
int launch_rank(hg_ctx* c, RankMode mode, const StepReq& req);   // the rank stage on the rows the step left: chooses the kernel, runs it, sets last_rank / ap_fused
int launch_rank_leftovers(hg_ctx* c);            // k_rank_fused on the queries a fused step's rank kernel flagged in bigq (finish_leftovers)
int launch_order(hg_ctx* c);                     // k_order: placement of an exact sequence on several shards
bool rank_dense_fits(const hg_ctx* c);           // the byte matrix (k_dense_bytes + k_rank_dense) takes these tables
inline bool lists_needed(const hg_ctx* c) { return c->want_lists || c->LW > 2; }   // the ranked idx / dist lists are written: somebody asked for them, or k_match gathers the labels through them (> 128 classes)
inline const int* cut_of(const hg_ctx* c, const StepReq& req) { return req.exact_cut ? c->t.as<int>() : c->tguess.as<int>(); }
// hg_pairs_valu.hip
int launch_hist(hg_ctx* c);                      // k_hist<NW>
int launch_hist_rel(hg_ctx* c, const Geo& g);    // k_hist_rel<NW, LW> into c->rh_part (g: full_geometry)
int launch_select_valu(hg_ctx* c, int lw, bool optimistic);   // k_select<NW, LW, OPT>
int launch_select_dense(hg_ctx* c, int lw);      // k_select_dense<NW, LW>
// hg_pairs_mx.hip (k_select_mx: hg_pairs_mx1.hip)
int ensure_mx_images(hg_ctx* c, bool need_db);  // fp4 images of database / query codes, built on first use
int launch_hist_mx(hg_ctx* c, u64* tot = nullptr);   // k_hist_i8 / k_hist_mx; tot: k_hist_i8 adds its planes into this table too (StepBufs::hist_tot)
bool hist_i8_applies(const hg_ctx* c);           // launch_hist_mx takes k_hist_i8
// (cut: each query's threshold -- c->tguess, or c->t for StepReq::exact_cut)
int launch_select_mx(hg_ctx* c, int lw, const int* cut);    // k_select_mx<NW, LW, QT, COMPACT>
int launch_select_mx3(hg_ctx* c, int lw, const int* cut);   // k_select_mx3 (codes of <= 64 bits, one-byte records)
int launch_select_mx4(hg_ctx* c, int lw, const int* cut);   // k_select_mx4 (codes of 65..128 bits, one-byte records)
int preload_valu(); int preload_mx(); int preload_mx1(); int preload_real(); int preload_seq(); int preload_rank(); int preload_side(); int preload_rerank(); int preload_pq_encode();   // one per translation unit with kernels (hg_preload)
// hg_comm.hip
void comm_release(hg_ctx* c);                    // destroys the context's communicator, if any

#define HG_DISPATCH_NW(fn, c, ...)                              \
    switch ((c)->NW) {                                          \
        case 1: return fn<1>(c, ##__VA_ARGS__);                 \
        case 2: return fn<2>(c, ##__VA_ARGS__);                 \
        case 3: return fn<3>(c, ##__VA_ARGS__);                 \
        case 4: return fn<4>(c, ##__VA_ARGS__);                 \
        case 5: return fn<5>(c, ##__VA_ARGS__);                 \
        case 6: return fn<6>(c, ##__VA_ARGS__);                 \
        case 7: return fn<7>(c, ##__VA_ARGS__);                 \
        case 8: return fn<8>(c, ##__VA_ARGS__);                 \
        default: return fail(HG_ERR_ARG, "unsupported code length: %d words", (c)->NW); \
    }

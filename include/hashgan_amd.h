/*
 * hashgan_amd -- C ABI of the MI355X-native retrieval-evaluation path.
 *
 * The reference has no FFI: its boundary for this path is the Python call
 *     MAPs(R).get_maps_by_feature(database, query)      lib/metric.py:4-24
 * made from evaluate()                                   main.py:161-164.
 * hashgan_amd/metric.py keeps that call surface; everything below is what that
 * Python binds through ctypes.  Conventions:
 *   - extern "C", plain pointers and sizes, no C++/torch types;
 *   - every function returns 0 (HG_OK) or a negative HG_ERR_* code and never
 *     throws; hg_last_error() gives the message of the calling thread's last
 *     failure;
 *   - "host" pointers are caller-owned host memory, "dev" pointers are device
 *     addresses (hipMalloc'ed by the caller or by torch) on the context's GPU;
 *   - a context owns one GPU stream; every call is complete (stream
 *     synchronised) when it returns; a context is not thread safe.
 *
 * Data layout (pinned by tests/test_capi.py::test_pack_sign_matches_python_packing and
 * tests/test_oracle_golden.py::test_pack_bits_layout):
 *   codes   uint64 [n][W], W = ceil(b/64); bit j of a code is bit (j % 64) of
 *           word j / 64; bit value = (feature[j] > 0); pad bits are zero.
 *   labels  uint64 [n][LW], LW = ceil(C/64), bit c set <=> label[c] != 0.
 *   ranked lists: position k of query q is element [q*R + k].
 *
 * Canonical order: Hamming distance ascending, then database
 * index ascending -- what np.argsort(-ips, 1) (metric.py:14) yields for +-1
 * codes once ties are broken by index.
 */
#ifndef HASHGAN_AMD_H
#define HASHGAN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_OK 0
#define HG_ERR_ARG (-1)    /* bad argument (R > N, b out of range, null pointer ...) */
#define HG_ERR_HIP (-2)    /* a HIP runtime call or kernel failed */
#define HG_ERR_STATE (-3)  /* call sequence violated (e.g. hg_select before hg_plan) */
#define HG_ERR_NOMEM (-4)  /* device allocation failed */

#define HG_MAX_BITS 255        /* longest supported code: a Hamming distance has to fit the 8 bits it gets in
                                  the records and in the ranked lists (two 256-bit codes can be 256 apart) */
#define HG_IDX_NONE 0xFFFFFFFFu /* ranked-list slot owned by another shard */

typedef struct hg_ctx hg_ctx;

const char* hg_last_error(void);
int hg_version(void);
int hg_device_count(int* count);

/* One context per (process, GPU).  Replaces nothing in the reference (it runs
 * the metric on the host); it is the handle the Python MAPs object keeps. */
int hg_init(int device, hg_ctx** out);
int hg_destroy(hg_ctx* ctx);

/* Binarise-and-pack, host side: bit j = (x[i*b + j] > 0).  This is the sign()
 * the reference never applies (its tanh features go straight into np.dot,
 * lib/architecture.py:147 -> metric.py:13); for +-1 features it is exact. */
int hg_pack_sign_f32(const float* host_x, int64_t n, int b, uint64_t* host_out);

/* database.output / database.label of metric.py:13,19 as packed codes/labels.
 * idx_base is the global index of this shard's row 0, n_total the size of the
 * whole (all-shard) database; single GPU: idx_base = 0, n_total = N. */
int hg_set_database(hg_ctx* ctx, const uint64_t* host_codes, const uint64_t* host_labels,
                    int64_t N, int b, int C, int64_t idx_base, int64_t n_total);
/* query.output / query.label of metric.py:13,17. Same b and C as the database. */
int hg_set_queries(hg_ctx* ctx, const uint64_t* host_codes, const uint64_t* host_labels, int64_t Q);

/* The same two calls fed with what forward_all() (main.py:151-158) actually returns: float32
 * features [n][b] and int64 labels [n][C].  Binarise (bit = x > 0) and pack run on a pool of host threads BEFORE the
 * upload (16 MB instead of 339 MB cross PCIe at C2; option "host_pack" = 0: upload raw, pack on the GPU).  The float
 * table itself follows only if it will be ranked by inner product: option "keep_floats" = 2 (default) uploads it iff the
 * database is not a +-1 code, 1 always, 0 never; the queries' floats follow the database's.
 * *bad_codes counts feature entries outside {-1, 0, +1}, *bad_labels label entries outside
 * {0, 1}: the caller decides what non-binary features mean (the Python mirror ranks them by inner product
 * like metric.py:13-14 unless binarize=True); hg_get_census has the finer census (zeros, minus ones). */
int hg_set_database_f32(hg_ctx* ctx, const float* host_features, const int64_t* host_labels, int64_t N, int b, int C,
                        int64_t idx_base, int64_t n_total, int64_t* bad_codes, int64_t* bad_labels);
int hg_set_queries_f32(hg_ctx* ctx, const float* host_features, const int64_t* host_labels, int64_t Q,
                       int64_t* bad_codes, int64_t* bad_labels);
/* The same two calls for a caller whose features never left the GPU (forward_all() runs on the device the metric runs on):
 * a 2-D array in DEVICE memory, described as the caller's framework laid it out -- any row / column stride (a slice, a
 * transposed view), float32 / IEEE float16 / bfloat16 features, int64 / int32 / uint8 (bool) / float32 labels; no alignment is
 * assumed.  One kernel (k_pack_dev, hg_dev_in.hpp) reads the caller's memory once and writes the packed code words, the census and
 * -- where "keep_floats" asks for it -- the float32 table; 16-bit features are widened exactly first.  With "keep_floats" = 2 the
 * census decides, so the floats of a table that is not a +-1 code are written by a second pass over the caller's memory.
 * Afterwards the context holds exactly what hg_set_*_f32 leaves for the same values ("host_pack" plays no part).
 *   Ordering  the context's stream waits for everything enqueued so far on features->stream and labels->stream (an event on each), so
 *             the producer need not synchronise; stream = NULL is the null stream -- work queued on a non-blocking stream of the
 *             caller's is only ordered if that stream's handle is passed.
 *   Copy-in   the call is complete when it returns: the caller may overwrite or free its arrays, no pointer to them is kept.
 *   Refused   with HG_ERR_ARG before anything is launched: a dtype outside the lists above, a stride < 1, unequal row counts, the
 *             shape limits of hg_set_*_f32, a pointer that hipPointerGetAttributes does not report as device memory (host, managed,
 *             unknown) of the context's device, an extent -- ptr .. ptr + ((rows-1)*row_stride + (cols-1)*col_stride + 1) * itemsize
 *             -- that does not lie inside the allocation hipMemGetAddressRange reports.
 * A label entry counts as bad unless it is exactly 0 or 1 (0.5 and NaN in float32 labels are bad).  HG_F64 is a dtype of
 * hg_export's destinations only: both loaders refuse it like any dtype outside their lists. */
#define HG_F32 0
#define HG_F16 1
#define HG_BF16 2
#define HG_I64 3
#define HG_I32 4
#define HG_U8 5     /* also bool */
#define HG_F64 6                       /* accepted by hg_export only */
typedef struct hg_dev_array {      /* a 2-D array in device memory, as the caller's framework laid it out */
    const void* ptr;
    int64_t rows, cols;
    int64_t row_stride, col_stride;    /* strides in ELEMENTS, both >= 1 */
    int dtype;                         /* HG_F32, HG_F16, HG_BF16 (features); HG_I64, HG_I32, HG_U8, HG_F32 (labels); hg_export: see HG_OUT_* */
    void* stream;                      /* producer's hipStream_t (hg_export: the consumer's); NULL = the null stream */
} hg_dev_array;
int hg_set_database_dev(hg_ctx* ctx, const hg_dev_array* features, const hg_dev_array* labels,
                        int64_t idx_base, int64_t n_total, int64_t* bad_codes, int64_t* bad_labels);
int hg_set_queries_dev(hg_ctx* ctx, const hg_dev_array* features, const hg_dev_array* labels,
                       int64_t* bad_codes, int64_t* bad_labels);
/* Packed device tables back to the host: which = 0 database, 1 queries; codes as dense
 * uint32 [n][ceil(b/32)], labels uint64 [n][ceil(C/64)]. */
int hg_get_packed(hg_ctx* ctx, int which, uint32_t* host_codes, uint64_t* host_labels);

/* ---- staged pipeline (what multi-GPU orchestration drives) ------------------
 * hg_hist    metric.py:13   XOR+popcount of every (query, db row) pair, reduced
 *                           to per-query distance histograms of this shard.
 * hg_plan    metric.py:14   per query: threshold distance t (the R-th smallest
 *                           over ALL shards), tie quota, output offsets.
 *                           dev_hist_all = G shard histograms, each laid out as
 *                           hg_hist_buffer describes, shard-rank order; pass
 *                           NULL, G = 1, rank = 0 on a single GPU.
 * hg_select  metric.py:14 + [0:R] at :19   second pass over the pairs: emits the
 *                           shard's members of the global top-R into their
 *                           global rank positions, canonical order, together
 *                           with their label-match bits (metric.py:17-19).
 * hg_match   metric.py:17-19  label match -> bit rows.  Already done by
 *                           hg_select for C <= 128 classes (then a no-op);
 *                           a gather pass over the ranked lists otherwise.
 * hg_merge_match            OR of G shards' bit rows (after an all-gather).
 * hg_ap      metric.py:20-23  per-query AP in float64, same rounding and
 *                           summation order as NumPy (pairwise, 8192 chunks).
 */
int hg_hist(hg_ctx* ctx);
/* The exchange unit of every histogram stage: uint32 [b+1][Qpad] followed by 64 tail words
 * ([0] "a slice overflowed" flag, [1] rows the pass visited). */
int hg_hist_buffer(hg_ctx* ctx, void** dev_ptr, int64_t* nbytes);
/* The relevant-row histogram of this shard, for hash-lookup metrics (precision / recall as functions of the Hamming radius): one
 * pass over the pairs counts, per query and distance d, the rows at distance d (all) and those of them that share a label with
 * the query (rel) -- no ranking, no lists.  Tables of its own: the staged pipeline's state (hg_hist's histogram, a plan, a step
 * of hg_map_begin in flight) is left as it was.  Additive over shards; a database or query reload invalidates the tables. */
int hg_rel_hist(hg_ctx* ctx);                                            /* needs database + queries */
/* The grade histogram of this shard, for graded relevance on multi-label data (grade = labels a row shares with the query): one pass
 * over the query x database label pairs -- no codes, no ranking -- counts, per query and grade g = 0..C, the rows with that grade.
 * The ideal ordering NDCG divides by is "the database sorted by grade", so IDCG at any k follows from this table.  C <= 255
 * (HG_ERR_ARG beyond).  Same rules as hg_rel_hist: a table of its own, the staged pipeline's state and a step of hg_map_begin in
 * flight are left as they were; additive over shards; a database or query reload invalidates it; hg_trim frees it. */
int hg_grade_hist(hg_ctx* ctx);                                          /* needs database + queries */
/* The distance-by-grade histogram of this shard, for tie-aware graded metrics (expected DCG / NDCG / ACG at k over the orders inside
 * the Hamming tie groups, and their exact extremes): one pass over the pairs counts, per query, distance d = 0..b and grade g = 0..G-1,
 * the rows at distance d that share exactly g labels with the query -- no ranking, no lists.  hg_rel_hist's tables are this one collapsed
 * to g = 0 / g > 0, hg_grade_hist's is this one summed over d.  G = 1 + min(most labels on a loaded query, most labels on a loaded
 * database row), an upper bound on any pair's grade, found on the device first (stat "joint_hist_grades"; the call synchronises once
 * for it whatever "stage_sync" says).  When (b+1) * G > 640 a wavefront's counters outgrow the LDS and the distances are served in
 * bands of 640 / G (stat "joint_hist_bands"); the table is the same for any band count.  C <= 255 (HG_ERR_ARG beyond), b up to
 * HG_MAX_BITS.  Same rules as hg_rel_hist: tables of its own, the staged pipeline's state, the other side metrics' results and a step
 * of hg_map_begin in flight are left as they were; additive over shards (zero-pad to a common G; idx_base plays no part); a database
 * or query reload invalidates it; hg_trim frees it. */
int hg_joint_hist(hg_ctx* ctx);                                          /* needs database + queries */
int hg_plan(hg_ctx* ctx, int64_t R, const uint32_t* dev_hist_all, int G, int rank);
int hg_select(hg_ctx* ctx);
int hg_match(hg_ctx* ctx);
int hg_match_buffer(hg_ctx* ctx, void** dev_ptr, int64_t* nbytes); /* uint64 [Q][ceil(R/64)] */
int hg_merge_match(hg_ctx* ctx, const uint64_t* dev_bits_all, int G);
int hg_ap(hg_ctx* ctx);

/* ---- staged optimistic sequence (R << N): one pass over the pairs instead of two ----
 * hg_bet_eligible      same verdict on every rank (uses only R, n_total, world, options)
 * hg_sample_hist       histogram of every k-th row batch            -> hg_hist_buffer -> all-gather
 * hg_guess             threshold guess from the G sample histograms ("guess_sigma" = 5 standard deviations high)
 * hg_select_candidates ONE pass over the pairs: superset of the members as records, plus the
 *                      exact histogram of those records              -> hg_hist_buffer -> all-gather
 * hg_rank              exact plan from the G record histograms + ordering + match bits.
 *                      *bet_lost = 1 (on every rank alike) when the superset was short of R rows
 *                      or a slice overflowed anywhere: run hg_hist/hg_plan/hg_select instead. */
int hg_bet_eligible(hg_ctx* ctx, int64_t R, int world, int* eligible);
int hg_sample_hist(hg_ctx* ctx, int64_t R);
int hg_guess(hg_ctx* ctx, int64_t R, const uint32_t* dev_hist_all, int G, int rank);
int hg_select_candidates(hg_ctx* ctx);
int hg_rank(hg_ctx* ctx, const uint32_t* dev_hist_all, int G, int rank, int* bet_lost);
/* With option "defer_verdict" = 1 hg_rank does not wait for the verdict (*bet_lost = -1): the caller carries on as
 * if the bet held -- match bits, their exchange, hg_ap -- and asks here once, next to its final download; on
 * *bet_lost = 1 it discards those results and runs the exact sequence.  Removes the only host round trip from
 * the middle of a sharded step. */
int hg_bet_verdict(hg_ctx* ctx, int* bet_lost);
/* The bet with ONE record pass and ONE exchange after the guess (AP only, no ranked lists):
 * hg_select_ranked   select with the shared guess, then rank this shard's own records.  Leaves the shard's
 *                    per-distance record counts in hg_hist_buffer and its match bitmap in LOCAL rank order
 *                    (metric.py:14,17-19 restricted to the shard) in hg_match_buffer -> all-gather both
 * hg_merge_ranked    shards own contiguous index ranges, so the global order is, per distance, shard 0's rows,
 *                    then shard 1's, ...: derives the cut from the gathered counts (metric.py:19's [0:R]) and
 *                    stitches the global match bitmap from bit ranges of the local ones; then hg_ap.
 *                    *bet_lost as in hg_rank (-1 with "defer_verdict"); G <= 64. */
int hg_select_ranked(hg_ctx* ctx);
int hg_merge_ranked(hg_ctx* ctx, const uint32_t* dev_hist_all, const uint64_t* dev_bits_all, int G, int* bet_lost);
/* The same with the per-query stages split over the ranks (hashgan_amd/sharded.py::evaluate_shard): after the all-gather
 * of record counts and local bitmaps, rank r merges and evaluates (k_merge_ranked + k_ap) only its own contiguous share
 * [q0, q0 + nq) of the queries instead of all Q on every rank.  Its results leave in one device buffer *dev_part of
 * (width + 1) pairs of doubles -- pair i < nq = {AP, hit count} of query q0 + i, pairs nq .. width - 1 zero, pair `width` =
 * {this rank's lost-bet flag, nq}; width >= nq is the same on every rank so that the parts can be all-gathered.
 * hg_unpack_parts takes the gathered G parts (rank order = query order), fills AP / hit counts of all Q queries on the host
 * and returns the bet's verdict (the OR of the ranks' flags: computed from gathered data, identical on every rank), doing
 * hg_bet_verdict's bookkeeping.  The reference has no counterpart (lib/metric.py:16-24 loops over all queries in one process). */
int hg_merge_ap_part(hg_ctx* ctx, const uint32_t* dev_hist_all, const uint64_t* dev_bits_all, int G, int64_t q0, int64_t nq,
                     int64_t width, void** dev_part, int64_t* nbytes);
int hg_unpack_parts(hg_ctx* ctx, const void* dev_parts_all, int G, int64_t width, double* host_ap, int64_t* host_rel, int* bet_lost);
/* The same sharded bet with its exchanges ROUTED BY QUERY OWNER (round 4).  The queries are split over the ranks like the
 * per-query stages above (contiguous, near-equal shares: rank o owns [q0(o), q0(o) + nq(o)), width = the largest share);
 * what a stage needs of a query it needs from every shard but only on the query's owner, so the tables travel by
 * all-to-all (hg_alltoall), one block per destination, instead of every rank receiving every query's rows of every
 * shard: at C4 on 8 GPUs 10.6 MB of ingress per GPU and step instead of 80 MB.  Results are those of the all-gather form
 * (and of one GPU) bit for bit.
 *   hg_sample_hist -> hg_pack_sample_by_owner   *dev_ptr = [G] blocks {rows sampled, counts [planes][width]}      -> all-to-all
 *   hg_guess_owned(dev_recv)                    the owner's guess of ITS queries; *dev_ptr = [G] answers [width][4 x u32]
 *                                               {T, sampled rows ahead of shard r's own, sample count to reach, found}  -> all-to-all
 *   hg_guess_finish(dev_answers)                the shared cut T + this shard's sstar for ALL queries; budget as hg_guess
 *   hg_select_ranked -> hg_pack_ranked_by_owner *dev_ptr = [G] blocks {record counts [b+1][width], tail, local bitmaps [width][RW]} -> all-to-all
 *   hg_merge_ap_owned(dev_recv)                 hg_merge_ap_part on the received blocks -> this rank's part -> hg_allgather -> hg_unpack_parts */
int hg_pack_sample_by_owner(hg_ctx* ctx, int G, void** dev_ptr, int64_t* nbytes_per_peer);
int hg_guess_owned(hg_ctx* ctx, int64_t R, const void* dev_recv, int G, int rank, void** dev_ptr, int64_t* nbytes_per_peer);
int hg_guess_finish(hg_ctx* ctx, int64_t R, const void* dev_answers, int G, int rank);
int hg_pack_ranked_by_owner(hg_ctx* ctx, int G, void** dev_ptr, int64_t* nbytes_per_peer);
int hg_merge_ap_owned(hg_ctx* ctx, const void* dev_recv, int G, int rank, void** dev_part, int64_t* nbytes);

/* Ranked lists in global-position space: uint32 idx [Q][R] (HG_IDX_NONE where a
 * slot belongs to another shard), uint8 dist [Q][R] (0xFF there). */
int hg_topr_buffers(hg_ctx* ctx, void** dev_idx, void** dev_dist, int64_t* n_slots);
/* Element-wise merge of G shards' ranked lists after an all-gather (min picks
 * the one owner of every slot). dev_idx_all: [G][Q][R], dev_dist_all likewise. */
int hg_merge_topr(hg_ctx* ctx, const uint32_t* dev_idx_all, const uint8_t* dev_dist_all, int G);

/* ---- one-shot forms (single shard) --------------------------------------------
 * Every stage is enqueued back to back with one synchronisation.  When R << N
 * they replace the full histogram pass by a sampled one and a verified guess of
 * the threshold (identical results; falls back to the staged sequence if the
 * verification fails).  hg_map skips the idx/dist lists -- mAP only needs the
 * match bits; use hg_topr when the ranked lists themselves are wanted. */
int hg_topr(hg_ctx* ctx, int64_t R);
int hg_map(hg_ctx* ctx, int64_t R, double* host_ap, int64_t* host_rel);
/* hg_map in two halves, for a caller that evaluates batch after batch (lib/metric.py:4-24 once per batch of queries):
 * hg_map_begin enqueues a step -- its kernels and the download of verdict, APs and hit counts into a pinned block of its
 * own -- and returns; hg_map_end waits for the OLDEST step in flight and hands over what hg_map would have returned.  Up to
 * two steps may be in flight (a third hg_map_begin is HG_ERR_STATE), so the GPU starts one step the moment the previous one
 * ends.  A step is only enqueued blind when the last synchronous hg_map on the same tables, options and R won its bet
 * outright; otherwise hg_map_begin runs the whole call itself.  A blind step that loses its bet is run again by hg_map_end.
 * Replacing the tables between the two halves is allowed only for steps that won: hg_map_end on a LOST step whose query or database
 * table has been loaded again since its hg_map_begin (whatever the new table's size) returns HG_ERR_STATE -- never the new batch's
 * results under the old step's name.  A new query table of the SAME size on an unchanged database and configuration keeps the licence
 * to enqueue blind, and hg_set_queries does not wait for the stream (the tables travel through a pinned block of the context's own):
 * a caller that hands over batch after batch -- hg_set_queries, hg_map_begin, the previous batch's hg_map_end -- keeps two steps in
 * flight.  Option "step_streams" (2, the default): slot 1's blind steps run on a second stream of the context, in buffers of their
 * own, so two consecutive steps overlap on the GPU; every other entry point first orders the context's stream behind it, and
 * hg_synchronize waits for both (1: one stream).  Stats "map_async_steps" / "map_async_redone" / "map_overlapped_steps".  Test hook: option "handicap_next_bet" (0..64; not a configuration change)
 * puts the NEXT bet's guess that many deviations below the expected count, once: the bet loses. */
int hg_map_begin(hg_ctx* ctx, int64_t R);
int hg_map_end(hg_ctx* ctx, double* host_ap, int64_t* host_rel);

/* ---- real-valued features (what main.py feeds when nothing is binarised) ----
 * Ranking by float32 inner product, lib/metric.py:13-14 as written, on the float tables kept by
 * hg_set_database_f32 / hg_set_queries_f32 (up to 255 features; one context holds the whole table -- several GPUs split
 * the QUERIES, hashgan_amd/sharded.py::evaluate_real_queries).  Order: inner product descending,
 * database index ascending.  The product's summation order is fixed (one float32 fma chain in feature
 * order: what the chained v_mfma_f32_32x32x2_f32 computes) and restated exactly by oracle/real_map.py; it equals the reference's
 * np.dot wherever float32 rounding does not reorder near-equal products, exactly so on inputs
 * whose arithmetic is exact.  hg_map_real = ranking + label match + AP; hg_topr_real = ranking only.
 * hg_get_topr_real copies the ranked lists of the last hg_topr_real; hg_map_real leaves them unwritten where it ranks in LDS (as hg_map
 * does for codes: the lists are Q x R x 8 bytes of stores the APs do not need) -- HG_ERR_STATE then, unless option "real_map_lists" is 1. */
int hg_map_real(hg_ctx* ctx, int64_t R, double* host_ap, int64_t* host_rel);
int hg_topr_real(hg_ctx* ctx, int64_t R);
int hg_get_topr_real(hg_ctx* ctx, uint32_t* host_idx, float* host_scores);   /* [Q][R] each */

/* ---- asymmetric ranking: real-valued queries against the database's packed codes (asymmetric distance, Gordo et al.) ----
 * What a deployed hashing system runs: the database is stored as codes, the fresh query keeps its float32 features, and rows are ranked
 * by s(q, n) = sum_k q_k x_nk with x_nk = +1.0f where bit k of row n's code is set (feature > 0, the loaders' rule: a zero feature is
 * -1) and -1.0f elsewhere -- in the fixed arithmetic of the real-valued ranking above: acc = fmaf(q_k, x_nk, acc) for k = 0 .. b - 1
 * from +0.0, then + 0.0.  Order: s descending, database index ascending; label match, AP and hit counts as hg_map_real's.  Bit for bit
 * what hg_topr_real / hg_map_real return on the same queries and the float table where(code bit, +1, -1), and what
 * oracle/real_map.py::map_from_features returns on that table -- without that table: the filter's image and the exact rescoring read
 * the codes (k_asym_image16, k_asym_rescore: 8 bytes per kept row at 64 bits instead of 256).
 *   Tables    the database's codes and labels from ANY loader (hg_set_database packed, hg_set_database_f32 with any "keep_floats",
 *             hg_set_database_dev): its float table is never needed and never created by a load.  The queries' float table: load them
 *             with hg_set_queries_f32 / hg_set_queries_dev under option "keep_query_floats" = 1 (0, the default: the query floats stay
 *             only when the database's do).  Without it: HG_ERR_STATE, and the message names the option.
 *   Limits    hg_map_real's: b <= 255, N < 2^31, one shard (HG_ERR_STATE on a shard), 1 <= R <= N (else HG_ERR_ARG).
 *   State     a successful call leaves what hg_topr_real / hg_map_real leave: hg_get_topr_real, hg_get_ap, hg_get_match, hg_ap_at,
 *             hg_graded, hg_votes and hg_export work on it unchanged (hg_export refuses HG_OUT_DIST as after any inner-product ranking).
 *             A failed or refused call leaves no lists.
 *   Fallback  a bet (R * 8 <= N, N >= 65536) under "real_mfma" = 2 runs from the codes alone.  The paths that read plain float rows
 *             (no cut: R = N or an exhausted ladder; "real_mfma" < 2; the vector kernels) get them from a work buffer of +-1.0 rows
 *             expanded from the codes on first need per database (k_asym_expand_rows; N x bpad x 4 bytes, counted in "device_bytes",
 *             freed by hg_trim, forgotten by a database load).
 *   Stats     "real_path" / "real_attempts" / "real_requeried" as for hg_map_real; "asym_calls" (successful asymmetric calls,
 *             cumulative); "asym_float_rows" (1: the last asymmetric call read the expanded float rows; 0: codes only). */
int hg_map_asym(hg_ctx* ctx, int64_t R, double* host_ap, int64_t* host_rel);
int hg_topr_asym(hg_ctx* ctx, int64_t R);

/* ---- quantised databases: real-valued queries against product-quantisation codes (AQD, the asymmetric quantiser distance) ----
 * The database is stored as PQ codes and small codebooks: M disjoint subspaces of dsub features each (b = M * dsub <= 255), K <= 256
 * codewords per subspace; codebooks float32 [M][K][dsub], codes uint8 [N][M].  A row decodes by pure gather,
 *     x[n][k] = codebooks[k / dsub][codes[n][k / dsub]][k % dsub],
 * and is ranked by s(q, n) in the fixed arithmetic of the real-valued ranking: acc = fmaf(q_k, x_nk, acc) for k = 0 .. b - 1 from +0.0,
 * then + 0.0.  Order: s descending, database index ascending; label match, AP and hit counts as hg_map_real's.  Bit for bit what
 * hg_topr_real / hg_map_real return on the decoded table and what oracle/real_map.py::map_from_features returns on it -- without that
 * table (256 MB at 1M x 64; the codes are 8 MB, the codebooks 64 KB): the filter's image and the exact rescoring look every feature up
 * (k_pq_image16, k_pq_rescore).  SQD (the query quantised too) is the same call on the query's decoded codes: a gather on the host.
 *   hg_set_database_pq   loads codes, codebooks and labels (int64 [N][C], as hg_set_database_f32).  Afterwards the context holds what
 *             hg_set_database_f32 leaves for the decoded table under "keep_floats" = 0 -- the sign codes (bit = decoded feature > 0,
 *             derived by host threads from per-codeword sign patterns: no N x b floats exist anywhere in a load), the labels, the census
 *             -- plus the PQ tables, so every Hamming-side call works on it unchanged.  Any other database loader forgets the PQ tables.
 *             Refused with HG_ERR_ARG, the message naming the offender: M, K or dsub < 1, K > 256, M * dsub > HG_MAX_BITS, a code byte
 *             >= K (row and subspace), a non-finite codebook entry (a deliberate restriction: the filter's norm bound and the NaN
 *             handling of a float table stay out of this form), idx_base != 0 or n_total != N (one shard only).
 *   Queries   their float table: hg_set_queries_f32 / hg_set_queries_dev under option "keep_query_floats" = 1.
 *   Refused   HG_ERR_STATE without PQ tables (the message names hg_set_database_pq) or without the queries' floats (names the option).
 *   Limits    hg_map_real's: N < 2^31, 1 <= R <= N (else HG_ERR_ARG).  Additive codebooks over the full dimension are not supported.
 *   State     a successful call leaves what hg_topr_real / hg_map_real leave (hg_get_topr_real, hg_get_ap, hg_get_match, hg_ap_at,
 *             hg_graded, hg_votes, hg_export; hg_export refuses HG_OUT_DIST).  A failed or refused call leaves no lists.
 *   Fallback  the paths that read plain float rows (no cut: R = N or an exhausted ladder; "real_mfma" < 2; the vector kernels; segments
 *             that are no multiple of 16 rows) get them from a work buffer decoded on first need per database (k_pq_expand_rows;
 *             N x bpad x 4 bytes, counted in "device_bytes", freed by hg_trim, forgotten by a database load).
 *   Stats     "real_path" / "real_attempts" / "real_requeried" as for hg_map_real; "pq_calls" (successful quantised calls, cumulative);
 *             "pq_float_rows" (1: the last quantised call read the decoded float rows; 0: codes and codebooks only). */
int hg_set_database_pq(hg_ctx* ctx, const uint8_t* host_codes, const float* host_codebooks, const int64_t* host_labels, int64_t N,
                       int M, int K, int dsub, int C, int64_t idx_base, int64_t n_total, int64_t* bad_codes, int64_t* bad_labels);
int hg_map_pq(hg_ctx* ctx, int64_t R, double* host_ap, int64_t* host_rel);
int hg_topr_pq(hg_ctx* ctx, int64_t R);
/* The codes themselves, from float features, on the GPU (k_pq_encode): the exact encoder.  For codebooks float32 [M][K][dsub] and a
 * feature row x (b = M * dsub <= 255, K <= 256) the code of subspace m is
 *     d_k = 0.0 (float64);  for j = 0 .. dsub-1:  t = (double)x[m*dsub+j] - (double)w[m][k][j];  d_k = d_k + t*t
 *     code = the lowest k with d_k minimal:   best = 0; for k = 1 .. K-1: if (d_k < d_best) best = k
 *     err(row) = 0.0; for m = 0 .. M-1: err += d_best(m)          (float64)
 * Every operation is IEEE float64 and rounded once; t*t and the addition are two roundings (no fused multiply-add); features and
 * codewords run in ascending order; the comparison is a strict `<`.  16-bit features (IEEE half, bfloat16) are widened exactly to
 * float32 first.  A row with a non-finite feature makes every d_k of that subspace +inf or NaN, so the strict `<` leaves code 0 there,
 * and its other subspaces are unaffected; such rows are counted in *bad_rows and not refused.
 *   hg_pq_encode       host features float32 [N][b], uploaded in row chunks through a bounded work buffer (option
 *             "pq_encode_chunk_rows"; 0 = the default, 256 MB of features); host_codes uint8 [N][M]; host_err float64 [N] or NULL.
 *   hg_pq_encode_dev   features in device memory: float32 / float16 / bfloat16, any strides >= 1, no alignment assumed; refusals and
 *             stream ordering as hg_set_database_dev's (copy-in, complete on return, waits on features->stream).
 *             Both need no database and no queries, and leave whatever the context holds -- tables, ranked lists, PQ tables,
 *             generations, hg_map_begin's licence -- exactly as it was; their work buffers are counted in "device_bytes" and freed by hg_trim.
 *             Refused with HG_ERR_ARG before anything is launched, the message naming the offender: null pointers or N < 1; M, K or
 *             dsub < 1; K > 256; M * dsub > HG_MAX_BITS; features->cols != M * dsub; a non-finite codebook entry; N >= 2^31.
 *   hg_set_database_pq_f32   encodes host features on the GPU and loads the result: the context is left exactly as
 *             hg_set_database_pq leaves it for those codes (which come back to the host on the way: N x M bytes).  It refuses what
 *             hg_set_database_pq refuses; with *bad_rows > 0 it loads nothing and returns HG_ERR_ARG.
 *   Stats     "pq_encode_calls" (encoder calls that succeeded) and "pq_encoded_rows" (the rows they encoded), both cumulative. */
int hg_pq_encode(hg_ctx* ctx, const float* host_features, int64_t N, const float* host_codebooks, int M, int K, int dsub,
                 uint8_t* host_codes, double* host_err, int64_t* bad_rows);
int hg_pq_encode_dev(hg_ctx* ctx, const hg_dev_array* features, const float* host_codebooks, int M, int K, int dsub,
                     uint8_t* host_codes, double* host_err, int64_t* bad_rows);
int hg_set_database_pq_f32(hg_ctx* ctx, const float* host_features, const float* host_codebooks, const int64_t* host_labels,
                           int64_t N, int M, int K, int dsub, int C, int64_t idx_base, int64_t n_total,
                           int64_t* bad_codes, int64_t* bad_labels, int64_t* bad_rows);

/* ---- Hamming ranking with the tie groups re-ranked by the features ("sign, rank by Hamming distance, re-rank inside equal
 * distances by the real-valued inner product") ----
 * Row n against query q has d = popcount(code_q xor code_n) on the codes the loaders make (bit = feature > 0) and s = the float32
 * inner product of the FLOAT features in the fixed summation order of the real-valued ranking above (one fma chain from +0.0 in
 * feature order, then + 0.0: never -0.0; oracle/real_map.py::inner_products restates it).  Rows are ranked by (d ascending, s descending,
 * database index ascending) and the top R kept: of the threshold group the rows with the highest s get in, not the ones with the lowest
 * index, so membership differs from hg_topr's as well as the order.  The order is total and does not depend on R: the top k of a
 * ranking at R is the ranking at k (hg_ap_at stays valid on it).  Among NaN scores the order is unspecified (the keys are their bits).
 * Needs both float tables on the device (hg_set_*_f32 / hg_set_*_dev with option "keep_floats" = 1 when the features are a +-1 code;
 * HG_ERR_STATE otherwise) and the whole database in one context (a shard: HG_ERR_STATE).  R within 1..N, up to 255 features, and at most
 * 2^24 = 16 777 216 rows -- a record's 64-bit sort key is {distance: 8, score: 32, index: 24 bits} -- HG_ERR_ARG beyond.
 * hg_topr_rerank is a ranking like hg_topr: it owns the step state and leaves the idx / dist lists (hg_get_topr), the match bitmap
 * (hg_get_match; gathered through the idx lists, any class count), stage select + match, plus a float32 score list [Q][R]
 * (hg_get_rerank_scores: HG_ERR_STATE unless the last ranking on the tables loaded now was a re-rank).  hg_ap, hg_ap_at and hg_graded
 * work on it unchanged; like every ranking it ends the results hg_graded and hg_ap_at computed from the previous one, leaves the histogram
 * side tables (hg_rel_hist ...) alone, and is ended by a later ranking, a reload of either table or hg_trim.  hg_map_rerank = the same,
 * then hg_ap's float64 AP and the download.  Pipeline: exact histogram and plan (no bet, no capacity guess), one pass over the pairs
 * that collects the rows with d <= t into exact per-(query, distance) ranges, the exact score per record, one sort per query -- in LDS
 * up to 16384 records or group by group, a group beyond the LDS by radix passes in global memory.  Queries are processed in contiguous
 * chunks whose records (16 bytes each) fit option "dense_budget_mb"; a query beyond it is a chunk of one.  The call synchronises once
 * in the middle (the record counts come home) and once at the end whatever "stage_sync" says; results do not depend on the chunks or
 * the segment geometry.  Stats "rerank_records" (records kept, all queries), "rerank_chunks", "rerank_groups_lds" / "rerank_groups_global"
 * (distance groups ordered in LDS / by the radix passes). */
int hg_topr_rerank(hg_ctx* ctx, int64_t R);
int hg_map_rerank(hg_ctx* ctx, int64_t R, double* host_ap, int64_t* host_rel);
int hg_get_rerank_scores(hg_ctx* ctx, float* host_scores);                   /* [Q][R] */

/* ---- results to the host ----------------------------------------------------- */
int hg_get_topr(hg_ctx* ctx, uint32_t* host_idx, uint8_t* host_dist);   /* [Q][R] each */
int hg_get_match(hg_ctx* ctx, uint8_t* host_imatch);                    /* [Q][R] of 0/1 */
int hg_get_ap(hg_ctx* ctx, double* host_ap, int64_t* host_rel);         /* [Q]; ap = NaN where rel == 0 */
int hg_get_hist(hg_ctx* ctx, uint32_t* host_hist);                      /* [b+1][Q] of this shard */
int hg_get_rel_hist(hg_ctx* ctx, uint32_t* host_all, uint32_t* host_rel); /* [b+1][Q] each, this shard (after hg_rel_hist) */
int hg_get_grade_hist(hg_ctx* ctx, uint32_t* host_hist);                /* [C+1][Q] of this shard (after hg_grade_hist) */
int hg_get_joint_hist(hg_ctx* ctx, uint32_t* host_hist);                /* [b+1][G][Q] of this shard, G = stat "joint_hist_grades" (after hg_joint_hist) */

/* ---- results into the caller's DEVICE memory -------------------------------------------------------------------------------------
 * hg_export writes what the host getters above return into arrays of the caller's on the context's GPU -- a torch tensor, anything a
 * hg_dev_array can describe: any row / column stride (a slice, a transposed view), no alignment assumed -- without a host pass: one
 * copy-convert kernel per item (k_export, hg_dev_out.hpp).  dst.ptr is written through; dst.rows must be Q; dst.cols = k with
 * 1 <= k <= R of the last ranking: the first k ranks of every list are written (the top k of a ranking at R is the ranking at k);
 * HG_OUT_AP and HG_OUT_HITS take cols = 1.  Every value is the one the matching getter returns, converted: an index zero-extended to
 * int64 (or its 32 bits as int32: refused when n_total > 2^31 - 1), a distance or grade byte widened, a score's or an AP's bits as they
 * are (AP as float32: the correctly rounded conversion; NaN where the query has no hit), a match bit as 0 / 1, a hit count widened.
 *   State     each item follows its getter: IDX needs ranked lists (hg_topr, hg_topr_real, hg_topr_rerank, a staged select with lists),
 *             DIST Hamming lists, SCORE a real-valued ranking with lists or a re-rank, MATCH the match stage with the global bitmap of
 *             all Q queries (hg_ap_at's rule), AP and HITS hg_ap, GRADES the last hg_graded with keep_grades on these lists; otherwise
 *             HG_ERR_STATE naming the call that would provide it.  HG_ERR_STATE also while a step of hg_map_begin is in flight or a
 *             verdict is pending ("defer_verdict"): results that may still be withdrawn are not handed to another stream.
 *   Refused   with HG_ERR_ARG: everything hg_set_*_dev refuses (null pointers, strides < 1, an extent that overflows, a pointer that is
 *             not plain device memory of the context's device, an extent outside its allocation), a dtype outside the item's list, a
 *             wrong shape, strides under which two elements share an address (accepted: one row or one column, row_stride >
 *             (cols-1)*col_stride, or col_stride > (rows-1)*row_stride -- every slice or transpose of a contiguous array), a
 *             destination that intersects a result buffer of the context, two items of one call whose extents intersect.
 *   All or nothing   every item is checked before anything is enqueued: a refused call writes no byte.
 *   Ordering  dst.stream is the CONSUMER's stream (NULL = the null stream).  The context's stream first waits for everything enqueued
 *             so far on each distinct dst.stream (an event on each: earlier readers and writers of the destination finish first), the
 *             kernels run on the context's stream, then every distinct dst.stream waits for an event recorded behind them: whatever
 *             the consumer enqueues on its stream after the call sees the data, with no host synchronisation.  With "stage_sync" = 1
 *             (default) the call is also complete on return; with 0 it only enqueues, and the destination must stay allocated until
 *             its stream has passed the wait.  Work on a non-blocking stream of the caller's is only ordered if that stream's handle
 *             is passed.
 *   No pointer is kept.  Timing name "k_export"; stats "export_bytes" (bytes the last call wrote) and "export_variant" (bit 0: a kernel
 *   of the last call took the 16-byte store path, bit 1: one took the element-wise path; 0: no call yet). */
#define HG_OUT_IDX    0   /* ranked database indices      [Q][k]  int64 | int32 */
#define HG_OUT_DIST   1   /* their Hamming distances      [Q][k]  uint8 | int32 */
#define HG_OUT_SCORE  2   /* float32 inner products       [Q][k]  float32 */
#define HG_OUT_MATCH  3   /* label match per rank, 0/1    [Q][k]  uint8 (bool) */
#define HG_OUT_AP     4   /* AP per query, NaN = no hit   [Q][1]  float64 | float32 */
#define HG_OUT_HITS   5   /* hits among the top R         [Q][1]  int64 | int32 */
#define HG_OUT_GRADES 6   /* grade per rank (hg_graded, keep_grades) [Q][k] uint8 | int32 */
typedef struct hg_export_item { int what; hg_dev_array dst; } hg_export_item;
int hg_export(hg_ctx* ctx, const hg_export_item* items, int n);     /* 1 <= n <= 8 */

/* ---- graded relevance along the ranked lists (ACG, NDCG, WAP at k) -------------
 * hg_graded walks the ranked index lists the last ranking left on the device -- hg_topr, a staged hg_select with lists, hg_topr_real;
 * HG_ERR_STATE after anything that writes none (hg_map, hg_map_real): call hg_topr / hg_topr_real first -- and leaves, per query and
 * cut-off k = ks[j], with g_i = popcount(query labels & labels of the row at rank i):
 *   gsum = sum_{i<=k} g_i,  hits = #{i<=k : g_i > 0},  dcg = sum_{i<=k} gain[g_i] * disc[i-1],  wsum = sum_{i<=k, g_i>0} (sum_{m<=i} g_m) / i
 * ks: nk (1..64) strictly ascending values in 1..R of the lists; gain: C + 1 doubles; disc: ks[nk-1] doubles (disc[i-1] belongs to rank i);
 * C <= 255; anything else HG_ERR_ARG.  The host arrays are copied before the call returns.  Indices outside the table count as grade 0.
 * The context must hold the whole database (idx_base 0, N = n_total) -- or a shard of it together with a current merged grade plane
 * (hg_merge_list_table, below): the same kernel then reads the grade of every rank from the plane; HG_ERR_STATE on a shard without one.
 * The summation order depends on ks
 * alone (chunks of 256 ranks cut at every k, fixed trees inside), so equal inputs give equal bits; float64 throughout, no atomics.
 * keep_grades != 0 also keeps the grade bytes of every rank for hg_get_grades.  The results belong to the lists they were computed on:
 * any later ranking, hg_merge_topr, a database or query reload and hg_trim invalidate them (the getters then return HG_ERR_STATE, as
 * they do before the first pass).  The ranking's own state -- stage, match bits, APs -- is untouched. */
int hg_graded(hg_ctx* ctx, const int64_t* host_ks, int nk, const double* host_gain, const double* host_disc, int keep_grades);
int hg_get_graded(hg_ctx* ctx, int64_t* host_gsum, int64_t* host_hits, double* host_dcg, double* host_wsum);   /* [Q][nk] each; null: skipped */
int hg_get_grades(hg_ctx* ctx, uint8_t* host_grades);                   /* [Q][R]; HG_ERR_STATE unless the last hg_graded kept them */

/* ---- tie-aware AP at the top-R cut (expected AP over the orders inside the Hamming tie groups, and its bounds) -------------
 * A b-bit code has b + 1 distances, so nearly every rank of a Hamming ranking lies inside a tie group, and AP@R depends on how the
 * relevant rows happen to be ordered inside each group.  hg_tie_ap computes, per query and cut-off R = Rs[j], from hg_rel_hist's two
 * tables alone (no select, no lists; it runs that pass itself unless the tables of the loaded queries and database are there):
 *   ap_exp   the expectation of the reference's AP@R (lib/metric.py:19-23) over uniformly random orders inside every tie group, given
 *            that the top R hold a relevant row (the reference skips a query without one); NaN when p_hit = 0
 *   p_hit    the probability of that condition
 *   ap_min, ap_max   the exact minimum and maximum of AP@R over all those orders (NaN when no order has a hit)
 *   rel_exp, rel_lo, rel_hi   expectation, minimum and maximum of the relevant rows among the top R
 * Rs: nR (1..64) strictly ascending values in 1..N, anything else HG_ERR_ARG; copied before the call returns.  The context holds the
 * whole database (idx_base 0, N = n_total) -- or a shard of it together with a merged rel table of the loaded queries and database
 * (hg_merge_side_table, below): the same kernel then reads the merged table, never runs the pass, and the cut-offs reach 1..n_total.  A
 * shard without a current merged table: HG_ERR_STATE.  A whole-database context never looks at a merged table.  float64 throughout; the order of every addition is a function of
 * the query's two table columns and R, so equal inputs give equal bits whatever Q is.  Tables of its own: the staged pipeline's
 * state, hg_hist's histogram, lists, match bits, APs and a step of hg_map_begin in flight are left as they were.  A database or query
 * reload and hg_trim invalidate the results (hg_get_tie_ap then returns HG_ERR_STATE, as it does before the first pass). */
int hg_tie_ap(hg_ctx* ctx, const int64_t* host_Rs, int nR);
int hg_get_tie_ap(hg_ctx* ctx, double* host_ap_exp, double* host_p_hit, double* host_ap_min, double* host_ap_max,
                  double* host_rel_exp, int64_t* host_rel_lo, int64_t* host_rel_hi);   /* [Q][nR] each; null: skipped */

/* ---- AP, precision and recall at many cut-offs from one ranking ------------------------------------------------------------------
 * The canonical order is total, so the top Rs[j] is a prefix of the top R: hg_ap_at walks the match bitmap the last ranking left --
 * hg_topr, hg_topr_real, hg_map, hg_map_real, a staged sequence up to hg_match, a merge of all queries -- once per query and gives,
 * for every cut-off, ap[q][j] with the very bits hg_ap gives after a ranking at R = Rs[j] (NaN where the top Rs[j] hold no hit) and
 * rel[q][j], the hits among the top Rs[j] (precision@k = rel / k; recall@k = rel / hg_rel_hist's total).  One kernel launch (k_ap_at).
 * Precondition: hg_ap's (the match stage), in global rank order for all Q queries: HG_ERR_STATE for a bitmap in a shard's local
 * rank order (hg_select_ranked before its merge), for a shard's own part of a bitmap (G > 1 before hg_merge_match / hg_merge_ranked),
 * after a merge of a query range only, and after a step of hg_map_begin that ran in the second stream's workspace.
 * Rs: nR (1..64) strictly ascending values in 1..R of the last ranking, anything else HG_ERR_ARG; copied before the call returns.
 * float64 throughout, no atomics: equal inputs give equal bits whatever Q and the other cut-offs are.  Tables and buffers of its own:
 * stage, hg_ap's results, lists, the one-R AP tables and a step of hg_map_begin in flight are left as they were.  Results belong to the
 * bitmap they were computed on: a later ranking, hg_match, hg_merge_match / hg_merge_ranked, a database or query reload and hg_trim
 * invalidate them (hg_get_ap_at then returns HG_ERR_STATE, as it does before the first pass). */
int hg_ap_at(hg_ctx* ctx, const int64_t* host_Rs, int nR);
int hg_get_ap_at(hg_ctx* ctx, double* host_ap, int64_t* host_rel);   /* [Q][nR] each; null: skipped */

/* ---- class votes along the ranked lists (kNN accuracy, retrieval confusion matrix) ------------------------------------------------
 * "Which classes did the query retrieve?"  hg_votes walks the ranked index lists the last ranking left on the device -- hg_graded's
 * precondition: hg_topr, a staged hg_select with lists, hg_topr_real, hg_topr_rerank; HG_ERR_STATE after anything that writes none
 * (hg_map, hg_map_real) and on a context that holds a shard (idx_base != 0 or N != n_total) without a current merged vote table
 * (hg_merge_list_table, below; with one, pred / top come from k_vote_pick and conf from k_vote_confusion on the merged counts, and ks
 * must be the merge's) -- and leaves, per query q, cut-off
 * k = ks[j] and class c:
 *   votes[q][j][c] = #{ranks i < k whose row idx[q][i] carries label c}                   uint32 [Q][nk][C]
 *   top[q][j]      = max_c votes[q][j][c];   pred[q][j] = the smallest c that reaches it, -1 when top is 0   [Q][nk]
 *   conf[j][a][b]  = sum over the queries q that carry label a of votes[q][j][b]          int64 [nk][C][C]
 * An index >= N (a slot of another shard included) votes for nothing; bits past class C - 1 of a label word are never counted; a query
 * without labels adds nothing to conf.  ks: nk (1..64) strictly ascending values in 1..R of the lists; C <= 255; anything else
 * HG_ERR_ARG.  ks is copied before the call returns.  Integers throughout -- every value is exact and independent of any order.  Two
 * kernel launches (k_votes, k_vote_confusion), tables and buffers of its own: stage, lists, match bits, APs, the other side metrics'
 * results and a step of hg_map_begin in flight are left as they were.  The results belong to the lists they were computed on: any later
 * ranking, hg_merge_topr, a database or query reload and hg_trim invalidate them, and so does a refused hg_votes call (the getters then
 * return HG_ERR_STATE, as they do before the first pass). */
int hg_votes(hg_ctx* ctx, const int64_t* host_ks, int nk);
int hg_get_vote_pred(hg_ctx* ctx, int32_t* host_pred, int64_t* host_top);   /* [Q][nk] each; null: skipped */
int hg_get_vote_confusion(hg_ctx* ctx, int64_t* host_conf);             /* [nk][C][C] */
int hg_get_votes(hg_ctx* ctx, uint32_t* host_votes);                    /* [Q][nk][C] */

/* ---- label-free relevance: ground-truth neighbour sets ----------------------------------------------------------------------------
 * Everything above calls a row relevant when it shares a class label with the query.  Unsupervised hashing, ANN benchmarks and
 * binary-embedding quantisation have no labels: the ground truth of a query q is a SET of database rows NB(q) -- its true nearest
 * neighbours in the original feature space -- and the question is how much of it a ranking recovers.  NB(q) holds n_q distinct global
 * row numbers in [0, n_total), 0 <= n_q <= G, 1 <= G <= 16384.  The sets are a table of the loaded queries and database like every side
 * result: a reload of either and hg_trim end them, and so does a refused call of the two that make them.  They need the whole database
 * in one context (idx_base == 0, N == n_total): HG_ERR_STATE on a shard.
 *   hg_set_neighbours         host_ids [Q][G] in any order, 0xFFFFFFFF pads a shorter set; Q must be the loaded query count, G in
 *                             1..16384 (HG_ERR_ARG otherwise).  Each row is sorted ascending on the device and n_q counted (k_nbr_sort);
 *                             a row with a duplicate or an id >= n_total is found there and refused with HG_ERR_ARG after one flag word
 *                             has come back.  Synchronises whatever "stage_sync" says.
 *   hg_neighbours_from_lists  the first G ranks (G <= R, else HG_ERR_ARG) of the ranked index lists the last ranking left on the device
 *                             -- hg_votes' precondition: hg_topr, hg_topr_real, hg_topr_asym, hg_topr_rerank, a staged hg_select with
 *                             lists; HG_ERR_STATE otherwise -- become the sets: after hg_topr_real the exact float32 top G is the ground
 *                             truth without ever leaving the GPU.  The lists are only read.
 *   hg_get_neighbours         the sorted table [Q][G], pads at the end, and n_q [Q]; either may be null.
 *   hg_match_neighbours       rewrites the match bitmap (uint64 [Q][ceil(R/64)], bits past R zero): slot k of query q matches iff
 *                             idx[q][k] is in NB(q); a slot holding 0xFFFFFFFF or an index >= N never matches (k_nbr_match).  Needs
 *                             the sets and ranked index lists in global rank order for all Q queries -- the lists hg_votes accepts on a
 *                             whole-database context; HG_ERR_STATE without either, after the list-free hg_map / hg_map_real /
 *                             hg_map_begin, and for lists in a shard's local rank order.  It sets the match stage, clears the AP stage
 *                             and ends hg_ap_at's tables; hg_ap, hg_get_ap, hg_get_match, hg_ap_at and hg_export (match, ap, hits) then
 *                             work unchanged on the neighbour bits: AP is the reference's (hits inside the top R in the denominator, NaN
 *                             where there are none), recall@k = hits@k / n_q.  hg_match is not changed: it sees the match stage set and
 *                             returns, so the label bits come back only with the next ranking.  Stat "match_source": 0 the bitmap came
 *                             from the labels, 1 from the neighbour sets; every ranking resets it to 0.
 *   hg_nbr_hist               nbr[d][q] = #{n in NB(q) : Hamming distance of q and n = d}, the shape and meaning of hg_rel_hist's rel
 *                             table: with that pass's all table, recall and precision over the Hamming radius for neighbour relevance,
 *                             no ranking needed.  Q x G pairs through the packed codes (k_nbr_hist), b up to HG_MAX_BITS, integers only:
 *                             independent of Q and of the order the set was given in.  A table of its own: stage, lists, bitmap, the
 *                             other side results and a step of hg_map_begin in flight are left as they were; a new set ends it.
 *   hg_get_nbr_hist           nbr [b+1][Q] and n_q [Q]; either may be null. */
int hg_set_neighbours(hg_ctx* ctx, const uint32_t* host_ids, int64_t Q, int G);
int hg_neighbours_from_lists(hg_ctx* ctx, int G);
int hg_get_neighbours(hg_ctx* ctx, uint32_t* host_ids_sorted, uint32_t* host_count);
int hg_match_neighbours(hg_ctx* ctx);
int hg_nbr_hist(hg_ctx* ctx);
int hg_get_nbr_hist(hg_ctx* ctx, uint32_t* host_nbr, uint32_t* host_count);

/* ---- the histogram tables of a database-sharded context: pack, exchange, merge -------------------------------------------------
 * hg_rel_hist's, hg_grade_hist's and hg_joint_hist's tables are additive over shards (contexts loaded with idx_base / n_total; the
 * queries replicated, so Q, b and C are equal on every rank).  Everything read from them -- the lookup curves over the Hamming radius,
 * tie-aware AP and precision / recall, tie-aware NDCG / ACG, IDCG -- is a function of the whole database's table alone, so a rank
 * that holds the SUM of the shards' tables gives the bits one context with the whole database gives.  The tables stay on the device:
 *   hg_<pass>  ->  hg_pack_side_table  ->  all-gather of the block (hg_allgather, or the caller's)  ->  hg_merge_side_table
 * The exchange unit is one contiguous block of uint32 planes [planes][Qpad], q fastest, Qpad = Q rounded up to 64:
 *   HG_SIDE_REL    [2][b+1][Qpad]     all, then rel
 *   HG_SIDE_GRADE  [C+1][Qpad]
 *   HG_SIDE_JOINT  [b+1][Gc][Qpad]    the shard's [b+1][Gs][Qpad] with zero planes for g = Gs..Gc-1.  A shard's Gs (stat
 *                                     "joint_hist_grades") depends on its own rows: the ranks agree on Gc = max Gs before they pack
 * hg_pack_side_table: needs the shard's table `which` of the loaded queries and database (HG_ERR_STATE, naming the pass, otherwise).
 *   Gc is ignored unless which is HG_SIDE_JOINT; there Gc < Gs or Gc > C + 1 is HG_ERR_ARG.  *dev_ptr / *nbytes: the block, owned by
 *   the context, valid until the next hg_pack_side_table, a reload or hg_trim.  One kernel (k_side_pack); ends like a staged call
 *   (synchronises unless "stage_sync" is 0).  Changes no result.
 * hg_merge_side_table: dev_tabs_all = Gsh (1..4096) such blocks back to back, 16-byte aligned (what hg_allgather leaves); Gc as packed
 *   (ignored unless joint).  One kernel (k_side_merge) sums them cell by cell in 64 bits into a merged table of the context's own and
 *   checks, for every query q < Q, that the column total -- over the `all` planes for rel, over g for grade, over (d, g) for joint --
 *   is n_total.  A cell of a real query that does not fit uint32 (overflow flag) or a column total other than n_total (column-total
 *   flag: a shard is missing, counted twice or stale) fails the call with HG_ERR_STATE and a message naming the flag.  Both flags are
 *   integer and independent of any order.  The host reads them: the call synchronises whatever "stage_sync" says.
 * A merged table belongs to the queries and database it was merged on: it is ended by its own merge call when that is refused or fails,
 * by a reload of the queries or the database and by hg_trim -- by nothing else.  The shard's own tables and their getters keep meaning
 * "this shard".  Stage, geometry, lists, match bits, APs, the other side results and a step of hg_map_begin in flight are left as they
 * were by all five calls.  Getters: [b+1][Q] twice, [C+1][Q], [b+1][Gc][Q] with Gc = stat "merged_joint_grades"; HG_ERR_STATE without
 * a current merged table.  hg_tie_ap on a shard reads the merged rel table (above). */
#define HG_SIDE_REL 0
#define HG_SIDE_GRADE 1
#define HG_SIDE_JOINT 2
int hg_pack_side_table(hg_ctx* ctx, int which, int Gc, void** dev_ptr, int64_t* nbytes);
int hg_merge_side_table(hg_ctx* ctx, int which, const void* dev_tabs_all, int Gsh, int Gc);
int hg_get_merged_rel_hist(hg_ctx* ctx, uint32_t* host_all, uint32_t* host_rel);   /* [b+1][Q] each, the whole database; null: skipped */
int hg_get_merged_grade_hist(hg_ctx* ctx, uint32_t* host_hist);                    /* [C+1][Q] */
int hg_get_merged_joint_hist(hg_ctx* ctx, uint32_t* host_hist);                    /* [b+1][Gc][Q] */

/* ---- the list-based side metrics of a database-sharded context: pack, exchange, merge ------------------------------------------
 * hg_graded and hg_votes walk the ranked lists, and a shard's lists are partial.  The exact staged sequence (hg_hist -> hg_plan ->
 * hg_select with "staged_lists" = 1) leaves a shard's members of the global top R in their GLOBAL rank positions -- the global row
 * index where slot i is the shard's, IDX_NONE where it is another's --, so every slot belongs to exactly one shard and two small
 * tables per shard carry everything the two passes need:
 *   HG_LIST_GRADES  uint8 [Q][Rp] then uint32 own[Qpad]   Rp = R rounded up to 16, Qpad = Q rounded up to 64.  Byte i of row q: the
 *                   labels query q shares with the shard's own row in slot i; 0 where the slot is another shard's and for i >= R.
 *                   own[q]: the slots i < R of query q that are this shard's.  Q Rp + 4 Qpad bytes.
 *   HG_LIST_VOTES   uint32 [nk][C+1][Qpad], q fastest.  Plane (j, c), c < C: the shard's own slots i < ks[j] whose row carries class
 *                   c; plane (j, C): the shard's own slots i < ks[j].  4 nk (C+1) Qpad bytes.
 *   ranking  ->  hg_pack_list_table  ->  all-gather of the block (hg_allgather, or the caller's)  ->  hg_merge_list_table  ->  hg_graded / hg_votes
 * hg_pack_list_table: needs position-space lists of the loaded tables -- a staged hg_select with lists, or hg_topr on a context that
 *   holds the whole database (one block, Gsh = 1); HG_ERR_STATE before such a ranking, after hg_select_ranked (local rank order) and on
 *   real-valued lists.  At most 255 classes (HG_ERR_ARG).  Grades: ks is ignored and may be NULL (the plane covers all R slots).  Votes:
 *   ks as hg_votes takes them -- nk (1..64) strictly ascending values in 1..R, else HG_ERR_ARG.  *dev_ptr / *nbytes: the block, owned by
 *   the context, valid until the next hg_pack_list_table, a reload or hg_trim.  One kernel (k_list_grades, or k_votes in its
 *   owned-slots form); ends like a staged call (synchronises unless "stage_sync" is 0).  Changes no result.
 * hg_merge_list_table: dev_blocks_all = Gsh (1..4096) such blocks back to back, 16-byte aligned; ks / nk as packed (ignored for
 *   grades).  NULL, Gsh out of range, a misaligned address or an unknown `which`: HG_ERR_ARG.  One kernel merges them into a table of
 *   the context's own -- k_list_merge_grades ORs the planes, k_list_merge_votes sums the tables in 64 bits -- and checks every query
 *   q < Q: grades -- the own words sum to R (owned-slots flag), no byte i < R is non-zero in two blocks (slot-claimed-twice flag), no
 *   byte exceeds C (grade-range flag: the merged plane indexes hg_graded's gain table); votes -- plane (j, C) sums to ks[j]
 *   (owned-slots flag), every cell fits uint32 (overflow flag).  A raised flag fails the call with HG_ERR_STATE and a message naming
 *   the flag and the smallest offending query, and leaves no merged table of that kind; the flags are integer and independent of any
 *   order; pad bytes and pad queries are never checked.  The host reads the flags: the call synchronises whatever "stage_sync" says.
 * With a current merged grade plane hg_graded on a shard runs from it (the same kernel, its grade read from the plane: the bits one
 * context gives; keep_grades copies the plane out); with a current merged vote table hg_votes on a shard picks the predictions
 * (k_vote_pick) and builds the confusion matrix from it -- its ks must be the merge's, else HG_ERR_ARG.  Without one both refuse a
 * shard as before.  The getters are hg_graded's and hg_votes'.  A context that holds the whole database never looks at a merged table.
 * A merged list table belongs to the ranking and tables it was made from: a new ranking, hg_merge_topr, a reload of the queries or
 * the database, hg_trim and a refused merge of its own kind end it; a side-table pass or merge, hg_ap_at and hg_tie_ap do not.  Stage,
 * geometry, lists, match bits, APs, the other side results and a step of hg_map_begin in flight are left as they were by both calls. */
#define HG_LIST_GRADES 0
#define HG_LIST_VOTES 1
int hg_pack_list_table(hg_ctx* ctx, int which, const int64_t* host_ks, int nk, void** dev_ptr, int64_t* nbytes);
int hg_merge_list_table(hg_ctx* ctx, int which, const void* dev_blocks_all, int Gsh, const int64_t* host_ks, int nk);

/* ---- collectives: RCCL over xGMI, one process per GPU (the reference has no counterpart --
 * main.py:260-263 only sets CUDA_VISIBLE_DEVICES) --------------------------------------------------------
 * librccl.so.1 is dlopen'ed by the first hg_comm_* call (HG_RCCL_LIBRARY overrides the search); a single-GPU
 * process never loads it.  Rank 0 obtains a unique id and hands its HG_COMM_ID_BYTES bytes to the other ranks out
 * of band (hashgan_amd/sharded.py: a file next to the launcher's rendezvous), then every rank calls hg_comm_init.
 * Collectives run on the context's own stream, ordered with its kernels; with "stage_sync" = 1 (default) a
 * call is complete when it returns.
 *   hg_allgather        every rank contributes nbytes from dev_src; *dev_gathered = [world][nbytes] in a buffer the
 *                       context owns (slot 0..3: that many gathered buffers can be live at once), rank order.
 *                       This is the exchange of every staged sequence above (histograms, match bitmaps).
 *   hg_allgather_topr   the north star's exchange: the shards' ranked (idx, dist) lists all-gathered and merged
 *                       (hg_merge_topr); hg_get_topr then returns the global lists on every rank.
 *   hg_allreduce_max_f64 / hg_barrier   benchmark plumbing (max of the ranks' step times; barrier). */
#define HG_COMM_ID_BYTES 128
int hg_comm_unique_id(uint8_t* id);
int hg_comm_init(hg_ctx* ctx, const uint8_t* id, int rank, int world);
int hg_comm_destroy(hg_ctx* ctx);
int hg_comm_info(hg_ctx* ctx, int* rank, int* world);          /* *world = 0: no communicator */
int hg_allgather(hg_ctx* ctx, int slot, const void* dev_src, int64_t nbytes, void** dev_gathered);
/*   hg_alltoall         dev_src = [world][nbytes_per_peer]: block r goes to rank r; *dev_out = [world][nbytes_per_peer], block r
 *                       = what rank r sent here (a context buffer, slot 0..3 shared with hg_allgather).  The exchange of
 *                       the owner-routed sequence below. */
int hg_alltoall(hg_ctx* ctx, int slot, const void* dev_src, int64_t nbytes_per_peer, void** dev_out);
/* One rank's WHOLE step of the database-sharded bet (AP only, exchanges routed by query owner), enqueued back to back on the
 * context's stream with a single synchronisation at its final download -- the sequence hg_sample_hist -> hg_pack_sample_by_owner ->
 * hg_alltoall -> hg_guess_owned -> hg_alltoall -> hg_guess_finish -> hg_select_ranked -> hg_pack_ranked_by_owner -> hg_alltoall ->
 * hg_merge_ap_owned -> hg_allgather -> hg_unpack_parts in one call.  host_ap / host_rel: [Q] of ALL queries, identical on every rank.
 * *bet_lost: 0 the bet held; 1 lost on some shard (the same on every rank: widen the slices -- "cap_boost" -- and call again, or run
 * the staged exact sequence); -1 nothing was enqueued (hg_bet_eligible says no, or more shards than hg_merge_ranked takes).
 * The exchange is the context's communicator (hg_comm_init).  Without one, replica_world >= 1 makes every peer a replica of this
 * rank (device-to-device copies of its own blocks): what ONE rank of a replica_world-GPU run executes, for timing on one GPU;
 * replica_world = 1 is the one-GPU result. */
int hg_shard_step(hg_ctx* ctx, int64_t R, int replica_world, double* host_ap, int64_t* host_rel, int* bet_lost);
int hg_allgather_topr(hg_ctx* ctx);
int hg_allreduce_max_f64(hg_ctx* ctx, double* host_inout);
int hg_barrier(hg_ctx* ctx);
/* Context-owned device scratch (slot 0..3, grows only) and a stream-ordered device-to-device copy: what an
 * in-process communicator needs to do hg_allgather's job between several contexts of ONE process
 * (virtual shards on one GPU: tests/test_sharded_gpu.py). */
int hg_scratch(hg_ctx* ctx, int slot, int64_t nbytes, void** dev_ptr);
int hg_memcpy_dtod(hg_ctx* ctx, void* dev_dst, const void* dev_src, int64_t nbytes);
/* The same between a device address and host memory, complete on return (a communicator that goes through the host,
 * for multi-process dry runs on ONE GPU: tests/file_comm.py). */
int hg_memcpy_dtoh(hg_ctx* ctx, void* host_dst, const void* dev_src, int64_t nbytes);
int hg_memcpy_htod(hg_ctx* ctx, void* dev_dst, const void* host_src, int64_t nbytes);

/* Wait until everything the context has enqueued is done (with "stage_sync" = 0 nothing else does). */
int hg_synchronize(hg_ctx* ctx);

/* Run the context on a stream of the caller's (NULL: back to a private one).  With option
 * "stage_sync" = 0 the staged calls (hg_allgather included) only enqueue: every stage and the collectives
 * between them then sit on ONE stream with no host synchronisation except the bet's verdict and the
 * final hg_get_*. */
int hg_set_stream(hg_ctx* ctx, void* hip_stream);

/* ---- tuning and measurement -------------------------------------------------- */
/* Engine options (39 keys, plus the test hooks "handicap_next_bet", described at hg_map_begin, and "real_far_cursors" -- 0; 1: the real-valued
 * filter keeps its 64-bit slice cursors at any size, same results --; DESIGN.md section 9 lists every key with its
 * default and the test that sets it):
 *   geometry      "target_units" (16384: wavefront-sized units the pair passes are split into), "min_segment" (256 rows), "max_segments" (2048)
 *   the bet       "optimistic" (1: one-shot calls bet on a sampled threshold -- verified on the device, exact fallback), "sample_stride" (0 = auto: every
 *                 24th tile of 16 rows), "guess_sigma" (5: margin of the guess in standard deviations of the sampled count), "cand_budget_x10" (40: record
 *                 budget per query in tenths of R), "second_bet" (1: a lost bet is retried once with twice the margin before the exact sequence),
 *                 "cap_boost" (1..4096: multiplier of the slices' capacity; every database load sets it back to 1, lost bets raise it; raising it also
 *                 forgives the sharded bet just lost), "crowd_probe" (1: the first bet on a database measures how its near rows crowd and widens the slices)
 *   kernels       "select_mfma" (1: the pair passes of bet and exact sequence on the matrix cores; 0: vector-ALU xor + popcount -- same records),
 *                 "select_packed" (3: k_select_mx3 / k_select_mx4, several distances per accumulator, one-byte records; else k_select_mx),
 *                 "compact_records" (1: one-byte records {match, dist} when no ranked lists are wanted), "hist_mfma" (2: k_hist_i8; 1: k_hist_mx; 0: k_hist),
 *                 "rank_lds" (2: k_rank_lean where it applies, else k_rank_cnt; 1: k_rank_cnt; 0: k_rank_fused only), "rank_slices" (7000: smallest R whose
 *                 bet is ranked by k_rank_dense<slices>; 0: off), "rank_dense" (1: N/8 < R <= N through the byte matrix), "rank_dense_gbm" (-1: auto; 1 / 0:
 *                 its bitmap in global memory / LDS), "dense_budget_mb" (16384), "all_rows_shortcut" (1: R = N needs no histogram and no plan),
 *                 "fuse_ap" (1: the AP leaves from the rank kernel's epilogue), "inline_leftovers" (1: queries the rank kernel declined are ranked within
 *                 the next step's stream), "ap_recip" (1: the AP's division as three multiply-adds against correctly rounded reciprocals -- the same bits), "ap_wide" (1: k_ap with 512 threads per query when the queries are few and their lists long)
 *   staging       "stage_sync" (1; 0: staged calls and collectives only enqueue, see hg_set_stream), "defer_verdict" (0; 1: hg_rank does not wait for the
 *                 bet's verdict), "staged_lists" (1: the staged hg_select materialises the idx / dist lists), "step_graph" (0; 1: hg_map replays its
 *                 sequence as a hipGraph), "timing_every" (1: kernel timing brackets every n-th step)
 *   loading       "host_pack" (1: hg_set_*_f32 pack on the host's cores before the upload), "keep_floats" (hg_set_*_f32: 0 never / 1 always / 2 = only
 *                 if not a +-1 code: keep the float table on the device), "keep_query_floats" (0; 1: hg_set_queries_f32 / hg_set_queries_dev keep
 *                 the query float table whether or not the database's is there -- what hg_map_asym needs)
 *   real-valued   "real_mfma" (2: bf16 matrix-core filter + exact float32 rescoring; 1: every pair on the float32 matrix-core instruction; 0: vector
 *                 ALU), "real_sample_half" (1: the sampled cut's scores in the filter's 16-bit arithmetic -- they only place the cut; 0: exact float32 chains), "real_second_sample" (1: a second, counting sample four times as large tightens that cut), "real_sort_lds" (1: ranked by the LDS-resident kernel when the records fit), "real_groups" (1: lists beyond the LDS ordered group by group), "real_map_lists" (0; 1: hg_map_real also writes the ranked idx / score lists), "real_whole_rounds" (3: without a cut -- R = N -- the database is cut so that k_real_select_mx's blocks fill whole rounds of that many per CU; 0: the plain geometry)
 *   ("probe_select" and "probe_votes" exist only in the measurement build, python -m hashgan_amd.build --probes) */
int hg_set_option(hg_ctx* ctx, const char* key, int64_t value);
/* Counters and facts about the last call (39 keys; the process-wide "cache_*" and "host_*" keys are listed at hg_release_cache): "optimistic_runs", "optimistic_fallbacks" (all queries rerun exactly),
 * "optimistic_requeried" (single queries rerun exactly after losing their bet), "optimistic_rebets" (second and widened bets), "last_optimistic",
 * "rank_leftovers" (queries the LDS-resident rank kernel left to the general one), "select_variant" (1 k_select, 2 k_select_dense, 3 k_select_mx,
 * 5 k_select_mx3, 6 k_select_mx4), "rank_variant" (1 k_rank_fused, 3 k_rank_cnt, 6 k_rank_lean, 7 k_rank_dense, 8 k_rank_dense<slices>), "hist_variant" (the kernel of the last histogram pass, full or sampled: 1 k_hist, 2 k_hist_mx, 3 k_hist_i8; 6 / 7: k_hist_mx / k_hist_i8 with one dword counter per query tile instead of 16-bit halves; 0: no pass yet), "rank_lds_recs" (records the last k_rank_lean / k_rank_cnt launch had LDS room for), "slice_cap" (capacity of a (segment, query) slice of the last bet), "rel_hist_variant" (the kernel of the last hg_rel_hist: 1 k_hist_rel, the vector-ALU pass -- the only one so far, whatever "hist_mfma" says; 0: no pass yet), "ap_at_cutoffs" (cut-offs of the last hg_ap_at; 0: no pass yet), "votes_cutoffs" (cut-offs of the last hg_votes; 0: no pass yet), "joint_hist_grades" / "joint_hist_bands" (grades G and distance bands of the last hg_joint_hist; 0: no pass yet), "merged_joint_grades" (the common grade count Gc of the last joint hg_merge_side_table that succeeded; 0: none yet), "rel_hist_current" / "grade_hist_current" / "joint_hist_current" (1: this shard's table of the loaded queries and database is there -- what hg_pack_side_table needs), "ap_fused",
 * "cap_boost", "crowding_x100", "segments", "records_kept" (records the last bet's select left in the slices: a download, not part of a step),
 * "device_bytes" (every device buffer the context and its requery child hold, the second stream's workspace included), "graph_replays", "map_async_steps" / "map_async_redone" / "map_overlapped_steps" (hg_map_begin: steps enqueued blind / of those, run again by hg_map_end /
 * of those, run on the second stream);
 * "export_bytes" / "export_variant" (see hg_export);
 * "cut_beyond_planes" (1: the last hg_guess_finish met a query whose cut lies beyond the b/2 + 2 planes the owner-routed exchange carries -- its bet
 * cannot be won by wider slices; a download); real-valued path: "real_attempts", "real_requeried" (queries that lost the first cut and were ranked again on their own, cumulative), "real_cap_boost", "real_path" (bit 0 filter + rescoring, bit 1 ranked in LDS,
 * bit 2 lists ordered group by group), "asym_calls" / "asym_float_rows" (see hg_map_asym), "pq_calls" / "pq_float_rows" (see hg_map_pq); re-rank: "rerank_records", "rerank_chunks", "rerank_groups_lds", "rerank_groups_global" (see hg_topr_rerank). */
int hg_get_stat(hg_ctx* ctx, const char* key, int64_t* value);
/* What hg_set_database_f32 (queries = 0) / hg_set_queries_f32 (queries = 1) found in the float table: out[0] entries outside
 * {-1, 0, +1}, out[1] zeros, out[2] minus ones, out[3] = 1 if the float table is resident on the device -- from which the caller
 * tells +-1 codes (ranked by Hamming distance), {0,1} bits and real-valued features (ranked by inner product, metric.py:13) apart. */
int hg_get_census(hg_ctx* ctx, int queries, int64_t out[4]);
/* Work buffers only grow; hg_trim frees every device buffer except the loaded code/label/feature tables -- work buffers, the second
 * stream's workspace, the images and AP tables built from the tables (rebuilt on their next use) and the requery child context --, so
 * that stat "device_bytes" reports what the tables alone hold, and empties the process-wide block cache (hg_release_cache): the memory
 * goes back to the HIP runtime, e.g. for another framework in the same process. */
int hg_trim(hg_ctx* ctx);
/* Device blocks, pinned host blocks and streams that a destroyed or trimmed context gives up go to a process-wide cache and the
 * next context takes them from there instead of the HIP runtime (hipMalloc now and then stalls for SECONDS on this stack, a
 * stream costs 1.5 - 18 ms to create: a caller that builds a context per evaluation -- main.py:164 builds a MAPs object per
 * evaluation -- would pay that per call).  At most HG_CACHE_MB (49152: a sixth of the part's 288 GB) of device and HG_PIN_CACHE_MB (512) of pinned memory are
 * held; hg_release_cache returns all of it to the runtime.  Stats (any context): "cache_device_bytes", "cache_pinned_bytes",
 * "cache_hits", "cache_misses", "cache_streams"; "host_us_<phase>" / "host_n_<phase>" / "host_max_us_<phase>" with phase one of
 * init, devmalloc, devfree, hostmalloc, hostfree, destroy, stream, event, sync (waiting for the GPU), pack (host packing pass), thread
 * (starting the float table's staging thread): what the process has spent there.
 * The reference has no counterpart (lib/metric.py allocates NumPy arrays per call). */
int hg_release_cache(void);
/* Pay now what a context otherwise pays on first use of each path: the second stream and the pinned staging of the float
 * tables' uploads (hg_set_database_f32), the result block, the code objects of every translation unit (the runtime loads one
 * when a kernel of it is first launched), the host packing threads.  ~30 ms; hashgan_amd's MAPs pool calls it once per context
 * it creates, so that the first evaluation of ANOTHER shape or path in a process costs what the later ones do. */
int hg_preload(hg_ctx* ctx);
/* HIP-event timing of the kernels launched on the context's stream.  on = 2: every kernel; 1: only the
 * select pass over the query x database pairs (k_select, k_select_mx*: the roofline kernel) -- two events per launch keep
 * consecutive kernels from being dispatched back to back, ~4 us each; 0: off.  Levels 1 and 2 also time the
 * whole one-shot step on the GPU ("step_gpu_span": first enqueue to the last byte of the result download), so
 * wall time per step - step_gpu_span = what the host adds.  Inside a captured step the events are event-record
 * nodes of the graph.  Option "timing_every" = n (default 1) makes level 1 record on every n-th one-shot step only:
 * the events of a step cost it ~0.025 ms (1.04 -> 1.07 ms at 10k x 1M), sampling one step in four keeps the average
 * kernel duration live at a quarter of that. */
int hg_timing_enable(hg_ctx* ctx, int on);
int hg_timing_reset(hg_ctx* ctx);
/* Fills up to cap entries; name[i] points to static strings. Returns count via *n. */
int hg_timing_read(hg_ctx* ctx, int cap, const char** names, double* total_ms, int64_t* launches, int* n);

#ifdef __cplusplus
}
#endif
#endif /* HASHGAN_AMD_H */

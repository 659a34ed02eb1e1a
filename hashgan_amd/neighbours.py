"""Label-free relevance: the ground truth of a query is a set of database rows, not a class.

Everything else in this package calls a row relevant when it shares a label with the query (lib/metric.py:17-19).  Unsupervised
hashing (SH, ITQ and what followed), every ANN benchmark and binary-embedding quantisation have no labels: the ground truth of a
query is the set of its true nearest neighbours in the original feature space, and the question is how much of the exact float32
top G the Hamming top k recovers, with and without re-ranking.

The GPU does all of it (hashgan_amd._native): Context.topr_real gives the exact float32 top G, Context.neighbours_from_lists turns
the lists it left into sorted per-query id sets without a download (Context.set_neighbours takes sets from the host instead),
Context.match_neighbours rewrites the match bitmap of any later ranking from the sets, and Context.ap_at reads AP and hits at many
cut-offs from it.  Context.nbr_hist counts a query's neighbours per Hamming distance: with Context.rel_hist's `all` table, recall and
precision over the Hamming radius.  What comes to the host is [Q, len(ks)] tables; recall_from_tables and std_ap_from_tables are
the NumPy reductions alone.

The loaders want a label table: a call without labels loads a one-class all-zero one (no pair is label-relevant; nothing here reads
a label bit).
"""
import numpy as np

from . import _native, metric
from . import extra_metrics as X
from .devarray import DeviceArray, as_device_array

MAX_G = 16384                      # ids per set (hg_set_neighbours)
PAD = _native.IDX_NONE             # pads a set shorter than G
MODES = ("hamming", "rerank", "asymmetric", "features")


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(MODES), mode))
    return mode


def _check_G(G):
    if not 1 <= int(G) <= MAX_G:
        raise ValueError("G=%d ids per set: must be in 1..%d" % (int(G), MAX_G))
    return int(G)


def _check_sets(gt_ids, Q, N):
    """-> uint32 [Q, G]: one row per query, ids in 0..N-1 in any order, PAD (0xFFFFFFFF) filling a shorter set."""
    a = np.asarray(gt_ids)
    if a.ndim != 2 or a.dtype.kind not in "iu":
        raise ValueError("gt_ids must be an integer array [Q, G]")
    if a.shape[0] != Q:
        raise ValueError("gt_ids has %d rows for %d queries" % (a.shape[0], Q))
    _check_G(a.shape[1])
    a = a.astype(np.int64)
    if (a < 0).any():
        raise ValueError("gt_ids holds a negative id (0xFFFFFFFF pads a shorter set)")
    if ((a >= N) & (a != PAD)).any():
        raise ValueError("gt_ids holds an id outside the database (N=%d; 0xFFFFFFFF pads a shorter set)" % N)
    return a.astype(np.uint32)


def _check_tables(q, db, what="features"):
    if q.ndim != 2 or db.ndim != 2 or q.shape[1] != db.shape[1]:
        raise ValueError("query and database %s must be [n, b] with the same b" % what)


def _sides(x, what):
    """A table as the loaders take it: a DeviceArray descriptor (device memory) or an ndarray."""
    d = as_device_array(x)
    return d if d is not None else np.asarray(x)


def _no_labels(eng, x, slot):
    """The one-class all-zero label table of x's rows, on x's side (device: a scratch block of the engine's context)."""
    n = x.shape[0]
    if isinstance(x, DeviceArray):
        ptr = eng.ctx.scratch(slot, n)
        eng.ctx.memcpy_htod(ptr, np.zeros(n, np.uint8), n)
        return DeviceArray(ptr, (n, 1), None, "uint8")
    return np.zeros((n, 1), dtype=np.int64)


def _want_query_floats(eng, on):
    if eng.ctx.option_values.get("keep_query_floats", 0) != on:      # (set only when it changes, like metric._rank)
        eng.ctx.set_option("keep_query_floats", on)


def _load(eng, q, db, mode):
    """Both tables with empty labels, the floats each ranking of `mode` needs kept on the GPU.  mode "all": every float table
    (binary_vs_float ranks four ways on one context)."""
    if mode == "hamming":
        _want_query_floats(eng, 0)
        return X._load_sided(eng, q, db, _no_labels(eng, q, 2), _no_labels(eng, db, 3))
    if db.shape[1] > 255:
        raise ValueError("inner-product ranking supports up to 255 features (have %d)" % db.shape[1])
    _want_query_floats(eng, 1 if mode in ("asymmetric", "all") else 0)
    if mode == "features":
        metric._load_database(eng, db, _no_labels(eng, db, 3), "reference", floats=1)
    else:
        metric._load_database(eng, db, _no_labels(eng, db, 3), "rerank" if mode in ("rerank", "all") else "asymmetric")
    metric._set_queries(eng, q, _no_labels(eng, q, 2))
    return eng.ctx


def _rank(ctx, mode, R):
    """One ranking with its lists left on the device."""
    if mode == "hamming":
        ctx.topr(R)
    elif mode == "rerank":
        ctx.topr_rerank(R, download=False)
    elif mode == "asymmetric":
        ctx.topr_asym(R, download=False)
    else:
        ctx.topr_real(R, download=False)


def _tables_at(ctx, ks):
    """The neighbour match of the lists held now, then every cut-off -> (ap float64 [Q, nk], hits int64 [Q, nk])."""
    ctx.match_neighbours()
    ctx.ap_at(ks)
    return ctx.get_ap_at()


def recall_from_tables(hits, count):
    """recall@k from the device tables (NumPy only).  hits [Q, nk]: neighbours among the top k; count [Q]: n_q, the size of the
    query's set.  -> recall [nk]: the mean of hits / n_q over the queries with n_q > 0 (NaN if none has)."""
    hits = np.asarray(hits, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    if hits.ndim != 2 or count.shape != hits.shape[:1]:
        raise ValueError("hits must be a [Q, len(ks)] table and count [Q]")
    ok = count > 0
    if not ok.any():
        return np.full(hits.shape[1], np.nan)
    return (hits[ok] / count[ok, None]).mean(0)


def std_ap_from_tables(ap, hits, count, ks):
    """AP@k with the textbook normalisation from the device tables (NumPy only).  The reference's AP divides by the hits inside the
    top k (metric.py:22-23); the textbook's by min(n_q, k), the most hits the top k could hold: ap_std = ap * hits / min(n_q, k), 0
    where the top k hold no hit, NaN where the query has no neighbours.
    -> (map_std [nk]: the mean over the queries with n_q > 0, NaN if none has; ap_std [Q, nk])"""
    ks = np.asarray(ks, dtype=np.int64).ravel()
    ap = np.asarray(ap, dtype=np.float64)
    hits = np.asarray(hits, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    if ap.ndim != 2 or ap.shape != hits.shape or ap.shape[1] != ks.size or count.shape != ap.shape[:1]:
        raise ValueError("ap and hits must be [Q, len(ks)] tables and count [Q]")
    most = np.minimum(count[:, None], ks[None, :])
    ap_std = np.where(hits > 0, ap, 0.0) * hits / np.maximum(most, 1)      # (ap is NaN exactly where hits is 0)
    ap_std[count == 0] = np.nan
    ok = count > 0
    return (ap_std[ok].mean(0) if ok.any() else np.full(ks.size, np.nan)), ap_std


def metrics_from_tables(ap, hits, count, ks):
    """Everything neighbour_metrics_at_k returns, from the three device tables (NumPy only).
    -> dict(recall, precision, map, map_std [nk]; per_query=dict(hits, ap, ap_std [Q, nk], count [Q])): recall over the queries with
    n_q > 0; precision = the mean over ALL queries of hits / k; map = the reference's mean over the queries with a hit
    (metric.mean_over_hits, NaN when none has); map_std = std_ap_from_tables."""
    ks = X._check_ks(ks, None)
    ap = np.asarray(ap, dtype=np.float64)
    hits = np.asarray(hits, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    m = np.full(ks.size, np.nan)
    for j in range(ks.size):
        if (hits[:, j] != 0).any():
            m[j] = metric.mean_over_hits(np.ascontiguousarray(ap[:, j]), np.ascontiguousarray(hits[:, j]))
    map_std, ap_std = std_ap_from_tables(ap, hits, count, ks)
    precision = (hits / ks[None, :]).mean(0) if ap.shape[0] else np.full(ks.size, np.nan)
    return {"recall": recall_from_tables(hits, count), "precision": precision, "map": m, "map_std": map_std,
            "per_query": {"hits": hits, "ap": ap, "ap_std": ap_std, "count": count}}


def exact_neighbours(q_feat, db_feat, G, device=0):
    """The exact float32 inner-product top G of every query (Context.topr_real; ties by index) -> int64 [Q, G]."""
    db, q = _sides(db_feat, "database"), _sides(q_feat, "query")
    _check_tables(q, db)
    G = _check_G(G)
    if G > db.shape[0]:
        raise ValueError("G=%d exceeds the database's %d rows" % (G, db.shape[0]))
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q, db, "features")
        idx, _ = ctx.topr_real(G)
    return idx.astype(np.int64)


def neighbour_metrics_at_k(q, db, gt_ids, ks, mode="hamming", device=0):
    """recall@k, precision@k and mAP@k against ground-truth neighbour sets, from ONE ranking at max(ks).  gt_ids [Q, G] (host
    integers): row q holds the ids of query q's neighbours in any order, 0xFFFFFFFF padding a shorter set, G <= 16384.
    mode: "hamming" -- q / db are binary codes ({0,1} or +-1) ranked by Hamming distance, ties by index; "features" -- real-valued
    features by float32 inner product; "rerank" -- features, sign() codes by Hamming distance and the inner product inside equal
    distances; "asymmetric" -- the queries' features against the database's sign() codes read as +-1.  q / db: host arrays or
    device memory.  The ranking, the match against the sets (Context.match_neighbours) and the walk over the bitmap
    (Context.ap_at) run on the GPU.  -> metrics_from_tables' dict"""
    _check_mode(mode)
    db, q = _sides(db, "database"), _sides(q, "query")
    _check_tables(q, db, "codes" if mode == "hamming" else "features")
    ks = X._check_ks(ks, db.shape[0])
    gt = _check_sets(gt_ids, q.shape[0], db.shape[0])
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q, db, mode)
        ctx.set_neighbours(gt)
        _rank(ctx, mode, int(ks[-1]))
        ap, hits = _tables_at(ctx, ks)
        count = ctx.get_neighbours(ids=False)[1].astype(np.int64)
    return metrics_from_tables(ap, hits, count, ks)


def neighbour_radius_curves(q_codes, db_codes, gt_ids, device=0):
    """Recall and precision over the Hamming radius r = 0..b for neighbour relevance, no ranking: Context.nbr_hist counts the
    neighbours per distance, Context.rel_hist's `all` table the rows.  -> extra_metrics.curves_from_histograms' dict (total_rel = n_q)"""
    db, q = _sides(db_codes, "database"), _sides(q_codes, "query")
    _check_tables(q, db, "codes")
    gt = _check_sets(gt_ids, q.shape[0], db.shape[0])
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q, db, "hamming")
        ctx.set_neighbours(gt)
        ctx.nbr_hist()
        nbr, _ = ctx.get_nbr_hist()
        ctx.rel_hist()
        all_hist, _ = ctx.get_rel_hist()
    return X.curves_from_histograms(all_hist.T.astype(np.int64), nbr.T.astype(np.int64))


def binary_vs_float(q_feat, db_feat, G, ks, modes=("hamming", "rerank", "asymmetric"), device=0):
    """How much of the exact float32 top G do the binary rankings recover?  One context holds the features and their sign() codes:
    Context.topr_real(G) ranks exactly, Context.neighbours_from_lists(G) makes its lists the ground truth, then each mode ranks at
    max(ks) and is matched against it (neighbour_metrics_at_k's modes).  No list and no id set crosses to the host.
    -> {mode: metrics_from_tables' dict}"""
    modes = tuple(_check_mode(m) for m in modes)
    db, q = _sides(db_feat, "database"), _sides(q_feat, "query")
    _check_tables(q, db)
    G = _check_G(G)
    ks = X._check_ks(ks, db.shape[0])
    if G > db.shape[0]:
        raise ValueError("G=%d exceeds the database's %d rows" % (G, db.shape[0]))
    out = {}
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q, db, "all")
        ctx.topr_real(G, download=False)
        ctx.neighbours_from_lists(G)
        count = None
        for mode in modes:
            _rank(ctx, mode, int(ks[-1]))
            ap, hits = _tables_at(ctx, ks)
            if count is None:
                count = ctx.get_neighbours(ids=False)[1].astype(np.int64)
            out[mode] = metrics_from_tables(ap, hits, count, ks)
    return out

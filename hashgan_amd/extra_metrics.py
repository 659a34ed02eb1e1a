"""Other retrieval metrics on the ranked lists the path already produces.
Not in the reference (lib/metric.py only has mAP); these are the standard companions in the hashing
literature HashGAN's paper reports: precision/recall at the top k, and precision within Hamming
radius r.  The ranking, label matching and histograms run on the GPU (hashgan_amd._native); the
host only reduces small per-query vectors.

Everything a Hamming-ball lookup is judged by -- ball sizes, hits inside the ball, the recall denominator, for every radius at
once -- comes from one table: per query and distance d, the rows at distance d and how many of them share a label with the
query (Context.rel_hist, one pass over the pairs; no ranking, no lists, nothing of size Q x N on the host).

Graded relevance for multi-label data (NUS-WIDE, COCO): the grade of a retrieved row is the number of labels it shares with the
query, and ACG@k, NDCG@k and WAP@k are read from four [Q, len(ks)] tables the GPU sums along the ranked lists (Context.graded) and
the grade histogram of the whole database (Context.grade_hist), which stands for the ideal ordering: graded_relevance_at_k for
binary codes and for real-valued features, graded_from_tables for the reduction alone, grade_histograms for the table.

Tie-aware mAP (He, Cakir, Bargal, Sclaroff, "Hashing as Tie-Aware Learning to Rank", CVPR 2018): a b-bit code has b + 1 distances,
so AP@R depends on how the rows happen to be ordered inside each tie group.  tie_aware_map gives the expectation of the reference's
AP@R over all those orders, the probability that the top R hold a hit, and the exact minimum and maximum, per query -- a function
of the relevant-row histogram and R alone (Context.tie_ap), no ranking and no lists; tie_aware_precision_recall_at_k the expected
precision and recall at k from the same call.  Shuffling the database rows leaves every one of these bits unchanged.

Tie-aware graded relevance (the same paper defines tie-aware DCG / NDCG next to tie-aware AP): along the canonical list NDCG@k and ACG@k
depend on how the rows happen to be ordered inside each tie group.  tie_aware_graded_at_k gives their expectation over uniformly random
orders inside every group and the exact minimum and maximum, per query -- functions of one table, the rows per (distance, grade)
(Context.joint_hist, one pass over the pairs; distance_grade_histograms for the table, tie_graded_from_tables for the reduction alone).
Shuffling the database rows leaves every one of these bits unchanged.

Many cut-offs from one ranking: map_at_k gives mAP@k, precision@k and recall@k for up to 64 cut-offs -- binary codes or real-valued
features, host or device arrays -- from ONE ranking at max(ks): the top k is a prefix of the top max(ks), and Context.ap_at walks the
match bitmap that ranking left once per query for all of them (hg_ap_at; every AP with the bits a ranking at that k alone gives).
What comes to the host is two [Q, len(ks)] tables and the relevant-row histogram; map_from_ap_tables is the reduction alone.
precision_recall_at_k takes its hits from the same pass.

Ties resolved instead of described: rerank_topr ranks by Hamming distance and, inside equal distances, by the float32 inner product of
the features the codes were taken from (Context.topr_rerank) -- the lists, distances, scores and match bits of that order.

Which classes a query retrieved: knn_vote_at_k gives k-nearest-neighbour accuracy by majority vote of the retrieved labels, the
retrieval confusion matrix and precision@k by query class for up to 64 cut-offs from ONE ranking at max(ks) -- binary codes, real-valued
features or the re-ranked order.  Context.votes counts the label bits per class along the ranked lists on the GPU; a [Q, len(ks)] and a
[len(ks), C, C] table come to the host.  knn_from_tables is the reduction alone.
"""
import numpy as np

from . import metric


def _load_sided(eng, q_codes, db_codes, q_labels, db_labels):
    """_load for tables as metric._sides hands them over: host arrays or device descriptors."""
    metric._load_database(eng, db_codes, db_labels, "codes")
    qbad = metric._set_queries(eng, q_codes, q_labels)
    if qbad[1]:
        raise ValueError("labels must be {0,1} indicator matrices")
    qk, dk = metric._kind(eng.ctx, 1), eng.db_kind
    if not (qk == dk and qk in ("pm1", "bits")):
        raise ValueError("codes must be binary: all {-1,+1} or all {0,1} (found %s queries, %s database)" % (qk, dk))
    return eng.ctx


def _load(eng, q_codes, db_codes, q_labels, db_labels):
    """Binary codes only ({0,1} bits or +-1, the same spelling on both sides), like metric.MAP."""
    metric._load_database(eng, np.asarray(db_codes), np.asarray(db_labels), "codes")
    qbad = eng.ctx.set_queries_f32(np.asarray(q_codes), np.asarray(q_labels))
    if qbad[1]:
        raise ValueError("labels must be {0,1} indicator matrices")
    qk, dk = metric._kind(eng.ctx, 1), eng.db_kind
    if not (qk == dk and qk in ("pm1", "bits")):
        raise ValueError("codes must be binary: all {-1,+1} or all {0,1} (found %s queries, %s database)" % (qk, dk))
    return eng.ctx


def _tables(ctx):
    """The relevant-row histogram of the loaded tables -> (all, rel), int64 [Q, b+1]."""
    ctx.rel_hist()
    a, r = ctx.get_rel_hist()
    return a.T.astype(np.int64), r.T.astype(np.int64)


def lookup_histograms(q_codes, db_codes, q_labels, db_labels, device=0):
    """Per query and Hamming distance d: the database rows at distance d, and those of them that share a label with the
    query.  -> (all_hist, rel_hist), int64 [Q, b+1]"""
    eng = metric._Shared.get(device)
    with eng.lock:
        return _tables(_load(eng, q_codes, db_codes, q_labels, db_labels))


def curves_from_histograms(all_hist, rel_hist):
    """Lookup curves over the Hamming radius r = 0..b from the two tables (NumPy only).
    ball[q, r] = rows within r, hit[q, r] = relevant rows within r, total_rel[q] = hit[q, b];
    precision[r] = mean over ALL queries of hit / ball (0 where the ball is empty);
    recall[r] = mean of hit / total_rel over the queries that have relevant rows (NaN for every r if none has).
    -> dict(precision, recall, ball, hit, total_rel)"""
    all_hist = np.asarray(all_hist, dtype=np.int64)
    rel_hist = np.asarray(rel_hist, dtype=np.int64)
    if all_hist.ndim != 2 or all_hist.shape != rel_hist.shape:
        raise ValueError("all_hist and rel_hist must be [Q, b+1] tables of the same shape")
    ball = np.cumsum(all_hist, axis=1)
    hit = np.cumsum(rel_hist, axis=1)
    total_rel = hit[:, -1].copy()
    precision = np.where(ball > 0, hit / np.maximum(ball, 1), 0.0).mean(0)
    ok = total_rel > 0
    recall = (hit[ok] / total_rel[ok, None]).mean(0) if ok.any() else np.full(all_hist.shape[1], np.nan)
    return {"precision": precision, "recall": recall, "ball": ball, "hit": hit, "total_rel": total_rel}


def hamming_radius_curves(q_codes, db_codes, q_labels, db_labels, device=0):
    """The lookup P-R curve: (recall[r], precision[r]) for r = 0..b, with the per-query ball, hit and total_rel tables
    (curves_from_histograms of lookup_histograms)."""
    return curves_from_histograms(*lookup_histograms(q_codes, db_codes, q_labels, db_labels, device))


MAX_CLASSES = 255      # a grade is a byte on the GPU
MAX_CUTOFFS = metric.MAX_CUTOFFS


def _check_ks(ks, N):
    """-> int64 array; strictly ascending values in 1..N, at most MAX_CUTOFFS of them."""
    return metric._check_cutoffs(ks, N, "ks")


def gain_table(gain, C):
    """float64 [C + 1]: "exp" -> 2^g - 1, "linear" -> g, or the given C + 1 values; must be non-decreasing in g."""
    if C > MAX_CLASSES:
        raise ValueError("graded relevance takes up to %d classes (have %d)" % (MAX_CLASSES, C))
    if isinstance(gain, str):
        g = np.arange(C + 1, dtype=np.float64)
        if gain == "exp":
            tab = np.exp2(g) - 1.0
        elif gain == "linear":
            tab = g
        else:
            raise ValueError('gain must be "exp", "linear" or an array of C + 1 values')
    else:
        tab = np.array(gain, dtype=np.float64)
        if tab.shape != (C + 1,):
            raise ValueError("gain must have C + 1 = %d values" % (C + 1))
    if not np.isfinite(tab).all() or (np.diff(tab) < 0).any():
        raise ValueError("gain must be finite and non-decreasing in the grade")
    return tab


def discount_table(kmax):
    """float64 [kmax]: 1 / log2(1 + i) for the ranks i = 1..kmax."""
    return 1.0 / np.log2(np.arange(2, int(kmax) + 2, dtype=np.float64))


def _idcg(grade_hist, ks, gain, cum):
    """IDCG@k [Q, len(ks)]: the DCG of the database sorted by grade descending (graded_from_tables)."""
    Q, G = grade_hist.shape
    above = np.zeros(Q, dtype=np.int64)                                  # rows with a higher grade than the one being placed
    idcg = np.zeros((Q, ks.size), dtype=np.float64)
    for g in range(G - 1, -1, -1):
        start = np.minimum(above[:, None], ks[None, :])
        above = above + grade_hist[:, g]
        end = np.minimum(above[:, None], ks[None, :])
        idcg += gain[g] * (cum[end] - cum[start])
    return idcg


def graded_from_tables(gsum, hits, dcg, wsum, grade_hist, ks, gain, disc):
    """ACG@k, NDCG@k and WAP@k from the device tables (NumPy only).  gsum, hits, dcg, wsum: [Q, len(ks)] (Context.get_graded);
    grade_hist: [Q, C + 1] rows of the whole database per grade; gain [C + 1], disc [>= max(ks)] the tables the GPU was given.
    IDCG@k is the DCG of the database sorted by grade descending: walking the grades from C down, grade g occupies the next
    grade_hist[q, g] positions and contributes gain[g] times the discounts of those of them that lie within k -- O(Q C) per k.
    NDCG = DCG / IDCG (NaN where IDCG is 0), WAP = wsum / hits (NaN where hits is 0); means: ACG over all queries, NDCG over
    those with IDCG > 0, WAP over those with a hit within k, NaN when none is left.
    -> dict(acg, ndcg, wap [len(ks)], per_query=dict(acg, dcg, idcg, ndcg, wap, hits [Q, len(ks)], total_rel [Q]))"""
    grade_hist = np.asarray(grade_hist, dtype=np.int64)
    if grade_hist.ndim != 2:
        raise ValueError("grade_hist must be a [Q, C + 1] table")
    Q, G = grade_hist.shape
    gain = gain_table(gain, G - 1)
    ks = _check_ks(ks, None)
    disc = np.asarray(disc, dtype=np.float64)
    if disc.ndim != 1 or disc.size < ks[-1]:
        raise ValueError("disc must hold a discount for every rank up to max(ks)")
    gsum, hits = np.asarray(gsum, dtype=np.int64), np.asarray(hits, dtype=np.int64)
    dcg, wsum = np.asarray(dcg, dtype=np.float64), np.asarray(wsum, dtype=np.float64)
    for a in (gsum, hits, dcg, wsum):
        if a.shape != (Q, ks.size):
            raise ValueError("gsum, hits, dcg and wsum must be [Q, len(ks)] tables")
    cum = np.concatenate([[0.0], np.cumsum(disc[:ks[-1]])])             # cum[n] = discounts of the ranks 1..n
    idcg = _idcg(grade_hist, ks, gain, cum)
    has = idcg > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ndcg = np.where(has, dcg / idcg, np.nan)
        wap = np.where(hits > 0, wsum / hits, np.nan)
    acg = gsum / ks[None, :]

    def mean_where(x, ok):
        return np.array([x[ok[:, j], j].mean() if ok[:, j].any() else np.nan for j in range(ks.size)])

    return {"acg": acg.mean(0) if Q else np.full(ks.size, np.nan), "ndcg": mean_where(ndcg, has), "wap": mean_where(wap, hits > 0),
            "per_query": {"acg": acg, "dcg": dcg, "idcg": idcg, "ndcg": ndcg, "wap": wap, "hits": hits,
                          "total_rel": grade_hist[:, 1:].sum(1)}}


def _check_graded_inputs(q, db, q_labels, db_labels):
    q, db, q_labels, db_labels = np.asarray(q), np.asarray(db), np.asarray(q_labels), np.asarray(db_labels)
    metric._check_shapes(q, db, q_labels, db_labels, 1)
    if db_labels.shape[1] > MAX_CLASSES:
        raise ValueError("graded relevance takes up to %d classes (have %d)" % (MAX_CLASSES, db_labels.shape[1]))
    return q, db, q_labels, db_labels


def grade_histograms(q_codes, db_codes, q_labels, db_labels, device=0):
    """Per query and grade g = 0..C: the database rows that share exactly g labels with the query.  -> int64 [Q, C + 1]"""
    q_codes, db_codes, q_labels, db_labels = _check_graded_inputs(q_codes, db_codes, q_labels, db_labels)
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q_codes, db_codes, q_labels, db_labels)
        ctx.grade_hist()
        return ctx.get_grade_hist().T.astype(np.int64)


def graded_relevance_at_k(q, db, q_labels, db_labels, ks, gain="exp", features=False, device=0):
    """ACG@k, NDCG@k and WAP@k with grade = number of labels a retrieved row shares with the query, at the strictly ascending
    cut-offs ks (at most 64, each in 1..N).  gain: "exp" (2^g - 1), "linear" (g) or C + 1 non-decreasing values; the discount is
    1 / log2(1 + rank).  features=False: q and db are binary codes ({0,1} or +-1), ranked by Hamming distance, ties by index;
    features=True: real-valued features (up to 255), ranked by float32 inner product descending, ties by index, as
    MAPs.get_maps_by_feature ranks them.  The ranking, the sums along the lists and the grade histogram run on the GPU; nothing of
    size Q x k or Q x N comes to the host.  -> graded_from_tables' dict"""
    q, db, q_labels, db_labels = _check_graded_inputs(q, db, q_labels, db_labels)
    ks = _check_ks(ks, db.shape[0])
    tab = gain_table(gain, db_labels.shape[1])
    if features and db.shape[1] > 255:
        raise ValueError("inner-product ranking supports up to 255 features (have %d)" % db.shape[1])
    disc = discount_table(ks[-1])
    eng = metric._Shared.get(device)
    with eng.lock:
        if features:
            metric._load_database(eng, db, db_labels, "reference", floats=1)
            if eng.ctx.set_queries_f32(q, q_labels)[1]:
                raise ValueError("labels must be {0,1} indicator matrices")
            ctx = eng.ctx
            ctx.topr_real(int(ks[-1]), download=False)
        else:
            ctx = _load(eng, q, db, q_labels, db_labels)
            ctx.topr(int(ks[-1]))
        ctx.graded(ks, tab, disc)
        gsum, hits, dcg, wsum = ctx.get_graded()
        ctx.grade_hist()
        hist = ctx.get_grade_hist().T
    return graded_from_tables(gsum, hits, dcg, wsum, hist, ks, tab, disc)


def _joint_table(q_codes, db_codes, q_labels, db_labels, device):
    """The four arrays as metric._sides hands them over -> int64 [Q, b + 1, G]."""
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load_sided(eng, q_codes, db_codes, q_labels, db_labels)
        ctx.joint_hist()
        return np.ascontiguousarray(ctx.get_joint_hist().transpose(2, 0, 1)).astype(np.int64)


def _sided_graded_inputs(q_codes, db_codes, q_labels, db_labels):
    db_codes, db_labels = metric._sides(db_codes, db_labels, "database")
    q_codes, q_labels = metric._sides(q_codes, q_labels, "query")
    metric._check_shapes(q_codes, db_codes, q_labels, db_labels, 1)
    if db_labels.shape[1] > MAX_CLASSES:
        raise ValueError("graded relevance takes up to %d classes (have %d)" % (MAX_CLASSES, db_labels.shape[1]))
    return q_codes, db_codes, q_labels, db_labels


def distance_grade_histograms(q_codes, db_codes, q_labels, db_labels, device=0):
    """Per query, Hamming distance d = 0..b and grade g = 0..G-1: the database rows at distance d that share exactly g labels with
    the query.  G = 1 + min(most labels on a query, most labels on a database row): no pair has a higher grade.  Binary codes
    ({0,1} or +-1); every array may be a host array or lie in device memory, like map_at_k's.  One pass over the pairs on the GPU
    (Context.joint_hist); no ranking, no lists.  -> int64 [Q, b + 1, G]"""
    return _joint_table(*_sided_graded_inputs(q_codes, db_codes, q_labels, db_labels), device)


def tie_graded_from_tables(joint, ks, gain, disc):
    """Tie-aware DCG@k, NDCG@k and ACG@k from the distance-by-grade table (NumPy only).  joint: [Q, b + 1, G] rows per (distance,
    grade) of the whole database; ks: strictly ascending cut-offs; gain: "exp", "linear" or G non-decreasing values; disc [>= max(ks)]:
    non-increasing, non-negative discounts (disc[i - 1] for rank i) -- both envelope arguments need the monotonicity.
    Per query, with n_d = sum_g J[d][g] the size of tie group d, a_d the rows closer than d, m_d(k) = clamp(k - a_d, 0, n_d) the group's
    positions within k and cum[n] the discounts of the ranks 1..n, over uniformly random, independent orders inside every group:
      gsum_exp = sum_d m_d (sum_g g J[d][g]) / n_d,   acg = gsum_exp / k,   hits_exp = sum_d m_d (n_d - J[d][0]) / n_d,
      dcg      = sum_d (sum_g gain[g] J[d][g]) / n_d (cum[a_d + m_d] - cum[a_d])           (the expectations)
      dcg_max, gsum_hi   the group's m_d highest grades fill its positions within k in descending order,
      dcg_min, gsum_lo   its m_d lowest grades in ascending order; the groups are independent, so these are the exact extremes.
    idcg as graded_from_tables computes it, from the table summed over d; ndcg, ndcg_min, ndcg_max = dcg, dcg_min, dcg_max / idcg
    (NaN where idcg is 0).  Means: acg over all queries, ndcg over those with idcg > 0.  The order of every float addition is fixed by the
    query's table and ks (d ascending; inside a group g ascending, descending for the maximum): a query's results do not depend on Q.
    -> dict(acg, ndcg [len(ks)], per_query=dict(acg, acg_min, acg_max, dcg, dcg_min, dcg_max, idcg, ndcg, ndcg_min, ndcg_max,
    gsum_exp, gsum_lo, gsum_hi, hits_exp [Q, len(ks)], total_rel [Q]))"""
    joint = np.asarray(joint)
    if joint.ndim != 3 or joint.shape[2] < 1:
        raise ValueError("joint must be a [Q, b + 1, G] table")
    joint = joint.astype(np.int64)
    Q, NB, G = joint.shape
    gain = gain_table(gain, G - 1)
    ks = _check_ks(ks, None)
    disc = np.asarray(disc, dtype=np.float64)
    if disc.ndim != 1 or disc.size < ks[-1]:
        raise ValueError("disc must hold a discount for every rank up to max(ks)")
    disc = disc[:ks[-1]]
    if not np.isfinite(disc).all() or (disc < 0).any() or (np.diff(disc) > 0).any():
        raise ValueError("disc must be finite, non-negative and non-increasing in the rank")
    nk = ks.size
    cum = np.concatenate([[0.0], np.cumsum(disc)])                       # cum[n] = discounts of the ranks 1..n
    grades = np.arange(G, dtype=np.int64)
    f = {k: np.zeros((Q, nk), dtype=np.float64) for k in ("gsum_exp", "hits_exp", "dcg", "dcg_min", "dcg_max")}
    gsum_lo, gsum_hi = np.zeros((Q, nk), dtype=np.int64), np.zeros((Q, nk), dtype=np.int64)
    a = np.zeros(Q, dtype=np.int64)                                      # rows closer than d

    def expected(m, n, s):
        """m s / n: what m of the group's n rows, drawn uniformly, are expected to add up to when all n add up to s (s when m = n)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            part = m.astype(np.float64) * s[:, None].astype(np.float64) / n[:, None].astype(np.float64)
        return np.where(m == n[:, None], s[:, None].astype(np.float64), np.where(m > 0, part, 0.0))

    for d in range(NB):
        J = joint[:, d, :]
        n = J.sum(1)
        start = np.minimum(a[:, None], ks[None, :])
        m = np.minimum((a + n)[:, None], ks[None, :]) - start            # the group's positions within k
        a = a + n
        if not m.any():
            continue
        f["gsum_exp"] += expected(m, n, (J * grades[None, :]).sum(1))
        f["hits_exp"] += expected(m, n, n - J[:, 0])
        w = np.zeros(Q, dtype=np.float64)
        for g in range(G):
            w = w + gain[g] * J[:, g]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(n > 0, w / n, 0.0)
        f["dcg"] += w[:, None] * (cum[start + m] - cum[start])
        for name, gs, order in (("dcg_min", gsum_lo, range(G)), ("dcg_max", gsum_hi, range(G - 1, -1, -1))):
            left, pos = m.copy(), start.copy()
            for g in order:
                take = np.minimum(J[:, g][:, None], left)
                f[name] += gain[g] * (cum[pos + take] - cum[pos])
                gs += g * take
                pos += take
                left -= take
    hist = joint.sum(1)
    idcg = _idcg(hist, ks, gain, cum)
    has = idcg > 0
    pq = {"acg": f["gsum_exp"] / ks[None, :], "acg_min": gsum_lo / ks[None, :], "acg_max": gsum_hi / ks[None, :],
          "dcg": f["dcg"], "dcg_min": f["dcg_min"], "dcg_max": f["dcg_max"], "idcg": idcg}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in ("ndcg", "ndcg_min", "ndcg_max"):
            pq[name] = np.where(has, pq[name[1:]] / idcg, np.nan)
    pq.update(gsum_exp=f["gsum_exp"], gsum_lo=gsum_lo, gsum_hi=gsum_hi, hits_exp=f["hits_exp"], total_rel=hist[:, 1:].sum(1))
    ndcg = np.array([pq["ndcg"][has[:, j], j].mean() if has[:, j].any() else np.nan for j in range(nk)])
    return {"acg": pq["acg"].mean(0) if Q else np.full(nk, np.nan), "ndcg": ndcg, "per_query": pq}


def tie_aware_graded_at_k(q_codes, db_codes, q_labels, db_labels, ks, gain="exp", device=0):
    """Tie-aware ACG@k and NDCG@k of a Hamming ranking with grade = number of labels a row shares with the query, at the strictly
    ascending cut-offs ks (at most 64, each in 1..N): per query the expectation over uniformly random orders inside every group of
    rows at equal distance, and the exact minimum and maximum over all those orders -- where graded_relevance_at_k reports the one
    order "by database index".  gain: "exp" (2^g - 1), "linear" (g) or C + 1 non-decreasing values; the discount is 1 / log2(1 + rank).
    Binary codes ({0,1} or +-1); every array may be a host array or lie in device memory, like map_at_k's.  One pass over the pairs
    on the GPU (Context.joint_hist) and a NumPy reduction of its [Q, b + 1, G] table: no ranking, no lists, nothing of size Q x N or
    Q x k on the host.  Out of scope: tie-aware WAP (its expectation is AP-shaped and needs tie_aware_map's machinery on the device);
    real-valued features (an inner-product ranking has no tie groups to average over); a matrix-core form of the pass (LDS atomics
    bound every histogram here).  -> tie_graded_from_tables' dict"""
    q_codes, db_codes, q_labels, db_labels = _sided_graded_inputs(q_codes, db_codes, q_labels, db_labels)
    ks = _check_ks(ks, db_codes.shape[0])
    tab = gain_table(gain, db_labels.shape[1])
    disc = discount_table(ks[-1])
    joint = _joint_table(q_codes, db_codes, q_labels, db_labels, device)
    return tie_graded_from_tables(joint, ks, tab[:joint.shape[2]], disc)


def _tie_tables(q_codes, db_codes, q_labels, db_labels, Rs, device):
    """-> (Rs int64, Context.get_tie_ap()'s dict, total_rel int64 [Q]); argument errors before any GPU use."""
    q_codes, db_codes, q_labels, db_labels = np.asarray(q_codes), np.asarray(db_codes), np.asarray(q_labels), np.asarray(db_labels)
    metric._check_shapes(q_codes, db_codes, q_labels, db_labels, 1)
    Rs = _check_ks(Rs, db_codes.shape[0])
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q_codes, db_codes, q_labels, db_labels)
        ctx.tie_ap(Rs)                                                   # (runs the histogram pass: the tables are new)
        t = ctx.get_tie_ap()
        total_rel = ctx.get_rel_hist()[1].astype(np.int64).sum(0)
    return Rs, t, total_rel


def map_from_tie_tables(ap, p_hit):
    """map[j] = sum_q p_hit * ap / sum_q p_hit over the queries with p_hit > 0, NaN when the denominator is 0 (NumPy only; tie_aware_map's
    docstring says what it is the expectation of).  ap, p_hit: [Q, nR] (Context.get_tie_ap).  -> float64 [nR]"""
    w = p_hit
    den = w.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(den > 0, np.where(w > 0, w * ap, 0.0).sum(0) / den, np.nan)
    return m


def tie_map_from_tables(t, total_rel):
    """tie_aware_map's dict from Context.get_tie_ap()'s tables and the relevant rows of the whole database per query (NumPy only)."""
    pq = dict(t)
    pq["total_rel"] = total_rel
    return {"map": map_from_tie_tables(t["ap"], t["p_hit"]), "per_query": pq}


def tie_precision_recall_from_tables(rel_exp, total_rel, ks):
    """tie_aware_precision_recall_at_k's two means from rel_exp [Q, len(ks)] and total_rel [Q] (NumPy only)."""
    precision = (rel_exp / ks[None, :]).mean(0)
    ok = total_rel > 0
    recall = (rel_exp[ok] / total_rel[ok, None]).mean(0) if ok.any() else np.full(len(ks), np.nan)
    return precision, recall


def tie_aware_map(q_codes, db_codes, q_labels, db_labels, Rs, device=0):
    """Tie-aware mAP@R of a Hamming ranking at the strictly ascending cut-offs Rs (at most 64, each in 1..N), binary codes
    ({0,1} or +-1).  Per query and R, over uniformly random orders inside every group of rows at equal distance:
      ap       the expectation of the reference's AP@R given that the top R hold a relevant row (NaN when they never do),
      p_hit    the probability that they do (the reference skips a query whose top R hold none),
      ap_min, ap_max   the exact extremes of AP@R over all those orders (NaN when no order has a hit),
      rel_exp, rel_lo, rel_hi   expectation and extremes of the number of relevant rows among the top R,
      total_rel   relevant rows in the whole database.
    The per-query values are exact (float64 rounding aside).  map[j] = sum_q p_hit * ap / sum_q p_hit (NaN when the denominator is
    0): the reference's mAP is the mean of AP over the queries that have a hit, so whenever every p_hit is 0 or 1 -- the set of
    averaged queries does not depend on the order -- map[j] IS the expectation of the reference's mAP@R over the tie orders; with a
    p_hit strictly between 0 and 1 the number of averaged queries is itself random and map[j] is the ratio of the expectations
    of the reference's numerator and denominator, not the expectation of their ratio.
    -> dict(map [nR], per_query=dict(ap, p_hit, ap_min, ap_max, rel_exp, rel_lo, rel_hi [Q, nR], total_rel [Q]))"""
    Rs, t, total_rel = _tie_tables(q_codes, db_codes, q_labels, db_labels, Rs, device)
    return tie_map_from_tables(t, total_rel)


def tie_aware_precision_recall_at_k(q_codes, db_codes, q_labels, db_labels, ks, device=0):
    """Expected precision@k and recall@k over the tie orders of a Hamming ranking: per query rel_exp / k and rel_exp / total_rel
    with rel_exp the expected number of relevant rows among the top k, averaged like precision_recall_at_k does -- precision over
    all queries, recall over the queries that have relevant rows in the whole database (NaN if none has).  ks: strictly ascending,
    at most 64, each in 1..N.  The same device call as tie_aware_map: no ranking, no lists.
    -> (precision [len(ks)], recall [len(ks)])"""
    ks, t, total_rel = _tie_tables(q_codes, db_codes, q_labels, db_labels, ks, device)
    return tie_precision_recall_from_tables(t["rel_exp"], total_rel, ks)


def _ap_at_tables(q, db, q_labels, db_labels, ks, features, device):
    """One ranking at ks[-1] (ks: strictly ascending int64, any number of them: passes of 64), every cut-off from its match
    bitmap.  The four arrays as metric._sides hands them over.  -> (ap float64 [Q, nk], hits int64 [Q, nk], total_rel int64 [Q])"""
    eng = metric._Shared.get(device)
    with eng.lock:
        if features:
            metric._load_database(eng, db, db_labels, "reference", floats=1)
            if metric._set_queries(eng, q, q_labels)[1]:
                raise ValueError("labels must be {0,1} indicator matrices")
            ctx = eng.ctx
            ctx.topr_real(int(ks[-1]), download=False)                   # ranked once; the lists stay on the device
        else:
            ctx = _load_sided(eng, q, db, q_labels, db_labels)
            ctx.topr(int(ks[-1]))
        ap, hits = [], []
        for i in range(0, len(ks), MAX_CUTOFFS):
            ctx.ap_at(ks[i:i + MAX_CUTOFFS])
            a, h = ctx.get_ap_at()
            ap.append(a)
            hits.append(h)
        total_rel = _tables(ctx)[1].sum(1)                               # relevant rows in the whole database, per query (a device table)
    return np.concatenate(ap, axis=1), np.concatenate(hits, axis=1), total_rel


def map_from_ap_tables(ap, hits, total_rel, ks):
    """mAP@k, precision@k and recall@k from the device tables (NumPy only).  ap [Q, len(ks)]: AP@k per query, NaN where the top k
    hold no hit; hits [Q, len(ks)]: relevant rows among the top k; total_rel [Q]: relevant rows in the whole database.
    map[j] = metric.mean_over_hits of column j -- the reference's mean over the queries with a hit (metric.py:22-24), NaN when none
    has; precision[j] = mean over ALL queries of hits / k; recall[j] = mean of hits / total_rel over the queries that have
    relevant rows (NaN if none has): precision_recall_at_k's conventions.
    -> dict(map, precision, recall [len(ks)], per_query=dict(ap, hits [Q, len(ks)], total_rel [Q]))"""
    ks = _check_ks(ks, None)
    ap = np.asarray(ap, dtype=np.float64)
    hits = np.asarray(hits, dtype=np.int64)
    total_rel = np.asarray(total_rel, dtype=np.int64)
    if ap.ndim != 2 or ap.shape != hits.shape or ap.shape[1] != ks.size or total_rel.shape != ap.shape[:1]:
        raise ValueError("ap and hits must be [Q, len(ks)] tables and total_rel [Q]")
    m = np.full(ks.size, np.nan)
    for j in range(ks.size):
        if (hits[:, j] != 0).any():
            m[j] = metric.mean_over_hits(np.ascontiguousarray(ap[:, j]), np.ascontiguousarray(hits[:, j]))
    precision = (hits / ks[None, :]).mean(0) if ap.shape[0] else np.full(ks.size, np.nan)
    ok = total_rel > 0
    recall = (hits[ok] / total_rel[ok, None]).mean(0) if ok.any() else np.full(ks.size, np.nan)
    return {"map": m, "precision": precision, "recall": recall, "per_query": {"ap": ap, "hits": hits, "total_rel": total_rel}}


def map_at_k(q, db, q_labels, db_labels, ks, features=False, device=0):
    """mAP@k, precision@k and recall@k at the strictly ascending cut-offs ks (at most 64, each in 1..N) from ONE ranking at max(ks).
    features=False: q and db are binary codes ({0,1} or +-1), ranked by Hamming distance, ties by index, like MAP;
    features=True: real-valued features (up to 255), ranked by float32 inner product descending, ties by index, like
    MAPs.get_maps_by_feature.  Every array may be a host array or lie in device memory (a torch tensor on the device, anything with
    __cuda_array_interface__, a DeviceArray; the two arrays of one table on the same side).  AP@k of every query has the bits
    MAP_per_query / Context.map_real give at R = k.  The ranking, the walk over the match bitmap (Context.ap_at) and the recall
    denominator (Context.rel_hist) run on the GPU; two [Q, len(ks)] tables come to the host.  -> map_from_ap_tables' dict"""
    db, db_labels = metric._sides(db, db_labels, "database")
    q, q_labels = metric._sides(q, q_labels, "query")
    metric._check_shapes(q, db, q_labels, db_labels, 1)
    ks = _check_ks(ks, db.shape[0])
    if features and db.shape[1] > 255:
        raise ValueError("inner-product ranking supports up to 255 features (have %d)" % db.shape[1])
    ap, hits, total_rel = _ap_at_tables(q, db, q_labels, db_labels, ks, features, device)
    return map_from_ap_tables(ap, hits, total_rel, ks)


def precision_recall_at_k(q_codes, db_codes, q_labels, db_labels, ks, device=0, features=False):
    """Mean precision@k and recall@k over the queries, Hamming ranking with the canonical tie order (features=True: real-valued
    features ranked by inner product, like map_at_k).  recall uses the number of relevant rows in the WHOLE database; queries
    without any are skipped for recall.  ks: any number of cut-offs in any order, repeats allowed; the results are in ascending
    order of k.  Ranked once at max(ks); the hits at every k come from one walk over the match bitmap per 64 distinct cut-offs
    (Context.ap_at): nothing of size Q x k on the host.  -> (precision [len(ks)], recall [len(ks)])"""
    ks = np.asarray(sorted(int(k) for k in ks), dtype=np.int64)
    db_codes, db_labels = metric._sides(db_codes, db_labels, "database")
    q_codes, q_labels = metric._sides(q_codes, q_labels, "query")
    N = db_codes.shape[0]
    if ks[0] < 1 or ks[-1] > N:
        raise ValueError("every k must be in 1..N")
    if features and db_codes.shape[1] > 255:
        raise ValueError("inner-product ranking supports up to 255 features (have %d)" % db_codes.shape[1])
    uniq, back = np.unique(ks, return_inverse=True)
    _, hits, total_rel = _ap_at_tables(q_codes, db_codes, q_labels, db_labels, uniq, features, device)
    hits = hits[:, back]
    precision = (hits / ks[None, :]).mean(0)
    ok = total_rel > 0
    recall = (hits[ok] / total_rel[ok, None]).mean(0) if ok.any() else np.full(len(ks), np.nan)
    return precision, recall


def precision_within_radius(q_codes, db_codes, q_labels, db_labels, radius=2, device=0):
    """Mean precision of Hamming-ball lookups: for every query, the fraction of database rows within
    `radius` that share a label with it; a query whose ball is empty contributes 0 (the usual
    convention).  -> (mean precision, per-query ball sizes)"""
    eng = metric._Shared.get(device)
    with eng.lock:
        all_hist, rel_hist = _tables(_load(eng, q_codes, db_codes, q_labels, db_labels))
    ball = all_hist[:, :radius + 1].sum(1)                               # rows within the radius, per query
    if ball.max() == 0:
        return 0.0, ball
    hits = rel_hist[:, :radius + 1].sum(1)
    prec = np.where(ball > 0, hits / np.maximum(ball, 1), 0.0)
    return float(prec.mean()), ball


def rerank_topr(q, db, q_labels, db_labels, R, device=0):
    """The Hamming ranking with its tie groups resolved by the features (hg_topr_rerank): sign() gives the codes, rows are ranked by
    (Hamming distance ascending, float32 inner product of the features descending, database index ascending) and the top R kept -- of
    the threshold distance's rows the ones with the highest inner product.  q / db: real-valued features [n, b] (b <= 255, at most
    2^24 database rows), host or device arrays.
    -> (idx uint32 [Q, R], dist uint8 [Q, R], scores float32 [Q, R], match uint8 [Q, R])"""
    db, db_labels = metric._sides(db, db_labels, "database")
    q, q_labels = metric._sides(q, q_labels, "query")
    metric._check_shapes(q, db, q_labels, db_labels, int(R))
    eng = metric._Shared.get(device)
    with eng.lock:
        metric._load_database(eng, db, db_labels, "rerank")
        if metric._set_queries(eng, q, q_labels)[1]:
            raise ValueError("labels must be {0,1} indicator matrices")
        idx, dist, scores = eng.ctx.topr_rerank(int(R))
        match = eng.ctx.get_match()
    return idx, dist, scores, match


def knn_from_tables(pred, conf, q_labels, ks):
    """k-nearest-neighbour accuracy and the retrieval confusion matrix from the device tables (NumPy only).  pred [Q, len(ks)]: the
    majority class among the top k per query, -1 where no retrieved row has a label (Context.get_vote_pred); conf [len(ks), C, C]:
    conf[j, a, b] = rows of class b among the top ks[j] of the queries that carry class a (Context.get_vote_confusion); q_labels
    [Q, C]: the queries' {0,1} labels.  A prediction is right when it is one of the query's labels; -1 is wrong.
      accuracy [len(ks)]               share of right predictions over the queries with at least one label (NaN if there is none),
      per_class_accuracy [len(ks), C]  the same over the queries that carry class a (NaN where no query does),
      confusion [len(ks), C, C]        conf as int64,
      class_precision [len(ks), C]     conf[j, a, a] / (ks[j] n_a), n_a the queries that carry a: on single-label data the mean
                                       precision@k of the queries of class a (NaN where n_a = 0),
      ks                               the cut-offs as int64.
    -> dict(accuracy, per_class_accuracy, confusion, class_precision, ks)"""
    ks = _check_ks(ks, None)
    pred = np.asarray(pred)
    conf = np.asarray(conf)
    lab = np.asarray(q_labels) != 0
    if lab.ndim != 2 or pred.ndim != 2 or pred.shape != (lab.shape[0], ks.size) or pred.dtype.kind not in "iu":
        raise ValueError("pred must be an integer [Q, len(ks)] table and q_labels [Q, C]")
    Q, C = lab.shape
    if conf.shape != (ks.size, C, C) or conf.dtype.kind not in "iu":
        raise ValueError("conf must be an integer [len(ks), C, C] table")
    pred = pred.astype(np.int64)
    if pred.size and (pred.min() < -1 or pred.max() >= C):
        raise ValueError("pred must hold classes 0..C-1 or -1")
    conf = conf.astype(np.int64)
    right = np.zeros((Q, ks.size), dtype=bool)
    if pred.size:
        right = (pred >= 0) & lab[np.arange(Q)[:, None], np.maximum(pred, 0)]
    labelled = lab.any(1)
    n_lab = int(labelled.sum())
    n_a = lab.sum(0).astype(np.int64)                                    # queries that carry class a
    hits_a = right.astype(np.int64).T @ lab.astype(np.int64)             # [nk, C]: right predictions among them
    with np.errstate(divide="ignore", invalid="ignore"):
        accuracy = right[labelled].sum(0) / n_lab if n_lab else np.full(ks.size, np.nan)
        per_class = np.where(n_a[None, :] > 0, hits_a / n_a[None, :], np.nan)
        diag = conf[:, np.arange(C), np.arange(C)]
        precision = np.where(n_a[None, :] > 0, diag / (ks[:, None] * n_a[None, :]), np.nan)
    return {"accuracy": accuracy, "per_class_accuracy": per_class, "confusion": conf, "class_precision": precision, "ks": ks}


def _check_vote_inputs(q, db, q_labels, db_labels, ks, features):
    """knn_vote_at_k's argument checks (graded_relevance_at_k's), before any GPU use -> the four arrays and ks as int64."""
    q, db, q_labels, db_labels = np.asarray(q), np.asarray(db), np.asarray(q_labels), np.asarray(db_labels)
    metric._check_shapes(q, db, q_labels, db_labels, 1)
    if db_labels.shape[1] > MAX_CLASSES:
        raise ValueError("class votes take up to %d classes (have %d)" % (MAX_CLASSES, db_labels.shape[1]))
    ks = _check_ks(ks, db.shape[0])
    if features and db.shape[1] > 255:
        raise ValueError("inner-product ranking supports up to 255 features (have %d)" % db.shape[1])
    return q, db, q_labels, db_labels, ks


def _vote_tables(ctx, ks):
    """votes() on the lists the context holds and the two small getters -> (pred int32 [Q, nk], conf int64 [nk, C, C])."""
    ctx.votes(ks)
    return ctx.get_vote_pred()[0], ctx.get_vote_confusion()


def knn_vote_at_k(q, db, q_labels, db_labels, ks, features=False, rerank=False, device=0):
    """k-nearest-neighbour classification by majority vote of the retrieved labels, and the retrieval confusion matrix, at the
    strictly ascending cut-offs ks (at most 64, each in 1..N; up to 255 classes) from ONE ranking at max(ks).  features=False: q and
    db are binary codes ({0,1} or +-1) ranked by Hamming distance, ties by index; features=True: real-valued features (up to 255)
    ranked by float32 inner product descending, as MAPs.get_maps_by_feature ranks them; rerank=True: real-valued features, sign()
    gives the codes and the inner product orders the rows inside equal Hamming distances, as rerank_topr ranks them.  A query's
    prediction at k is the class most of its top k rows carry (the smallest such class; none when no retrieved row has a label).
    The ranking, the votes (Context.votes) and the confusion matrix run on the GPU; what comes to the host is a [Q, len(ks)] and a
    [len(ks), C, C] table, nothing of size Q x k.  -> knn_from_tables' dict"""
    q, db, q_labels, db_labels, ks = _check_vote_inputs(q, db, q_labels, db_labels, ks, features or rerank)
    eng = metric._Shared.get(device)
    with eng.lock:
        if rerank:
            metric._load_database(eng, db, db_labels, "rerank")
            if metric._set_queries(eng, q, q_labels)[1]:
                raise ValueError("labels must be {0,1} indicator matrices")
            ctx = eng.ctx
            ctx.topr_rerank(int(ks[-1]), download=False)
        elif features:
            metric._load_database(eng, db, db_labels, "reference", floats=1)
            if eng.ctx.set_queries_f32(q, q_labels)[1]:
                raise ValueError("labels must be {0,1} indicator matrices")
            ctx = eng.ctx
            ctx.topr_real(int(ks[-1]), download=False)
        else:
            ctx = _load(eng, q, db, q_labels, db_labels)
            ctx.topr(int(ks[-1]))
        pred, conf = _vote_tables(ctx, ks)
    return knn_from_tables(pred, conf, q_labels, ks)


def rank_into(q, db, q_labels, db_labels, R, features=False, rerank=False, device=0, stream=None, **outs):
    """Rank and write the results into arrays of the caller's in GPU memory (MAPs.rank_into, query first): outs are idx, dist, score,
    match [Q, k <= R] and ap, hits [Q] or [Q, 1] -- torch tensors on the device, anything with __cuda_array_interface__ or
    devarray.DeviceOut; `stream` is the consumer's HIP stream.  features=False: q and db are binary codes ({0,1} or +-1) ranked by
    Hamming distance like MAP; features=True: what MAPs(R) ranks (real-valued features by float32 inner product); rerank=True: what
    MAPs(R, rerank=True) ranks (sign(), Hamming distance, then the inner product inside equal distances).  Inputs may be host or device
    arrays.  -> {"by": "hamming" | "inner_product" | "rerank", "R": R}"""
    unknown = set(outs) - set(metric.OUT_NAMES)
    if unknown:
        raise TypeError("rank_into: unknown destination %s (known: %s)" % (", ".join(sorted(unknown)), ", ".join(metric.OUT_NAMES)))
    db, db_labels = metric._sides(db, db_labels, "database")
    q, q_labels = metric._sides(q, q_labels, "query")
    R = int(R)
    metric._check_shapes(q, db, q_labels, db_labels, R)
    dsts = metric._check_outs(outs, q.shape[0], db.shape[0], R, stream)
    mode = "rerank" if rerank else "reference" if features else "codes"
    eng = metric._Shared.get(device)
    with eng.lock:
        metric._load_database(eng, db, db_labels, mode)
        return metric._rank_into(eng, q, q_labels, R, mode, dsts)

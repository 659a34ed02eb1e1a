"""Other retrieval metrics on the ranked lists the path already produces.
Not in the reference (lib/metric.py only has mAP); these are the standard companions in the hashing
literature HashGAN's paper reports: precision/recall at the top k, and precision within Hamming
radius r.  The ranking, label matching and histograms run on the GPU (hashgan_amd._native); the
host only reduces small per-query vectors.

Everything a Hamming-ball lookup is judged by -- ball sizes, hits inside the ball, the recall denominator, for every radius at
once -- comes from one table: per query and distance d, the rows at distance d and how many of them share a label with the
query (Context.rel_hist, one pass over the pairs; no ranking, no lists, nothing of size Q x N on the host).
"""
import numpy as np

from . import metric


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


def precision_recall_at_k(q_codes, db_codes, q_labels, db_labels, ks, device=0):
    """Mean precision@k and recall@k over the queries, Hamming ranking with the canonical tie order.
    recall uses the number of relevant rows in the WHOLE database; queries without any are skipped
    for recall.  -> (precision [len(ks)], recall [len(ks)])"""
    ks = np.asarray(sorted(int(k) for k in ks), dtype=np.int64)
    N = np.asarray(db_codes).shape[0]
    if ks[0] < 1 or ks[-1] > N:
        raise ValueError("every k must be in 1..N")
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = _load(eng, q_codes, db_codes, q_labels, db_labels)
        ctx.topr(int(ks[-1]))                                            # ranked once, for the hits at k
        match = ctx.get_match()
        total_rel = _tables(ctx)[1].sum(1)                               # relevant rows in the whole database, per query
    cum = np.cumsum(match.astype(np.int64), axis=1)                      # [Q, kmax]
    hits = cum[:, ks - 1]
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

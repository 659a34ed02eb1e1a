"""Brute-force NumPy statements of the list metrics and the histogram passes, shared by the per-feature GPU files and by the
second-hand-memory matrix (tests/test_second_hand_gpu.py).  Each was written next to the feature it checks and moved here unchanged;
nothing below is derived from the library's own results.  Not a test."""
import warnings

import numpy as np

from oracle import hamming_map as O
from oracle import real_map as RM
from tests import tie_oracle as T


def hamming(qb, db):
    """Q x N Hamming distances: +-1 products in float32 are exact for any code length here."""
    b = qb.shape[1]
    ip = (2.0 * qb.astype(np.float32) - 1.0) @ (2.0 * db.astype(np.float32) - 1.0).T
    return ((b - ip) / 2).astype(np.int64)


def ranked_by(key):
    """np.lexsort((index, key)) per query: key ascending, then index ascending."""
    return np.argsort(key, axis=1, kind="stable")


def pair_grades(ql, dl):
    return ql.astype(np.int64) @ dl.astype(np.int64).T


# ------------------------------------------------------------------ inner-product rankings (tests/test_pq_gpu.py, tests/test_asym_gpu.py)
def real_lists(qf, x, ql, dl, R):
    """oracle.real_map on the float table x -> (ap float64 [Q], idx, score float32 [Q, R], match uint8 [Q, R], rel int64 [Q])."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, idx, score = RM.map_from_features(qf, x, ql.astype(np.int8), dl.astype(np.int8), R)
    match = (dl[idx].astype(bool) & ql[:, None, :].astype(bool)).any(-1)
    return ap, idx, score, match.astype(np.uint8), match.sum(1).astype(np.int64)


# ------------------------------------------------------------------ hg_ap_at (tests/test_ap_at_gpu.py)
def ap_at_oracle(imatch, Rs):
    """imatch bool [Q, >= max(Rs)] in canonical order -> (ap float64 [Q, nR] with nan for skipped queries, rel int64 [Q, nR])."""
    Q = imatch.shape[0]
    ap, rel = np.full((Q, len(Rs)), np.nan), np.zeros((Q, len(Rs)), np.int64)
    for q in range(Q):
        for j, R in enumerate(Rs):
            a, r = O.average_precision(imatch[q, :R], int(R))
            rel[q, j] = r
            if a is not None:
                ap[q, j] = a
    return ap, rel


# ------------------------------------------------------------------ hg_graded, hg_grade_hist (tests/test_graded_gpu.py)
def REL(k):
    """Two summation orders of k non-negative float64 terms, each carrying one rounding, differ by at most (k + 2) 2^-52, relatively."""
    return (np.asarray(k, dtype=np.float64) + 2.0) * 2.0 ** -52


def graded_tables(G, ks, gain, disc):
    """G: int64 [Q, R] grades in rank order -> gsum, hits, dcg, wsum [Q, len(ks)] by the definitions."""
    ks = np.asarray(ks, dtype=np.int64)
    R = G.shape[1]
    S = np.cumsum(G, axis=1)
    gsum = S[:, ks - 1]
    hits = np.cumsum(G > 0, axis=1)[:, ks - 1]
    t1 = gain[G] * disc[None, :R]
    t2 = np.where(G > 0, S / np.arange(1, R + 1, dtype=np.float64)[None, :], 0.0)
    dcg = np.stack([t1[:, :k].sum(1) for k in ks], axis=1)
    wsum = np.stack([t2[:, :k].sum(1) for k in ks], axis=1)
    return gsum, hits, dcg, wsum


def assert_graded_tables(got, ref, ks):
    gsum, hits, dcg, wsum = got
    assert gsum.dtype == np.int64 and hits.dtype == np.int64 and dcg.dtype == np.float64 and wsum.dtype == np.float64
    assert np.array_equal(gsum, ref[0]), "gsum"
    assert np.array_equal(hits, ref[1]), "hits"
    tol = REL(ks)[None, :]
    for name, a, r in (("dcg", dcg, ref[2]), ("wsum", wsum, ref[3])):
        err = np.abs(a - r)
        worst = (err / np.maximum(tol * np.abs(r), 1e-300)).max()
        print("%s: largest error %.3g of its bound" % (name, worst))
        assert (err <= tol * np.abs(r)).all(), (name, worst)


def grade_hist(ql, dl):
    Gm = pair_grades(ql, dl)
    C = ql.shape[1]
    return np.stack([np.bincount(Gm[q], minlength=C + 1) for q in range(len(ql))]).T    # [C + 1, Q]


# ------------------------------------------------------------------ hg_votes (tests/test_votes_gpu.py)
def vote_tables(L, ql, ks):
    """L: {0,1} [Q, R, C] labels in rank order -> votes uint32 [Q, nk, C], pred int32, top int64 [Q, nk], conf int64 [nk, C, C]."""
    ks = np.asarray(ks, dtype=np.int64)
    votes = np.cumsum(L.astype(np.int64), axis=1)[:, ks - 1, :]
    top = votes.max(2)
    pred = np.where(top > 0, votes.argmax(2), -1).astype(np.int32)       # (argmax: the first, so the smallest, class at the maximum)
    conf = np.einsum("qa,qjb->jab", ql.astype(np.int64), votes)
    return votes.astype(np.uint32), pred, top, conf


# ------------------------------------------------------------------ hg_rel_hist (tests/test_rel_hist_gpu.py)
def rel_hist(qb, db, ql, dl):
    """-> (all, rel) int64 [b+1, Q] from the Q x N distance matrix and the label match."""
    b = qb.shape[1]
    D = np.zeros((qb.shape[0], db.shape[0]), np.int64)
    for j in range(b):                                 # (bit by bit: no Q x N x b temporary)
        D += qb[:, j, None] != db[None, :, j]
    rel = (ql.astype(np.int64) @ dl.astype(np.int64).T) > 0
    all_h = np.stack([np.bincount(D[q], minlength=b + 1) for q in range(len(qb))])
    rel_h = np.stack([np.bincount(D[q][rel[q]], minlength=b + 1) for q in range(len(qb))])
    return all_h.T, rel_h.T


# ------------------------------------------------------------------ hg_joint_hist (tests/test_tie_graded_gpu.py)
def defined_G(ql, dl):
    return 1 + int(min(ql.sum(1).max(), dl.sum(1).max()))


def joint_hist(qb, db, ql, dl, G):
    """uint32 [b + 1, G, Q] by the definition; a grade beyond G - 1 would raise."""
    d = (qb[:, None, :] != db[None, :, :]).sum(2)
    g = ql.astype(np.int64) @ dl.astype(np.int64).T
    J = np.zeros((qb.shape[1] + 1, G, len(qb)), dtype=np.uint32)
    np.add.at(J, (d, g, np.arange(len(qb))[:, None]), 1)
    return J


# ------------------------------------------------------------------ hg_tie_ap (tests/test_tie_ap_gpu.py)
TIE_FLOATS = ("ap", "p_hit", "ap_min", "ap_max")
TIE_ALL = TIE_FLOATS + ("rel_exp", "rel_lo", "rel_hi")


def assert_tie_close(got, ref, Rs):
    """got: Context.get_tie_ap(); ref: tie_oracle.over_queries(...).  -> the largest error met, as a fraction of its bound."""
    Rs = np.asarray(Rs, dtype=np.int64)
    tol = T.bound(Rs[None, :], ref["H"])
    assert (tol <= 1e-10).all(), tol.max()
    for k in TIE_ALL:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    assert np.array_equal(got["rel_lo"], ref["rel_lo"]) and np.array_equal(got["rel_hi"], ref["rel_hi"])
    assert (np.abs(got["rel_exp"] - ref["rel_exp"]) <= 4 * 2.0 ** -52 * ref["rel_exp"]).all()
    worst = 0.0
    for k in TIE_FLOATS:
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k]), nan), k
        g, r = np.where(nan, 0.0, got[k]), np.where(nan, 0.0, ref[k])
        err = np.abs(g - r)
        frac = (err / np.maximum(tol * np.abs(r), 1e-300)).max()
        worst = max(worst, frac)
        print("%s: largest error %.3g of its bound" % (k, frac))
        assert (err <= tol * np.abs(r)).all(), (k, frac)
    return worst

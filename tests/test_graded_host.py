"""Graded relevance, the host side: extra_metrics.graded_from_tables against the definitions (IDCG from the grade histogram, the NaN
and skip rules), the argument errors that are raised before the GPU is touched, and the five entry points in the header and the binding."""
import os
import re

import numpy as np
import pytest

from hashgan_amd import _native
from hashgan_amd import extra_metrics as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hg_graded", "hg_get_graded", "hg_get_grades", "hg_grade_hist", "hg_get_grade_hist"]


def REL(k):
    return (np.asarray(k, dtype=np.float64) + 2.0) * 2.0 ** -52


def brute(G, Gm, ks, gain, disc):
    """Everything by the definitions: G [Q, R] grades in rank order, Gm [Q, N] grades of every pair."""
    ks = np.asarray(ks, dtype=np.int64)
    Q, R = G.shape
    out = {k: np.zeros((Q, len(ks))) for k in ("gsum", "hits", "dcg", "wsum", "idcg")}
    for q in range(Q):
        ideal = np.sort(Gm[q])[::-1]
        for j, k in enumerate(ks):
            S = 0
            for i in range(1, k + 1):
                g = G[q, i - 1]
                S += g
                out["dcg"][q, j] += gain[g] * disc[i - 1]
                out["idcg"][q, j] += gain[ideal[i - 1]] * disc[i - 1]
                if g > 0:
                    out["hits"][q, j] += 1
                    out["wsum"][q, j] += S / i
            out["gsum"][q, j] = S
    out["gsum"] = out["gsum"].astype(np.int64)
    out["hits"] = out["hits"].astype(np.int64)
    return out


def make(seed, Q=7, N=60, C=5, zero_queries=(), p=0.3):
    rng = np.random.default_rng(seed)
    Gm = rng.binomial(C, p, (Q, N)).astype(np.int64)
    for q in zero_queries:
        Gm[q] = 0
    order = np.stack([rng.permutation(N) for _ in range(Q)])
    G = np.take_along_axis(Gm, order, axis=1)
    hist = np.stack([np.bincount(Gm[q], minlength=C + 1) for q in range(Q)])
    return G, Gm, hist


@pytest.mark.parametrize("gain", ["exp", "linear", "custom"])
def test_graded_from_tables_against_the_definitions(gain):
    C, ks = 5, (1, 2, 9, 33, 60)
    G, Gm, hist = make(1, zero_queries=(2,))
    G[4, :9] = 0                                           # a query without a hit in its first nine ranks (it has relevant rows)
    tab = X.gain_table(np.array([0.0, 1.0, 1.0, 2.5, 7.0, 7.0]) if gain == "custom" else gain, C)
    disc = X.discount_table(60)
    assert disc[0] == 1.0 and abs(disc[2] - 0.5) < 1e-16
    ref = brute(G, Gm, ks, tab, disc)
    out = X.graded_from_tables(ref["gsum"], ref["hits"], ref["dcg"], ref["wsum"], hist, ks, tab, disc)
    pq = out["per_query"]
    tol = REL(ks)[None, :]
    idcg_abs = tol * tab.sum() * np.array([disc[:k].sum() for k in ks])[None, :]
    assert (np.abs(pq["idcg"] - ref["idcg"]) <= idcg_abs).all()
    assert np.array_equal(pq["total_rel"], (Gm > 0).sum(1))
    assert np.array_equal(pq["acg"], ref["gsum"] / np.array(ks)[None, :])
    # NaN rules: no relevant row at all -> NDCG NaN at every k; no hit within k -> WAP NaN there
    assert np.isnan(pq["ndcg"][2]).all() and np.isnan(pq["wap"][2]).all()
    assert np.isnan(pq["wap"][4, :3]).all() and not np.isnan(pq["wap"][4, 3:]).any()
    assert not np.isnan(pq["ndcg"][4]).any() and (pq["ndcg"][4, :3] == 0).all()
    has, hit = ref["idcg"] > 0, ref["hits"] > 0
    assert np.array_equal(np.isnan(pq["ndcg"]), ~has) and np.array_equal(np.isnan(pq["wap"]), ~hit)
    nd = np.where(has, ref["dcg"] / np.where(has, ref["idcg"], 1), np.nan)
    wp = np.where(hit, ref["wsum"] / np.maximum(ref["hits"], 1), np.nan)
    for j in range(len(ks)):
        assert np.allclose(pq["ndcg"][has[:, j], j], nd[has[:, j], j], rtol=1e-13, atol=0)
        assert (pq["ndcg"][has[:, j], j] <= 1 + 1e-13).all()
        assert abs(out["acg"][j] - pq["acg"][:, j].mean()) < 1e-15
        assert abs(out["ndcg"][j] - nd[has[:, j], j].mean()) <= 1e-13        # the skipped queries are not in the mean
        assert abs(out["wap"][j] - wp[hit[:, j], j].mean()) <= 1e-13


def test_all_irrelevant_and_single_grade():
    ks = (1, 10, 60)
    disc = X.discount_table(60)
    # nobody shares a label with anything: ACG 0, NDCG and WAP NaN (no query left in the mean)
    G, Gm, hist = make(2, zero_queries=range(7))
    tab = X.gain_table("exp", 5)
    ref = brute(G, Gm, ks, tab, disc)
    out = X.graded_from_tables(ref["gsum"], ref["hits"], ref["dcg"], ref["wsum"], hist, ks, tab, disc)
    assert (out["acg"] == 0).all() and np.isnan(out["ndcg"]).all() and np.isnan(out["wap"]).all()
    assert (out["per_query"]["idcg"] == 0).all()
    # a single grade (one-hot labels): grades are 0 / 1, WAP is AP@k over the hits, NDCG's ideal is "all hits first"
    G, Gm, hist = make(3, C=1, p=0.2)
    tab = X.gain_table("exp", 1)
    ref = brute(G, Gm, ks, tab, disc)
    out = X.graded_from_tables(ref["gsum"], ref["hits"], ref["dcg"], ref["wsum"], hist, ks, tab, disc)
    pq = out["per_query"]
    for q in range(len(G)):
        n1 = int((Gm[q] > 0).sum())
        for j, k in enumerate(ks):
            assert abs(pq["idcg"][q, j] - disc[:min(k, n1)].sum()) <= REL(k) * disc[:k].sum()
            m = G[q, :k] > 0
            if m.any():
                ap = (np.cumsum(m)[m] / (np.flatnonzero(m) + 1)).mean()
                assert abs(pq["wap"][q, j] - ap) <= 1e-14


def test_argument_errors_before_the_gpu():
    rng = np.random.default_rng(0)
    q, db = rng.integers(0, 2, (3, 8)), rng.integers(0, 2, (20, 8))
    ql, dl = rng.integers(0, 2, (3, 4)), rng.integers(0, 2, (20, 4))
    f = X.graded_relevance_at_k
    for ks in ((0, 5), (1, 21), (), (5, 3), (3, 3, 5), tuple(range(1, 66))):
        with pytest.raises(ValueError):
            f(q, db, ql, dl, ks)
    with pytest.raises(ValueError):
        f(q, db, ql, dl, (1, 5), gain=[0, 1, 3, 2, 4])                       # decreasing
    with pytest.raises(ValueError):
        f(q, db, ql, dl, (1, 5), gain=[0, 1, 2])                             # not C + 1 values
    with pytest.raises(ValueError):
        f(q, db, ql, dl, (1, 5), gain="log")
    wide_q, wide_d = np.zeros((3, 256), np.int8), np.zeros((20, 256), np.int8)
    with pytest.raises(ValueError):
        f(q, db, wide_q, wide_d, (1, 5))                                     # C > 255
    with pytest.raises(ValueError):
        X.grade_histograms(q, db, wide_q, wide_d)
    with pytest.raises(ValueError):
        f(np.zeros((3, 256), np.float32), np.zeros((20, 256), np.float32), ql, dl, (1, 5), features=True)
    with pytest.raises(ValueError):
        X.graded_from_tables(*(np.zeros((3, 2)),) * 4, np.zeros((3, 5), np.int64), (1, 5), [0, 1, 3, 2, 4], X.discount_table(5))


def test_the_new_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "hashgan_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in _native.EXPORTS, name
    for method in ("graded", "get_graded", "get_grades", "grade_hist", "get_grade_hist"):
        assert callable(getattr(_native.Context, method))

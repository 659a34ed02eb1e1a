"""Class votes, host side (no GPU): extra_metrics.knn_from_tables against a direct NumPy computation from random small vote tables, its
nan and -1 conventions, and the argument errors of knn_vote_at_k, which are raised before any GPU use.  Everything compared with ==
is an integer or a quotient of the same two integers formed the same way."""
import numpy as np
import pytest
from hashgan_amd import extra_metrics as X

Q, C = 40, 7
KS = (1, 5, 30)


def tables(votes, ql):
    """votes int64 [Q, nk, C] -> (pred [Q, nk], conf [nk, C, C]) by the definitions, with loops."""
    Qn, nk, Cn = votes.shape
    pred = np.full((Qn, nk), -1, np.int32)
    conf = np.zeros((nk, Cn, Cn), np.int64)
    for q in range(Qn):
        for j in range(nk):
            top = votes[q, j].max()
            if top > 0:
                pred[q, j] = min(c for c in range(Cn) if votes[q, j, c] == top)
            for a in range(Cn):
                if ql[q, a]:
                    conf[j, a] += votes[q, j]
    return pred, conf


def direct(votes, ql, ks):
    """The dict's entries straight from the vote tables, query by query."""
    Qn, nk, Cn = votes.shape
    pred, conf = tables(votes, ql)
    acc = np.full(nk, np.nan)
    per = np.full((nk, Cn), np.nan)
    prec = np.full((nk, Cn), np.nan)
    for j in range(nk):
        right = [bool(pred[q, j] >= 0 and ql[q, pred[q, j]]) for q in range(Qn)]
        labelled = [q for q in range(Qn) if ql[q].any()]
        if labelled:
            acc[j] = sum(right[q] for q in labelled) / len(labelled)
        for a in range(Cn):
            qs = [q for q in range(Qn) if ql[q, a]]
            if qs:
                per[j, a] = sum(right[q] for q in qs) / len(qs)
                prec[j, a] = sum(int(votes[q, j, a]) for q in qs) / (ks[j] * len(qs))
    return pred, conf, acc, per, prec


def random_votes(rng, multi_hot):
    """Running vote counts of a made-up ranking: cumulative label sums of 30 random rows per query, read at KS."""
    if multi_hot:
        rows = (rng.random((Q, KS[-1], C)) < 0.25).astype(np.int64)
        ql = (rng.random((Q, C)) < 0.3).astype(np.int64)
    else:
        rows = np.eye(C, dtype=np.int64)[rng.integers(0, C, (Q, KS[-1]))]
        ql = np.eye(C, dtype=np.int64)[rng.integers(0, C - 1, Q)]          # (no query of class C - 1: a nan column)
    rows[3] = 0                                                           # a query whose rows have no label: pred -1 at every k
    rows[:, 0][5] = 0                                                     # ... and one whose first row has none
    ql[0] = 0                                                             # a query without labels
    votes = np.cumsum(rows, axis=1)[:, np.array(KS) - 1, :]
    return votes, ql


@pytest.mark.parametrize("multi_hot", [False, True])
def test_knn_from_tables_against_the_definitions(multi_hot):
    rng = np.random.default_rng(11 + multi_hot)
    votes, ql = random_votes(rng, multi_hot)
    pred, conf, acc, per, prec = direct(votes, ql, KS)
    assert (pred == -1).any() and (pred >= 0).any()
    out = X.knn_from_tables(pred, conf, ql, KS)
    assert sorted(out) == ["accuracy", "class_precision", "confusion", "ks", "per_class_accuracy"]
    assert out["confusion"].dtype == np.int64 and np.array_equal(out["confusion"], conf)
    assert out["ks"].dtype == np.int64 and np.array_equal(out["ks"], KS)
    assert out["accuracy"].shape == (3,) and out["per_class_accuracy"].shape == (3, C) and out["class_precision"].shape == (3, C)
    assert np.array_equal(out["accuracy"], acc)
    assert np.array_equal(out["per_class_accuracy"], per, equal_nan=True)
    assert np.array_equal(out["class_precision"], prec, equal_nan=True)
    if not multi_hot:
        assert np.isnan(out["per_class_accuracy"][:, C - 1]).all() and np.isnan(out["class_precision"][:, C - 1]).all()
        assert not np.isnan(out["per_class_accuracy"][:, :C - 1]).any()
        # single label: class_precision is the mean precision@k of the class's queries, and the rows of conf sum to k n_a
        n_a = ql.sum(0)
        assert (conf.sum(2) <= np.array(KS)[:, None] * n_a[None, :]).all() and (conf.sum(2)[-1, :C - 1] > 0).all()
        assert (out["class_precision"][:, :C - 1] <= 1.0).all()


def test_conventions():
    ql = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 0]])
    # -1 is wrong; an unlabelled query is excluded whatever it predicts; a multi-label query is right with either of its labels
    pred = np.array([[0, -1], [2, 1], [0, 0], [1, -1]], np.int32)
    conf = np.zeros((2, 3, 3), np.int64)
    conf[0, 0, 0], conf[1, 1, 1] = 2, 6
    out = X.knn_from_tables(pred, conf, ql, (1, 3))
    assert np.array_equal(out["accuracy"], [2 / 3, 1 / 3])
    assert np.array_equal(out["per_class_accuracy"], [[1.0, 0.5, np.nan], [0.0, 0.5, np.nan]], equal_nan=True)
    assert np.array_equal(out["class_precision"], [[2 / 2, 0.0, np.nan], [0.0, 6 / 6, np.nan]], equal_nan=True)
    # no labelled query at all: nan everywhere
    out = X.knn_from_tables(pred, conf, np.zeros_like(ql), (1, 3))
    assert np.isnan(out["accuracy"]).all() and np.isnan(out["per_class_accuracy"]).all() and np.isnan(out["class_precision"]).all()
    assert np.array_equal(out["confusion"], conf)
    # every prediction -1: accuracy 0, not nan
    out = X.knn_from_tables(np.full((4, 2), -1, np.int32), conf, ql, (1, 3))
    assert np.array_equal(out["accuracy"], [0.0, 0.0])
    # shapes and ranges
    with pytest.raises(ValueError):
        X.knn_from_tables(pred[:, :1], conf, ql, (1, 3))
    with pytest.raises(ValueError):
        X.knn_from_tables(pred, conf[:, :2], ql, (1, 3))
    with pytest.raises(ValueError):
        X.knn_from_tables(np.full((4, 2), 3, np.int32), conf, ql, (1, 3))
    with pytest.raises(ValueError):
        X.knn_from_tables(pred, conf, ql, (3, 1))


def test_argument_errors_need_no_gpu():
    rng = np.random.default_rng(3)
    N, Qn, b, Cn = 70, 4, 16, 5
    db, q = rng.integers(0, 2, (N, b)), rng.integers(0, 2, (Qn, b))
    dl, ql = rng.integers(0, 2, (N, Cn)), rng.integers(0, 2, (Qn, Cn))
    for features, rerank in ((False, False), (True, False), (False, True)):
        kw = dict(features=features, rerank=rerank)
        with pytest.raises(ValueError):
            X.knn_vote_at_k(q, db, ql, dl, (5, 1), **kw)                    # not ascending
        with pytest.raises(ValueError):
            X.knn_vote_at_k(q, db, ql, dl, (5, 5), **kw)
        with pytest.raises(ValueError):
            X.knn_vote_at_k(q, db, ql, dl, (1, N + 1), **kw)                # k > N
        with pytest.raises(ValueError):
            X.knn_vote_at_k(q, db, ql, dl, tuple(range(1, 66)), **kw)       # 65 cut-offs, each within 1..N
        with pytest.raises(ValueError):
            X.knn_vote_at_k(q, db, ql, dl, (), **kw)
        with pytest.raises(ValueError):
            X.knn_vote_at_k(q, db, ql[:, :4], dl, (1, 5), **kw)             # C differs
        with pytest.raises(ValueError):                                      # C = 256
            X.knn_vote_at_k(q, db, np.zeros((Qn, 256), np.int64), np.zeros((N, 256), np.int64), (1, 5), **kw)
    wide_db, wide_q = rng.standard_normal((N, 256)).astype(np.float32), rng.standard_normal((Qn, 256)).astype(np.float32)
    with pytest.raises(ValueError):
        X.knn_vote_at_k(wide_q, wide_db, ql, dl, (1, 5), features=True)      # 256 features
    with pytest.raises(ValueError):
        X.knn_vote_at_k(wide_q, wide_db, ql, dl, (1, 5), rerank=True)


def test_maps_argument_errors_need_no_gpu():
    from hashgan_amd import MAPs

    class T:
        def __init__(self, o, l):
            self.output, self.label = o, l

    rng = np.random.default_rng(4)
    db = T(rng.standard_normal((50, 16)).astype(np.float32), rng.integers(0, 2, (50, 5)))
    q = T(rng.standard_normal((4, 16)).astype(np.float32), rng.integers(0, 2, (4, 5)))
    m = MAPs(10)
    with pytest.raises(ValueError):
        m.get_knn_at(db, q, (5, 1))
    with pytest.raises(ValueError):
        m.get_knn_at(db, q, (1, 51))
    with pytest.raises(ValueError):
        m.get_knn_at(db, q, tuple(range(1, 66)))
    with pytest.raises(ValueError):
        m.get_knn_at(T(db.output, np.zeros((50, 256), np.int64)), T(q.output, np.zeros((4, 256), np.int64)), (1, 5))

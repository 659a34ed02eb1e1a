"""curves_from_histograms (NumPy only): precision / recall over the Hamming radius from the two lookup tables, against the
brute-force definition on the pairs themselves."""
import numpy as np

from hashgan_amd import extra_metrics as X


def _case(seed=7, Q=23, N=400, b=12, C=5):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    qb[1] = 1 - db[0]                                  # far from most rows ...
    db[(db != qb[1]).sum(1) <= 2] ^= 1                 # ... and nothing within radius 2 of it: an empty ball at small r
    dl = (rng.random((N, C)) < 0.3).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.3).astype(np.int64)
    ql[0] = 0                                          # a query without labels: total_rel = 0
    return qb, db, ql, dl


def _tables(qb, db, ql, dl):
    """Brute force: the Q x N distance matrix, the label match, a bincount per query -> (all, rel) int64 [Q, b+1], D, match."""
    b = qb.shape[1]
    D = (qb[:, None, :] != db[None, :, :]).sum(2)
    rel = (ql @ dl.T) > 0
    all_h = np.stack([np.bincount(D[q], minlength=b + 1) for q in range(len(qb))])
    rel_h = np.stack([np.bincount(D[q][rel[q]], minlength=b + 1) for q in range(len(qb))])
    return all_h, rel_h, D, rel


def test_curves_match_the_definition():
    qb, db, ql, dl = _case()
    Q, b, N = qb.shape[0], qb.shape[1], db.shape[0]
    all_h, rel_h, D, rel = _tables(qb, db, ql, dl)
    out = X.curves_from_histograms(all_h, rel_h)
    tot = rel.sum(1)
    assert tot[0] == 0 and (tot > 0).any()
    ok = tot > 0
    for r in range(b + 1):
        inside = D <= r
        ball = inside.sum(1)
        hit = (inside & rel).sum(1)
        assert np.array_equal(out["ball"][:, r], ball) and np.array_equal(out["hit"][:, r], hit)
        p = np.where(ball > 0, hit / np.maximum(ball, 1), 0.0).mean()
        rc = (hit[ok] / tot[ok]).mean()
        assert abs(out["precision"][r] - p) <= 1e-15 and abs(out["recall"][r] - rc) <= 1e-15
    assert np.array_equal(out["total_rel"], tot)
    assert out["precision"].dtype == np.float64 and out["recall"].dtype == np.float64
    assert out["ball"].dtype == np.int64 and out["hit"].dtype == np.int64 and out["total_rel"].dtype == np.int64
    # the query with the empty ball: it is there, and contributes precision 0 at those radii
    assert out["ball"][1, 2] == 0 and out["ball"][1, b] == N
    # monotone in r; the widest ball is the database; hits never exceed the ball
    assert (np.diff(out["ball"], axis=1) >= 0).all() and (np.diff(out["hit"], axis=1) >= 0).all()
    assert (out["ball"][:, b] == N).all() and (out["hit"] <= out["ball"]).all()
    assert out["recall"][b] == 1.0


def test_empty_ball_counts_as_zero_precision():
    all_h = np.array([[0, 0, 4], [2, 0, 2]])
    rel_h = np.array([[0, 0, 1], [1, 0, 0]])
    out = X.curves_from_histograms(all_h, rel_h)
    assert np.allclose(out["precision"], [0.25, 0.25, (0.25 + 0.25) / 2], rtol=0, atol=1e-15)
    assert np.allclose(out["recall"], [0.5, 0.5, 1.0], rtol=0, atol=1e-15)


def test_no_relevant_rows_anywhere_gives_nan_recall():
    qb, db, ql, dl = _case(seed=9)
    ql[:] = 0
    all_h, rel_h, _, _ = _tables(qb, db, ql, dl)
    assert rel_h.sum() == 0
    out = X.curves_from_histograms(all_h, rel_h)
    assert out["recall"].shape == (qb.shape[1] + 1,) and np.isnan(out["recall"]).all()
    assert (out["precision"] == 0.0).all() and (out["total_rel"] == 0).all()

"""The NumPy statement of the re-ranked Hamming ranking (tests/rerank_oracle.py) against three things it must agree with: a plain
Python sort by the triple, the canonical Hamming ranking when the features are +-1 (every score is b - 2 d: nothing to re-rank), and
the real-valued ranking when every code is equal (one tie group: the inner product decides alone).  No GPU."""
import numpy as np

from oracle import hamming_map as H
from oracle import real_map as RM
from tests import rerank_oracle as RO


def test_helper_equals_a_python_sort_by_the_triple():
    qf, dbf, ql, dl = RO.generate(5, 61, 6, 3, seed=1)
    R = 40
    o = RO.rerank(qf, dbf, ql, dl, R)
    for q in range(len(qf)):
        d = [sum(int((x > 0) != (y > 0)) for x, y in zip(qf[q], dbf[n])) for n in range(len(dbf))]
        s = o["s"][q]
        want = sorted(range(len(dbf)), key=lambda n: (d[n], -float(s[n]), n))[:R]
        assert o["idx"][q].tolist() == want
        assert o["dist"][q].tolist() == [d[n] for n in want]
        assert o["score"][q].tobytes() == s[want].tobytes()
    # duplicated rows: equal (d, s), the index decides
    assert (o["s"][:, 5] == o["s"][:, 4]).all() and (o["d"][:, 5] == o["d"][:, 4]).all()


def test_pm1_features_give_the_canonical_hamming_ranking():
    rng = np.random.default_rng(2)
    b, N, Q, R = 24, 300, 9, 120
    dbits = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qbits = dbits[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.15).astype(np.uint8)
    lab = lambda n: np.eye(4, dtype=np.int64)[rng.integers(0, 4, n)]
    o = RO.rerank(qbits.astype(np.float32) * 2 - 1, dbits.astype(np.float32) * 2 - 1, lab(Q), lab(N), R)
    idx, dist = H.topr_from_codes(qbits, dbits, R)
    assert (o["idx"] == idx).all() and (o["dist"] == dist).all()
    assert (o["score"] == (b - 2 * dist).astype(np.float32)).all()


def test_all_positive_features_give_the_real_valued_ranking():
    rng = np.random.default_rng(3)
    b, N, Q, R = 12, 400, 6, 150
    dbf = rng.uniform(0.05, 1.0, (N, b)).astype(np.float32)
    qf = rng.uniform(0.05, 1.0, (Q, b)).astype(np.float32)
    dbf[7::31] = dbf[6::31]
    lab = lambda n: np.eye(5, dtype=np.int64)[rng.integers(0, 5, n)]
    ql, dl = lab(Q), lab(N)
    o = RO.rerank(qf, dbf, ql, dl, R)
    _, ap, idx, score = RM.map_from_features(qf, dbf, ql, dl, R)
    assert (o["dist"] == 0).all()
    assert (o["idx"] == idx).all()
    assert o["score"].tobytes() == score.tobytes()
    assert o["ap"].tobytes() == ap.tobytes()

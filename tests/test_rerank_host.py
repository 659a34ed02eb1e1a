"""The NumPy statement of the re-ranked Hamming ranking (tests/rerank_oracle.py) against three things it must agree with: a plain
Python sort by the triple, the canonical Hamming ranking when the features are +-1 (every score is b - 2 d: nothing to re-rank), and
the real-valued ranking when every code is equal (one tie group: the inner product decides alone).  Below them: the premises of
tests/test_rerank_routes_gpu.py -- that each of its cases reaches the route it is named after -- asserted from the oracle's d and s
alone (the thresholds are the kernel's: rerank_oracle.RR_LDS_KEYS, 2^16, 2^20).  No GPU."""
import numpy as np
import pytest

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


# ---- the premises of tests/test_rerank_routes_gpu.py ----
def test_route_counts_the_groups_as_the_kernel_does():
    """rerank_oracle.route on hand-made distances: a short query counts its non-empty groups as LDS groups; a long one goes group by
    group, and only a group beyond RR_LDS_KEYS is a radix group.  The threshold group counts whole (M_q), whatever R cuts off."""
    K = RO.RR_LDS_KEYS
    d = np.concatenate([np.zeros(3, np.int64), np.full(K + 1, 2), np.full(K, 3), np.full(5, 7)])
    def at(R):
        order = np.argsort(d, kind="stable")[:R]
        return RO.route(dict(d=d[None, :], dist=d[order][None, :]), R)
    r = at(3)
    assert (r["t"][0], r["m"][0], r["groups_lds"], r["groups_global"], r["records"]) == (0, 3, 1, 0, 3)
    r = at(4)                                             # 3 + K + 1 records: group by group, d = 1 is empty
    assert (r["t"][0], r["m"][0], r["groups_lds"], r["groups_global"]) == (2, K + 4, 1, 1)
    r = at(K + 5)
    assert (r["t"][0], r["m"][0], r["groups_lds"], r["groups_global"]) == (3, 2 * K + 4, 2, 1)
    r = at(len(d))
    assert (r["t"][0], r["m"][0], r["groups_lds"], r["groups_global"]) == (7, 2 * K + 9, 3, 1)


@pytest.mark.parametrize("b", RO.WIDTHS)
def test_premises_of_every_code_width(b):
    qf, dbf, ql, dl, R, o = RO.width_case(b)
    assert [(w + 31) // 32 for w in RO.WIDTHS] == [1, 2, 3, 4, 5, 6, 7, 8, 4, 6]         # code words: k_rr_collect<NW>
    RO.width_premises(qf, dbf, R, o)


def test_premises_of_the_group_by_group_route():
    *_, R, o = RO.lds_groups_case()
    RO.lds_groups_premises(R, o)


@pytest.mark.parametrize("name", list(RO.MIXED_R))
def test_premises_of_the_mixed_route(name):
    *_, R, o = RO.mixed_case(name)
    RO.mixed_premises(name, o)


def test_premises_of_the_high_index_case():
    *_, R, o = RO.high_index_case()
    RO.high_index_premises(R, o)
    *_, R, o = RO.high_index_head_case()
    RO.high_index_head_premises(R, o)


def test_premises_of_the_chunk_case():
    *_, R, o = RO.chunk_case()
    RO.chunk_premises(R, o, budget_mb=1)


def test_premises_of_the_score_range_cases():
    *_, R, o = RO.denormal_case()
    RO.denormal_premises(R, o)
    *_, R, o = RO.overflow_case()
    RO.overflow_premises(R, o)


def test_premises_of_the_permuted_case():
    (qf, dbf, ql, dl, R, o), (dbf_p, dl_p), perm = RO.untied_case()
    RO.untied_premises(R, o)
    assert sorted(perm.tolist()) == list(range(len(dbf))) and (perm != np.arange(len(dbf))).any()
    assert (dbf_p == dbf[perm]).all() and (dl_p == dl[perm]).all()
    # what the GPU case expects of the permuted run, on the oracle itself: the same lists, idx through the permutation
    p = RO.rerank(qf, dbf_p, ql, dl_p, R)
    assert (perm[p["idx"]] == o["idx"]).all()
    for k in ("dist", "score", "match", "ap", "rel"):
        assert np.ascontiguousarray(p[k]).tobytes() == np.ascontiguousarray(o[k]).tobytes(), k


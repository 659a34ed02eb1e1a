"""Tie-aware graded relevance, the host side: extra_metrics.tie_graded_from_tables against an enumeration of every order inside the tie
groups in exact rational arithmetic (which shares no code with the library), its degenerate cases (no ties, one group), the ordering of
minimum, expectation and maximum, the independence of a query's results from the batch it is reduced in, the refusals, and the two
entry points in the header and the binding."""
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from hashgan_amd import _native
from hashgan_amd import extra_metrics as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12           # sums of at most a few dozen float64 terms, each rounded a handful of times
FLOATS = ("acg", "acg_min", "acg_max", "dcg", "dcg_min", "dcg_max", "idcg", "ndcg", "ndcg_min", "ndcg_max", "gsum_exp", "hits_exp")
TABLES = FLOATS + ("gsum_lo", "gsum_hi")


def enumerate_orders(groups, gain, disc):
    """groups: the grades of the rows of every tie group, nearest group first.  Every order inside the groups, each once per distinct
    sequence of grades (every such sequence stands for the same number of row orders, so their plain mean is the expectation).
    -> {name: [value at k = 1..N]} in Fractions: mean / min / max of DCG@k and of the grade sum, mean of the hits, IDCG."""
    fg, fd = [Fraction(float(x)) for x in gain], [Fraction(float(x)) for x in disc]
    per_group = [sorted(set(itertools.permutations(g))) for g in groups]
    N = sum(len(g) for g in groups)
    dcgs, sums, hits = [], [], []
    for combo in itertools.product(*per_group):
        order = [g for part in combo for g in part]
        d, s, h, dk, sk, hk = Fraction(0), 0, 0, [], [], []
        for i, g in enumerate(order):
            d += fg[g] * fd[i]
            s += g
            h += g > 0
            dk.append(d), sk.append(s), hk.append(h)
        dcgs.append(dk), sums.append(sk), hits.append(hk)
    n = len(dcgs)
    ideal = sorted((g for part in groups for g in part), reverse=True)
    idcg = list(itertools.accumulate(fg[g] * fd[i] for i, g in enumerate(ideal)))
    col = lambda rows, k: [r[k] for r in rows]
    return {"dcg": [sum(col(dcgs, k), Fraction(0)) / n for k in range(N)], "dcg_min": [min(col(dcgs, k)) for k in range(N)],
            "dcg_max": [max(col(dcgs, k)) for k in range(N)], "gsum_exp": [Fraction(sum(col(sums, k)), n) for k in range(N)],
            "gsum_lo": [min(col(sums, k)) for k in range(N)], "gsum_hi": [max(col(sums, k)) for k in range(N)],
            "hits_exp": [Fraction(sum(col(hits, k)), n) for k in range(N)], "idcg": idcg}


def table_of(groups, G=4):
    """[1, len(groups), G]: rows per (distance, grade) of one query."""
    J = np.zeros((1, len(groups), G), dtype=np.int64)
    for d, part in enumerate(groups):
        for g in part:
            J[0, d, g] += 1
    return J


def close(x, frac):
    return abs(Fraction(float(x)) - frac) <= Fraction(RTOL) * abs(frac)


def random_groups(rng):
    """N <= 8 rows with grades 0..3 in <= 3 tie groups; now and then a distance nobody is at."""
    N = int(rng.integers(2, 9))
    cuts = sorted(rng.integers(0, N + 1, int(rng.integers(0, 3))))
    grades = [int(g) for g in rng.integers(0, 4, N)]
    groups = [grades[a:b] for a, b in zip([0] + cuts, cuts + [N])]
    return groups


STRUCTURES = [[[3, 0, 1], [2, 2, 0, 1], [0]],                 # three groups, every grade
              [[0, 0], [0, 3, 3, 1, 1, 2]],                   # no hit in the nearest group
              [[1, 2, 3, 0, 1, 2, 3, 0]],                     # one group of eight
              [[2], [], [1, 1, 0], [3]],                      # an empty distance between groups
              [[0, 0, 0], [0, 0]]]                            # nothing relevant: IDCG 0, NDCG NaN


@pytest.mark.parametrize("case", list(range(len(STRUCTURES) + 12)))
@pytest.mark.parametrize("gain", ["exp", "linear"])
def test_against_the_enumeration_of_every_order(case, gain):
    groups = STRUCTURES[case] if case < len(STRUCTURES) else random_groups(np.random.default_rng(100 + case))
    N = sum(len(g) for g in groups)
    ks = np.arange(1, N + 1)
    tab, disc = X.gain_table(gain, 3), X.discount_table(N)
    ref = enumerate_orders(groups, tab, disc)
    pq = X.tie_graded_from_tables(table_of(groups), ks, tab, disc)["per_query"]
    for j in range(N):
        k = j + 1
        assert pq["gsum_lo"][0, j] == ref["gsum_lo"][j] and pq["gsum_hi"][0, j] == ref["gsum_hi"][j], (groups, k)
        for name in ("dcg", "dcg_min", "dcg_max", "gsum_exp", "hits_exp", "idcg"):
            assert close(pq[name][0, j], ref[name][j]), (groups, k, name, pq[name][0, j], float(ref[name][j]))
        assert close(pq["acg"][0, j], ref["gsum_exp"][j] / k)
        assert pq["acg_min"][0, j] == ref["gsum_lo"][j] / k and pq["acg_max"][0, j] == ref["gsum_hi"][j] / k
        for name in ("ndcg", "ndcg_min", "ndcg_max"):
            if ref["idcg"][j] == 0:
                assert np.isnan(pq[name][0, j])
            else:
                assert close(pq[name][0, j], ref[name[1:]][j] / ref["idcg"][j]), (groups, k, name)
    assert pq["total_rel"][0] == sum(g > 0 for part in groups for g in part)


def test_no_ties_is_the_canonical_list():
    """Every row at a distance of its own: one order, so expectation = minimum = maximum = the list's values."""
    rng = np.random.default_rng(5)
    Q, N, G = 6, 40, 5
    grades = rng.integers(0, G, (Q, N))
    J = np.zeros((Q, N, G), dtype=np.int64)
    J[np.arange(Q)[:, None], np.arange(N)[None, :], grades] = 1
    ks = np.array([1, 2, 7, 33, 40])
    tab, disc = X.gain_table("exp", G - 1), X.discount_table(N)
    pq = X.tie_graded_from_tables(J, ks, tab, disc)["per_query"]
    gsum = np.cumsum(grades, axis=1)[:, ks - 1]
    dcg = np.cumsum(tab[grades] * disc[None, :], axis=1)[:, ks - 1]
    hits = np.cumsum(grades > 0, axis=1)[:, ks - 1]
    for name in ("gsum_exp", "gsum_lo", "gsum_hi"):
        assert np.array_equal(pq[name], gsum), name
    assert np.array_equal(pq["hits_exp"], hits)
    for name in ("dcg", "dcg_min", "dcg_max"):
        assert np.allclose(pq[name], dcg, rtol=RTOL, atol=0), name
    assert np.array_equal(pq["dcg_min"], pq["dcg"]) and np.array_equal(pq["dcg_max"], pq["dcg"])


def test_one_group_is_the_mean_gain_times_the_discounts():
    """Every row at one distance: a rank holds a uniformly drawn row, so dcg[k] = mean gain x cum[k]; at k = N every row is inside."""
    rng = np.random.default_rng(6)
    Q, N, G, NB = 5, 30, 4, 9
    counts = rng.multinomial(N, [0.4, 0.3, 0.2, 0.1], Q)
    J = np.zeros((Q, NB, G), dtype=np.int64)
    J[:, 4, :] = counts
    ks = np.array([1, 3, 10, N])
    tab, disc = X.gain_table("exp", G - 1), X.discount_table(N)
    pq = X.tie_graded_from_tables(J, ks, tab, disc)["per_query"]
    cum = np.array([disc[:k].sum() for k in ks])
    mean_gain = (counts * tab[None, :]).sum(1) / N
    assert np.allclose(pq["dcg"], mean_gain[:, None] * cum[None, :], rtol=RTOL, atol=0)
    total = (counts * np.arange(G)[None, :]).sum(1)
    assert np.array_equal(pq["gsum_exp"][:, -1], total)
    assert np.array_equal(pq["gsum_lo"][:, -1], total) and np.array_equal(pq["gsum_hi"][:, -1], total)
    assert np.allclose(pq["gsum_exp"], total[:, None] * ks[None, :] / N, rtol=RTOL, atol=0)


def random_table(seed, Q=50, NB=17, G=6, rows=400):
    rng = np.random.default_rng(seed)
    J = rng.multinomial(rows, rng.dirichlet(np.full(NB * G, 0.3)), Q).reshape(Q, NB, G).astype(np.int64)
    J[3] = 0
    J[3, :, 0] = rng.multinomial(rows, np.full(NB, 1 / NB))   # a query nothing is relevant to
    J[:, 5, :] = 0                                             # a distance nobody is at
    return J


def test_minimum_expectation_maximum_are_ordered_and_hits_are_the_rel_hist_formula():
    J = random_table(7)
    Q, NB, G = J.shape
    ks = np.array([1, 2, 5, 50, 199, 400])
    tab, disc = X.gain_table("exp", G - 1), X.discount_table(400)
    out = X.tie_graded_from_tables(J, ks, tab, disc)
    pq = out["per_query"]
    eps = 1 + 1e-12
    assert (pq["dcg_min"] <= pq["dcg"] * eps).all() and (pq["dcg"] <= pq["dcg_max"] * eps).all()
    assert (pq["gsum_lo"] <= pq["gsum_exp"] * eps).all() and (pq["gsum_exp"] <= pq["gsum_hi"] * eps).all()
    assert (pq["acg_min"] <= pq["acg"] * eps).all() and (pq["acg"] <= pq["acg_max"] * eps).all()
    ok = pq["idcg"] > 0
    assert np.array_equal(~ok, np.isnan(pq["ndcg"])) and not ok[3].any() and ok[np.arange(Q) != 3].all()
    assert (pq["ndcg_min"][ok] <= pq["ndcg"][ok] * eps).all() and (pq["ndcg"][ok] <= pq["ndcg_max"][ok] * eps).all()
    assert (pq["ndcg_max"][ok] <= eps).all()
    # k = N: every row is inside, all three grade sums are the total
    total = (J * np.arange(G)[None, None, :]).sum((1, 2))
    for name in ("gsum_exp", "gsum_lo", "gsum_hi"):
        assert np.array_equal(pq[name][:, -1], total), name
    # the expected hits are tie_aware_map's rel_exp: sum_d m_d r_d / n_d from the two tables of the relevant-row histogram
    n_d, r_d = J.sum(2), J[:, :, 1:].sum(2)
    a_d = np.cumsum(n_d, axis=1) - n_d
    rel_exp = np.zeros((Q, ks.size))
    for j, k in enumerate(ks):
        m_d = np.clip(k - a_d, 0, n_d)
        rel_exp[:, j] = np.where(n_d > 0, m_d * r_d / np.maximum(n_d, 1), 0.0).sum(1)
    assert np.allclose(pq["hits_exp"], rel_exp, rtol=RTOL, atol=0)
    assert np.array_equal(pq["total_rel"], r_d.sum(1))
    # the means: ACG over all queries, NDCG over those with an ideal gain
    assert np.allclose(out["acg"], pq["acg"].mean(0), rtol=1e-15)
    assert np.allclose(out["ndcg"], [pq["ndcg"][ok[:, j], j].mean() for j in range(ks.size)], rtol=1e-15)


def test_a_query_does_not_depend_on_the_batch():
    J = random_table(8)
    ks = np.array([1, 3, 64, 311, 400])
    tab, disc = X.gain_table("linear", J.shape[2] - 1), X.discount_table(400)
    batch = X.tie_graded_from_tables(J, ks, tab, disc)["per_query"]
    for q in (0, 3, 17, 49):
        alone = X.tie_graded_from_tables(J[q:q + 1], ks, tab, disc)["per_query"]
        for name in TABLES:
            assert alone[name][0].tobytes() == batch[name][q].tobytes(), (q, name)
        assert alone["total_rel"][0] == batch["total_rel"][q]


def test_refusals():
    J = random_table(9)[:3]
    G = J.shape[2]
    tab, disc = X.gain_table("exp", G - 1), X.discount_table(400)
    f = X.tie_graded_from_tables
    f(J, (1, 400), tab, disc)
    up = disc.copy()
    up[7] = up[6] * 1.5
    for args in ((J, (1, 400), tab, up),                                          # an increasing discount
                 (J, (1, 400), tab[::-1].copy(), disc),                           # a decreasing gain
                 (J, (1, 400), tab, disc[:399]),                                  # a discount table shorter than max(ks)
                 (J, (5, 3), tab, disc), (J, (3, 3), tab, disc), (J, (), tab, disc), (J, (0, 3), tab, disc),   # cut-offs
                 (J[0], (1, 400), tab, disc), (J.sum(2), (1, 400), tab, disc),    # a table that is not 3-D
                 (J, (1, 400), tab[:-1], disc)):                                  # not one gain per grade
        with pytest.raises(ValueError):
            f(*args)
    assert f(J, (1, 8), tab, up[:7].tolist() + [up[6]] * 393)["per_query"]["dcg"].shape == (3, 2)   # equal discounts are allowed


def test_argument_errors_before_the_gpu():
    rng = np.random.default_rng(0)
    q, db = rng.integers(0, 2, (3, 8)), rng.integers(0, 2, (20, 8))
    ql, dl = rng.integers(0, 2, (3, 4)), rng.integers(0, 2, (20, 4))
    f = X.tie_aware_graded_at_k
    for ks in ((0, 5), (1, 21), (), (5, 3), (3, 3, 5), tuple(range(1, 66))):
        with pytest.raises(ValueError):
            f(q, db, ql, dl, ks)
    with pytest.raises(ValueError):
        f(q, db, ql, dl, (1, 5), gain=[0, 1, 3, 2, 4])
    with pytest.raises(ValueError):
        f(q, db, ql, dl, (1, 5), gain="log")
    wide_q, wide_d = np.zeros((3, 256), np.int8), np.zeros((20, 256), np.int8)
    with pytest.raises(ValueError):
        f(q, db, wide_q, wide_d, (1, 5))                                          # C > 255
    with pytest.raises(ValueError):
        X.distance_grade_histograms(q, db, wide_q, wide_d)
    with pytest.raises(ValueError):
        X.distance_grade_histograms(q, db[:, :7], ql, dl)


def test_the_new_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "hashgan_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", src))
    for name in ("hg_joint_hist", "hg_get_joint_hist"):
        assert name in declared, name
        assert name in _native.EXPORTS, name
    for method in ("joint_hist", "get_joint_hist"):
        assert callable(getattr(_native.Context, method))

"""Graded relevance on the GPU: hg_graded (sums of the grades along the ranked lists at a list of cut-offs) and hg_grade_hist (rows per
grade and query) against brute-force NumPy -- the full Q x N Hamming (or inner-product) matrix, a stable sort by it, and ql @ dl.T
for the grades; nothing here is derived from the library's own lists -- and hashgan_amd.extra_metrics' ACG / NDCG / WAP on top.

Tolerances.  Integer outputs are compared with ==.  dcg and wsum are sums of k non-negative float64 terms, each carrying one
rounding (a product, a quotient): any summation order is within (k - 1) 2^-53 of the exact sum, relatively, plus the term's own
2^-53, so two orders differ by at most twice that, k 2^-52 <= (k + 2) 2^-52 -- REL(k).  IDCG comes from differences of prefix sums
of the discounts, whose errors are relative to the prefix, not to the difference: absolute bound REL(k) * sum(gain) * sum(disc[:k])."""
import functools

import numpy as np
import pytest
from tests import brute_refs, cases
from hashgan_amd import _native, metric
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG


# the brute-force tables and the bound REL(k) of the docstring: tests/brute_refs.py (shared with tests/test_second_hand_gpu.py)
REL, hamming, ranked_by, pair_grades = brute_refs.REL, brute_refs.hamming, brute_refs.ranked_by, brute_refs.pair_grades
brute_tables, assert_tables, brute_hist = brute_refs.graded_tables, brute_refs.assert_graded_tables, brute_refs.grade_hist


def code_ctx(qb, db, ql, dl, opts=(), idx_base=0, n_total=None):
    ctx = _native.Context(0)
    for k, v in opts:
        ctx.set_option(k, v)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1], idx_base, n_total)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
    return ctx


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


KS1 = (1, 7, 64, 65, 256, 257, 1000, 5000)


@functools.lru_cache(maxsize=None)
def case1():
    """tests/test_rel_hist_gpu.py::case1's inputs: multi-hot labels, a query without labels, rows without labels, a query with all."""
    rng = np.random.default_rng(4)
    Q, N, b, C = 60, 5000, 16, 6
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.08).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.3).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.3).astype(np.int8)
    ql[0] = 0
    dl[::7] = 0
    ql[1] = 1
    Gm = pair_grades(ql, dl)
    order = ranked_by(hamming(qb, db))
    G = np.take_along_axis(Gm, order, axis=1)
    gain, disc = X.gain_table("exp", C), X.discount_table(N)
    ref = brute_tables(G, KS1, gain, disc)
    for a in (qb, db, ql, dl, Gm, G, gain, disc) + ref:
        a.flags.writeable = False
    return dict(qb=qb, db=db, ql=ql, dl=dl, Gm=Gm, G=G, gain=gain, disc=disc, ref=ref)


def test_multi_hot_chunk_edges():
    c = case1()
    assert c["Gm"].max() == 6 and (c["Gm"].max(1) == 0).sum() == 8 and (c["ref"][1][:, 1] == 0).sum() == 11
    ctx = code_ctx(c["qb"], c["db"], c["ql"], c["dl"])
    try:
        ctx.topr(5000)
        ctx.graded(KS1, c["gain"], c["disc"], keep_grades=True)
        got = ctx.get_graded()
        assert_tables(got, c["ref"], KS1)
        assert np.array_equal(ctx.get_grades(), c["G"])
        assert np.array_equal(got[1], np.cumsum(ctx.get_match().astype(np.int64), 1)[:, np.array(KS1) - 1])
        # the last cut-off short of the lists' end: the grade bytes still cover every rank
        ks = (3, 300)
        ctx.graded(ks, c["gain"], c["disc"][:300], keep_grades=True)
        assert_tables(ctx.get_graded(), brute_tables(c["G"], ks, c["gain"], c["disc"]), ks)
        assert np.array_equal(ctx.get_grades(), c["G"])
    finally:
        ctx.close()


@pytest.mark.parametrize("C", [33, 64, 65, 128, 130, 255])
def test_label_widths(C):
    """The last label word (rows and queries that carry only class C - 1), the loop over more than two label words, grade 255."""
    rng = np.random.default_rng(C)
    Q, N, b = 33, 500, 32
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.1).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.2).astype(np.int8)
    dl[::5] = 0
    dl[::5, C - 1] = 1
    ql[:4] = 0
    ql[:4, C - 1] = 1
    if C == 255:
        ql[7] = 1
        dl[123] = 1
    Gm = pair_grades(ql, dl)
    assert Gm[:4, ::5].min() == 1 and Gm.max() == (255 if C == 255 else Gm.max()) and Gm.max() > 1
    G = np.take_along_axis(Gm, ranked_by(hamming(qb, db)), axis=1)
    ks = (1, 64, 257, 500)
    gain, disc = X.gain_table("exp", C), X.discount_table(N)
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.topr(N)
        ctx.graded(ks, gain, disc, keep_grades=True)
        assert_tables(ctx.get_graded(), brute_tables(G, ks, gain, disc), ks)
        assert np.array_equal(ctx.get_grades(), G)
        ctx.grade_hist()
        assert np.array_equal(ctx.get_grade_hist(), brute_hist(ql, dl))
    finally:
        ctx.close()


def test_256_classes_are_refused():
    rng = np.random.default_rng(256)
    Q, N, b, C = 5, 300, 32, 256
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl = (rng.random((N, C)) < 0.1).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.1).astype(np.int8)
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.topr(10)
        raises(ARG, ctx.graded, (1, 10), np.arange(C + 1, dtype=np.float64), X.discount_table(10))
        raises(ARG, ctx.grade_hist)
    finally:
        ctx.close()


def grade_hist_of(qb, db, ql, dl, opts=(), idx_base=0, n_total=None, with_rel=False):
    ctx = code_ctx(qb, db, ql, dl, opts, idx_base, n_total)
    try:
        ctx.grade_hist()
        h = ctx.get_grade_hist()
        assert h.dtype == np.uint32 and h.shape == (ql.shape[1] + 1, len(ql))
        rel = None
        if with_rel:
            ctx.rel_hist()
            rel = ctx.get_rel_hist()[1]
        ctx.hist()
        return h, rel, ctx.get_stat("segments")
    finally:
        ctx.close()


def test_grade_hist_multi_hot():
    c = case1()
    h, rel, _ = grade_hist_of(c["qb"], c["db"], c["ql"], c["dl"], with_rel=True)
    assert np.array_equal(h, brute_hist(c["ql"], c["dl"]))
    assert (h.astype(np.int64).sum(0) == len(c["db"])).all()
    assert np.array_equal(h[1:].astype(np.int64).sum(0), rel.astype(np.int64).sum(0))


def test_grade_hist_ragged_segments():
    rng = np.random.default_rng(5)
    Q, N, b, C = 70, 1001, 64, 10
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl = np.eye(C, dtype=np.int8)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int8)[rng.integers(0, C, Q)]
    h, rel, S = grade_hist_of(qb, db, ql, dl, opts=(("min_segment", 64), ("target_units", 22)), with_rel=True)
    assert S >= 3, S
    assert np.array_equal(h, brute_hist(ql, dl))
    assert (h.astype(np.int64).sum(0) == N).all()
    assert np.array_equal(h[1:].astype(np.int64).sum(0), rel.astype(np.int64).sum(0))


def test_grade_hist_counter_width():
    """One bin holds 140000: a 16-bit column or a narrow partial would wrap."""
    Q, N, b, C = 3, 140000, 32, 2
    rng = np.random.default_rng(6)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    db = np.repeat(qb[:1], N, axis=0)
    ql = np.array([[1, 0], [0, 1], [1, 1]], np.int8)
    dl = np.repeat(np.array([[1, 0]], np.int8), N, axis=0)
    h, _, S = grade_hist_of(qb, db, ql, dl, opts=(("max_segments", 2),))
    assert S == 2
    assert np.array_equal(h, np.array([[0, N, 0], [N, 0, N], [0, 0, 0]]))


def test_grade_hist_additive_over_shards():
    c = case1()
    N, cut = len(c["db"]), 2437
    h0, *_ = grade_hist_of(c["qb"], c["db"][:cut], c["ql"], c["dl"][:cut], idx_base=0, n_total=N)
    h1, *_ = grade_hist_of(c["qb"], c["db"][cut:], c["ql"], c["dl"][cut:], idx_base=cut, n_total=N)
    assert np.array_equal(h0.astype(np.int64) + h1, brute_hist(c["ql"], c["dl"]))


@functools.lru_cache(maxsize=None)
def real_case():
    """Integer-valued float32 features: products and sums are exact, so np.lexsort((index, -ip)) is THE order."""
    rng = np.random.default_rng(44)
    Q, N, F, C = 20, 2000, 24, 81
    dbf = rng.integers(-3, 4, (N, F)).astype(np.float32)
    qf = rng.integers(-3, 4, (Q, F)).astype(np.float32)
    dl = (rng.random((N, C)) < 0.03).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.05).astype(np.int64)
    ip = qf.astype(np.int64) @ dbf.astype(np.int64).T
    Gm = pair_grades(ql, dl)
    G = np.take_along_axis(Gm, ranked_by(-ip), axis=1)
    for a in (dbf, qf, dl, ql, Gm, G):
        a.flags.writeable = False
    return dict(qf=qf, dbf=dbf, ql=ql, dl=dl, Gm=Gm, G=G)


def test_real_valued_lists():
    c = real_case()
    ks = (1, 100, 2000)
    gain, disc = X.gain_table("exp", 81), X.discount_table(2000)
    assert c["G"].max() >= 2
    ctx = _native.Context(0)
    try:
        ctx.set_option("keep_floats", 1)
        ctx.set_database_f32(c["dbf"], c["dl"])
        ctx.set_queries_f32(c["qf"], c["ql"])
        ctx.topr_real(2000, download=False)
        ctx.graded(ks, gain, disc)
        assert_tables(ctx.get_graded(), brute_tables(c["G"], ks, gain, disc), ks)
    finally:
        ctx.close()


def test_state_and_arguments():
    c = case1()
    qb, db, ql, dl, gain, disc = c["qb"], c["db"], c["ql"], c["dl"], c["gain"], c["disc"]
    R = 100
    ctx = code_ctx(qb, db, ql, dl)
    try:
        raises(STATE, ctx.graded, (1, 5), gain, disc[:5])                    # no ranking yet
        raises(STATE, ctx.get_graded)
        raises(STATE, ctx.get_grade_hist)
        ctx.map(R)
        msg = raises(STATE, ctx.graded, (1, 5), gain, disc[:5])              # hg_map leaves no lists
        assert "hg_topr" in msg
        ctx.topr(R)
        raises(ARG, ctx.graded, (5, 1), gain, disc[:5])
        raises(ARG, ctx.graded, (5, 5), gain, disc[:5])
        raises(ARG, ctx.graded, (1, R + 1), gain, disc[:R + 1])
        raises(ARG, ctx.graded, (0, 5), gain, disc[:5])
        raises(ARG, ctx.graded, tuple(range(1, 66)), gain, disc[:65])
        raises(ARG, ctx.graded, (), gain, disc[:5])
        raises(STATE, ctx.get_graded)                                        # a refused call leaves no results
        ks = tuple(range(1, 65))                                             # 64 cut-offs are fine
        ctx.graded(ks, gain, disc[:64])
        assert_tables(ctx.get_graded(), brute_tables(c["G"], ks, gain, disc), ks)
        raises(STATE, ctx.get_grades)                                        # not kept
        # a later ranking ends the results; hg_map too
        ctx.topr(R)
        raises(STATE, ctx.get_graded)
        ctx.graded((R,), gain, disc[:R])
        ctx.map(R)
        raises(STATE, ctx.get_graded)
        # reloads
        ctx.topr(R)
        ctx.graded((R,), gain, disc[:R], keep_grades=True)
        ctx.grade_hist()
        ctx.get_graded(), ctx.get_grades(), ctx.get_grade_hist()
        ctx.set_queries(metric.pack_codes(qb[:10].copy()), metric.pack_labels(ql[:10].copy()))
        raises(STATE, ctx.get_graded)
        raises(STATE, ctx.get_grades)
        raises(STATE, ctx.get_grade_hist)
        raises(STATE, ctx.graded, (R,), gain, disc[:R])                      # the lists were the old queries'
        ctx.topr(R)
        ctx.graded((R,), gain, disc[:R])
        ctx.grade_hist()
        assert np.array_equal(ctx.get_graded()[0][:, 0], c["G"][:10, :R].sum(1))
        assert np.array_equal(ctx.get_grade_hist(), brute_hist(ql[:10], dl))
        ctx.set_database(metric.pack_codes(db[:200].copy()), metric.pack_labels(dl[:200].copy()), db.shape[1], dl.shape[1])
        ctx.set_queries(metric.pack_codes(qb[:10].copy()), metric.pack_labels(ql[:10].copy()))
        raises(STATE, ctx.get_graded)
        raises(STATE, ctx.get_grade_hist)
        # hg_trim
        ctx.topr(R)
        ctx.graded((R,), gain, disc[:R], keep_grades=True)
        ctx.grade_hist()
        ctx.trim()
        raises(STATE, ctx.get_graded)
        raises(STATE, ctx.get_grades)
        raises(STATE, ctx.get_grade_hist)
        raises(STATE, ctx.graded, (R,), gain, disc[:R])
    finally:
        ctx.close()
    # a shard: graded sums over partial lists mean nothing
    ctx = code_ctx(qb, db[:1000], ql, dl[:1000], idx_base=100, n_total=1100)
    try:
        msg = raises(STATE, ctx.graded, (1, 5), gain, disc[:5])
        assert "whole database" in msg
    finally:
        ctx.close()


def test_leaves_the_map_path_alone(case_cache):
    c = case_cache("c3_nus_q64")
    g = cases.load_golden("c3_nus_q64")
    R = c["R"]
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    assert dl.shape[1] == 81 and R == 5000
    ks = (1, 100, 5000)
    order = ranked_by(hamming(qb, db))[:, :R]
    G = np.take_along_axis(pair_grades(ql, dl), order, axis=1)
    gain, disc = X.gain_table("linear", 81), X.discount_table(R)
    ref = brute_tables(G, ks, gain, disc)
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ap, rel = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.topr(R)
        ctx.graded(ks, gain, disc)
        ctx.grade_hist()
        gsum, hits, dcg, wsum = ctx.get_graded()
        assert np.array_equal(gsum, ref[0]) and np.array_equal(hits, ref[1])
        h = ctx.get_grade_hist()
        assert (h.astype(np.int64).sum(0) == len(db)).all()
        ap, rel = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.map_begin(R)
        ctx.grade_hist()
        ap, rel = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert np.array_equal(ctx.get_grade_hist(), h)
    finally:
        ctx.close()


def test_two_runs_give_identical_bits():
    c = case1()
    ctx = code_ctx(c["qb"], c["db"], c["ql"], c["dl"])
    try:
        ctx.topr(5000)
        ctx.graded(KS1, c["gain"], c["disc"])
        a = ctx.get_graded()
        ctx.graded(KS1, c["gain"], c["disc"])
        b = ctx.get_graded()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    finally:
        ctx.close()


# ------------------------------------------------------------------ the Python surface
def definitions(G, Gm, ks, gain, disc):
    """Per-query ACG, DCG, IDCG, NDCG, WAP at ks from the grades in rank order (G) and of every pair (Gm)."""
    ks = np.asarray(ks, dtype=np.int64)
    gsum, hits, dcg, wsum = brute_tables(G, ks, gain, disc)
    ideal = -np.sort(-Gm, axis=1)[:, :ks[-1]]
    ti = gain[ideal] * disc[None, :ks[-1]]
    idcg = np.stack([ti[:, :k].sum(1) for k in ks], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ndcg = np.where(idcg > 0, dcg / idcg, np.nan)
        wap = np.where(hits > 0, wsum / hits, np.nan)
    return dict(acg=gsum / ks[None, :], dcg=dcg, idcg=idcg, ndcg=ndcg, wap=wap, hits=hits, total_rel=(Gm > 0).sum(1))


def assert_metrics(out, ref, ks, gain, disc):
    """DCG and WAP within REL(k); IDCG within its absolute bound; NDCG = DCG / IDCG within the sum of the two relative errors and
    the division's rounding; a mean over n queries of non-negative values adds at most n 2^-52."""
    ks = np.asarray(ks, dtype=np.int64)
    pq = out["per_query"]
    eps = 2.0 ** -52
    rel = REL(ks)[None, :]
    idcg_abs = rel * gain.sum() * np.array([disc[:k].sum() for k in ks])[None, :]
    assert np.array_equal(pq["hits"], ref["hits"]) and np.array_equal(pq["total_rel"], ref["total_rel"])
    assert np.array_equal(pq["acg"], ref["acg"])
    assert (np.abs(pq["dcg"] - ref["dcg"]) <= rel * ref["dcg"]).all()
    assert (np.abs(pq["idcg"] - ref["idcg"]) <= idcg_abs).all()
    assert np.array_equal(np.isnan(pq["ndcg"]), np.isnan(ref["ndcg"])) and np.array_equal(np.isnan(pq["wap"]), np.isnan(ref["wap"]))
    has, hit = ref["idcg"] > 0, ref["hits"] > 0
    ndcg_tol = np.where(has, (rel + idcg_abs / np.where(has, ref["idcg"], 1.0) + 4 * eps) * np.nan_to_num(ref["ndcg"]), 0.0)
    assert (np.abs(np.nan_to_num(pq["ndcg"]) - np.nan_to_num(ref["ndcg"])) <= ndcg_tol).all()
    wap_tol = (rel + 4 * eps) * np.nan_to_num(ref["wap"])
    assert (np.abs(np.nan_to_num(pq["wap"]) - np.nan_to_num(ref["wap"])) <= wap_tol).all()
    n = len(ref["hits"])
    for j, k in enumerate(ks):
        assert abs(out["acg"][j] - ref["acg"][:, j].mean()) <= n * eps * ref["acg"][:, j].mean()
        m = ref["ndcg"][has[:, j], j].mean()
        assert abs(out["ndcg"][j] - m) <= ndcg_tol[has[:, j], j].mean() + n * eps * m
        m = ref["wap"][hit[:, j], j].mean()
        assert abs(out["wap"][j] - m) <= wap_tol[hit[:, j], j].mean() + n * eps * m


@pytest.mark.parametrize("spelling", ["bits", "pm1"])
@pytest.mark.parametrize("gain", ["exp", "linear"])
def test_python_surface_codes(spelling, gain):
    c = case1()
    qb, db, ql, dl = c["qb"], c["db"], c["ql"], c["dl"]
    q_in, d_in = (qb, db) if spelling == "bits" else (2 * qb.astype(np.int8) - 1, 2 * db.astype(np.int8) - 1)
    tab = X.gain_table(gain, 6)
    out = X.graded_relevance_at_k(q_in, d_in, ql, dl, KS1, gain=gain)
    ref = definitions(c["G"], c["Gm"], KS1, tab, c["disc"])
    assert not (ref["idcg"] > 0).all() and not (ref["hits"][:, 1] > 0).all()
    assert_metrics(out, ref, KS1, tab, c["disc"])
    assert np.array_equal(X.grade_histograms(q_in, d_in, ql, dl), brute_hist(ql, dl).T)


def test_python_surface_features():
    c = real_case()
    ks = (1, 100, 2000)
    tab, disc = X.gain_table("exp", 81), X.discount_table(2000)
    out = X.graded_relevance_at_k(c["qf"], c["dbf"], c["ql"], c["dl"], ks, features=True)
    assert_metrics(out, definitions(c["G"], c["Gm"], ks, tab, disc), ks, tab, disc)


def test_ideal_ranking_has_ndcg_one():
    """One query that carries every label, rows whose Hamming distance falls strictly as their grade rises: the ranking IS the ideal
    ordering, NDCG = 1 at every k within the tolerance of two orders of the same sum."""
    rng = np.random.default_rng(8)
    N, b = 40, 8
    grade = rng.integers(0, b + 1, N)
    grade[:9] = np.arange(9)
    dl = (np.arange(b)[None, :] < grade[:, None]).astype(np.int8)
    db = (np.arange(b)[None, :] < (b - grade)[:, None]).astype(np.uint8)      # distance to the zero code = 8 - grade
    ql = np.ones((1, b), np.int8)
    qb = np.zeros((1, b), np.uint8)
    ks = np.arange(1, N + 1)
    out = X.graded_relevance_at_k(qb, db, ql, dl, ks)
    assert (np.abs(out["per_query"]["ndcg"][0] - 1.0) <= REL(ks)).all()
    assert (np.abs(out["ndcg"] - 1.0) <= REL(ks)).all()


def test_one_pass_each_and_no_relevant_row_histogram():
    c = case1()
    eng = metric._Shared.get(0)
    with eng.lock:
        X.graded_relevance_at_k(c["qb"], c["db"], c["ql"], c["dl"], KS1)         # (first use of every path outside the table)
        eng.ctx.timing_enable(2)
        eng.ctx.timing_reset()
        try:
            X.graded_relevance_at_k(c["qb"], c["db"], c["ql"], c["dl"], KS1)
            launches = {k: n for k, (ms, n) in eng.ctx.timing_read().items() if n}
        finally:
            eng.ctx.timing_enable(False)
    assert launches.get("k_graded") == 1 and launches.get("k_grade_hist") == 1 and launches.get("k_grade_hist_reduce") == 1, launches
    assert "k_hist_rel" not in launches and "k_hist_rel_reduce" not in launches, launches

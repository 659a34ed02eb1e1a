"""hg_tie_ap (k_tie_ap): the expectation of AP@R over the orders inside the Hamming tie groups, the hit probability and the exact
envelope [ap_min, ap_max], against the oracles of tests/tie_oracle.py fed with brute-force NumPy tables (the Q x N distance matrix,
the label match, a bincount) -- nothing here is derived from the library's own tables.

Tolerance: tie_oracle.bound(R, H) = (1.25 R + 4 H + 32) 2^-52 relative, the first-order rounding bound of the kernel's summation
order, for ap, p_hit, ap_min and ap_max; at every shape here it stays below 1e-10, five orders under what a
tie order moves AP by.  rel_exp within 4 * 2^-52; rel_lo, rel_hi and total_rel exactly."""
import functools

import numpy as np
import pytest
from oracle import hamming_map
from tests import brute_refs, cases
from tests import tie_oracle as T
from hashgan_amd import _native, metric
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG
FLOATS = ("ap", "p_hit", "ap_min", "ap_max")
ALL = FLOATS + ("rel_exp", "rel_lo", "rel_hi")
WORST = {"fraction": 0.0}


def code_ctx(qb, db, ql, dl, idx_base=0, n_total=None):
    ctx = _native.Context(0)
    load(ctx, qb, db, ql, dl, idx_base, n_total)
    return ctx


def load(ctx, qb, db, ql, dl, idx_base=0, n_total=None):
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1], idx_base, n_total)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))


def gpu_tie(qb, db, ql, dl, Rs):
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.tie_ap(Rs)
        return ctx.get_tie_ap()
    finally:
        ctx.close()


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def assert_close(got, ref, Rs):
    """got: Context.get_tie_ap(); ref: tie_oracle.over_queries(...).  The rule itself: tests/brute_refs.py (shared with
    tests/test_second_hand_gpu.py)."""
    WORST["fraction"] = max(WORST["fraction"], brute_refs.assert_tie_close(got, ref, Rs))


def from_groups(groups, b=None):
    """One query (the zero code, label 0) and a database whose table is the given one: groups[d] = (n_d, r_d) rows at distance d,
    r_d of them relevant.  -> qb, db, ql, dl"""
    b = b or max(1, len(groups) - 1)
    codes, labels = [], []
    for d, (n, r) in enumerate(groups):
        rel = np.zeros(n, dtype=bool)
        rel[(np.arange(r) * n) // max(r, 1)] = True    # spread over the index order (distinct places: n >= r)
        assert rel.sum() == r
        codes.append(np.tile((np.arange(b) < d).astype(np.uint8), (n, 1)))
        labels.append(np.where(rel[:, None], np.array([[1, 0]], np.int8), np.array([[0, 1]], np.int8)))
    return np.zeros((1, b), np.uint8), np.concatenate(codes), np.array([[1, 0]], np.int8), np.concatenate(labels)


def check_groups(groups, Rs, fn=T.exact, b=None):
    qb, db, ql, dl = from_groups(groups, b)
    n = [g[0] for g in groups]
    r = [g[1] for g in groups]
    a, rl = T.tables(qb, db, ql, dl)
    assert list(a[0][:len(n)]) == n and list(rl[0][:len(r)]) == r                # the table is the one asked for
    got = gpu_tie(qb, db, ql, dl, Rs)
    ref = T.over_queries(fn, a, rl, Rs)
    assert_close(got, ref, Rs)
    return got, ref


# ------------------------------------------------------------------ 1, 2: many queries
@functools.lru_cache(maxsize=None)
def small_case():
    rng = np.random.default_rng(11)
    Q, N, b, C = 60, 600, 8, 6
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.25).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.25).astype(np.int8)
    ql[0] = 0                                          # a query without labels: p_hit 0, AP NaN
    ql[2] = np.eye(C, dtype=np.int8)[3]
    dl[::5] = 0                                        # rows without labels
    for a in (qb, db, ql, dl):
        a.flags.writeable = False
    return qb, db, ql, dl


RS_SMALL = (1, 2, 7, 64, 257, 599, 600)
RS_MID = (1, 100, 1000, 4999, 5000)


def test_exact_many_queries():
    qb, db, ql, dl = small_case()
    assert len(qb) % 32 != 0 and (ql.sum(1) == 0).any() and (dl.sum(1) == 0).any()
    a, r = T.tables(qb, db, ql, dl)
    ref = T.over_queries(T.exact, a, r, RS_SMALL)
    assert np.isnan(ref["ap"][0]).all() and (ref["p_hit"][0] == 0).all()
    assert ((ref["p_hit"] > 0) & (ref["p_hit"] < 1)).any()                       # a first hit that depends on the order
    got = gpu_tie(qb, db, ql, dl, RS_SMALL)
    assert_close(got, ref, RS_SMALL)


@functools.lru_cache(maxsize=None)
def mid_case():
    """tests/test_rel_hist_gpu.py::case1's inputs, with the fast oracle on brute-force tables."""
    rng = np.random.default_rng(4)
    Q, N, b, C = 60, 5000, 16, 6
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.08).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.3).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.3).astype(np.int8)
    ql[0] = 0
    dl[::7] = 0
    ql[1] = 1
    a, r = T.tables(qb, db, ql, dl)
    ref = T.over_queries(T.fast, a, r, RS_MID)
    for x in (qb, db, ql, dl, a, r) + tuple(ref.values()):
        x.flags.writeable = False
    return qb, db, ql, dl, a, r, ref


def test_fast_oracle_mid_size():
    qb, db, ql, dl, a, r, ref = mid_case()
    got = gpu_tie(qb, db, ql, dl, RS_MID)
    assert_close(got, ref, RS_MID)
    ok = ~np.isnan(got["ap"])
    assert (got["ap_min"][ok] <= got["ap"][ok]).all() and (got["ap"][ok] <= got["ap_max"][ok]).all()
    # the envelope is wide where ties are: that is what the expectation is for
    assert (got["ap_max"][ok] - got["ap_min"][ok]).max() > 1e-3


# ------------------------------------------------------------------ 3: cut-group edges
@pytest.mark.parametrize("name, groups, Rs", [
    ("one group, pure hypergeometric", [(40, 13)], (1, 2, 17, 39, 40)),
    ("cut on a group boundary", [(10, 3), (20, 5), (30, 9)], (10, 30, 60)),
    ("groups of one row", [(1, 1), (1, 0), (1, 1)], (1, 2, 3)),
    ("groups of one row before a cut group", [(1, 0), (1, 1), (25, 6)], (2, 3, 9, 27)),
    ("c = 1", [(12, 4), (30, 11)], (1, 13)),
    ("r_t = 0", [(12, 4), (30, 0), (5, 2)], (13, 20, 42)),
    ("r_t = n_t", [(12, 4), (30, 30), (5, 2)], (13, 20, 42, 43)),
    ("first relevant rows only in the cut group", [(9, 0), (20, 3), (4, 1)], (10, 12, 28, 29)),
    ("no relevant row within R", [(9, 0), (20, 0), (4, 2)], (5, 9, 29, 30)),
    ("no relevant row at all", [(9, 0), (20, 0)], (1, 29)),
    ("empty distances between groups", [(0, 0), (7, 2), (0, 0), (9, 4)], (3, 7, 8, 16)),
    ("one row", [(1, 1)], (1,)),
    ("one irrelevant row", [(1, 0)], (1,)),
])
def test_cut_group_edges(name, groups, Rs):
    got, ref = check_groups(groups, Rs)
    if name == "first relevant rows only in the cut group":
        assert 0 < got["p_hit"][0, 0] < 1 and got["p_hit"][0, 2] == 1.0
    if name.startswith("no relevant row"):
        assert got["p_hit"][0, 0] == 0 and np.isnan(got["ap"][0, 0]) and np.isnan(got["ap_min"][0, 0]) and np.isnan(got["ap_max"][0, 0])
    if name == "one row":
        assert got["ap"][0, 0] == 1.0 and got["p_hit"][0, 0] == 1.0 and got["ap_min"][0, 0] == 1.0 and got["ap_max"][0, 0] == 1.0


# ------------------------------------------------------------------ 4: long sums
def test_long_cut_group_exact():
    """3000 rows in whole groups, then a cut group of 2000 rows with 700 relevant ones, of which R = 4000 takes 1000."""
    got, ref = check_groups([(1200, 300), (1800, 700), (2000, 700)], (4000,))
    assert ref["H"][0, 0] == 701


def test_very_long_single_group():
    """70 000 identical codes, R = 40 000: one workgroup walks 40 000 ranks and tens of thousands of values of h."""
    N, R, b = 70000, 40000, 8
    qb = np.zeros((1, b), np.uint8)
    db = np.zeros((N, b), np.uint8)
    ql = np.array([[1, 0]], np.int8)
    for r in (35000, N):
        dl = np.zeros((N, 2), np.int8)
        dl[:, 1] = 1
        dl[np.arange(r) * (N // r), :] = (1, 0)
        assert dl[:, 0].sum() == r
        got = gpu_tie(qb, db, ql, dl, (R,))
        h_lo, h_hi = max(0, R - (N - r)), min(R, r)
        tol = float(T.bound(R, h_hi - h_lo + 1))
        assert tol <= 1e-10
        assert got["p_hit"][0, 0] == 1.0
        assert got["rel_exp"][0, 0] == R * r / N and got["rel_lo"][0, 0] == h_lo and got["rel_hi"][0, 0] == h_hi
        ap, lo, hi = got["ap"][0, 0], got["ap_min"][0, 0], got["ap_max"][0, 0]
        assert lo <= ap <= hi
        if r == N:
            assert abs(ap - 1.0) <= tol and abs(lo - 1.0) <= tol and abs(hi - 1.0) <= tol
        else:
            assert abs(hi - 1.0) <= tol and lo < 0.5 * ap < ap < 0.6


# ------------------------------------------------------------------ 5: code lengths
@pytest.mark.parametrize("b", [1, 8, 33, 65, 128, 255])
def test_code_lengths(b):
    rng = np.random.default_rng(100 + b)
    Q, N, C = 5, 300, 4
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    qb[1] = 1 - db[0]                                  # distance b is populated
    dl = np.eye(C, dtype=np.int8)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int8)[rng.integers(0, C, Q)]
    a, r = T.tables(qb, db, ql, dl)
    assert a[1, b] >= 1
    if b == 255:
        assert (a == 0).mean() > 0.5                   # most distances are empty
    Rs = (1, 50, 299, 300)
    assert_close(gpu_tie(qb, db, ql, dl, Rs), T.over_queries(T.exact, a, r, Rs), Rs)


# ------------------------------------------------------------------ 6: against the existing path
def test_hg_map_lies_inside_the_envelope():
    qb, db, ql, dl, a, r, ref = mid_case()
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.tie_ap(RS_MID)
        t = ctx.get_tie_ap()
        strictly_inside = 0
        for j, R in enumerate(RS_MID):
            ap, rel = ctx.map(R)
            tol = T.bound(R, ref["H"][:, j])
            assert (rel >= t["rel_lo"][:, j]).all() and (rel <= t["rel_hi"][:, j]).all()
            hit = rel > 0
            assert np.array_equal(np.isnan(ap), ~hit)
            assert (t["p_hit"][hit, j] > 0).all()
            lo, hi = t["ap_min"][hit, j] * (1 - tol[hit]), t["ap_max"][hit, j] * (1 + tol[hit])
            assert (ap[hit] >= lo).all() and (ap[hit] <= hi).all()
            strictly_inside += ((ap[hit] > t["ap_min"][hit, j]) & (ap[hit] < t["ap_max"][hit, j])).sum()
        assert strictly_inside > len(qb)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7: row order
ORDER_SEED = 3


@functools.lru_cache(maxsize=None)
def order_case():
    rng = np.random.default_rng(ORDER_SEED)
    Q, N, b, C, R = 20, 500, 8, 5, 100
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl = np.eye(C, dtype=np.int8)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int8)[rng.integers(0, C, Q)]
    perm = rng.permutation(N)
    return qb, db, ql, dl, perm, R


def test_row_order_changes_map_but_no_tie_aware_bit():
    qb, db, ql, dl, perm, R = order_case()
    db2, dl2 = np.ascontiguousarray(db[perm]), np.ascontiguousarray(dl[perm])
    m1 = hamming_map.map_from_codes(qb, db, ql, dl, R)[0]
    m2 = hamming_map.map_from_codes(qb, db2, ql, dl2, R)[0]
    assert abs(m1 - m2) > 1e-6, (m1, m2)               # the index-order mAP is an accident of the row order ...
    g1, g2 = metric.MAP(qb, db, ql, dl, R), metric.MAP(qb, db2, ql, dl2, R)
    assert g1 != g2 and abs(g1 - m1) <= 1e-12 and abs(g2 - m2) <= 1e-12
    Rs = (1, 10, R, 499)
    t1, t2 = gpu_tie(qb, db, ql, dl, Rs), gpu_tie(qb, db2, ql, dl2, Rs)
    for k in ALL:                                      # ... the tie-aware outputs are not
        assert t1[k].tobytes() == t2[k].tobytes(), k
    o1 = X.tie_aware_map(qb, db, ql, dl, Rs)
    o2 = X.tie_aware_map(qb, db2, ql, dl2, Rs)
    assert o1["map"].tobytes() == o2["map"].tobytes()
    # and the index-order values lie around it
    j = Rs.index(R)
    assert np.nanmean(t1["ap_min"][:, j]) < min(m1, m2) and max(m1, m2) < np.nanmean(t1["ap_max"][:, j])


# ------------------------------------------------------------------ 8: label-pure ties
def test_label_pure_ties():
    """Every row carries its class prototype as code and a one-hot label: all rows at one distance from a query belong to one
    class (the prototypes' weights 0, 1, 3, 7 give distinct distances from each), so no order inside a tie changes anything."""
    rng = np.random.default_rng(21)
    C, b, N = 4, 8, 400
    proto = (np.arange(b)[None, :] < np.array([0, 1, 3, 7])[:, None]).astype(np.uint8)
    cls = rng.integers(0, C, N)
    cls[:C] = np.arange(C)
    db, dl = proto[cls], np.eye(C, dtype=np.int8)[cls]
    qb, ql = proto.copy(), np.eye(C, dtype=np.int8)
    counts = np.bincount(cls, minlength=C)
    Rs = tuple(sorted({1, int(counts[0]) // 2, int(counts[0]), int(counts[0]) + 5, N - 3, N}))
    a, r = T.tables(qb, db, ql, dl)
    assert ((r == 0) | (r == a)).all()
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.tie_ap(Rs)
        t = ctx.get_tie_ap()
        ref = T.over_queries(T.exact, a, r, Rs)
        assert_close(t, ref, Rs)
        assert (ref["H"] == 1).all()
        assert t["ap_min"].tobytes() == t["ap_max"].tobytes()
        tol = T.bound(np.asarray(Rs)[None, :], 1)
        assert (np.abs(t["ap"] - t["ap_max"]) <= tol * t["ap_max"]).all()
        assert np.array_equal(t["rel_lo"], t["rel_hi"]) and np.array_equal(t["rel_exp"], t["rel_lo"].astype(np.float64))
        assert ((t["p_hit"] == 0) | (t["p_hit"] == 1)).all()
        for j, R in enumerate(Rs):
            ap, rel = ctx.map(R)
            assert np.array_equal(rel, t["rel_lo"][:, j])
            assert (np.abs(ap - t["ap"][:, j]) <= tol[0, j] * ap).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9: state and arguments
def launches(ctx):
    return {k: n for k, (ms, n) in ctx.timing_read().items() if n}


def test_state_and_arguments():
    qb, db, ql, dl = small_case()
    N = len(db)
    ctx = _native.Context(0)
    try:
        raises(STATE, ctx.tie_ap, (1, 5))                                        # nothing loaded
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1])
        raises(STATE, ctx.tie_ap, (1, 5))                                        # no queries
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        raises(STATE, ctx.get_tie_ap)                                            # no pass yet
        assert ctx.get_stat("rel_hist_variant") == 0
        for bad in ((5, 1), (5, 5), (0, 5), (1, N + 1), tuple(range(1, 66)), ()):
            raises(ARG, ctx.tie_ap, bad)
        raises(STATE, ctx.get_tie_ap)                                            # a refused call leaves no results
        assert ctx.get_stat("rel_hist_variant") == 0                             # ... and has run no pass
        bytes0 = ctx.get_stat("device_bytes")
        ctx.timing_enable(2)
        ctx.timing_reset()
        Rs = tuple(range(1, 65))                                                 # 64 cut-offs are fine
        ctx.tie_ap(Rs)
        first = launches(ctx)
        assert first.get("k_hist_rel") == 1 and first.get("k_hist_rel_reduce") == 1 and first.get("k_tie_ap") == 1, first
        assert ctx.get_stat("rel_hist_variant") == 1
        assert ctx.get_stat("device_bytes") >= bytes0 + 7 * 8 * len(qb) * 64
        a = ctx.get_tie_ap()
        ctx.timing_reset()
        ctx.tie_ap(Rs)                                                           # the tables are there: no second histogram pass
        second = launches(ctx)
        assert second.get("k_tie_ap") == 1 and "k_hist_rel" not in second and "k_hist_rel_reduce" not in second, second
        ctx.timing_reset()
        ctx.rel_hist()                                                           # the caller's own pass serves as well
        ctx.tie_ap((7,))
        third = launches(ctx)
        assert third.get("k_hist_rel") == 1 and third.get("k_tie_ap") == 1, third
        ctx.timing_enable(False)
        assert ctx.get_tie_ap()["ap"].tobytes() == a["ap"][:, 6:7].tobytes()
        ta, tr = T.tables(qb, db, ql, dl)
        ga, gr = ctx.get_rel_hist()                                              # the tables hg_tie_ap computed are hg_rel_hist's
        assert np.array_equal(ga.T, ta) and np.array_equal(gr.T, tr)
        # a refused call ends the previous results too
        raises(ARG, ctx.tie_ap, (2, 1))
        raises(STATE, ctx.get_tie_ap)
        # reloads
        ctx.tie_ap((7,))
        ctx.set_queries(metric.pack_codes(qb[:10].copy()), metric.pack_labels(ql[:10].copy()))
        raises(STATE, ctx.get_tie_ap)
        ctx.tie_ap((7,))
        assert ctx.get_tie_ap()["ap"].tobytes() == a["ap"][:10, 6:7].tobytes()
        ctx.set_database(metric.pack_codes(db[:200].copy()), metric.pack_labels(dl[:200].copy()), db.shape[1], dl.shape[1])
        raises(STATE, ctx.get_tie_ap)                                            # a new database wants its queries again ...
        raises(STATE, ctx.tie_ap, (200,))
        ctx.set_queries(metric.pack_codes(qb[:10].copy()), metric.pack_labels(ql[:10].copy()))
        raises(STATE, ctx.get_tie_ap)                                            # ... and the old results are not theirs
        raises(ARG, ctx.tie_ap, (201,))
        ctx.tie_ap((200,))
        assert ctx.get_tie_ap()["ap"].shape == (10, 1)
        # hg_trim
        ctx.trim()
        raises(STATE, ctx.get_tie_ap)
        ctx.tie_ap((200,))
        ctx.get_tie_ap()
    finally:
        ctx.close()
    # a shard: the cut at R needs the whole database
    ctx = code_ctx(qb, db[:300], ql, dl[:300], idx_base=100, n_total=400)
    try:
        msg = raises(STATE, ctx.tie_ap, (1, 5))
        assert "whole database" in msg
        raises(STATE, ctx.get_tie_ap)
    finally:
        ctx.close()


def test_leaves_the_map_path_alone(case_cache):
    c = case_cache("c3_nus_q64")
    g = cases.load_golden("c3_nus_q64")
    R = c["R"]
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    assert R == 5000
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ap, rel = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.tie_ap((100, R))
        t = ctx.get_tie_ap()
        ap, rel = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        hit = rel > 0
        assert (rel >= t["rel_lo"][:, 1]).all() and (rel <= t["rel_hi"][:, 1]).all()
        assert (ap[hit] >= t["ap_min"][hit, 1] * (1 - 1e-10)).all() and (ap[hit] <= t["ap_max"][hit, 1] * (1 + 1e-10)).all()
        ctx.trim()                                                               # the step in flight below finds no tables: the pass runs beside it
        ap, rel = ctx.map(R)
        ctx.map_begin(R)
        ctx.tie_ap((100, R))
        ap, rel = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        t2 = ctx.get_tie_ap()
        for k in ALL:
            assert t2[k].tobytes() == t[k].tobytes(), k
        # the staged path's own state survives: a histogram, then the pass, then the plan on that histogram
        ctx.hist()
        h = ctx.get_hist()
        ctx.tie_ap((R,))
        assert np.array_equal(ctx.get_hist(), h)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 10: determinism
def test_two_runs_give_identical_bits_whatever_q_is():
    qb, db, ql, dl, a, r, ref = mid_case()
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.tie_ap(RS_MID)
        x = ctx.get_tie_ap()
        ctx.tie_ap(RS_MID)
        y = ctx.get_tie_ap()
        for k in ALL:
            assert x[k].tobytes() == y[k].tobytes(), k
        # a query's results are a function of its two columns and R: alone, or as one cut-off of a longer list, the same bits
        ctx.set_queries(metric.pack_codes(qb[37:38].copy()), metric.pack_labels(ql[37:38].copy()))
        ctx.tie_ap((1000,))
        z = ctx.get_tie_ap()
        for k in ALL:
            assert z[k].tobytes() == x[k][37:38, 2:3].tobytes(), k
    finally:
        ctx.close()


# ------------------------------------------------------------------ 11: the Python surface
@pytest.mark.parametrize("spelling", ["bits", "pm1"])
def test_python_surface(spelling):
    qb, db, ql, dl = small_case()
    q_in, d_in = (qb, db) if spelling == "bits" else (2 * qb.astype(np.int8) - 1, 2 * db.astype(np.int8) - 1)
    a, r = T.tables(qb, db, ql, dl)
    ref = T.over_queries(T.fast, a, r, RS_SMALL)
    out = X.tie_aware_map(q_in, d_in, ql, dl, RS_SMALL)
    pq = out["per_query"]
    assert sorted(pq) == sorted(("ap", "p_hit", "ap_min", "ap_max", "rel_exp", "rel_lo", "rel_hi", "total_rel"))
    assert_close(pq, ref, RS_SMALL)
    assert np.array_equal(pq["total_rel"], r.sum(1)) and pq["total_rel"].dtype == np.int64
    # map follows the p_hit weighting
    assert out["map"].shape == (len(RS_SMALL),)
    partial = 0
    for j, R in enumerate(RS_SMALL):
        w = ref["p_hit"][:, j]
        partial += ((w > 0) & (w < 1)).sum()
        m = (w[w > 0] * ref["ap"][w > 0, j]).sum() / w.sum()
        tol = float(T.bound(R, ref["H"][:, j].max())) + len(qb) * 2.0 ** -52
        assert abs(out["map"][j] - m) <= tol * m, (j, out["map"][j], m)
    assert partial > 0
    # expected precision and recall at k from brute-force tables
    prec, rec = X.tie_aware_precision_recall_at_k(q_in, d_in, ql, dl, RS_SMALL)
    total = r.sum(1)
    ok = total > 0
    assert not ok.all()
    eps = (4 + len(qb)) * 2.0 ** -52
    for j, k in enumerate(RS_SMALL):
        p = (ref["rel_exp"][:, j] / k).mean()
        rc = (ref["rel_exp"][ok, j] / total[ok]).mean()
        assert abs(prec[j] - p) <= eps * p and abs(rec[j] - rc) <= eps * rc
    assert rec[-1] == 1.0                              # k = N


def test_map_is_nan_without_any_hit():
    qb, db, ql, dl = small_case()
    out = X.tie_aware_map(qb[:1], db, ql[:1], dl, (5, 600))                      # the query without labels
    assert np.isnan(out["map"]).all() and (out["per_query"]["p_hit"] == 0).all()
    prec, rec = X.tie_aware_precision_recall_at_k(qb[:1], db, ql[:1], dl, (5, 600))
    assert (prec == 0).all() and np.isnan(rec).all()


def test_largest_error_for_the_record():
    """Printed for DESIGN.md: the largest error of the tests above as a fraction of the bound (run the whole file with -s)."""
    print("largest observed error: %.3g of the bound" % WORST["fraction"])
    assert WORST["fraction"] <= 1.0

"""The re-ranked Hamming ranking on the GPU (hg_topr_rerank / hg_map_rerank / hg_get_rerank_scores: k_rr_scan, k_rr_collect, k_rr_score,
k_rr_order) against tests/rerank_oracle.py: Hamming distance of the sign bits, then the float32 inner product of the features inside
equal distances, then the database index (needs an MI355X).

Everything is compared with ==: idx, dist and match as arrays, scores and APs by their bits."""
import functools
import types

import numpy as np
import pytest

from hashgan_amd import MAPs, _native
from hashgan_amd import extra_metrics as X
from oracle import hamming_map as H
from oracle import real_map as RM
from tests import rerank_oracle as RO

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG
Q, N = 70, 773                                           # two query tiles, Qpad = 128 != Q; with min_segment = 16 several segments, a
OPTS = (("min_segment", 16),)                            # ragged last one and a ragged batch tail


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def new_ctx(qf, dbf, ql, dl, opts=OPTS, keep_floats=1, **kw):
    ctx = _native.Context(0)
    ctx.set_option("keep_floats", keep_floats)
    for k, v in opts:
        ctx.set_option(k, v)
    ctx.set_database_f32(dbf, dl, **kw)
    ctx.set_queries_f32(qf, ql)
    return ctx


def outputs(ctx, R):
    """Everything a re-rank leaves, as bytes-comparable arrays."""
    ap, rel = ctx.map_rerank(R)
    idx, dist = ctx.get_topr()
    return dict(idx=idx, dist=dist, score=ctx.get_rerank_scores(), match=ctx.get_match(), ap=ap, rel=rel)


def assert_equals_oracle(got, o):
    assert (got["idx"] == o["idx"]).all()
    assert (got["dist"] == o["dist"]).all()
    assert bits(got["score"]) == bits(o["score"])
    assert (got["match"] == o["match"]).all()
    assert (got["rel"] == o["rel"]).all()
    assert bits(got["ap"]) == bits(o["ap"])


#         b,   R,   C, multi-hot
CASES = {"b8_r200_c10": (8, 200, 10, False),
         "b33_rN_c81_multi_hot": (33, N, 81, True),
         "b70_r1_c10": (70, 1, 10, False),
         "b130_r100_c200_gather_match": (130, 100, 200, False),
         "b255_r300_c10_complement": (255, 300, 10, False)}


@functools.lru_cache(maxsize=None)
def case(name):
    b, R, C, multi = CASES[name]
    qf, dbf, ql, dl = RO.generate(Q, N, b, C, seed=b * 1000 + C, multi_hot=multi)
    if b == 255:
        dbf[700] = -qf[3]                                # the exact sign complement of a query: d = 255 occurs
        assert (qf[3] != 0).all()
    # a query with no relevant row anywhere: AP NaN, rel 0
    ql[11] = 0
    for a in (qf, dbf, ql, dl):
        a.setflags(write=False)
    return qf, dbf, ql, dl, RO.rerank(qf, dbf, ql, dl, R)


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_oracle(name):
    b, R, C, _ = CASES[name]
    qf, dbf, ql, dl, o = case(name)
    d, s = o["d"], o["s"]
    if b == 255:
        assert d[3, 700] == 255
    assert o["rel"][11] == 0 and np.isnan(o["ap"][11])
    if R < N:
        # the generator is not degenerate: the threshold group is cut strictly inside, the kept set differs from the canonical
        # (distance, index) set, and duplicated rows put equal (d, s) next to each other
        cut_inside = differs = 0
        canon, _ = H.topr_from_codes(qf > 0, dbf > 0, R)
        for q in range(Q):
            t = o["dist"][q, -1]
            cut_inside += int((d[q] <= t).sum() > R and (d[q] < t).sum() < R)
            differs += int(set(canon[q].tolist()) != set(o["idx"][q].tolist()))
        print("cut inside: %d queries, set differs from hg_topr's: %d queries" % (cut_inside, differs))
        assert cut_inside >= 1
        assert differs >= 1
    if R > 1:
        adjacent = ((o["dist"][:, 1:] == o["dist"][:, :-1]) & (o["score"][:, 1:] == o["score"][:, :-1])).any(1).sum()
        print("adjacent records of equal (d, s): %d queries" % adjacent)
        assert adjacent >= 1
    ctx = new_ctx(qf, dbf, ql, dl)
    try:
        assert_equals_oracle(outputs(ctx, R), o)
        assert ctx.get_stat("rerank_records") == int(sum((d[q] <= o["dist"][q, -1]).sum() for q in range(Q)))
        assert ctx.get_stat("rerank_chunks") == 1 and ctx.get_stat("rerank_groups_global") == 0 and ctx.get_stat("rerank_groups_lds") >= Q
        # topr_rerank alone leaves the same lists
        idx, dist, score = ctx.topr_rerank(R)
        assert (idx == o["idx"]).all() and (dist == o["dist"]).all() and bits(score) == bits(o["score"])
        assert (ctx.get_match() == o["match"]).all()
    finally:
        ctx.close()


def test_pm1_features_equal_hg_topr():
    rng = np.random.default_rng(24)
    b, R, C = 24, 300, 6
    dbf = (rng.integers(0, 2, (N, b)) * 2 - 1).astype(np.float32)
    qf = np.where(rng.random((Q, b)) < 0.1, -1, 1).astype(np.float32) * dbf[rng.integers(0, N, Q)]
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, C, Q)]
    ctx = new_ctx(qf, dbf, ql, dl)
    try:
        got = outputs(ctx, R)
        ap, rel = ctx.map(R)
        ctx.topr(R)
        idx, dist = ctx.get_topr()
        assert (got["idx"] == idx).all() and (got["dist"] == dist).all()
        assert (got["match"] == ctx.get_match()).all()
        assert bits(got["ap"]) == bits(ap) and (got["rel"] == rel).all()
        assert (got["score"] == (b - 2 * dist.astype(np.int64)).astype(np.float32)).all()
    finally:
        ctx.close()


def test_all_positive_features_equal_hg_topr_real():
    rng = np.random.default_rng(7)
    b, n, nq, R, C = 24, 3000, 7, 700, 5
    dbf = rng.uniform(0.05, 1.0, (n, b)).astype(np.float32)
    qf = rng.uniform(0.05, 1.0, (nq, b)).astype(np.float32)
    dbf[5::97] = dbf[4::97]
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, C, n)]
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, C, nq)]
    ctx = new_ctx(qf, dbf, ql, dl)
    try:
        idx, dist, score = ctx.topr_rerank(R)
        ridx, rscore = ctx.topr_real(R)
        assert (dist == 0).all()
        assert (idx == ridx).all()
        assert bits(score) == bits(rscore)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def big_group():
    """Every code equal: one group of all N rows per query, cut inside."""
    rng = np.random.default_rng(40)
    n, nq, b, R, C = 40000, 8, 16, 25000, 4
    dbf = rng.uniform(0.05, 1.0, (n, b)).astype(np.float32)
    qf = rng.uniform(0.05, 1.0, (nq, b)).astype(np.float32)
    dbf[5::97] = dbf[4::97]
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, C, n)]
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, C, nq)]
    return qf, dbf, ql, dl, R, RO.rerank(qf, dbf, ql, dl, R)


def test_a_group_beyond_the_lds():
    qf, dbf, ql, dl, R, o = big_group()
    ctx = new_ctx(qf[:2], dbf, ql[:2], dl)
    try:
        got = outputs(ctx, R)
        assert ctx.get_stat("rerank_groups_global") >= 1
        assert ctx.get_stat("rerank_records") == 2 * len(dbf)
        assert_equals_oracle(got, {k: v[:2] for k, v in o.items()})
    finally:
        ctx.close()


def test_chunks_leave_the_same_bytes():
    qf, dbf, ql, dl, R, o = big_group()
    whole = new_ctx(qf, dbf, ql, dl)
    cut = new_ctx(qf, dbf, ql, dl, opts=OPTS + (("dense_budget_mb", 1),))
    try:
        a, b_ = outputs(whole, R), outputs(cut, R)
        assert whole.get_stat("rerank_chunks") == 1
        assert cut.get_stat("rerank_chunks") >= 2
        for k in a:
            assert bits(a[k]) == bits(b_[k]), k
        assert_equals_oracle(b_, o)
    finally:
        whole.close()
        cut.close()


def test_same_bytes_twice_and_in_another_geometry():
    b, R, C, _ = CASES["b8_r200_c10"]
    qf, dbf, ql, dl, o = case("b8_r200_c10")
    ctx = new_ctx(qf, dbf, ql, dl)
    other = new_ctx(qf, dbf, ql, dl, opts=(("min_segment", 256), ("target_units", 64)))
    try:
        first, second, third = outputs(ctx, R), outputs(ctx, R), outputs(other, R)
        assert ctx.get_stat("segments") != other.get_stat("segments")
        for k in first:
            assert bits(first[k]) == bits(second[k]) == bits(third[k]), k
        assert_equals_oracle(first, o)
    finally:
        ctx.close()
        other.close()


def test_downstream_calls_take_the_lists():
    b, R, C, _ = CASES["b8_r200_c10"]
    qf, dbf, ql, dl, o = case("b8_r200_c10")
    ctx = new_ctx(qf, dbf, ql, dl)
    try:
        ks = np.array([1, 7, 64, R], np.int64)
        per_k = [ctx.map_rerank(int(k)) for k in ks]
        ctx.topr_rerank(R, download=False)
        ctx.ap_at(ks)
        ap, rel = ctx.get_ap_at()
        for j in range(len(ks)):
            assert bits(ap[:, j]) == bits(per_k[j][0]), ks[j]
            assert (rel[:, j] == per_k[j][1]).all()
        # graded relevance along the lists: the hits are the prefix sums of the match bits
        ctx.graded(ks, np.arange(C + 1, dtype=np.float64), 1.0 / np.log2(np.arange(2, R + 2, dtype=np.float64)))
        hits = ctx.get_graded()[1]
        assert (hits == np.cumsum(o["match"], axis=1)[:, ks - 1]).all()
        assert bits(ctx.get_rerank_scores()) == bits(o["score"])
        # a later ranking ends the re-rank: the score list is no longer its lists'
        ctx.topr(R)
        raises(STATE, ctx.get_rerank_scores)
        ctx.topr_rerank(R, download=False)
        assert bits(ctx.get_rerank_scores()) == bits(o["score"])
        ctx.topr_real(R)
        raises(STATE, ctx.get_rerank_scores)
        ctx.topr_rerank(R, download=False)
        ctx.set_queries_f32(qf, ql)                      # a reload ends it too
        raises(STATE, ctx.get_rerank_scores)
        ctx.topr_rerank(R, download=False)
        before = ctx.get_stat("device_bytes")
        ctx.trim()
        assert ctx.get_stat("device_bytes") < before
        raises(STATE, ctx.get_rerank_scores)
        assert_equals_oracle(outputs(ctx, R), o)
    finally:
        ctx.close()


def test_refusals():
    qf, dbf, ql, dl, o = case("b8_r200_c10")
    pm1 = np.where(dbf > 0, 1, -1).astype(np.float32), np.where(qf > 0, 1, -1).astype(np.float32)
    no_floats = new_ctx(pm1[1], pm1[0], ql, dl, keep_floats=0)
    shard = new_ctx(qf, dbf, ql, dl, idx_base=5, n_total=N + 5)
    ctx = new_ctx(qf, dbf, ql, dl)
    try:
        raises(STATE, no_floats.topr_rerank, 10)
        raises(STATE, no_floats.map_rerank, 10)
        raises(STATE, shard.topr_rerank, 10)
        raises(ARG, ctx.topr_rerank, 0)
        raises(ARG, ctx.topr_rerank, N + 1)
        raises(STATE, ctx.get_rerank_scores)             # no ranking yet
        assert_equals_oracle(outputs(ctx, 200), o)       # a refused call leaves the context usable
    finally:
        for c in (no_floats, shard, ctx):
            c.close()


def sides(qf, dbf, ql, dl):
    return types.SimpleNamespace(output=dbf, label=dl), types.SimpleNamespace(output=qf, label=ql)


def test_python_surface():
    b, R, C, _ = CASES["b8_r200_c10"]
    qf, dbf, ql, dl, o = case("b8_r200_c10")
    database, query = sides(qf, dbf, ql, dl)
    m = MAPs(R, rerank=True)
    plain, signed = MAPs(R), MAPs(R, binarize=True)
    try:
        assert m.get_maps_by_feature(database, query) == RO.mean_ap(o["ap"])
        ks = [1, 7, 64, R]
        at = m.get_maps_at(database, query, ks)
        for j, k in enumerate(ks):
            mk = MAPs(k, rerank=True)
            try:
                assert at[j] == mk.get_maps_by_feature(database, query), k
            finally:
                mk.close()
        # the existing modes on the same objects: the inner-product ranking and the canonical Hamming ranking, as before
        assert plain.get_maps_by_feature(database, query) == RM.map_from_features(qf, dbf, ql, dl, R)[0]
        assert signed.get_maps_by_feature(database, query) == H.map_from_codes(qf > 0, dbf > 0, ql, dl, R)[0]
        assert m.get_maps_by_feature(database, query) == RO.mean_ap(o["ap"])
    finally:
        for x in (m, plain, signed):
            x.close()
    idx, dist, score, match = X.rerank_topr(qf, dbf, ql, dl, R)
    assert (idx == o["idx"]).all() and (dist == o["dist"]).all() and bits(score) == bits(o["score"]) and (match == o["match"]).all()


def test_python_surface_takes_device_tensors():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    b, R, C, _ = CASES["b8_r200_c10"]
    qf, dbf, ql, dl, o = case("b8_r200_c10")
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    database = types.SimpleNamespace(output=t(dbf), label=t(dl))
    query = types.SimpleNamespace(output=t(qf), label=t(ql))
    m = MAPs(R, rerank=True)
    try:
        assert m.get_maps_by_feature(database, query) == RO.mean_ap(o["ap"])
    finally:
        m.close()

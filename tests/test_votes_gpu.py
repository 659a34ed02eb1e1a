"""Class votes along the ranked lists on the GPU (hg_votes: k_votes, k_vote_confusion; needs an MI355X) against brute-force NumPy -- the
full Q x N Hamming matrix, a stable argsort, labels[order], a cumulative sum per class; nothing is derived from the library's own lists
(except where the ranking is somebody else's test: the real-valued and the re-ranked lists) -- and hashgan_amd.extra_metrics'
knn_vote_at_k / MAPs.get_knn_at on top.

Every comparison is == on integers (or on quotients of the same two integers): no tolerance anywhere."""
import functools
import types

import numpy as np
import pytest
from tests import brute_refs, cases
from hashgan_amd import MAPs, _native, metric
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG


hamming, tables_of = brute_refs.hamming, brute_refs.vote_tables      # (shared with tests/test_second_hand_gpu.py)


def brute(qb, db, ql, dl, R, ks):
    order = np.argsort(hamming(qb, db), axis=1, kind="stable")[:, :R]
    return tables_of(dl[order], ql, ks)


def from_lists(idx, ql, dl, ks):
    return tables_of(dl[idx.astype(np.int64)], ql, ks)


def code_ctx(qb, db, ql, dl, idx_base=0, n_total=None, qwords=None, dwords=None):
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl) if dwords is None else dwords, db.shape[1], dl.shape[1], idx_base, n_total)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql) if qwords is None else qwords)
    return ctx


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def assert_tables(ctx, ref):
    votes, (pred, top), conf = ctx.get_votes(), ctx.get_vote_pred(), ctx.get_vote_confusion()
    assert votes.dtype == np.uint32 and pred.dtype == np.int32 and top.dtype == np.int64 and conf.dtype == np.int64
    assert votes.shape == ref[0].shape and np.array_equal(votes, ref[0]), "votes"
    assert np.array_equal(top, ref[2]), "top"
    assert np.array_equal(pred, ref[1]), "pred"
    assert conf.shape == ref[3].shape and np.array_equal(conf, ref[3]), "conf"


# ------------------------------------------------------------------ 1. chunk edges, single label
KS1 = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)
R1 = 1000


@functools.lru_cache(maxsize=None)
def case1():
    rng = np.random.default_rng(21)
    Q, N, b, C = 70, 3000, 16, 10
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.08).astype(np.uint8)
    dl = np.eye(C, dtype=np.int8)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int8)[rng.integers(0, C, Q)]
    dl[::7] = 0
    ql[0] = 0
    ref = brute(qb, db, ql, dl, R1, KS1)
    for a in (qb, db, ql, dl) + ref:
        a.flags.writeable = False
    return dict(qb=qb, db=db, ql=ql, dl=dl, ref=ref)


def test_chunk_edges_single_label():
    c = case1()
    votes, pred, top, conf = c["ref"]
    # the case holds what the tie rule and pred = -1 need
    tied = ((votes == top[:, :, None].astype(np.uint32)).sum(2) >= 2) & (top > 0)
    assert tied.any() and tied[:, 2:].any(), "no (q, k) where two classes tie for the maximum"
    assert (top == 0).any() and ((pred == -1) == (top == 0)).all(), "no (q, k) where every vote is 0"
    assert (conf[:, :, :].sum(2)[-1] > 0).sum() == 10 and conf[:, 0].sum() > 0
    ctx = code_ctx(c["qb"], c["db"], c["ql"], c["dl"])
    try:
        ctx.topr(R1)
        ctx.votes(KS1)
        assert ctx.get_stat("votes_cutoffs") == len(KS1)
        assert_tables(ctx, c["ref"])
        # cut-offs short of the lists' end, and only one of them
        ctx.votes((513,))
        assert ctx.get_stat("votes_cutoffs") == 1
        assert_tables(ctx, tuple(np.ascontiguousarray(t[:, 10:11]) for t in c["ref"][:3]) + (np.ascontiguousarray(c["ref"][3][10:11]),))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. label-word edges, multi-hot
@pytest.mark.parametrize("C", [1, 63, 64, 65, 81, 128, 129, 255])
def test_label_word_edges_multi_hot(C):
    """LW = 1, 2, 3, 4 label words, classes 31 / 32 / 63 / 64 / C - 1, a row and a query with every label, one of each with none; and
    the pad bits of the last label word set on both tables (packed words handed over as they are): never counted, never a counter."""
    rng = np.random.default_rng(1000 + C)
    Q, N, b = 5, 600, 32
    ks = (1, 300, 600)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.15).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.3).astype(np.int8)
    dl[::5, C - 1] = 1
    dl[::3, min(31, C - 1)] = 1
    dl[17], dl[18] = 1, 0
    ql[1], ql[2] = 1, 0
    ql[3, C - 1] = 1
    ref = brute(qb, db, ql, dl, N, ks)
    assert ref[0][:, 2, C - 1].min() >= N // 5 and ref[0].max() <= N
    dwords, qwords = metric.pack_labels(dl), metric.pack_labels(ql)
    if C % 64:
        pad = np.uint64(((1 << 64) - 1) ^ ((1 << (C % 64)) - 1))
        dwords[::2, -1] |= pad
        qwords[:, -1] |= pad
    ctx = code_ctx(qb, db, ql, dl, qwords=qwords, dwords=dwords)
    try:
        ctx.topr(N)
        ctx.votes(ks)
        assert_tables(ctx, ref)
    finally:
        ctx.close()


def test_more_queries_than_a_confusion_segment():
    """k_vote_confusion splits the queries into segments of 512 and adds the segments' sums: two segments, the second ragged."""
    rng = np.random.default_rng(23)
    Q, N, b, C, R = 600, 400, 24, 70, 130
    ks = (1, 64, 130)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl = (rng.random((N, C)) < 0.05).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.05).astype(np.int8)
    ql[512:, 69] = 1                                                      # a class only the second segment's queries carry
    ql[:512, 69] = 0
    ref = brute(qb, db, ql, dl, R, ks)
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.topr(R)
        ctx.votes(ks)
        assert_tables(ctx, ref)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. other rankings
KS3 = (1, 100, 500)
R3 = 500


@functools.lru_cache(maxsize=None)
def real_case():
    """tanh-like float features; C = 81 multi-hot."""
    rng = np.random.default_rng(33)
    Q, N, F, C = 8, 2000, 32, 81
    dbf = np.tanh(rng.standard_normal((N, F)) * 1.5).astype(np.float32)
    qf = np.tanh(rng.standard_normal((Q, F)) * 1.5).astype(np.float32)
    dl = (rng.random((N, C)) < 0.04).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.06).astype(np.int64)
    ql[0] = 0
    for a in (dbf, qf, dl, ql):
        a.flags.writeable = False
    return dict(qf=qf, dbf=dbf, ql=ql, dl=dl)


@functools.lru_cache(maxsize=None)
def real_case_tables(rerank):
    """The tables of the real-valued / re-ranked ranking at R3, in NumPy from the lists the ranking's own getter returns (the ranking is
    tested elsewhere), and what hg_votes left on the same context."""
    c = real_case()
    ctx = _native.Context(0)
    try:
        ctx.set_option("keep_floats", 1)
        ctx.set_database_f32(c["dbf"], c["dl"])
        ctx.set_queries_f32(c["qf"], c["ql"])
        idx = ctx.topr_rerank(R3)[0] if rerank else ctx.topr_real(R3)[0]
        ref = from_lists(idx, c["ql"], c["dl"], KS3)
        ctx.votes(KS3)
        got = (ctx.get_votes(), ) + ctx.get_vote_pred() + (ctx.get_vote_confusion(),)
    finally:
        ctx.close()
    return ref, got


@pytest.mark.parametrize("rerank", [False, True])
def test_other_rankings(rerank):
    ref, got = real_case_tables(rerank)
    assert ref[0][:, 2].sum() > 0 and (ref[1] >= 0).any()
    for name, a, r in zip(("votes", "pred", "top", "conf"), got, ref):
        assert a.dtype == r.dtype and np.array_equal(a, r), name


# ------------------------------------------------------------------ 4. cross-checks against existing kernels at a medium shape
def test_cross_checks_at_a_medium_shape():
    rng = np.random.default_rng(41)
    Q, N, b, R = 256, 100000, 64, 5000
    ks = (100, 1000, 5000)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.2).astype(np.uint8)
    # single label: the votes for the query's own class are the hits hg_ap_at counts
    lab_d, lab_q = rng.integers(0, 10, N), rng.integers(0, 10, Q)
    dl, ql = np.eye(10, dtype=np.int8)[lab_d], np.eye(10, dtype=np.int8)[lab_q]
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.topr(R)
        ctx.votes(ks)
        ctx.ap_at(ks)
        votes, (pred, top), conf = ctx.get_votes(), ctx.get_vote_pred(), ctx.get_vote_confusion()
        rel = ctx.get_ap_at()[1]
        assert np.array_equal(votes[np.arange(Q), :, lab_q].astype(np.int64), rel)
        assert np.array_equal(votes.astype(np.int64).sum(2), np.broadcast_to(np.array(ks), (Q, 3)))     # every row has one label
        assert np.array_equal(top, votes.max(2)) and np.array_equal(pred, votes.argmax(2))
        assert np.array_equal(conf, np.einsum("qa,qjb->jab", ql.astype(np.int64), votes.astype(np.int64)))
        # C = 6 multi-hot rows, queries that carry every label: the votes add up to the grades hg_graded sums
        dl6 = (rng.random((N, 6)) < 0.3).astype(np.int8)
        ql6 = np.ones((Q, 6), np.int8)
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl6), b, 6)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql6))
        ctx.topr(R)
        ctx.votes(ks)
        ctx.graded(ks, X.gain_table("linear", 6), X.discount_table(R))
        votes6 = ctx.get_votes().astype(np.int64)
        assert np.array_equal(votes6.sum(2), ctx.get_graded()[0])
        assert np.array_equal(ctx.get_vote_confusion(), np.broadcast_to(votes6.sum(0)[:, None, :], (3, 6, 6)))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. state and arguments
def raw(x):
    if isinstance(x, dict):
        x = tuple(x[k] for k in sorted(x))
    return tuple(a.tobytes() for a in x) if isinstance(x, tuple) else x.tobytes()


def test_state_and_arguments():
    c = case1()
    qb, db, ql, dl = c["qb"], c["db"], c["ql"], c["dl"]
    R = 100
    getters = ("get_votes", "get_vote_pred", "get_vote_confusion")
    ctx = code_ctx(qb, db, ql, dl)

    def all_refused():
        for g in getters:
            raises(STATE, getattr(ctx, g))

    try:
        raises(STATE, ctx.votes, (1, 5))                                     # no ranking yet
        all_refused()
        ctx.map(R)
        msg = raises(STATE, ctx.votes, (1, 5))                               # hg_map leaves no lists
        assert "hg_topr" in msg and "hg_map and hg_map_real write none" in msg
        ctx.topr(R)
        all_refused()                                                        # a ranking alone computes nothing
        ctx.votes((1, R))
        for g in getters:
            getattr(ctx, g)()
        for bad in ((5, 1), (5, 5), (1, R + 1), (0, 5), tuple(range(1, 66)), ()):
            ctx.votes((1, R))
            raises(ARG, ctx.votes, bad)
            all_refused()                                                    # a refused call ends the earlier valid result
        ctx.votes((1, R))
        assert ctx._lib.hg_votes(ctx._h, None, 1) == ARG                     # a null pointer
        all_refused()
        ks = tuple(range(1, 65))                                             # 64 cut-offs are fine
        ctx.votes(ks)
        ref = brute(qb, db, ql, dl, R, ks)
        assert_tables(ctx, ref)
        assert ctx._lib.hg_get_votes(ctx._h, None) == ARG and ctx._lib.hg_get_vote_confusion(ctx._h, None) == ARG
        assert ctx._lib.hg_get_vote_pred(ctx._h, None, None) == 0            # both outputs unwanted: allowed, like hg_get_ap_at
        assert_tables(ctx, ref)
        # a later ranking ends the results (hg_map too); the other side metrics' results survive a votes call
        ctx.topr(R)
        all_refused()
        ctx.rel_hist(), ctx.grade_hist(), ctx.tie_ap((1, R)), ctx.joint_hist(), ctx.ap_at((1, R))
        ctx.graded((1, R), X.gain_table("exp", 10), X.discount_table(R), keep_grades=True)
        others = ("get_rel_hist", "get_grade_hist", "get_tie_ap", "get_joint_hist", "get_ap_at", "get_graded", "get_grades")
        want = {g: raw(getattr(ctx, g)()) for g in others}
        ctx.votes((1, R))
        raises(ARG, ctx.votes, (5, 1))
        ctx.votes((1, R))
        for g in others:
            assert raw(getattr(ctx, g)()) == want[g], g
        ctx.map(R)
        all_refused()
        # reloads
        ctx.topr(R)
        ctx.votes((R,))
        ctx.set_queries(metric.pack_codes(qb[:10].copy()), metric.pack_labels(ql[:10].copy()))
        all_refused()
        raises(STATE, ctx.votes, (R,))                                       # the lists were the old queries'
        ctx.topr(R)
        ctx.votes((R,))
        assert np.array_equal(ctx.get_votes(), brute(qb[:10], db, ql[:10], dl, R, (R,))[0])
        ctx.set_database(metric.pack_codes(db[:200].copy()), metric.pack_labels(dl[:200].copy()), db.shape[1], dl.shape[1])
        ctx.set_queries(metric.pack_codes(qb[:10].copy()), metric.pack_labels(ql[:10].copy()))
        all_refused()
        # hg_trim
        ctx.topr(R)
        ctx.votes((R,))
        bytes1 = ctx.get_stat("device_bytes")
        ctx.trim()
        all_refused()
        assert ctx.get_stat("device_bytes") < bytes1
        raises(STATE, ctx.votes, (R,))
        ctx.topr(R)
        ctx.votes((R,))
        assert np.array_equal(ctx.get_votes(), brute(qb[:10], db[:200], ql[:10], dl[:200], R, (R,))[0])
    finally:
        ctx.close()
    # a shard: votes over partial lists mean nothing
    ctx = code_ctx(qb, db[:1000], ql, dl[:1000], idx_base=100, n_total=1100)
    try:
        msg = raises(STATE, ctx.votes, (1, 5))
        assert "whole database" in msg
    finally:
        ctx.close()
    # 256 classes
    rng = np.random.default_rng(256)
    dl256, ql256 = (rng.random((300, 256)) < 0.1).astype(np.int8), (rng.random((5, 256)) < 0.1).astype(np.int8)
    ctx = code_ctx(qb[:5], db[:300], ql256, dl256)
    try:
        ctx.topr(10)
        raises(ARG, ctx.votes, (1, 10))
    finally:
        ctx.close()


def test_every_buffer_is_on_the_contexts_list():
    """device_bytes after a trim is the tables alone, whatever hg_votes had reserved."""
    c = case1()
    ctx = code_ctx(c["qb"], c["db"], c["ql"], c["dl"])
    try:
        ctx.trim()
        bytes0 = ctx.get_stat("device_bytes")
        ctx.topr(100)
        ranked = ctx.get_stat("device_bytes")
        ctx.votes((1, 100))
        assert ctx.get_stat("device_bytes") > ranked
        ctx.trim()
        assert ctx.get_stat("device_bytes") == bytes0
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. step state untouched
def test_leaves_the_map_path_alone(case_cache):
    """hg_map's APs before and after a votes call are the same bits, and a FIRST votes call (its buffers are new) between two
    hg_map_begin steps leaves the licence to enqueue blind (tests/test_side_results_gpu.py's sequence and stat)."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R = c["R"]
    ctx = _native.Context(0)

    def staged():
        ctx.hist()
        ctx.plan(R)
        ctx.select()

    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        staged()                                                             # (sizes the list buffers once)
        ap0, rel0 = ctx.map(R)
        assert np.array_equal(ap0, g["ap"], equal_nan=True)
        assert ctx.get_stat("last_optimistic") == 1
        staged()
        n0 = ctx.get_stat("map_async_steps")
        ctx.votes((100, R))
        ctx.map_begin(R)
        assert ctx.get_stat("map_async_steps") == n0 + 1, "hg_votes' first reservations ended the licence to enqueue blind"
        ap1, rel1 = ctx.map_end()
        assert ap1.tobytes() == ap0.tobytes() and np.array_equal(rel1, rel0)
        assert ctx.get_stat("map_async_redone") == 0
        # the votes of those lists: the query's own class against the hits hg_map counted
        ctx.topr(R)
        ctx.votes((100, R))
        own = ctx.get_votes()[np.arange(len(c["qlab"])), 1, c["qlab"].argmax(1)]
        assert np.array_equal(own.astype(np.int64), rel0)
        ap2, rel2 = ctx.map(R)
        assert ap2.tobytes() == ap0.tobytes() and np.array_equal(rel2, rel0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. the Python surface
def assert_same_dict(out, ref):
    assert sorted(out) == sorted(ref)
    for k in ref:
        assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k], equal_nan=ref[k].dtype.kind == "f"), k


@pytest.mark.parametrize("spelling", ["bits", "pm1"])
def test_python_surface_codes(spelling):
    c = case1()
    qb, db, ql, dl = c["qb"], c["db"], c["ql"], c["dl"]
    q_in, d_in = (qb, db) if spelling == "bits" else (2 * qb.astype(np.int8) - 1, 2 * db.astype(np.int8) - 1)
    ref = X.knn_from_tables(c["ref"][1], c["ref"][3], ql, KS1)
    assert 0.0 < ref["accuracy"][-1] < 1.0 and ref["confusion"].sum() > 0
    assert_same_dict(X.knn_vote_at_k(q_in, d_in, ql, dl, KS1), ref)


def test_python_surface_maps():
    c = case1()
    ref = X.knn_from_tables(c["ref"][1], c["ref"][3], c["ql"], KS1)
    pm1 = lambda x: (2.0 * x.astype(np.float32) - 1.0)                      # (+-1 codes: MAPs ranks them by Hamming distance)
    database = types.SimpleNamespace(output=pm1(c["db"]), label=c["dl"].astype(np.int64))
    query = types.SimpleNamespace(output=pm1(c["qb"]), label=c["ql"].astype(np.int64))
    m = MAPs(5)                                                             # (self.R is not used)
    try:
        assert_same_dict(m.get_knn_at(database, query, KS1), ref)
        assert_same_dict(m.get_knn_at(None, query, KS1[:3]), X.knn_from_tables(c["ref"][1][:, :3], c["ref"][3][:3], c["ql"], KS1[:3]))
        assert m.get_maps_by_feature(None, query) >= 0.0                     # the object goes on as before
    finally:
        m.close()


@pytest.mark.parametrize("rerank", [False, True])
def test_python_surface_features(rerank):
    c = real_case()
    tab = real_case_tables(rerank)[0]
    ref = X.knn_from_tables(tab[1], tab[3], c["ql"], KS3)
    out = X.knn_vote_at_k(c["qf"], c["dbf"], c["ql"], c["dl"], KS3, features=not rerank, rerank=rerank)
    assert_same_dict(out, ref)
    database = types.SimpleNamespace(output=c["dbf"], label=c["dl"])
    query = types.SimpleNamespace(output=c["qf"], label=c["ql"])
    m = MAPs(5, rerank=rerank)
    try:
        assert_same_dict(m.get_knn_at(database, query, KS3), ref)
    finally:
        m.close()

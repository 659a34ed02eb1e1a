"""hg_rel_hist: per query and Hamming distance, the rows at that distance and those of them that share a label with the query --
against brute-force NumPy, exactly, under both settings of the option hist_mfma (the pass has one kernel so far, k_hist_rel on the
vector ALU, so stat rel_hist_variant must say 1 under either); and the lookup metrics of hashgan_amd.extra_metrics that read the tables."""
import functools

import numpy as np
import pytest
from tests import brute_refs, cases
from hashgan_amd import _native, metric

pytestmark = pytest.mark.gpu


def expected_variant(b, C, hist_mfma):
    """DESIGN.md, "The relevant-row histogram": no matrix-core form is built, the vector-ALU kernel takes every shape."""
    return 1


brute = brute_refs.rel_hist                            # (shared with tests/test_second_hand_gpu.py)


def gpu_pass(qb, db, ql, dl, hist_mfma, opts=(), idx_base=0, n_total=None):
    """A private context: -> (all, rel, hg_hist's histogram, rel_hist_variant, segments)."""
    ctx = _native.Context(0)
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        ctx.set_option("hist_mfma", hist_mfma)
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1], idx_base, n_total)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        ctx.rel_hist()
        a, r = ctx.get_rel_hist()
        variant = ctx.get_stat("rel_hist_variant")
        ctx.hist()
        return a, r, ctx.get_hist(), variant, ctx.get_stat("segments")
    finally:
        ctx.close()


def check(qb, db, ql, dl, opts=(), ref=None):
    """Both settings of hist_mfma equal the brute force (hence each other), `all` equals hg_hist's histogram, the stat names the kernel."""
    ref_all, ref_rel = ref if ref is not None else brute(qb, db, ql, dl)
    b, C = db.shape[1], dl.shape[1]
    got = {}
    for hm in (0, 2):
        a, r, h, variant, S = gpu_pass(qb, db, ql, dl, hm, opts)
        assert a.dtype == np.uint32 and a.shape == (b + 1, len(qb)) and r.shape == a.shape
        assert np.array_equal(a, ref_all), (hm, "all")
        assert np.array_equal(r, ref_rel), (hm, "rel")
        assert np.array_equal(a, h), (hm, "hg_hist")
        assert variant == expected_variant(b, C, hm), (hm, variant)
        got[hm] = (a, r, S)
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
    return got[2][2]


@functools.lru_cache(maxsize=None)
def case1():
    """Multi-hot labels (a pair may share several: the match is 0/1 all the same), near queries, N % 16 != 0, Q % 32 != 0."""
    rng = np.random.default_rng(4)
    Q, N, b, C = 60, 5000, 16, 6
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.08).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.3).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.3).astype(np.int8)
    ql[0] = 0                                          # a query without labels
    dl[::7] = 0                                        # rows without labels
    ql[1] = 1                                          # shares up to C labels with a row
    for a in (qb, db, ql, dl):
        a.flags.writeable = False
    return qb, db, ql, dl, brute(qb, db, ql, dl)


def test_multi_hot_labels():
    qb, db, ql, dl, ref = case1()
    assert ((ql.astype(np.int64) @ dl.astype(np.int64).T) > 1).any()
    assert ref[0][:3].sum() > 0                        # the low-distance bins are populated
    check(qb, db, ql, dl, ref=ref)


def test_tiles_and_segments():
    """An odd number of segments with a ragged last one (a last batch of fewer rows than a scalar-load batch), a query tile that
    straddles 64."""
    rng = np.random.default_rng(5)
    Q, N, b, C = 70, 1001, 64, 10
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl = np.eye(C, dtype=np.int8)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int8)[rng.integers(0, C, Q)]
    S = check(qb, db, ql, dl, opts=(("min_segment", 64), ("target_units", 22)))
    # (segments are a multiple of 32 rows long and N is not: the last one is ragged, whatever their number)
    assert S >= 3 and S % 2 == 1 and N % 32 != 0, S


@pytest.mark.parametrize("b", [40, 72, 128, 255])
def test_code_widths(b):
    """Bits beyond the code contribute nothing; bin b is populated (exact complements); 255 bits: the vector-ALU form whatever
    hist_mfma says (expected_variant)."""
    rng = np.random.default_rng(b)
    Q, N, C = 5, 300, 4
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    db[17] = 1 - qb[0]
    db[299] = 1 - qb[4]
    dl = (rng.random((N, C)) < 0.4).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.4).astype(np.int8)
    ql[0] = dl[17] = [0, 0, 0, 1]
    ref = brute(qb, db, ql, dl)
    assert ref[0][b, 0] >= 1 and ref[1][b, 0] >= 1 and ref[0][b, 4] >= 1
    assert expected_variant(255, C, 2) == 1
    check(qb, db, ql, dl, ref=ref)


@pytest.mark.parametrize("C", [32, 33, 64, 65, 128, 130])
def test_label_widths(C):
    """The last label word (rows and queries that carry only their highest class); 130 classes: the loop over more than two label
    words."""
    rng = np.random.default_rng(C)
    Q, N, b = 33, 500, 32
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.02).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.05).astype(np.int8)
    dl[::5] = 0
    dl[::5, C - 1] = 1                                 # only the highest class
    ql[:4] = 0
    ql[:4, C - 1] = 1
    ql[4] = 0
    ql[4, 0] = 1
    ref = brute(qb, db, ql, dl)
    assert ref[1][:, 0].sum() >= N // 5
    check(qb, db, ql, dl, ref=ref)


def test_counter_width():
    """One counter reaches 140000 -- first the relevant one, then (labels disjoint from query 0's) the other: a 16-bit shared column
    or a narrow partial would wrap.  Two long segments, so that a segment pair holds more than 65535 rows."""
    Q, N, b, C = 3, 140000, 32, 2
    rng = np.random.default_rng(6)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    qb[1] = 1 - qb[0]
    db = np.repeat(qb[:1], N, axis=0)
    ql = np.array([[1, 0], [0, 1], [1, 1]], np.int8)
    for lab in ([1, 0], [0, 1]):
        dl = np.repeat(np.array([lab], np.int8), N, axis=0)
        ref_all = np.zeros((b + 1, Q), np.int64)
        ref_rel = np.zeros((b + 1, Q), np.int64)
        d = (qb != qb[0]).sum(1)
        ref_all[d, np.arange(Q)] = N
        ref_rel[d, np.arange(Q)] = N * ((ql @ np.array(lab)) > 0)
        assert ref_rel[0, 0] == (N if lab == [1, 0] else 0)
        S = check(qb, db, ql, dl, opts=(("max_segments", 2),), ref=(ref_all, ref_rel))
        assert S == 2


def test_additive_over_shards():
    """Two contexts on the two halves of the database (idx_base / n_total as for shards): the tables add up to the whole's."""
    qb, db, ql, dl, ref = case1()
    N = len(db)
    cut = 2437
    for hm in (0, 2):
        a0, r0, *_ = gpu_pass(qb, db[:cut], ql, dl[:cut], hm, idx_base=0, n_total=N)
        a1, r1, *_ = gpu_pass(qb, db[cut:], ql, dl[cut:], hm, idx_base=cut, n_total=N)
        assert np.array_equal(a0.astype(np.int64) + a1, ref[0]) and np.array_equal(r0.astype(np.int64) + r1, ref[1])


def test_state_errors_and_reload():
    qb, db, ql, dl, ref = case1()
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1])
        with pytest.raises(_native.HashganNativeError) as e:
            ctx.rel_hist()                             # no queries yet
        assert e.value.code == _native.HG_ERR_STATE
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        with pytest.raises(_native.HashganNativeError) as e:
            ctx.get_rel_hist()                         # no pass yet
        assert e.value.code == _native.HG_ERR_STATE
        ctx.rel_hist()
        a, r = ctx.get_rel_hist()
        assert np.array_equal(a, ref[0]) and np.array_equal(r, ref[1])
        # other queries, another count: the old tables are gone, the new ones are the new queries'
        sel = slice(40, 3, -2)
        ctx.set_queries(metric.pack_codes(qb[sel].copy()), metric.pack_labels(ql[sel].copy()))
        with pytest.raises(_native.HashganNativeError) as e:
            ctx.get_rel_hist()
        assert e.value.code == _native.HG_ERR_STATE
        ctx.rel_hist()
        a, r = ctx.get_rel_hist()
        assert np.array_equal(a, ref[0][:, sel]) and np.array_equal(r, ref[1][:, sel])
        # a database reload invalidates them as well
        ctx.set_database(metric.pack_codes(db[:100].copy()), metric.pack_labels(dl[:100].copy()), db.shape[1], dl.shape[1])
        ctx.set_queries(metric.pack_codes(qb[sel].copy()), metric.pack_labels(ql[sel].copy()))
        with pytest.raises(_native.HashganNativeError) as e:
            ctx.get_rel_hist()
        assert e.value.code == _native.HG_ERR_STATE
        # hg_trim frees the tables
        ctx.rel_hist()
        ctx.trim()
        with pytest.raises(_native.HashganNativeError) as e:
            ctx.get_rel_hist()
        assert e.value.code == _native.HG_ERR_STATE
    finally:
        ctx.close()


def test_pass_leaves_the_map_path_alone(case_cache):
    """hg_map before and after an interleaved hg_rel_hist, and hg_map_begin -> hg_rel_hist -> hg_map_end: the golden AP each time;
    a staged hg_hist -> hg_rel_hist -> hg_plan sequence goes on as if the pass had not happened."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R = c["R"]
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        ap, rel = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.rel_hist()
        a0, r0 = ctx.get_rel_hist()
        assert (a0.astype(np.int64).sum(0) == c["dbbits"].shape[0]).all() and (r0 <= a0).all()
        ap, rel = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.map_begin(R)
        ctx.rel_hist()
        ap, rel = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.map_begin(R)
        ctx.map_begin(R)
        ctx.rel_hist()
        for _ in range(2):
            ap, rel = ctx.map_end()
            assert np.array_equal(ap, g["ap"], equal_nan=True)
        a1, r1 = ctx.get_rel_hist()
        assert np.array_equal(a0, a1) and np.array_equal(r0, r1)
        # staged: the histogram and the plan's state are the staged sequence's own
        ctx.hist()
        ctx.rel_hist()
        assert np.array_equal(ctx.get_hist(), a0)
        ctx.plan(R)
        ctx.select()
        ctx.match()
        ctx.ap()
        ap, rel = ctx.get_ap()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("spelling", ["bits", "pm1"])
def test_python_surface(spelling):
    from hashgan_amd import extra_metrics as X
    qb, db, ql, dl, ref = case1()
    b = qb.shape[1]
    q_in, d_in = (qb, db) if spelling == "bits" else (2 * qb.astype(np.int8) - 1, 2 * db.astype(np.int8) - 1)
    all_h, rel_h = X.lookup_histograms(q_in, d_in, ql, dl)
    assert all_h.dtype == np.int64 and all_h.shape == (len(qb), b + 1)
    assert np.array_equal(all_h, ref[0].T) and np.array_equal(rel_h, ref[1].T)
    # the curves against the definition on the pairs
    D = (qb[:, None, :] != db[None, :, :]).sum(2)
    rel = (ql.astype(np.int64) @ dl.astype(np.int64).T) > 0
    tot = rel.sum(1)
    ok = tot > 0
    assert not ok.all() and ok.any()
    out = X.hamming_radius_curves(q_in, d_in, ql, dl)
    for r in range(b + 1):
        inside = D <= r
        ball, hit = inside.sum(1), (inside & rel).sum(1)
        assert np.array_equal(out["ball"][:, r], ball) and np.array_equal(out["hit"][:, r], hit)
        assert abs(out["precision"][r] - np.where(ball > 0, hit / np.maximum(ball, 1), 0.0).mean()) <= 1e-15
        assert abs(out["recall"][r] - (hit[ok] / tot[ok]).mean()) <= 1e-15
    assert np.array_equal(out["total_rel"], tot)
    # precision_within_radius reads the tables: the kernel timing table shows one k_hist_rel pass and no histogram, select, rank,
    # order or match kernel of the ranking path
    eng = metric._Shared.get(0)
    with eng.lock:
        before = {k: eng.ctx.get_stat(k) for k in ("optimistic_runs", "optimistic_fallbacks")}
        eng.ctx.timing_enable(2)
        eng.ctx.timing_reset()
        try:
            got, balls = X.precision_within_radius(q_in, d_in, ql, dl, radius=4)
            launches = {k: n for k, (ms, n) in eng.ctx.timing_read().items() if n}
        finally:
            eng.ctx.timing_enable(False)
        assert launches.get("k_hist_rel") == 1 and launches.get("k_hist_rel_reduce") == 1, launches
        assert not set(launches) - {"k_hist_rel", "k_hist_rel_reduce", "k_pack"}, launches
        inside = D <= 4
        ball = inside.sum(1)
        assert np.array_equal(balls, ball)
        assert abs(got - np.where(ball > 0, (inside & rel).sum(1) / np.maximum(ball, 1), 0.0).mean()) < 1e-15
        assert eng.ctx.get_stat("optimistic_runs") == before["optimistic_runs"]
        assert eng.ctx.get_stat("optimistic_fallbacks") == before["optimistic_fallbacks"]
        assert eng.ctx.get_stat("rel_hist_variant") != 0

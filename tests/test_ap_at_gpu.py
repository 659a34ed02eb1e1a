"""hg_ap_at (k_ap_at): AP@R and the hits among the top R at many cut-offs from one ranking, against the CPU oracle (which tests/golden
pins to the reference).  Every comparison is bitwise -- np.array_equal(..., equal_nan=True) -- there is no tolerance anywhere.

Codes: imatch from oracle.hamming_map.map_from_codes at R_max, then average_precision(imatch[q, :R_j], R_j) per cut-off (None -> NaN).
Features: oracle.real_map.map_from_features per R_j.  Shapes are the smallest that reach every branch of the kernel: leaf lengths
below, at and above 8, 128 and 129, a full chunk ending exactly at a cut-off, cut-offs in the first, second and third chunk, 64
cut-offs in one chunk, a list beyond 2^20 (no reciprocal table, the 512-thread geometry)."""
import functools
import types

import numpy as np
import pytest
from oracle import hamming_map as O
from oracle import real_map
from tests import brute_refs
from hashgan_amd import DeviceArray, MAPs, _native, metric
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG
RS_TREE = [1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 8191, 8192, 8193, 8200, 16384, 16385, 16513]
N1, R1 = 17000, 16513


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def one_hot(rng, n, C):
    return np.eye(C, dtype=np.int64)[rng.integers(0, C, n)]


oracle_at = brute_refs.ap_at_oracle                       # (shared with tests/test_second_hand_gpu.py)


@functools.lru_cache(maxsize=None)
def case1():
    """Q = 12, N = 17000, b = 16, C = 4 one-hot: the tables of cases 1, 2, 6 and 8 and the oracle's match rows at R = 16513."""
    rng = np.random.default_rng(20)
    Q, b, C = 12, 16, 4
    db = rng.integers(0, 2, (N1, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl, ql = one_hot(rng, N1, C), one_hot(rng, Q, C)
    imatch = O.map_from_codes(qb, db, ql, dl, R1)[2]
    for a in (db, qb, dl, ql, imatch):
        a.flags.writeable = False
    return qb, db, ql, dl, imatch


def code_ctx(qb, db, ql, dl):
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1])
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
    return ctx


def gpu_at(qb, db, ql, dl, R, Rs, options=()):
    ctx = code_ctx(qb, db, ql, dl)
    try:
        for k, v in options:
            ctx.set_option(k, v)
        ctx.topr(R)
        ctx.ap_at(Rs)
        assert ctx.get_stat("ap_at_cutoffs") == len(Rs)
        return ctx.get_ap_at()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 1, 2: tree boundaries; 64 cut-offs in one chunk
@pytest.mark.parametrize("Rs", [RS_TREE, list(range(100, 6401, 100))], ids=["tree_boundaries", "64_in_one_chunk"])
def test_codes_equal_the_oracle(Rs):
    qb, db, ql, dl, imatch = case1()
    ap, rel = gpu_at(qb, db, ql, dl, R1, Rs)
    ap_ref, rel_ref = oracle_at(imatch, Rs)
    assert ap.dtype == np.float64 and rel.dtype == np.int64
    assert same(rel, rel_ref)
    assert same(ap, ap_ref)


# ------------------------------------------------------------------ 3: a single cut-off is hg_map at that R
@pytest.mark.parametrize("R", [1, 64, 65, 5000, N1])
def test_single_cutoff_equals_map(R):
    qb, db, ql, dl, imatch = case1()
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ap_map, rel_map = ctx.map(R)
        ctx.topr(R)                                                      # (R = N: the dense rank path's bitmap)
        ctx.ap_at([R])
        ap, rel = ctx.get_ap_at()
    finally:
        ctx.close()
    assert same(ap[:, 0], ap_map) and same(rel[:, 0], rel_map)
    if R <= R1:
        ap_ref, rel_ref = oracle_at(imatch, [R])
        assert same(ap, ap_ref) and same(rel, rel_ref)


# ------------------------------------------------------------------ 4: NaN, then a value
@functools.lru_cache(maxsize=None)
def late_case():
    """Queries 4 and 5 meet their first relevant row at rank ~300, queries 6 and 7 have none in the database."""
    rng = np.random.default_rng(21)
    Q, N, b, C = 8, 3000, 16, 6
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, 3, N)]                # classes 0..2 only
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, 3, Q)]
    idx = O.topr_from_codes(qb, db, 1000)[0]
    ql[4], ql[5] = np.eye(C, dtype=np.int64)[3], np.eye(C, dtype=np.int64)[4]
    dl[idx[4, 299:340]] = np.eye(C, dtype=np.int64)[3]                   # first hit of query 4 at rank 300
    late5 = np.setdiff1d(idx[5, 319:400], idx[4, 299:340])
    dl[late5] = np.eye(C, dtype=np.int64)[4]
    ql[6] = ql[7] = np.eye(C, dtype=np.int64)[5]                         # a class no database row has
    return qb, db, ql, dl


def test_nan_then_a_value():
    qb, db, ql, dl = late_case()
    Rs = [10, 100, 1000]
    imatch = O.map_from_codes(qb, db, ql, dl, Rs[-1])[2]
    ap_ref, rel_ref = oracle_at(imatch, Rs)
    assert np.isnan(ap_ref[4:6, :2]).all() and not np.isnan(ap_ref[4:6, 2]).any() and np.isnan(ap_ref[6:]).all()
    assert not np.isnan(ap_ref[:4]).any()
    ap, rel = gpu_at(qb, db, ql, dl, Rs[-1], Rs)
    assert same(np.isnan(ap), np.isnan(ap_ref)) and same(rel == 0, rel_ref == 0)
    assert same(ap, ap_ref) and same(rel, rel_ref)
    out = X.map_at_k(qb, db, ql, dl, Rs)
    want = np.array([metric.mean_over_hits(np.ascontiguousarray(ap_ref[:, j]), np.ascontiguousarray(rel_ref[:, j])) for j in range(3)])
    assert same(out["map"], want)
    assert same(out["per_query"]["ap"], ap_ref) and same(out["per_query"]["hits"], rel_ref)
    total = ((ql @ dl.T) > 0).sum(1)
    assert same(out["per_query"]["total_rel"], total) and (total[6:] == 0).all()
    ok = total > 0
    assert same(out["precision"], (rel_ref / np.array(Rs)[None, :]).mean(0))
    assert same(out["recall"], (rel_ref[ok] / total[ok, None]).mean(0))


# ------------------------------------------------------------------ 5: dense and sparse rows
@pytest.mark.parametrize("C", [1, 50], ids=["every_bit_set", "one_bit_in_fifty"])
def test_dense_and_sparse_rows(C):
    qb, db = case1()[:2]
    rng = np.random.default_rng(22)
    dl, ql = one_hot(rng, N1, C), one_hot(rng, len(qb), C)
    Rs = [129, 4097, 9000]
    imatch = O.map_from_codes(qb, db, ql, dl, Rs[-1])[2]
    assert imatch.all() if C == 1 else 0.01 < imatch.mean() < 0.03
    ap, rel = gpu_at(qb, db, ql, dl, Rs[-1], Rs)
    ap_ref, rel_ref = oracle_at(imatch, Rs)
    assert same(ap, ap_ref) and same(rel, rel_ref)


# ------------------------------------------------------------------ 6: the division path
def test_division_equals_the_reciprocal_table():
    qb, db, ql, dl, imatch = case1()
    a1, r1 = gpu_at(qb, db, ql, dl, R1, RS_TREE, options=(("ap_recip", 1),))
    a0, r0 = gpu_at(qb, db, ql, dl, R1, RS_TREE, options=(("ap_recip", 0),))
    ap_ref, rel_ref = oracle_at(imatch, RS_TREE)
    assert same(a0, a1) and same(r0, r1)
    assert same(a0, ap_ref) and same(r0, rel_ref)


def test_one_long_list_without_a_reciprocal_table():
    rng = np.random.default_rng(23)
    Q, N, b, C = 2, (1 << 20) + 8200, 16, 4
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    dl, ql = one_hot(rng, N, C), one_hot(rng, Q, C)
    Rs = [1 << 20, (1 << 20) + 1, N]
    imatch = O.map_from_codes(qb, db, ql, dl, N)[2]
    ap_ref, rel_ref = oracle_at(imatch, Rs)
    ap, rel = gpu_at(qb, db, ql, dl, N, Rs)
    assert same(rel, rel_ref)
    assert same(ap, ap_ref)


# ------------------------------------------------------------------ 7: real-valued features
@functools.lru_cache(maxsize=None)
def real_case():
    Q, N, b, C = 8, 3000, 16, 5
    rng = np.random.default_rng(24)
    dbf, qf = real_map.quantised_features(241, N, b), real_map.quantised_features(242, Q, b)
    dl, ql = one_hot(rng, N, C), one_hot(rng, Q, C)
    return qf, dbf, ql, dl


def test_features_equal_the_oracle():
    qf, dbf, ql, dl = real_case()
    Rs = [1, 129, 2048, 2500]
    ap_ref = np.stack([real_map.map_from_features(qf, dbf, ql, dl, R)[1] for R in Rs], axis=1)
    ctx = _native.Context(0)
    try:
        ctx.set_option("keep_floats", 1)
        ctx.set_database_f32(dbf, dl)
        ctx.set_queries_f32(qf, ql)
        ctx.topr_real(2500, download=False)
        ctx.ap_at(Rs)
        ap, rel = ctx.get_ap_at()
        for j, R in enumerate(Rs):                                       # secondary: this build's one-R call
            a, r = ctx.map_real(R)
            assert same(ap[:, j], a) and same(rel[:, j], r)
    finally:
        ctx.close()
    assert same(ap, ap_ref)
    assert same(rel == 0, np.isnan(ap_ref))
    side = types.SimpleNamespace
    got = MAPs(1).get_maps_at(side(output=dbf, label=dl), side(output=qf, label=ql), Rs)
    want = np.array([MAPs(R).get_maps_by_feature(side(output=dbf, label=dl), side(output=qf, label=ql)) for R in Rs])
    assert got.dtype == np.float64 and same(got, want)
    out = X.map_at_k(qf, dbf, ql, dl, Rs, features=True)
    assert same(out["per_query"]["ap"], ap_ref) and same(out["map"], want)


def test_get_maps_at_routes_pm1_codes_to_the_hamming_kernels():
    qb, db, ql, dl, imatch = case1()
    Rs = [9, 129, 8200]
    ap_ref, rel_ref = oracle_at(imatch, Rs)
    side = types.SimpleNamespace
    pm = lambda x: (2.0 * x - 1.0).astype(np.float32)
    got = MAPs(1).get_maps_at(side(output=pm(db), label=dl), side(output=pm(qb), label=ql), Rs)
    want = np.array([metric.mean_over_hits(np.ascontiguousarray(ap_ref[:, j]), np.ascontiguousarray(rel_ref[:, j])) for j in range(len(Rs))])
    assert same(got, want)


# ------------------------------------------------------------------ 8: one launch
def launches(ctx):
    return {k: n for k, (ms, n) in ctx.timing_read().items() if n}


def test_one_launch_for_all_cutoffs():
    qb, db, ql, dl, _ = case1()
    ctx = code_ctx(qb, db, ql, dl)
    try:
        ctx.topr(R1)
        ctx.timing_enable(2)
        ctx.timing_reset()
        ctx.ap_at(RS_TREE)
        ctx.synchronize()
        seen = launches(ctx)
    finally:
        ctx.close()
    assert seen.get("k_ap_at") == 1 and "k_ap" not in seen, seen


# ------------------------------------------------------------------ 9: state rules
def test_state_and_arguments():
    qb, db, ql, dl, _ = case1()
    R = 300
    ctx = _native.Context(0)
    try:
        raises(STATE, ctx.get_ap_at)                                             # nothing loaded
        raises(STATE, ctx.ap_at, [1, 5])
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1])
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        raises(STATE, ctx.get_ap_at)                                             # no pass yet
        raises(STATE, ctx.ap_at, [1, 5])                                         # no ranking yet
        assert ctx.get_stat("ap_at_cutoffs") == 0
        ctx.trim()
        bytes0 = ctx.get_stat("device_bytes")                                    # the tables alone
        ctx.topr(R)
        ctx.ap()
        before = (ctx.get_ap(), ctx.get_match(), ctx.get_topr())
        for bad in ([1, R + 1], [], list(range(1, 66)), [5, 1], [5, 5], [0, 5]):
            raises(ARG, ctx.ap_at, bad)
        raises(STATE, ctx.get_ap_at)                                             # a refused call leaves no results
        ctx.ap_at([1, 5, R])
        first = ctx.get_ap_at()
        assert same(first[0][:, 2], before[0][0]) and same(first[1][:, 2], before[0][1])
        after = (ctx.get_ap(), ctx.get_match(), ctx.get_topr())                  # the ranking's own results are untouched
        for x, y in zip(before, after):
            assert same(x[0], y[0]) and same(x[1], y[1]) if isinstance(x, tuple) else same(x, y)
        assert same(ctx.get_ap_at()[0], first[0])                                # (and can be read again)
        ctx.topr(R)                                                              # a later ranking ends them
        raises(STATE, ctx.get_ap_at)
        ctx.ap_at([1, 5, R])
        assert same(ctx.get_ap_at()[0], first[0])
        ctx.map(R)                                                               # ... so does a one-shot call
        raises(STATE, ctx.get_ap_at)
        ctx.ap_at([1, 5, R])                                                     # hg_map leaves the whole bitmap too
        assert same(ctx.get_ap_at()[0], first[0])
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        raises(STATE, ctx.get_ap_at)
        raises(STATE, ctx.ap_at, [1, 5])                                         # the new queries are not ranked yet
        ctx.topr(R)
        ctx.ap_at([1, 5, R])
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1])
        raises(STATE, ctx.get_ap_at)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        raises(STATE, ctx.get_ap_at)
        ctx.topr(R)
        ctx.ap_at([1, 5, R])
        assert ctx.get_stat("device_bytes") > bytes0
        ctx.trim()
        raises(STATE, ctx.get_ap_at)
        assert ctx.get_stat("device_bytes") == bytes0                            # the feature's buffers are on the context's list
        ctx.topr(R)
        ctx.ap_at([1, 5, R])
        assert same(ctx.get_ap_at()[0], first[0]) and same(ctx.get_ap_at()[1], first[1])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 10: device arrays; precision_recall_at_k
class Producer:
    """Device memory without a framework: scratch slots of private contexts, filled with memcpy_htod."""

    def __init__(self):
        self.ctxs, self.n = [], 0

    def put(self, host):
        host = np.ascontiguousarray(host)
        if self.n % 4 == 0:
            self.ctxs.append(_native.Context())
        c = self.ctxs[-1]
        ptr = c.scratch(self.n % 4, host.nbytes)
        self.n += 1
        c.memcpy_htod(ptr, host, host.nbytes)
        return ptr

    def close(self):
        for c in self.ctxs:
            c.close()


def test_map_at_k_takes_device_arrays():
    qf, dbf, ql, dl = real_case()
    Rs = [1, 129, 2048, 2500]
    host = X.map_at_k(qf, dbf, ql, dl, Rs, features=True)
    prod = Producer()
    try:
        wide = np.zeros((len(dbf), dbf.shape[1] + 3), np.float32)
        wide[:, 2:2 + dbf.shape[1]] = dbf
        d_db = DeviceArray(prod.put(wide) + 8, dbf.shape, (wide.shape[1], 1), "float32")       # a strided view with a misaligned base
        d_dl = DeviceArray(prod.put(dl.astype(np.bool_)), dl.shape, None, "bool")
        d_q = DeviceArray(prod.put(qf), qf.shape, None, "float32")
        d_ql = DeviceArray(prod.put(ql.astype(np.bool_)), ql.shape, None, "bool")
        dev = X.map_at_k(d_q, d_db, d_ql, d_dl, Rs, features=True)
        mixed = X.map_at_k(qf, d_db, ql, d_dl, Rs, features=True)                # database on the device, queries on the host
        # binary codes from device memory
        qb, db, cl, _, imatch = case1()
        c_db = DeviceArray(prod.put(db.astype(np.float32)), db.shape, None, "float32")
        c_dl = DeviceArray(prod.put(case1()[3].astype(np.int32)), case1()[3].shape, None, "int32")
        codes = X.map_at_k(qb, c_db, cl, c_dl, [9, 129, 8200])
    finally:
        prod.close()
    for got in (dev, mixed):
        for k in ("map", "precision", "recall"):
            assert same(got[k], host[k]), k
        for k in ("ap", "hits", "total_rel"):
            assert same(got["per_query"][k], host["per_query"][k]), k
    ap_ref, rel_ref = oracle_at(imatch, [9, 129, 8200])
    assert same(codes["per_query"]["ap"], ap_ref) and same(codes["per_query"]["hits"], rel_ref)


def test_map_at_k_takes_torch_tensors():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    qf, dbf, ql, dl = real_case()
    Rs = [1, 129, 2048, 2500]
    host = X.map_at_k(qf, dbf, ql, dl, Rs, features=True)
    dev = torch.device("cuda")
    wide = torch.zeros(len(dbf), dbf.shape[1] + 3)
    wide[:, 2:2 + dbf.shape[1]] = torch.from_numpy(dbf)
    view = wide.to(dev)[:, 2:2 + dbf.shape[1]]
    assert not view.is_contiguous()
    got = X.map_at_k(torch.from_numpy(qf).to(dev), view, torch.from_numpy(ql).to(dev).bool(), torch.from_numpy(dl).to(dev).bool(), Rs,
                     features=True)
    for k in ("map", "precision", "recall"):
        assert same(got[k], host[k]), k
    for k in ("ap", "hits", "total_rel"):
        assert same(got["per_query"][k], host["per_query"][k]), k


def test_precision_recall_at_k_unsorted_repeated_and_more_than_64():
    """tests/test_extra_metrics.py's recipe with ks the new pass has to deduplicate, sort and split into batches of 64."""
    rng = np.random.default_rng(4)
    Q, N, b, C = 60, 5000, 16, 6
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.08).astype(np.uint8)
    dl = (rng.random((N, C)) < 0.3).astype(np.int8)
    ql = (rng.random((Q, C)) < 0.3).astype(np.int8)
    ql[0] = 0                                                    # a query without labels
    D = O.hamming_matrix(O.pack_bits(qb), O.pack_bits(db))
    rel = (ql.astype(np.int64) @ dl.astype(np.int64).T) > 0
    ks_in = [1000, 10, 10, 100] + list(range(1, 71))
    ks = sorted(ks_in)                                           # results come in ascending order of k, repeats kept
    order = np.argsort(D, axis=1, kind="stable")
    relo = np.take_along_axis(rel, order, 1)
    p_ref = np.array([relo[:, :k].sum(1) / k for k in ks]).T.mean(0)
    tot = rel.sum(1)
    ok = tot > 0
    # (recall: the recipe's transposed table is summed along its contiguous axis, the function's row by row -- the guard's 1e-15 is
    # that difference in the ORDER of one float64 sum; the brute-force hits in the function's layout give its very bits)
    hits = np.stack([relo[:, :k].sum(1) for k in ks], axis=1)
    r_ref = (hits[ok] / tot[ok, None]).mean(0)
    p, r = X.precision_recall_at_k(qb, db, ql, dl, ks_in)
    assert p.shape == r.shape == (len(ks_in),)
    assert same(p, p_ref) and same(r, r_ref)

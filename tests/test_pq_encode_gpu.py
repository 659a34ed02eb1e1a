"""The exact PQ encoder on the GPU (hg_pq_encode, hg_pq_encode_dev, hg_set_database_pq_f32, pq.encode_gpu, MAPs(quantised=True) on
.output + .codebooks and with quantise_queries=True).  The contract is arithmetic fixed to the bit (include/hashgan_amd.h), so every
comparison is == / array_equal: against the brute-force oracle of tests/pq_encode_oracle.py (codes and the errors' bits) and against
pq.encode (codes).  Device memory comes from producer contexts' scratch slots, as in tests/test_dev_input_gpu.py."""
import ctypes
import gc
import re
import types

import numpy as np
import pytest

from tests import pq_encode_oracle as O
from hashgan_amd import _native, metric, pq, MAPs, pool_stats, release_engines
from hashgan_amd.devarray import DeviceArray

pytestmark = pytest.mark.gpu

ARG, STATE = _native.HG_ERR_ARG, _native.HG_ERR_STATE
BIG, ODD = (5003, 8, 8, 256), (2001, 3, 11, 16)


def bits(err):
    return np.ascontiguousarray(err).view(np.uint64)


def refused(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def labels_for(N, C=7, seed=5):
    return (np.random.default_rng(seed).random((N, C)) < 0.25).astype(np.int64)


class Producer:
    """Device buffers out of producer contexts' scratch slots (four per context), filled with memcpy_htod."""

    def __init__(self):
        self.ctxs, self.n = [], 0

    def put(self, host):
        host = np.ascontiguousarray(host)
        if self.n % 4 == 0:
            self.ctxs.append(_native.Context())
        c = self.ctxs[-1]
        ptr = c.scratch(self.n % 4, max(host.nbytes, 1))
        self.n += 1
        c.memcpy_htod(ptr, host, host.nbytes)
        return ptr

    def array(self, a, dtype=None):
        a = np.ascontiguousarray(a)
        return DeviceArray(self.put(a), a.shape, None, dtype or str(a.dtype))

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture()
def prod():
    p = Producer()
    yield p
    p.close()


@pytest.fixture()
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ host features
@pytest.mark.parametrize("shape", O.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codes_and_errors_equal_the_oracle(ctx, shape):
    c = O.case(*shape)
    codes, err, bad = ctx.pq_encode(c.x, c.books, want_err=True)
    assert bad == 0
    assert np.array_equal(codes, c.codes)
    assert np.array_equal(bits(err), bits(c.err))
    assert np.array_equal(codes, pq.encode(c.x, c.books))
    again, err2, _ = ctx.pq_encode(c.x, c.books, want_err=True)               # a second call: the same bytes
    assert again.tobytes() == codes.tobytes() and err2.tobytes() == err.tobytes()
    only_codes, none, _ = ctx.pq_encode(c.x, c.books)
    assert none is None and np.array_equal(only_codes, codes)
    assert ctx.get_stat("pq_encode_calls") == 3 and ctx.get_stat("pq_encoded_rows") == 3 * c.N


@pytest.mark.parametrize("shape", [(200, 2, 16, 5), (200, 2, 17, 5), (130, 1, 255, 3), (70, 1, 253, 2)], ids=lambda s: "x".join(map(str, s)))
def test_path_boundaries(ctx, shape):
    """dsub = 16 is the register path's last, 17 the generic path's first (padded to 20 in LDS and in the float64 codewords); 255 fills
    64 KB of LDS; 253 pads three features."""
    c = O.case(*shape)
    codes, err, bad = ctx.pq_encode(c.x, c.books, want_err=True)
    assert bad == 0 and np.array_equal(codes, c.codes) and np.array_equal(bits(err), bits(c.err))
    assert np.array_equal(codes, pq.encode(c.x, c.books))
    x = c.x.copy()
    x[1, shape[2] - 1] = np.inf                                               # the last feature of subspace 0: next to the padding
    codes, err, bad = ctx.pq_encode(x, c.books, want_err=True)
    want = O.encode(x, c.books)
    assert bad == 1 and np.array_equal(codes, want[0]) and np.array_equal(bits(err), bits(want[1]))


@pytest.mark.parametrize("shape", [O.DUPLICATED, BIG], ids=lambda s: "x".join(map(str, s)))
def test_chunk_seams(ctx, shape):
    c = O.case(*shape)
    whole = ctx.pq_encode(c.x, c.books, want_err=True)
    ctx.set_option("pq_encode_chunk_rows", 1000)                              # seams at rows 1000, 2000, ..: inside wavefronts' row blocks
    chunked = ctx.pq_encode(c.x, c.books, want_err=True)
    assert chunked[0].tobytes() == whole[0].tobytes() == c.codes.tobytes()
    assert chunked[1].tobytes() == whole[1].tobytes() == c.err.tobytes()
    ctx.set_option("pq_encode_chunk_rows", 0)
    assert ctx.pq_encode(c.x, c.books)[0].tobytes() == c.codes.tobytes()


def test_exact_ties_a_fused_multiply_add_would_break(ctx):
    t = O.tie_case()
    assert t.fused_wrong >= 10
    for r in range(t.rows):
        codes, err, bad = ctx.pq_encode(t.x[r:r + 1], t.books[r], want_err=True)
        assert bad == 0 and not codes.any(), (r, np.flatnonzero(codes))       # the lower index on all 400 pairs
        assert np.array_equal(bits(err), bits(O.encode(t.x[r:r + 1], t.books[r])[1]))


def test_non_finite_rows(ctx):
    c = O.case(*ODD)
    x = c.x.copy()
    spots = {(3, 0): np.nan, (64, 12): np.inf, (1999, 32): -np.inf, (2000, 11): np.nan, (2000, 31): np.inf}
    for (r, k), v in spots.items():
        x[r, k] = v
    want, want_err = O.encode(x, c.books)
    codes, err, bad = ctx.pq_encode(x, c.books, want_err=True)
    assert bad == 4                                                           # rows, not entries
    for (r, k) in spots:
        assert codes[r, k // c.dsub] == 0
    assert np.array_equal(codes, want)                                        # the other subspaces and rows: as the oracle says
    clean = np.ones(c.N, bool); clean[[3, 64, 1999, 2000]] = False
    assert np.array_equal(codes[clean], c.codes[clean]) and np.array_equal(bits(err[clean]), bits(c.err[clean]))
    assert np.isnan(err[3]) and err[64] == np.inf and err[1999] == np.inf and np.isnan(err[2000])
    assert np.array_equal(np.isnan(err), np.isnan(want_err))
    with pytest.raises(ValueError, match="4 feature rows"):
        pq.encode_gpu(x, c.books)
    # the loader: HG_ERR_ARG, bad_rows reported, nothing loaded
    lab = labels_for(c.N)
    bc, bl, br = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = ctx._lib.hg_set_database_pq_f32(ctx._h, _native._ptr(x), _native._ptr(c.books), _native._ptr(lab), c.N, c.M, c.K, c.dsub, lab.shape[1],
                                         0, c.N, ctypes.byref(bc), ctypes.byref(bl), ctypes.byref(br))
    assert rc == ARG and br.value == 4 and b"hg_set_database_pq_f32" in ctx._lib.hg_last_error()
    assert "hg_set_database" in refused(STATE, ctx.set_queries_f32, c.x[:5], lab[:5])     # the context has no database
    with pytest.raises(ValueError, match="4 feature rows"):
        ctx.set_database_pq_f32(x, c.books, lab)
    ctx.set_database_pq_f32(c.x, c.books, lab)                                # ... and is usable
    assert ctx.N == c.N


# ------------------------------------------------------------------ device features
def layouts(prod, a, isz, name):
    rows, cols = a.shape
    yield "dense", DeviceArray(prod.put(a), a.shape, None, name)
    wide = np.zeros((rows, cols + 7), a.dtype)
    wide[:, :cols] = a
    yield "pitched", DeviceArray(prod.put(wide), a.shape, (cols + 7, 1), name)
    off = np.full((rows, cols + 1), 7, a.dtype)                               # x[:, 1:]: the base sits one element off
    off[:, 1:] = a
    yield "column slice", DeviceArray(prod.put(off) + isz, a.shape, (cols + 1, 1), name)
    yield "transposed", DeviceArray(prod.put(a.T), a.shape, (1, rows), name)
    both = np.full((rows * 2, cols * 3), 7, a.dtype)                          # every second row, every third column
    both[::2, ::3] = a
    yield "both strides", DeviceArray(prod.put(both), a.shape, (cols * 3 * 2, 3), name)


@pytest.mark.parametrize("shape", [ODD, (777, 5, 51, 256)], ids=lambda s: "x".join(map(str, s)))
def test_device_inputs_equal_the_widened_host_array(ctx, prod, shape):
    c = O.case(*shape)
    for what, f in layouts(prod, c.x, 4, "float32"):
        codes, err, bad = ctx.pq_encode(f, c.books, want_err=True)
        assert bad == 0 and np.array_equal(codes, c.codes) and np.array_equal(bits(err), bits(c.err)), what
    ctx.set_option("pq_encode_chunk_rows", 300)                               # device rows in chunks: the row offset goes through the stride
    for what, f in layouts(prod, c.x, 4, "float32"):
        codes, err, _ = ctx.pq_encode(f, c.books, want_err=True)
        assert np.array_equal(codes, c.codes) and np.array_equal(bits(err), bits(c.err)), what
    ctx.set_option("pq_encode_chunk_rows", 0)
    h = c.x.astype(np.float16)
    want = O.encode(h.astype(np.float32), c.books)
    assert np.array_equal(ctx.pq_encode(h.astype(np.float32), c.books)[0], want[0])
    for what, f in layouts(prod, h, 2, "float16"):
        codes, err, bad = ctx.pq_encode(f, c.books, want_err=True)
        assert bad == 0 and np.array_equal(codes, want[0]) and np.array_equal(bits(err), bits(want[1])), what
    bf, pattern = O.bf16_exact(c.x)
    want = O.encode(bf, c.books)
    for what, f in layouts(prod, pattern, 2, "bfloat16"):
        codes, err, bad = ctx.pq_encode(f, c.books, want_err=True)
        assert bad == 0 and np.array_equal(codes, want[0]) and np.array_equal(bits(err), bits(want[1])), what
    assert np.array_equal(pq.encode_gpu(prod.array(c.x), c.books), c.codes)
    nf = h.copy()
    nf[5, 3] = np.inf
    assert ctx.pq_encode(prod.array(nf), c.books)[2] == 1


def test_device_inputs_refused(ctx, prod):
    c = O.case(*ODD)
    dev = prod.array(c.x)

    def no(f, word):
        assert word in refused(ARG, ctx.pq_encode, f, c.books)
        assert np.array_equal(ctx.pq_encode(dev, c.books)[0], c.codes)        # the context stays usable

    no(DeviceArray(c.x.ctypes.data, c.x.shape), "pointer")                    # a NumPy array's host address
    no(types.SimpleNamespace(ptr=dev.ptr, shape=(c.N // 2, c.b), strides=(c.b, 1), dtype="float64", stream=None), "float64")
    no(DeviceArray(dev.ptr, (c.N // 2, c.b), None, "int64"), "int64")
    no(DeviceArray(dev.ptr, (c.N // 4, c.b), None, "uint8"), "uint8")
    no(DeviceArray(dev.ptr, (c.N, c.b - 1), (c.b, 1)), "columns")             # cols != M * dsub
    no(types.SimpleNamespace(ptr=dev.ptr, shape=(c.N, c.b), strides=(c.b, 0), dtype="float32", stream=None), "strides")
    # an extent that runs one element past its allocation.  Where the allocation ends is asked of the library, not assumed (the
    # allocator rounds and caches): a descriptor that certainly overruns it is refused with a message that says where it ends
    edge = _native.Context()
    nbytes = 1 << 20
    ptr = edge.scratch(0, nbytes)
    edge.memcpy_htod(ptr, np.zeros(nbytes // 4, np.float32), nbytes)
    msg = refused(ARG, ctx.pq_encode, DeviceArray(ptr, (64 * nbytes // (c.b * 4), c.b)), c.books)
    size = int(re.search(r"allocation ends (\d+) bytes from there", msg).group(1))
    assert nbytes <= size < 64 * nbytes and size % 4 == 0, msg
    rows = size // (c.b * 4)
    last = ptr + size - rows * c.b * 4                                        # [last, last + rows x b x 4) ends where the allocation ends
    codes, _, bad = ctx.pq_encode(DeviceArray(last, (rows, c.b)), c.books)    # accepted: ends exactly there
    assert bad == 0 and codes.shape == (rows, c.M)
    no(DeviceArray(last + 4, (rows, c.b)), "allocation")                      # one float further
    edge.close()


# ------------------------------------------------------------------ the loader
@pytest.mark.parametrize("shape", [BIG, ODD], ids=lambda s: "x".join(map(str, s)))
def test_loader_equals_set_database_pq_on_encoded_codes(shape):
    c = O.case(*shape)
    Q, R = 33, 700
    lab = labels_for(c.N)
    rng = np.random.default_rng(9)
    qf = np.tanh(rng.standard_normal((Q, c.b))).astype(np.float32)
    ql = labels_for(Q, seed=6)
    a, b = _native.Context(0), _native.Context(0)
    for k in (a, b):
        k.set_option("keep_query_floats", 1)
    ra = a.set_database_pq_f32(c.x, c.books, lab)
    rb = b.set_database_pq(pq.encode(c.x, c.books), c.books, lab)
    assert ra == rb
    assert a.get_stat("pq_encoded_rows") == c.N and a.get_stat("pq_encode_calls") == 1
    pa, pb = a.get_packed(0), b.get_packed(0)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert a.census(0) == b.census(0)
    for k in (a, b):
        assert k.set_queries_f32(qf, ql)[1] == 0
    ia, sa = a.topr_pq(R)
    ib, sb = b.topr_pq(R)
    assert np.array_equal(ia, ib) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    ma, mb = a.map_pq(R), b.map_pq(R)
    assert np.array_equal(bits(ma[0]), bits(mb[0])) and np.array_equal(ma[1], mb[1])
    a.close(); b.close()


def test_encoding_disturbs_nothing(ctx):
    c = O.case(*ODD)
    rng = np.random.default_rng(4)
    N, Q, b, R = 3000, 20, 32, 100
    db = np.sign(rng.standard_normal((N, b))).astype(np.float32)
    qf = np.sign(rng.standard_normal((Q, b))).astype(np.float32)
    dl, ql = labels_for(N), labels_for(Q, seed=8)
    ctx.set_database_f32(db, dl)
    ctx.set_queries_f32(qf, ql)
    ap0 = ctx.map(R)
    ctx.topr(R)
    ctx.match(); ctx.ap()
    lists0, apx0 = ctx.get_topr(), ctx.get_ap()
    probe = _native.Context(0)                       # what a trimmed context with these tables holds, measured on a twin
    probe.set_database_f32(db, dl); probe.set_queries_f32(qf, ql); probe.map(R); probe.topr(R); probe.match(); probe.ap(); probe.trim()
    bytes0 = probe.get_stat("device_bytes")
    probe.close()
    assert np.array_equal(ctx.pq_encode(c.x, c.books)[0], c.codes)
    assert ctx.get_stat("device_bytes") > bytes0                              # the work buffers are counted
    lists1, apx1 = ctx.get_topr(), ctx.get_ap()
    assert all(np.array_equal(x, y) for x, y in zip(lists0, lists1))
    assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(apx0, apx1))
    ctx.trim()
    assert ctx.get_stat("device_bytes") == bytes0                             # ... and freed by hg_trim
    ap1 = ctx.map(R)
    assert np.array_equal(bits(ap0[0]), bits(ap1[0])) and np.array_equal(ap0[1], ap1[1])


# ------------------------------------------------------------------ Python surface
def test_maps_on_features_and_codebooks(prod):
    c = O.case(*ODD)
    Q, R = 33, 700
    lab, ql = labels_for(c.N), labels_for(Q, seed=6)
    lab.flags.writeable = False
    qf = np.tanh(np.random.default_rng(9).standard_normal((Q, c.b))).astype(np.float32)
    q = types.SimpleNamespace(output=qf, label=ql)
    coded = types.SimpleNamespace(codes=pq.encode(c.x, c.books), codebooks=c.books, label=lab)
    m = MAPs(R, quantised=True)
    want = m.get_maps_by_feature(coded, q)
    host = types.SimpleNamespace(output=c.x, codebooks=c.books, label=lab)
    assert m.get_maps_by_feature(host, q) == want
    n_enc = m._engine().ctx.get_stat("pq_encode_calls")
    assert m.get_maps_by_feature(host, q) == want                             # the same immutable arrays as last time
    assert m._engine().ctx.get_stat("pq_encode_calls") == n_enc               # ... were not encoded again
    dev = types.SimpleNamespace(output=prod.array(c.x), codebooks=c.books, label=lab)
    assert m.get_maps_by_feature(dev, q) == want
    assert m.get_maps_by_feature(None, q) == want
    # SQD from features == the existing SQD call on pq.encode(query.output)
    sqd = m.get_maps_by_feature(coded, types.SimpleNamespace(codes=pq.encode(qf, c.books), label=ql))
    mq = MAPs(R, quantised=True, quantise_queries=True)
    assert mq.get_maps_by_feature(coded, q) == sqd
    assert mq.get_maps_by_feature(host, types.SimpleNamespace(output=prod.array(qf), label=ql)) == sqd
    bad = qf.copy(); bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="1 query rows"):
        mq.get_maps_by_feature(None, types.SimpleNamespace(output=bad, label=ql))
    with pytest.raises(ValueError, match="codes / .codebooks"):
        m.get_maps_by_feature(types.SimpleNamespace(output=c.x, label=lab), q)
    m.close(); mq.close()
    release_engines()


def test_twenty_new_objects_draw_one_pooled_context():
    c = O.case(*ODD)
    Q, R = 9, 300
    lab, ql = labels_for(c.N), labels_for(Q, seed=6)
    q = types.SimpleNamespace(output=c.x[:Q], label=ql)
    db = types.SimpleNamespace(output=c.x, codebooks=c.books, label=lab)
    release_engines()
    gc.collect()
    s0 = pool_stats()
    assert s0["contexts_idle"] == 0
    want = MAPs(R, quantised=True).get_maps_by_feature(db, q)                 # the object dies with the statement
    gc.collect()
    assert pool_stats()["contexts_idle"] == 1
    for i in range(20):
        assert MAPs(R, quantised=True, quantise_queries=i % 2 == 1).get_maps_by_feature(db, q) is not None
        assert np.array_equal(pq.encode_gpu(c.x[:100], c.books), c.codes[:100])
    assert MAPs(R, quantised=True).get_maps_by_feature(db, q) == want
    gc.collect()
    st = pool_stats()
    assert st["contexts_idle"] == 1 and st["contexts_created"] - s0["contexts_created"] == 1
    release_engines()


# ------------------------------------------------------------------ refusals
def test_refusals_name_the_offender_and_leave_the_context_usable(ctx, prod):
    c = O.case(*ODD)
    lib, h, P = ctx._lib, ctx._h, _native._ptr
    codes = np.empty((c.N, c.M), np.uint8)
    bad = ctypes.c_int64()
    lab = labels_for(c.N)
    dev = _native._dev_struct(prod.array(c.x))

    def host(x=c.x, N=c.N, books=c.books, M=c.M, K=c.K, dsub=c.dsub, out=codes, br=bad):
        return lib.hg_pq_encode(h, P(x), N, P(books), M, K, dsub, P(out), None, ctypes.byref(br) if br is not None else None)

    def device(f=dev, books=c.books, M=c.M, K=c.K, dsub=c.dsub):
        return lib.hg_pq_encode_dev(h, ctypes.byref(f) if f is not None else None, P(books), M, K, dsub, P(codes), None, ctypes.byref(bad))

    def loader(x=c.x, books=c.books, labels=lab, N=c.N, M=c.M, K=c.K, dsub=c.dsub, C_=lab.shape[1], base=0, total=c.N):
        return lib.hg_set_database_pq_f32(h, P(x), P(books), P(labels), N, M, K, dsub, C_, base, total, None, None, ctypes.byref(bad))

    nf = c.books.copy()
    nf[1, 5, 7] = np.nan
    calls = {"hg_pq_encode": host, "hg_pq_encode_dev": device, "hg_set_database_pq_f32": loader}
    for name, fn in calls.items():
        for kw, word in [(dict(M=0), "M=0"), (dict(K=0), "K=0"), (dict(K=257), "K=257"), (dict(dsub=0), "dsub=0"),
                         (dict(M=32, dsub=8), "M * dsub = 256"), (dict(books=nf), "[1][5][7]"), (dict(books=None), "null")]:
            assert fn(**kw) == ARG, (name, kw)
            msg = lib.hg_last_error().decode()
            assert name in msg and word in msg, msg
    for kw in (dict(x=None), dict(N=0), dict(out=None), dict(br=None)):
        assert host(**kw) == ARG and "hg_pq_encode" in lib.hg_last_error().decode()
    assert host(N=1 << 31) == ARG and "2^31" in lib.hg_last_error().decode()
    assert device(f=None) == ARG
    assert device(M=c.M - 1) == ARG and "columns" in lib.hg_last_error().decode()
    for kw, word in [(dict(x=None), "data"), (dict(labels=None), "data"), (dict(N=0), "N >= 1"), (dict(C_=0), "C=0"),
                     (dict(base=1), "one shard"), (dict(total=c.N + 1), "one shard"), (dict(N=1 << 31, total=1 << 31), "2^31")]:
        assert loader(**kw) == ARG and word in lib.hg_last_error().decode(), (kw, lib.hg_last_error())
    assert lib.hg_pq_encode(None, P(c.x), c.N, P(c.books), c.M, c.K, c.dsub, P(codes), None, ctypes.byref(bad)) == ARG
    assert ctx.get_stat("pq_encode_calls") == 0
    assert host() == 0 and np.array_equal(codes, c.codes)                     # the context is usable, on both forms
    assert device() == 0 and np.array_equal(codes, c.codes)

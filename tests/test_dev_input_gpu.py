"""Features and labels handed over in DEVICE memory (hg_set_database_dev / hg_set_queries_dev, devarray.DeviceArray): the fused pack
against NumPy, every layout and dtype against the contiguous float32 / int64 run, rankings against the host-array path bit for bit,
the Python surfaces, copy-in, stream ordering, and the refusals that must never reach a launch.

Device memory comes from private producer contexts (scratch + memcpy_htod): nothing here needs torch (the last test uses it where
present)."""
import ctypes
import re
import types
import warnings

import numpy as np
import pytest

from hashgan_amd import _native, metric
from hashgan_amd import MAP, MAP_per_query, MAPs
from hashgan_amd.devarray import DeviceArray
from oracle import hamming_map as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ device memory without a framework
class Producer:
    """Device buffers out of producer contexts' scratch slots (four per context), filled with memcpy_htod."""

    def __init__(self):
        self.ctxs, self.n = [], 0

    def alloc(self, nbytes):
        if self.n % 4 == 0:
            self.ctxs.append(_native.Context())
        c = self.ctxs[-1]
        ptr = c.scratch(self.n % 4, max(int(nbytes), 1))
        self.n += 1
        return c, ptr

    def put(self, host):
        """Raw bytes of `host` (made contiguous) -> (context, device address)."""
        host = np.ascontiguousarray(host)
        c, ptr = self.alloc(host.nbytes)
        c.memcpy_htod(ptr, host, host.nbytes)
        return c, ptr

    def array(self, a, dtype=None, stream=None):
        """A contiguous 2-D host array -> a contiguous DeviceArray of the same bytes (dtype: its name when NumPy has none)."""
        a = np.ascontiguousarray(a)
        _, ptr = self.put(a)
        return DeviceArray(ptr, a.shape, None, dtype or str(a.dtype), stream)

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture()
def prod():
    p = Producer()
    yield p
    p.close()


class Slot:
    """One device buffer that is filled again and again (the sweeps)."""

    def __init__(self, prod, nbytes):
        self.ctx, self.ptr = prod.alloc(nbytes)
        self.cap = nbytes

    def fill(self, a, dtype=None):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.cap
        self.ctx.memcpy_htod(self.ptr, a, a.nbytes)
        return DeviceArray(self.ptr, a.shape, None, dtype or str(a.dtype))


def bf16_bits(x):
    """float32 values that bfloat16 holds exactly -> their uint16 bit patterns."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def np_codes_u32(x):
    """metric.pack_codes in the layout get_packed returns: uint32 [n, ceil(b/32)]."""
    n, b = x.shape
    return metric.pack_codes(x).view(np.uint32).reshape(n, -1)[:, :(b + 31) // 32]


def np_label_words(lab):
    """Bit = (label != 0), also for matrices metric.pack_labels refuses (entries outside {0,1})."""
    n, C_ = lab.shape
    bits = np.zeros((n, (C_ + 63) // 64 * 64), dtype=np.uint8)
    bits[:, :C_] = lab != 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n, -1)


def np_census(x):
    with np.errstate(invalid="ignore"):
        return int((~np.isin(x, (-1.0, 0.0, 1.0))).sum()), int((x == 0).sum()), int((x == -1).sum())


def load_both(ctx, f, l, keep=None):
    """The same device arrays as database and as queries -> everything the loads report."""
    if keep is not None:
        ctx.set_option("keep_floats", keep)
    bad_db = ctx.set_database_dev(f, l)
    bad_q = ctx.set_queries_dev(f, l)
    return bad_db, bad_q, ctx.get_packed(0), ctx.get_packed(1), ctx.census(0), ctx.census(1)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context()
    yield c
    c.close()


# ------------------------------------------------------------------ 1. pack parity
PALETTE = (np.array([1.0], np.float32), np.array([-1.0], np.float32), np.array([0.0, -0.0], np.float32),
           np.array([0.5, -0.25, np.nan, np.inf, -np.inf], np.float32))     # plus ones, minus ones, zeros, everything else


def planted(rng, n, b, mask):
    """[n, b] float32 drawn from the palette classes whose bit is set in mask (1..15)."""
    vals = np.concatenate([PALETTE[k] for k in range(4) if mask >> k & 1])
    return vals[rng.integers(0, len(vals), (n, b))]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, 70001])      # WPB = 4: the block edge, a ragged last block; 70001: blocks stride over the rows
def test_pack_parity_with_numpy(ctx, prod, n):
    bs, Cs = (1, 31, 32, 33, 64, 65, 100, 128, 255), (1, 10, 63, 64, 65, 81, 200)
    if n > 257:
        bs, Cs = (33, 64), (10, 65)
    rng = np.random.default_rng(1000 + n)
    fs, ls = Slot(prod, n * 256 * 4), Slot(prod, n * 200 * 8)
    seen = np.zeros((4, 2), dtype=bool)                        # class x (empty, non-empty)
    k = 0
    for b in bs:
        for C_ in Cs:
            k += 1
            mask = k % 15 + 1
            x = planted(rng, n, b, mask)
            lab = (rng.random((n, C_)) < 0.3).astype(np.int64)
            bad_db, bad_q, (cd, ld), (cq, lq), cen_db, cen_q = load_both(ctx, fs.fill(x), ls.fill(lab), keep=0)
            want_c, want_l = np_codes_u32(x), metric.pack_labels(lab)
            other, zeros, neg = np_census(x)
            assert np.array_equal(cd, want_c) and np.array_equal(cq, want_c), (n, b, C_)
            assert np.array_equal(ld, want_l) and np.array_equal(lq, want_l), (n, b, C_)
            assert bad_db == (other, 0) and bad_q == (other, 0), (n, b, C_)
            assert cen_db == (other, zeros, neg, False) and cen_q == (other, zeros, neg, False), (n, b, C_)
            for cls, cnt in enumerate((x.size - other - zeros - neg, neg, zeros, other)):
                seen[cls, int(cnt > 0)] = True
    if n <= 257:
        assert seen.all()                                      # every census class was empty in some case and non-empty in another


# ------------------------------------------------------------------ 2. layouts
def test_every_layout_gives_the_same_tables(ctx, prod):
    n, b, C_ = 37, 33, 65
    rng = np.random.default_rng(2)
    x = planted(rng, n, b, 15)
    lab = (rng.random((n, C_)) < 0.3).astype(np.int64)
    want = load_both(ctx, prod.array(x), prod.array(lab), keep=1)
    assert np.array_equal(want[2][0], np_codes_u32(x)) and np.array_equal(want[2][1], metric.pack_labels(lab))
    assert want[4][3] and want[5][3]                            # (keep_floats = 1: the float rows are written too)

    def views(a, isz):
        name = str(a.dtype)
        rows, cols = a.shape
        wide = np.zeros((rows, cols + 7), a.dtype)               # row pitch > cols; pitch 40 floats = 160 bytes: the 16-byte path
        wide[:, :cols] = a
        yield "pitched", DeviceArray(prod.put(wide)[1], a.shape, (cols + 7, 1), name)
        off = np.full((rows, cols + 1), 7, a.dtype)              # x[:, 1:]: the base sits one element off
        off[:, 1:] = a
        yield "column slice", DeviceArray(prod.put(off)[1] + isz, a.shape, (cols + 1, 1), name)
        yield "transposed", DeviceArray(prod.put(a.T)[1], a.shape, (1, rows), name)
        both = np.full((rows * 2, cols * 3), 7, a.dtype)         # every second row, every third column
        both[::2, ::3] = a
        yield "both strides", DeviceArray(prod.put(both)[1], a.shape, (cols * 3 * 2, 3), name)

    for (what, f), (_, l) in zip(views(x, 4), views(lab, 8)):
        got = load_both(ctx, f, l, keep=1)
        for g, w in zip(got, want):
            if isinstance(w[0], np.ndarray):
                assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what
            else:
                assert g == w, what


def test_both_load_paths_write_the_same_float_rows(prod):
    """The 16-byte path and the element-wise path, through what they leave for the inner-product ranking: identical lists."""
    n, b, Q, R = 300, 33, 8, 300
    rng = np.random.default_rng(22)
    x = np.tanh(rng.standard_normal((n, b))).astype(np.float32)
    lab = np.eye(5, dtype=np.int64)[rng.integers(0, 5, n)]
    wide = np.zeros((n, 36), np.float32)
    wide[:, :b] = x
    off = np.zeros((n, b + 1), np.float32)
    off[:, 1:] = x
    l = prod.array(lab)
    layouts = {"16-byte": DeviceArray(prod.put(wide)[1], (n, b), (36, 1)), "element": DeviceArray(prod.put(off)[1] + 4, (n, b), (b + 1, 1))}
    out = {}
    for what, f in layouts.items():
        c = _native.Context()
        c.set_option("keep_floats", 1)
        c.set_database_dev(f, l)
        c.set_queries_dev(DeviceArray(f.ptr, (Q, b), f.strides), DeviceArray(l.ptr, (Q, 5), None, "int64"))
        out[what] = c.topr_real(R)
        c.close()
    assert np.array_equal(out["16-byte"][0], out["element"][0]) and np.array_equal(out["16-byte"][1], out["element"][1])


# ------------------------------------------------------------------ 3. dtypes
def test_feature_and_label_dtypes(ctx, prod):
    n, b, C_ = 37, 33, 65
    rng = np.random.default_rng(3)
    # values float16 AND bfloat16 hold exactly: small multiples of 1/8, the specials
    vals = np.array([1, -1, 0, -0.0, 0.5, -0.25, 1.5, -3.0, 0.125, np.nan, np.inf, -np.inf], np.float32)
    x = vals[rng.integers(0, len(vals), (n, b))]
    lab = (rng.random((n, C_)) < 0.3).astype(np.int64)
    want = load_both(ctx, prod.array(x), prod.array(lab), keep=1)
    assert want[0] == (np_census(x)[0], 0)
    f16 = x.astype(np.float16)
    assert np.array_equal(f16.astype(np.float32), x, equal_nan=True)

    def same(got, what):
        for g, w in zip(got, want):
            if isinstance(w[0], np.ndarray):
                assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what
            else:
                assert g == w, what

    l64 = prod.array(lab)
    same(load_both(ctx, prod.array(f16), l64, keep=1), "float16")
    same(load_both(ctx, prod.array(bf16_bits(x), "bfloat16"), l64, keep=1), "bfloat16")
    # 16-bit features off the 16-byte path as well: a column slice starting at element 1
    for name, bits in (("float16", f16.view(np.uint16)), ("bfloat16", bf16_bits(x))):
        off = np.zeros((n, b + 1), np.uint16)
        off[:, 1:] = bits
        same(load_both(ctx, DeviceArray(prod.put(off)[1] + 2, (n, b), (b + 1, 1), name), l64, keep=1), name + " slice")
    f32 = prod.array(x)
    same(load_both(ctx, f32, prod.array(lab.astype(np.int32)), keep=1), "int32 labels")
    same(load_both(ctx, f32, prod.array(lab.astype(np.uint8)), keep=1), "uint8 labels")
    same(load_both(ctx, f32, prod.array(lab.astype(bool)), keep=1), "bool labels")
    same(load_both(ctx, f32, prod.array(lab.astype(np.float32)), keep=1), "float32 labels")
    # entries that are not exactly 0 or 1 are counted, whatever the label dtype; the bit is still (v != 0)
    labf = lab.astype(np.float32)
    labf[0, 0], labf[5, 64], labf[36, 7] = 0.5, np.nan, -1.0
    got = load_both(ctx, f32, prod.array(labf), keep=1)
    assert got[0][1] == 3 and got[1][1] == 3 and np.array_equal(got[2][1], np_label_words(labf))
    labi = lab.copy()
    labi[1, 1], labi[2, 64] = 2, -1
    for dt in (np.int64, np.int32):
        got = load_both(ctx, f32, prod.array(labi.astype(dt)), keep=1)
        assert got[0][1] == 2 and np.array_equal(got[2][1], np_label_words(labi))
    got = load_both(ctx, f32, prod.array(np.where(labi == 2, 255, lab).astype(np.uint8)), keep=1)
    assert got[0][1] == 1


def test_sixteen_bit_features_on_the_16_byte_path(ctx, prod):
    """float16 / bfloat16 rows whose base and pitch are multiples of 16 bytes: a lane unpacks 8 halves, a code word is OR-ed across 4
    lanes, the float row leaves as two 16-byte stores per lane.  Same packed tables and census as the float32 run of the same values,
    and the same float rows -- seen through the inner-product lists they give."""
    n, C_ = 37, 65
    rng = np.random.default_rng(33)
    special = np.array([1, -1, 0, -0.0, 0.5, -0.25, 1.5, -3.0, 0.125, np.nan, np.inf, -np.inf], np.float32)
    finite = (np.arange(-16, 17) / 8).astype(np.float32)         # rankable; exact in both 16-bit formats and in float32 sums
    l64 = prod.array((rng.random((n, C_)) < 0.3).astype(np.int64))
    for b, pitch in ((64, 64), (33, 40), (255, 256)):            # contiguous; a view of a wider allocation, the last lane straddling the row's end
        for vals, ranked in ((special, False), (finite, True)):
            x = vals[rng.integers(0, len(vals), (n, b))]
            want = load_both(ctx, prod.array(x), l64, keep=1)
            want_lists = ctx.topr_real(n) if ranked else None
            assert want[0] == (np_census(x)[0], 0) and np.array_equal(want[2][0], np_codes_u32(x))
            for name, bits in (("float16", x.astype(np.float16).view(np.uint16)), ("bfloat16", bf16_bits(x))):
                wide = np.full((n, pitch), 0x3C00, np.uint16)    # (the columns beyond b are not zero: they must not be read as features)
                wide[:, :b] = bits
                f = DeviceArray(prod.put(wide)[1], (n, b), (pitch, 1), name)
                assert f.ptr % 16 == 0 and pitch * 2 % 16 == 0   # what the 16-byte path asks for
                got = load_both(ctx, f, l64, keep=1)
                for g, w in zip(got, want):
                    if isinstance(w[0], np.ndarray):
                        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (name, b)
                    else:
                        assert g == w, (name, b)
                if ranked:
                    idx, score = ctx.topr_real(n)
                    assert np.array_equal(idx, want_lists[0]) and np.array_equal(score.view(np.uint32), want_lists[1].view(np.uint32)), (name, b)


# ------------------------------------------------------------------ 4. ranking is the same call
def tables(seed, Q, N, b, C_, real):
    rng = np.random.default_rng(seed)
    if real:
        db, q = (np.tanh(rng.standard_normal((m, b))).astype(np.float32) for m in (N, Q))
    else:
        db, q = (np.where(rng.random((m, b)) < 0.5, 1.0, -1.0).astype(np.float32) for m in (N, Q))
    dl = np.eye(C_, dtype=np.int64)[rng.integers(0, C_, N)]
    ql = np.eye(C_, dtype=np.int64)[rng.integers(0, C_, Q)]
    ql[0] = 0                                                 # a query without a hit: its AP is NaN
    return q, db, ql, dl


@pytest.mark.parametrize("b, real", [(64, False), (100, False), (48, True), (255, True)])
def test_ranking_equals_the_host_array_path(prod, b, real):
    Q, N, C_ = 8, 300, 6
    q, db, ql, dl = tables(40 + b, Q, N, b, C_, real)
    host, dev = _native.Context(), _native.Context()
    host.set_database_f32(db, dl)
    host.set_queries_f32(q, ql)
    dev.set_database_dev(prod.array(db), prod.array(dl))
    dev.set_queries_dev(prod.array(q), prod.array(ql))
    assert host.census(0) == dev.census(0) and host.census(1) == dev.census(1)
    for R in (1, 50, 300):
        if real:
            (ap_h, rel_h), (ap_d, rel_d) = host.map_real(R), dev.map_real(R)
            (idx_h, sc_h), (idx_d, sc_d) = host.topr_real(R), dev.topr_real(R)
            assert np.array_equal(idx_h, idx_d) and np.array_equal(sc_h.view(np.uint32), sc_d.view(np.uint32)), R
        else:
            (ap_h, rel_h), (ap_d, rel_d) = host.map(R), dev.map(R)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, ap_o, *_ = O.map_from_codes(q > 0, db > 0, ql, dl, R)
            assert np.array_equal(ap_d, ap_o, equal_nan=True), R
        assert np.array_equal(ap_h.view(np.uint64), ap_d.view(np.uint64)) and np.array_equal(rel_h, rel_d), R
        assert np.isnan(ap_d[0]) and rel_d[0] == 0
    host.close()
    dev.close()


@pytest.mark.parametrize("real", [False, True])
def test_keep_floats_residency_matches_the_host_path(prod, real):
    q, db, ql, dl = tables(45, 8, 300, 64, 6, real)
    host, dev = _native.Context(), _native.Context()
    fd, ld, fq, lq = prod.array(db), prod.array(dl), prod.array(q), prod.array(ql)
    for keep in (0, 1, 2):
        host.set_option("keep_floats", keep)
        dev.set_option("keep_floats", keep)
        host.set_database_f32(db, dl)
        host.set_queries_f32(q, ql)
        dev.set_database_dev(fd, ld)
        dev.set_queries_dev(fq, lq)
        assert dev.census(0) == host.census(0) and dev.census(1) == host.census(1), keep
        assert dev.census(0)[3] == (keep == 1 or (keep == 2 and real)), keep
        if dev.census(0)[3]:                                     # (the second pass of keep_floats = 2 wrote the same rows)
            assert np.array_equal(host.map_real(50)[0].view(np.uint64), dev.map_real(50)[0].view(np.uint64)), keep
    host.close()
    dev.close()


# ------------------------------------------------------------------ 5. the Python surfaces; copy-in
def test_surfaces_take_device_arrays(prod):
    Q, N, b, C_, R = 8, 300, 64, 6, 50
    q, db, ql, dl = tables(50, Q, N, b, C_, False)
    want = MAP_per_query(q, db, ql, dl, R)
    dq, ddb, dql, ddl = prod.array(q), prod.array(db), prod.array(ql), prod.array(dl)
    got = MAP_per_query(dq, ddb, dql, ddl, R)
    assert got[0] == want[0] and np.array_equal(got[1], want[1], equal_nan=True) and np.array_equal(got[2], want[2])
    assert MAP(dq, ddb, dql, ddl, R) == want[0]
    assert MAP(q, ddb, ql, ddl, R) == want[0] and MAP(dq, db, dql, dl, R) == want[0]      # host and device sides mixed
    with pytest.raises(ValueError, match="same side"):
        MAP(q, ddb, ql, dl, R)

    # MAPs: what main.py:164 writes, on real-valued features and on +-1 codes
    for real in (True, False):
        q, db, ql, dl = tables(51, Q, N, b, C_, real)
        q2 = tables(52, Q, N, b, C_, real)[0]
        host_db, host_q, host_q2 = (types.SimpleNamespace(output=o, label=l) for o, l in ((db, dl), (q, ql), (q2, ql)))
        w1, w2 = MAPs(R).get_maps_by_feature(host_db, host_q), MAPs(R).get_maps_by_feature(host_db, host_q2)
        buf_c, buf_p = prod.put(db)
        dev_db = types.SimpleNamespace(output=DeviceArray(buf_p, db.shape), label=prod.array(dl))
        dev_q = types.SimpleNamespace(output=prod.array(q), label=prod.array(ql))
        assert MAPs(R).get_maps_by_feature(dev_db, host_q) == w1                           # device database, host queries
        assert MAPs(R).get_maps_by_feature(host_db, dev_q) == w1                           # and the other way round
        m = MAPs(R)
        m.set_database(dev_db)
        assert m.get_maps_by_feature(None, host_q) == w1 and m.get_maps_by_feature(dev_db, host_q2) == w2
        # copy-in: the caller's buffer is overwritten, the resident database is not
        zeros = np.zeros_like(db)
        buf_c.memcpy_htod(buf_p, zeros, zeros.nbytes)
        assert m.get_maps_by_feature(None, dev_q) == w1 and m.get_maps_by_feature(None, host_q2) == w2
        m.close()


# ------------------------------------------------------------------ 6. stream ordering
def hip_stream():
    """A non-blocking HIP stream of the test's own, if the runtime library can be reached through ctypes: (handle, destroy)."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        s = ctypes.c_void_p()
        if hip.hipStreamCreateWithFlags(ctypes.byref(s), ctypes.c_uint(1)) != 0 or not s.value:     # 1 = hipStreamNonBlocking
            return None, None
        return s.value, lambda: hip.hipStreamDestroy(s)
    except (OSError, AttributeError):
        return None, None


def test_the_load_waits_for_the_producers_stream(prod):
    """A load handed the producer's stream must wait for what is queued there.  The consumer context is created and its buffers are
    sized by throw-away loads of the same shapes BEFORE the producer's work is enqueued, so that nothing but the load's own host path
    lies between the enqueue and the pack kernel's launch; the producer's queue holds BACKLOG copies of 256 MB (64 GB moved: tens of
    milliseconds at the memory's rate) in front of the small copy that fills the buffer, which holds zeros until then.  The test
    measures how long the queue stays busy after the enqueue has returned and how long a whole warm load takes -- kernels and
    synchronisation included, an upper bound of the time to launch --, prints both and asserts the first to be more than ten times
    the second: it cannot pass because the queue happened to be empty.  A load that did not wait would pack the zeros."""
    import time
    BACKLOG, big = 128, 256 << 20
    Q, N, b, C_, R = 8, 300, 64, 6, 50
    q, db, ql, dl = tables(60, Q, N, b, C_, True)
    dq, dql, ddl = prod.array(q), prod.array(ql), prod.array(dl)
    ref = _native.Context()
    ref.set_option("keep_floats", 1)
    ref.set_database_dev(prod.array(db), ddl)                   # the synchronised run
    ref.set_queries_dev(dq, dql)
    want = ref.map_real(R)

    p = _native.Context()
    handle, destroy = hip_stream()
    if handle:
        p.set_stream(handle)
    a, bb, stage, buf = p.scratch(0, big), p.scratch(1, big), p.scratch(2, db.nbytes), p.scratch(3, db.nbytes)
    p.memcpy_htod(stage, db, db.nbytes)
    zeros = np.zeros_like(db)
    p.memcpy_htod(buf, zeros, zeros.nbytes)                     # what a load that does not wait would read
    got_ctx = _native.Context()
    got_ctx.set_option("keep_floats", 1)
    target = DeviceArray(buf, db.shape, None, "float32", handle)
    got_ctx.set_database_dev(target, ddl)                       # throw-away loads: every buffer of the consumer is there
    got_ctx.set_queries_dev(dq, dql)
    t0 = time.perf_counter()
    got_ctx.set_database_dev(target, ddl)
    host_path_ms = (time.perf_counter() - t0) * 1e3             # a whole warm load, kernels and synchronisation included: an upper bound
    assert got_ctx.get_packed(0)[0].any() == 0                  # (the zeros)

    def enqueue():
        for _ in range(BACKLOG):
            p.memcpy_dtod(bb, a, big)
        p.memcpy_dtod(buf, stage, db.nbytes)

    p.set_option("stage_sync", 0)                               # memcpy_dtod now only enqueues
    t0 = time.perf_counter()
    enqueue()                                                   # once for the clock (it writes what is already there afterwards)
    t1 = time.perf_counter()
    p.synchronize()
    drain_ms = (time.perf_counter() - t1) * 1e3                 # what was still queued when the last enqueue returned
    print("stream ordering: enqueue %.3f ms, queue still busy for %.3f ms after it, warm load %.3f ms" % ((t1 - t0) * 1e3, drain_ms, host_path_ms))
    p.set_option("stage_sync", 1)
    p.memcpy_htod(buf, zeros, zeros.nbytes)
    p.set_option("stage_sync", 0)
    enqueue()
    if not handle:
        p.synchronize()                                         # (no handle to pass: the context's own stream cannot be named)
    got_ctx.set_database_dev(target, ddl)
    got_ctx.set_queries_dev(dq, dql)
    got = got_ctx.map_real(R)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1])
    if handle:
        assert drain_ms > 10 * host_path_ms, (drain_ms, host_path_ms)
    p.synchronize()
    if handle:
        p.set_stream(None)
        destroy()
    for c in (ref, p, got_ctx):
        c.close()


# ------------------------------------------------------------------ 7. refusals that never launch
def test_bad_descriptors_are_refused_before_any_launch(prod):
    Q, N, b, C_, R = 8, 300, 64, 6, 50
    q, db, ql, dl = tables(70, Q, N, b, C_, False)
    want = MAP_per_query(q, db, ql, dl, R)
    dq, ddb, dql, ddl = prod.array(q), prod.array(db), prod.array(ql), prod.array(dl)
    c = _native.Context()

    def still_works():
        c.set_database_dev(ddb, ddl)
        c.set_queries_dev(dq, dql)
        ap, rel = c.map(R)
        assert np.array_equal(ap, want[1], equal_nan=True) and np.array_equal(rel, want[2])

    def refused(f, l, queries=False):
        with pytest.raises(_native.HashganNativeError) as e:
            (c.set_queries_dev if queries else c.set_database_dev)(f, l)
        assert e.value.code == _native.HG_ERR_ARG, str(e.value)
        still_works()

    still_works()
    host_mem = np.ones((N, b), np.float32)
    refused(DeviceArray(host_mem.ctypes.data, (N, b)), ddl)                               # a NumPy array's host address
    refused(ddb, DeviceArray(dl.ctypes.data, dl.shape, None, "int64"))
    # an extent that runs one element past its allocation.  Where the allocation ends is asked of the library, not assumed: a
    # descriptor that certainly overruns it (64 times the request) is refused with a message that says how far from the pointer
    # the allocation ends -- whatever slack, rounding or cached block the allocator chose
    edge = _native.Context()
    nbytes = 1 << 20
    ptr = edge.scratch(0, nbytes)
    zeros = np.zeros((nbytes // 4,), np.float32)
    edge.memcpy_htod(ptr, zeros, zeros.nbytes)
    with pytest.raises(_native.HashganNativeError) as e:
        c.set_database_dev(DeviceArray(ptr, (64 * nbytes // (b * 4), b)), DeviceArray(ddl.ptr, (64 * nbytes // (b * 4), C_), (C_, 1), "int64"))
    assert e.value.code == _native.HG_ERR_ARG
    size = int(re.search(r"allocation ends (\d+) bytes from there", str(e.value)).group(1))
    assert nbytes <= size < 64 * nbytes and size % 4 == 0, str(e.value)
    still_works()
    rows = size // (b * 4)
    last = ptr + size - rows * b * 4                                                      # [last, last + rows x b x 4) ends where the allocation ends
    lab_rows = prod.array(np.ones((rows, C_), np.int64))
    c.set_database_dev(DeviceArray(last, (rows, b)), lab_rows)                            # accepted: ends exactly there
    refused(DeviceArray(last + 4, (rows, b)), lab_rows)                                   # one float further
    refused(DeviceArray(last, (rows, b), (b, 1), "float32"), DeviceArray(lab_rows.ptr, (rows, C_), (64 * C_, 1), "int64"))   # labels past THEIR allocation
    refused(DeviceArray(ddb.ptr, (N, b), None, "int64"), ddl)                             # an int64 feature dtype
    refused(ddb, DeviceArray(ddl.ptr, dl.shape, None, "float16"))
    refused(types.SimpleNamespace(ptr=ddb.ptr, shape=(N, b), strides=(b, 0), dtype="float32", stream=None), ddl)   # a stride of 0
    refused(types.SimpleNamespace(ptr=ddb.ptr, shape=(N, b), strides=(-b, 1), dtype="float32", stream=None), ddl)
    refused(ddb, DeviceArray(ddl.ptr, (N - 1, C_), None, "int64"))                        # unequal row counts
    refused(DeviceArray(dq.ptr, (Q, b - 1), (b, 1)), dql, queries=True)                   # queries of another width
    edge.close()
    c.close()


# ------------------------------------------------------------------ 8. torch, where present
def test_torch_tensors_on_the_current_stream():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    Q, N, b, C_, R = 8, 300, 48, 6, 50
    g = torch.Generator().manual_seed(8)
    dev = torch.device("cuda")
    db = torch.tanh(torch.randn(N, b + 3, generator=g)).to(dev)
    q = torch.tanh(torch.randn(Q, b, generator=g)).to(dev).to(torch.bfloat16)
    dl = torch.nn.functional.one_hot(torch.randint(0, C_, (N,), generator=g), C_).to(dev)
    ql = torch.nn.functional.one_hot(torch.randint(0, C_, (Q,), generator=g), C_).to(dev)
    db_view = db[:, 2:2 + b]                                     # a non-contiguous float32 slice with a misaligned base
    assert not db_view.is_contiguous()
    host = lambda t: t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()
    want = MAPs(R).get_maps_by_feature(types.SimpleNamespace(output=host(db_view), label=host(dl)),
                                       types.SimpleNamespace(output=host(q), label=host(ql)))
    got = MAPs(R).get_maps_by_feature(types.SimpleNamespace(output=db_view, label=dl), types.SimpleNamespace(output=q, label=ql))
    assert got == want

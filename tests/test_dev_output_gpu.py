"""Results written into the caller's DEVICE memory (hg_export, devarray.DeviceOut, MAPs.rank_into): every item in every dtype against
the host getters byte for byte, prefixes, every layout with canaries around and between the addressed elements, blocks that stride,
refusals that write nothing, stream ordering in both directions, and the Python surfaces.

Device memory comes from private producer contexts (scratch + memcpy_htod / memcpy_dtoh): nothing here needs torch (the last test
uses it where present)."""
import ctypes
import re
import time
import types

import numpy as np
import pytest

from hashgan_amd import _native, extra_metrics
from hashgan_amd import MAP_per_query, MAPs
from hashgan_amd.devarray import DeviceArray, DeviceOut
from tests.dev_arena import CANARY, NP, Arena               # device memory without a framework (shared with tests/test_second_hand_gpu.py)

pytestmark = pytest.mark.gpu

ARG, STATE = _native.HG_ERR_ARG, _native.HG_ERR_STATE
Q, N, B, C_ = 5, 400, 64, 6


@pytest.fixture()
def arena():
    a = Arena(1 << 20)
    yield a
    a.close()


def raises(code, fn, *args):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    return str(e.value)


# ------------------------------------------------------------------ base data, ranked once per (kind, R) where a test shares it
def tables(seed, Q_, N_, b, C, real):
    rng = np.random.default_rng(seed)
    if real:
        db, q = (np.tanh(rng.standard_normal((m, b))).astype(np.float32) for m in (N_, Q_))
    else:
        db, q = (np.where(rng.random((m, b)) < 0.5, 1.0, -1.0).astype(np.float32) for m in (N_, Q_))
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, C, N_)]
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, C, Q_)]
    ql[0] = 0                                                 # a query without a hit: its AP is NaN
    return q, db, ql, dl


CODES = tables(900, Q, N, B, C_, False)
FEATS = tables(901, Q, N, B, C_, True)


def context(data, keep_floats=None):
    q, db, ql, dl = data
    c = _native.Context()
    if keep_floats is not None:
        c.set_option("keep_floats", keep_floats)
    c.set_database_f32(db, dl)
    c.set_queries_f32(q, ql)
    return c


@pytest.fixture(scope="module")
def ham():
    c = context(CODES)
    yield c
    c.close()


@pytest.fixture(scope="module")
def real():
    c = context(FEATS, keep_floats=1)
    yield c
    c.close()


def rank_hamming(ctx, R):
    """hg_topr + match + AP -> what the host getters return."""
    ctx.topr(R)
    ctx.match()
    ctx.ap()
    idx, dist = ctx.get_topr()
    ap, rel = ctx.get_ap()
    assert np.isnan(ap[0]) and rel[0] == 0
    return dict(idx=idx, dist=dist, match=ctx.get_match(), ap=ap, hits=rel)


def rank_rerank(ctx, R):
    idx, dist, score = ctx.topr_rerank(R)
    ctx.ap()
    ap, rel = ctx.get_ap()
    return dict(idx=idx, dist=dist, score=score, match=ctx.get_match(), ap=ap, hits=rel)


def keep_grades(ctx, R):
    ctx.graded((R,), np.arange(C_ + 1, dtype=np.float64), np.ones(R), keep_grades=True)
    return ctx.get_grades()


def converted(name, host, dtype, k=None):
    """A getter's array as the export writes it: [Q, k] (or [Q, 1]) of `dtype`."""
    a = host.reshape(host.shape[0], -1)
    if k is not None:
        a = a[:, :k]
    if name == "score":
        return np.ascontiguousarray(a)                        # the same bits
    if name == "idx" and dtype == "int32":
        return np.ascontiguousarray(a).view(np.int32)         # the same low 32 bits
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(a.astype(NP[dtype]))


DTYPES = {"idx": ("int64", "int32"), "dist": ("uint8", "int32"), "score": ("float32",), "match": ("uint8",), "ap": ("float64", "float32"),
          "hits": ("int64", "int32"), "grades": ("uint8", "int32")}


def export_all(ctx, arena, host, k, names=None):
    """Every item of `host` in every allowed dtype into contiguous destinations (at most 8 per call), checked against the getters."""
    arena.reset()
    todo = [(n, dt) for n in (names or host) for dt in DTYPES[n]]
    done = []
    for i in range(0, len(todo), 8):
        items = []
        for n, dt in todo[i:i + 8]:
            want = converted(n, host[n], dt, None if n in ("ap", "hits") else k)
            d = arena.out(want.shape, dt)
            arena.expect(d, want)
            items.append((n, d))
        ctx.export(items)
        assert ctx.get_stat("export_bytes") == sum(d.shape[0] * d.shape[1] * d.itemsize for _, d in items)
        done += items
    got = arena.read()
    ap32 = [d for n, d in done if n == "ap" and d.dtype == "float32"]
    for d in ap32:                                            # float32 AP: NaN where the float64 is NaN (whatever NaN it is), else the rounded value
        o = d.ptr - arena.base
        g, w = got[o:o + Q * 4].view(np.float32), arena.host[o:o + Q * 4].view(np.float32)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.isnan(g[0])
        got[o:o + Q * 4][np.repeat(np.isnan(g), 4)] = arena.host[o:o + Q * 4][np.repeat(np.isnan(g), 4)]
    bad = np.flatnonzero(got != arena.host)
    assert bad.size == 0, "k=%d: %d bytes differ, the first at offset %d" % (k, bad.size, bad[0])


# ------------------------------------------------------------------ 1. bytes equal the host getters
@pytest.mark.parametrize("R", [1, 63, 64, 65, 130, 400])     # the bitmap's word edges; k = R
def test_hamming_items_equal_the_getters(ham, arena, R):
    host = rank_hamming(ham, R)
    export_all(ham, arena, host, R)
    host["grades"] = keep_grades(ham, R)
    export_all(ham, arena, host, R, names=("grades",))
    # float64 AP: the very bits, NaN included
    arena.reset()
    d = arena.out((Q, 1), "float64")
    ham.export([("ap", d)])
    o = d.ptr - arena.base
    assert np.array_equal(arena.read()[o:o + Q * 8].view(np.uint64), host["ap"].view(np.uint64))


@pytest.mark.parametrize("R", [1, 63, 64, 65, 130, 400])
def test_real_valued_items_equal_the_getters(real, arena, R):
    idx, score = real.topr_real(R)
    real.match()
    real.ap()
    ap, rel = real.get_ap()
    host = dict(idx=idx, score=score, match=real.get_match(), ap=ap, hits=rel)
    export_all(real, arena, host, R)
    raises(STATE, real.export, [("dist", arena.out((Q, R), "uint8"))])                  # an inner-product ranking has no distances


@pytest.mark.parametrize("R", [1, 63, 64, 65, 130, 400])
def test_rerank_items_equal_the_getters(real, arena, R):
    host = rank_rerank(real, R)
    assert np.array_equal(host["score"], real.get_rerank_scores())
    export_all(real, arena, host, R)
    host["grades"] = keep_grades(real, R)
    export_all(real, arena, host, R, names=("grades",))


# ------------------------------------------------------------------ 2. prefixes
@pytest.mark.parametrize("k", [1, 17, 129])
def test_the_first_k_ranks(real, arena, k):
    R = 130
    host = rank_rerank(real, R)
    host["grades"] = keep_grades(real, R)
    export_all(real, arena, host, k)                                                    # (the first k columns of every list)


# ------------------------------------------------------------------ 3. layouts and canaries
def layouts(dtype, k):
    """(name, k, strides, skip, takes the 16-byte path) for a [Q, k] destination of `dtype`."""
    isz = NP[dtype]().itemsize
    pitch37 = (37 * isz + 15) // 16 * 16 // isz
    return [("pitched", k, (k + 3, 1), 0, False),
            ("column stride 2", k, (2 * k + 1, 2), 0, False),
            ("transposed", k, (1, Q), 0, False),
            ("one element off", k, (k, 1), 1, False),
            ("aligned pitch, k = 37", 37, (pitch37, 1), 0, True)]


def test_every_layout_and_the_bytes_around_it(real, arena):
    R = 130
    host = rank_rerank(real, R)
    host["grades"] = keep_grades(real, R)
    seen = set()
    for name, dtype in (("idx", "int64"), ("idx", "int32"), ("dist", "uint8"), ("dist", "int32"), ("score", "float32"), ("match", "uint8"),
                        ("grades", "uint8")):
        for what, k, strides, skip, vec in layouts(dtype, R):
            arena.reset()
            d = arena.out((Q, k), dtype, strides, skip)
            if vec:
                assert d.ptr % 16 == 0 and d.strides[0] * d.itemsize % 16 == 0 and k % (16 // d.itemsize) != 0     # a straddling tail
            arena.expect(d, converted(name, host[name], dtype, k))
            real.export([(name, d)])
            arena.check("%s as %s, %s" % (name, dtype, what))
            assert real.get_stat("export_variant") == (1 if vec else 2), (name, dtype, what)
            seen.add(real.get_stat("export_variant"))
    assert seen == {1, 2}                                                               # both paths ran
    # one value per query: a pitched column, a column one element off, a one-column view with a wide column stride
    for name, dtype in (("ap", "float64"), ("ap", "float32"), ("hits", "int64"), ("hits", "int32")):
        want = converted(name, host[name], dtype)
        for strides, skip in (((4, 1), 0), ((1, 1), 1), ((3, 7), 0)):
            arena.reset()
            d = arena.out((Q, 1), dtype, strides, skip)
            arena.expect(d, want)
            real.export([(name, d)])
            got = arena.read()
            if name == "ap":                                                            # (the NaN of query 0: any NaN)
                o = d.ptr - arena.base
                assert np.isnan(got[o:o + d.itemsize].view(NP[dtype])[0])
                got[o:o + d.itemsize] = arena.host[o:o + d.itemsize]
            assert np.array_equal(got, arena.host), (name, dtype, strides, skip)
    # both paths in one call, and a contiguous run on the 16-byte path equals the element-wise run
    arena.reset()
    a, b_ = arena.out((Q, 128), "int64"), arena.out((Q, 128), "int64", None, 1)
    arena.expect(a, converted("idx", host["idx"], "int64", 128))
    arena.expect(b_, converted("idx", host["idx"], "int64", 128))
    real.export([("idx", a), ("idx", b_)])
    arena.check("two paths")
    assert real.get_stat("export_variant") == 3


# ------------------------------------------------------------------ 4. blocks stride over the elements
def test_more_elements_than_one_pass_of_the_grid():
    Q_, N_ = 2100, 4100                                      # Q x k = 8.6 M elements: the bounded grid's blocks go round many times
    q, db, ql, dl = tables(904, Q_, N_, 32, C_, False)
    ctx = context((q, db, ql, dl))
    pitch = (N_ + 15) // 16 * 16                             # match rows at a multiple of 16 bytes: the 16-byte path
    big = Arena(Q_ * (N_ * 8 + pitch) + 4096)
    try:
        ctx.topr(N_)
        ctx.match()
        idx, _ = ctx.get_topr()
        match = ctx.get_match()
        for strides, skip in ((None, 0), (None, 1)):          # the 16-byte path, the element-wise path
            big.reset()
            di, dm = big.out((Q_, N_), "int64", strides, skip), big.out((Q_, N_), "uint8", (pitch, 1), skip)
            big.expect(di, idx.astype(np.int64))
            big.expect(dm, match)
            ctx.export([("idx", di), ("match", dm)])
            big.check("Q x k = %d, skip %d" % (Q_ * N_, skip))
            assert ctx.get_stat("export_variant") == (2 if skip else 1)
    finally:
        big.close()
        ctx.close()


# ------------------------------------------------------------------ 5. refusals write nothing
def test_refused_descriptors_write_nothing(ham, arena):
    R = 130
    host = rank_hamming(ham, R)
    arena.reset()
    spot = arena.out((Q, R), "int64")                          # room for every case below
    ptr = spot.ptr

    def refused(items, code=ARG):
        msg = raises(code, ham.export, items)
        assert arena.untouched(), msg
        return msg

    refused([("idx", DeviceOut(ptr, (Q, R), None, "float32"))])                          # a dtype outside the item's list
    refused([("dist", DeviceOut(ptr, (Q, R), None, "int64"))])
    refused([("match", DeviceOut(ptr, (Q, R), None, "int32"))])
    refused([("ap", DeviceOut(ptr, (Q, 1), None, "int64"))])
    refused([("score", DeviceOut(ptr, (Q, R), None, "float32"))], STATE)                 # a plain Hamming ranking has no scores
    refused([("idx", types.SimpleNamespace(ptr=ptr, shape=(Q, R), strides=(R, 1), dtype="float16", stream=None))])
    refused([("idx", DeviceOut(ptr, (Q - 1, R), None, "int64"))])                        # rows != Q
    refused([("idx", DeviceOut(ptr, (Q + 1, R), None, "int32"))])
    refused([("idx", DeviceOut(ptr, (Q, R + 1), None, "int32"))])                        # k > R
    refused([("ap", DeviceOut(ptr, (Q, 2), None, "float64"))])                           # cols != 1
    refused([("hits", DeviceOut(ptr, (Q, 2), None, "int64"))])
    refused([("idx", DeviceOut(ptr, (Q, 3), (2, 1), "int64"))])                          # aliasing strides
    refused([("idx", DeviceOut(ptr, (Q, 2), (1, 1), "int64"))])
    refused([("idx", types.SimpleNamespace(ptr=ptr, shape=(Q, R), strides=(R, 0), dtype="int64", stream=None))])     # a stride of 0
    refused([("idx", types.SimpleNamespace(ptr=ptr, shape=(Q, R), strides=(-R, 1), dtype="int64", stream=None))])
    refused([("idx", types.SimpleNamespace(ptr=ptr, shape=(Q, 2), strides=(2 ** 62, 1), dtype="int64", stream=None))])   # an extent beyond 63 bits
    refused([("idx", types.SimpleNamespace(ptr=0, shape=(Q, R), strides=(R, 1), dtype="int64", stream=None))])       # a null pointer
    refused([(7, DeviceOut(ptr, (Q, R), None, "int64"))])                                # an unknown item
    refused([])                                                                          # no item; more than eight
    refused([("match", DeviceOut(ptr + 64 * i, (Q, 1), None, "uint8")) for i in range(9)])
    host_mem = np.full((Q, R), 7, np.int64)
    refused([("idx", DeviceOut(host_mem.ctypes.data, (Q, R), None, "int64"))])           # a NumPy array's host address
    assert (host_mem == 7).all()
    # two items of one call that intersect; one good and one bad item: neither is written
    refused([("idx", DeviceOut(ptr, (Q, R), None, "int64")), ("dist", DeviceOut(ptr + 8 * R, (Q, R), None, "uint8"))])
    refused([("idx", DeviceOut(ptr, (Q, 8), None, "int64")), ("match", DeviceOut(ptr + 8 * 8 * Q - 1, (Q, 8), None, "uint8"))])
    refused([("idx", DeviceOut(ptr, (Q, 8), None, "int64")), ("dist", DeviceOut(ptr + 1024, (Q, R + 1), None, "uint8"))])
    refused([("idx", DeviceOut(ptr, (Q, 8), None, "int64")), ("score", DeviceOut(ptr + 1024, (Q, 8), None, "float32"))], STATE)
    # the destination inside a result buffer of the context (hg_topr_buffers names the lists)
    p_idx, p_dist, slots = ham.topr_buffers()
    assert slots == Q * R
    refused([("dist", DeviceOut(p_idx, (Q, R), None, "uint8"))])
    refused([("idx", DeviceOut(p_idx, (Q, R // 2), None, "int32"))])
    refused([("match", DeviceOut(p_dist + 3, (Q, 1), (7, 1), "uint8"))])
    idx, dist = ham.get_topr()
    assert np.array_equal(idx, host["idx"]) and np.array_equal(dist, host["dist"])
    # hg_set_*_dev keep refusing float64
    f64 = DeviceOut(ptr, (Q, B), None, "float64")
    raises(ARG, ham.set_queries_dev, f64, DeviceArray(ptr, (Q, C_), None, "int64"))
    ham.set_queries_f32(CODES[0], CODES[2])                                              # (the refused load left no queries behind)
    rank_hamming(ham, R)
    # and the accepted call still works
    d = DeviceOut(ptr, (Q, R), None, "int64")
    arena.expect(d, host["idx"].astype(np.int64))
    ham.export([("idx", d)])
    arena.check("after the refusals")


def test_an_extent_one_element_past_its_allocation(ham):
    """Where the allocation ends is asked of the library, not assumed: a descriptor that certainly overruns it is refused with a message
    that says how far from the pointer the allocation ends -- whatever slack, rounding or cached block the allocator chose."""
    R = 65
    host = rank_hamming(ham, R)
    edge = _native.Context()
    nbytes = 1 << 20
    ptr = edge.scratch(0, nbytes)
    fill = np.full(64 * nbytes, CANARY, np.uint8)
    edge.memcpy_htod(ptr, fill, nbytes)
    try:
        msg = raises(ARG, ham.export, [("match", DeviceOut(ptr, (Q, 1), (16 * nbytes, 1), "uint8"))])
        size = int(re.search(r"allocation ends (\d+) bytes from there", msg).group(1))
        assert nbytes <= size < 64 * nbytes, msg
        edge.memcpy_htod(ptr, fill, size)
        rs = (size - R) // (Q - 1)
        last = ptr + size - ((Q - 1) * rs + R)                 # [last, last + extent) ends where the allocation ends
        raises(ARG, ham.export, [("match", DeviceOut(last + 1, (Q, R), (rs, 1), "uint8"))])     # one byte further
        rs4 = (size // 4 - R) // (Q - 1)                        # the same with 4-byte elements, one element further
        raises(ARG, ham.export, [("dist", DeviceOut(ptr + size - ((Q - 1) * rs4 + R) * 4 + 4, (Q, R), (rs4, 1), "int32"))])
        got = np.empty(size, np.uint8)
        edge.memcpy_dtoh(got, ptr, size)
        assert (got == CANARY).all()
        ham.export([("match", DeviceOut(last, (Q, R), (rs, 1), "uint8"))])                      # accepted: ends exactly there
        edge.memcpy_dtoh(got, ptr, size)
        o = last - ptr
        for q in range(Q):
            assert np.array_equal(got[o + q * rs:o + q * rs + R], host["match"][q])
            got[o + q * rs:o + q * rs + R] = CANARY
        assert (got == CANARY).all()
    finally:
        edge.close()


def test_state_refusals(arena):
    R = 50
    gain, disc = np.arange(C_ + 1, dtype=np.float64), np.ones(R)
    real, ham = context(FEATS, keep_floats=1), context(CODES)
    arena.reset()
    ptr = arena.out((Q, R), "int64").ptr
    every = [("idx", DeviceOut(ptr, (Q, R), None, "int64")), ("dist", DeviceOut(ptr, (Q, R), None, "uint8")),
             ("score", DeviceOut(ptr, (Q, R), None, "float32")), ("match", DeviceOut(ptr, (Q, R), None, "uint8")),
             ("ap", DeviceOut(ptr, (Q, 1), None, "float64")), ("hits", DeviceOut(ptr, (Q, 1), None, "int64")),
             ("grades", DeviceOut(ptr, (Q, R), None, "uint8"))]
    item = dict(every)

    def refused(ctx, *names):
        for n in names:
            msg = raises(STATE, ctx.export, [(n, item[n])])
            assert "hg_" in msg, msg                                                     # (it names the call that would provide the item)
        assert arena.untouched()

    def accepted(ctx, *names):
        for n in names:
            ctx.export([(n, item[n])])
        arena.reset()

    try:
        for ctx in (real, ham):
            refused(ctx, *item)                                                          # nothing ranked yet
        real.topr_real(R)
        refused(real, "dist", "grades")                                                  # DIST after topr_real
        accepted(real, "idx", "score", "match")
        ham.topr(R)
        refused(ham, "score", "ap", "hits", "grades")                                    # SCORE after a plain topr; no AP yet
        accepted(ham, "idx", "dist", "match")
        ham.ap()
        accepted(ham, "ap", "hits")
        ham.graded((R,), gain, disc)
        refused(ham, "grades")                                                           # GRADES without keep_grades
        ham.graded((R,), gain, disc, keep_grades=True)
        accepted(ham, "grades")
        ham.topr(R)
        refused(ham, "grades")                                                           # a later ranking ends them
        ham.map(R)
        refused(ham, "idx", "dist", "score")                                             # IDX after map: no lists
        accepted(ham, "match", "ap", "hits")
        real.topr_rerank(R)
        accepted(real, "idx", "dist", "score", "match")
        real.topr_real(R)
        refused(real, "dist")
        accepted(real, "score")
        # a query reload ends everything
        ham.topr(R)
        ham.ap()
        ham.graded((R,), gain, disc, keep_grades=True)
        ham.set_queries_f32(CODES[0], CODES[2])
        refused(ham, *item)
        # a step of hg_map_begin in flight: nothing is handed out
        ham.topr(R)
        ham.ap()
        accepted(ham, "idx", "ap")
        ham.map(R)
        ham.map_begin(R)
        refused(ham, *item)
        ham.map_end()
        ham.topr(R)
        accepted(ham, "idx", "dist", "match")
    finally:
        real.close()
        ham.close()


# ------------------------------------------------------------------ 6. stream ordering, both directions
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


def test_ordering_with_the_consumers_stream(ham):
    """No host synchronisation between producer and consumer ("stage_sync" = 0 on both contexts; the consumer runs on a non-blocking
    stream of the test's own).
      consumer sees the data   the exporting context's stream holds BACKLOG device-to-device copies of 256 MB; the export behind them
                               names the consumer's stream; the consumer enqueues a copy of the destination into a second buffer and
                               only the consumer synchronises: the second buffer holds the exported values, not the canary.
      export waits for readers the consumer's stream holds the backlog and then a copy OUT OF the destination; the export that
                               overwrites the destination is enqueued at once: the saved copy holds the old contents.
    Each half measures how long the queue stays busy after the enqueue has returned and how long a whole warm export takes -- kernel
    and synchronisation included, an upper bound of the time to launch --, prints both and asserts the first to be more than ten times
    the second: neither can pass because the queue happened to be empty.  (Measured with 64 copies: busy for 6.7 / 6.0 ms against a
    warm export of 0.03 ms; 16 copies -- 4 GB moved -- leave a factor of about fifty.)"""
    BACKLOG, big = 16, 256 << 20
    R = 130
    exp, con = context(CODES), _native.Context()
    handle, destroy = hip_stream()
    if handle:
        con.set_stream(handle)
    try:
        host = rank_hamming(exp, R)
        want = host["idx"].astype(np.int64)
        n = want.nbytes
        canary, old = np.full(n, CANARY, np.uint8), np.full(n, 0x5A, np.uint8)
        dst, second = con.scratch(0, n), con.scratch(1, n)
        got = np.empty(n, np.uint8)
        item = [("idx", DeviceOut(dst, (Q, R), None, "int64", handle))]
        exp.export(item)                                       # warm: code object, events
        t0 = time.perf_counter()
        exp.export(item)
        export_ms = (time.perf_counter() - t0) * 1e3
        for first in ("export", "reader"):
            busy = exp if first == "export" else con           # whose stream holds the backlog
            a, b_ = busy.scratch(2, big), busy.scratch(3, big)
            con.memcpy_htod(dst, canary if first == "export" else old, n)
            con.memcpy_htod(second, canary, n)
            exp.set_option("stage_sync", 0)
            con.set_option("stage_sync", 0)
            t0 = time.perf_counter()
            for _ in range(BACKLOG):
                busy.memcpy_dtod(b_, a, big)
            if first == "export":
                exp.export(item)                               # behind the backlog; the consumer's stream waits for it
                if not handle:
                    exp.synchronize()                          # (no handle to pass: the consumer's own stream cannot be named)
                con.memcpy_dtod(second, dst, n)
            else:
                con.memcpy_dtod(second, dst, n)                # the earlier reader of the destination, behind the backlog
                if not handle:
                    con.synchronize()
                exp.export(item)                               # waits for it, then overwrites
            t1 = time.perf_counter()
            con.synchronize()                                  # only the consumer waits
            drain_ms = (time.perf_counter() - t1) * 1e3
            if first == "reader":
                exp.synchronize()
            exp.set_option("stage_sync", 1)
            con.set_option("stage_sync", 1)
            print("export ordering (%s first): enqueue %.3f ms, queue still busy for %.3f ms after it, warm export %.3f ms"
                  % (first, (t1 - t0) * 1e3, drain_ms, export_ms))
            con.memcpy_dtoh(got, second, n)
            if first == "export":
                assert np.array_equal(got.view(np.int64).reshape(Q, R), want)            # not the canary
            else:
                assert np.array_equal(got, old)                                          # the old contents were read first
                con.memcpy_dtoh(got, dst, n)
                assert np.array_equal(got.view(np.int64).reshape(Q, R), want)            # and then overwritten
            if handle:
                assert drain_ms > 10 * export_ms, (first, drain_ms, export_ms)
            exp.synchronize()
    finally:
        exp.synchronize()
        con.synchronize()
        if handle:
            con.set_stream(None)
            destroy()
        exp.close()
        con.close()


# ------------------------------------------------------------------ 7. the Python surfaces
def ns(out, lab):
    return types.SimpleNamespace(output=out, label=lab)


def test_rank_into_against_the_host_calls(arena):
    R, k = 130, 17
    q, db, ql, dl = CODES
    fq, fdb, fql, fdl = FEATS

    def outs(names, k_=R):
        arena.reset()
        return {n: arena.out((Q, 1) if n in ("ap", "hits") else (Q, k_), DTYPES[n][0]) for n in names}

    def fill(o, host, k_=R):
        for n, d in o.items():
            arena.expect(d, converted(n, host[n], d.dtype, None if n in ("ap", "hits") else k_))

    def check_but_nan(o, what):
        got = arena.read()
        if "ap" in o:                                           # (query 0 has no hit: any NaN)
            off = o["ap"].ptr - arena.base
            assert np.isnan(got[off:off + 8].view(np.float64)[0])
            got[off:off + 8] = arena.host[off:off + 8]
        assert np.array_equal(got, arena.host), what

    # +-1 codes: the Hamming kernels
    ref = context(CODES)
    host = rank_hamming(ref, R)
    ap_host = MAP_per_query(q, db, ql, dl, R)
    assert np.array_equal(ap_host[1].view(np.uint64), host["ap"].view(np.uint64))
    m = MAPs(R)
    o = outs(("idx", "dist", "match", "ap", "hits"))
    assert m.rank_into(ns(db, dl), ns(q, ql), **o) == {"by": "hamming", "R": R}
    fill(o, host)
    check_but_nan(o, "MAPs(R).rank_into")
    o = outs(("idx", "match"), k)                               # a prefix, against the resident database
    assert m.rank_into(None, ns(q, ql), **o) == {"by": "hamming", "R": R}
    fill(o, host, k)
    arena.check("prefix")
    with pytest.raises(ValueError, match="score"):
        m.rank_into(None, ns(q, ql), score=outs(("score",))["score"])
    assert arena.untouched()
    m.close()
    o = outs(("idx", "dist", "ap"))
    assert extra_metrics.rank_into(q, db, ql, dl, R, **o) == {"by": "hamming", "R": R}
    fill(o, host)
    check_but_nan(o, "extra_metrics.rank_into")
    ref.close()

    # real-valued features: inner product; binarize: sign() first; rerank
    ref = context(FEATS, keep_floats=1)
    idx, score = ref.topr_real(R)
    ap, rel = ref.map_real(R)
    m = MAPs(R)
    o = outs(("idx", "score", "ap", "hits"))
    assert m.rank_into(ns(fdb, fdl), ns(fq, fql), **o) == {"by": "inner_product", "R": R}
    fill(o, dict(idx=idx, score=score, ap=ap, hits=rel))
    check_but_nan(o, "inner product")
    with pytest.raises(ValueError, match="dist"):
        m.rank_into(None, ns(fq, fql), dist=outs(("dist",))["dist"])
    assert arena.untouched()
    m.close()
    o = outs(("idx", "score"))
    assert extra_metrics.rank_into(fq, fdb, fql, fdl, R, features=True, **o) == {"by": "inner_product", "R": R}
    fill(o, dict(idx=idx, score=score))
    arena.check("extra_metrics.rank_into, features")

    host = rank_rerank(ref, R)
    m = MAPs(R, rerank=True)
    o = outs(("idx", "dist", "score", "match", "ap", "hits"))
    assert m.rank_into(ns(fdb, fdl), ns(fq, fql), **o) == {"by": "rerank", "R": R}
    fill(o, host)
    check_but_nan(o, "rerank")
    m.close()
    o = outs(("idx", "dist", "score"))
    assert extra_metrics.rank_into(fq, fdb, fql, fdl, R, rerank=True, **o) == {"by": "rerank", "R": R}
    fill(o, host)
    arena.check("extra_metrics.rank_into, rerank")
    ref.close()

    sign = context((np.sign(fq), np.sign(fdb), fql, fdl))
    host = rank_hamming(sign, R)
    sign.close()
    m = MAPs(R, binarize=True)
    o = outs(("idx", "dist", "match", "hits"))
    assert m.rank_into(ns(fdb, fdl), ns(fq, fql), **o) == {"by": "hamming", "R": R}
    fill(o, host)
    arena.check("binarize")

    # shapes are judged before any GPU use; host memory is no destination
    arena.reset()
    good = arena.out((Q, R), "int64")
    for bad in (dict(idx=DeviceOut(good.ptr, (Q + 1, R), None, "int64")), dict(idx=DeviceOut(good.ptr, (Q, R + 1), None, "int64")),
                dict(ap=DeviceOut(good.ptr, (Q, 2), None, "float64")), dict(idx=np.empty((Q, R), np.int64)), dict()):
        with pytest.raises(ValueError):
            m.rank_into(ns(fdb, fdl), ns(fq, fql), **bad)
        with pytest.raises(ValueError):
            extra_metrics.rank_into(q, db, ql, dl, R, **bad)
    with pytest.raises(TypeError):
        extra_metrics.rank_into(q, db, ql, dl, R, index=good)
    assert arena.untouched()
    m.close()


def test_torch_tensors_on_the_current_stream():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    R, k = 130, 40
    q, db, ql, dl = CODES
    dev = torch.device("cuda")
    tq, tdb, tql, tdl = (torch.from_numpy(x).to(dev) for x in (q, db, ql, dl))
    idx = torch.empty((Q, k), dtype=torch.long, device=dev)
    match = torch.empty((Q, k), dtype=torch.bool, device=dev)
    ap = torch.empty((Q,), dtype=torch.float64, device=dev)
    hits = torch.empty((Q,), dtype=torch.int32, device=dev)
    m = MAPs(R)
    res = m.rank_into(ns(tdb, tdl), ns(tq, tql), idx=idx, match=match, ap=ap, hits=hits, stream=torch.cuda.current_stream().cuda_stream)
    assert res == {"by": "hamming", "R": R}
    m.close()
    gathered = (tdl[idx] * tql[:, None, :]).sum(-1) > 0         # the labels of the ranked rows, gathered on the GPU
    assert torch.equal(gathered, match)
    _, ap_host, rel_host = MAP_per_query(q, db, ql, dl, R)
    assert np.array_equal(ap.cpu().numpy().view(np.uint64)[1:], ap_host.view(np.uint64)[1:]) and np.isnan(ap.cpu().numpy()[0])
    assert np.array_equal(hits.cpu().numpy(), rel_host.astype(np.int32))
    ref = context(CODES)
    ref.topr(R)
    assert np.array_equal(idx.cpu().numpy(), ref.get_topr()[0][:, :k].astype(np.int64))
    ref.close()

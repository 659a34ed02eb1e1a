"""The table loaders' contract (hg_tables.hip; DESIGN.md, "The loaders' contract"; needs an MI355X): a refused load leaves the context
as it was, and after every pairing of a database loader with a query loader the float tables' residency and c->bpad are what the
real-valued entry points found before the loaders shared one commit per table.

The shape has an odd word count (b = 80: NW = 3, the strided upload) and two label words (C = 70)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.dev_arena import Arena
from hashgan_amd import _native, metric

pytestmark = pytest.mark.gpu

N, Q, b, Cn, R = 1000, 33, 80, 70, 100
M, K, DSUB = 10, 16, 8                                   # the quantised database: M * dsub = b
ARG, STATE = _native.HG_ERR_ARG, _native.HG_ERR_STATE
_ptr = _native._ptr


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(80)
    d = dict(x=np.tanh(rng.standard_normal((N, b))).astype(np.float32), qf=np.tanh(rng.standard_normal((Q, b))).astype(np.float32),
             dl=(rng.random((N, Cn)) < 0.05).astype(np.int64), ql=(rng.random((Q, Cn)) < 0.05).astype(np.int64),
             codes=rng.integers(0, K, (N, M)).astype(np.uint8), books=rng.standard_normal((M, K, DSUB)).astype(np.float32))
    for a in d.values():
        a.flags.writeable = False
    return d


@pytest.fixture(scope="module")
def arena():
    a = Arena(4 * (N + Q) * (b + 1) + 8 * (N + Q) * Cn + 4096)
    yield a
    a.close()


def _record(ctx):
    """What a refusal must leave byte for byte: hg_map's APs and hit counts, both packed tables, both censuses."""
    ap, rel = ctx.map(R)
    parts = [ap, rel, *ctx.get_packed(0), *ctx.get_packed(1), np.array(ctx.census(0), np.int64), np.array(ctx.census(1), np.int64)]
    return [p.tobytes() for p in parts]


def _host_desc(a, dtype):
    """hg_dev_array whose pointer is HOST memory."""
    return _native.DevArrayStruct(_ptr(a), a.shape[0], a.shape[1], a.shape[1], 1, dtype, None)


def _refusals(ctx, d, arena):
    """name -> a call that every loader must refuse with HG_ERR_ARG (raw C ABI: the Python wrappers would refuse some of these first)."""
    lib, h = ctx._lib, ctx._h
    dcodes, dlab = _native.pack_sign_f32(d["x"]), metric.pack_labels(d["dl"])
    qcodes, qlab = _native.pack_sign_f32(d["qf"]), metric.pack_labels(d["ql"])
    last_bad = d["codes"].copy()
    last_bad[N - 1, M - 1] = K
    wide_books = np.zeros((M, 257, DSUB), np.float32)
    fx, fl = _host_desc(d["x"], _native.HG_F32), _host_desc(d["dl"], _native.HG_I64)
    arena.reset()
    wide_q = _native._dev_struct(arena.put(np.zeros((Q, b + 1), np.float32), "float32"))
    dev_ql = _native._dev_struct(arena.put(d["ql"], "int64"))
    return {
        "set_database b=0": lambda: lib.hg_set_database(h, _ptr(dcodes), _ptr(dlab), N, 0, Cn, 0, N),
        "set_database_f32 n_total<N": lambda: lib.hg_set_database_f32(h, _ptr(d["x"]), _ptr(d["dl"]), N, b, Cn, 0, N - 1, None, None),
        "set_database_pq K=257": lambda: lib.hg_set_database_pq(h, _ptr(d["codes"]), _ptr(wide_books), _ptr(d["dl"]), N, M, 257, DSUB, Cn, 0, N,
                                                                  None, None),
        "set_database_pq byte=K in the last row": lambda: lib.hg_set_database_pq(h, _ptr(last_bad), _ptr(d["books"]), _ptr(d["dl"]), N, M, K,
                                                                                   DSUB, Cn, 0, N, None, None),
        "set_database_dev host pointer": lambda: lib.hg_set_database_dev(h, C.byref(fx), C.byref(fl), 0, N, None, None),
        "set_queries Q=0": lambda: lib.hg_set_queries(h, _ptr(qcodes), _ptr(qlab), 0),
        "set_queries_f32 null labels": lambda: lib.hg_set_queries_f32(h, _ptr(d["qf"]), None, Q, None, None),
        "set_queries_dev cols!=b": lambda: lib.hg_set_queries_dev(h, C.byref(wide_q), C.byref(dev_ql), None, None),
    }


def test_a_refused_load_changes_nothing(data, arena):
    ctx = _native.Context(0)
    try:
        ctx.set_database_f32(data["x"], data["dl"])
        ctx.set_queries_f32(data["qf"], data["ql"])
        before = _record(ctx)
        calls = _refusals(ctx, data, arena)
        assert len(calls) == 8
        for name, call in calls.items():
            assert call() == ARG, name
            assert _record(ctx) == before, name
    finally:
        ctx.close()


# ------------------------------------------------------------------ every pairing of a database loader with a query loader
# (option keep_floats / keep_query_floats, loader).  "f32 not up" under a database whose floats are resident cannot be reached: the
# queries' floats follow the database's.
DATABASES = ("packed", "f32_up", "f32_not_up", "pq", "dev")
QUERIES = ("packed", "f32_up", "f32_not_up", "dev")
CALLS = ("topr_rerank", "map_real", "map_asym")
# The parent commit's outcomes, recorded once on an MI355X (before the loaders moved into hg_tables.hip): per pairing and call, "STATE"
# or the first twelve hex digits of the SHA-1 of what the call returned; then whether the database's and the queries' floats are resident.
PARENT = {
    ('packed', 'packed'): ('STATE', 'STATE', 'STATE', False, False),
    ('packed', 'f32_up'): ('STATE', 'STATE', '6b8ec70182a3', False, True),
    ('packed', 'f32_not_up'): ('STATE', 'STATE', 'STATE', False, False),
    ('packed', 'dev'): ('STATE', 'STATE', '6b8ec70182a3', False, True),
    ('f32_up', 'packed'): ('STATE', 'STATE', 'STATE', True, False),
    ('f32_up', 'f32_up'): ('2132fb069cba', '439f93ed5818', '6b8ec70182a3', True, True),
    ('f32_up', 'f32_not_up'): ('2132fb069cba', '439f93ed5818', '6b8ec70182a3', True, True),
    ('f32_up', 'dev'): ('2132fb069cba', '439f93ed5818', '6b8ec70182a3', True, True),
    ('f32_not_up', 'packed'): ('STATE', 'STATE', 'STATE', False, False),
    ('f32_not_up', 'f32_up'): ('STATE', 'STATE', '6b8ec70182a3', False, True),
    ('f32_not_up', 'f32_not_up'): ('STATE', 'STATE', 'STATE', False, False),
    ('f32_not_up', 'dev'): ('STATE', 'STATE', '6b8ec70182a3', False, True),
    ('pq', 'packed'): ('STATE', 'STATE', 'STATE', False, False),
    ('pq', 'f32_up'): ('STATE', 'STATE', '1efe9e8562df', False, True),
    ('pq', 'f32_not_up'): ('STATE', 'STATE', 'STATE', False, False),
    ('pq', 'dev'): ('STATE', 'STATE', '1efe9e8562df', False, True),
    ('dev', 'packed'): ('STATE', 'STATE', 'STATE', True, False),
    ('dev', 'f32_up'): ('2132fb069cba', '439f93ed5818', '6b8ec70182a3', True, True),
    ('dev', 'f32_not_up'): ('2132fb069cba', '439f93ed5818', '6b8ec70182a3', True, True),
    ('dev', 'dev'): ('2132fb069cba', '439f93ed5818', '6b8ec70182a3', True, True),
}


def _load_database(ctx, kind, d, arena):
    ctx.set_option("keep_floats", {"f32_not_up": 0}.get(kind, 1))
    if kind == "packed":
        ctx.set_database(_native.pack_sign_f32(d["x"]), metric.pack_labels(d["dl"]), b, Cn)
    elif kind == "pq":
        ctx.set_database_pq(d["codes"], d["books"], d["dl"])
    elif kind == "dev":
        ctx.set_database_dev(arena.put(d["x"], "float32"), arena.put(d["dl"], "int64"))
    else:
        ctx.set_database_f32(d["x"], d["dl"])


def _load_queries(ctx, kind, d, arena):
    ctx.set_option("keep_query_floats", 0 if kind == "f32_not_up" else 1)
    if kind == "packed":
        ctx.set_queries(_native.pack_sign_f32(d["qf"]), metric.pack_labels(d["ql"]))
    elif kind == "dev":
        ctx.set_queries_dev(arena.put(d["qf"], "float32"), arena.put(d["ql"], "int64"))
    else:
        ctx.set_queries_f32(d["qf"], d["ql"])


def _outcome(ctx, call):
    try:
        out = getattr(ctx, call)(R)
    except _native.HashganNativeError as e:
        assert e.code == STATE, (call, str(e))
        return "STATE"
    sha = hashlib.sha1()
    for a in out:
        sha.update(np.ascontiguousarray(a).tobytes())
    return sha.hexdigest()[:12]


def pairing_outcomes(data, arena):
    """{(database, queries): (outcome of each of CALLS)} on ONE context, so that every load meets what the pairing before it left."""
    ctx = _native.Context(0)
    got = {}
    try:
        for dk in DATABASES:
            for qk in QUERIES:
                arena.reset()
                _load_database(ctx, dk, data, arena)
                _load_queries(ctx, qk, data, arena)
                got[dk, qk] = tuple(_outcome(ctx, call) for call in CALLS) + (ctx.census(0)[3], ctx.census(1)[3])
    finally:
        ctx.close()
    return got


def test_every_pairing_of_loaders_leaves_the_float_tables_as_before(data, arena):
    got = pairing_outcomes(data, arena)
    for key in got:
        print(repr(key) + ": " + repr(got[key]) + ",")                 # (the table, to be read where a pairing differs)
        assert got[key] == PARENT[key], key
    assert set(got) == set(PARENT)

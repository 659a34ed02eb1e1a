"""Asymmetric ranking on the GPU (hg_topr_asym / hg_map_asym, MAPs(asymmetric=True)): real-valued queries against the database's packed
codes read as +-1.  By definition bit for bit what the real-valued ranking returns on the float table where(code bit, +1, -1): every
comparison here is == / array_equal on bits, against oracle/real_map.py on that table and against hg_topr_real on a second context that
holds it."""
import functools
import types
import warnings

import numpy as np
import pytest

from oracle import real_map as RM
from hashgan_amd import _native, metric, MAPs
from hashgan_amd.devarray import DeviceArray, DeviceOut

pytestmark = pytest.mark.gpu

ARG, STATE = _native.HG_ERR_ARG, _native.HG_ERR_STATE
BET = (65, 70000, 64, 2500, 10)           # the bet: sample, filter, rescore from codes, LDS rank; two code words
SHAPES = [BET,
          (33, 70000, 33, 1200, 70),      # odd b: pad bits in the second word, two label words
          (16, 66000, 200, 1000, 5),      # more than 128 features: one query tile in the filter, the rescore's run-time word loop
          (12, 70000, 12, 3000, 4),       # ~17 copies of every code: tie groups across the cut, ordered by index
          (10, 2000, 128, 2000, 3),       # R = N, no cut
          (3, 500, 1, 40, 2),
          (9, 3000, 129, 500, 4),
          (5, 1000, 255, 1000, 3)]
# The smallest sizes at which real_ladder bets (N >= 65536, 8 R <= N): k_asym_image16 and k_asym_rescore on full words, one bit into a new
# word, and the rescore's run-time word loop at NW = 3, 4, 5 and 8 (one and two words are template instances)
FILTER_SHAPES = [(6, 65536, b, 640, 5) for b in (32, 65, 96, 128, 129, 255)]


@functools.lru_cache(maxsize=None)
def case(Q, N, b, R, C, kind="tanh"):
    """Features, labels, the +-1 table of the database's codes, and the oracle's ranking on it -- computed once, never modified."""
    rng = np.random.default_rng(Q * 7 + b)
    if kind == "sorted":
        # features that follow the class, rows stored class by class: a query's top rows crowd into a tenth of the slices
        cls, qcls = np.sort(rng.integers(0, C, N)), rng.integers(0, C, Q)
        proto = rng.standard_normal((C, b)).astype(np.float32)
        dbf = np.tanh(proto[cls] + 0.5 * rng.standard_normal((N, b))).astype(np.float32)
        qf = np.tanh(proto[qcls] + 0.5 * rng.standard_normal((Q, b))).astype(np.float32)
        dl, ql = np.eye(C, dtype=np.int8)[cls], np.eye(C, dtype=np.int8)[qcls]
    else:
        dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
        qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
        dl = (rng.random((N, C)) < 0.25).astype(np.int8)
        ql = (rng.random((Q, C)) < 0.25).astype(np.int8)
    dbf[rng.integers(0, N, 7), rng.integers(0, b, 7)] = 0.0          # exactly zero: a clear bit, read as -1
    dbf[N // 3] = dbf[N // 3 + 1]                                    # a duplicated row: exact tie, index order
    pm1 = np.where(dbf > 0, 1, -1).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, idx, score = RM.map_from_features(qf, pm1, ql, dl, R)
    match = (dl[idx].astype(bool) & ql[:, None, :].astype(bool)).any(-1)
    c = types.SimpleNamespace(Q=Q, N=N, b=b, R=R, C=C, dbf=dbf, qf=qf, dl=dl.astype(np.int64), ql=ql.astype(np.int64), pm1=pm1,
                              ap=ap, idx=idx, score=score, match=match.astype(np.uint8), rel=match.sum(1).astype(np.int64))
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def asym_context(c, Q=None):
    """A context with the database's codes only (keep_floats = 0) and the queries' floats (keep_query_floats = 1)."""
    ctx = _native.Context(0)
    ctx.set_option("keep_floats", 0)
    ctx.set_option("keep_query_floats", 1)
    assert ctx.set_database_f32(c.dbf, c.dl)[1] == 0
    assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
    return ctx


def real_context(c, Q=None):
    """The only way to this ranking without the feature: hg_topr_real on the +-1.0 float table."""
    ctx = _native.Context(0)
    ctx.set_option("keep_floats", 1)
    assert ctx.set_database_f32(c.pm1, c.dl)[1] == 0
    assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
    return ctx


def same_lists(got, c, Q=None, what=""):
    idx, score = got
    assert np.array_equal(score.view(np.uint32), c.score[:Q].view(np.uint32)), what
    assert np.array_equal(idx, c.idx[:Q]), what


def refused(code, fn, *args):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def no_real_lists(ctx):
    idx, score = np.empty((ctx.Q, 1), np.uint32), np.empty((ctx.Q, 1), np.float32)
    return ctx._lib.hg_get_topr_real(ctx._h, _native._ptr(idx), _native._ptr(score)) == STATE


class Producer:
    """Device memory without a framework: one scratch allocation of a context of its own, carved into 256-byte aligned pieces."""

    def __init__(self, nbytes):
        self.ctx = _native.Context(0)
        self.cap, self.top = int(nbytes), 0
        self.base = self.ctx.scratch(0, self.cap)

    def take(self, nbytes):
        off = self.top
        self.top = (off + int(nbytes) + 255) // 256 * 256
        assert self.top <= self.cap, "producer arena too small"
        return self.base + off

    def put(self, a, dtype):
        """A host array copied to the device -> DeviceArray."""
        a = np.ascontiguousarray(a)
        ptr = self.take(a.nbytes)
        self.ctx.memcpy_htod(ptr, a, a.nbytes)
        return DeviceArray(ptr, a.shape, None, dtype)

    def out(self, shape, dtype):
        """An uninitialised destination -> DeviceOut (contiguous)."""
        return DeviceOut(self.take(int(np.prod(shape)) * np.dtype(dtype).itemsize), shape, None, dtype)

    def get(self, d):
        """The contents of a DeviceArray / DeviceOut made here."""
        host = np.empty(d.shape, dtype=d.dtype)
        self.ctx.memcpy_dtoh(host, d.ptr, host.nbytes)
        return host

    def close(self):
        self.ctx.close()


# ------------------------------------------------------------------ 1. parity with the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lists_scores_ap_and_match_bits_equal_the_oracle(shape):
    c = case(*shape)
    ctx = asym_context(c)
    try:
        same_lists(ctx.topr_asym(c.R), c)
        path = ctx.get_stat("real_path")
        assert np.array_equal(ctx.get_match(), c.match)
        if shape in SHAPES[:3]:                                      # a bet without tie groups: filter + rescore ran, from the codes alone
            assert path & 1, "not the filter path"
            assert ctx.get_stat("asym_float_rows") == 0
            assert not ctx.census(0)[3], "database floats resident"
        ap, rel = ctx.map_asym(c.R)
        assert np.array_equal(ap, c.ap, equal_nan=True)
        assert np.array_equal(rel, c.rel)
        if shape in SHAPES[:3]:
            assert ctx.get_stat("real_path") & 1, "not the filter path"
            assert ctx.get_stat("asym_float_rows") == 0
        assert ctx.get_stat("asym_calls") == 2
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_word_count_at_filter_size_equals_the_oracle_from_the_codes_alone(shape):
    c = case(*shape)
    ctx = asym_context(c)
    try:
        same_lists(ctx.topr_asym(c.R), c)
        assert ctx.get_stat("real_path") & 1, "not the filter path"
        assert ctx.get_stat("asym_float_rows") == 0
        assert np.array_equal(ctx.get_match(), c.match)
        assert not ctx.census(0)[3], "database floats resident"
        ap, rel = ctx.map_asym(c.R)
        assert np.array_equal(ap, c.ap, equal_nan=True)
        assert np.array_equal(rel, c.rel)
        assert ctx.get_stat("real_path") & 1, "not the filter path"
        assert ctx.get_stat("asym_float_rows") == 0
        assert ctx.get_stat("asym_calls") == 2
        ctx.timing_enable(2)
        ctx.topr_asym(c.R, download=False)
        names = set(ctx.timing_read())
        ctx.timing_enable(0)
        assert "k_asym_rescore" in names and "k_real_rescore" not in names and "k_pq_rescore" not in names, names
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. differential on the GPU (+ 7. downstream)
@pytest.fixture(scope="module")
def pair():
    c = case(*BET)
    a, r = asym_context(c), real_context(c)
    yield c, a, r
    a.close()
    r.close()


def test_equals_the_real_valued_ranking_on_the_float_table(pair):
    c, a, r = pair
    idx_a, score_a = a.topr_asym(c.R)
    idx_r, score_r = r.topr_real(c.R)
    assert np.array_equal(idx_a, idx_r) and np.array_equal(score_a.view(np.uint32), score_r.view(np.uint32))
    assert a.get_stat("real_path") == r.get_stat("real_path")
    ap_a, rel_a = a.map_asym(c.R)
    ap_r, rel_r = r.map_real(c.R)
    assert np.array_equal(ap_a, ap_r, equal_nan=True) and np.array_equal(rel_a, rel_r)
    assert a.get_stat("device_bytes") < r.get_stat("device_bytes")


def test_downstream_of_the_lists_matches_the_real_valued_ranking(pair):
    c, a, r = pair
    ks = [10, 100, c.R]
    gain = np.arange(c.C + 1, dtype=np.float64) ** 2
    disc = 1.0 / np.log2(np.arange(2, c.R + 2, dtype=np.float64))
    prod = Producer(2 * (c.Q * c.R * 12 + c.Q * 66 + 8192) + 8192)
    res = []
    for ctx, rank in ((a, a.topr_asym), (r, r.topr_real)):
        rank(c.R, download=False)
        ctx.ap_at(ks)
        out = list(ctx.get_ap_at())
        ctx.votes(ks)
        out += [ctx.get_votes(), *ctx.get_vote_pred(), ctx.get_vote_confusion()]
        ctx.graded(ks, gain, disc)
        out += list(ctx.get_graded())
        ctx.match()
        ctx.ap()
        t = dict(idx=prod.out((c.Q, c.R), "int64"), score=prod.out((c.Q, c.R), "float32"), match=prod.out((c.Q, 50), "uint8"),
                 ap=prod.out((c.Q, 1), "float64"), hits=prod.out((c.Q, 1), "int64"))
        ctx.export(list(t.items()))
        ctx.synchronize()
        out += [prod.get(t[k]) for k in ("idx", "score", "match", "ap", "hits")]
        res.append(out)
    for x, y in zip(*res):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(res[0][-5], c.idx) and np.array_equal(res[0][-1][:, 0], c.rel)
    a.topr_asym(c.R, download=False)
    refused(STATE, a.export, [("dist", prod.out((c.Q, 4), "uint8"))])
    prod.close()


# ------------------------------------------------------------------ 3. every loader feeds it
def test_every_loader_feeds_it_with_identical_results():
    c = case(*BET)
    prod = Producer(c.dbf.nbytes + c.dl.nbytes + c.qf.nbytes + c.ql.nbytes + 4096)
    ddb, ddl = prod.put(c.dbf, "float32"), prod.put(c.dl, "int64")
    dq, dql = prod.put(c.qf, "float32"), prod.put(c.ql, "int64")
    loaders = {
        "packed": lambda x: x.set_database(metric.pack_codes(c.dbf), metric.pack_labels(c.dl), c.b, c.C),
        "f32 keep 0": lambda x: (x.set_option("keep_floats", 0), x.set_database_f32(c.dbf, c.dl)),
        "f32 keep 2": lambda x: (x.set_option("keep_floats", 2), x.set_database_f32(c.dbf, c.dl)),
        "dev": lambda x: (x.set_option("keep_floats", 0), x.set_database_dev(ddb, ddl)),
    }
    queries = {"f32": lambda x: x.set_queries_f32(c.qf, c.ql), "dev": lambda x: x.set_queries_dev(dq, dql)}
    try:
        for dname, load in loaders.items():
            for qname, loadq in queries.items():
                ctx = _native.Context(0)
                try:
                    ctx.set_option("keep_query_floats", 1)
                    load(ctx)
                    loadq(ctx)
                    same_lists(ctx.topr_asym(c.R), c, what=dname + " / " + qname)
                    ap, rel = ctx.map_asym(c.R)
                    assert np.array_equal(ap, c.ap, equal_nan=True) and np.array_equal(rel, c.rel), dname + " / " + qname
                    assert ctx.get_stat("asym_float_rows") == 0
                    assert ctx.census(0)[3] == (dname == "f32 keep 2")      # tanh features are no +-1 code: keep_floats = 2 kept them, unused
                finally:
                    ctx.close()
        # without the option, and with no database floats, the queries' floats are dropped: a state error that names the remedy
        ctx = _native.Context(0)
        try:
            ctx.set_option("keep_floats", 0)
            ctx.set_database_f32(c.dbf, c.dl)
            ctx.set_queries_f32(c.qf, c.ql)
            assert "keep_query_floats" in refused(STATE, ctx.map_asym, c.R)
            assert "keep_query_floats" in refused(STATE, ctx.topr_asym, c.R)
            assert no_real_lists(ctx)
            ctx.set_database(metric.pack_codes(c.dbf), metric.pack_labels(c.dl), c.b, c.C)
            ctx.set_queries(metric.pack_codes(c.qf), metric.pack_labels(c.ql))
            refused(STATE, ctx.topr_asym, c.R)
        finally:
            ctx.close()
    finally:
        prod.close()


# ------------------------------------------------------------------ 4. fallback
def test_without_the_filter_the_rows_are_expanded_into_a_work_buffer():
    c = case(*BET)
    Q = 12
    ctx = asym_context(c, Q)
    try:
        loaded = ctx.get_stat("device_bytes")
        rows = c.N * 64 * 4                                          # f32 [N][bpad]
        assert loaded < rows
        ctx.set_option("real_mfma", 0)
        same_lists(ctx.topr_asym(c.R), c, Q)
        assert ctx.get_stat("asym_float_rows") == 1
        assert ctx.get_stat("device_bytes") >= loaded + rows
        assert not ctx.census(0)[3], "a work buffer, not a loaded table"
        ctx.trim()
        assert ctx.get_stat("device_bytes") < rows
        assert no_real_lists(ctx)
        same_lists(ctx.topr_asym(c.R), c, Q, "after trim")           # expanded again
        ap, rel = ctx.map_asym(c.R)
        assert np.array_equal(ap, c.ap[:Q], equal_nan=True) and np.array_equal(rel, c.rel[:Q])
        ctx.set_option("real_mfma", 1)                               # the float32 MFMA passes: the same rows
        same_lists(ctx.topr_asym(c.R), c, Q, "real_mfma 1")
        assert ctx.get_stat("asym_float_rows") == 1
        ctx.set_option("real_mfma", 2)                               # and back: codes only
        same_lists(ctx.topr_asym(c.R), c, Q, "real_mfma 2")
        assert ctx.get_stat("asym_float_rows") == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. requery child
def test_class_sorted_database_where_queries_may_lose_the_first_bet():
    """Rows stored class by class, features that follow the class: a query's top rows crowd into few slices.  Observed on the MI355X:
    the requery child is not engaged (real_requeried stays 0: it takes at most a sixteenth of the queries, and more lose here); the
    ladder widens its slices instead -- three attempts, real_cap_boost 16 -- on the filter path, ranked in LDS, from the codes alone;
    the calls after it bet with the wide slices at once.  The oracle's lists throughout -- and the existing hg_topr_real agrees on the
    float table."""
    c = case(*BET, kind="sorted")
    a, r = asym_context(c), real_context(c)
    try:
        same_lists(r.topr_real(c.R), c, what="hg_topr_real")
        same_lists(a.topr_asym(c.R), c)
        assert a.get_stat("real_attempts") >= 2 and a.get_stat("real_cap_boost") > 1
        assert a.get_stat("real_path") & 1, "not the filter path"
        assert a.get_stat("asym_float_rows") == 0
        ap, rel = a.map_asym(c.R)
        assert np.array_equal(ap, c.ap, equal_nan=True) and np.array_equal(rel, c.rel)
        assert a.get_stat("real_attempts") == 1 and a.get_stat("real_cap_boost") > 1      # the widened slices are remembered
        assert a.get_stat("real_path") & 1 and a.get_stat("asym_float_rows") == 0
        same_lists(a.topr_asym(c.R), c, what="second call (escalated slices kept)")
        assert a.get_stat("real_attempts") == 1 and a.get_stat("real_path") & 1 and a.get_stat("asym_float_rows") == 0
    finally:
        a.close()
        r.close()


def test_both_row_sources_alternate_on_one_context_where_queries_may_lose_the_bet():
    """One context holds the tanh float table and its codes; real-valued and asymmetric calls alternate on it, through every
    real_mfma, without a reload -- on the class-sorted case, where the requery child may be engaged by either.  Each call finds what
    belongs to its own source: the oracle's bits, whatever the path.  The rows expanded from the codes stay a work buffer."""
    c = case(*BET, kind="sorted")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, apf, idxf, scoref = RM.map_from_features(c.qf, c.dbf, c.ql.astype(np.int8), c.dl.astype(np.int8), c.R)
    relf = (c.dl[idxf].astype(bool) & c.ql[:, None, :].astype(bool)).any(-1).sum(1).astype(np.int64)
    table = c.N * 64 * 4                                             # f32 [N][bpad]
    ctx = _native.Context(0)
    try:
        ctx.set_option("keep_floats", 1)
        ctx.set_database_f32(c.dbf, c.dl)
        ctx.set_queries_f32(c.qf, c.ql)

        def real_lists(what):
            idx, score = ctx.topr_real(c.R)
            assert np.array_equal(idx, idxf) and np.array_equal(score.view(np.uint32), scoref.view(np.uint32)), what

        before_rows = None
        for mfma in (2, 1, 0):
            what = "real_mfma %d" % mfma
            ctx.set_option("real_mfma", mfma)
            real_lists(what)
            if mfma < 2 and before_rows is None:
                before_rows = ctx.get_stat("device_bytes")
            same_lists(ctx.topr_asym(c.R), c, what=what)
            ap, rel = ctx.map_real(c.R)
            assert np.array_equal(ap, apf, equal_nan=True) and np.array_equal(rel, relf), what
            ap, rel = ctx.map_asym(c.R)
            assert np.array_equal(ap, c.ap, equal_nan=True) and np.array_equal(rel, c.rel), what
            real_lists(what + ", after the asymmetric calls")
        ctx.trim()
        assert ctx.get_stat("device_bytes") < before_rows + table
        assert ctx.census(0)[3], "the float table is a loaded table: hg_trim keeps it"
        real_lists("after trim")
        same_lists(ctx.topr_asym(c.R), c, what="after trim")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. state
def test_a_hamming_ranking_ends_the_real_lists_and_the_other_way_round():
    c = case(40, 3000, 20, 700, 7)
    ctx = asym_context(c)
    try:
        same_lists(ctx.topr_asym(c.R), c)
        ctx.topr(c.R)
        assert no_real_lists(ctx)
        ctx.get_topr()
        ctx.topr_asym(c.R, download=False)
        refused(STATE, ctx.get_topr)
        idx, score = np.empty((c.Q, c.R), np.uint32), np.empty((c.Q, c.R), np.float32)
        _native.check(ctx._lib.hg_get_topr_real(ctx._h, _native._ptr(idx), _native._ptr(score)))
        same_lists((idx, score), c)
        # refused calls leave no lists
        refused(ARG, ctx.topr_asym, 0)
        assert no_real_lists(ctx)
        same_lists(ctx.topr_asym(c.R), c)
        refused(ARG, ctx.topr_asym, c.N + 1)
        assert no_real_lists(ctx)
        refused(ARG, ctx.map_asym, 0)
        refused(ARG, ctx.map_asym, c.N + 1)
        # a shard of a larger database
        ctx.set_database_f32(c.dbf, c.dl, 0, c.N + 5)
        ctx.set_queries_f32(c.qf, c.ql)
        assert "single-shard" in refused(STATE, ctx.topr_asym, c.R)
        refused(STATE, ctx.map_asym, c.R)
        assert no_real_lists(ctx)
    finally:
        ctx.close()


def test_a_database_reload_rebuilds_what_was_derived_from_the_codes():
    """Different codes, the same N and b, on one context: the results follow the new codes -- on the bet (the 16-bit image) and on
    the fallback (the expanded rows)."""
    c = case(*BET)
    Q = 12
    other = np.ascontiguousarray(c.dbf[::-1])
    ol = np.ascontiguousarray(c.dl[::-1])
    pm1 = np.where(other > 0, 1, -1).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap2, idx2, score2 = RM.map_from_features(c.qf[:Q], pm1, c.ql[:Q].astype(np.int8), ol.astype(np.int8), c.R)
    assert not np.array_equal(idx2, c.idx[:Q])
    ctx = asym_context(c, Q)
    try:
        for mfma in (2, 0):
            ctx.set_option("real_mfma", mfma)
            ctx.set_database_f32(c.dbf, c.dl)
            ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])
            same_lists(ctx.topr_asym(c.R), c, Q, "first database, real_mfma %d" % mfma)
            ctx.set_database_f32(other, ol)
            ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])
            idx, score = ctx.topr_asym(c.R)
            assert np.array_equal(idx, idx2) and np.array_equal(score.view(np.uint32), score2.view(np.uint32)), mfma
            ap, _ = ctx.map_asym(c.R)
            assert np.array_equal(ap, ap2, equal_nan=True), mfma
    finally:
        ctx.close()


def test_real_valued_ranking_on_a_float_table_is_unchanged_around_an_asymmetric_call():
    """hg_map_real on tanh features (no +-1 table), before and after asymmetric calls on another context and on the SAME context
    (which then holds both a float table and its codes): its own image and lists, untouched."""
    c = case(*BET)
    Q = 12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, apf, idxf, scoref = RM.map_from_features(c.qf[:Q], c.dbf, c.ql[:Q].astype(np.int8), c.dl.astype(np.int8), c.R)
    r = _native.Context(0)
    a = asym_context(c, Q)
    try:
        r.set_option("keep_floats", 1)
        r.set_database_f32(c.dbf, c.dl)
        r.set_queries_f32(c.qf[:Q], c.ql[:Q])

        def real_ok(what):
            idx, score = r.topr_real(c.R)
            assert np.array_equal(idx, idxf) and np.array_equal(score.view(np.uint32), scoref.view(np.uint32)), what
            ap, _ = r.map_real(c.R)
            assert np.array_equal(ap, apf, equal_nan=True), what

        real_ok("before")
        same_lists(a.topr_asym(c.R), c, Q)
        real_ok("after an asymmetric call on another context")
        same_lists(r.topr_asym(c.R), c, Q, "asymmetric on the float-table context")
        assert r.get_stat("asym_float_rows") == 0
        real_ok("after an asymmetric call on the same context")
        same_lists(r.topr_asym(c.R), c, Q, "and again")
    finally:
        a.close()
        r.close()


def test_keep_query_floats_is_an_option_of_the_table():
    """Accepted at 0 (the default) and 1, refused beyond either end; at 0 the query floats follow the database's, as before the option."""
    c = case(40, 3000, 20, 700, 7)
    ctx = _native.Context(0)
    try:
        for v in (0, 1, 0):
            ctx.set_option("keep_query_floats", v)
        for v in (-1, 2):
            refused(ARG, ctx.set_option, "keep_query_floats", v)
        ctx.set_option("keep_floats", 0)
        ctx.set_database_f32(c.dbf, c.dl)
        ctx.set_queries_f32(c.qf, c.ql)
        assert not ctx.census(1)[3], "query floats kept without the option and without the database's"
        ctx.set_option("keep_query_floats", 1)
        ctx.set_queries_f32(c.qf, c.ql)
        assert ctx.census(1)[3] and not ctx.census(0)[3]
        same_lists(ctx.topr_asym(c.R), c)
        ctx.set_option("keep_floats", 1)                             # the database's floats resident: the queries' follow, option or not
        ctx.set_option("keep_query_floats", 0)
        ctx.set_database_f32(c.dbf, c.dl)
        ctx.set_queries_f32(c.qf, c.ql)
        assert ctx.census(1)[3] and ctx.census(0)[3]
        same_lists(ctx.topr_asym(c.R), c)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. Python surface
@pytest.mark.parametrize("where", ["host", "device"])
def test_maps_asymmetric(where):
    c = case(40, 3000, 20, 700, 7)
    Rs = [10, 100, c.R]
    ql8, dl8 = c.ql.astype(np.int8), c.dl.astype(np.int8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        at = [RM.map_from_features(c.qf, c.pm1, ql8, dl8, k)[1:3] for k in Rs]
    per_k = []
    for ap_k, idx_k in at:
        rel_k = (dl8[idx_k].astype(bool) & ql8[:, None, :].astype(bool)).any(-1).sum(1)
        per_k.append(metric.mean_over_hits(ap_k, rel_k.astype(np.int64)))
    prod = Producer(c.dbf.nbytes + c.dl.nbytes + c.qf.nbytes + c.ql.nbytes + c.Q * c.R * 22 + c.Q * 16 + 16384)
    if where == "device":
        db = types.SimpleNamespace(output=prod.put(c.dbf, "float32"), label=prod.put(c.dl, "int64"))
        q = types.SimpleNamespace(output=prod.put(c.qf, "float32"), label=prod.put(c.ql, "int64"))
    else:
        db, q = types.SimpleNamespace(output=c.dbf, label=c.dl), types.SimpleNamespace(output=c.qf, label=c.ql)
    with pytest.raises(ValueError):
        MAPs(c.R, asymmetric=True, rerank=True)
    with pytest.raises(ValueError):
        MAPs(c.R, asymmetric=True, binarize=True)
    m = MAPs(c.R, asymmetric=True)
    try:
        assert m.get_maps_by_feature(db, q) == metric.mean_over_hits(c.ap, c.rel)
        assert not m._eng.ctx.census(0)[3], "the database's floats went to the GPU"
        assert m._eng.ctx.get_stat("asym_calls") >= 1
        assert np.array_equal(m.get_maps_at(db, q, Rs), np.array(per_k))
        knn = m.get_knn_at(db, q, [1, 10])
        assert set(knn) and m._eng.ctx.get_stat("votes_cutoffs") == 2
        idx, score, ap = prod.out((c.Q, c.R), "int64"), prod.out((c.Q, c.R), "float32"), prod.out((c.Q, 1), "float64")
        match, hits = prod.out((c.Q, c.R), "uint8"), prod.out((c.Q, 1), "int64")
        assert m.rank_into(db, q, idx=idx, score=score, ap=ap, match=match, hits=hits) == {"by": "inner_product", "R": c.R}
        m._eng.ctx.synchronize()
        assert np.array_equal(prod.get(idx), c.idx)
        assert np.array_equal(prod.get(score).view(np.uint32), c.score.view(np.uint32))
        assert np.array_equal(prod.get(ap)[:, 0], c.ap, equal_nan=True)
        assert np.array_equal(prod.get(match), c.match) and np.array_equal(prod.get(hits)[:, 0], c.rel)
        with pytest.raises(ValueError, match="inner-product"):
            m.rank_into(db, q, dist=prod.out((c.Q, c.R), "uint8"))
        # the resident database is reused (None: the copy the last load left)
        assert m.get_maps_by_feature(None, q) == metric.mean_over_hits(c.ap, c.rel)
    finally:
        m.close()
    # the pooled context goes back to the other modes: the reference routing on the same arrays still ranks by the features
    ref = MAPs(c.R)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, apf, idxf, _ = RM.map_from_features(c.qf, c.dbf, ql8, dl8, c.R)
        relf = (dl8[idxf].astype(bool) & ql8[:, None, :].astype(bool)).any(-1).sum(1).astype(np.int64)
        assert ref.get_maps_by_feature(db, q) == metric.mean_over_hits(apf, relf)
    finally:
        ref.close()
        prod.close()

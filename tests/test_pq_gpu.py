"""Quantised databases on the GPU (hg_set_database_pq, hg_topr_pq / hg_map_pq, MAPs(quantised=True)): real-valued queries against
product-quantisation codes.  A PQ row decodes by pure gather, so the ranking is by definition bit for bit what the real-valued ranking
returns on the decoded table: every comparison here is == / array_equal on bits, against oracle/real_map.py on pq.decode(codes,
codebooks) and against hg_topr_real on a second context that holds that table."""
import functools
import gc
import types
import warnings

import numpy as np
import pytest

from oracle import real_map as RM
from tests import brute_refs
from hashgan_amd import _native, metric, pq, MAPs, pool_stats, release_engines
from hashgan_amd.devarray import DeviceOut

pytestmark = pytest.mark.gpu

ARG, STATE = _native.HG_ERR_ARG, _native.HG_ERR_STATE
#        Q, N, M, dsub, K, R, C
BET = (65, 70000, 8, 8, 256, 2500, 10)            # the bet: sample, filter, rescore from the codes (64 KB of codebooks, 16-byte reads), LDS rank
TIES = (12, 70000, 2, 6, 4, 3000, 4)              # 16 distinct rows: tie groups thousands long across the cut, index order
SMALL = (40, 3000, 4, 5, 16, 700, 7)
SHAPES = [BET,
          (33, 70000, 3, 11, 16, 1200, 70),       # odd b = 33, two label words, MP padding, one feature per codebook read
          (16, 66000, 8, 25, 256, 1000, 5),       # b = 200: over 128 features, 200 KB of codebooks, dsub = 25: one feature per read; sampled_rows
          TIES,
          (10, 2000, 16, 8, 64, 2000, 3),         # R = N: no cut, expanded rows, pq_float_rows = 1
          (3, 500, 1, 1, 2, 40, 2),
          (5, 1000, 5, 51, 256, 1000, 3)]         # b = 255


oracle = brute_refs.real_lists                            # (shared with tests/test_second_hand_gpu.py)


@functools.lru_cache(maxsize=None)
def case(Q, N, M, dsub, K, R, C):
    """tanh features; codebooks = K rows drawn per subspace from the database's own features, one codeword holding an exact 0.0 and one a
    -0.0; codes = encode; one database row duplicated; the decoded table and the oracle's ranking on it -- computed once, never modified."""
    rng = np.random.default_rng(Q * 7 + M * dsub)
    b = M * dsub
    dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
    dl = (rng.random((N, C)) < 0.25).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.25).astype(np.int64)
    books = np.stack([dbf[rng.choice(N, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    books[0, 0, 0] = 0.0
    books[M - 1, K - 1, dsub - 1] = -0.0
    codes = pq.encode(dbf, books)
    codes[N // 3] = codes[N // 3 + 1]                                # a duplicated row: exact tie, index order
    x = pq.decode(codes, books)
    ap, idx, score, match, rel = oracle(qf, x, ql, dl, R)
    c = types.SimpleNamespace(Q=Q, N=N, M=M, dsub=dsub, K=K, b=b, R=R, C=C, qf=qf, ql=ql, dl=dl, books=books, codes=codes, x=x,
                              ap=ap, idx=idx, score=score, match=match, rel=rel)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def pq_context(c, Q=None):
    """A context with the database's PQ tables and the queries' floats (keep_query_floats = 1)."""
    ctx = _native.Context(0)
    ctx.set_option("keep_query_floats", 1)
    assert ctx.set_database_pq(c.codes, c.books, c.dl)[1] == 0
    assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
    return ctx


def real_context(c, Q=None):
    """The only way to this ranking without the feature: hg_topr_real on the decoded float table."""
    ctx = _native.Context(0)
    ctx.set_option("keep_floats", 1)
    assert ctx.set_database_f32(c.x, c.dl)[1] == 0
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


class Arena:
    """Device memory without a framework: one scratch allocation of a context of its own, carved into 256-byte aligned destinations."""

    def __init__(self, nbytes):
        self.ctx = _native.Context(0)
        self.cap, self.top = int(nbytes), 0
        self.base = self.ctx.scratch(0, self.cap)

    def out(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        off = self.top
        self.top = (off + nbytes + 255) // 256 * 256
        assert self.top <= self.cap, "arena too small"
        return DeviceOut(self.base + off, shape, None, dtype)

    def get(self, d):
        host = np.empty(d.shape, dtype=d.dtype)
        self.ctx.memcpy_dtoh(host, d.ptr, host.nbytes)
        return host

    def close(self):
        self.ctx.close()


# ------------------------------------------------------------------ the cases themselves (host arithmetic only)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_case_has_hits_and_the_tie_shape_has_a_group_across_the_cut(shape):
    c = case(*shape)
    assert (c.rel > 0).any(), "no query with a hit"
    assert np.array_equal(c.x[c.N // 3], c.x[c.N // 3 + 1])
    assert (c.x.view(np.uint32) == 0x80000000).any() or c.K * c.M <= 2, "the -0.0 codeword does not occur"
    if shape == TIES:
        assert len(np.unique(c.x, axis=0)) <= 16
        ap, idx, score, _, _ = oracle(c.qf[:1], c.x, c.ql[:1], c.dl, c.R + 1)
        assert score.view(np.uint32)[0, c.R] == score.view(np.uint32)[0, c.R - 1], "no tie group crosses R"


# ------------------------------------------------------------------ 1. parity with the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lists_scores_ap_and_match_bits_equal_the_oracle(shape):
    c = case(*shape)
    ctx = pq_context(c)
    try:
        loaded = ctx.get_stat("device_bytes")
        same_lists(ctx.topr_pq(c.R), c)
        assert np.array_equal(ctx.get_match(), c.match)
        assert not ctx.census(0)[3], "database floats resident"
        if shape in SHAPES[:4]:                                      # the bet: filter + rescore from the codes and codebooks alone
            assert ctx.get_stat("real_path") & 1
            assert ctx.get_stat("pq_float_rows") == 0
        if shape == SHAPES[4]:                                       # no cut on <= 128 features: the float32 MFMA pass on decoded rows
            assert ctx.get_stat("pq_float_rows") == 1
            assert ctx.get_stat("device_bytes") >= loaded + c.N * c.b * 4
        ap, rel = ctx.map_pq(c.R)
        assert np.array_equal(ap, c.ap, equal_nan=True)
        assert np.array_equal(rel, c.rel)
        assert ctx.get_stat("pq_calls") == 2
        if shape == BET:
            ctx.timing_enable(2)
            ctx.topr_pq(c.R, download=False)
            names = set(ctx.timing_read())
            ctx.timing_enable(0)
            assert "k_pq_rescore" in names and "k_real_rescore" not in names and "k_asym_rescore" not in names
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. differential on the GPU
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_real_valued_ranking_on_the_decoded_table(shape):
    c = case(*shape)
    a, r = pq_context(c), real_context(c)
    try:
        idx_a, score_a = a.topr_pq(c.R)
        idx_r, score_r = r.topr_real(c.R)
        assert np.array_equal(idx_a, idx_r) and np.array_equal(score_a.view(np.uint32), score_r.view(np.uint32))
        assert a.get_stat("real_path") == r.get_stat("real_path")
        assert a.get_stat("real_attempts") == r.get_stat("real_attempts")
        if shape == BET:
            assert a.get_stat("pq_float_rows") == 0
            assert not a.census(0)[3] and r.census(0)[3]
            assert a.get_stat("device_bytes") < r.get_stat("device_bytes")
            ap_a, rel_a = a.map_pq(c.R)
            ap_r, rel_r = r.map_real(c.R)
            assert np.array_equal(ap_a, ap_r, equal_nan=True) and np.array_equal(rel_a, rel_r)
    finally:
        a.close()
        r.close()


# ------------------------------------------------------------------ 3. the Hamming side of a PQ-loaded context
def test_hamming_ranking_on_a_pq_loaded_context_is_that_of_its_sign_codes():
    c = case(*SMALL)
    a, h = pq_context(c), _native.Context(0)
    try:
        h.set_database(pq.sign_codes(c.codes, c.books), metric.pack_labels(c.dl), c.b, c.C)
        h.set_queries(metric.pack_codes(c.qf), metric.pack_labels(c.ql))
        a.topr(c.R)
        h.topr(c.R)
        (idx_a, dist_a), (idx_h, dist_h) = a.get_topr(), h.get_topr()
        assert np.array_equal(idx_a, idx_h) and np.array_equal(dist_a, dist_h)
        ap_a, rel_a = a.map(c.R)
        ap_h, rel_h = h.map(c.R)
        assert np.array_equal(ap_a, ap_h, equal_nan=True) and np.array_equal(rel_a, rel_h)
        got_codes, got_labels = a.get_packed(0)
        assert np.array_equal(got_codes, pq.sign_codes(c.codes, c.books).view(np.uint32)[:, :got_codes.shape[1]])
        assert np.array_equal(got_labels, metric.pack_labels(c.dl))
        # the census of the decoded table, without the table: what hg_set_database_f32 reports for it
        f = _native.Context(0)
        try:
            f.set_option("keep_floats", 0)
            f.set_database_f32(c.x, c.dl)
            assert a.census(0) == f.census(0)
        finally:
            f.close()
    finally:
        a.close()
        h.close()


# ------------------------------------------------------------------ 4. downstream calls
def test_downstream_of_the_lists_matches_the_real_valued_ranking():
    c = case(*SMALL)
    a, r = pq_context(c), real_context(c)
    ks = [10, 100, c.R]
    gain = np.arange(c.C + 1, dtype=np.float64) ** 2
    disc = 1.0 / np.log2(np.arange(2, c.R + 2, dtype=np.float64))
    arena = Arena(2 * (c.Q * c.R * 12 + c.Q * 66 + 8192) + 8192)
    try:
        res = []
        for ctx, rank in ((a, a.topr_pq), (r, r.topr_real)):
            rank(c.R, download=False)
            ctx.ap_at(ks)
            out = list(ctx.get_ap_at())
            ctx.votes(ks)
            out += [ctx.get_votes(), *ctx.get_vote_pred(), ctx.get_vote_confusion()]
            ctx.graded(ks, gain, disc)
            out += list(ctx.get_graded())
            ctx.match()
            ctx.ap()
            t = dict(idx=arena.out((c.Q, c.R), "int64"), score=arena.out((c.Q, c.R), "float32"), match=arena.out((c.Q, 50), "uint8"),
                     ap=arena.out((c.Q, 1), "float64"), hits=arena.out((c.Q, 1), "int64"))
            ctx.export(list(t.items()))
            ctx.synchronize()
            out += [arena.get(t[k]) for k in ("idx", "score", "match", "ap", "hits")]
            res.append(out)
        for x, y in zip(*res):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.array_equal(res[0][-5], c.idx) and np.array_equal(res[0][-1][:, 0], c.rel)
        a.topr_pq(c.R, download=False)
        refused(STATE, a.export, [("dist", arena.out((c.Q, 4), "uint8"))])
    finally:
        arena.close()
        a.close()
        r.close()


# ------------------------------------------------------------------ 5. state and arguments
def test_calls_without_their_tables_are_state_errors_that_name_the_remedy():
    c = case(*SMALL)
    ctx = _native.Context(0)
    try:
        # no PQ tables: a float database
        ctx.set_option("keep_floats", 0)
        ctx.set_option("keep_query_floats", 1)
        ctx.set_database_f32(c.x, c.dl)
        ctx.set_queries_f32(c.qf, c.ql)
        assert "hg_set_database_pq" in refused(STATE, ctx.topr_pq, c.R)
        assert "hg_set_database_pq" in refused(STATE, ctx.map_pq, c.R)
        assert no_real_lists(ctx)
        # PQ tables, but the queries' floats were not kept
        ctx.set_option("keep_query_floats", 0)
        ctx.set_database_pq(c.codes, c.books, c.dl)
        refused(STATE, ctx.topr_pq, c.R)                             # (no queries at all yet)
        ctx.set_queries_f32(c.qf, c.ql)
        assert "keep_query_floats" in refused(STATE, ctx.topr_pq, c.R)
        assert "keep_query_floats" in refused(STATE, ctx.map_pq, c.R)
        assert no_real_lists(ctx)
        ctx.set_option("keep_query_floats", 1)
        ctx.set_queries_f32(c.qf, c.ql)
        same_lists(ctx.topr_pq(c.R), c)
        # a refused call leaves no real lists
        refused(ARG, ctx.topr_pq, 0)
        assert no_real_lists(ctx)
        same_lists(ctx.topr_pq(c.R), c)
        refused(ARG, ctx.map_pq, c.N + 1)
        assert no_real_lists(ctx)
        # any other loader forgets the PQ tables
        for load in (lambda: ctx.set_database_f32(c.x, c.dl),
                     lambda: ctx.set_database(pq.sign_codes(c.codes, c.books), metric.pack_labels(c.dl), c.b, c.C)):
            ctx.set_database_pq(c.codes, c.books, c.dl)
            ctx.set_queries_f32(c.qf, c.ql)
            same_lists(ctx.topr_pq(c.R), c)
            load()
            ctx.set_queries_f32(c.qf, c.ql)
            assert "hg_set_database_pq" in refused(STATE, ctx.topr_pq, c.R)
            assert no_real_lists(ctx)
    finally:
        ctx.close()


def test_the_loader_refuses_what_it_cannot_rank_and_names_the_offender():
    c = case(*SMALL)
    ctx = pq_context(c)
    lib, h = ctx._lib, ctx._h

    def load(codes, books, M=None, K=None, dsub=None, idx_base=0, n_total=None):
        codes, books = np.ascontiguousarray(codes), np.ascontiguousarray(books)
        N = codes.shape[0]
        M, K, dsub = (v if v is not None else books.shape[i] for i, v in enumerate((M, K, dsub)))
        return lib.hg_set_database_pq(h, _native._ptr(codes), _native._ptr(books), _native._ptr(c.dl), N, M, K, dsub, c.C, idx_base,
                                      N if n_total is None else n_total, None, None)

    def said():
        return lib.hg_last_error().decode()

    try:
        same_lists(ctx.topr_pq(c.R), c)
        bad = c.codes.copy()
        bad[1234, 2] = c.K
        assert load(bad, c.books) == ARG
        assert "1234" in said() and "subspace 2" in said()
        for v in (np.nan, np.inf, -np.inf):
            books = c.books.copy()
            books[3, 5, 1] = v
            assert load(c.codes, books) == ARG
            assert "[3][5][1]" in said()
        assert load(np.zeros((10, 1), np.uint8), np.zeros((1, 257, 1), np.float32)) == ARG and "K=257" in said()
        assert load(np.zeros((10, 16), np.uint8), np.zeros((16, 2, 16), np.float32)) == ARG and "256" in said()
        assert load(c.codes, c.books, M=0) == ARG
        assert load(c.codes, c.books, K=0) == ARG
        assert load(c.codes, c.books, dsub=0) == ARG
        assert load(c.codes, c.books, idx_base=1, n_total=c.N + 1) == ARG and "shard" in said()
        assert load(c.codes, c.books, n_total=c.N + 5) == ARG
        # every refusal came before the context was touched: the loaded database still ranks
        same_lists(ctx.topr_pq(c.R), c)
    finally:
        ctx.close()


def test_trim_and_reload_rebuild_what_was_derived_from_the_tables():
    c = case(*BET)
    Q = 12
    ctx = pq_context(c, Q)
    try:
        same_lists(ctx.topr_pq(c.R), c, Q)
        tables = ctx.get_stat("device_bytes")
        ctx.trim()
        assert ctx.get_stat("device_bytes") < tables and ctx.get_stat("device_bytes") >= c.N * c.M + c.books.nbytes
        assert no_real_lists(ctx)
        same_lists(ctx.topr_pq(c.R), c, Q, "after trim")
        # without the filter the rows are decoded into a work buffer, which hg_trim frees
        ctx.set_option("real_mfma", 0)
        same_lists(ctx.topr_pq(c.R), c, Q, "real_mfma 0")
        assert ctx.get_stat("pq_float_rows") == 1 and not ctx.census(0)[3]
        assert ctx.get_stat("device_bytes") >= c.N * 64 * 4
        ctx.set_option("real_mfma", 1)
        same_lists(ctx.topr_pq(c.R), c, Q, "real_mfma 1")
        ctx.trim()
        assert ctx.get_stat("device_bytes") < c.N * 64 * 4
        ctx.set_option("real_mfma", 2)
        same_lists(ctx.topr_pq(c.R), c, Q, "real_mfma 2 after trim")
        assert ctx.get_stat("pq_float_rows") == 0
        # other codes, the same shape, on the same context: the results follow the new tables
        other = np.ascontiguousarray(c.codes[::-1])
        ol = np.ascontiguousarray(c.dl[::-1])
        ap2, idx2, score2, _, _ = oracle(c.qf[:Q], pq.decode(other, c.books), c.ql[:Q], ol, c.R)
        assert not np.array_equal(idx2, c.idx[:Q])
        ctx.set_database_pq(other, c.books, ol)
        ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])
        idx, score = ctx.topr_pq(c.R)
        assert np.array_equal(idx, idx2) and np.array_equal(score.view(np.uint32), score2.view(np.uint32))
        ap, _ = ctx.map_pq(c.R)
        assert np.array_equal(ap, ap2, equal_nan=True)
    finally:
        ctx.close()


def test_the_other_real_valued_rankings_are_unchanged_around_a_quantised_call():
    """hg_map_real on the decoded table and hg_map_asym on its signs, on contexts of their own, before and after quantised calls."""
    c = case(*BET)
    Q = 12
    pm1 = np.where(c.x > 0, 1, -1).astype(np.float32)
    ap_s, idx_s, score_s, _, rel_s = oracle(c.qf[:Q], pm1, c.ql[:Q], c.dl, c.R)
    r, s, a = real_context(c, Q), _native.Context(0), pq_context(c, Q)
    try:
        s.set_option("keep_floats", 0)
        s.set_option("keep_query_floats", 1)
        s.set_database_f32(c.x, c.dl)
        s.set_queries_f32(c.qf[:Q], c.ql[:Q])

        def others_ok(what):
            same_lists(r.topr_real(c.R), c, Q, what)
            ap, rel = r.map_real(c.R)
            assert np.array_equal(ap, c.ap[:Q], equal_nan=True) and np.array_equal(rel, c.rel[:Q]), what
            idx, score = s.topr_asym(c.R)
            assert np.array_equal(idx, idx_s) and np.array_equal(score.view(np.uint32), score_s.view(np.uint32)), what
            ap, rel = s.map_asym(c.R)
            assert np.array_equal(ap, ap_s, equal_nan=True) and np.array_equal(rel, rel_s), what

        others_ok("before")
        same_lists(a.topr_pq(c.R), c, Q)
        ap, rel = a.map_pq(c.R)
        assert np.array_equal(ap, c.ap[:Q], equal_nan=True) and np.array_equal(rel, c.rel[:Q])
        others_ok("after")
        # ... and the asymmetric call on the PQ-loaded context itself reads its sign codes
        idx, score = a.topr_asym(c.R)
        assert np.array_equal(idx, idx_s) and np.array_equal(score.view(np.uint32), score_s.view(np.uint32))
        same_lists(a.topr_pq(c.R), c, Q, "after an asymmetric call on the same context")
    finally:
        r.close()
        s.close()
        a.close()


# ------------------------------------------------------------------ 6. Python surface
def test_maps_quantised():
    c = case(*SMALL)
    Rs = [10, 100, c.R]
    per_k = []
    for k in Rs:
        ap_k, _, _, _, rel_k = oracle(c.qf, c.x, c.ql, c.dl, k)
        per_k.append(metric.mean_over_hits(ap_k, rel_k))
    db = types.SimpleNamespace(codes=c.codes, codebooks=c.books, label=c.dl)
    q = types.SimpleNamespace(output=c.qf, label=c.ql)
    arena = Arena(c.Q * c.R * 22 + c.Q * 16 + 16384)
    m = MAPs(c.R, quantised=True)
    try:
        assert m.get_maps_by_feature(db, q) == metric.mean_over_hits(c.ap, c.rel)
        assert not m._eng.ctx.census(0)[3], "a float table of the database went to the GPU"
        assert m._eng.ctx.get_stat("pq_calls") >= 1
        assert np.array_equal(m.get_maps_at(db, q, Rs), np.array(per_k))
        knn = m.get_knn_at(db, q, [1, 10])
        assert set(knn) and m._eng.ctx.get_stat("votes_cutoffs") == 2
        idx, score, ap = arena.out((c.Q, c.R), "int64"), arena.out((c.Q, c.R), "float32"), arena.out((c.Q, 1), "float64")
        match, hits = arena.out((c.Q, c.R), "uint8"), arena.out((c.Q, 1), "int64")
        assert m.rank_into(db, q, idx=idx, score=score, ap=ap, match=match, hits=hits) == {"by": "inner_product", "R": c.R}
        m._eng.ctx.synchronize()
        assert np.array_equal(arena.get(idx), c.idx)
        assert np.array_equal(arena.get(score).view(np.uint32), c.score.view(np.uint32))
        assert np.array_equal(arena.get(ap)[:, 0], c.ap, equal_nan=True)
        assert np.array_equal(arena.get(match), c.match) and np.array_equal(arena.get(hits)[:, 0], c.rel)
        with pytest.raises(ValueError, match="inner-product"):
            m.rank_into(db, q, dist=arena.out((c.Q, c.R), "uint8"))
        assert m.get_maps_by_feature(None, q) == metric.mean_over_hits(c.ap, c.rel)      # the resident copy
        # SQD: a query given as codes is the query's decoded codes
        qcodes = pq.encode(c.qf, c.books)
        sq = types.SimpleNamespace(codes=qcodes, label=c.ql)
        aq = types.SimpleNamespace(output=pq.decode(qcodes, c.books), label=c.ql)
        sqd = m.get_maps_by_feature(db, sq)
        assert sqd == m.get_maps_by_feature(db, aq) and sqd == m.get_maps_by_feature(None, sq)
        ap_q, _, _, _, rel_q = oracle(aq.output, c.x, c.ql, c.dl, c.R)
        assert sqd == metric.mean_over_hits(ap_q, rel_q)
        with pytest.raises(ValueError, match="quantised"):
            m.get_maps_by_feature(types.SimpleNamespace(output=c.x, codes=None, codebooks=None, label=c.dl), q)
    finally:
        m.close()
        arena.close()
    # the pooled context goes back to the other modes
    ref = MAPs(c.R)
    try:
        assert ref.get_maps_by_feature(types.SimpleNamespace(output=c.x, label=c.dl), q) == metric.mean_over_hits(c.ap, c.rel)
    finally:
        ref.close()


def test_twenty_new_objects_draw_one_pooled_context():
    c = case(*SMALL)
    db = types.SimpleNamespace(codes=c.codes, codebooks=c.books, label=c.dl)
    q = types.SimpleNamespace(output=c.qf, label=c.ql)
    want = metric.mean_over_hits(c.ap, c.rel)
    release_engines()
    gc.collect()
    s0 = pool_stats()
    assert s0["contexts_idle"] == 0
    assert MAPs(c.R, quantised=True).get_maps_by_feature(db, q) == want      # the object dies with the statement
    gc.collect()
    one = pool_stats()
    assert one["contexts_idle"] == 1
    for i in range(20):
        assert MAPs(c.R, quantised=True).get_maps_by_feature(db, q) == want, i
    gc.collect()
    st = pool_stats()
    assert st["contexts_idle"] == 1 and st["contexts_created"] - s0["contexts_created"] == 1
    assert st["contexts_recycled"] - s0["contexts_recycled"] == 20
    assert abs(st["idle_device_bytes"] - one["idle_device_bytes"]) < 65536, (st, one)
    release_engines()

"""Every branch of real_ladder on the two derived row sources -- the database's sign codes read as +-1 (hg_topr_asym / hg_map_asym) and
product-quantisation codes (hg_topr_pq / hg_map_pq): the requery child on a borrowed row source, the widened slices, R = N beyond the
LDS, the global ranking passes and the exact-chain sample.  tests/test_hip_real.py pins these branches for the float table; here each
runs from the source's own image, rescore and expand kernels, and each test asserts the stat that proves its branch was taken.  A code
row is +-1.0 and a PQ row decodes by gather: oracle/real_map.py on that table is the whole reference, every comparison is on bits."""
import functools
import types

import numpy as np
import pytest

from hashgan_amd import _native, pq
from tests.test_asym_gpu import asym_context
from tests.test_pq_gpu import oracle, pq_context, same_lists

pytestmark = pytest.mark.gpu

STATE = _native.HG_ERR_STATE
SOURCES = pytest.mark.parametrize("source", ["codes", "pq"])


def on_source(source, dbf, qf, dl, ql, R, M=4, K=256, seed=0):
    """One case on one row source: the tables its loader takes, the float table the source stands for (+-1.0 of the signs, or the
    decoded PQ rows) and the oracle's ranking on it -- never modified."""
    c = types.SimpleNamespace(source=source, Q=qf.shape[0], N=dbf.shape[0], b=dbf.shape[1], R=R, C=dl.shape[1], qf=qf,
                              ql=ql.astype(np.int64), dl=dl.astype(np.int64))
    if source == "codes":
        c.dbf = dbf
        x = np.where(dbf > 0, 1, -1).astype(np.float32)
    else:
        rng = np.random.default_rng(seed)
        dsub = c.b // M
        c.books = np.stack([dbf[rng.choice(c.N, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
        c.codes = pq.encode(dbf, c.books)
        x = pq.decode(c.codes, c.books)
    c.ap, c.idx, c.score, c.match, c.rel = oracle(qf, x, c.ql, c.dl, R)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


class Ranker:
    """The context of a case's source, its ranking calls and its stat for "the last call read expanded float rows"."""

    def __init__(self, c, opts=None):
        self.c = c
        self.ctx = asym_context(c) if c.source == "codes" else pq_context(c)
        for k, v in (opts or {}).items():
            self.ctx.set_option(k, v)
        self.topr = self.ctx.topr_asym if c.source == "codes" else self.ctx.topr_pq
        self.map = self.ctx.map_asym if c.source == "codes" else self.ctx.map_pq

    def stat(self, key):
        return self.ctx.get_stat(key)

    def seen(self):
        """What the last call did, for an assertion's message."""
        return {k: self.stat(k) for k in ("real_attempts", "real_requeried", "real_cap_boost", "real_path")} | {"float_rows": self.float_rows()}

    def float_rows(self):
        return self.ctx.get_stat("asym_float_rows" if self.c.source == "codes" else "pq_float_rows")

    def reload(self, c):
        """Another database of the same shape through the source's own loader, the same queries."""
        if c.source == "codes":
            assert self.ctx.set_database_f32(c.dbf, c.dl)[1] == 0
        else:
            assert self.ctx.set_database_pq(c.codes, c.books, c.dl)[1] == 0
        assert self.ctx.set_queries_f32(c.qf, c.ql)[1] == 0

    def lists(self):
        """(return code, message, idx, score) of hg_get_topr_real on what the last call left."""
        idx, score = np.empty((self.c.Q, self.c.R), np.uint32), np.empty((self.c.Q, self.c.R), np.float32)
        rc = self.ctx._lib.hg_get_topr_real(self.ctx._h, _native._ptr(idx), _native._ptr(score))
        return rc, self.ctx._lib.hg_last_error().decode(), idx, score

    def same_ap(self, got, c=None, what=""):
        c = c or self.c
        ap, rel = got
        assert np.array_equal(ap, c.ap, equal_nan=True), what
        assert np.array_equal(rel, c.rel), what

    def close(self):
        self.ctx.close()


# ------------------------------------------------------------------ a. a few lost queries go to the requery child
LOST_Q, LOST_AT, LOST_LEN = 5, 30000, 1600


@functools.lru_cache(maxsize=None)
def lost_case(source):
    """test_hip_real._lost_queries_ranked_again, shrunk: one of 48 queries has its whole top R in one stretch of the database
    (near-copies of itself stored together), so its slices overflow whatever the cut; the others win their bet.  48 queries let up to
    three go to the child (real_requery_lost: 16 x lost <= Q).  (The draw: the first one from 17 up in which, on both sources, fewer
    than ten rows of any other query's list lie in the stretch -- a query that crowds there loses its bet too.)"""
    rng = np.random.default_rng(34)
    Q, N, b, R, C = 48, 70000, 32, 1000, 7
    dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
    v = np.sign(rng.standard_normal(b)).astype(np.float32) * 0.9
    qf[LOST_Q] = v
    dbf[LOST_AT:LOST_AT + LOST_LEN] = np.tanh(0.75 * np.sign(v) + 0.3 * rng.standard_normal((LOST_LEN, b))).astype(np.float32)
    dl = (rng.random((N, C)) < 0.25).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.25).astype(np.int64)
    return on_source(source, dbf, qf, dl, ql, R, seed=34)


@SOURCES
def test_the_planted_query_has_its_whole_list_in_the_stretch_and_no_other_query_crowds_there(source):
    """Host arithmetic: the premise of the requery tests."""
    c = lost_case(source)
    inside = ((c.idx >= LOST_AT) & (c.idx < LOST_AT + LOST_LEN)).sum(1)
    assert inside[LOST_Q] == c.R
    assert np.delete(inside, LOST_Q).max() < 10, inside
    assert (c.rel > 0).any()


@SOURCES
@pytest.mark.parametrize("opts", [{}, {"real_sample_half": 0, "real_second_sample": 0}], ids=["default", "exact-chain-sample"])
def test_lost_queries_are_ranked_again_on_the_parents_row_source(source, opts):
    """The parent's call stays at one attempt on the filter path; only the losers run again, on a child context that shares the source's
    image and borrows its tables, with the parent's options.  With the default options no call, the child's included, reads expanded
    float rows; the exact-chain sample (real_sample_half = 0) reads them by design, up to 128 features.  hg_map_* leaves no ranked
    lists unless real_map_lists asks for them -- with the child engaged too."""
    c = lost_case(source)
    r = Ranker(c, opts)
    try:
        n0 = r.stat("real_requeried")
        r.same_ap(r.map(c.R))
        n1 = r.stat("real_requeried") - n0
        assert n1 >= 1, r.seen()
        assert r.stat("real_attempts") == 1, r.seen()
        assert r.stat("real_path") & 1, r.seen()
        assert r.float_rows() == (1 if opts else 0), r.seen()
        rc, said, _, _ = r.lists()
        assert rc == STATE and "real_map_lists" in said
        same_lists(r.topr(c.R), c)
        assert r.stat("real_requeried") - n0 == 2 * n1, r.seen()
        assert r.stat("real_attempts") == 1 and r.stat("real_path") & 1, r.seen()
        assert r.float_rows() == (1 if opts else 0), r.seen()
        r.ctx.set_option("real_map_lists", 1)
        r.same_ap(r.map(c.R), what="real_map_lists")
        assert r.stat("real_requeried") - n0 == 3 * n1
        rc, said, idx, score = r.lists()
        assert rc == 0, said
        same_lists((idx, score), c, what="real_map_lists")
    finally:
        r.close()


# ------------------------------------------------------------------ b. widened slices
@functools.lru_cache(maxsize=None)
def sorted_case(source, permuted=False):
    """test_hip_real.test_features_that_follow_the_labels_in_a_class_sorted_database: rows stored class by class, features that follow the
    class, so a query's top rows sit in its class's tenth of the segments.  permuted: the same rows shuffled -- ordinary slices."""
    rng = np.random.default_rng(11)
    Q, N, b, R, C = 5, 200000, 64, 4000, 10
    proto = rng.standard_normal((C, b)).astype(np.float32)
    cls, qcls = np.sort(rng.integers(0, C, N)), rng.integers(0, C, Q)
    dbf = np.tanh(0.7 * proto[cls] + rng.standard_normal((N, b), dtype=np.float32)).astype(np.float32)
    qf = np.tanh(0.7 * proto[qcls] + rng.standard_normal((Q, b), dtype=np.float32)).astype(np.float32)
    eye = np.eye(C, dtype=np.int64)
    dl = eye[cls]
    if permuted:
        perm = rng.permutation(N)
        dbf, dl = np.ascontiguousarray(dbf[perm]), np.ascontiguousarray(dl[perm])
    return on_source(source, dbf, qf, dl, eye[qcls], R, seed=11)       # (seed: the same codebook rows by number, not by content)


@SOURCES
def test_crowded_slices_are_widened_remembered_and_reset_by_a_reload(source):
    """Both sampled cuts lose on slice capacity, the slices are widened (real_cap_boost) and the third bet holds; the next call bets with
    the wide slices at once; a reload through the source's own loader starts from ordinary slices again."""
    c, p = sorted_case(source), sorted_case(source, True)
    r = Ranker(c)
    try:
        r.same_ap(r.map(c.R))
        assert r.stat("real_attempts") >= 3 and r.stat("real_cap_boost") > 1 and r.stat("real_path") & 1, r.seen()
        same_lists(r.topr(c.R), c)
        assert r.stat("real_attempts") == 1 and r.stat("real_path") & 1, r.seen()     # the widened slices are remembered
        r.reload(p)
        assert r.stat("real_cap_boost") == 1
        r.same_ap(r.map(c.R), p, "permuted")
        assert r.stat("real_attempts") == 1 and r.stat("real_cap_boost") == 1 and r.stat("real_path") & 1, r.seen()
    finally:
        r.close()


# ------------------------------------------------------------------ c. R = N beyond the LDS
@functools.lru_cache(maxsize=None)
def every_row_case(source, kind):
    """continuous: tanh queries (PQ: K = 256) -- score groups of LDS size; piled: queries on the grid {-1, 0, 1} (PQ: 16 distinct rows)
    -- scores pile up in the buckets."""
    rng = np.random.default_rng(31)
    Q, N, b, C = 6, 30000, 32, 10
    dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    if kind == "continuous":
        qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
    else:
        qf = rng.integers(-1, 2, (Q, b)).astype(np.float32)
    dl = (rng.random((N, C)) < 0.2).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.2).astype(np.int64)
    M, K = (4, 256) if kind == "continuous" else (2, 4)
    return on_source(source, dbf, qf, dl, ql, N, M=M, K=K, seed=31)


@SOURCES
@pytest.mark.parametrize("kind", ["continuous", "piled"])
def test_every_row_a_record_ranked_group_by_group_or_by_radix_passes(source, kind):
    """No cut: the rows are expanded (the float32 MFMA pass), every row is a record, far more than the LDS holds.  Continuous scores are
    ordered group by group (k_real_group_split / k_real_group_sort, bit 2 of real_path); piled scores, and real_groups = 0, take the
    radix passes."""
    c = every_row_case(source, kind)
    assert (c.rel > 0).any()
    r = Ranker(c)
    try:
        same_lists(r.topr(c.R), c)
        assert r.float_rows() == 1, r.seen()
        assert ((r.stat("real_path") >> 2) & 1) == (1 if kind == "continuous" else 0), r.seen()
        assert r.stat("real_attempts") == 1
        assert np.array_equal(r.ctx.get_match(), c.match)
        r.same_ap(r.map(c.R))
        assert ((r.stat("real_path") >> 2) & 1) == (1 if kind == "continuous" else 0)
        r.ctx.set_option("real_groups", 0)
        same_lists(r.topr(c.R), c, what="real_groups 0")
        assert ((r.stat("real_path") >> 2) & 1) == 0
        r.same_ap(r.map(c.R), what="real_groups 0")
    finally:
        r.close()


# ------------------------------------------------------------------ d. the global ranking passes and the exact-chain sample at filter size
@functools.lru_cache(maxsize=None)
def tanh_case(source):
    rng = np.random.default_rng(41)
    Q, N, b, R, C = 12, 70000, 64, 2500, 10
    dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
    dl = (rng.random((N, C)) < 0.2).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.2).astype(np.int64)
    return on_source(source, dbf, qf, dl, ql, R, seed=41)


@SOURCES
def test_every_option_row_of_the_filter_path_equals_the_oracle(source):
    """test_hip_real.test_filter_and_rescore_equals_the_exact_passes' option rows (real_mfma, real_sort_lds, real_sample_half,
    real_second_sample) on one context: the filter (bit 0 of real_path) exactly when real_mfma = 2, the LDS rank (bit 1) exactly when
    real_sort_lds allows it, one attempt, the oracle's lists and APs each time."""
    c = tanh_case(source)
    assert (c.rel > 0).any()
    r = Ranker(c)
    try:
        for mode, lds, half_sample, second in ((2, 1, 1, 1), (2, 1, 1, 0), (2, 1, 0, 1), (2, 0, 1, 1), (1, 1, 1, 1), (0, 1, 1, 1)):
            what = "real_mfma %d, real_sort_lds %d, real_sample_half %d, real_second_sample %d" % (mode, lds, half_sample, second)
            r.ctx.set_option("real_mfma", mode)
            r.ctx.set_option("real_sort_lds", lds)
            r.ctx.set_option("real_sample_half", half_sample)
            r.ctx.set_option("real_second_sample", second)
            for call in ("topr", "map"):
                if call == "topr":
                    same_lists(r.topr(c.R), c, what=what)
                else:
                    r.same_ap(r.map(c.R), what=what)
                path = r.stat("real_path")
                assert r.stat("real_attempts") == 1, (what, call, r.seen())
                assert (path & 1) == (1 if mode == 2 else 0), (what, call, r.seen())
                assert ((path >> 1) & 1) == (1 if mode == 2 and lds else 0), (what, call, r.seen())
                if mode < 2:
                    assert r.float_rows() == 1, (what, call)
                elif half_sample:
                    assert r.float_rows() == 0, (what, call)
    finally:
        r.ctx.set_option("real_mfma", 2)
        r.ctx.set_option("real_sort_lds", 1)
        r.ctx.set_option("real_sample_half", 1)
        r.ctx.set_option("real_second_sample", 1)
        r.close()

"""No result depends on what the memory held before (needs an MI355X): every entry point of the engine on second-hand contexts and on
poisoned fresh memory, against the host references of the per-feature files (tests/second_hand_cases.py: the shapes, the inputs, the
references, the family table; DESIGN.md section 10, "Second-hand memory: what the suite pins").

Device buffers only grow, MAPs recycles contexts, and a trimmed or destroyed context gives its blocks to a process-wide cache that hands
them out again uncleared: in production a kernel runs on memory that holds another job's data.  Each pair of the matrix runs a SOIL job
(only to dirty the buffers), then a PROBE job that differs from it in every padded quantity, three times:
    (a) same_context    the probe on the context that just ran the soil       guard: device_bytes does not shrink (PQ tables apart)
    (b) trim            soil -> trim() -> probe                              guard: trim() frees memory, the probe allocates again
    (c) close_and_new   soil -> close() -> a new Context(0) -> probe          guard: the process-wide stat cache_hits rises
(under HG_EFENCE the cache is bypassed, so the guards on its counters are not applied there).  hg_trim gives the work buffers to the
cache and then returns the whole cache to the runtime (hg_core.hip: a caller that trims wants the memory back at the runtime), so on
route (b) no block CAN come back from the cache: the probe's work buffers are the runtime's next allocations, which hold whatever the
runtime left in them -- the poisoned child makes that case deterministic.  Every probe result equals its host reference by
the rule of the feature's own file -- bit for bit where that file is, its stated bound where it has one -- and the exact results are
byte-identical on the three routes.  The last test runs the same matrix in a child process under HG_EFENCE=2, where every new device
buffer starts as 0xCB bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import brute_refs as B
from tests import second_hand_cases as S
from tests.dev_arena import Arena
from hashgan_amd import _native, metric

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFENCE = bool(os.environ.get("HG_EFENCE"))


class Recorder:
    """A context that notes which of its public methods are called (the family table of second_hand_cases must name exactly these)."""

    def __init__(self, ctx, log):
        self.__dict__["_ctx"], self.__dict__["_log"] = ctx, log

    def __getattr__(self, name):
        a = getattr(self._ctx, name)
        if callable(a) and not name.startswith("_"):
            self._log.add(name)
        return a


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def load_codes(ctx, c):
    ctx.set_database(metric.pack_codes(c.db), metric.pack_labels(c.dl), c.s.b, c.s.C)
    ctx.set_queries(metric.pack_codes(c.qb), metric.pack_labels(c.ql))


def load_f32(ctx, d):
    assert ctx.set_database_f32(d.dbf, d.dl)[1] == 0
    assert ctx.set_queries_f32(d.qf, d.ql)[1] == 0


# ------------------------------------------------------------------ the jobs: (context, data, arena) -> {name: array}; a name that
# starts with "~" is compared under a bound, every other bit for bit (and byte for byte between the routes)
def job_hamming(ctx, c, arena):
    R, out = c.s.R, {}
    load_codes(ctx, c)
    out["map_ap"], out["map_rel"] = ctx.map(R)
    out["optimistic"] = np.array([ctx.get_stat("last_optimistic")])
    ctx.topr(R)
    out["idx"], out["dist"] = ctx.get_topr()
    out["match"] = ctx.get_match()
    ctx.hist(); ctx.plan(R); ctx.select(); ctx.match(); ctx.ap()         # the staged exact sequence
    out["staged_ap"], out["staged_rel"] = ctx.get_ap()
    ctx.map_begin(R); ctx.map_begin(R)                                   # two steps in flight
    out["step1_ap"], out["step1_rel"] = ctx.map_end()
    out["step2_ap"], out["step2_rel"] = ctx.map_end()
    return out


def check_hamming(c, got):
    for k in ("map", "staged", "step1", "step2"):
        assert same(got[k + "_ap"], c.ap), k
        assert same(got[k + "_rel"], c.rel), k
    assert same(got["idx"], c.idx) and same(got["dist"], c.dist)
    assert same(got["match"].astype(bool), c.imatch)
    if c.s.name.startswith("bet"):
        assert got["optimistic"][0] == 1, "the bet was not taken (or lost)"


def job_lists(ctx, d, arena):
    c, l = d
    ks, out = c.s.ks, {}
    load_codes(ctx, c)
    ctx.topr(c.s.R)
    ctx.ap_at(ks)
    out["ap_at"], out["ap_at_rel"] = ctx.get_ap_at()
    ctx.graded(ks, l.gain, l.disc, keep_grades=True)
    out["gsum"], out["ghits"], out["~dcg"], out["~wsum"] = ctx.get_graded()
    out["grades"] = ctx.get_grades()
    ctx.votes(ks)
    out["votes"] = ctx.get_votes()
    out["vote_pred"], out["vote_top"] = ctx.get_vote_pred()
    out["vote_conf"] = ctx.get_vote_confusion()
    ctx.tie_ap(ks)
    tie = ctx.get_tie_ap()
    out.update({("~tie_" + k if k in B.TIE_FLOATS or k == "rel_exp" else "tie_" + k): v for k, v in tie.items()})
    ctx.rel_hist()
    out["rel_all"], out["rel_rel"] = ctx.get_rel_hist()
    ctx.grade_hist()
    out["grade_hist"] = ctx.get_grade_hist()
    ctx.joint_hist()
    out["joint_grades"] = np.array([ctx.get_stat("joint_hist_grades")])
    out["joint"] = ctx.get_joint_hist()
    return out


def check_lists(d, got):
    c, l = d
    ks = c.s.ks
    assert same(got["ap_at"], l.ap_at[0]) and same(got["ap_at_rel"], l.ap_at[1])
    B.assert_graded_tables((got["gsum"], got["ghits"], got["~dcg"], got["~wsum"]), l.graded, ks)
    assert same(got["grades"], l.grades)
    votes, pred, top, conf = l.votes
    assert same(got["votes"], votes) and same(got["vote_top"], top) and same(got["vote_pred"], pred) and same(got["vote_conf"], conf)
    B.assert_tie_close({k: got[("~tie_" if "~tie_" + k in got else "tie_") + k] for k in B.TIE_ALL}, l.tie, ks)
    assert np.array_equal(got["rel_all"], l.rel_hist[0]) and np.array_equal(got["rel_rel"], l.rel_hist[1])
    assert np.array_equal(got["grade_hist"], l.grade_hist)
    assert got["joint_grades"][0] == l.nG and same(got["joint"], l.joint)


def job_rerank(ctx, d, arena):
    R, out = d.s.R, {}
    load_f32(ctx, d)
    out["ap"], out["rel"] = ctx.map_rerank(R)
    out["idx"], out["dist"] = ctx.get_topr()
    out["score"] = ctx.get_rerank_scores()
    out["match"] = ctx.get_match()
    out["idx2"], out["dist2"], out["score2"] = ctx.topr_rerank(R)
    out["match2"] = ctx.get_match()
    out["counters"] = np.array([ctx.get_stat(k) for k in ("rerank_records", "rerank_groups_lds", "rerank_groups_global")])
    return out


def check_rerank(d, got):
    for k in ("", "2"):
        assert (got["idx" + k] == d.idx).all() and (got["dist" + k] == d.dist).all(), k
        assert bits(got["score" + k]) == bits(d.score), k
        assert (got["match" + k] == d.match).all(), k
    assert (got["rel"] == d.rel).all()
    assert bits(got["ap"]) == bits(d.ap)
    assert got["counters"].tolist() == [d.records, d.groups, 0], "the device counters of the call (records, groups in LDS, groups by radix)"


def _inner_product_job(topr, mapper):
    def job(ctx, d, arena):
        out = {}
        out["idx"], out["score"] = getattr(ctx, topr)(d.s.R)
        out["real_path"] = np.array([ctx.get_stat("real_path")])
        out["match"] = ctx.get_match()
        out["ap"], out["rel"] = getattr(ctx, mapper)(d.s.R)
        return out
    return job


def check_inner_product(d, got):
    assert np.array_equal(got["score"].view(np.uint32), d.score.view(np.uint32))
    assert np.array_equal(got["idx"], d.idx)
    assert np.array_equal(got["match"], d.match)
    assert same(got["ap"], d.ap) and np.array_equal(got["rel"], d.rel)


def job_real(ctx, d, arena):
    load_f32(ctx, d)
    return _inner_product_job("topr_real", "map_real")(ctx, d, arena)


def check_real(d, got):
    check_inner_product(d, got)
    if d.s.name.startswith("filter"):
        assert got["real_path"][0] & 1, "not the filter path"


def job_asym(ctx, d, arena):
    load_f32(ctx, d)
    return _inner_product_job("topr_asym", "map_asym")(ctx, d, arena)


def job_pq(ctx, d, arena):
    assert ctx.set_database_pq(d.codes, d.books, d.dl)[1] == 0
    assert ctx.set_queries_f32(d.qf, d.ql)[1] == 0
    return _inner_product_job("topr_pq", "map_pq")(ctx, d, arena)


def job_pq_encode(ctx, d, arena):
    out = {}
    out["codes"], out["err"], bad = ctx.pq_encode(d.dbf, d.books, want_err=True)
    out["bad"] = np.array([bad])
    assert ctx.set_database_pq_f32(d.dbf, d.books, d.dl)[1] == 0
    assert ctx.set_queries_f32(d.qf, d.ql)[1] == 0
    out["idx"], out["score"] = ctx.topr_pq(d.s.R)
    out["match"] = ctx.get_match()
    return out


def check_pq_encode(d, got):
    assert np.array_equal(got["codes"], d.codes)
    assert bits(got["err"]) == bits(d.err)
    assert got["bad"][0] == 0
    assert np.array_equal(got["score"].view(np.uint32), d.score.view(np.uint32))
    assert np.array_equal(got["idx"], d.idx) and np.array_equal(got["match"], d.match)


def job_neighbours(ctx, d, arena):
    c, n = d
    R, out = c.s.R, {}
    load_codes(ctx, c)
    ctx.topr(R)
    out["idx"] = ctx.get_topr()[0]
    ctx.neighbours_from_lists(c.s.G)                                      # the first G ranks, captured on the device
    out["first_ids"], out["first_cnt"] = ctx.get_neighbours()
    ctx.match_neighbours()
    out["first_match"] = ctx.get_match()
    ctx.set_neighbours(n.gt)                                              # ragged sets from the host
    out["ids"], out["cnt"] = ctx.get_neighbours()
    ctx.topr(R)
    ctx.match_neighbours()
    out["match"] = ctx.get_match()
    ctx.ap()
    out["ap"], out["rel"] = ctx.get_ap()
    ctx.nbr_hist()
    out["nbr_hist"], out["nbr_cnt"] = ctx.get_nbr_hist()
    return out


def check_neighbours(d, got):
    c, n = d
    assert np.array_equal(got["idx"], c.idx)
    assert np.array_equal(got["first_ids"], n.first_sorted[0]) and np.array_equal(got["first_cnt"], n.first_sorted[1])
    assert np.array_equal(got["first_match"], n.first_match)
    assert np.array_equal(got["ids"], n.gt_sorted[0]) and np.array_equal(got["cnt"], n.gt_sorted[1])
    assert np.array_equal(got["match"], n.match)
    assert bits(got["ap"]) == bits(n.ap[0]) and np.array_equal(got["rel"], n.ap[1])
    assert np.array_equal(got["nbr_hist"], n.nbr_hist) and np.array_equal(got["nbr_cnt"], n.gt_sorted[1])


def job_devmem(ctx, d, arena):
    """Inputs from the arena (a producer context's scratch, filled through memcpy_htod), results exported into the same arena, which is
    pre-filled with the canary byte.  The arena's expected image holds the inputs, the ORACLE's results at the destinations and the
    canary everywhere else; the image read back is the job's result."""
    r, s = d.real, d.s
    arena.reset()
    f, l = arena.put(r.dbf, "float32"), arena.put(r.dl, "int64")
    fq, lq = arena.put(r.qf, "float32"), arena.put(r.ql, "int64")
    assert ctx.set_database_dev(f, l)[1] == 0
    assert ctx.set_queries_dev(fq, lq)[1] == 0
    aps = []

    def export(items):
        dsts = []
        for name, dtype, want in items:
            dst = arena.out(want.shape, dtype)
            arena.expect(dst, want)
            dsts.append((name, dst))
            if name == "ap":
                aps.append(dst)
        ctx.export(dsts)

    ctx.topr(s.R); ctx.match(); ctx.ap()
    export([("idx", "int64", d.idx.astype(np.int64)), ("dist", "uint8", d.dist.astype(np.uint8)), ("match", "uint8", d.match),
            ("ap", "float64", d.ap.reshape(-1, 1))])
    ctx.topr_real(s.R, download=False); ctx.match(); ctx.ap()
    export([("idx", "int64", r.idx.astype(np.int64)), ("score", "float32", r.score), ("match", "uint8", r.match),
            ("ap", "float64", r.ap.reshape(-1, 1))])
    image = arena.read()
    for dst in aps:                                                      # (a query without a hit: any NaN stands for the oracle's)
        o = dst.ptr - arena.base
        g, w = image[o:o + s.Q * 8].view(np.float64), arena.host[o:o + s.Q * 8].view(np.float64)
        both = np.isnan(g) & np.isnan(w)
        assert both.any()
        g[both] = w[both]
    return {"image": image, "expected": arena.host.copy()}


def check_devmem(d, got):
    bad = np.flatnonzero(got["image"] != got["expected"])
    assert bad.size == 0, "%d bytes of the arena differ from the inputs, the oracle's results and the canary, the first at offset %d" % (bad.size, bad[0])


def job_shard_step(ctx, c, arena):
    load_codes(ctx, c)
    ap, rel, lost = ctx.shard_step(c.s.R, replica_world=1)
    return {"ap": ap, "rel": rel, "lost": np.array([-1 if lost is None else int(lost)])}


def check_shard_step(c, got):
    assert got["lost"][0] == 0, "the sharded bet was not taken (-1) or lost (1)"
    assert same(got["ap"], c.ap) and same(got["rel"], c.rel)


JOBS = {"hamming": (job_hamming, check_hamming), "lists": (job_lists, check_lists), "rerank": (job_rerank, check_rerank),
        "real": (job_real, check_real), "asym": (job_asym, check_inner_product), "pq": (job_pq, check_inner_product),
        "pq_encode": (job_pq_encode, check_pq_encode), "neighbours": (job_neighbours, check_neighbours), "devmem": (job_devmem, check_devmem),
        "shard_step": (job_shard_step, check_shard_step)}
assert set(JOBS) == set(S.FAMILIES) == set(S.DATA)


def run_job(family, ctx, data, arena, select, log):
    for k, v in dict(S.OPTIONS, **S.FAMILY_OPTIONS.get(family, {}), **S.BET_SELECTS[select]).items():
        ctx.set_option(k, v)
    return JOBS[family][0](Recorder(ctx, log), data, arena)


@pytest.fixture(scope="module")
def arena():
    a = Arena(8 << 20)                                   # (allocated once, outside every window a cache_hits guard watches)
    yield a
    a.close()


@pytest.mark.parametrize("pair", S.PAIRS, ids=[p[0] for p in S.PAIRS])
def test_probe_equals_its_reference_on_every_route(pair, arena):
    tag, soil_family, soil_shape, family, probe_shape, select = pair
    soil, probe = S.DATA[soil_family](soil_shape), S.DATA[family](probe_shape)
    results = {}
    for route in S.ROUTES:
        ctx = _native.Context(0)
        try:
            run_job(soil_family, ctx, soil, arena, select, set())
            bytes0, hits0 = ctx.get_stat("device_bytes"), ctx.get_stat("cache_hits")
            if route == "trim":
                ctx.trim()
                trimmed, misses0 = ctx.get_stat("device_bytes"), ctx.get_stat("cache_misses")
            elif route == "close_and_new":
                ctx.close()
                ctx = _native.Context(0)
            log = set()
            got = run_job(family, ctx, probe, arena, select, log)
            # the premise of the route
            if route == "same_context":
                # (the PQ code and codebook tables are the one exception to "buffers only grow": every database loader releases them,
                # hg_ctx.hpp forget_tables(), and the PQ loaders allocate them again at the new size)
                s = S.shape(soil_shape)
                released = s.N * s.M + s.M * s.K * s.dsub * 4 if soil_family in ("pq", "pq_encode") else 0
                assert ctx.get_stat("device_bytes") >= bytes0 - released, (tag, route, "the context gave memory back between soil and probe")
            elif route == "trim":
                assert trimmed < bytes0, (tag, route, "trim() freed nothing")
                if not EFENCE:
                    assert ctx.get_stat("cache_misses") > misses0, (tag, route, "no work buffer was allocated again")
            elif not EFENCE:
                assert ctx.get_stat("cache_hits") > hits0, (tag, route, "no block came back from the cache")
            assert log - set(S.EXCLUDED) == set(S.FAMILIES[family]), (tag, "the family table names other calls than the job makes",
                                                                       sorted((log - set(S.EXCLUDED)) ^ set(S.FAMILIES[family])))
            print("%s, route %s" % (tag, route))
            JOBS[family][1](probe, got)
            results[route] = {k: bits(v) for k, v in got.items() if not k.startswith("~")}
        finally:
            ctx.close()
    for route in S.ROUTES[1:]:
        differ = sorted(k for k in results[route] if results[route][k] != results[S.ROUTES[0]][k])
        assert not differ, (tag, "routes %s and %s leave different bytes in" % (S.ROUTES[0], route), differ)


# The un-poisoned module on an MI355X, measured: 9.2 s inside pytest (30 pairs x 3 routes), 11 s with the interpreter's start
# (DESIGN.md section 10).  The poison fill adds a hipMemset and a device synchronisation to every allocation: the child gets three
# times that (it took 10.1 s).
MODULE_SECONDS = 11.0
THIS = "tests/test_second_hand_gpu.py::test_the_matrix_on_poisoned_fresh_memory"


def test_the_matrix_on_poisoned_fresh_memory():
    """The matrix again in a fresh child process under HG_EFENCE=2: every new device buffer is a plain hipMalloc filled with 0xCB, so a
    kernel that relies on new memory being zero fails deterministically.  The mode is read once per process: a child is the only way to
    set it.  Mode 2 ONLY: modes 1 and 3 put an unmapped page behind or in front of every buffer, which turns an overrun into a GPU
    fault on purpose -- not something to run on a shared machine.  (Kept last in the file.)"""
    env = dict(os.environ, HG_EFENCE="2")
    cmd = [sys.executable, "-m", "pytest", "tests/test_second_hand_gpu.py", "-m", "gpu", "-q", "-x", "--deselect", THIS]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=3 * MODULE_SECONDS)
    if r.returncode != 0:
        print("\n".join(r.stdout.splitlines()[-60:]))
    assert r.returncode == 0, "the matrix fails on poisoned fresh memory (exit status %d)" % r.returncode

"""The order-free side metrics on a database-sharded context (needs an MI355X): hg_pack_side_table / hg_merge_side_table (k_side_pack,
k_side_merge), hg_tie_ap on a shard, and the `*_shard` functions of hashgan_amd.sharded on virtual shards of one GPU -- G threads, G
contexts, LocalComm, tests/test_sharded_gpu.py's idiom -- against the extra_metrics functions on one context with the whole database.

Every comparison is ==: the merged tables are integers, and k_tie_ap and the NumPy reductions are functions of a query's table and the
cut-offs alone.  Shapes and their properties: tests/shard_side_cases.py (checked by tests/test_shard_side_host.py)."""
import functools

import numpy as np
import pytest
from tests import cases
from tests import shard_side_cases as S
from hashgan_amd import _native, metric, sharded
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG
Q, N = S.Q, S.N
QPAD = 128
WHICH = ("rel", "grade", "joint")


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def same(got, ref, where=""):
    """Every array of the structure, bit for bit where it is integer and with NaN == NaN where it is float."""
    if isinstance(ref, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(ref), where
        for k in ref:
            same(got[k], ref[k], "%s[%s]" % (where, k))
    elif isinstance(ref, tuple):
        assert isinstance(got, tuple) and len(got) == len(ref), where
        for i, (g, r) in enumerate(zip(got, ref)):
            same(g, r, "%s[%d]" % (where, i))
    else:
        assert got.dtype == ref.dtype and got.shape == ref.shape, (where, got.dtype, ref.dtype, got.shape, ref.shape)
        assert np.array_equal(got, ref, equal_nan=ref.dtype.kind == "f"), where


def shard_ctx(name, r, G):
    """Shard r of G of the case's database, the queries replicated."""
    qb, db, ql, dl = S.make(name)
    lo, n = sharded.shard_bounds(N, G)[r]
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db[lo:lo + n]), metric.pack_labels(dl[lo:lo + n]), db.shape[1], dl.shape[1], idx_base=lo, n_total=N)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
    return ctx


def whole_ctx(name):
    return shard_ctx(name, 0, 1)


def run_shards(name, G, fn):
    """fn(ctx, comm, rank) on G virtual shards -> [its result per rank]."""
    def work(r, comm):
        ctx = shard_ctx(name, r, G)
        try:
            comm.ctx = ctx
            return fn(ctx, comm, r)
        finally:
            ctx.close()

    return sharded.LocalComm.run(G, work)


def seven(ctx, comm):
    return {"lookup": sharded.lookup_histograms_shard(ctx, comm),
            "curves": sharded.hamming_radius_curves_shard(ctx, comm),
            "tie_map": sharded.tie_aware_map_shard(ctx, comm, S.CUTOFFS),
            "tie_pr": sharded.tie_aware_precision_recall_at_k_shard(ctx, comm, S.CUTOFFS),
            "grade": sharded.grade_histograms_shard(ctx, comm),
            "joint": sharded.distance_grade_histograms_shard(ctx, comm),
            "tie_graded": sharded.tie_aware_graded_at_k_shard(ctx, comm, S.CUTOFFS)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The seven extra_metrics functions on the whole database in one context: computed once per shape, never changed."""
    a = S.make(name)
    return {"lookup": X.lookup_histograms(*a), "curves": X.hamming_radius_curves(*a), "tie_map": X.tie_aware_map(*a, S.CUTOFFS),
            "tie_pr": X.tie_aware_precision_recall_at_k(*a, S.CUTOFFS), "grade": X.grade_histograms(*a),
            "joint": X.distance_grade_histograms(*a), "tie_graded": X.tie_aware_graded_at_k(*a, S.CUTOFFS)}


# ------------------------------------------------------------------ 1: the same bits as one context
@pytest.mark.parametrize("G", S.GS)
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_every_rank_returns_what_one_context_returns(name, G):
    b, C, multihot = S.SHAPES[name]
    ref = reference(name)

    def work(ctx, comm, r):
        out = seven(ctx, comm)
        return out, ctx.get_stat("joint_hist_grades"), ctx.get_stat("joint_hist_bands"), ctx.get_stat("merged_joint_grades")

    res = run_shards(name, G, work)
    for r, (out, Gs, bands, Gc) in enumerate(res):
        same(out, ref, "%s G=%d rank %d: " % (name, G, r))
        assert Gc == ref["joint"].shape[2]
        if multihot:
            last = r == G - 1
            assert Gc == 12 and Gs == (12 if last else 5) and bands == (2 if last else 1), (r, Gs, bands, Gc)
    if multihot and G > 1:
        assert all(Gs < Gc for _, Gs, _, Gc in res[:-1])                     # the zero-padding in g was exercised


# ------------------------------------------------------------------ 2: the merged tables, and the shard's own next to them
def tables_of(ctx, merged):
    pre = "get_merged_" if merged else "get_"
    return {"rel": getattr(ctx, pre + "rel_hist")(), "grade": getattr(ctx, pre + "grade_hist")(), "joint": getattr(ctx, pre + "joint_hist")()}


@pytest.mark.parametrize("name,G", [("b8_c10", 2), ("b100_c10", 3), ("b64_c81_multihot", 8)])
def test_merged_getters_are_the_whole_databases_and_the_own_getters_still_the_shards(name, G):
    qb, db, ql, dl = S.make(name)
    one = whole_ctx(name)
    try:
        one.rel_hist(), one.grade_hist(), one.joint_hist()
        whole = tables_of(one, merged=False)
        for which in WHICH:                                                  # nothing merged yet
            raises(STATE, getattr(one, "get_merged_%s_hist" % which))
    finally:
        one.close()

    def work(ctx, comm, r):
        for which in WHICH:
            sharded.merge_side_table(ctx, comm, which)
        return tables_of(ctx, merged=True), tables_of(ctx, merged=False)

    for r, (merged, own) in enumerate(run_shards(name, G, work)):
        same(merged, whole, "merged, rank %d: " % r)
        lo, n = sharded.shard_bounds(N, G)[r]
        part = (qb, db[lo:lo + n], ql, dl[lo:lo + n])
        same(own["rel"], S.brute_rel(*part), "own rel, rank %d" % r)
        same(own["grade"], S.brute_grade(*part), "own grade, rank %d" % r)
        same(own["joint"], S.brute_joint(*part, S.defined_G(ql, dl[lo:lo + n])), "own joint, rank %d" % r)
        assert (own["rel"][0].sum(0) == n).all() and (merged["rel"][0].sum(0) == N).all()


# ------------------------------------------------------------------ 3: the check refuses wrong input
def packed_blocks(name, G):
    """-> (context of shard 0 with its three passes done, {which: [every shard's block as host uint32 [planes, Qpad]]}, Gc)."""
    ctxs = [shard_ctx(name, r, G) for r in range(G)]
    try:
        for c in ctxs:
            c.rel_hist(), c.grade_hist(), c.joint_hist()
        Gc = max(c.get_stat("joint_hist_grades") for c in ctxs)
        blocks = {w: [] for w in WHICH}
        for c in ctxs:
            for w in WHICH:
                ptr, nbytes = c.pack_side_table(w, Gc)
                assert nbytes % (QPAD * 4) == 0
                host = np.empty((nbytes // (QPAD * 4), QPAD), dtype=np.uint32)
                c.memcpy_dtoh(host, ptr, nbytes)
                blocks[w].append(host)
    except Exception:
        for c in ctxs:
            c.close()
        raise
    for c in ctxs[1:]:
        c.close()
    return ctxs[0], blocks, Gc


def put(ctx, blocks, slot=0):
    buf = np.ascontiguousarray(np.concatenate(blocks))
    ptr = ctx.scratch(slot, buf.nbytes)
    ctx.memcpy_htod(ptr, buf, buf.nbytes)
    return ptr


def test_the_merge_refuses_duplicated_zeroed_and_overflowing_blocks():
    name, G = "b64_c81_multihot", 3
    b, C, _ = S.SHAPES[name]
    ctx, blocks, Gc = packed_blocks(name, G)
    try:
        assert Gc == 12 and ctx.get_stat("joint_hist_grades") == 5
        assert [len(blocks[w][0]) for w in WHICH] == [2 * (b + 1), C + 1, (b + 1) * Gc]       # the exchange layout's planes
        own = tables_of(ctx, merged=False)
        good = {}
        for w in WHICH:                                                      # the real blocks pass, from any address that is aligned
            ctx.merge_side_table(w, put(ctx, blocks[w]), G, Gc)
            good[w] = getattr(ctx, "get_merged_%s_hist" % w)()
        getter = {w: getattr(ctx, "get_merged_%s_hist" % w) for w in WHICH}

        def refused(w, fabricated, flag, n_blocks=G):
            msg = raises(STATE, ctx.merge_side_table, w, put(ctx, fabricated), n_blocks, Gc)
            assert flag in msg, msg
            raises(STATE, getter[w])                                         # no merged result is left
            for other in WHICH:                                              # ... the other merged results are
                if other != w:
                    same(getter[other](), good[other], other)
            same(tables_of(ctx, merged=False), own, "the shard's own tables")
            ctx.merge_side_table(w, put(ctx, blocks[w]), G, Gc)              # and the real blocks pass again
            same(getter[w](), good[w], w)

        for w in WHICH:
            b0, b1, b2 = blocks[w]
            refused(w, [b0, b1, b1], "column-total")                         # a block counted twice, one missing
            refused(w, [b0, b1, np.zeros_like(b2)], "column-total")          # a block zeroed
            refused(w, [b0, b1], "column-total", n_blocks=2)                 # a shard missing
        # one cell raised so that its sum leaves 32 bits: a real query's column, a plane where another block counts rows too
        b0, b1, b2 = blocks["rel"]
        p = int(np.flatnonzero(b1[:b + 1, 3])[0])
        high = b0.copy()
        high[p, 3] = 0xFFFFFFFF
        refused("rel", [high, b1, b2], "overflow")
        # the pad columns never reach either check
        pads = [x.copy() for x in blocks["rel"]]
        for x in pads:
            x[:, Q:] = 0xFFFFFFFF
        ctx.merge_side_table("rel", put(ctx, pads), G, Gc)
        same(getter["rel"](), good["rel"], "rel with poisoned pad columns")
        # bad arguments end the merged result of their table too, and only that one
        for bad in (lambda: ctx.merge_side_table("rel", put(ctx, blocks["rel"]), 0, Gc), lambda: ctx.merge_side_table("rel", None, G, Gc),
                    lambda: ctx.merge_side_table("rel", put(ctx, blocks["rel"]) + 4, G, Gc)):
            ctx.merge_side_table("rel", put(ctx, blocks["rel"]), G, Gc)
            raises(ARG, bad)
            raises(STATE, getter["rel"])
            same(getter["grade"](), good["grade"], "grade")
        raises(ARG, ctx.merge_side_table, 3, put(ctx, blocks["rel"]), G, Gc)
        same(getter["joint"](), good["joint"], "joint")                      # (no table named: nothing ended)
        raises(ARG, ctx.merge_side_table, "joint", put(ctx, blocks["joint"]), G, C + 2)
        raises(STATE, getter["joint"])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4: state rules
def merge_from(ctxs, which, Gc=0):
    """The gather by hand: every context's block copied into a scratch slot of ctxs[0], merged there."""
    packs = [c.pack_side_table(which, Gc) for c in ctxs]
    n = packs[0][1]
    assert all(nb == n for _, nb in packs)
    base = ctxs[0].scratch(1, n * len(ctxs))
    for r, (ptr, _) in enumerate(packs):
        ctxs[0].memcpy_dtod(base + r * n, ptr, n)
    ctxs[0].merge_side_table(which, base, len(ctxs), Gc)


def test_state_rules_on_a_shard():
    name = "b64_c81_multihot"
    b, C, _ = S.SHAPES[name]
    qb, db, ql, dl = S.make(name)
    ref = reference(name)["tie_map"]["per_query"]
    a, other = shard_ctx(name, 0, 2), shard_ctx(name, 1, 2)
    KS = np.asarray(S.CUTOFFS, dtype=np.int64)

    def tie_equals_reference():
        a.tie_ap(KS)
        t = a.get_tie_ap()
        for k in t:
            same(t[k], ref[k], k)

    def merged_ended():
        for w in WHICH:
            raises(STATE, getattr(a, "get_merged_%s_hist" % w))
        assert "holds rows" in raises(STATE, a.tie_ap, KS)

    def merge_all():
        for c in (a, other):
            c.rel_hist(), c.grade_hist(), c.joint_hist()
        Gc = max(c.get_stat("joint_hist_grades") for c in (a, other))
        for w in WHICH:
            merge_from([a, other], w, Gc)
        return Gc

    try:
        a.trim()
        bytes0 = a.get_stat("device_bytes")                                  # the tables alone
        assert "holds rows" in raises(STATE, a.tie_ap, KS)                    # refused as before: no merged table
        for w, pass_name in zip(WHICH, ("hg_rel_hist", "hg_grade_hist", "hg_joint_hist")):
            assert pass_name in raises(STATE, a.pack_side_table, w, C + 1)    # pack before the pass
        raises(ARG, a.pack_side_table, 3, 0)
        a.joint_hist()
        Gs = a.get_stat("joint_hist_grades")
        assert Gs == 5
        raises(ARG, a.pack_side_table, "joint", Gs - 1)
        raises(ARG, a.pack_side_table, "joint", C + 2)
        ptr, nbytes = a.pack_side_table("joint", Gs)                         # its own count is fine
        assert ptr and nbytes == (b + 1) * Gs * QPAD * 4
        raises(STATE, a.pack_side_table, "rel", 0)                           # (the other passes have still not run)
        Gc = merge_all()
        assert Gc == 12 and a.get_stat("merged_joint_grades") == 12 and a.get_stat("joint_hist_grades") == 5
        merged = tables_of(a, merged=True)
        tie_equals_reference()                                               # R up to n_total = N > this shard's rows
        assert a.N < KS[-1] == a.n_total == N
        raises(ARG, a.tie_ap, [N + 1])
        raises(ARG, a.tie_ap, [1, N, N + 1])
        raises(STATE, a.get_tie_ap)                                          # (the refused call ended its own results ...)
        same(tables_of(a, merged=True), merged, "after a refused hg_tie_ap")  # ... and no merged table
        # nothing but a reload, hg_trim and its own merge ends a merged table
        a.rel_hist(), a.grade_hist(), a.joint_hist()
        a.pack_side_table("grade", 0)
        same(tables_of(a, merged=True), merged, "after the passes again and a pack")
        tie_equals_reference()
        a.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))         # the same queries again: a new generation
        merged_ended()
        merge_all()
        same(tables_of(a, merged=True), merged, "merged again after the queries' reload")
        lo, n = sharded.shard_bounds(N, 2)[0]
        a.set_database(metric.pack_codes(db[lo:lo + n]), metric.pack_labels(dl[lo:lo + n]), b, C, idx_base=lo, n_total=N)
        a.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        merged_ended()
        merge_all()
        tie_equals_reference()
        assert a.get_stat("device_bytes") > bytes0
        a.trim()
        merged_ended()
        assert a.get_stat("device_bytes") == bytes0                          # every new buffer is on the context's list
        merge_all()
        same(tables_of(a, merged=True), merged, "merged again after hg_trim")
        tie_equals_reference()
    finally:
        a.close()
        other.close()


def test_a_whole_database_context_keeps_its_own_rules():
    """hg_tie_ap on a whole-database context runs its own pass, is bounded by N and takes no notice of a merged table; the pack and the
    merge work there too (one block)."""
    name = "b8_c10"
    ref = reference(name)["tie_map"]["per_query"]
    ctx = whole_ctx(name)
    try:
        ctx.tie_ap(S.CUTOFFS)                                                # (runs hg_rel_hist)
        t = ctx.get_tie_ap()
        ctx.timing_enable(True)
        merge_from([ctx], "rel")
        timed = ctx.timing_read()
        assert timed["k_side_pack"][1] == 1 and timed["k_side_merge"][1] == 1, timed      # the two kernels' timing names
        ctx.timing_enable(False)
        a, r = ctx.get_merged_rel_hist()
        same((a, r), ctx.get_rel_hist(), "one block merged")
        ctx.tie_ap(S.CUTOFFS)
        t2 = ctx.get_tie_ap()
        for k in t:
            same(t[k], ref[k], k)
            same(t2[k], ref[k], k)
        raises(ARG, ctx.tie_ap, [N + 1])
    finally:
        ctx.close()


def test_a_step_in_flight_and_the_licence_to_enqueue_blind_survive_pack_and_merge(case_cache):
    """hg_map_begin's step started before a pass + pack + merge returns the golden APs from hg_map_end, and their first reservations
    -- made while that step is in flight -- move no buffer a blind step touches: the next hg_map_begin is still enqueued blind."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R = c["R"]
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        ap, _ = ctx.map(R)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert ctx.get_stat("last_optimistic") == 1
        n0 = ctx.get_stat("map_async_steps")
        ctx.map_begin(R)
        assert ctx.get_stat("map_async_steps") == n0 + 1
        ctx.rel_hist()
        ptr, nbytes = ctx.pack_side_table("rel")                             # first reservations, a step in flight
        ctx.merge_side_table("rel", ptr, 1)
        ap, _ = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.map_begin(R)
        assert ctx.get_stat("map_async_steps") == n0 + 2, "pack and merge's first reservations ended the licence to enqueue blind"
        ap, _ = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert ctx.get_stat("map_async_redone") == 0
        same(ctx.get_merged_rel_hist(), ctx.get_rel_hist(), "merged == own on one shard")
        assert (ctx.get_merged_rel_hist()[0].sum(0) == len(c["dbbits"])).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5: one real communicator
@pytest.mark.parametrize("name", ["b8_c10", "b64_c81_multihot"])
def test_one_rank_over_rccl_equals_one_context(name):
    ref = reference(name)
    ctx = whole_ctx(name)
    try:
        try:
            comm = sharded.init_rccl(ctx, rank=0, world=1)
        except _native.HashganNativeError as e:
            pytest.skip("RCCL cannot be opened here: %s" % e)
        assert (comm.rank, comm.world) == (0, 1)
        same(seven(ctx, comm), ref, name)
        ctx.set_option("stage_sync", 0)                                      # pack, hg_allgather and merge ordered on the one stream
        same(seven(ctx, comm), ref, name + ", stage_sync = 0")
        ctx.comm_destroy()
    finally:
        ctx.close()

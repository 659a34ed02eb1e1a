"""The list-based side metrics on a database-sharded context (needs an MI355X): hg_pack_list_table / hg_merge_list_table (k_list_grades,
k_votes' owned-slots form, k_list_merge_grades, k_list_merge_votes), hg_graded and hg_votes from the merged tables (k_graded's plane
form, k_vote_pick) and the `*_shard` functions of hashgan_amd.sharded on virtual shards of one GPU -- G threads, G contexts, LocalComm,
tests/test_shard_side_gpu.py's idiom -- against the extra_metrics functions on one context with the whole database.

Every comparison is ==: the merged tables are integers, and k_graded's float sums are a function of the cut-offs and the grade bytes
alone.  Shapes, cut-offs and the host model of the two exchange units: tests/shard_list_cases.py (checked by
tests/test_shard_lists_host.py)."""
import functools

import numpy as np
import pytest
from tests import cases
from tests import shard_list_cases as L
from hashgan_amd import _native, metric, sharded
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG
Q, N, QPAD = L.Q, L.N, L.QPAD
KS = {"long": L.KS_LONG, "short": L.KS_SHORT}
NEW_KERNELS = ("k_list_grades", "k_list_merge_grades", "k_list_merge_votes", "k_vote_pick")


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
    elif isinstance(ref, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(ref), where
        for i, (g, r) in enumerate(zip(got, ref)):
            same(g, r, "%s[%d]" % (where, i))
    else:
        assert got.dtype == ref.dtype and got.shape == ref.shape, (where, got.dtype, ref.dtype, got.shape, ref.shape)
        assert np.array_equal(got, ref, equal_nan=ref.dtype.kind == "f"), where


def shard_ctx(name, r, G):
    """Shard r of G of the case's database, the queries replicated."""
    qb, db, ql, dl = L.make(name)
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


def three(ctx, comm, ks, ql):
    return {"map": sharded.map_at_k_shard(ctx, comm, ks),
            "graded_exp": sharded.graded_relevance_at_k_shard(ctx, comm, ks, gain="exp"),
            "graded_linear": sharded.graded_relevance_at_k_shard(ctx, comm, ks, gain="linear"),
            "knn": sharded.knn_vote_at_k_shard(ctx, comm, ks, ql)}


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """The extra_metrics functions on the whole database in one context: computed once per shape and cut-off list, never changed."""
    a = L.make(name)
    ks = KS[which]
    return {"map": X.map_at_k(*a, ks), "graded_exp": X.graded_relevance_at_k(*a, ks, gain="exp"),
            "graded_linear": X.graded_relevance_at_k(*a, ks, gain="linear"), "knn": X.knn_vote_at_k(*a, ks)}


@functools.lru_cache(maxsize=None)
def one_context(name, which):
    """What one context with the whole database leaves at the cut-off list: Context.map's (ap, rel) at R = ks[-1], hg_graded's four
    tables and grade bytes (gain "exp"), hg_votes' three tables."""
    ks = np.asarray(KS[which], dtype=np.int64)
    R = int(ks[-1])
    ctx = whole_ctx(name)
    try:
        out = {"map": ctx.map(R)}
        ctx.topr(R)
        ctx.graded(ks, X.gain_table("exp", ctx.C), X.discount_table(R), keep_grades=True)
        out["graded"], out["grades"] = ctx.get_graded(), ctx.get_grades()
        ctx.votes(ks)
        out["votes"], out["pred"], out["conf"] = ctx.get_votes(), ctx.get_vote_pred(), ctx.get_vote_confusion()
    finally:
        ctx.close()
    return out


def list_tables(ctx, ks):
    """graded() with the grade bytes kept and votes() on whatever the context runs them from -> one_context's entries."""
    ks = np.asarray(ks, dtype=np.int64)
    ctx.graded(ks, X.gain_table("exp", ctx.C), X.discount_table(int(ks[-1])), keep_grades=True)
    out = {"graded": ctx.get_graded(), "grades": ctx.get_grades()}
    ctx.votes(ks)
    out["votes"], out["pred"], out["conf"] = ctx.get_votes(), ctx.get_vote_pred(), ctx.get_vote_confusion()
    return out


def merge_both(ctx, comm, ks):
    sharded.merge_list_table(ctx, comm, "grades")
    sharded.merge_list_table(ctx, comm, "votes", ks)


def refuses_a_shard(ctx, ks=(1, 7)):
    """hg_graded and hg_votes without a merged table: the refusal of a shard, as before."""
    ks = np.asarray(ks, dtype=np.int64)
    assert "whole database" in raises(STATE, ctx.graded, ks, X.gain_table("exp", ctx.C), X.discount_table(int(ks[-1])))
    assert "whole database" in raises(STATE, ctx.votes, ks)


# ------------------------------------------------------------------ 1: the same bits as one context
@pytest.mark.parametrize("G", L.GS)
@pytest.mark.parametrize("name", list(L.SHAPES))
def test_every_rank_returns_what_one_context_returns(name, G):
    ql = L.make(name)[2]

    def work(ctx, comm, r):
        out = {}
        for which, ks in KS.items():
            out[which] = three(ctx, comm, ks, ql)
            out[which, "rank"] = sharded.rank_lists_shard(ctx, comm, ks[-1])
        assert "staged_lists" not in ctx.options_touched                      # left as found
        return out

    for r, out in enumerate(run_shards(name, G, work)):
        for which in KS:
            where = "%s G=%d rank %d, %s cut-offs: " % (name, G, r, which)
            same(out[which], reference(name, which), where)
            same(out[which, "rank"], one_context(name, which)["map"], where + "(ap, rel)")


# ------------------------------------------------------------------ 2: the blocks, the merged tables, the kernels' names
@pytest.mark.parametrize("name,G,which", [("b8_c10", 2, "long"), ("b64_c81_multihot", 3, "long"), (L.OWN, 8, "long"), ("b100_c10", 8, "short"),
                                          ("b64_c10", 3, "short")])
def test_packed_blocks_are_the_host_models_and_the_getters_one_contexts(name, G, which):
    ks = np.asarray(KS[which], dtype=np.int64)
    R = int(ks[-1])
    C = L.SHAPES[name][1]

    def work(ctx, comm, r):
        sharded.rank_lists_shard(ctx, comm, R)
        ptr, nbytes = ctx.pack_list_table("grades")
        assert nbytes == Q * L.rp_of(R) + 4 * QPAD
        grades = np.empty(nbytes, dtype=np.uint8)
        ctx.memcpy_dtoh(grades, ptr, nbytes)
        ptr, nbytes = ctx.pack_list_table("votes", ks)
        assert nbytes == 4 * len(ks) * (C + 1) * QPAD
        votes = np.empty((len(ks), C + 1, QPAD), dtype=np.uint32)
        ctx.memcpy_dtoh(votes, ptr, nbytes)
        ctx.synchronize()
        ctx.timing_enable(True)
        merge_both(ctx, comm, ks)
        tables = list_tables(ctx, ks)
        timed = ctx.timing_read()
        ctx.timing_enable(False)
        return grades, votes, tables, timed

    ref = one_context(name, which)
    for r, (grades, votes, tables, timed) in enumerate(run_shards(name, G, work)):
        where = "%s G=%d rank %d: " % (name, G, r)
        assert np.array_equal(grades, L.grade_block(name, G, r, R)), where + "grade plane"
        assert np.array_equal(votes, L.vote_table(name, G, r, ks)), where + "vote table"
        same(tables, {k: ref[k] for k in tables}, where)
        for k in NEW_KERNELS:
            assert timed[k][1] == 1, (k, timed)
        assert timed["k_votes"][1] == 1 and timed["k_graded"][1] == 1 and timed["k_vote_confusion"][1] == 1, timed


# ------------------------------------------------------------------ 3: the merge refuses wrong input
def put(ctx, blocks, slot=0):
    buf = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(b).view(np.uint8).ravel() for b in blocks]))
    ptr = ctx.scratch(slot, buf.nbytes)
    ctx.memcpy_htod(ptr, buf, buf.nbytes)
    return ptr


def test_the_merge_refuses_fabricated_blocks():
    """Every rank of three holds all three blocks of both kinds on the host (the model's, which test 2 holds the device's against) and
    merges fabricated sets of them from a scratch buffer: an error code each time, the results of everything else untouched."""
    name, G = "b64_c81_multihot", 3
    C = L.SHAPES[name][1]
    ks = np.asarray(L.KS_LONG, dtype=np.int64)
    R, Rp, nk = N, L.rp_of(N), len(ks)
    assert Rp > R                                                             # there are pad bytes
    ref = one_context(name, "long")
    gb = [L.grade_block(name, G, r, R) for r in range(G)]
    vb = [L.vote_table(name, G, r, ks) for r in range(G)]
    zeros = {"grades": np.zeros_like(gb[0]), "votes": np.zeros_like(vb[0])}
    real = {"grades": gb, "votes": vb}

    def work(ctx, comm, r):
        sharded.rank_lists_shard(ctx, comm, R)
        sharded.merge_side_table(ctx, comm, "rel")
        sharded.merge_side_table(ctx, comm, "grade")
        side = (ctx.get_merged_rel_hist(), ctx.get_merged_grade_hist())
        merge_both(ctx, comm, ks)
        same(list_tables(ctx, ks), {k: ref[k] for k in ("graded", "grades", "votes", "pred", "conf")}, "the real blocks")
        gain, disc = X.gain_table("exp", C), X.discount_table(R)

        def merge(kind, blocks, n=G):
            ctx.merge_list_table(kind, put(ctx, blocks), n, ks if kind == "votes" else None)

        def intact(kind):
            if kind == "grades":
                ctx.graded(ks, gain, disc, keep_grades=True)
                same((ctx.get_graded(), ctx.get_grades()), (ref["graded"], ref["grades"]), "graded")
            else:
                ctx.votes(ks)
                same((ctx.get_votes(), ctx.get_vote_pred(), ctx.get_vote_confusion()), (ref["votes"], ref["pred"], ref["conf"]), "votes")

        def gone(kind):
            msg = raises(STATE, ctx.graded, ks, gain, disc) if kind == "grades" else raises(STATE, ctx.votes, ks)
            assert "whole database" in msg, msg

        def refused(kind, fabricated, flag, n=G, code=STATE):
            msg = raises(code, merge, kind, fabricated, n)
            assert flag in msg, msg
            gone(kind)                                                        # no merged table of that kind is left
            intact("votes" if kind == "grades" else "grades")                 # ... the other kind's is
            same((ctx.get_merged_rel_hist(), ctx.get_merged_grade_hist()), side, "the merged side tables")
            merge(kind, real[kind])                                           # and the real blocks merge again
            intact(kind)

        for kind in ("grades", "votes"):
            b0, b1, b2 = real[kind]
            refused(kind, [b0, b1, b1], "owned-slots")                        # a block counted twice, one missing
            refused(kind, [b0, b1, zeros[kind]], "owned-slots")               # a block zeroed
            refused(kind, [b0, b1], "owned-slots", n=2)                       # a shard missing
        # grades: a slot of shard 1 with a grade claimed by shard 0 too (own counts untouched); a byte of C + 1 in a slot shard 0 owns
        p1 = gb[1][:Q * Rp].reshape(Q, Rp)
        q, i = [int(x[0]) for x in np.nonzero(p1)]
        twice = gb[0].copy()
        twice[q * Rp + i] = 1
        refused("grades", [twice, gb[1], gb[2]], "slot-claimed-twice")
        assert "query %d" % q in raises(STATE, merge, "grades", [twice, gb[1], gb[2]])
        merge("grades", gb)
        p0 = gb[0][:Q * Rp].reshape(Q, Rp)
        q, i = [int(x[0]) for x in np.nonzero(p0)]
        high = gb[0].copy()
        high[q * Rp + i] = C + 1
        refused("grades", [high, gb[1], gb[2]], "grade-range")
        top = gb[0].copy()
        top[q * Rp + i] = C                                                   # C itself is a grade
        merge("grades", [top, gb[1], gb[2]])
        merge("grades", gb)
        # votes: a cell of a real query raised so that its sum leaves 32 bits, in a plane where another block counts rows too
        j, c, q = [int(x[0]) for x in np.nonzero(vb[1][:, :C, :Q])]
        over = vb[0].copy()
        over[j, c, q] = 0xFFFFFFFF
        refused("votes", [over, vb[1], vb[2]], "overflow")
        # poisoned pad bytes, pad queries and pad columns are ignored
        pads = [b.copy() for b in gb]
        for b in pads:
            b[:Q * Rp].reshape(Q, Rp)[:, R:] = 0xFF
            b[Q * Rp:].view(np.uint32)[Q:] = 0xFFFFFFFF
        merge("grades", pads)
        intact("grades")
        pads = [b.copy() for b in vb]
        for b in pads:
            b[:, :, Q:] = 0xFFFFFFFF
        merge("votes", pads)
        intact("votes")
        # bad arguments end the merged table of their kind, and only that one
        for kind in ("grades", "votes"):
            k = ks if kind == "votes" else None
            for bad in (lambda: ctx.merge_list_table(kind, put(ctx, real[kind]), 0, k), lambda: ctx.merge_list_table(kind, None, G, k),
                        lambda: ctx.merge_list_table(kind, put(ctx, real[kind]) + 4, G, k)):
                merge(kind, real[kind])
                raises(ARG, bad)
                gone(kind)
                intact("votes" if kind == "grades" else "grades")
            merge(kind, real[kind])
        raises(ARG, ctx.merge_list_table, 2, put(ctx, gb), G, ks)
        raises(ARG, ctx.merge_list_table, "votes", put(ctx, vb), G, None)     # votes without cut-offs
        raises(ARG, ctx.merge_list_table, "votes", put(ctx, vb), G, (7, 1))
        merge("votes", vb)
        intact("grades"), intact("votes")                                    # (no kind named: nothing ended)
        return True

    assert all(run_shards(name, G, work))


# ------------------------------------------------------------------ 4: state rules
def test_state_rules_on_a_shard():
    name, G = "b64_c81_multihot", 2
    C = L.SHAPES[name][1]
    qb, db, ql, dl = L.make(name)
    ks = np.asarray((1, 7, 500), dtype=np.int64)
    R = 500
    gain, disc = X.gain_table("exp", C), X.discount_table(R)

    def work(ctx, comm, r):
        lo, n = sharded.shard_bounds(N, G)[r]
        engine = sharded.HipShardEngine(ctx, want_lists=True)

        def ranked_and_merged():
            sharded.rank_lists_shard(ctx, comm, R)
            merge_both(ctx, comm, ks)
            ctx.graded(ks, gain, disc)
            ctx.votes(ks)
            return ctx.get_graded(), ctx.get_vote_pred()

        def ended():
            refuses_a_shard(ctx, ks)
            raises(STATE, ctx.get_graded)
            raises(STATE, ctx.get_votes)

        ctx.trim()
        bytes0 = ctx.get_stat("device_bytes")                                 # the tables alone
        refuses_a_shard(ctx)
        for kind, k in (("grades", None), ("votes", ks)):                     # the pack before a ranking with lists
            raises(STATE, ctx.pack_list_table, kind, k)
        ctx.set_option("staged_lists", 0)
        sharded.evaluate_shard(sharded.HipShardEngine(ctx, want_lists=False), comm, R, bet=False)
        assert "no ranked lists" in raises(STATE, ctx.pack_list_table, "grades")      # ... and after one without
        ctx.set_option("staged_lists", 1)
        good = ranked_and_merged()
        same(good, one_context_at(name, tuple(int(k) for k in ks)), "graded and pred")
        # arguments of the pack, and of hg_votes on the merged table
        raises(ARG, ctx.pack_list_table, 2)
        raises(ARG, ctx.pack_list_table, "votes", None)
        raises(ARG, ctx.pack_list_table, "votes", (7, 1))
        raises(ARG, ctx.pack_list_table, "votes", (1, R + 1))
        assert ctx._lib.hg_pack_list_table(ctx._h, 0, None, 0, None, None) == ARG
        ctx.pack_list_table("grades", None)                                  # grades take no cut-offs
        raises(ARG, ctx.votes, (1, 7))                                        # not the merged cut-offs
        raises(ARG, ctx.votes, (1, 7, 499))
        ctx.votes(ks)
        same(ctx.get_vote_pred(), good[1], "votes after the refused ones")
        # what does not end a merged list table: side-table passes and merges, hg_ap_at, hg_tie_ap
        ctx.rel_hist(), ctx.grade_hist(), ctx.joint_hist()
        for w in ("rel", "grade", "joint"):
            sharded.merge_side_table(ctx, comm, w)
        ctx.ap_at(ks)
        ctx.tie_ap(ks)
        ctx.graded(ks, gain, disc), ctx.votes(ks)
        same((ctx.get_graded(), ctx.get_vote_pred()), good, "after side tables, hg_ap_at and hg_tie_ap")
        # what ends it: a new ranking
        sharded.rank_lists_shard(ctx, comm, R)
        ended()
        # hg_merge_topr
        ranked_and_merged()
        ti, td = engine.topr_buffers()
        engine.merge_topr(comm.all_gather(ti), comm.all_gather(td), comm.world)
        ended()
        # a reload of the queries, of the database
        ranked_and_merged()
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        ended()
        same(ranked_and_merged(), good, "after the queries' reload")
        ctx.set_database(metric.pack_codes(db[lo:lo + n]), metric.pack_labels(dl[lo:lo + n]), db.shape[1], C, idx_base=lo, n_total=N)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        ended()
        same(ranked_and_merged(), good, "after the database's reload")
        # hg_trim; every new buffer is on the context's list
        assert ctx.get_stat("device_bytes") > bytes0
        ctx.trim()
        ended()
        assert ctx.get_stat("device_bytes") == bytes0
        same(ranked_and_merged(), good, "after hg_trim")
        return True

    assert all(run_shards(name, G, work))


@functools.lru_cache(maxsize=None)
def one_context_at(name, ks):
    """-> (get_graded(), get_vote_pred()) of one context with the whole database at the cut-offs ks (a tuple; gain "exp")."""
    ks = np.asarray(ks, dtype=np.int64)
    ctx = whole_ctx(name)
    try:
        ctx.topr(int(ks[-1]))
        ctx.graded(ks, X.gain_table("exp", ctx.C), X.discount_table(int(ks[-1])))
        ctx.votes(ks)
        return ctx.get_graded(), ctx.get_vote_pred()
    finally:
        ctx.close()


def test_the_pack_refuses_real_valued_lists():
    rng = np.random.default_rng(5)
    n, q, F, C = 2000, 8, 32, 81
    dbf = np.tanh(rng.standard_normal((n, F)) * 1.5).astype(np.float32)
    qf = np.tanh(rng.standard_normal((q, F)) * 1.5).astype(np.float32)
    dl = (rng.random((n, C)) < 0.04).astype(np.int64)
    ql = (rng.random((q, C)) < 0.06).astype(np.int64)
    ctx = _native.Context(0)
    try:
        ctx.set_option("keep_floats", 1)
        ctx.set_database_f32(dbf, dl)
        ctx.set_queries_f32(qf, ql)
        ctx.topr_real(50)
        assert "real-valued" in raises(STATE, ctx.pack_list_table, "grades")
        assert "real-valued" in raises(STATE, ctx.pack_list_table, "votes", (1, 50))
        ctx.votes((1, 50))                                                    # hg_votes itself walks such lists as before
    finally:
        ctx.close()


def test_a_whole_database_context_keeps_its_rules_and_its_outputs():
    """Pack and merge work on a whole-database context (one block); hg_graded and hg_votes there take no notice of a merged table --
    with one in place, even a fabricated one that passes the checks, their outputs are the gather's."""
    name = L.OWN
    ks = np.asarray(L.KS_LONG, dtype=np.int64)
    R = N
    ref = one_context(name, "long")
    ctx = whole_ctx(name)
    try:
        ctx.topr(R)
        before = list_tables(ctx, ks)
        same(before, {k: ref[k] for k in before}, "before")
        for kind, k, model in (("grades", None, L.grade_block(name, 1, 0, R)), ("votes", ks, L.vote_table(name, 1, 0, ks))):
            ptr, nbytes = ctx.pack_list_table(kind, k)
            got = np.empty(model.shape, dtype=model.dtype)
            ctx.memcpy_dtoh(got, ptr, nbytes)
            ctx.synchronize()
            assert np.array_equal(got, model), kind
            ctx.merge_list_table(kind, ptr, 1, k)
        same(list_tables(ctx, ks), before, "with merged tables in place")
        lying = L.grade_block(name, 1, 0, R).copy()
        plane = lying[:Q * L.rp_of(R)].reshape(Q, -1)[:, :R]
        plane[...] = np.where(plane < L.SHAPES[name][1], plane + 1, plane)                # every grade wrong, every check passed
        ctx.merge_list_table("grades", put(ctx, [lying]), 1)
        same(list_tables(ctx, ks), before, "with a wrong merged plane in place")
        raises(ARG, ctx.votes, (1, N + 1))
        ctx.votes((1, 7))                                                     # any cut-offs: the merge's bind a shard only
        ctx.trim()
        raises(STATE, ctx.pack_list_table, "grades")                          # the lists went with the work buffers
    finally:
        ctx.close()


def test_a_step_in_flight_and_the_licence_to_enqueue_blind_survive_pack_and_merge(case_cache):
    """Pack and merge of both kinds -- their first reservations -- between an hg_map that won its bet and hg_map_begin leave the licence to
    enqueue blind; with the blind step in flight the pack finds the step's state (no lists) and refuses without disturbing it; and the
    lists of hg_select_ranked are refused too."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R = c["R"]
    ks = np.asarray((100, R), dtype=np.int64)
    ctx = _native.Context(0)

    def staged():
        ctx.hist()
        ctx.plan(R)
        ctx.select()

    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        staged()                                                             # (sizes the list buffers once)
        ap0, rel0 = ctx.map(R)
        assert np.array_equal(ap0, g["ap"], equal_nan=True)
        assert ctx.get_stat("last_optimistic") == 1
        staged()
        n0 = ctx.get_stat("map_async_steps")
        for kind, k in (("grades", None), ("votes", ks)):
            ptr, nbytes = ctx.pack_list_table(kind, k)
            ctx.merge_list_table(kind, ptr, 1, k)
        ctx.map_begin(R)
        assert ctx.get_stat("map_async_steps") == n0 + 1, "pack and merge's first reservations ended the licence to enqueue blind"
        raises(STATE, ctx.pack_list_table, "grades")                          # the step's state: no lists
        ap1, rel1 = ctx.map_end()
        assert ap1.tobytes() == ap0.tobytes() and np.array_equal(rel1, rel0)
        ctx.map_begin(R)
        assert ctx.get_stat("map_async_steps") == n0 + 2
        ap1, rel1 = ctx.map_end()
        assert ap1.tobytes() == ap0.tobytes() and np.array_equal(rel1, rel0)
        assert ctx.get_stat("map_async_redone") == 0
        # the owned-slot column of the whole database's vote table is the cut-off, the query's own class the hits hg_map counted
        staged()
        ptr, nbytes = ctx.pack_list_table("votes", ks)
        tab = np.empty((2, c["dblab"].shape[1] + 1, 64), dtype=np.uint32)
        ctx.memcpy_dtoh(tab, ptr, nbytes)
        ctx.synchronize()
        assert (tab[0, -1] == 100).all() and (tab[1, -1] == R).all()
        assert np.array_equal(tab[1, c["qlab"].argmax(1), np.arange(64)].astype(np.int64), rel0)
        # local rank order
        ctx.sample_hist(R)
        ctx.guess(R)
        ctx.select_ranked()
        assert "local rank order" in raises(STATE, ctx.pack_list_table, "grades")
        ap2, rel2 = ctx.map(R)
        assert ap2.tobytes() == ap0.tobytes() and np.array_equal(rel2, rel0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5: one real communicator
@pytest.mark.parametrize("name", ["b8_c10", L.OWN])
def test_one_rank_over_rccl_equals_one_context(name):
    ql = L.make(name)[2]
    ctx = whole_ctx(name)
    try:
        try:
            comm = sharded.init_rccl(ctx, rank=0, world=1)
        except _native.HashganNativeError as e:
            pytest.skip("RCCL cannot be opened here: %s" % e)
        assert (comm.rank, comm.world) == (0, 1)
        for which, ks in KS.items():
            same(three(ctx, comm, ks, ql), reference(name, which), "%s, %s" % (name, which))
        ctx.set_option("stage_sync", 0)                                      # ranking, pack, hg_allgather and merge ordered on the one stream
        for which, ks in KS.items():
            same(three(ctx, comm, ks, ql), reference(name, which), "%s, %s, stage_sync = 0" % (name, which))
        ctx.comm_destroy()
    finally:
        ctx.close()

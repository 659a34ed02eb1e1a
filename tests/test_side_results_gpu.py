"""The five side metrics on ONE context (hg_side.hip; needs an MI355X): whose results an event ends and whose it leaves, and that
each metric's first reservations leave hg_map_begin its licence to enqueue blind.  The per-feature files check the numbers; this
one records the lifetime rules of DESIGN.md's table across the features.
"""
import numpy as np
import pytest
from tests import cases
from hashgan_amd import _native, metric
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE = _native.HG_ERR_STATE
Q, N, B, C, R = 70, 300, 33, 3, 50                     # Qpad = 128 != Q (pitched downloads), two code words
KS = (1, 7, 50)                                          # more than one plane per table
BAD = (5, 1)                                             # refused: not ascending
GETTERS = ("get_rel_hist", "get_graded", "get_grades", "get_grade_hist", "get_tie_ap", "get_ap_at")


def raw(x):
    if isinstance(x, dict):
        x = tuple(x[k] for k in sorted(x))
    return tuple(a.tobytes() for a in x) if isinstance(x, tuple) else x.tobytes()


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_an_event_ends_exactly_its_own_results():
    rng = np.random.default_rng(7)
    qc, dbc = (metric.pack_codes(rng.integers(0, 2, (n, B), dtype=np.uint8)) for n in (Q, N))
    ql, dbl = (metric.pack_labels(rng.integers(0, 2, (n, C))) for n in (Q, N))
    gain, disc = X.gain_table("exp", C), X.discount_table(KS[-1])
    ctx = _native.Context(0)

    def graded(ks=KS, keep=True):
        ctx.graded(ks, gain, disc, keep_grades=keep)

    compute = {"get_rel_hist": ctx.rel_hist, "get_graded": graded, "get_grades": graded, "get_grade_hist": ctx.grade_hist,
               "get_tie_ap": lambda: ctx.tie_ap(KS), "get_ap_at": lambda: ctx.ap_at(KS)}

    def all_five():
        for name in GETTERS:
            compute[name]()
        return {name: raw(getattr(ctx, name)()) for name in GETTERS}

    def event(what, fn, ends, refused=False):
        """`fn` ends the results of `ends` (their getters raise HG_ERR_STATE) and leaves every other getter its recorded bytes;
        what ended is computed again before the next event."""
        raises(_native.HG_ERR_ARG, fn) if refused else fn()
        for name in GETTERS:
            if name in ends:
                raises(STATE, getattr(ctx, name))
            else:
                assert raw(getattr(ctx, name)()) == want[name], (what, name)
        for again in dict.fromkeys(compute[name] for name in ends):
            again()

    def all_ended():
        for name in GETTERS:
            raises(STATE, getattr(ctx, name))

    try:
        ctx.set_database(dbc, dbl, B, C)
        ctx.set_queries(qc, ql)
        ctx.trim()
        bytes0 = ctx.get_stat("device_bytes")                                    # the tables alone
        ctx.topr(R)
        want = all_five()
        event("refused graded", lambda: graded(BAD), ("get_graded", "get_grades"), refused=True)
        event("refused tie_ap", lambda: ctx.tie_ap(BAD), ("get_tie_ap",), refused=True)
        event("refused ap_at", lambda: ctx.ap_at(BAD), ("get_ap_at",), refused=True)
        event("graded without grades", lambda: graded(keep=False), ("get_grades",))
        event("rel_hist again", ctx.rel_hist, ())
        event("a later ranking", lambda: ctx.topr(R), ("get_graded", "get_grades", "get_ap_at"))
        ctx.set_queries(qc, ql)                                                  # the same queries again: a new generation
        all_ended()
        ctx.topr(R)
        assert all_five() == want
        assert ctx.get_stat("device_bytes") > bytes0
        ctx.trim()
        all_ended()
        assert ctx.get_stat("device_bytes") == bytes0                            # every buffer of the five is on the context's list
        ctx.topr(R)
        assert all_five() == want
    finally:
        ctx.close()


def _graded(ctx, R):
    C_ = ctx.C
    ctx.graded((100, R), X.gain_table("exp", C_), X.discount_table(R))


# (name, the first call, it needs ranked lists)
FIRST_CALLS = (("rel_hist", lambda ctx, R: ctx.rel_hist(), False), ("grade_hist", lambda ctx, R: ctx.grade_hist(), False),
               ("tie_ap", lambda ctx, R: ctx.tie_ap((100, R)), False), ("ap_at", lambda ctx, R: ctx.ap_at((100, R)), False),
               ("graded", _graded, True))


def test_first_reservations_keep_the_licence_to_enqueue_blind(case_cache):
    """A side metric's first call on a context allocates its buffers; none of them is one a blind step touches, so the hg_map_begin
    after it is still enqueued blind (stat map_async_steps) and its results are the golden's.  hg_graded needs ranked lists, and
    hg_map, the only call that gives the licence, writes none: a staged sequence after it does -- without moving a buffer, once an
    earlier one has sized them all."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R = c["R"]
    ctx = _native.Context(0)

    def staged():
        ctx.hist()
        ctx.plan(R)
        ctx.select()

    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        for name, first_call, lists in FIRST_CALLS:
            if lists:
                staged()
            ap, _ = ctx.map(R)
            assert np.array_equal(ap, g["ap"], equal_nan=True), name
            assert ctx.get_stat("last_optimistic") == 1, name
            if lists:
                staged()
            n0 = ctx.get_stat("map_async_steps")
            first_call(ctx, R)
            ctx.map_begin(R)
            assert ctx.get_stat("map_async_steps") == n0 + 1, "%s: its first reservations ended the licence to enqueue blind" % name
            ap, _ = ctx.map_end()
            assert np.array_equal(ap, g["ap"], equal_nan=True), name
            assert ctx.get_stat("map_async_redone") == 0, name
    finally:
        ctx.close()

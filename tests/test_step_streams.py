"""hg_map_begin / hg_map_end with the option "step_streams": slot 1's blind steps on a second stream of the context, in a
workspace of their own, overlapping the step before them.  Results must be those of hg_map, bit for bit, in every order of
calls; the Python wrapper's bookkeeping of the steps in flight must survive a failing hg_map_end (CPU test below)."""
import numpy as np
import pytest
from tests import cases
from hashgan_amd import _native, metric


def _load(ctx, c):
    ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
    ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))


def _queries(ctx, c, sel):
    ctx.set_queries(metric.pack_codes(c["qbits"][sel].copy()), metric.pack_labels(c["qlab"][sel].copy()))


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@pytest.fixture
def c2(case_cache):
    return case_cache("c2_q64"), cases.load_golden("c2_q64")


@pytest.mark.gpu
def test_two_tables_alternating_equal_map(c2):
    """begin, begin, end, end over two alternating query tables -- of the same count (the steps stay blind, slot 1 on the second
    stream) and of different counts (every begin runs the call itself) -- each step equal to the synchronous hg_map."""
    c, g = c2
    R = c["R"]
    fwd, rev, few = slice(None), slice(None, None, -1), slice(0, 37)
    ctx = _native.Context(0)
    try:
        _load(ctx, c)
        want = {}
        for name, sel in (("fwd", fwd), ("rev", rev), ("few", few)):
            _queries(ctx, c, sel)
            want[name] = ctx.map(R)
        assert np.array_equal(want["fwd"][0], g["ap"], equal_nan=True)
        for pair in (("fwd", "rev"), ("fwd", "few")):
            sels = {"fwd": fwd, "rev": rev, "few": few}
            _queries(ctx, c, sels[pair[0]])
            ctx.map(R)                                     # (warm: the next begin may enqueue blind)
            n0 = ctx.get_stat("map_overlapped_steps")
            for k in range(4):
                _queries(ctx, c, sels[pair[0]])
                ctx.map_begin(R)
                _queries(ctx, c, sels[pair[1]])
                ctx.map_begin(R)
                got0 = ctx.map_end()
                got1 = ctx.map_end()
                assert _same(got0, want[pair[0]]), (pair, k, 0)
                assert _same(got1, want[pair[1]]), (pair, k, 1)
            if pair == ("fwd", "rev") and ctx.get_stat("last_optimistic"):
                assert ctx.get_stat("map_overlapped_steps") > n0, "slot 1's blind steps never ran on the second stream"
        assert ctx.get_stat("map_async_redone") == 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_lost_bet_beside_a_step_in_flight(c2):
    """A blind step that loses its bet (test hook "handicap_next_bet") while the other slot's step is in flight -- the loser on the
    second stream, then on the context's own -- is run again by hg_map_end; both steps' results equal hg_map's."""
    c, g = c2
    R = c["R"]
    ctx = _native.Context(0)
    try:
        _load(ctx, c)
        ap0, rel0 = ctx.map(R)
        assert np.array_equal(ap0, g["ap"], equal_nan=True)
        assert ctx.get_stat("last_optimistic"), "the bet applies to this shape"
        redone = ctx.get_stat("map_async_redone")
        # slots alternate from 0 (a fresh context; two begins and two ends per round leave it so): the loser in slot 1 runs on
        # the second stream behind a won slot-0 step, the loser in slot 0 has a slot-1 step in flight beside its rerun
        for loser in (1, 0, 1, 0):
            if loser == 1:
                ctx.map_begin(R)
                ctx.set_option("handicap_next_bet", 12)
                ctx.map_begin(R)
            else:
                ctx.set_option("handicap_next_bet", 12)
                ctx.map_begin(R)
                ctx.map_begin(R)
            a1, r1 = ctx.map_end()
            a2, r2 = ctx.map_end()
            assert _same((a1, r1), (ap0, rel0)) and _same((a2, r2), (ap0, rel0)), loser
            redone += 1
            assert ctx.get_stat("map_async_redone") == redone, loser
        assert _same(ctx.map(R), (ap0, rel0))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_set_queries_between_begin_and_end(c2):
    """The query table replaced (same count) while both steps are in flight: each step answers for the table it was enqueued on,
    and the next steps for the new one."""
    c, g = c2
    R = c["R"]
    ctx = _native.Context(0)
    try:
        _load(ctx, c)
        ap0, rel0 = ctx.map(R)
        _queries(ctx, c, slice(None, None, -1))
        ap_rev, rel_rev = ctx.map(R)
        _queries(ctx, c, slice(None))
        ctx.map(R)
        for k in range(3):
            ctx.map_begin(R)
            ctx.map_begin(R)
            _queries(ctx, c, slice(None, None, -1))
            assert _same(ctx.map_end(), (ap0, rel0)), k
            ctx.map_begin(R)
            _queries(ctx, c, slice(None))
            assert _same(ctx.map_end(), (ap0, rel0)), k
            assert _same(ctx.map_end(), (ap_rev, rel_rev)), k
        assert np.array_equal(ap_rev, g["ap"][::-1], equal_nan=True)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_one_and_two_streams_identical(c2):
    """step_streams = 1 and 2: the same pipelined sequence gives byte-identical APs and hit counts, and with 2 the second stream
    carries slot 1's blind steps (with 1 it carries none)."""
    c, _ = c2
    R = c["R"]
    out = {}
    for streams in (1, 2):
        ctx = _native.Context(0)
        try:
            _load(ctx, c)
            ctx.set_option("step_streams", streams)
            ctx.map(R)
            res = []
            ctx.map_begin(R)
            for i in range(8):
                if i + 1 < 8:
                    ctx.map_begin(R)
                res.append(ctx.map_end())
            ctx.synchronize()
            out[streams] = res
            n = ctx.get_stat("map_overlapped_steps")
            if streams == 1:
                assert n == 0
            elif ctx.get_stat("last_optimistic"):
                assert n >= 3
        finally:
            ctx.close()
    for (a1, r1), (a2, r2) in zip(out[1], out[2]):
        assert a1.tobytes() == a2.tobytes() and r1.tobytes() == r2.tobytes()
    with pytest.raises(_native.HashganNativeError):
        ctx = _native.Context(0)
        try:
            ctx.set_option("step_streams", 3)
        finally:
            ctx.close()


@pytest.mark.gpu
def test_device_bytes_count_the_second_workspace(c2):
    """Batch after batch through hg_map_begin / hg_map_end with one and with two streams: the second stream's workspace is held by
    the context (stat "device_bytes" counts it), and hg_trim gives it back -- both contexts then hold their tables alone, what
    they held after loading them and trimming."""
    c, _ = c2
    R = c["R"]
    fwd, rev = slice(None), slice(None, None, -1)
    held, tables, trimmed = {}, {}, {}
    for streams in (1, 2):
        ctx = _native.Context(0)
        try:
            _load(ctx, c)
            ctx.set_option("step_streams", streams)
            ctx.trim()
            tables[streams] = ctx.get_stat("device_bytes")
            ctx.map(R)                                     # (warm: the next begin may enqueue blind)
            for k in range(3):
                _queries(ctx, c, fwd)
                ctx.map_begin(R)
                _queries(ctx, c, rev)
                ctx.map_begin(R)
                ctx.map_end()
                ctx.map_end()
            ctx.synchronize()
            if streams == 2:
                assert ctx.get_stat("map_overlapped_steps") >= 1
            held[streams] = ctx.get_stat("device_bytes")
            ctx.trim()
            trimmed[streams] = ctx.get_stat("device_bytes")
        finally:
            ctx.close()
    assert held[2] > held[1], held
    assert trimmed[1] == trimmed[2] == tables[1] == tables[2], (trimmed, tables)


class _FailingEnd:
    """Stand-in for the library: hg_map_end fails (as when a lost step's tables were replaced)."""

    def hg_map_end(self, h, ap, rel):
        return _native.HG_ERR_STATE

    def hg_last_error(self):
        return b"stub: tables replaced"


def test_map_end_error_drops_the_in_flight_entry(monkeypatch):
    """hg_map_end dequeues the step whatever it returns; the wrapper must too, or the next map_end sizes its arrays from a stale
    entry (another query count) and the library writes past them."""
    stub = _FailingEnd()
    monkeypatch.setattr(_native, "load", lambda: stub)
    ctx = _native.Context.__new__(_native.Context)
    ctx._lib = stub
    ctx._h = None
    ctx.Q = 10
    ctx._in_flight = [64, 10]
    with pytest.raises(_native.HashganNativeError):
        ctx.map_end()
    assert ctx._in_flight == [10]
    with pytest.raises(_native.HashganNativeError):
        ctx.map_end()
    assert ctx._in_flight == []

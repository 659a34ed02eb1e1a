"""The control flow of hashgan_amd.sharded.evaluate_shard, pinned call by call (CPU, no threads, no processes): which engine
methods run, in which order, between which exchanges, and what comes back -- for the exact sequence, the candidates bet, the four
exchanges of the ranked bet (held / lost and widened / lost and given up) and the first-call self-check of the owner-routed form
over an RcclComm.

A recording engine appends the name of every call to a trace and answers `lost`, the deferred verdict and widen_slices() from
scripts; a one-thread communicator (world 2) appends "g" for an all_gather and "a" for an all_to_all and hands back a tagged
tuple.  The RCCL-only branches run over a real sharded.RcclComm on a recording context.  An engine is composed of one mixin per
form of the bet, so it has a form's methods exactly when it declares the form (`bet_forms`)."""
import numpy as np
import pytest

from hashgan_amd import sharded
from hashgan_amd.sharded import DevBuf

EXACT = ["hist", "g", "plan", "select_match", "g"]
CANDIDATES = ["sample_hist", "g", "guess", "select_candidates", "g", "rank_candidates"]
GUARD = ["ranked_merge_ok", "bet_eligible"]
WHOLE_1 = ["sample_hist", "guess", "select_ranked", "merge_ranked"]                      # one rank: nothing is exchanged
SPLIT = ["sample_hist", "g", "guess", "select_ranked", "g", "g", "merge_ap_part", "g", "unpack_parts"]
ROUTED = ["sample_hist", "pack_sample_by_owner", "a", "guess_owned", "a", "guess_finish", "select_ranked", "pack_ranked_by_owner", "a",
          "merge_ap_owned", "g", "unpack_parts"]
ONE_CALL = ["shard_step"]


class _Scripted:
    """What every recording engine has: the trace, the scripts, and a result per finishing call (1.0, 2.0, ... unless scripted)."""

    def __init__(self, trace=None, lost=(), verdicts=(), widen=(), values=(), eligible=True, merge_ok=True):
        self.trace = [] if trace is None else trace
        self.lost, self.verdicts, self.widen, self.values = list(lost), list(verdicts), list(widen), list(values)
        self.eligible, self.merge_ok = eligible, merge_ok
        self.args = {}
        self.results = 0
        self.ctx = self

    def _call(self, name, *args):
        self.trace.append(name)
        self.args[name] = args
        return DevBuf(name, 8)

    def _result(self):
        self.results += 1
        v = self.values.pop(0) if self.values else float(self.results)
        return np.array([v, np.nan]), np.array([int(v) if v == v else 0, 0], dtype=np.int64)

    # (the library's own list exchange, reached through engine.ctx over an RcclComm or with one rank)
    def allgather_topr(self):
        self.trace.append("ctx.allgather_topr")

    def get_topr(self):
        self.trace.append("ctx.get_topr")
        return "ctx lists"


class _Exact(_Scripted):
    def hist(self):
        return self._call("hist")

    def plan(self, R, gathered, world, rank):
        self._call("plan", R, gathered, world, rank)

    def select_match(self):
        return self._call("select_match")

    def match_bits(self):
        return self._call("match_bits")

    def verdict(self):
        self.trace.append("verdict")
        return self.verdicts.pop(0)

    def finish(self, gathered_bits, world):
        self._call("finish", gathered_bits, world)
        return self._result()

    def topr_buffers(self):
        self.trace.append("topr_buffers")
        return DevBuf("idx", 32), DevBuf("dist", 8)

    def merge_topr(self, gathered_idx, gathered_dist, world):
        self._call("merge_topr", gathered_idx, gathered_dist, world)
        return "merged lists"


class _Bet:
    def bet_eligible(self, R, world):
        self.trace.append("bet_eligible")
        return self.eligible

    def sample_hist(self, R):
        return self._call("sample_hist", R)

    def guess(self, R, gathered, world, rank):
        self._call("guess", R, gathered, world, rank)


class _Candidates(_Bet):
    def select_candidates(self):
        return self._call("select_candidates")

    def rank_candidates(self, gathered, world, rank):
        self._call("rank_candidates", gathered, world, rank)
        return self.lost.pop(0)


class _Ranked(_Bet):
    def ranked_merge_ok(self, world):
        self.trace.append("ranked_merge_ok")
        return self.merge_ok

    def widen_slices(self):
        self.trace.append("widen_slices")
        return self.widen.pop(0)

    def select_ranked(self):
        self.trace.append("select_ranked")
        return DevBuf("counts", 8), DevBuf("local bits", 8)

    def merge_ranked(self, gathered_hist, gathered_bits, world):
        self._call("merge_ranked", gathered_hist, gathered_bits, world)
        return self.lost.pop(0)


class _Split:
    def merge_ap_part(self, gathered_hist, gathered_bits, world, rank):
        return self._call("merge_ap_part", gathered_hist, gathered_bits, world, rank)

    def unpack_parts(self, gathered_parts, world):
        self._call("unpack_parts", gathered_parts, world)
        return self._result() + (self.lost.pop(0),)


class _Routed:
    def pack_sample_by_owner(self, world):
        return self._call("pack_sample_by_owner", world)

    def guess_owned(self, R, received, world, rank):
        return self._call("guess_owned", R, received, world, rank)

    def guess_finish(self, R, answers, world, rank):
        self._call("guess_finish", R, answers, world, rank)

    def pack_ranked_by_owner(self, world):
        return self._call("pack_ranked_by_owner", world)

    def merge_ap_owned(self, received, world, rank):
        if self.routed_raises:
            raise RuntimeError("hg_alltoall failed on this rank")
        return self._call("merge_ap_owned", received, world, rank)

    routed_raises = False


class _OneCall:
    def shard_step(self, R):
        self._call("shard_step", R)
        return self._result() + (self.lost.pop(0),)


_MIXINS = {"candidates": _Candidates, "ranked": _Ranked, "split": _Split, "routed": _Routed, "one_call": _OneCall}
ALL = ("candidates", "ranked", "split", "routed", "one_call")


def engine(forms, **script):
    """A recording engine that declares -- and has the methods of -- exactly `forms`."""
    cls = type("Engine", tuple(_MIXINS[f] for f in forms) + (_Exact,), {"bet_forms": frozenset(forms)})
    return cls(**script)


class Comm:
    """One thread's view of a `world`-rank communicator: every exchange is recorded and answered with a tagged tuple."""

    def __init__(self, trace, world=2):
        self.trace, self.rank, self.world = trace, 0, world

    def all_gather(self, buf):
        self.trace.append("g")
        return ("gathered", buf)

    def all_to_all(self, buf):
        self.trace.append("a")
        return ("routed", buf)

    def barrier(self):
        pass

    def all_gather_host(self, arr):
        return np.stack([arr] * self.world)


class RcclCtx:
    """The four calls sharded.RcclComm makes on its context."""

    def __init__(self, trace, world=2):
        self.trace, self.world, self.reduced = trace, world, []

    def comm_info(self):
        return 0, self.world

    def allgather(self, slot, ptr, nbytes):
        self.trace.append("g")
        return ("gathered", ptr)

    def alltoall(self, slot, ptr, nbytes):
        self.trace.append("a")
        return ("routed", ptr)

    def allreduce_max(self, x):
        self.trace.append("allreduce_max")
        self.reduced.append(x)
        return x


def run(forms, world=2, rccl=False, script=None, **kw):
    """-> (engine, comm, what evaluate_shard(engine, comm, 100, **kw) returned)"""
    eng = engine(forms, **(script or {}))
    comm = sharded.RcclComm(RcclCtx(eng.trace, world)) if rccl else Comm(eng.trace, world)
    return eng, comm, sharded.evaluate_shard(eng, comm, 100, **kw)


def value(out):
    return out[0][0]


# ------------------------------------------------------------------ exact sequence
@pytest.mark.parametrize("forms", [(), ALL])
def test_exact_sequence(forms):
    eng, _, out = run(forms, bet=False)
    assert eng.trace == EXACT + ["finish"] and len(out) == 2 and value(out) == 1.0
    assert eng.args["plan"] == (100, ("gathered", DevBuf("hist", 8)), 2, 0)
    assert eng.args["finish"] == (("gathered", DevBuf("select_match", 8)), 2)


def test_exact_sequence_is_what_an_engine_without_forms_gets():
    eng, _, out = run(())
    assert eng.trace == EXACT + ["finish"] and value(out) == 1.0


def test_exact_sequence_with_one_rank_exchanges_nothing():
    eng, _, out = run((), world=1, bet=False)
    assert eng.trace == ["hist", "plan", "select_match", "finish"]
    assert eng.args["plan"] == (100, None, 1, 0) and eng.args["finish"] == (None, 1)
    eng, _, out = run((), world=1, bet=False, always_gather=True)
    assert eng.trace == EXACT + ["finish"]


def test_exact_sequence_with_the_lists_gathered():
    eng, _, out = run((), bet=False, gather_topr=True)
    assert eng.trace == EXACT + ["topr_buffers", "g", "g", "merge_topr", "finish"]
    assert len(out) == 3 and value(out) == 1.0 and out[2] == "merged lists"
    assert eng.args["merge_topr"] == (("gathered", DevBuf("idx", 32)), ("gathered", DevBuf("dist", 8)), 2)
    eng, _, out = run((), bet=False, gather_topr=True, rccl=True)             # the list exchange inside the library
    assert eng.trace == EXACT + ["ctx.allgather_topr", "ctx.get_topr", "finish"] and out[2] == "ctx lists"
    eng, _, out = run((), bet=False, gather_topr=True, world=1)               # one rank: its lists are the lists
    assert eng.trace == ["hist", "plan", "select_match", "ctx.get_topr", "finish"] and out[2] == "ctx lists"


# ------------------------------------------------------------------ candidates bet
HELD = ["bet_eligible"] + CANDIDATES + ["match_bits", "g"]


@pytest.mark.parametrize("forms,kw", [(("candidates",), {}), (ALL, {"gather_topr": True})])
def test_candidates_bet_held(forms, kw):
    eng, _, out = run(forms, script=dict(lost=[False]), **kw)
    lists = ["topr_buffers", "g", "g", "merge_topr"] if kw else []
    assert eng.trace == HELD + lists + ["finish"] and value(out) == 1.0 and len(out) == (3 if kw else 2)
    assert eng.args["guess"] == (100, ("gathered", DevBuf("sample_hist", 8)), 2, 0)
    assert eng.args["rank_candidates"] == (("gathered", DevBuf("select_candidates", 8)), 2, 0)
    assert eng.args["finish"] == (("gathered", DevBuf("match_bits", 8)), 2)


def test_candidates_bet_is_what_an_engine_that_does_not_rank_locally_takes():
    eng, _, out = run(("candidates",), script=dict(lost=[False]))
    assert eng.trace == HELD + ["finish"]


def test_candidates_bet_not_eligible_is_the_exact_sequence():
    eng, _, out = run(("candidates",), script=dict(eligible=False))
    assert eng.trace == ["bet_eligible"] + EXACT + ["finish"]


def test_candidates_bet_lost_runs_the_exact_sequence_once_and_widens_nothing():
    eng, _, out = run(("candidates",), script=dict(lost=[True]))
    assert eng.trace == ["bet_eligible"] + CANDIDATES + EXACT + ["finish"] and value(out) == 1.0
    assert eng.args["finish"] == (("gathered", DevBuf("select_match", 8)), 2)
    eng, _, out = run(ALL, gather_topr=True, script=dict(lost=[True]))
    assert eng.trace == ["bet_eligible"] + CANDIDATES + EXACT + ["topr_buffers", "g", "g", "merge_topr", "finish"]


def test_candidates_bet_deferred_verdict_comes_after_the_finish():
    eng, _, out = run(("candidates",), script=dict(lost=[None], verdicts=[False]))
    assert eng.trace == HELD + ["finish", "verdict"] and value(out) == 1.0
    eng, _, out = run(("candidates",), script=dict(lost=[None], verdicts=[True]))
    assert eng.trace == HELD + ["finish", "verdict"] + EXACT + ["finish"]
    assert value(out) == 2.0                                                  # the second finish's result
    assert eng.args["finish"] == (("gathered", DevBuf("select_match", 8)), 2)


def test_candidates_bet_deferred_verdict_comes_before_the_lists():
    eng, _, out = run(ALL, gather_topr=True, script=dict(lost=[None], verdicts=[False]))
    assert eng.trace == HELD + ["verdict", "topr_buffers", "g", "g", "merge_topr", "finish"] and len(out) == 3
    eng, _, out = run(ALL, gather_topr=True, script=dict(lost=[None], verdicts=[True]))
    assert eng.trace == HELD + ["verdict"] + EXACT + ["topr_buffers", "g", "g", "merge_topr", "finish"] and value(out) == 1.0


# ------------------------------------------------------------------ ranked bet: the guard
def test_ranked_guard_is_asked_once_merge_limits_first():
    eng, _, out = run(ALL, script=dict(lost=[False]))
    assert eng.trace[:2] == GUARD and eng.trace.count("bet_eligible") == 1
    # the merge's limits exceeded: the bet is not asked about here, and the candidates bet asks for itself
    eng, _, out = run(ALL, script=dict(merge_ok=False, lost=[False]))
    assert eng.trace == ["ranked_merge_ok"] + HELD + ["finish"]
    # not eligible: both bets ask, neither runs
    eng, _, out = run(ALL, script=dict(eligible=False))
    assert eng.trace == GUARD + ["bet_eligible"] + EXACT + ["finish"]


# ------------------------------------------------------------------ ranked bet: the four exchanges, three outcomes each
def whole(verdicts=()):
    return WHOLE_1 + ["finish"] + ["verdict"] * len(verdicts)


EXCHANGES = {
    # name: (forms, world, rccl, keywords, one attempt's trace)
    "whole": (("ranked",), 1, False, {}, WHOLE_1),
    "whole_of_all": (ALL, 1, False, {}, WHOLE_1),
    "whole_2": (("ranked",), 2, False, {}, ["sample_hist", "g", "guess", "select_ranked", "g", "g", "merge_ranked"]),
    "split": (("ranked", "split"), 2, False, {}, SPLIT),
    "split_unrouted": (ALL, 2, False, {"route_by_owner": False}, SPLIT),
    "split_one_rank": (ALL, 1, False, {"always_gather": True, "route_by_owner": False}, SPLIT),
    "routed": (("ranked", "split", "routed"), 2, False, {}, ROUTED),
    "routed_no_rccl": (ALL, 2, False, {}, ROUTED),                            # one call needs the library's own communicator
    "routed_staged": (ALL, 2, True, {"one_call": False, "route_by_owner": True}, ROUTED),
    "routed_one_rank": (ALL, 1, True, {"one_call": False, "always_gather": True}, ROUTED),
    "one_call": (ALL, 1, True, {"always_gather": True}, ONE_CALL),
}


def exchange(name, script, monkeypatch):
    forms, world, rccl, kw, attempt = EXCHANGES[name]
    monkeypatch.setenv("HG_ROUTE_BY_OWNER", "1")                             # (world 2 over RCCL: no self-check here)
    eng, _, out = run(forms, world=world, rccl=rccl, script=script, **kw)
    tail = [] if attempt[-1] in ("unpack_parts", "shard_step") else ["finish"]
    return eng, out, attempt, tail


@pytest.mark.parametrize("name", sorted(EXCHANGES))
def test_ranked_bet_held(name, monkeypatch):
    eng, out, attempt, tail = exchange(name, dict(lost=[False]), monkeypatch)
    assert eng.trace == GUARD + attempt + tail and len(out) == 2 and value(out) == 1.0
    if tail:
        assert eng.args["finish"][0] is None                                 # merged already: nothing to OR


@pytest.mark.parametrize("name", sorted(EXCHANGES))
def test_ranked_bet_lost_widens_and_bets_again_without_asking_again(name, monkeypatch):
    eng, out, attempt, tail = exchange(name, dict(lost=[True, False], widen=[True]), monkeypatch)
    assert eng.trace == GUARD + attempt + ["widen_slices"] + attempt + tail
    assert value(out) == (1.0 if tail else 2.0)                               # the second attempt's result
    eng, out, attempt, tail = exchange(name, dict(lost=[True, True, False], widen=[True, True]), monkeypatch)
    assert eng.trace == GUARD + (attempt + ["widen_slices"]) * 2 + attempt + tail


@pytest.mark.parametrize("name", sorted(EXCHANGES))
def test_ranked_bet_lost_and_not_widened_is_the_exact_sequence_never_the_candidates_bet(name, monkeypatch):
    eng, out, attempt, tail = exchange(name, dict(lost=[True], widen=[False]), monkeypatch)
    exact = EXACT if "g" in attempt or "a" in attempt or EXCHANGES[name][3].get("always_gather") else ["hist", "plan", "select_match"]
    assert eng.trace == GUARD + attempt + ["widen_slices"] + exact + ["finish"]
    assert value(out) == (1.0 if tail else 2.0)
    eng, out, attempt, tail = exchange(name, dict(lost=[True, True], widen=[True, False]), monkeypatch)
    assert eng.trace == GUARD + (attempt + ["widen_slices"]) * 2 + exact + ["finish"]


@pytest.mark.parametrize("name", ["whole", "whole_2"])
def test_whole_merge_deferred_verdict(name, monkeypatch):
    eng, out, attempt, _ = exchange(name, dict(lost=[None], verdicts=[False]), monkeypatch)
    assert eng.trace == GUARD + attempt + ["finish", "verdict"] and value(out) == 1.0
    eng, out, attempt, _ = exchange(name, dict(lost=[None, None], verdicts=[True, False], widen=[True]), monkeypatch)
    assert eng.trace == GUARD + attempt + ["finish", "verdict", "widen_slices"] + attempt + ["finish", "verdict"] and value(out) == 2.0
    eng, out, attempt, _ = exchange(name, dict(lost=[None], verdicts=[True], widen=[False]), monkeypatch)
    exact = EXACT if "g" in attempt else ["hist", "plan", "select_match"]
    assert eng.trace == GUARD + attempt + ["finish", "verdict", "widen_slices"] + exact + ["finish"] and value(out) == 2.0
    eng, out, attempt, _ = exchange(name, dict(lost=[False]), monkeypatch)
    assert "verdict" not in eng.trace                                        # a verdict that was not deferred is not asked for


def test_one_call_that_took_no_bet_goes_exact_without_widening(monkeypatch):
    eng, out, attempt, _ = exchange("one_call", dict(lost=[None]), monkeypatch)
    assert eng.trace == GUARD + ONE_CALL + EXACT + ["finish"] and value(out) == 2.0


def test_what_travels_in_the_routed_exchanges(monkeypatch):
    eng, out, _, _ = exchange("routed", dict(lost=[False]), monkeypatch)
    a = eng.args
    assert a["guess_owned"] == (100, ("routed", DevBuf("pack_sample_by_owner", 8)), 2, 0)
    assert a["guess_finish"] == (100, ("routed", DevBuf("guess_owned", 8)), 2, 0)
    assert a["merge_ap_owned"] == (("routed", DevBuf("pack_ranked_by_owner", 8)), 2, 0)
    assert a["unpack_parts"] == (("gathered", DevBuf("merge_ap_owned", 8)), 2)
    eng, out, _, _ = exchange("split", dict(lost=[False]), monkeypatch)
    assert eng.args["merge_ap_part"] == (("gathered", DevBuf("counts", 8)), ("gathered", DevBuf("local bits", 8)), 2, 0)
    assert eng.args["unpack_parts"] == (("gathered", DevBuf("merge_ap_part", 8)), 2)


def test_gathered_lists_or_no_bet_never_take_the_ranked_bet():
    eng, _, out = run(ALL, gather_topr=True, script=dict(lost=[False]))
    assert "ranked_merge_ok" not in eng.trace and "select_ranked" not in eng.trace
    eng, _, out = run(ALL, bet=False)
    assert eng.trace == EXACT + ["finish"]


# ------------------------------------------------------------------ first-call self-check of the routed form (RcclComm, world > 1)
ALLGATHER_RUN = GUARD + SPLIT
ROUTED_RUN = GUARD + ONE_CALL


@pytest.fixture
def no_force(monkeypatch):
    monkeypatch.delenv("HG_ROUTE_BY_OWNER", raising=False)


def test_self_check_runs_both_forms_and_returns_the_all_gather_result(no_force):
    eng, comm, out = run(ALL, rccl=True, script=dict(lost=[False, False], values=[7.0, 7.0]))
    assert eng.trace == ALLGATHER_RUN + ROUTED_RUN + ["allreduce_max"]
    assert comm.ctx.reduced == [0.0] and comm.routed_verified is True and value(out) == 7.0
    eng.trace.clear()
    eng.lost = [False]
    sharded.evaluate_shard(eng, comm, 100)                                   # later calls: routed, no check
    assert eng.trace == ROUTED_RUN
    eng, comm, out = run(ALL, rccl=True, one_call=False, script=dict(lost=[False, False], values=[7.0, 7.0]))
    assert eng.trace == ALLGATHER_RUN + GUARD + ROUTED + ["allreduce_max"] and comm.routed_verified is True


def test_self_check_a_difference_keeps_the_all_gather_form(no_force):
    for values in ([7.0, 8.0], [np.nan, 7.0]):
        eng, comm, out = run(ALL, rccl=True, script=dict(lost=[False, False], values=list(values)))
        assert eng.trace == ALLGATHER_RUN + ROUTED_RUN + ["allreduce_max"]
        assert comm.ctx.reduced == [1.0] and comm.routed_verified is False
        assert np.array_equal(out[0], [values[0], np.nan], equal_nan=True)
        eng.trace.clear()
        eng.lost = [False]
        sharded.evaluate_shard(eng, comm, 100)
        assert eng.trace == ALLGATHER_RUN


def test_self_check_swallows_an_error_of_the_routed_run_and_tells_the_ranks(no_force):
    eng = engine(ALL, lost=[False], values=[7.0])
    eng.routed_raises = True
    comm = sharded.RcclComm(RcclCtx(eng.trace))
    out = sharded.evaluate_shard(eng, comm, 100, one_call=False)
    assert eng.trace == ALLGATHER_RUN + GUARD + ROUTED[:ROUTED.index("merge_ap_owned")] + ["allreduce_max"]
    assert comm.ctx.reduced == [2.0] and comm.routed_verified is False and value(out) == 7.0


def test_self_check_another_ranks_error_is_learnt_from_the_reduction(no_force):
    eng = engine(ALL, lost=[False, False], values=[7.0, 7.0])
    ctx = RcclCtx(eng.trace)
    ctx.allreduce_max = lambda x: 2.0
    comm = sharded.RcclComm(ctx)
    sharded.evaluate_shard(eng, comm, 100)
    assert comm.routed_verified is False


@pytest.mark.parametrize("forced,attempt", [("0", SPLIT), ("1", ONE_CALL)])
def test_self_check_is_skipped_when_the_form_is_forced(forced, attempt, monkeypatch):
    monkeypatch.setenv("HG_ROUTE_BY_OWNER", forced)
    eng, comm, out = run(ALL, rccl=True, script=dict(lost=[False]))
    assert eng.trace == GUARD + attempt and comm.routed_verified is None


def test_self_check_is_never_entered_without_the_ranked_routed_bet(no_force):
    for kw, forms in (({"gather_topr": True}, ALL), ({"bet": False}, ALL), ({"route_by_owner": False}, ALL), ({}, ("ranked", "split")),
                      ({}, ("candidates",))):
        eng, comm, out = run(forms, rccl=True, script=dict(lost=[False]), **kw)
        assert "allreduce_max" not in eng.trace and comm.routed_verified is None, kw
    eng, comm, out = run(ALL, rccl=True, world=1, always_gather=True, script=dict(lost=[False]))      # one rank: nothing to verify
    assert eng.trace == ROUTED_RUN and comm.routed_verified is None
    eng, comm, out = run(ALL, script=dict(lost=[False]))                                              # not the library's communicator
    assert eng.trace == GUARD + ROUTED and "allreduce_max" not in eng.trace

"""What an engine declares is what hashgan_amd.sharded.evaluate_shard calls (CPU): the defaults of sharded.ShardEngine, the forms the
engines of this repository declare, and that a declared form whose method is missing fails loudly instead of falling through to a
slower sequence.  The sequences themselves: tests/test_shard_orchestration.py."""
import pytest

from hashgan_amd import sharded
from tests.test_shard_orchestration import Comm, EXACT, RcclCtx, engine


def test_defaults_of_the_base_class():
    e = sharded.ShardEngine()
    assert e.bet_forms == frozenset()
    assert e.bet_eligible(100, 2) is False and e.ranked_merge_ok(2) is False and e.widen_slices() is False


def test_what_the_engines_declare():
    from tests import numpy_shard_engine as N
    assert sharded.HipShardEngine.bet_forms == sharded.BET_FORMS == {"candidates", "ranked", "split", "routed", "one_call"}
    assert N.NumpyShardEngine.bet_forms == frozenset()
    assert N.NumpyRankedEngine.bet_forms == {"ranked", "split"}
    assert N.NumpyRoutedEngine.bet_forms == {"ranked", "split", "routed"}
    for cls in (sharded.HipShardEngine, N.NumpyShardEngine, N.NumpyRankedEngine, N.NumpyRoutedEngine):
        assert issubclass(cls, sharded.ShardEngine)


def test_a_misspelt_form_is_refused_where_it_is_declared():
    with pytest.raises(TypeError, match="routd"):
        type("Engine", (sharded.ShardEngine,), {"bet_forms": ("ranked", "routd")})


@pytest.mark.parametrize("has,declares,missing", [((), "candidates", "bet_eligible"), (("candidates",), "ranked", "ranked_merge_ok"),
                                                  (("ranked",), "split", "merge_ap_part"), (("ranked", "split"), "routed", "guess_owned"),
                                                  (("ranked", "split", "routed"), "one_call", "shard_step")])
def test_a_declared_form_whose_method_is_missing_fails_loudly(has, declares, missing, monkeypatch):
    """An engine with the methods of `has` that also declares `declares`: the first missing method raises."""
    eng = engine(has, lost=[False])
    eng.bet_forms = frozenset(has + (declares,))
    comm = Comm(eng.trace)
    if declares == "one_call":                                                # (needs the library's own communicator)
        monkeypatch.setenv("HG_ROUTE_BY_OWNER", "1")
        comm = sharded.RcclComm(RcclCtx(eng.trace))
    with pytest.raises(AttributeError, match=missing):
        sharded.evaluate_shard(eng, comm, 100)
    assert "hist" not in eng.trace and "finish" not in eng.trace              # ... and nothing went on to another sequence


def test_an_undeclared_form_is_never_called():
    eng = engine(("candidates", "ranked", "split", "routed", "one_call"))
    eng.bet_forms = frozenset()
    sharded.evaluate_shard(eng, Comm(eng.trace), 100)
    assert eng.trace == EXACT + ["finish"]


def test_an_engine_that_declares_nothing_at_all_gets_the_exact_sequence():
    """No `bet_forms` and not a ShardEngine -- the NumPy engines as they were before engines declared their forms: whatever methods
    it has, only the exact sequence is asked of it."""
    eng = engine(("candidates", "ranked", "split", "routed", "one_call"))
    del type(eng).bet_forms
    out = sharded.evaluate_shard(eng, Comm(eng.trace), 100)
    assert eng.trace == EXACT + ["finish"] and out[0][0] == 1.0

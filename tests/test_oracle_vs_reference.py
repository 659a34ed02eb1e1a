"""The oracle against the unmodified reference on seeded inputs: the reference's own results were recorded by
tests/golden/make_golden.py (reference_live.npz: `MAPs(R).get_maps_by_feature` of lib/metric.py on exactly these inputs,
and the exception it raises for R > N), so the comparison runs wherever the repository does."""
import types
import warnings
import numpy as np
import pytest
from oracle import hamming_map as O
from hashgan_amd import synth
from tests import cases

# (Q, N, b, R, C, multi-hot labels)
LIVE_CASES = [(30, 5000, 32, 5000, 10, False), (25, 8000, 64, 1000, 10, False),
              (20, 6000, 48, 900, 81, True), (10, 3000, 128, 300, 10, False),
              (9, 700, 7, 50, 3, False)]


def live_key(Q, N, b, R, C, multi):
    return "map_Q%d_N%d_b%d_R%d_C%d_%s" % (Q, N, b, R, C, "multi" if multi else "one")


def live_inputs(Q, N, b, R, C, multi):
    """codes, labels and the reference's database / query objects (+-1 features with the tie-breaking coordinate)."""
    seed = Q * 1000 + b
    if multi:
        dl, ql = synth.multihot_labels(seed, N, C), synth.multihot_labels(seed + 1, Q, C)
    else:
        dl, ql = synth.onehot_labels(seed, N, C)[0], synth.onehot_labels(seed + 1, Q, C)[0]
    db, qb = synth.planted_codes(seed, dl, b, 0.3), synth.planted_codes(seed, ql, b, 0.3)
    database = types.SimpleNamespace(output=O.tie_free_features(db, False, N), label=dl.astype(np.int64))
    query = types.SimpleNamespace(output=O.tie_free_features(qb, True, N), label=ql.astype(np.int64))
    return qb, db, ql, dl, database, query


def r_gt_n_inputs():
    d = types.SimpleNamespace(output=np.ones((5, 4)), label=np.ones((5, 2), np.int64))
    q = types.SimpleNamespace(output=np.ones((2, 4)), label=np.ones((2, 2), np.int64))
    return d, q, 6


def _recorded():
    return cases.load_golden("reference_live")


@pytest.mark.parametrize("Q,N,b,R,C,multi", LIVE_CASES)
def test_oracle_equals_unmodified_reference(Q, N, b, R, C, multi):
    ref = _recorded()[live_key(Q, N, b, R, C, multi)][()]
    qb, db, ql, dl, database, query = live_inputs(Q, N, b, R, C, multi)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, *_ = O.map_from_codes(qb, db, ql, dl, R)
        aw = O.reference_as_written(database.output, database.label, query.output, query.label, R)
    assert m == ref
    assert aw == ref


def test_reference_rejects_r_gt_n():
    assert str(_recorded()["r_gt_n_raises"]) == "ValueError"        # what the reference raised on these inputs
    d, q, R = r_gt_n_inputs()
    with pytest.raises(ValueError):
        O.reference_as_written(d.output, d.label, q.output, q.label, R)

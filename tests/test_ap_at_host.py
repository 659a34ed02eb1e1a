"""AP, precision and recall at many cut-offs without a GPU: the NumPy reduction (extra_metrics.map_from_ap_tables) against hand-built
tables, and the argument checks of map_at_k and MAPs.get_maps_at, which come before any native call -- without a GPU a native call
raises HashganNativeError, so a ValueError proves the order of the checks."""
import types
import warnings

import numpy as np
import pytest

from hashgan_amd import MAPs, metric
from hashgan_amd import extra_metrics as X

NAN = np.nan


def test_map_from_ap_tables_hand_built():
    ks = [2, 5, 9]
    #             k = 2        k = 5            k = 9
    ap = np.array([[NAN, 0.5, 0.25],
                   [NAN, NAN, 0.125],
                   [NAN, 1.0, 0.75],
                   [NAN, NAN, NAN]])
    hits = np.array([[0, 1, 3],
                     [0, 0, 1],
                     [0, 2, 4],
                     [0, 0, 0]])
    total_rel = np.array([6, 1, 4, 0])                   # the last query has no relevant row anywhere
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # (an all-skipped column is NaN without np.mean's empty-slice warning)
        out = X.map_from_ap_tables(ap, hits, total_rel, ks)
    assert np.isnan(out["map"][0])                       # every query skipped
    assert out["map"][1] == np.mean(np.array([0.5, 1.0]))            # some skipped: the mean of the rest, in query order
    assert out["map"][2] == np.mean(np.array([0.25, 0.125, 0.75]))
    assert np.array_equal(out["precision"], (hits / np.array(ks)[None, :]).mean(0))      # over ALL four queries
    assert out["precision"][1] == (1 / 5 + 0 + 2 / 5 + 0) / 4
    ok = np.array([True, True, True, False])             # recall: the query with total_rel == 0 is left out of the denominator
    assert np.array_equal(out["recall"], (hits[ok] / total_rel[ok, None]).mean(0))
    assert out["recall"][2] == (3 / 6 + 1 / 1 + 4 / 4) / 3
    pq = out["per_query"]
    assert np.array_equal(pq["ap"], ap, equal_nan=True) and np.array_equal(pq["hits"], hits) and np.array_equal(pq["total_rel"], total_rel)
    assert pq["hits"].dtype == np.int64 and pq["total_rel"].dtype == np.int64


def test_map_from_ap_tables_all_hit_and_no_relevant_rows():
    ap = np.array([[0.5, 0.75], [1.0, 0.25]])
    hits = np.array([[1, 2], [1, 1]])
    out = X.map_from_ap_tables(ap, hits, np.array([2, 3]), [1, 4])
    assert np.array_equal(out["map"], np.array([np.mean(ap[:, 0].copy()), np.mean(ap[:, 1].copy())]))
    # no query has a relevant row in the database: recall is NaN for every k, precision 0, mAP NaN
    z = X.map_from_ap_tables(np.full((3, 2), NAN), np.zeros((3, 2), int), np.zeros(3, int), [1, 4])
    assert np.isnan(z["recall"]).all() and (z["precision"] == 0).all() and np.isnan(z["map"]).all()
    for bad in ([], [4, 1], [1, 1], [1.5, 2.0]):
        with pytest.raises(ValueError):
            X.map_from_ap_tables(ap, hits, np.array([2, 3]), bad)
    with pytest.raises(ValueError):
        X.map_from_ap_tables(ap, hits[:, :1], np.array([2, 3]), [1, 4])
    with pytest.raises(ValueError):
        X.map_from_ap_tables(ap, hits, np.array([2, 3, 4]), [1, 4])


def _arrays(N=80, Q=3, b=8, C=4):
    rng = np.random.default_rng(0)
    return (rng.integers(0, 2, (Q, b)), rng.integers(0, 2, (N, b)), rng.integers(0, 2, (Q, C)), rng.integers(0, 2, (N, C)))


BAD_KS = ([], [5, 1], [5, 5], list(range(1, 66)), [0, 5], [1, 81], [1.5, 2.5], [[1, 2]])


@pytest.mark.parametrize("features", [False, True])
def test_map_at_k_refuses_bad_arguments_before_any_native_call(features):
    qb, db, ql, dl = _arrays()
    for ks in BAD_KS:
        with pytest.raises(ValueError):
            X.map_at_k(qb, db, ql, dl, ks, features=features)
    with pytest.raises(ValueError):
        X.map_at_k(qb, db[:, :7], ql, dl, [1], features=features)          # code lengths differ
    with pytest.raises(ValueError):
        X.map_at_k(qb, db, ql[:1], dl, [1], features=features)             # rows of codes and labels differ
    with pytest.raises(ValueError):
        X.map_at_k(qb, db, ql, dl[:, :3], [1], features=features)          # label widths differ


def test_map_at_k_refuses_more_than_255_feature_columns():
    rng = np.random.default_rng(1)
    q, d = rng.standard_normal((2, 256)).astype(np.float32), rng.standard_normal((9, 256)).astype(np.float32)
    with pytest.raises(ValueError):
        X.map_at_k(q, d, np.ones((2, 3), int), np.ones((9, 3), int), [1, 5], features=True)
    with pytest.raises(ValueError):
        X.precision_recall_at_k(q, d, np.ones((2, 3), int), np.ones((9, 3), int), [1, 5], features=True)


def _side(out, lab):
    return types.SimpleNamespace(output=out, label=lab)


def test_get_maps_at_refuses_bad_arguments_before_any_native_call():
    qb, db, ql, dl = _arrays()
    m = MAPs(5)
    for Rs in BAD_KS:
        with pytest.raises(ValueError):
            m.get_maps_at(_side(db, dl), _side(qb, ql), Rs)
    with pytest.raises(ValueError):
        m.get_maps_at(_side(db[:, :7], dl), _side(qb, ql), [1, 5])         # code lengths differ
    with pytest.raises(ValueError):
        m.get_maps_at(_side(db, dl[:-1]), _side(qb, ql), [1, 5])           # rows of codes and labels differ
    with pytest.raises(ValueError):
        m.get_maps_at(_side(db, dl), _side(qb, ql[:1]), [1, 5])
    with pytest.raises(ValueError):
        m.get_maps_at(_side(db, dl), _side(qb, ql[:, :3]), [1, 5])         # label widths differ
    with pytest.raises(ValueError):
        m.get_maps_at(None, _side(qb, ql), [1, 5])                         # no resident database
    assert m._eng is None                                                  # no context was ever asked for


def test_check_cutoffs_is_the_rule_of_the_native_call():
    assert metric.MAX_CUTOFFS == X.MAX_CUTOFFS == 64
    assert metric._check_cutoffs(range(1, 65), 64).dtype == np.int64
    assert np.array_equal(metric._check_cutoffs(np.array([1, 7, 80], dtype=np.uint8), 80), [1, 7, 80])

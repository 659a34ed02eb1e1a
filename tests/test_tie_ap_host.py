"""Tie-aware AP without a GPU: the oracles the GPU tests lean on (tests/tie_oracle.py) against the full enumeration of the tie orders
and against each other, and the argument checks of the Python surface, which come before any GPU use."""
import math
import random

import numpy as np
import pytest

from hashgan_amd import extra_metrics as X
from tests import tie_oracle as T

FLOATS = ("ap", "p_hit", "ap_min", "ap_max", "rel_exp")


def _same(x, y):
    return (math.isnan(x) and math.isnan(y)) or x == y


def _structures(seed, count, groups, rows):
    rng = random.Random(seed)
    for _ in range(count):
        n = [rng.randint(0, rows) for _ in range(rng.randint(1, groups))]
        if sum(n) == 0:
            n[0] = 1
        yield n, [rng.randint(0, x) for x in n]


def test_exact_oracle_is_mean_min_max_over_all_tie_orders():
    """<= 3 groups of <= 4 rows, every R: the exact oracle equals the mean, minimum and maximum of the reference's AP over all
    tie orders, the hit probability and the moments of the hit count, bit for bit after the one rounding to float."""
    seen_partial = seen_nan = 0
    for n, r in _structures(1, 250, 3, 4):
        for R in range(1, sum(n) + 1):
            e, m = T.exact(n, r, R), T.enumerated(n, r, R)
            for k in FLOATS:
                assert _same(e[k], m[k]), (n, r, R, k, e[k], m[k])
            assert e["rel_lo"] == m["rel_lo"] and e["rel_hi"] == m["rel_hi"], (n, r, R)
            seen_partial += 0.0 < e["p_hit"] < 1.0
            seen_nan += math.isnan(e["ap"])
    assert seen_partial > 20 and seen_nan > 20


def test_bmin_recurrence_is_the_definition():
    for P, S, c in ((0, 0, 5), (3, 2, 7), (100, 17, 40), (7, 0, 1)):
        B = U = T.Fraction(0)
        for h in range(0, c):
            x = P + c - h
            U += T.Fraction(1, x)
            B += T.Fraction(S, x) + U
            assert B == T.bmin_by_definition(P, S, c, h + 1)


def test_fast_oracle_agrees_with_the_exact_one():
    """Within 8 * 2^-52 relatively, up to a 300-row cut group."""
    tol = 8 * 2.0 ** -52
    cases = list(_structures(2, 40, 4, 30))
    cases += [([50, 100, 300, 50], [5, 40, 120, 10]), ([0, 7, 300], [0, 0, 299]), ([300], [150]), ([120, 1, 300, 1], [0, 1, 3, 0])]
    worst = 0.0
    for n, r in cases:
        N = sum(n)
        for R in sorted({1, min(2, N), max(1, N // 3), max(1, N // 2), max(1, N - 1), N}):
            e, f = T.exact(n, r, R), T.fast(n, r, R)
            assert e["rel_lo"] == f["rel_lo"] and e["rel_hi"] == f["rel_hi"] and e["H"] == f["H"]
            for k in FLOATS:
                if math.isnan(e[k]):
                    assert math.isnan(f[k]), (n, r, R, k)
                    continue
                err = abs(e[k] - f[k])
                worst = max(worst, err / (tol * abs(e[k])) if e[k] else 0.0)
                assert err <= tol * abs(e[k]), (n, r, R, k, e[k], f[k])
    print("fast against exact: largest error %.3g of 8 * 2^-52" % worst)


def test_envelope_holds_the_expectation():
    for n, r in _structures(3, 60, 5, 40):
        for R in (1, max(1, sum(n) // 2), sum(n)):
            e = T.exact(n, r, R)
            if not math.isnan(e["ap"]):
                assert e["ap_min"] <= e["ap"] <= e["ap_max"] <= 1.0
            assert e["rel_lo"] <= e["rel_exp"] <= e["rel_hi"]


@pytest.mark.parametrize("fn", ["tie_aware_map", "tie_aware_precision_recall_at_k"])
def test_python_surface_refuses_bad_cutoffs_before_any_gpu_use(fn):
    rng = np.random.default_rng(0)
    N, Q, b, C = 80, 3, 8, 4
    db, qb = rng.integers(0, 2, (N, b)), rng.integers(0, 2, (Q, b))
    dl, ql = rng.integers(0, 2, (N, C)), rng.integers(0, 2, (Q, C))
    f = getattr(X, fn)
    for Rs in ([], [5, 1], [5, 5], [0, 5], [1, N + 1], list(range(1, 66)), [1.5, 2.5], [[1, 2]]):
        with pytest.raises(ValueError):
            f(qb, db, ql, dl, Rs)
    with pytest.raises(ValueError):
        f(qb, db[:, :7], ql, dl, [1])

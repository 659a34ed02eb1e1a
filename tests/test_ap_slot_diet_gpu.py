"""The AP epilogue's leaf loop (ap_eval2 in hashgan_amd/csrc/hg_kernels.hpp) through every kernel that inlines it, on list lengths
and match patterns chosen for the loop: per-query AP (nan where a query has no hit) and hit counts `==` the oracle's
metric.py:20-23 arithmetic (oracle.hamming_map.label_match / average_precision on the canonical order).  No tolerance: the
kernels perform NumPy's additions in NumPy's order.

What drives a case is R, not N: a leaf of the summation tree is walked in 32-slot windows, eight lanes per leaf, four slots per
lane and window; the lengths below give leaves shorter than 8, exact multiples of 8, 32 and 64, one-window leaves, ragged last
windows (of 8, 16 and 24 slots), the chunk boundary of 8192 elements and a second chunk with a short last one.

Callers and how a case reaches them (stat "rank_variant" says that it did):
  k_ap          N = 3000 / 17000, `all_rows_shortcut` = 0: the exact sequence's k_rank_fused (1), then k_ap
  k_rank_dense  N = 3000 / 17000, R > N / 8 up to R = N: the byte matrix (7), the AP from its epilogue
  k_rank_lean   the bet's rank stage takes databases of >= 65536 rows with 8 R <= N only, so these cases run on N = 66000:
                `rank_lds` = 2 (6), with the guessed and with the exact cut (`optimistic` = 0: the matrix-core select at the exact
                threshold feeds the same rank stage)
  k_rank_cnt    N = 66000, `rank_lds` = 1 (3): its epilogue (ap_eval with the reciprocals: the same element values and additions by
                the per-element walk, pinned next to ap_eval2 on the same lists); and with the lists wanted (hg_topr, then hg_ap:
                k_rank_cnt, then k_ap)

Structured match patterns come through the labels: every query of such a case has the same code, hence the same ranking, and a
one-hot class of its own (query i: class i mod 10); class c is given to the database rows by their rank p (0-based) in that
ranking -- 0 every row, 1 no row, 2 only the R-th ranked, 3 every eighth rank (one accumulator only), 4 a dense head followed by
none, 5 every eighth rank from the seventh (the last accumulator), 6 a dense head and the R-th, 7..9 random at densities 0.5, 0.1
and 0.9.  The random cases have distinct queries and multi-hot labels at 10 and at 81 classes.
"""
import functools

import numpy as np
import pytest

from hashgan_amd import _native, metric
from oracle import hamming_map as O

pytestmark = pytest.mark.gpu

SMALL_R = (1, 7, 8, 9, 63, 64, 65, 72, 79, 80, 81, 127, 128, 129, 136, 255, 257, 1000, 2999)
CHUNK_R = (8191, 8192, 8193, 8200, 16385)
N_SMALL, N_CHUNK, N_BET = 3000, 17000, 66000
C = 10


@functools.lru_cache(maxsize=None)
def _codes(N, b, Q, same):
    """(qbits, dbbits, order [Q or 1, N]): iid codes; `same`: one query code for all Q queries.  The canonical order once."""
    rng = np.random.default_rng(70000 + 13 * N + 3 * b + Q + (1000 if same else 0))
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = rng.integers(0, 2, (1 if same else Q, b), dtype=np.uint8)
    order, _ = O.topr_from_codes(qb, db, N)
    if same:
        qb = np.repeat(qb, Q, axis=0)
    for a in (qb, db, order):
        a.setflags(write=False)
    return qb, db, order


def _structured_labels(N, order0, R, seed):
    """dblab [N, 10] by the rank of a row in order0 (see the module's docstring)."""
    rng = np.random.default_rng(seed)
    p = np.empty(N, dtype=np.int64)
    p[order0] = np.arange(N)
    head = max(1, R // 3)
    dl = np.zeros((N, C), dtype=np.int8)
    dl[:, 0] = 1
    dl[:, 2] = p == R - 1
    dl[:, 3] = p % 8 == 0
    dl[:, 4] = p < head
    dl[:, 5] = p % 8 == 7
    dl[:, 6] = (p < head) | (p == R - 1)
    for c, dens in ((7, 0.5), (8, 0.1), (9, 0.9)):
        dl[:, c] = rng.random(N) < dens
    return dl


def _reference(ql, dl, order, R):
    """(ap [Q] with nan, hits [Q]) by metric.py:17-23 on the canonical order; order has one row per query, or one for all."""
    Q = ql.shape[0]
    ap, rel = np.full(Q, np.nan), np.zeros(Q, dtype=np.int64)
    memo = {}
    for i in range(Q):
        key = (ql[i].tobytes(), i if order.shape[0] > 1 else 0)
        if key not in memo:
            im = O.label_match(ql[i], dl[order[key[1], :R]])
            a, r = O.average_precision(im, R)
            memo[key] = (np.nan if a is None else a, int(r))
        ap[i], rel[i] = memo[key]
    return ap, rel


def _check(got, ref, what):
    ap, rel = got
    assert np.array_equal(rel, ref[1]), "%s: hits differ at queries %s" % (what, np.flatnonzero(np.asarray(rel) != ref[1])[:8])
    assert np.array_equal(ap, ref[0], equal_nan=True), "%s: AP differs at queries %s" % (what, np.flatnonzero(~((ap == ref[0]) | (np.isnan(ap) & np.isnan(ref[0]))))[:8])


def _case(N, b, Q, kind, R):
    """(qbits, qlab, dbbits, dblab, reference) of one list length; for Q = 1 the structured kind yields one query per class."""
    same = kind == "structured"
    qb, db, order = _codes(N, b, Q, same)
    if same:
        dl = _structured_labels(N, order[0], R, 100 * R + b)
        qls = [np.eye(C, dtype=np.int8)[(np.arange(Q) + s) % C] for s in (range(C) if Q == 1 else (0,))]
    else:
        nc, dens = (10, 0.15) if kind == "random10" else (81, 0.02)
        rng = np.random.default_rng(900 + 7 * R + b + Q + nc)
        dl = (rng.random((N, nc)) < dens).astype(np.int8)
        ql = (rng.random((Q, nc)) < dens).astype(np.int8)
        ql[0] = 0
        ql[0, R % nc] = 1                          # (never an empty query label in front; empty ones further back give nan)
        qls = [ql]
    return qb, qls, db, dl, order


def _run(N, b, Q, kind, Rs, modes):
    """modes: (name, options, R filter, R -> accepted values of "rank_variant", lists) -- every mode runs every R it accepts."""
    ctx = _native.Context(0)
    try:
        for R in Rs:
            qb, qls, db, dl, order = _case(N, b, Q, kind, R)
            ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, dl.shape[1])
            for ql in qls:
                ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
                ref = _reference(ql, dl, order, R)
                for name, options, accepts, variant, lists in modes:
                    if not accepts(R):
                        continue
                    for k, v in options.items():
                        ctx.set_option(k, v)
                    what = "%s N=%d b=%d Q=%d %s R=%d" % (name, N, b, Q, kind, R)
                    f0 = ctx.get_stat("optimistic_fallbacks")
                    if lists:
                        ctx.topr(R)
                        ctx.ap()
                        got = ctx.get_ap()
                    else:
                        got = ctx.map(R)
                    _check(got, ref, what)
                    if ctx.get_stat("optimistic_fallbacks") == f0:
                        assert ctx.get_stat("rank_variant") in variant(R), (what, ctx.get_stat("rank_variant"))
    finally:
        ctx.close()


_BASE = {"optimistic": 1, "all_rows_shortcut": 1, "rank_lds": 2}
# databases below the bet's floor: the exact sequence + k_ap for every R, the byte matrix + its epilogue for R > N / 8
_SMALL_MODES = lambda N: (
    ("k_ap", dict(_BASE, all_rows_shortcut=0), lambda R: True, lambda R: (1,), False),
    ("k_rank_dense", dict(_BASE), lambda R: 8 * R > N, lambda R: (7,), False),
)
# the bet's floor: k_rank_lean with the guessed and the exact cut, k_rank_cnt's epilogue, k_rank_cnt with lists + k_ap
# (lists of more than a few thousand ranks do not fit the LDS-resident kernels next to four other blocks: choose_rank hands them to
# k_rank_dense<slices> (8), whose epilogue is the same ap_eval2 -- accepted for the lengths around the chunk boundary only)
_LONG = lambda R, small: (small,) if R <= max(SMALL_R) else (small, 8)
_BET_MODES = (
    ("k_rank_lean", dict(_BASE), lambda R: True, lambda R: _LONG(R, 6), False),
    ("k_rank_lean exact cut", dict(_BASE, optimistic=0), lambda R: True, lambda R: _LONG(R, 6), False),
    ("k_rank_cnt", dict(_BASE, rank_lds=1), lambda R: True, lambda R: _LONG(R, 3), False),
    ("k_rank_cnt lists + k_ap", dict(_BASE, rank_lds=1), lambda R: True, lambda R: (3,), True),
)
KINDS = ("structured", "random10", "random81")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q", [1, 65, 130])
@pytest.mark.parametrize("b", [32, 64])
def test_k_ap_and_the_dense_epilogue_on_every_leaf_shape(b, Q, kind):
    """N = 3000, every R of SMALL_R and R = N: k_ap after the exact sequence, k_rank_dense's epilogue where R > N / 8."""
    _run(N_SMALL, b, Q, kind, SMALL_R + (N_SMALL,), _SMALL_MODES(N_SMALL))


@pytest.mark.parametrize("kind", KINDS)
def test_the_chunk_boundary(kind):
    """N = 17000, Q = 3, R around AP_CHUNK = 8192 and two chunks with a short last one: k_ap and k_rank_dense's epilogue."""
    _run(N_CHUNK, 64, 3, kind, CHUNK_R, _SMALL_MODES(N_CHUNK))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q", [1, 65, 130])
@pytest.mark.parametrize("b", [32, 64])
def test_the_bets_rank_kernels_on_every_leaf_shape(b, Q, kind):
    """N = 66000 (the bet takes >= 65536 rows and 8 R <= N): k_rank_lean, k_rank_cnt, and k_rank_cnt with lists followed by k_ap, on
    SMALL_R and the lengths around the chunk boundary that 8 R <= N admits."""
    _run(N_BET, b, Q, kind, SMALL_R + tuple(R for R in CHUNK_R if 8 * R <= N_BET), _BET_MODES)

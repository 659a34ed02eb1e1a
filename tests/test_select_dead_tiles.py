"""The packed matrix-core selects (k_select_mx3, k_select_mx4) where wavefronts and query tiles of the last query block
have no live query, where the last segment is short or has no partner, and where the drain takes its rare routes: the
one-pass bet against the exact two-pass sequence of the same library, bit for bit.

A block is 512 queries = eight wavefronts of two 32-query tiles: Q = 1 and 33 leave seven wavefronts dead (and, at 1, the
live one's second tile), 64 and 65 end on a wavefront boundary and one query past it, 511 and 513 do the same at the
block boundary, 2100 is the C3 workload's count (33 live wavefronts of 40).  Code widths 32 / 64 select k_select_mx3 with
one and two code words, 96 / 128 k_select_mx4 with three and four; 10 and 81 classes are one and two label words."""
import numpy as np
import pytest
from hashgan_amd import _native, metric

pytestmark = pytest.mark.gpu

QS = (1, 33, 64, 65, 511, 513, 2100)
BS = (32, 64, 96, 128)


def _bet_and_exact(ctx, R, key):
    ctx.set_option("optimistic", 1)
    runs = ctx.get_stat("optimistic_runs")
    ap, rel = ctx.map(R)
    # the bet ran and held: the packed select produced this
    assert ctx.get_stat("optimistic_runs") == runs + 1 and ctx.get_stat("last_optimistic") == 1, key
    ctx.set_option("optimistic", 0)
    ap0, rel0 = ctx.map(R)
    assert ctx.get_stat("optimistic_runs") == runs + 1, key   # no bet: histogram, plan, select
    ctx.set_option("optimistic", 1)
    assert np.array_equal(ap, ap0, equal_nan=True), key
    assert np.array_equal(rel, rel0, equal_nan=True), key


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("Q", QS)
def test_bet_equals_exact_on_padded_query_blocks(Q, b):
    C = (10, 81)[(QS.index(Q) + BS.index(b)) % 2]             # every width and every count meets both label widths
    rng = np.random.default_rng(1000 * Q + b)
    N = 70000 + int(rng.integers(1, 95))                      # never a multiple of a segment: the last one is short
    R = 600
    cen = rng.integers(0, 2, (23, b), dtype=np.uint8)         # noisy copies of a few centres: dense and empty supertiles both
    db = cen[rng.integers(0, 23, N)] ^ (rng.random((N, b)) < 0.2).astype(np.uint8)
    qb = cen[rng.integers(0, 23, Q)] ^ (rng.random((Q, b)) < 0.2).astype(np.uint8)
    dl = np.eye(C, dtype=np.int8)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int8)[rng.integers(0, C, Q)]
    ctx = _native.Context(0)
    try:
        nqt = (Q + 63) // 64
        # three segments (below four the engine keeps the count it is asked for): the third has no partner, and is short;
        # then the engine's own choice for the shape
        for units in (3 * nqt, 16384):
            ctx.set_option("target_units", units)
            ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, C)
            ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
            key = (Q, b, C, N, units)
            _bet_and_exact(ctx, R, key)
            S = ctx.get_stat("segments")
            if units == 3 * nqt:
                assert S == 3, key + (S,)
    finally:
        ctx.set_option("target_units", 16384)
        ctx.close()


@pytest.mark.parametrize("Q,b,C", [(65, 64, 10), (33, 128, 10), (513, 32, 81)])
def test_bet_equals_exact_on_a_class_sorted_database(Q, b, C):
    """Rows stored class by class with codes that follow the class: a query's near rows crowd into its class's share of
    the segments, the slices are widened (cap_boost) and whole supertiles of hits arrive at once -- the drain's
    make_room and direct_walk run."""
    rng = np.random.default_rng(4242 + Q)
    N, R = 200000 + 17, 3000
    cls = np.sort(rng.integers(0, C, N))
    proto = (rng.random((C, b)) < 0.5).astype(np.uint8)
    db = proto[cls] ^ (rng.random((N, b)) < 0.25).astype(np.uint8)
    qcls = rng.integers(0, C, Q)
    qb = proto[qcls] ^ (rng.random((Q, b)) < 0.25).astype(np.uint8)
    dl = np.eye(C, dtype=np.int8)[cls]
    ql = np.eye(C, dtype=np.int8)[qcls]
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, C)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        _bet_and_exact(ctx, R, (Q, b, C))
        assert ctx.get_stat("cap_boost") > 1, (Q, b, C)
    finally:
        ctx.close()

"""The builders of tests/rank_cases.py deliver what they promise -- checked with the oracle alone, on the CPU.  This is what
keeps tests/test_rank_stage_gpu.py from passing vacuously: a span, a threshold or a plateau that is not in the data is not
tested on the GPU either."""
import numpy as np
import pytest

from tests import rank_cases as rc


@pytest.mark.parametrize("b", [16, 64, 100])
def test_ordinary_cases_are_ordinary(b):
    c = rc.ordinary(b)
    ap, rel, imatch, idx, dist = rc.reference("ordinary", b)
    Q, N = c["qbits"].shape[0], c["dbbits"].shape[0]
    assert (Q, c["R"], c["qlab"].shape[1]) == (130, 600, 10) and 66000 <= N <= 70001 and 8 * c["R"] <= N
    assert c["qbits"].shape[1] == c["dbbits"].shape[1] == b
    assert c["dblab"].sum(1).max() > 1                                       # multi-hot
    assert np.isnan(ap[5]) and rel[5] == 0 and np.isfinite(ap).sum() > Q // 2
    assert rc.span_of(dist).max() <= rc.maxb(b)                              # nothing for a rank kernel to decline
    # the three layouts of the counters (cut_counters in hg_rank.hip): RC_MAXB + 2 of them where that is fewer than b + 1
    assert {16: 17, 64: 18, 100: 34}[b] == min(rc.maxb(b) + 2, b + 1)


@pytest.mark.parametrize("b", [17, 64, 100])
def test_spans_are_the_listed_ones(b):
    c = rc.spans(b)
    _, _, _, _, dist = rc.reference("spans", b)
    span = rc.span_of(dist)
    planted = c["planted"]
    assert tuple(sorted(planted.values())) == rc.SPANS[b]
    for q, s in planted.items():
        assert span[q] == s, (q, span[q], s)
    others = np.array([span[q] for q in range(len(span)) if q not in planted])
    assert others.max() <= rc.SPAN_SMALL[b] < rc.maxb(b)
    m = rc.maxb(b)
    listed = set(planted.values())
    assert {m, m + 1} <= listed and m - 1 in listed | {15}                    # the edge itself, one below, one beyond
    if b != 17:
        assert m + 2 in listed and max(listed) > m + 2                       # `nbk > RC_MAXB` (+1, +2) and the window check (wider)
    N = c["dbbits"].shape[0]
    assert 66000 <= N <= 70001 and 8 * c["R"] <= N and len(span) <= 200


@pytest.mark.parametrize("b", [128, 129, 255])
def test_byte_edge_thresholds_are_exact(b):
    c = rc.cut_at_the_byte_edge(b)
    N = c["dbbits"].shape[0]
    assert 66000 <= N <= 70001 and c["R"] == 500
    for batch, want in (("below", rc.EDGE_BELOW), ("across", rc.edge_across(b))):
        _, _, _, _, dist = rc.reference("cut_at_the_byte_edge", b, batch)
        t = dist[:, -1]
        assert np.array_equal(t, c[batch]["thresholds"])
        assert tuple(sorted(set(t.tolist()))) == tuple(want), (batch, sorted(set(t.tolist())))
        # ties at the threshold are thin and the rows within it few: the exact cut's slices hold them
        assert max(int((dist[i] == t[i]).sum()) for i in range(len(t))) < c["R"]
        assert rc.span_of(dist).max() <= 4
    assert max(rc.EDGE_BELOW) == 127 and min(rc.EDGE_BELOW) == 122
    assert rc.edge_across(255) == (126, 127, 128, 129, 130) and rc.edge_across(129) == (126, 127, 128) and rc.edge_across(128) == (126, 127)


def test_plateau_reaches_the_code_length():
    c = rc.plateau_at_b(128)
    _, _, _, _, dist = rc.reference("plateau_at_b", 128)
    assert np.array_equal(dist[:, -1], c["thresholds"]) and dist[:, -1].max() == 128


def test_long_slice_case_crowds_three_blocks():
    c = rc.crowded(rc.LONG_SLICE_R)
    _, _, _, idx, dist = rc.reference("crowded", rc.LONG_SLICE_R)
    q, R = c["crowded_query"], c["R"]
    assert rc.span_of(dist).max() <= 16                                       # every query is ranked in place
    t = dist[q, -1]
    blocks = idx[q] // 96
    per_block = np.bincount(blocks, minlength=c["dbbits"].shape[0] // 96 + 1)
    for m in c["blocks"]:
        # the run is inside the cut (ties at t included or not: it lies below t), in ONE 96-row block
        assert per_block[m] >= rc.LONG_SLICE_RUN and dist[q][blocks == m].max() < t
    # everywhere else a 384-row window (a segment of the geometries in use) holds a fraction of that, the guessed cut's surplus included
    D = rc.O.hamming_matrix(rc.O.pack_bits(c["qbits"][q:q + 1]), rc.O.pack_bits(c["dbbits"]))[0]
    near = (D <= t + 1).astype(np.int64)
    win = np.add.reduceat(near, np.arange(0, len(near), 96))
    planted = np.zeros(len(win), bool)
    planted[list(c["blocks"])] = True
    assert win[~planted].max() <= 16 and win[planted].min() >= 50 and win[planted].max() <= 64
    assert 8 * R <= c["dbbits"].shape[0]


def test_too_many_records_case_has_its_plateaus():
    c = rc.crowded(rc.TOO_MANY_R)
    R, N = c["R"], c["dbbits"].shape[0]
    assert (R, N) == (6000, 131072)
    _, _, _, _, dist = rc.reference("crowded", rc.TOO_MANY_R)
    assert rc.span_of(dist).max() <= 16
    qs = list(c["plateau_queries"])
    D = rc.O.hamming_matrix(rc.O.pack_bits(c["qbits"][qs]), rc.O.pack_bits(c["dbbits"]))
    for i, q in enumerate(qs):
        t = dist[q, -1]
        assert t == c["plateau_distance"]
        below, ties = int((D[i] < t).sum()), int((D[i] == t).sum())
        assert below == 3 * R // 10 and ties == c["plateau"] == 33 * R // 10
        # any cut from t to t + 4 keeps the same records: more than k_rank_lean holds (16 * 1024), fewer than the budget of 4 R
        assert int((D[i] <= t + 4).sum()) == below + ties and 16 * 1024 < below + ties < 4 * R
        # evenly over the database: a window of 512 rows holds ~84 of them, far below a slice's capacity
        per = np.add.reduceat((D[i] <= t).astype(np.int64), np.arange(0, N, 512))
        assert per.max() - per.min() <= 4 and per.max() < 100
    others = [q for q in range(len(dist)) if q not in qs]
    assert dist[others, -1].min() >= 16                                      # the other queries are ordinary: no plateau, no near rows

"""Deterministic workloads aimed at the rank stage of the sampled-threshold bet (launch_rank in hashgan_amd/csrc/hg_rank.hip):
which kernel takes a query's records, and every reason k_rank_lean / k_rank_cnt have to hand a query to the general kernel.

Pure NumPy, one fixed seed per case.  Every builder returns a dict with qbits, dbbits, qlab, dblab ({0,1} matrices), b, R and
the properties it guarantees; tests/test_rank_cases_host.py asserts those properties with the oracle alone, so that the GPU
tests (tests/test_rank_stage_gpu.py) cannot pass vacuously.  The bet needs N >= 65536 and 8 R <= N: the databases stay just
above that floor, and Q <= 200 keeps the oracle at seconds.

Builders and their oracle results are cached per process: treat the arrays as read-only (they are flagged so).
"""
import functools
import warnings

import numpy as np

from oracle import hamming_map as O

C = 10          # classes, multi-hot


def _labels(rng, n):
    return (rng.random((n, C)) < 0.15).astype(np.int8)


def _bits(rng, n, b):
    return rng.integers(0, 2, (n, b), dtype=np.uint8)


def _flip(rng, code, d):
    """code with d distinct bits flipped: Hamming distance exactly d."""
    row = code.copy()
    row[rng.choice(code.shape[0], d, replace=False)] ^= 1
    return row


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def oracle(qbits, dbbits, qlab, dblab, R):
    """(ap [Q] with nan, rel [Q], imatch [Q, R], idx [Q, R], dist [Q, R]) of oracle.hamming_map.map_from_codes."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, imatch, idx, dist = O.map_from_codes(qbits, dbbits, qlab, dblab, R)
    return ap, imatch.sum(1), imatch, idx, dist


def span_of(dist):
    """Distinct consecutive distance values a top-R list reaches over, per query."""
    return dist[:, -1] - dist[:, 0] + 1


def maxb(b):
    """rank_cnt_maxb (hg_rank_cnt.hpp): the distances a ranked list may span in k_rank_cnt / k_rank_lean."""
    return 16 if b + 1 <= 65 else 32


# ---------------------------------------------------------------------------------------------------------------- ordinary
@functools.lru_cache(maxsize=None)
def ordinary(b):
    """iid codes, Q = 130, R = 600, multi-hot labels; query 5 has no label (its AP is nan).  b = 16: a counter for every
    distance and no cut read; 64: 18 counters, lists of up to 16 distances; 100: 34 counters, up to 32."""
    rng = np.random.default_rng(1000 + b)
    Q, N, R = 130, 66000 + b, 600
    ql = _labels(rng, Q)
    ql[5] = 0
    return _freeze(dict(qbits=_bits(rng, Q, b), dbbits=_bits(rng, N, b), qlab=ql, dblab=_labels(rng, N), b=b, R=R))


# ------------------------------------------------------------------------------------------------------------------- spans
SPANS = {17: (16, 17), 64: (15, 16, 17, 18, 19, 22), 100: (31, 32, 33, 34, 35)}
SPAN_QUERIES = (3, 20, 41, 64, 77, 129)          # in several 64-query tiles, first and last query of the batch nearly included
SPAN_SMALL = {17: 12, 64: 12, 100: 24}           # what every other query stays within


def _plant_spans(rng, qb, db, R, wanted, rows_of):
    """Give query SPAN_QUERIES[i] a top-R list that spans wanted[i] distances: two rows at distance t - span + 1, far apart in
    the database (different segments), t being the query's threshold AFTER planting -- so plant, look, and plant again."""
    qs = list(SPAN_QUERIES[:len(wanted)])
    for _ in range(6):
        _, dist = O.topr_from_codes(qb[qs], db, R)
        have = span_of(dist)
        if np.array_equal(have, wanted):
            return qs
        for i, q in enumerate(qs):
            if have[i] == wanted[i]:
                continue
            d = int(dist[i, -1]) - wanted[i] + 1
            if d < 0:
                raise AssertionError("span %d does not fit below threshold %d" % (wanted[i], dist[i, -1]))
            for r in rows_of(i):
                db[r] = _flip(rng, qb[q], d)
    raise AssertionError("planting did not converge")


@functools.lru_cache(maxsize=None)
def spans(b):
    """A database in which a handful of queries (`planted`: query -> span) have top-R lists spanning a chosen number of distances
    around RC_MAXB = 16 (32 at b = 100), every other query a span of at most SPAN_SMALL[b].

    b = 64, 100: an ordinary (iid) database with two rows planted per such query.
    b = 17: no iid database can do it.  A list that spans 16+ of the 18 distances has its threshold at 15+, so fewer than R rows
    lie closer than 15 to the query: all but R rows sit within distance 2 of the query's complement.  The database is therefore
    a cloud around one centre (75 % of the rows the centre itself, 22 % with one bit flipped, 3 % with two, in random order) and
    EVERY query is far from it: the centre's complement with e = 3..5 bits flipped, whose threshold is 16 - e (the rows with one
    bit, away from the query's e: a fifth of every segment, which a slice of R = 2400 holds).
    The planted queries (e = 1, 0) also find two copies of themselves: spans 16 and 17; the copies are rows at distance >= 2 of
    every other query, whose spans stay <= 12.  A span of 18 needs the threshold 17 = b:
    all rows but R equal the query's complement, a plateau of ties that overflows the slices of every cut -- no rank kernel of the
    bet ever sees such a query (the vector-ALU exact sequence answers the whole call), so 18 is not a case."""
    rng = np.random.default_rng(2000 + b)
    wanted = np.array(SPANS[b])
    Q = 130
    if b == 17:
        N, R = 68000 + b, 2400
        centre = _bits(rng, 1, b)[0]
        db = np.stack([_flip(rng, centre, int(w)) for w in rng.choice(3, N, p=(0.75, 0.22, 0.03))])
        qb = np.stack([_flip(rng, 1 - centre, int(e)) for e in rng.integers(3, 6, Q)])
        for i, q in enumerate(SPAN_QUERIES[:len(wanted)]):
            qb[q] = _flip(rng, 1 - centre, (1, 0)[i])
    else:
        N, R = 68000 + b, 600
        db, qb = _bits(rng, N, b), _bits(rng, Q, b)
    qs = _plant_spans(rng, qb, db, R, wanted, lambda i: (1009 + 9973 * i, 40009 + 3331 * i))
    ql = _labels(rng, Q)
    return _freeze(dict(qbits=qb, dbbits=db, qlab=ql, dblab=_labels(rng, N), b=b, R=R,
                        planted={int(q): int(s) for q, s in zip(qs, wanted)}))


# ---------------------------------------------------------------------------------------------------------- the byte edge
EDGE_BELOW = tuple(range(122, 128))


def edge_across(b):
    """Thresholds the `across` batch covers: 126..130, as far as the construction below reaches (b - 1: see there)."""
    return tuple(range(126, min(130, b - 1) + 1))


@functools.lru_cache(maxsize=None)
def cut_at_the_byte_edge(b):
    """Exact thresholds next to 127, the largest distance of a one-byte record {match:1 | dist:7}.

    The database is the complement of a centre code with bits flipped back: 3000 rows one bit, 300 two, 100 three, at random
    places; all others are the complement itself.  A query is the centre with e bits flipped.  A row whose flipped-back bits F
    miss the query's E lies at b - e - |F|, so the query's R = 500 nearest are the 400 rows with two or three bits and the
    first of the ~3000 (1 - e / b) with one: the threshold is b - 1 - e exactly, its ties a few per cent of the rows, evenly
    spread (the exact matrix-core select keeps all ties of one segment: a tie plateau would overflow its slice), and the
    untouched complements lie at b - e, beyond the cut.  `below`: e such that the thresholds are 122..127, four queries each;
    `across`: 126..min(130, b - 1).

    A threshold of b itself cannot come from this database, nor from any that serves `below`: it means all rows but R equal
    the query's complement, and then every other query's threshold is a plateau of N - R ties.  plateau_at_b() has that case."""
    rng = np.random.default_rng(3000 + b)
    N, R = 66000 + b, 500
    centre = _bits(rng, 1, b)[0]
    db = np.repeat((1 - centre)[None, :], N, axis=0)
    rows = rng.choice(N, 3400, replace=False)
    for i, r in enumerate(rows):
        db[r] = _flip(rng, 1 - centre, 1 if i < 3000 else 2 if i < 3300 else 3)

    def batch(ts):
        ts = [t for t in ts for _ in range(4)]
        return np.stack([_flip(rng, centre, b - 1 - t) for t in ts]), np.array(ts)

    q_below, t_below = batch(EDGE_BELOW)
    q_across, t_across = batch(edge_across(b))
    return _freeze(dict(dbbits=db, dblab=_labels(rng, N), b=b, R=R,
                        below=dict(qbits=q_below, qlab=_labels(rng, len(q_below)), thresholds=t_below),
                        across=dict(qbits=q_across, qlab=_labels(rng, len(q_across)), thresholds=t_across)))


@functools.lru_cache(maxsize=None)
def plateau_at_b(b=128):
    """The threshold b itself (128: the one value of `across` that cut_at_the_byte_edge(128) cannot reach): all rows but 400 are
    the complement of the centre, the queries are the centre (threshold b) and the centre with one bit flipped (b - 1)."""
    rng = np.random.default_rng(3500 + b)
    N, R = 66000 + b, 500
    centre = _bits(rng, 1, b)[0]
    db = np.repeat((1 - centre)[None, :], N, axis=0)
    for r in rng.choice(N, 400, replace=False):
        db[r] = _flip(rng, 1 - centre, int(rng.integers(1, 4)))
    qb = np.stack([centre, centre, _flip(rng, centre, 1), _flip(rng, centre, 1)])
    return _freeze(dict(qbits=qb, dbbits=db, qlab=_labels(rng, 4), dblab=_labels(rng, N), b=b, R=R,
                        thresholds=np.array([b, b, b - 1, b - 1])))


# ----------------------------------------------------------------------------------------------------------------- crowded
LONG_SLICE_R, TOO_MANY_R = 1500, 6000
LONG_SLICE_RUN = 50                      # near rows per planted run
LONG_SLICE_BLOCKS = (100, 333, 601)      # the 96-row blocks that hold a run


@functools.lru_cache(maxsize=None)
def crowded(R):
    """The record-count branches of k_rank_lean, b = 64.  How the densities follow from hg_seq.hip and hg_rank.hip:

    crowded(1500), the long slice.  enqueue_optimistic budgets mean = 4 R / S records per (segment, query) slice and
    slice_capacity gives it cap = mean + 6 sqrt(mean) + 16, rounded up to 16.  choose_rank has k_rank_lean fetch PSP 16-byte pieces of every
    slice up front, PSP = ceil((est + 4 sqrt(est) + 1) / 16) with est = 0.7 (sqrt(cap - 7) - 3)^2, and a slice with more than
    16 PSP records is finished by its own thread (`pc > PSP`).  N = 66064 rows in segments of 288 give S = 230: mean 26,
    cap 80, est 21.6, PSP 3 -- the tail starts at 49 records, the slice overflows at 81.  A slice of the exact cut holds
    ~R / S = 6.5 records, one of the guessed cut ~2 R / S = 13.  Query 37 gets runs of 50 near rows (distance 14..19,
    inside its threshold of 24 and its list's usual span) in three 96-row blocks -- segments are whole multiples of 96 rows at b <= 64, so a run never
    straddles two: those slices hold 50 + 6..20 records, several times their neighbours', and stay below the capacity.

    crowded(6000), too many records, N = 131072.  k_rank_lean keeps lds_recs = min(S cap, its LDS room, 16 * 1024) records in
    whole 16-byte pieces, at most RL_MAX_PIECES = 1024 of them; choose_rank takes the shape only if that is at least
    2.2 R + 256 + 16 S = 13456 + 16 S, i.e. with S <= 183 segments (the test asks for at most 128: max_segments), and then
    lds_recs = 16384.  Queries 5, 50 and 90 (90 has the code of 5, other labels) have 0.3 R = 1800 rows at distances 1..7 and
    a plateau of 3.3 R = 19800 rows at distance 8, both spread evenly over the database (every 6.6th row); their next row is
    an iid one at ~14 or more.  The plateau alone does not crowd the rank stage: the guess is two-dimensional (k_guess_direct:
    the cut T AND the last segment up to which rows AT distance T are collected), so a bet keeps R + sigma sqrt(24 R) + 24
    records whatever lies at its threshold -- 1.3 R at the default margin of sigma = 5.  What the plateau does is let a WIDE
    margin land inside it: with `guess_sigma` = 36 the bet asks for 24 (250 + 36 sqrt(250) + 1) = 3.3 R = 19700 records, which
    these queries deliver from distance <= 8 (an ordinary query from one or two distances more): more than 16384, more than
    1024 pieces, fewer than the budget of 4 R, ~130 per slice of 256."""
    b, Qn = 64, 96 if R == TOO_MANY_R else 130
    rng = np.random.default_rng(4000 + R)
    if R == LONG_SLICE_R:
        N = 66064
        db, qb = _bits(rng, N, b), _bits(rng, Qn, b)
        for m in LONG_SLICE_BLOCKS:
            for j in range(LONG_SLICE_RUN):
                db[96 * m + j] = _flip(rng, qb[37], 14 + j % 6)
        props = dict(crowded_query=37, blocks=LONG_SLICE_BLOCKS)
    elif R == TOO_MANY_R:
        N = 131072
        db, qb = _bits(rng, N, b), _bits(rng, Qn, b)
        plateau = 33 * R // 10
        base = (np.arange(plateau, dtype=np.int64) * N) // plateau          # every 6.6th row: gaps of 6 or 7
        for q, off in ((5, 0), (50, 3)):
            for k, r in enumerate(base):
                db[(r + off) % N] = _flip(rng, qb[q], 8)
                if k % 11 == 0:
                    db[(r + off + 2) % N] = _flip(rng, qb[q], 1 + (k // 11) % 7)
        qb[90] = qb[5]
        props = dict(plateau_queries=(5, 50, 90), plateau=plateau, plateau_distance=8)
    else:
        raise ValueError("crowded(%d): R is %d (long slice) or %d (too many records)" % (R, LONG_SLICE_R, TOO_MANY_R))
    return _freeze(dict(qbits=qb, dbbits=db, qlab=_labels(rng, Qn), dblab=_labels(rng, N), b=b, R=R, **props))


@functools.lru_cache(maxsize=None)
def reference(name, arg, batch=None):
    """The oracle's answer for a case, computed once per process: reference("spans", 64), reference("cut_at_the_byte_edge", 128, "below")."""
    c = globals()[name](arg)
    q = c[batch] if batch else c
    out = oracle(q["qbits"], c["dbbits"], q["qlab"], c["dblab"], c["R"])
    for a in out:
        a.setflags(write=False)
    return out

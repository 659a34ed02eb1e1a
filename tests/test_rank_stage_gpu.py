"""The rank stage of the sampled-threshold bet (launch_rank in hashgan_amd/csrc/hg_rank.hip), kernel by kernel and branch by
branch, bit-exact against oracle.hamming_map.map_from_codes: per-query AP (nan included), hit counts and -- where the lists
are asked for -- idx, dist and match bits.  No tolerances.

The workloads come from tests/rank_cases.py; tests/test_rank_cases_host.py proves on the CPU that they hold the spans,
thresholds and plateaus the assertions here rely on.  Every test opens a context of its own, so the engine options it sets
(`rank_lds`, `compact_records`, `fuse_ap`, `optimistic`, `inline_leftovers`, `max_segments`) end with it.

"rank_variant": 1 k_rank_fused, 3 k_rank_cnt, 6 k_rank_lean.  "rank_leftovers": queries a fused step's LDS-resident rank kernel
handed to the general one.  With `optimistic` = 0 a call of these sizes goes through enqueue_exact_mx: the matrix-core select
at the EXACT threshold feeding the same rank stage, so what a rank kernel declines is a property of the data alone."""
import math

import numpy as np
import pytest

from hashgan_amd import _native, metric
from tests import cases
from tests import rank_cases as rc
from tests.test_sharded_gpu import _run_virtual

pytestmark = pytest.mark.gpu

FAILS = ("optimistic_fallbacks", "optimistic_requeried", "optimistic_rebets")


def _open(c, queries=None, **options):
    ctx = _native.Context(0)
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        _queries(ctx, queries or c)
    except Exception:
        ctx.close()
        raise
    return ctx


def _queries(ctx, q):
    ctx.set_queries(metric.pack_codes(q["qbits"]), metric.pack_labels(q["qlab"]))


def _first_diff(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return "first mismatch at %s: got %s want %s (%d mismatches)" % (bad[0], a[tuple(bad[0])], b[tuple(bad[0])], len(bad))


def _map_equals(ctx, ref, R, what):
    ap_ref, rel_ref = ref[0], ref[1]
    ap, rel = ctx.map(R)
    assert np.array_equal(rel, rel_ref), "%s: hits: %s" % (what, _first_diff(rel, rel_ref))
    assert np.array_equal(ap, ap_ref, equal_nan=True), "%s: ap: %s" % (what, _first_diff(ap, ap_ref))


def _topr_equals(ctx, ref, R, what):
    ap_ref, rel_ref, imatch_ref, idx_ref, dist_ref = ref
    ctx.topr(R)
    idx, dist = ctx.get_topr()
    assert np.array_equal(dist, dist_ref), "%s: dist: %s" % (what, _first_diff(dist.astype(np.int64), dist_ref))
    assert np.array_equal(idx, idx_ref), "%s: idx: %s" % (what, _first_diff(idx.astype(np.int64), idx_ref))
    m = ctx.get_match().astype(bool)
    assert np.array_equal(m, imatch_ref), "%s: match: %s" % (what, _first_diff(m, imatch_ref))
    ctx.ap()
    ap, rel = ctx.get_ap()
    assert np.array_equal(rel, rel_ref) and np.array_equal(ap, ap_ref, equal_nan=True), "%s: ap after topr" % what


def _stats(ctx, keys):
    return tuple(ctx.get_stat(k) for k in keys)


# ------------------------------------------------------------------------------------------------ a. every kernel, ordinary bet
def _variant_after_map(rank_lds, compact):
    return {2: 6 if compact else 3, 1: 3, 0: 1}[rank_lds]      # (the lean kernel takes one-byte records only)


@pytest.mark.parametrize("b", [16, 64, 100])
def test_every_rank_kernel_on_an_ordinary_bet(b):
    """`rank_lds` x `compact_records` x `fuse_ap` x `optimistic` on iid codes: hg_map, then hg_topr with lists, match bits and
    hg_ap, equal the oracle every time; the bet (or the exact matrix-core sequence) holds, and "rank_variant" says that the kernel
    the options ask for really ranked: k_rank_lean (6) for rank_lds = 2 with one-byte records, k_rank_cnt (3) for rank_lds = 2 with
    8-byte records and for rank_lds = 1, k_rank_fused (1) for rank_lds = 0; with lists wanted 3 for rank_lds >= 1, else 1.

    b = 100 runs with `max_segments` = 200: at the default a database of 66 100 rows of four-word codes is cut into 258 segments
    of 256 rows, k_rank_lean takes at most 256 slices per query (choose_rank), and rank_lds = 2 would mean k_rank_cnt -- the
    table above would then hold 3 where it says 6, and the lean kernel's 34-counter layout would not run at all."""
    c = rc.ordinary(b)
    ref = rc.reference("ordinary", b)
    R = c["R"]
    ctx = _open(c, **({"max_segments": 200} if b == 100 else {}))
    try:
        for rank_lds in (2, 1, 0):
            for compact in (1, 0):
                for fuse in (1, 0):
                    for optimistic in (1, 0):
                        what = "b=%d rank_lds=%d compact_records=%d fuse_ap=%d optimistic=%d" % (b, rank_lds, compact, fuse, optimistic)
                        for k, v in (("rank_lds", rank_lds), ("compact_records", compact), ("fuse_ap", fuse), ("optimistic", optimistic)):
                            ctx.set_option(k, v)
                        f0 = ctx.get_stat("optimistic_fallbacks")
                        _map_equals(ctx, ref, R, what)
                        assert ctx.get_stat("last_optimistic") == 1 and ctx.get_stat("optimistic_fallbacks") == f0, what
                        assert ctx.get_stat("rank_variant") == _variant_after_map(rank_lds, compact), (what, ctx.get_stat("rank_variant"))
                        _topr_equals(ctx, ref, R, what)
                        assert ctx.get_stat("last_optimistic") == 1 and ctx.get_stat("optimistic_fallbacks") == f0, what
                        assert ctx.get_stat("rank_variant") == (3 if rank_lds >= 1 else 1), (what, ctx.get_stat("rank_variant"))
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------- b. span edges
@pytest.mark.parametrize("b", [17, 64, 100])
def test_lists_spanning_more_distances_than_the_lds_kernels_place(b):
    """Queries whose top-R lists span RC_MAXB - 1 .. RC_MAXB + 6 distances (RC_MAXB = 16; 32 at b = 100) among ordinary ones.
    With the exact cut (`optimistic` = 0) k_rank_lean and k_rank_cnt hand over exactly the queries whose span exceeds RC_MAXB:
    RC_MAXB itself is ranked in place, + 1 and + 2 leave through `nbk > RC_MAXB`, wider ones through the counters' window --
    "rank_leftovers" grows by their number, call after call.  With the guessed cut, which may lie above the exact one, by at least
    that number.  The same bits without the inline leftover pass and from the general kernel alone.  (b = 17: a counter for every
    distance, no window; see rank_cases.spans for why its spans are 16 and 17 only.)"""
    c = rc.spans(b)
    ref = rc.reference("spans", b)
    R = c["R"]
    over = int((rc.span_of(ref[4]) > rc.maxb(b)).sum())
    assert over == sum(s > rc.maxb(b) for s in c["planted"].values()) >= 1
    ctx = _open(c, **({"max_segments": 200} if b == 100 else {}))
    try:
        ctx.set_option("optimistic", 0)
        for rank_lds in (2, 1):
            ctx.set_option("rank_lds", rank_lds)
            for call in range(2):                        # (the second call expects the leftovers and ranks them within its stream)
                what = "b=%d exact cut rank_lds=%d call %d" % (b, rank_lds, call)
                l0, f0 = ctx.get_stat("rank_leftovers"), _stats(ctx, FAILS)
                _map_equals(ctx, ref, R, what)
                assert ctx.get_stat("last_optimistic") == 1 and _stats(ctx, FAILS) == f0, what
                assert ctx.get_stat("rank_variant") == (6 if rank_lds == 2 else 3), what
                assert ctx.get_stat("rank_leftovers") - l0 == over, (what, ctx.get_stat("rank_leftovers") - l0, over)
        ctx.set_option("optimistic", 1)
        for rank_lds in (2, 1):
            ctx.set_option("rank_lds", rank_lds)
            what = "b=%d guessed cut rank_lds=%d" % (b, rank_lds)
            l0 = ctx.get_stat("rank_leftovers")
            _map_equals(ctx, ref, R, what)
            assert ctx.get_stat("rank_leftovers") - l0 >= over, (what, ctx.get_stat("rank_leftovers") - l0, over)
        for optimistic in (1, 0):
            ctx.set_option("optimistic", optimistic)
            for options in ({"rank_lds": 2, "inline_leftovers": 0}, {"rank_lds": 1, "inline_leftovers": 0}, {"rank_lds": 0, "inline_leftovers": 1}):
                for k, v in options.items():
                    ctx.set_option(k, v)
                what = "b=%d optimistic=%d %r" % (b, optimistic, options)
                _map_equals(ctx, ref, R, what)
                _map_equals(ctx, ref, R, what + " again")
                _topr_equals(ctx, ref, R, what)
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------- c. the byte edge
@pytest.mark.parametrize("b", [128, 129, 255])
def test_cuts_at_the_largest_distance_of_a_byte_record(b):
    """Exact thresholds 122..127 (`below`) and 126..min(130, b - 1) (`across`) under `optimistic` x `rank_lds` x `compact_records`,
    hg_map and hg_topr: the oracle's bits in every combination.  For `below` with the exact cut the bet's rank stage itself must
    have ranked -- thresholds up to 127 on byte records --, not the vector-ALU exact sequence: last_optimistic == 1, no fallback.
    There k_rank_lean (one-byte records, `max_segments` = 200 so that it takes the shape) declines exactly the queries whose cut
    is 127 -- the padding of a slice's last piece is the distance cut + 1, which seven bits hold up to 127 -- and k_rank_cnt none.
    A cut beyond 127 (`across`) may lose: results only."""
    c = rc.cut_at_the_byte_edge(b)
    R = c["R"]
    ctx = _open(c, queries=c["below"], max_segments=200)
    try:
        for batch in ("below", "across"):
            q = c[batch]
            ref = rc.reference("cut_at_the_byte_edge", b, batch)
            _queries(ctx, q)
            at_127 = int((q["thresholds"] == 127).sum())
            for optimistic in (1, 0):
                for rank_lds in (2, 1, 0):
                    for compact in (1, 0):
                        what = "b=%d %s optimistic=%d rank_lds=%d compact_records=%d" % (b, batch, optimistic, rank_lds, compact)
                        for k, v in (("optimistic", optimistic), ("rank_lds", rank_lds), ("compact_records", compact)):
                            ctx.set_option(k, v)
                        l0, f0 = ctx.get_stat("rank_leftovers"), _stats(ctx, FAILS)
                        _map_equals(ctx, ref, R, what)
                        if batch == "below" and optimistic == 0:
                            assert ctx.get_stat("last_optimistic") == 1 and _stats(ctx, FAILS) == f0, what
                            assert ctx.get_stat("rank_variant") == _variant_after_map(rank_lds, compact), (what, ctx.get_stat("rank_variant"))
                            left = ctx.get_stat("rank_leftovers") - l0
                            assert left == (at_127 if rank_lds == 2 and compact else 0), (what, left, at_127)
                        _topr_equals(ctx, ref, R, what)
                        if batch == "below" and optimistic == 0:
                            assert ctx.get_stat("last_optimistic") == 1 and _stats(ctx, FAILS) == f0, what
    finally:
        ctx.close()


def test_a_cut_at_the_code_length_128_is_answered_exactly():
    """Threshold 128 = b, the one value beyond 127 that two-word-pair codes reach (k_select_mx4's `T > 127`): all rows but 400 are
    the queries' complement.  Nothing here can win a bet; the results are the oracle's."""
    c = rc.plateau_at_b(128)
    ref = rc.reference("plateau_at_b", 128)
    ctx = _open(c)
    try:
        for optimistic in (1, 0):
            for rank_lds in (2, 0):
                ctx.set_option("optimistic", optimistic)
                ctx.set_option("rank_lds", rank_lds)
                what = "optimistic=%d rank_lds=%d" % (optimistic, rank_lds)
                _map_equals(ctx, ref, c["R"], what)
                _topr_equals(ctx, ref, c["R"], what)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ d. record-count branches
def _segment_rows(N, S, b):
    """The segment length behind stat "segments": the one multiple of the select's row tile (96 rows for codes of <= 64 bits, else
    32: make_geometry) that cuts N rows into S segments."""
    lq = 96 if b <= 64 else 32
    Ls = [L for L in range(lq, N + lq, lq) if -(-N // L) == S]
    assert len(Ls) == 1, (N, S, Ls)
    return Ls[0]


def _spec_pieces(cap, S):
    """choose_rank's PSP: the 16-byte pieces of a slice k_rank_lean fetches before it knows the slice's count."""
    est = 0.7 * (math.sqrt(max(cap - 7.0, 0.0)) - 3.0) ** 2
    return max(1, min(math.ceil((est + 4.0 * math.sqrt(est) + 1.0) / 16.0), cap >> 4, 1024 // S))


def test_a_slice_longer_than_the_speculative_fetch():
    """k_rank_lean's `pc > PSP` tail: three slices of query 37 hold 50+ records, more than the PSP pieces fetched up front and
    fewer than a slice's capacity (both from the launcher's own numbers: stats "slice_cap", "segments").  Ranked in place -- no
    leftover, no lost bet --, the oracle's bits; then the same from k_rank_cnt and k_rank_fused."""
    R = rc.LONG_SLICE_R
    c = rc.crowded(R)
    ref = rc.reference("crowded", R)
    q = c["crowded_query"]
    N = c["dbbits"].shape[0]
    t = ref[4][q, -1]
    D = rc.O.hamming_matrix(rc.O.pack_bits(c["qbits"][q:q + 1]), rc.O.pack_bits(c["dbbits"]))[0]
    ctx = _open(c)
    try:
        for optimistic in (1, 0):
            ctx.set_option("optimistic", optimistic)
            ctx.set_option("rank_lds", 2)
            what = "optimistic=%d" % optimistic
            l0, f0 = ctx.get_stat("rank_leftovers"), _stats(ctx, FAILS)
            _map_equals(ctx, ref, R, what)
            assert ctx.get_stat("last_optimistic") == 1 and _stats(ctx, FAILS) == f0 and ctx.get_stat("rank_leftovers") == l0, what
            assert ctx.get_stat("rank_variant") == 6, what
            S, cap = ctx.get_stat("segments"), ctx.get_stat("slice_cap")
            L = _segment_rows(N, S, c["b"])
            inside = np.add.reduceat((D < t).astype(np.int64), np.arange(0, N, L))       # records of ANY cut >= t, per slice
            psp = _spec_pieces(cap, S)
            dense = sorted({96 * m // L for m in c["blocks"]})
            print(what, "segments", S, "rows", L, "slice_cap", cap, "PSP", psp, "dense slices", [int(inside[s]) for s in dense], "others <=", int(np.delete(inside, dense).max()))
            assert all(16 * psp < inside[s] <= cap for s in dense), (S, L, cap, psp, inside[dense])
            assert np.delete(inside, dense).max() <= 16 * psp
        for rank_lds in (1, 0):
            ctx.set_option("rank_lds", rank_lds)
            _map_equals(ctx, ref, R, "rank_lds=%d" % rank_lds)
    finally:
        ctx.close()


def test_more_records_than_the_lean_kernel_holds():
    """R = 6000, N = 131072, three queries with a tie plateau of 3.3 R rows at their threshold.  At the default margin the plateau
    costs nothing (the guess also picks the last segment whose ties it collects: 1.3 R records) and k_rank_lean ranks every query
    in place.  With `guess_sigma` = 36 the bet keeps about 24 (R / 24 + 36 sqrt(R / 24) + 1) = 3.3 R records per query -- more than
    k_rank_lean's record capacity (stat "rank_lds_recs"; 16 * 1024 = RL_MAX_PIECES pieces at most), inside the bet's budget of 4 R
    and every slice's capacity (stats "records_kept", "segments", "slice_cap"): the bet holds, the lean kernel declines the queries
    (`n16 * 16 > lds_recs`, `n16 > RL_MAX_PIECES`) and the general kernel -- after the step, then within the next step's stream --
    ranks them.  k_rank_cnt takes such a list in two tiles.  `max_segments` = 128: choose_rank takes R = 6000 only with <= 183
    segments (rank_cases.crowded says why)."""
    R = rc.TOO_MANY_R
    c = rc.crowded(R)
    ref = rc.reference("crowded", R)
    Q = c["qbits"].shape[0]
    ctx = _open(c, max_segments=128)
    try:
        l0, f0 = ctx.get_stat("rank_leftovers"), _stats(ctx, FAILS)
        _map_equals(ctx, ref, R, "default margin")
        assert ctx.get_stat("last_optimistic") == 1 and _stats(ctx, FAILS) == f0 and ctx.get_stat("rank_variant") == 6
        print("default margin: records / (Q R)", ctx.get_stat("records_kept") / (Q * R), "leftovers", ctx.get_stat("rank_leftovers") - l0)
        ctx.set_option("guess_sigma", 36)
        for call in range(2):
            l0, f0 = ctx.get_stat("rank_leftovers"), _stats(ctx, FAILS)
            _map_equals(ctx, ref, R, "rank_lds=2 call %d" % call)
            assert ctx.get_stat("last_optimistic") == 1 and _stats(ctx, FAILS) == f0
            assert ctx.get_stat("rank_variant") == 6
            recs, S, cap, kept = (ctx.get_stat(k) for k in ("rank_lds_recs", "segments", "slice_cap", "records_kept"))
            print("call", call, "segments", S, "slice_cap", cap, "rank_lds_recs", recs, "records / (Q R)", kept / (Q * R), "leftovers", ctx.get_stat("rank_leftovers") - l0)
            assert recs <= 16 * 1024 and 16 * 1024 * Q < kept < 4 * R * Q and 4 * R < S * cap      # (on average; the margin is the same for every query)
            assert ctx.get_stat("rank_leftovers") - l0 >= len(c["plateau_queries"])
        for rank_lds in (1, 0):
            ctx.set_option("rank_lds", rank_lds)
            f0 = _stats(ctx, FAILS)
            _map_equals(ctx, ref, R, "rank_lds=%d" % rank_lds)
            assert _stats(ctx, FAILS) == f0 and ctx.get_stat("rank_variant") == (3 if rank_lds else 1)
            if rank_lds == 1:
                assert ctx.get_stat("rank_lds_recs") < 3 * R       # (two tiles)
    finally:
        ctx.close()


# -------------------------------------------------------------------------------------------------- e. the sharded form
@pytest.mark.parametrize("rank_lds", [1, 0])
def test_virtual_shards_rank_locally_with_every_kernel(rank_lds, case_cache):
    """The merged-ranking bet (rank kernels' mode 3: every shard ranks its own records, hg_merge_ranked stitches the bitmaps) with
    k_rank_cnt and with k_rank_fused on every shard: the golden AP of the unmodified reference, on the one-pass route."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    res = _run_virtual(c, 4, gather_topr=False, options={"rank_lds": rank_lds})
    for r in range(4):
        ap, rel = res[r]
        assert np.array_equal(ap, g["ap"], equal_nan=True), (rank_lds, r)
    assert all(st == (1, 0) for st in _run_virtual.last_stats), _run_virtual.last_stats

"""The first two stages of the bet, kernel by kernel: the sampled histogram pass (k_hist at a batch stride, k_hist_mx, k_hist_i8) and
the guessed cut (k_guess; k_guess_owner / k_guess_finish in the owner-routed form; k_guess_direct in the one-shot step).  The bet
is verified on the device, so a wrong sample or a wrong guess never changes a result -- it only costs records or a lost bet -- and
end-to-end parity cannot fail for these kernels.  Here their own outputs are read: the tables behind hg_hist_buffer, uint32
[b + 1][Qpad] + 64 tail words ([0] overflow flag, [1] rows visited), downloaded with hg_memcpy_dtoh.  With "stage_sync" = 1 (the
default, kept here) every staged call returns after its kernels have finished, and hg_memcpy_dtoh is enqueued on the same stream
and waits for it: the download sees the finished stage either way.

All comparisons are on integers and exact; the one float is the guess's `need`, computed in float64 by the documented formula and
required to lie more than 1e-9 from an integer.  The host side is tests/sample_cases.py, proven on the CPU by
tests/test_sample_cases_host.py.

"hist_variant": 1 k_hist, 2 k_hist_mx, 3 k_hist_i8; 6 / 7: k_hist_mx / k_hist_i8 with dword counters instead of 16-bit halves."""
import functools
import warnings

import numpy as np
import pytest

from hashgan_amd import _native, metric
from hashgan_amd.sharded import shard_bounds
from oracle import hamming_map as O
from tests import sample_cases as sc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _open(**options):
    ctx = _native.Context(0)
    try:
        ctx.set_option("staged_lists", 0)
        for k, v in options.items():
            ctx.set_option(k, v)
    except Exception:
        ctx.close()
        raise
    return ctx


def _load_db(ctx, dbbits, dblab, idx_base=0, n_total=None):
    ctx.set_database(metric.pack_codes(dbbits), metric.pack_labels(dblab), dbbits.shape[1], dblab.shape[1], idx_base, n_total)


def _load_q(ctx, qbits, qlab):
    ctx.set_queries(metric.pack_codes(qbits), metric.pack_labels(qlab))


def _table(ctx):
    """The table behind hg_hist_buffer -> (int64 [b + 1, Q] of the live queries, overflow flag, rows visited)."""
    ptr, nbytes = ctx.hist_buffer()
    words = np.empty(nbytes // 4, np.uint32)
    ctx.memcpy_dtoh(words, ptr, nbytes)
    return sc.split_table(words, ctx.b, ctx.Q)


def _first_diff(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return "first mismatch at [d, q] = %s: got %s want %s (%d mismatches)" % (bad[0], a[tuple(bad[0])], b[tuple(bad[0])], len(bad))


def _oracle_ap(qbits, dbbits, qlab, dblab, R):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, imatch, _, _ = O.map_from_codes(qbits, dbbits, qlab, dblab, R)
    return ap, imatch.sum(1)


def _discover(ctx, rng, b, N, Q, variant, dblab, qlab, idx_base=0, n_total=None, keep_launches=False):
    """What the sampled pass of this context -- its options, and a database of N rows of b bits under Q queries -- visits, from probe
    launches alone: -> dict(visited = boolean mask [N], vbatches, B, launches = [(dist [Q, N], table, rows-visited word)], segments).
    `variant`: the "hist_variant" every launch must report (it decides the batch the probe numbers: sample_cases.unit_rows).
    Single probe for one query (N <= B (b + 1)); else the two-level probe, window by window, with random queries beside the probe
    queries so that the query count -- the geometry depends on it -- is the case's own."""
    B = sc.unit_rows(variant == 1, b)
    launches, counts = [], []
    if Q == 1:
        qbits = np.zeros((1, b), np.uint8)
        dbs = [sc.single_db(rng, b, B, N)]
        m = w = None
    else:
        m, w = sc.probe_split(b, Q - 3)
        qbits = np.concatenate([sc.probe_queries(b, m, w), sc.bits(rng, Q - w, b)])
        dbs = (sc.probe_db(b, B, N, m, w, k) for k in range(sc.probe_windows(N, B, m, w)))
    segments = None
    for k, db in enumerate(dbs):
        _load_db(ctx, db, dblab, idx_base, n_total)
        _load_q(ctx, qbits, qlab)                                       # (a new database takes the queries with it)
        ctx.sample_hist(1)
        table, flag, visited = _table(ctx)
        assert flag == 0
        assert ctx.get_stat("hist_variant") == variant, ("hist_variant", ctx.get_stat("hist_variant"), "expected", variant)
        assert segments in (None, ctx.get_stat("segments"))             # (the same launch every time: nothing depends on the data)
        segments = ctx.get_stat("segments")
        counts.append(table[:-(-N // B), 0] if Q == 1 else sc.decode(table, B, N, m, w, k))
        if keep_launches:
            launches.append((sc.distances(qbits, db).astype(np.int16), table, visited))
    mask, vb = sc.visited_rows(np.concatenate(counts), N, B)            # every probe count 0 or its whole batch
    return dict(visited=mask, vbatches=vb, B=B, launches=launches, segments=segments, segs={})


def _check_sample(what, dist, table, visited_word, mask, b):
    """A sampled table against the visited set: the rows-visited word is |V|, every live query's column sums to it, and every
    column IS the histogram of the query's distances over V."""
    assert visited_word == int(mask.sum()), "%s: the tail says %d rows visited, the probe found %d" % (what, visited_word, int(mask.sum()))
    assert (table.sum(0) == visited_word).all(), "%s: column sums %s, rows visited %d" % (what, table.sum(0), visited_word)
    want = sc.histogram(dist, b, mask)
    assert np.array_equal(table, want), "%s: %s" % (what, _first_diff(table, want))


# -------------------------------------------------------------------------------------- 1. the sample is a definite set of rows
# (hist_mfma, b, sample_stride, N, Q, geometry options, hist_variant expected); every kernel at b = 1, 31, 32, 33, 64, 65, 127, 128 -- the
# edges of the 32-bit code words and of the 64-bit fp4 image -- and k_hist_mx and k_hist, which take longer codes, at 200 and 255 too
_GEO3 = {"max_segments": 3}                   # three segments: an odd count, the last one without a partner in its pair
_SHORT = {"min_segment": 16}                  # segments of the least length: 96 rows of <= 64 bits, 32 of longer codes
_ONE = {"max_segments": 1}                    # one segment of >= 65504 rows at stride 2: dword counters (>= 65536 visited rows per pair)
SAMPLE_CASES = [
    # k_hist_i8 (codes of <= 128 bits)
    (2, 1, 2, 32, 1, {}, 3), (2, 31, 3, 5000, 33, _SHORT, 3), (2, 32, 2, 3000, 70, _GEO3, 3), (2, 33, 24, 4099, 130, _SHORT, 3),
    (2, 64, 3, 5989, 70, {}, 3), (2, 65, 2, 9001, 33, _GEO3, 3), (2, 127, 24, 22521, 130, _SHORT, 3), (2, 128, 3, 25000, 70, {}, 3),
    (2, 64, 2, 65531, 33, _ONE, 7),
    # k_hist_mx (any length; hist_mfma = 2 with codes beyond 128 bits is this kernel too)
    (1, 1, 2, 32, 1, {}, 2), (1, 32, 2, 5000, 33, _GEO3, 2), (1, 65, 3, 7000, 70, _SHORT, 2), (1, 128, 24, 24997, 130, {}, 2),
    (1, 200, 2, 12000, 33, {}, 2), (1, 255, 3, 20011, 130, _GEO3, 2), (1, 127, 2, 65531, 70, _ONE, 6), (2, 200, 24, 3000, 33, {}, 2),
    (1, 31, 24, 4003, 130, _SHORT, 2), (1, 33, 3, 3001, 70, {}, 2), (1, 64, 2, 5989, 33, _GEO3, 2), (1, 127, 3, 6007, 33, _SHORT, 2),
    # hist_mx_applies declines: dword counters for 201 distances exceed the LDS (4 x 2 x 201 x 128 bytes > 160 KiB) -- k_hist
    (1, 200, 2, 65531, 33, _ONE, 1),
    # k_hist: batches of 16, 8 and 4 rows
    (0, 1, 2, 32, 1, {}, 1), (0, 31, 3, 5000, 70, _GEO3, 1), (0, 64, 24, 5989, 130, _SHORT, 1), (0, 65, 2, 9001, 33, {}, 1),
    (0, 128, 3, 25000, 70, {"max_segments": 5}, 1), (0, 200, 24, 8000, 33, _SHORT, 1), (0, 255, 2, 21003, 130, {}, 1),
    (0, 32, 2, 3000, 33, _SHORT, 1), (0, 33, 24, 4099, 70, {}, 1), (0, 127, 3, 6007, 130, _GEO3, 1),
]


@pytest.mark.parametrize("hist_mfma,b,stride,N,Q,geometry,variant", SAMPLE_CASES,
                         ids=["mfma%d-b%d-s%d-N%d-Q%d%s" % (c[0], c[1], c[2], c[3], c[4], "".join("-%s%d" % kv for kv in c[5].items())) for c in SAMPLE_CASES])
def test_sampled_histogram_is_the_exact_histogram_of_a_definite_set_of_rows(hist_mfma, b, stride, N, Q, geometry, variant):
    """The visited set V is read off probe launches (sample_cases.probe_db: every batch's number is in its rows' codes), then:

      - every probe count is 0 or its whole batch: no batch partly, none twice;
      - tail word [1] = |V| in rows, and every live query's column sums to it (the host's mirror of the kernel's walk);
      - every live query's column -- the random queries that share the probe launches, and all queries of a second launch on a
        random database of the same shape, for which V is reused: sampling must not depend on the data -- equals np.bincount of
        its distances over V, exactly;
      - coverage (sample_cases.coverage, from the rule "every stride-th batch of each segment"): |V| stride >= N - (ragged segment
        ends: the N mod B rows behind k_hist's last whole batch -- its segments are whole batches otherwise --, nothing for the
        matrix-core kernels, which count a ragged tile by its rows), batch 0 visited, no two consecutive visited batches more than `stride` apart, the last one among
        the last `stride` batches;
      - the sampled table is elementwise <= the full histogram of the same context, which equals NumPy's.

    "hist_variant" says which kernel ran; where the code declines a kernel for the shape (hist_mx_applies) the case asserts that."""
    rng = np.random.default_rng([hist_mfma, b, stride, N, Q])
    dblab, qlab = sc.labels(rng, N), sc.labels(rng, Q)
    ctx = _open(hist_mfma=hist_mfma, sample_stride=stride, **geometry)
    try:
        what = "hist_mfma=%d b=%d stride=%d N=%d Q=%d %s" % (hist_mfma, b, stride, N, Q, geometry)
        found = _discover(ctx, rng, b, N, Q, variant, dblab, qlab, keep_launches=True)
        S = found["segments"]
        if geometry is _GEO3:
            assert S == 3, (what, S)
        if geometry is _SHORT:
            assert 4 * S >= 3 * -(-N // (96 if b <= 64 else 32)), (what, S)           # (the least length, or a count within a quarter of it)
        if geometry is _ONE:
            assert S == 1, (what, S)
        mask, vb = found["visited"], found["vbatches"]
        for k, (dist, table, visited_word) in enumerate(found["launches"]):
            _check_sample("%s, probe launch %d" % (what, k), dist, table, visited_word, mask, b)
        bad = sc.coverage_violations(vb, int(mask.sum()), N, found["B"], stride, variant != 1)
        assert not bad, (what, bad)
        # a random database of the same shape, random queries: the same rows
        qbits, dbbits = sc.bits(rng, Q, b), sc.bits(rng, N, b)
        _load_db(ctx, dbbits, dblab)
        _load_q(ctx, qbits, qlab)
        ctx.sample_hist(1)
        table, flag, visited_word = _table(ctx)
        assert flag == 0 and ctx.get_stat("hist_variant") == variant and ctx.get_stat("segments") == S, what
        dist = sc.distances(qbits, dbbits)
        _check_sample(what + ", random database", dist, table, visited_word, mask, b)
        ctx.hist()
        full = ctx.get_hist().astype(np.int64)
        assert np.array_equal(full, sc.histogram(dist, b)), what
        assert (table <= full).all(), what
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------- 2. the guess is the documented rule
@functools.lru_cache(maxsize=2)
def _bet_case(b, N, Q, p=0.5, far=None):
    """iid codes (bits set with probability p) in the bet's range; `far`: that query is all ones -- with p = 0.15 every row lies beyond
    b / 2 + 2 of it.  (Two cases are kept at a time -- consecutive tests share them -- and the distances as int16: a case is tens
    of megabytes.)"""
    rng = np.random.default_rng([b, N, Q, int(p * 100)])
    c = dict(b=b, N=N, Q=Q, qbits=sc.bits(rng, Q, b, p), dbbits=sc.bits(rng, N, b, p), qlab=sc.labels(rng, Q), dblab=sc.labels(rng, N))
    if far is not None:
        c["qbits"][far] = 1
    c["dist"] = sc.distances(c["qbits"], c["dbbits"]).astype(np.int16)
    c["H"] = sc.histogram(c["dist"], b)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=16)                 # (per-query AP and hit counts only: a few kilobytes each)
def _bet_oracle(b, N, Q, p, far, R):
    c = _bet_case(b, N, Q, p, far)
    return _oracle_ap(c["qbits"], c["dbbits"], c["qlab"], c["dblab"], R)


def _reference_for(c, shards, founds, S_of, need):
    """For every combination of candidate segment lengths (sample_cases.segment_lengths: "segments" does not say which length the
    geometry took) -> [(lengths, T, found, keep)]; T and found do not depend on the lengths."""
    out = []
    lens = [sc.segment_lengths(n, S_of[r]) for r, (_, n) in enumerate(shards)]
    assert all(lens), (shards, S_of)

    def walk(r, chosen):
        if r == len(shards):
            segs = []
            for i, (lo, n) in enumerate(shards):
                if chosen[i] not in founds[i]["segs"]:
                    founds[i]["segs"][chosen[i]] = sc.segment_counts(c["dist"][:, lo:lo + n], founds[i]["visited"], c["b"], n, chosen[i])
                segs.append(founds[i]["segs"][chosen[i]])
            out.append((tuple(chosen),) + sc.guess(segs, need))
            return
        for L in lens[r]:
            walk(r + 1, chosen + [L])
    walk(0, [])
    assert len(out) <= 16, "too many candidate geometries to try: %s" % (lens,)
    return out


def _check_records(what, c, shard, rec, flag, refs, r, cap):
    """One shard's record table against the reference: exact below and above the cut for every candidate geometry (the cut does not
    depend on it); AT the cut one candidate must explain every query.  -> the candidates that do."""
    lo, n = shard
    dist = c["dist"][:, lo:lo + n]
    H = sc.histogram(dist, c["b"])
    _, T, found, _ = refs[0]
    for q in range(c["Q"]):
        t = int(T[q])
        assert np.array_equal(rec[:t, q], H[:t, q]), "%s: query %d below the cut %d: %s / %s" % (what, q, t, rec[:t + 1, q], H[:t + 1, q])
        assert not rec[t + 1:, q].any(), "%s: query %d holds records beyond the cut %d: %s" % (what, q, t, np.nonzero(rec[:, q])[0])
        assert 0 <= rec[t, q] <= H[t, q], (what, q)
    fits = []
    for lengths, T, found, keep in refs:
        want = sc.records(dist, c["b"], n, lengths[r], T, found, keep[r])
        if np.array_equal(rec, want):
            fits.append((lengths, keep))
            assert sc.fullest_slice(dist, n, lengths[r], T, found, keep[r]) <= cap, (what, "the reference itself overflows a slice of", cap)
    want_any = [sc.records(dist, c["b"], n, lengths[r], T, found, keep[r])[T, np.arange(c["Q"])] for lengths, T, found, keep in refs]
    assert fits, "%s: the records AT the cut fit no candidate geometry: got %s, candidates %s" % (what, rec[refs[0][1], np.arange(c["Q"])], want_any)
    assert flag == 0, (what, "overflow flag raised although every slice of the reference fits", cap)
    return fits


BET_CASES = [(32, 66017, 33, {}), (64, 68003, 130, {}), (100, 69989, 33, {"max_segments": 200})]


@pytest.mark.parametrize("b,N,Q,options", BET_CASES, ids=["b%d-N%d-Q%d" % c[:3] for c in BET_CASES])
def test_guess_is_the_documented_rule_applied_to_the_sample(b, N, Q, options):
    """hg_sample_hist, hg_guess, hg_select_candidates on iid codes, R in {1, 50, 1000, N // 9} x guess_sigma in {0, 5, 12}; the record
    table that hg_hist_buffer then holds is the observable.  Reference (sample_cases.guess, integers on the per-segment sample counts
    that V gives): need = ceil(f R + sigma sqrt(f R) + 1) with f = |V| / N; T = the smallest distance whose cumulative sample count
    reaches need; rows AT T are collected inside the smallest prefix of sampled segments whose count of {dist < T} + {dist = T inside
    the prefix} reaches need.  So with H the full NumPy histogram:

      rec[d] = H[d] for d < T,   rec[d] = 0 for d > T,   rec[T] = the rows at distance T inside the prefix,

    and tail word [0] = 0: the reference's fullest slice is checked against "slice_cap" on the host first.  The select segment length
    is not a stat: every length consistent with "segments" is tried and ONE of them must explain all queries at once
    (sample_cases.segment_lengths).  Where the prefix is a proper one rec[T] < H[T] for at least one query -- a guess that always
    collects the cut's bucket everywhere fails here whatever the geometry.

    The verdict of hg_rank is the reference's too.  The margin is what makes a bet hold: with guess_sigma = 0 the cut is placed where
    the SAMPLE reaches f R + 1, and the rows below it come up short of R for nearly every other query -- that bet is lost by design, not
    by a fault.  So the bet must be reported held exactly when the reference's records reach R for every query (they always do at
    guess_sigma = 5 and 12 here, asserted), and then the AP is the oracle's."""
    c = _bet_case(b, N, Q)
    rng = np.random.default_rng([b, N, Q, 2])
    ctx = _open(**options)
    try:
        found = _discover(ctx, rng, b, N, Q, 3, c["dblab"], c["qlab"])      # (the default: k_hist_i8)
        mask, S = found["visited"], found["segments"]
        assert not sc.coverage_violations(found["vbatches"], int(mask.sum()), N, 16, 24, True)
        _load_db(ctx, c["dbbits"], c["dblab"])
        _load_q(ctx, c["qbits"], c["qlab"])
        proper = nheld = 0
        for R in (1, 50, 1000, N // 9):
            for sigma in (0, 5, 12):
                what = "b=%d N=%d Q=%d R=%d guess_sigma=%d" % (b, N, Q, R, sigma)
                ctx.set_option("guess_sigma", sigma)
                ctx.sample_hist(R)
                table, flag, visited_word = _table(ctx)
                _check_sample(what, c["dist"], table, visited_word, mask, b)
                need, v = sc.need_of(R, visited_word, N, sigma)
                assert sc.need_is_safe(v), (what, v)
                ctx.guess(R)
                ctx.select_candidates()
                rec, flag, _ = _table(ctx)
                assert ctx.get_stat("segments") == S
                refs = _reference_for(c, [(0, N)], [found], [S], need)
                assert refs[0][2].all(), what                              # (a cut is found for every query)
                fits = _check_records(what, c, (0, N), rec, flag, refs, 0, ctx.get_stat("slice_cap"))
                T = refs[0][1]
                held = bool((rec.sum(0) >= R).all())                       # (rec IS the reference's table by now)
                assert held or sigma == 0, (what, rec.sum(0).min())
                for lengths, keep in fits:
                    short = keep[0] < -(-N // (sc.SAMPLE_RATIO * lengths[0]))
                    cut = rec[T, np.arange(Q)]
                    assert (cut[short] <= c["H"][T, np.arange(Q)][short]).all()
                    proper += int((cut[short] < c["H"][T, np.arange(Q)][short]).sum())
                assert ctx.rank() is (not held), (what, held)               # the verdict the reference predicts
                if not held:
                    continue
                nheld += 1
                ctx.match()
                ctx.ap()
                ap, rel = ctx.get_ap()
                ap_ref, rel_ref = _bet_oracle(b, N, Q, 0.5, None, R)
                assert np.array_equal(rel, rel_ref) and np.array_equal(ap, ap_ref, equal_nan=True), what
        assert proper > 0 and nheld >= 8
    finally:
        ctx.close()


@pytest.mark.parametrize("b", [32, 64])
def test_a_sample_too_thin_for_the_guess_takes_every_row(b):
    """sample_stride = 1024 on two segments leaves a sample of a few tiles; with R = 0.9 N and guess_sigma = 12 the count the cut must
    reach exceeds the whole sample.  The reference then gives T = b for every query and no prefix: every row becomes a record -- or
    the overflow flag is raised.  Which: the budget 4 R / S exceeds a segment, so the capacity is cut to a whole segment's rows
    rounded up to 16 ("slice_cap" is that of one of the candidate lengths) and no slice can overflow.  b = 32: the flag stays 0 and the
    record table is the full histogram.  b = 64: the cut T = 64 is the one value k_select_mx3 ("select_variant" 5) declines -- its 7-bit
    fields hold T - dist + 64 for T <= 63 only, "such a query loses its bet" (hg_select_mx3.hpp) -- so the flag is raised.  What the
    record table holds for a query that has lost is unspecified (the kernel takes such a query out of its pass and the rank stage
    skips its records), so it is not looked at there."""
    N, Q = 66017, 33
    c = _bet_case(b, N, Q)
    R = N - N // 10
    ctx = _open(sample_stride=1024, max_segments=2, guess_sigma=12)
    try:
        found = _discover(ctx, np.random.default_rng(77), b, N, Q, 3, c["dblab"], c["qlab"])
        mask, S = found["visited"], found["segments"]
        assert S == 2 and 0 < mask.sum() < 1024
        _load_db(ctx, c["dbbits"], c["dblab"])
        _load_q(ctx, c["qbits"], c["qlab"])
        ctx.sample_hist(R)
        table, flag, visited_word = _table(ctx)
        _check_sample("thin sample", c["dist"], table, visited_word, mask, b)
        need, v = sc.need_of(R, visited_word, N, 12)
        assert sc.need_is_safe(v) and need > visited_word
        lens = sc.segment_lengths(N, S)
        T, found_cut, keep = sc.guess([sc.segment_counts(c["dist"], mask, b, N, lens[0])], need)
        assert (T == b).all() and not found_cut.any()
        ctx.guess(R)
        ctx.select_candidates()
        rec, flag, _ = _table(ctx)
        assert ctx.get_stat("slice_cap") in {(L + 15) // 16 * 16 for L in lens}
        if b == 64:
            assert ctx.get_stat("select_variant") == 5 and flag == 1
        else:
            assert flag == 0
            assert np.array_equal(rec, c["H"]), _first_diff(rec, c["H"])
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------- 3. the three forms of the guess agree
def _exchange(ctxs, slot, bufs, all_to_all):
    """The exchange of G virtual ranks on one GPU, as sharded.LocalComm makes it: device-to-device copies into every rank's own
    scratch.  bufs[r] = (address, bytes) on rank r; all-gather: rank r receives every rank's whole buffer; all-to-all: block r of every
    rank's buffer.  (Every producing stage has synchronised: stage_sync = 1.)  -> the addresses of the received buffers."""
    G = len(ctxs)
    n = bufs[0][1]
    assert all(nb == n for _, nb in bufs)
    per = n // G if all_to_all else n
    out = []
    for r, ctx in enumerate(ctxs):
        base = ctx.scratch(slot, per * G)
        for s, (ptr, _) in enumerate(bufs):
            ctx.memcpy_dtod(base + s * per, ptr + (r * per if all_to_all else 0), per)
        out.append(base)
    return out


def _open_shards(c, G, rng, **options):
    """G contexts on one GPU, shard r with rows shard_bounds(N, G)[r] of the case; the visited set of every shard from probes."""
    shards = shard_bounds(c["N"], G)
    ctxs, founds = [], []
    try:
        for lo, n in shards:
            ctx = _open(**options)
            ctxs.append(ctx)
            founds.append(_discover(ctx, rng, c["b"], n, c["Q"], 3, c["dblab"][lo:lo + n], c["qlab"], lo, c["N"]))
            _load_db(ctx, c["dbbits"][lo:lo + n], c["dblab"][lo:lo + n], lo, c["N"])
            _load_q(ctx, c["qbits"], c["qlab"])
    except Exception:
        for ctx in ctxs:
            ctx.close()
        raise
    return shards, ctxs, founds


def _gathered_form(ctxs, R):
    """sample -> all-gather -> hg_guess -> hg_select_candidates on every rank -> [(sampled table, rows visited)], [(record table, flag)]."""
    G = len(ctxs)
    for ctx in ctxs:
        ctx.sample_hist(R)
    samples = [_table(ctx) for ctx in ctxs]
    gathered = _exchange(ctxs, 0, [ctx.hist_buffer() for ctx in ctxs], False)
    for r, ctx in enumerate(ctxs):
        ctx.guess(R, gathered[r], G, r)
    for ctx in ctxs:
        ctx.select_candidates()
    return [(t, v) for t, _, v in samples], [_table(ctx)[:2] for ctx in ctxs]


def _routed_form(ctxs, R):
    """sample -> hg_pack_sample_by_owner -> all-to-all -> hg_guess_owned -> all-to-all -> hg_guess_finish -> hg_select_ranked
    -> [(record table, flag)]."""
    G = len(ctxs)
    for ctx in ctxs:
        ctx.sample_hist(R)
    packed = []
    for ctx in ctxs:
        p, n = ctx.pack_sample_by_owner(G)
        packed.append((p, n * G))
    recv = _exchange(ctxs, 2, packed, True)
    answers = []
    for r, ctx in enumerate(ctxs):
        p, n = ctx.guess_owned(R, recv[r], G, r)
        answers.append((p, n * G))
    back = _exchange(ctxs, 3, answers, True)
    for r, ctx in enumerate(ctxs):
        ctx.guess_finish(R, back[r], G, r)
    for ctx in ctxs:
        ctx.select_ranked()
    return [_table(ctx)[:2] for ctx in ctxs]


@pytest.mark.parametrize("G,Q", [(2, 33), (3, 70)])
def test_sharded_guess_in_both_forms_leaves_the_records_the_reference_predicts(G, Q):
    """G shards of one database as G contexts on one GPU (Q does not divide by G).  All-gather form: T comes from the summed samples,
    the prefix runs over the shards in rank order and then over a shard's sampled segments -- every rank's record table after
    hg_select_candidates is the reference's for that rank (lower shards collect the cut's bucket everywhere, the shard where the
    prefix ends up to a segment, higher ones not at all), and hg_rank on the gathered record tables reports the bet held exactly when
    the reference's records reach R for every query (guess_sigma = 0 loses by design, see above).  Owner-routed
    form (hg_pack_sample_by_owner -> all-to-all -> hg_guess_owned -> all-to-all -> hg_guess_finish -> hg_select_ranked): the same
    record tables bit for bit, "cut_beyond_planes" = 0."""
    b, N = 64, 66017 + G
    c = _bet_case(b, N, Q)
    shards, ctxs, founds = _open_shards(c, G, np.random.default_rng([G, Q]))
    try:
        S_of = [f["segments"] for f in founds]
        sampled_rows = sum(int(f["visited"].sum()) for f in founds)
        partial = 0
        for R, sigma in ((50, 5), (1000, 0), (N // 9, 12)):
            what = "G=%d Q=%d R=%d guess_sigma=%d" % (G, Q, R, sigma)
            for ctx in ctxs:
                ctx.set_option("guess_sigma", sigma)
            samples, recs = _gathered_form(ctxs, R)
            for r, (lo, n) in enumerate(shards):
                _check_sample("%s rank %d" % (what, r), c["dist"][:, lo:lo + n], samples[r][0], samples[r][1], founds[r]["visited"], b)
            need, v = sc.need_of(R, sampled_rows, N, sigma)
            assert sc.need_is_safe(v), (what, v)
            refs = _reference_for(c, shards, founds, S_of, need)
            assert refs[0][2].all(), what
            for r, ctx in enumerate(ctxs):
                fits = _check_records("%s rank %d" % (what, r), c, shards[r], recs[r][0], recs[r][1], refs, r, ctx.get_stat("slice_cap"))
                partial += int(any((keep[r] == 0).any() for _, keep in fits))
            held = bool((sum(rec for rec, _ in recs).sum(0) >= R).all())
            assert held or sigma == 0, what
            gathered = _exchange(ctxs, 1, [ctx.hist_buffer() for ctx in ctxs], False)
            assert [ctx.rank(gathered[r], G, r) for r, ctx in enumerate(ctxs)] == [not held] * G, (what, held)
            routed = _routed_form(ctxs, R)
            for r, ctx in enumerate(ctxs):
                assert routed[r][1] == recs[r][1] == 0, (what, r)
                assert np.array_equal(routed[r][0], recs[r][0]), "%s rank %d, owner-routed against all-gather: %s" % (what, r, _first_diff(routed[r][0], recs[r][0]))
                assert ctx.get_stat("cut_beyond_planes") == 0, (what, r)
        assert partial > 0                        # (some rank, some query: the prefix ended on a lower shard)
    finally:
        for ctx in ctxs:
            ctx.close()


def test_a_cut_beyond_the_exchanged_planes_is_reported_and_takes_every_row():
    """Codes with 15 % of their bits set and one query of all ones: its nearest rows lie beyond b / 2 + 2, the planes the
    owner-routed exchange carries.  The all-gather form reads every plane and finds the query's cut like any other -- the reference's
    record tables, "cut_beyond_planes" = 0.  The owner-routed form finds no cut within its planes: include/hashgan_amd.h documents
    "cut_beyond_planes" = 1 for it, on every rank, and a bet that wider slices cannot win -- the query takes every row up to the last
    plane, which no slice of the budgeted capacity holds ("slice_cap" is less than a segment's rows of it), so the shard's overflow flag
    is raised.  Every other query's records are those of the all-gather form, bit for bit."""
    G, b, N, Q, far, R = 2, 64, 66020, 33, 7, 1000
    c = _bet_case(b, N, Q, 0.15, far)
    assert c["dist"][far].min() > b // 2 + 2
    shards, ctxs, founds = _open_shards(c, G, np.random.default_rng(123))
    try:
        samples, recs = _gathered_form(ctxs, R)
        need, v = sc.need_of(R, sum(int(f["visited"].sum()) for f in founds), N, 5)
        assert sc.need_is_safe(v)
        refs = _reference_for(c, shards, founds, [f["segments"] for f in founds], need)
        assert refs[0][2].all() and refs[0][1][far] > b // 2 + 2 and (np.delete(refs[0][1], far) < b // 2 + 2).all()
        for r, ctx in enumerate(ctxs):
            _check_records("all-gather rank %d" % r, c, shards[r], recs[r][0], recs[r][1], refs, r, ctx.get_stat("slice_cap"))
            assert ctx.get_stat("cut_beyond_planes") == 0
        routed = _routed_form(ctxs, R)
        others = np.arange(Q) != far
        for r, ctx in enumerate(ctxs):
            assert ctx.get_stat("cut_beyond_planes") == 1, r
            lo, n = shards[r]
            assert ctx.get_stat("slice_cap") < min(sc.segment_lengths(n, founds[r]["segments"]))
            assert routed[r][1] != 0, "rank %d: a query that takes every row overflowed no slice" % r
            assert np.array_equal(routed[r][0][:, others], recs[r][0][:, others]), "rank %d: %s" % (r, _first_diff(routed[r][0][:, others], recs[r][0][:, others]))
    finally:
        for ctx in ctxs:
            ctx.close()


# (b, N, Q, options, sampled segments k_guess_direct's dispatch sees: <= 64 -> 4 lanes per query, <= 512 -> 16, more -> 64)
ONESHOT_CASES = [(64, 66017, 33, {"max_segments": 100}, (1, 64)), (32, 66017, 33, {}, (65, 512)),
                 (100, 69989, 33, {"min_segment": 16, "max_segments": 4096}, (513, 1 << 20))]


@pytest.mark.parametrize("b,N,Q,options,sampled_segments", ONESHOT_CASES, ids=["b%d-parts%d" % (c[0], p) for c, p in zip(ONESHOT_CASES, (4, 16, 64))])
def test_one_shot_guess_keeps_the_records_of_the_staged_guess(b, N, Q, options, sampled_segments):
    """k_guess_direct is observable through "records_kept" after hg_map.  hg_seq.hip: enqueue_optimistic samples with the same stride
    and geometry as hg_sample_hist (do_hist), hands the kernel the same rows-visited figure (sampled_rows), sigma = "guess_sigma", the
    same R and n_total, and the kernel derives T and sstar as k_guess does -- but its sampled pass writes, and it reads, only the
    planes below hcap = b / 2 + 2 (the matrix-core kernels).  The crowding probe and `second_bet` change the slices' width, never T.  So
    where the reference's cuts lie below hcap (asserted), "records_kept" of the one-shot step equals the sum of the staged record
    table on the same context, options and data -- which section 2's reference pins.  4, 16 and 64 lanes per query by the number of
    sampled segments.  The AP is the oracle's and the bet holds."""
    c = _bet_case(b, N, Q)
    ctx = _open(**options)
    try:
        _load_db(ctx, c["dbbits"], c["dblab"])
        _load_q(ctx, c["qbits"], c["qlab"])
        for R, sigma in ((50, 5), (1000, 12), (N // 9, 5)):
            what = "b=%d R=%d guess_sigma=%d %s" % (b, R, sigma, options)
            ctx.set_option("guess_sigma", sigma)
            ctx.sample_hist(R)
            table, _, visited_word = _table(ctx)
            need, v = sc.need_of(R, visited_word, N, sigma)
            assert sc.need_is_safe(v)
            T = (np.cumsum(table, axis=0) >= need).argmax(0)
            assert (np.cumsum(table, axis=0)[-1] >= need).all() and (T < b // 2 + 2).all(), what      # every cut below hcap
            ctx.guess(R)
            ctx.select_candidates()
            rec, flag, _ = _table(ctx)
            assert flag == 0 and ctx.get_stat("hist_variant") == 3
            assert (rec.sum(0) >= R).all(), what                           # (these records hold the bet: the one-shot step's first attempt is its last)
            S = ctx.get_stat("segments")
            assert sampled_segments[0] <= -(-S // sc.SAMPLE_RATIO) <= sampled_segments[1], (what, S)
            f0 = tuple(ctx.get_stat(k) for k in ("optimistic_fallbacks", "optimistic_requeried", "optimistic_rebets"))
            ap, rel = ctx.map(R)
            assert ctx.get_stat("last_optimistic") == 1 and ctx.get_stat("segments") == S, what
            assert tuple(ctx.get_stat(k) for k in ("optimistic_fallbacks", "optimistic_requeried", "optimistic_rebets")) == f0, what
            assert ctx.get_stat("records_kept") == int(rec.sum()), (what, ctx.get_stat("records_kept"), int(rec.sum()))
            ap_ref, rel_ref = _bet_oracle(b, N, Q, 0.5, None, R)
            assert np.array_equal(rel, rel_ref) and np.array_equal(ap, ap_ref, equal_nan=True), what
    finally:
        ctx.close()


def test_one_shot_cut_beyond_the_planes_limit_reads_as_a_thin_sample():
    """hcap, from the other side: a query whose nearest rows lie beyond the b / 2 + 2 planes the one-shot sampled pass writes.
    hg_kernels.hpp: "sample too thin (or the cut beyond the planes the pass wrote): take everything" -- its slices overflow, it alone
    loses its bet and is rerun exactly ("optimistic_requeried" + 1, no fallback of the whole call), and every AP is the oracle's."""
    b, N, Q, far, R = 64, 66020, 33, 7, 1000
    c = _bet_case(b, N, Q, 0.15, far)
    ctx = _open()
    try:
        _load_db(ctx, c["dbbits"], c["dblab"])
        _load_q(ctx, c["qbits"], c["qlab"])
        before = ctx.get_stat("optimistic_requeried"), ctx.get_stat("optimistic_fallbacks")
        ap, rel = ctx.map(R)
        assert ctx.get_stat("hist_variant") == 3
        assert (ctx.get_stat("optimistic_requeried") - before[0], ctx.get_stat("optimistic_fallbacks") - before[1]) == (1, 0)
        ap_ref, rel_ref = _bet_oracle(b, N, Q, 0.15, far, R)
        assert np.array_equal(rel, rel_ref) and np.array_equal(ap, ap_ref, equal_nan=True)
    finally:
        ctx.close()

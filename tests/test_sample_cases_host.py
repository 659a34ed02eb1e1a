"""tests/sample_cases.py on the CPU: the probe databases decode ANY set of visited batches, the reference guess agrees with a
brute-force search over the prefixes, and the documented sampling rule meets the coverage conditions the GPU tests impose on what
the kernels visited -- so that tests/test_sample_guess_gpu.py can neither pass vacuously nor fail for a reason of its own."""
import numpy as np
import pytest

from tests import sample_cases as sc


def _sampled_table(qbits, dbbits, b, rows):
    return sc.histogram(sc.distances(qbits, dbbits), b, rows)


# ------------------------------------------------------------------------------------------------------------------ probes
@pytest.mark.parametrize("b,B,N,max_w", [(64, 16, 5984, 64), (64, 16, 5977, 32), (127, 16, 22528, 64), (127, 8, 9001, 69), (31, 16, 5000, 32),
                                          (255, 4, 21003, 129), (200, 4, 3000, 129), (33, 16, 1000, 5), (100, 8, 66003, 32)])
def test_two_level_probe_decodes_an_arbitrary_set_of_batches(b, B, N, max_w):
    """Random subsets of the batches, whole databases probed window by window: the decoded counts are the rows of the chosen batches
    and 0 elsewhere -- among random queries that share the launch, whose columns must not matter."""
    rng = np.random.default_rng(b * 1000 + B)
    m, w = sc.probe_split(b, max_w)
    assert 3 * m + w <= b and 1 <= w <= max_w and m >= 1
    if (b, max_w) in ((64, 64), (127, 64)):
        assert (m + 1) * w == {64: 374, 127: 1408}[b]
    nb = -(-N // B)
    windows = sc.probe_windows(N, B, m, w)
    assert (windows - 1) * (m + 1) * w < nb <= windows * (m + 1) * w
    q = np.concatenate([sc.probe_queries(b, m, w), sc.bits(rng, 3, b)])
    for density in (0.0, 0.04, 0.5, 1.0):
        chosen = rng.random(nb) < density
        rows = np.repeat(chosen, B)[:N]
        counts = np.concatenate([sc.decode(_sampled_table(q, sc.probe_db(b, B, N, m, w, k), b, rows), B, N, m, w, k) for k in range(windows)])
        assert np.array_equal(counts, np.where(chosen, sc.batch_sizes(N, B), 0))
        mask, vb = sc.visited_rows(counts, N, B)
        assert np.array_equal(mask, rows) and np.array_equal(vb, np.nonzero(chosen)[0])


def test_probe_distances_are_what_the_decoding_assumes():
    b, B, N = 64, 16, 5984
    m, w = sc.probe_split(b, 64)
    d = sc.distances(sc.probe_queries(b, m, w), sc.probe_db(b, B, N, m, w))
    k = np.arange(N) // B
    want = 3 * (k // w)[None, :] + np.where((k % w)[None, :] == np.arange(w)[:, None], 0, 2)
    assert np.array_equal(d, want)
    # a second window's rows: the background code, two bits from every probe query
    d2 = sc.distances(sc.probe_queries(b, m, w), sc.probe_db(b, B, 2 * N, m, w, 1))
    assert (d2[:, :N] == 2).all() and np.array_equal(d2[:, N:], want)


@pytest.mark.parametrize("b,B,N", [(1, 16, 32), (1, 16, 20), (31, 16, 512), (12, 4, 50), (200, 4, 804)])
def test_single_probe_decodes_an_arbitrary_set_of_batches(b, B, N):
    rng = np.random.default_rng(b + N)
    db = sc.single_db(rng, b, B, N)
    assert np.array_equal(db.sum(1), np.arange(N) // B)
    nb = -(-N // B)
    for density in (0.0, 0.3, 1.0):
        chosen = rng.random(nb) < density
        table = _sampled_table(np.zeros((1, b), np.uint8), db, b, np.repeat(chosen, B)[:N])
        assert np.array_equal(table[:nb, 0], np.where(chosen, sc.batch_sizes(N, B), 0))


def test_a_batch_counted_partly_or_twice_is_refused():
    N, B = 100, 16
    size = sc.batch_sizes(N, B)
    assert list(size) == [16] * 6 + [4]
    sc.visited_rows(size * (np.arange(7) % 2), N, B)
    for batch, count in ((2, 8), (2, 32), (6, 16), (6, 3)):
        counts = np.zeros(7, np.int64)
        counts[batch] = count
        with pytest.raises(AssertionError):
            sc.visited_rows(counts, N, B)


def test_split_table_reads_the_exported_layout():
    b, Q = 5, 70
    words = np.arange((b + 1) * 128 + sc.TAIL_WORDS, dtype=np.uint32)
    table, flag, visited = sc.split_table(words, b, Q)
    assert table.shape == (6, 70) and table[2, 69] == 2 * 128 + 69 and (flag, visited) == (6 * 128, 6 * 128 + 1)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_the_documented_rule_meets_the_coverage_conditions():
    """Every stride-th batch of each segment, over random geometry: both conditions hold for the vector kernel's whole batches of
    segments two select segments long and for the matrix-core kernels' 16-row tiles, ragged ones included, of the select segments."""
    rng = np.random.default_rng(5)
    for _ in range(400):
        vector_alu = bool(rng.integers(2))
        B = int(rng.choice([16, 8, 4])) if vector_alu else 16
        L = 32 * int(rng.integers(1, 40))
        N = int(rng.integers(1, 30 * L))
        stride = int(rng.choice([2, 3, 5, 24, 100]))
        vb = sc.rule_visited(N, sc.SAMPLE_RATIO * L if vector_alu else L, B, stride, not vector_alu)
        assert np.all(np.diff(vb) > 0)
        nrows = int(sc.batch_sizes(N, B)[vb].sum())
        assert sc.coverage_violations(vb, nrows, N, B, stride, not vector_alu) == [], (vector_alu, B, L, N, stride)


def test_the_coverage_conditions_catch_what_they_are_for():
    N, L, B, stride = 5000, 320, 16, 3
    S = -(-N // L)
    size = sc.batch_sizes(N, B)
    vb = sc.rule_visited(N, L, B, stride, True)
    rows = lambda v: int(size[v].sum())
    assert sc.coverage_violations(vb, rows(vb), N, B, stride, True) == []
    last_segment = vb[vb < (S - 1) * L // B]                               # the pass skips its last segment
    assert sc.coverage_violations(last_segment, rows(last_segment), N, B, stride, True)
    middle = vb[(vb < 5 * L // B) | (vb >= 6 * L // B)]                   # ... or one in the middle
    assert sc.coverage_violations(middle, rows(middle), N, B, stride, True)
    assert sc.coverage_violations(vb[1:], rows(vb[1:]), N, B, stride, True)      # ... or the first batch
    sparse = sc.rule_visited(N, L, B, stride + 1, True)                    # a larger stride than asked for
    assert sc.coverage_violations(sparse, rows(sparse), N, B, stride, True)
    # k_hist's whole batches: only the database's end is ragged, so a pass that loses one batch in every segment comes up short
    N, L, B = 5003, 640, 8
    size = sc.batch_sizes(N, B)
    vb = sc.rule_visited(N, L, B, stride, False)
    assert sc.coverage_violations(vb, rows(vb), N, B, stride, False) == [] and rows(vb) * stride < N + 8 * B * stride
    lossy = np.array([k for i, k in enumerate(vb) if i + 1 == len(vb) or vb[i + 1] // (L // B) == k // (L // B)])
    assert len(lossy) == len(vb) - 7 and sc.coverage_violations(lossy, rows(lossy), N, B, stride, False)


# ------------------------------------------------------------------------------------------------------------------- guess
def test_need_follows_the_documented_formula():
    need, v = sc.need_of(1000, 2752, 66000, 5)
    fr = 1000 * 2752 / 66000
    assert v == fr + 5 * fr ** 0.5 + 1 and need == int(np.ceil(v)) and sc.need_is_safe(v)
    assert sc.need_of(50, 100, 100, 0) == (51, 51.0) and not sc.need_is_safe(51.0)


@pytest.mark.parametrize("G", [1, 2, 3])
def test_reference_guess_agrees_with_a_brute_force_prefix_search(G):
    """Random shards, visited sets and needs -- cuts in the first bucket, ties that span several shards, prefixes that end on a
    segment boundary, needs nobody reaches."""
    rng = np.random.default_rng(40 + G)
    b, Q = 12, 9
    seen_short = seen_thin = seen_lower = 0
    for trial in range(60):
        Ns = [int(rng.integers(40, 700)) for _ in range(G)]
        Ls = [32 * int(rng.integers(1, 4)) for _ in range(G)]
        q = sc.bits(rng, Q, b)
        dbs = [sc.bits(rng, n, b, 0.3 if trial % 2 else 0.5) for n in Ns]
        if trial % 3 == 0:
            dbs = [np.where(rng.random((n, 1)) < 0.5, q[0][None, :], d) for n, d in zip(Ns, dbs)]      # many rows AT distance 0 of query 0
        dists = [sc.distances(q, d) for d in dbs]
        visiteds = [np.repeat(rng.random(-(-n // 4)) < 0.4, 4)[:n] for n in Ns]
        sampled = sum(int(v.sum()) for v in visiteds)
        need = sampled + 1 if trial % 10 == 9 else int(rng.integers(1, sampled + 1))
        segs = [sc.segment_counts(dists[r], visiteds[r], b, Ns[r], Ls[r]) for r in range(G)]
        assert all(len(segs[r]) == -(-Ns[r] // (2 * Ls[r])) for r in range(G))
        T, found, keep = sc.guess(segs, need)
        T2, found2, keep2 = sc.guess_brute_force(dists, visiteds, b, Ns, Ls, need)
        assert np.array_equal(T, T2) and np.array_equal(found, found2) and np.array_equal(keep, keep2), trial
        nseg = np.array([len(s) for s in segs])
        seen_short += int((found & (keep < nseg[:, None]).any(0)).sum())
        seen_thin += int((~found).sum())
        seen_lower += int((found & (keep[-1] == 0)).sum()) if G > 1 else 1
        # the records that guess selects: everything below T, a prefix at T, nothing above; together at least the sample's need
        for r in range(G):
            rec = sc.records(dists[r], b, Ns[r], Ls[r], T, found, keep[r])
            H = sc.histogram(dists[r], b)
            for qq in range(Q):
                t = int(T[qq])
                assert np.array_equal(rec[:t, qq], H[:t, qq]) and 0 <= rec[t, qq] <= H[t, qq] and not rec[t + 1:, qq].any()
                if keep[r, qq] == nseg[r]:
                    assert rec[t, qq] == H[t, qq]
            assert sc.fullest_slice(dists[r], Ns[r], Ls[r], T, found, keep[r]) <= Ls[r]
    assert seen_short and seen_thin and seen_lower


def test_segment_lengths_hold_the_length_the_geometry_took():
    """make_geometry rounds ceil(N / S0) up to 32 or 96 rows and recounts the segments: whatever S0 and the rounding, the length is
    among the candidates for the resulting count, and every candidate gives that count."""
    rng = np.random.default_rng(9)
    for _ in range(300):
        N = int(rng.integers(32, 80000))
        lq = int(rng.choice([32, 96]))
        S0 = int(rng.integers(1, 3000))
        L = max(-(-(-(-N // S0)) // lq) * lq, lq)
        S = -(-N // L)
        cands = sc.segment_lengths(N, S)
        assert L in cands and all(-(-N // c) == S and c % 32 == 0 for c in cands)

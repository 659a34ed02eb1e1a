"""Host side of the tests that pin the bet's first two stages -- the sampled histogram pass (k_hist at a batch stride, k_hist_mx,
k_hist_i8) and the guessed cut (k_guess, k_guess_direct, k_guess_owner / k_guess_finish) -- to a NumPy reference.

The reference never restates a kernel's sampling loop.  What a sampled pass visited is DISCOVERED from the output of a probe
launch: a database whose rows carry the number of their batch in their code, read back through the distances to probe queries
(probe_db / probe_queries / decode).  Everything else -- every other query's column, the rows-visited word, the guess -- is then
held to that set V of visited rows, and V itself to the two coverage conditions that follow from the documented rule
("every stride-th batch of each segment", coverage()).

Pure NumPy; tests/test_sample_cases_host.py proves on the CPU that the probe decodes arbitrary sets, that the reference guess
agrees with a brute-force search over prefixes, and that the documented rule meets the coverage conditions.
tests/test_sample_guess_gpu.py drives the kernels against all of it.
"""
import math

import numpy as np

TAIL_WORDS = 64          # words behind an exported table: [0] overflow flag, [1] rows the pass visited (hg_hist_buffer)
SAMPLE_RATIO = 2         # a segment of the sampled pass is this many select segments long ("segments" counts select segments)
C = 10                   # classes, multi-hot


# ------------------------------------------------------------------------------------------------------------ plain helpers
def bits(rng, n, b, p=0.5):
    return (rng.random((n, b)) < p).astype(np.uint8)


def labels(rng, n):
    return (rng.random((n, C)) < 0.15).astype(np.int8)


def distances(qbits, dbbits):
    """Hamming distances, int64 [Q, N] (|q| + |x| - 2 q.x in float64: exact far beyond any code length here)."""
    q = np.asarray(qbits, np.float64)
    x = np.asarray(dbbits, np.float64)
    return (q.sum(1)[:, None] + x.sum(1)[None, :] - 2.0 * (q @ x.T)).astype(np.int64)


def histogram(dist, b, rows=None):
    """int64 [b + 1, Q]: rows at every distance, per query; `rows`: a boolean mask or an index array over the columns of dist."""
    d = dist if rows is None else dist[:, rows]
    Q = d.shape[0]
    flat = (d + (np.arange(Q, dtype=np.int64) * (b + 1))[:, None]).ravel()
    return np.bincount(flat, minlength=Q * (b + 1)).reshape(Q, b + 1).T


def split_table(words, b, Q):
    """What hg_hist_buffer hands out, uint32 [(b + 1) * Qpad + TAIL_WORDS] -> (int64 [b + 1, Q] of the live queries, overflow flag,
    rows visited)."""
    qpad = (Q + 63) // 64 * 64
    words = np.asarray(words)
    assert words.shape == ((b + 1) * qpad + TAIL_WORDS,), words.shape
    table = words[:(b + 1) * qpad].reshape(b + 1, qpad)[:, :Q].astype(np.int64)
    return table, int(words[(b + 1) * qpad]), int(words[(b + 1) * qpad + 1])


def unit_rows(vector_alu, b):
    """Rows of one batch of the sampled pass: the matrix-core kernels walk tiles of 16 rows; k_hist walks its scalar-load batches --
    16 rows of codes of <= 64 bits, 8 of <= 128, 4 of longer ones (hg_kernels.hpp, Batch)."""
    if not vector_alu:
        return 16
    return 16 if b <= 64 else 8 if b <= 128 else 4


# ------------------------------------------------------------------------------------------------------------------- probes
def probe_split(b, max_w):
    """(m, w): the two-level probe's fields -- a thermometer in steps of 3 bits over 3 m bits and a one-hot over w bits, 3 m + w <= b
    and w <= max_w (one probe query per bit of the right field), with the most batches (m + 1) w per launch.  A database of
    more batches than that is probed window by window, which takes m >= 1 (probe_db's background code); None when no field fits
    (b < 4: the single probe is for those)."""
    best = None
    for m in range(1, b // 3 + 1):
        w = min(b - 3 * m, max_w)
        if w >= 1 and (best is None or (m + 1) * w > (best[0] + 1) * best[1]):
            best = (m, w)
    return best


def probe_windows(N, B, m, w):
    nb = -(-N // B)
    return -(-nb // ((m + 1) * w))


def probe_db(b, B, N, m, w, window=0):
    """The probe database of one window: batch k = row // B of the window's (m + 1) w batches has j1 = k' // w, j2 = k' % w
    (k' its number inside the window), a left field with its first 3 j1 bits set and a right field one-hot(j2).  Rows of other
    windows carry the background code -- bit 0 alone -- which lies at distance 2 from every probe query, where no batch is read."""
    cap = (m + 1) * w
    k = np.arange(N) // B - window * cap
    inwin = (k >= 0) & (k < cap)
    j1 = np.where(inwin, k // w, 0)
    j2 = np.where(inwin, k % w, 0)
    out = np.zeros((N, b), np.uint8)
    out[:, :3 * m] = np.arange(3 * m)[None, :] < 3 * j1[:, None]
    rows = np.nonzero(inwin)[0]
    out[rows, 3 * m + j2[rows]] = 1
    if not inwin.all():
        assert m >= 1
        out[~inwin, 0] = 1
    return out


def probe_queries(b, m, w):
    """Probe query t: left field zero, right field one-hot(t).  Batch (j1, j2) lies at distance 3 j1 from query j2 and at 3 j1 + 2
    from every other probe query, so the count at distance 3 j1 in column t is the number of visited rows of batch (j1, t)."""
    out = np.zeros((w, b), np.uint8)
    out[np.arange(w), 3 * m + np.arange(w)] = 1
    return out


def decode(table, B, N, m, w, window=0):
    """Visited rows per batch of the window, from the probe columns (the first w) of a sampled table: int64 [batches of the
    window], in batch order."""
    cap = (m + 1) * w
    nb = -(-N // B)
    k = np.arange(window * cap, min(nb, (window + 1) * cap)) - window * cap
    return table[3 * (k // w), k % w]


def single_db(rng, b, B, N):
    """Single probe, for databases of at most b + 1 batches: the rows of batch j are random codes of j set bits; the probe query is all
    zeros, so the count at distance j in its column is the number of visited rows of batch j."""
    assert N <= B * (b + 1)
    out = np.zeros((N, b), np.uint8)
    for r in range(N):
        out[r, rng.permutation(b)[:r // B]] = 1
    return out


def batch_sizes(N, B):
    nb = -(-N // B)
    return np.minimum(B, N - np.arange(nb) * B)


def visited_rows(counts, N, B):
    """Batch counts -> (boolean mask [N] of the visited rows, sorted numbers of the visited batches); every count must be 0 or its
    whole batch: no batch partly, none twice."""
    size = batch_sizes(N, B)
    counts = np.asarray(counts)
    assert counts.shape == size.shape
    bad = np.nonzero((counts != 0) & (counts != size))[0]
    if len(bad):
        raise AssertionError("batch %d holds %d rows and %d of them were counted (%d such batches)" % (bad[0], size[bad[0]], counts[bad[0]], len(bad)))
    hit = counts != 0
    return np.repeat(hit, B)[:N], np.nonzero(hit)[0]


# ----------------------------------------------------------------------------------------------------------------- coverage
def coverage(N, B, stride, ragged_counted):
    """The two conditions a visited set must meet to stand for the whole database, from the documented rule -- "every stride-th batch of
    each segment", first batch included ("1 tile of 16 rows in 24" at the default stride) -- and nothing else of the kernels:

      rows:  a visited batch stands for itself and the at most stride - 1 batches after it in its segment, none of them larger than it,
             so |V| stride >= N - (rows of ragged segment ends the pass skips).  The matrix-core kernels count a ragged last tile by
             its rows (ragged_counted) and skip nothing; k_hist skips what is left behind the last whole batch of a segment -- and
             its segments are whole multiples of 64 rows (two select segments of a multiple of 32), which every batch size divides,
             so only the database's own end can be ragged: N mod B rows, once.
      gaps:  batch 0 is visited, consecutive visited batches are at most `stride` apart (inside a segment exactly, across a segment
             boundary the next segment's first batch comes sooner), and the last visited batch is among the last `stride` batches
             (whole ones for k_hist).

    -> (least |V| in rows, batches that count for the last condition)"""
    skipped = 0 if ragged_counted else N % B
    least = -(-(N - skipped) // stride)
    return least, (-(-N // B) if ragged_counted else N // B)


def coverage_violations(vbatches, nrows, N, B, stride, ragged_counted):
    """The conditions of coverage() on the sorted visited batch numbers and |V| in rows -> list of what fails (empty: covered)."""
    least, nb = coverage(N, B, stride, ragged_counted)
    out = []
    if nrows < least:
        out.append("|V| = %d rows, the rule visits at least %d of N = %d at stride %d" % (nrows, least, N, stride))
    if nb == 0:
        return out
    if len(vbatches) == 0 or vbatches[0] != 0:
        out.append("batch 0 is not visited")
        return out
    gaps = np.diff(vbatches)
    if len(gaps) and gaps.max() > stride:
        i = int(gaps.argmax())
        out.append("no batch visited between %d and %d (stride %d)" % (vbatches[i], vbatches[i + 1], stride))
    if vbatches[-1] < nb - stride:
        out.append("last visited batch %d of %d (stride %d)" % (vbatches[-1], nb, stride))
    return out


def rule_visited(N, L, B, stride, ragged_counted):
    """The documented rule itself, for the host test that shows it meets coverage() -- never the reference of a GPU test: every
    stride-th batch of each segment of L rows, from the segment's first; a ragged last batch only where ragged_counted."""
    out = []
    for lo in range(0, N, L):
        hi = min(lo + L, N)
        nb = -(-(hi - lo) // B) if ragged_counted else (hi - lo) // B
        out.extend(lo // B + t for t in range(0, nb, stride))
    return np.asarray(out, np.int64)


# -------------------------------------------------------------------------------------------------------------------- guess
def need_of(R, sampled, n_total, sigma):
    """The sample count the cut must reach (hg_kernels.hpp above k_guess): f = sampled rows / n_total, need = ceil(f R +
    sigma sqrt(f R) + 1), in float64 -> (need, the value before the ceiling)."""
    fr = float(R) * float(sampled) / float(n_total)
    v = fr + float(sigma) * math.sqrt(fr) + 1.0
    return int(math.ceil(v)), v


def need_is_safe(v):
    """Not within 1e-9 of an integer: the ceiling cannot depend on how the last bit of the float64 arithmetic falls."""
    return abs(v - round(v)) > 1e-9


def segment_lengths(N, S):
    """Every select-segment length L consistent with "segments" = S: multiples of 32 (make_geometry rounds to 32 or 96 rows) with
    ceil(N / L) = S.  The stat does not say which of them the geometry took; a test that needs L tries each and asks that ONE
    of them explains every query."""
    lo = max(32, -(-N // S) // 32 * 32)
    return [L for L in range(lo, N + 64, 32) if -(-N // L) == S]


def segment_counts(dist, visited, b, N, L):
    """int64 [Sh, b + 1, Q]: the sample counts of every segment of the sampled pass (SAMPLE_RATIO select segments of L rows)."""
    LL = SAMPLE_RATIO * L
    return np.stack([histogram(dist[:, lo:lo + LL], b, visited[lo:lo + LL]) for lo in range(0, N, LL)])


def guess(seg_counts, need):
    """The documented rule on the shards' per-segment sample counts (list over the shards in rank order of int64 [Sh_r, b + 1, Q]):
    T [Q] = the smallest distance whose cumulative sample count over all shards reaches need, b where none does (found [Q] False);
    keep [G, Q] = how many of shard r's sampled segments, in order, still collect rows AT distance T -- the smallest prefix of
    (shard 0's segments, shard 1's, ...) whose sample count of {dist < T} + {dist = T inside the prefix} reaches need.  Shards
    before the one where the prefix ends keep all their segments, shards after it none; not found: all of every shard.
    Integer arithmetic throughout."""
    G = len(seg_counts)
    nb, Q = seg_counts[0].shape[1:]
    total = sum(s.sum(0) for s in seg_counts)                      # [b + 1, Q]
    cum = np.cumsum(total, axis=0)
    T = np.full(Q, nb - 1, np.int64)
    found = np.zeros(Q, bool)
    keep = np.zeros((G, Q), np.int64)
    for q in range(Q):
        reach = np.nonzero(cum[:, q] >= need)[0]
        if len(reach) == 0:
            keep[:, q] = [len(s) for s in seg_counts]
            continue
        t = int(reach[0])
        T[q], found[q] = t, True
        have = int(cum[t - 1, q]) if t else 0
        done = False
        for r in range(G):
            if done or have >= need:
                done = True
                continue                                           # keep[r, q] = 0: the prefix ended on a lower shard
            run = have + np.cumsum(seg_counts[r][:, t, q])
            hit = np.nonzero(run >= need)[0]
            keep[r, q] = int(hit[0]) + 1 if len(hit) else len(seg_counts[r])
            have = int(run[-1])
    return T, found, keep


def guess_brute_force(dists, visiteds, b, Ns, Ls, need):
    """The same answer by searching the prefixes one after the other on the rows themselves: for every query the smallest T, then the
    shortest prefix in whole sampled segments, counted afresh each time.  -> (T, found, keep) like guess()."""
    G, Q = len(dists), dists[0].shape[0]
    T = np.full(Q, b, np.int64)
    found = np.zeros(Q, bool)
    keep = np.zeros((G, Q), np.int64)
    nseg = [-(-Ns[r] // (SAMPLE_RATIO * Ls[r])) for r in range(G)]
    for q in range(Q):
        sample = [dists[r][q][visiteds[r]] for r in range(G)]
        for t in range(b + 1):
            if sum(int((s <= t).sum()) for s in sample) >= need:
                T[q], found[q] = t, True
                break
        if not found[q]:
            keep[:, q] = nseg
            continue
        t = int(T[q])
        below = sum(int((s < t).sum()) for s in sample)
        prefixes = [(r, k) for r in range(G) for k in range(nseg[r] + 1)]       # shards < r whole, k segments of shard r
        for r, k in prefixes:
            n = below
            for r2 in range(r):
                n += int((sample[r2] == t).sum())
            end = min(k * SAMPLE_RATIO * Ls[r], Ns[r])
            n += int(((dists[r][q][:end] == t) & visiteds[r][:end]).sum())
            if n >= need:
                keep[:r, q] = nseg[:r]
                keep[r, q] = k
                break
        else:
            raise AssertionError("no prefix reaches need although the cut was found")
    return T, found, keep


def records(dist, b, N, L, T, found, keep_r):
    """The record table of one shard after the select pass with that guess, int64 [b + 1, Q]: every row closer than T, the rows at T
    inside the first keep_r[q] sampled segments (all rows where no cut was found), nothing beyond T."""
    H = histogram(dist, b)
    out = np.zeros_like(H)
    for q in range(dist.shape[0]):
        t = int(T[q])
        out[:t, q] = H[:t, q]
        end = N if not found[q] else min(int(keep_r[q]) * SAMPLE_RATIO * L, N)
        out[t, q] = int((dist[q, :end] == t).sum())
    return out


def fullest_slice(dist, N, L, T, found, keep_r):
    """The most records any (select segment, query) slice receives with that guess -- to be held against "slice_cap"."""
    worst = 0
    for q in range(dist.shape[0]):
        t = int(T[q])
        end = N if not found[q] else min(int(keep_r[q]) * SAMPLE_RATIO * L, N)
        sel = dist[q] < t
        sel[:end] |= dist[q, :end] == t
        pad = -(-N // L) * L - N
        worst = max(worst, int(np.concatenate([sel, np.zeros(pad, bool)]).reshape(-1, L).sum(1).max()))
    return worst

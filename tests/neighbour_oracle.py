"""NumPy statement of label-free relevance (hg_set_neighbours, hg_match_neighbours, hg_nbr_hist): the ground truth of query q is a set
NB(q) of database rows; slot k of its ranked list matches iff idx[q][k] is in NB(q); AP is oracle.hamming_map's on those bits; the
neighbour histogram counts NB(q) per Hamming distance.  The ranked lists themselves come from oracle.hamming_map / oracle.real_map."""
import numpy as np

from oracle import hamming_map as H

PAD = 0xFFFFFFFF


def members(row):
    """The ids of one row of a [Q][G] table, pads dropped."""
    row = np.asarray(row, dtype=np.int64)
    return row[row != PAD]


def sorted_table(gt):
    """-> (uint32 [Q][G] ascending with the pads at the end, uint32 [Q] valid ids): what hg_get_neighbours returns."""
    gt = np.asarray(gt, dtype=np.uint32)
    return np.sort(gt, axis=1), (gt != PAD).sum(1).astype(np.uint32)


def match_bits(idx, gt):
    """-> uint8 [Q][R]: np.isin(idx[q], NB(q))."""
    idx = np.asarray(idx, dtype=np.int64)
    return np.stack([np.isin(idx[q], members(gt[q])) for q in range(idx.shape[0])]).astype(np.uint8)


def ap_rows(match, k=None):
    """-> (ap float64 [Q], NaN where the top k hold no hit; rel int64 [Q]) of the first k slots (all of them by default)."""
    match = np.asarray(match)[:, :k].astype(bool)
    ap = np.full(match.shape[0], np.nan)
    rel = np.zeros(match.shape[0], np.int64)
    for q in range(match.shape[0]):
        a, r = H.average_precision(match[q], match.shape[1])
        rel[q] = r
        if a is not None:
            ap[q] = a
    return ap, rel


def ap_at(match, ks):
    """-> (ap [Q][nk], hits [Q][nk]) at every cut-off."""
    cols = [ap_rows(match, int(k)) for k in ks]
    return np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)


def bitmap_words(match):
    """-> uint64 [Q][ceil(R/64)]: bit k % 64 of word k // 64 is slot k, the bits past R zero (the raw match buffer)."""
    match = np.asarray(match, dtype=np.uint8)
    Q, R = match.shape
    RW = (R + 63) // 64
    padded = np.zeros((Q, RW * 64), np.uint8)
    padded[:, :R] = match
    return np.packbits(padded.reshape(Q, RW, 64), axis=2, bitorder="little").reshape(Q, RW, 8).copy().view(np.uint64).reshape(Q, RW)


def nbr_hist(qbits, dbbits, gt):
    """-> uint32 [b+1][Q]: nbr[d][q] = the neighbours of q at Hamming distance d (bincount of xor-popcount distances)."""
    qw, dw = H.pack_bits(qbits), H.pack_bits(dbbits)
    b = qbits.shape[1]
    out = np.zeros((b + 1, qw.shape[0]), np.uint32)
    for q in range(qw.shape[0]):
        ids = members(gt[q])
        d = H.hamming_matrix(qw[q:q + 1], dw[ids])[0]
        out[:, q] = np.bincount(d, minlength=b + 1)
    return out


def random_sets(rng, idx, N, G, empty=(), outside=()):
    """Ragged ground truth for the lists idx [Q][R]: per query n_q in 0..G ids, about half of them drawn from its own list (so the
    ranking has hits), the rest from anywhere, in random order with the pads in between.  Queries in `empty` get no id; queries in
    `outside` only ids that are not on their list.  -> uint32 [Q][G]"""
    idx = np.asarray(idx, dtype=np.int64)
    Q, R = idx.shape
    gt = np.full((Q, G), PAD, dtype=np.uint32)
    for q in range(Q):
        if q in empty:
            continue
        n = int(rng.integers(1, G + 1))
        rest = np.setdiff1d(np.arange(N), idx[q])
        if q in outside:
            ids = rng.choice(rest, size=min(n, rest.size), replace=False)
        else:
            a = rng.choice(idx[q], size=min((n + 1) // 2, R), replace=False)
            ids = np.concatenate([a, rng.choice(rest, size=min(n - a.size, rest.size), replace=False)])
        gt[q, rng.permutation(G)[:ids.size]] = ids
    return gt

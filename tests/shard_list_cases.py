"""Inputs and a NumPy model of the two list exchange units of a database-sharded context (hashgan_amd/csrc/hg_list_merge.hpp):
tests/test_shard_lists_host.py checks the model and the shapes' properties, tests/test_shard_lists_gpu.py reads the device blocks back
against it.

The shapes are tests/shard_side_cases.py's four (Q = 70, N = 1031, Qpad = 128) and one of this file's: b64_c200_multihot, 200 classes in
four label words -- the match bits then come from k_match through the lists, and k_votes / k_list_grades walk every label word -- with
one to six labels per row, a query without labels and a query that shares up to 9 labels with a row.

The ranking is the canonical one: Hamming distance ascending, database index ascending.  Shard r of G owns the rows
shard_bounds(N, G)[r]; slot i of query q belongs to the shard that owns the row ranked i-th.
"""
import functools

import numpy as np
from tests import shard_side_cases as S

Q, N, QPAD = S.Q, S.N, 128
GS = S.GS
KS_LONG = (1, 7, 256, 257, 500, N)       # a chunk boundary of the list walk on and next to a cut-off; the last one gives R = N
KS_SHORT = (1, 7)                        # R = 7: many shards own nothing
OWN = "b64_c200_multihot"
SHAPES = dict(S.SHAPES)
SHAPES[OWN] = (64, 200, True)
NO_LABEL_QUERY, HEAVY_QUERY, HEAVY_LABELS = 5, 7, 9


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (qb, db uint8 {0,1} codes, ql, dl int8 {0,1} labels), read-only."""
    if name != OWN:
        return S.make(name)
    b, C, _ = SHAPES[name]
    rng = np.random.default_rng(64200)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl, ql = np.zeros((N, C), dtype=np.int8), np.zeros((Q, C), dtype=np.int8)
    for lab, n in ((dl, N), (ql, Q)):
        for i in range(n):
            lab[i, rng.choice(C, int(rng.integers(1, 7)), replace=False)] = 1
    ql[NO_LABEL_QUERY] = 0
    heavy = rng.choice(C, 12, replace=False)
    ql[HEAVY_QUERY] = 0
    ql[HEAVY_QUERY, heavy] = 1
    dl[N // 2] = 0
    dl[N // 2, heavy[:HEAVY_LABELS]] = 1
    dl[0, C - 1] = 1                                     # the last class of the last label word is in use
    ql[0, C - 1] = 1
    out = (qb, db, ql, dl)
    for a in out:
        a.flags.writeable = False
    return out


def rp_of(R):
    return (R + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def ranking(name):
    """-> (idx int64 [Q, N], dist int64 [Q, N]): every query's whole database in the canonical order."""
    qb, db, _, _ = make(name)
    d = (qb[:, None, :] != db[None, :, :]).sum(2)
    idx = np.argsort(d, axis=1, kind="stable")
    return idx, np.take_along_axis(d, idx, axis=1)


@functools.lru_cache(maxsize=None)
def grades(name):
    """-> uint8 [Q, N]: the labels query q shares with the row ranked i-th."""
    _, _, ql, dl = make(name)
    g = ql.astype(np.int64) @ dl.astype(np.int64).T
    return np.take_along_axis(g, ranking(name)[0], axis=1).astype(np.uint8)


def owner_mask(name, G, r, R):
    """-> bool [Q, R]: slot i of query q is shard r's."""
    lo, n = S.shard_bounds(N, G)[r]
    idx = ranking(name)[0][:, :R]
    return (idx >= lo) & (idx < lo + n)


def grade_plane(name, G, r, R):
    """Shard r's grade plane -> (uint8 [Q, Rp], own uint32 [QPAD])."""
    mine = owner_mask(name, G, r, R)
    plane = np.zeros((Q, rp_of(R)), dtype=np.uint8)
    plane[:, :R] = np.where(mine, grades(name)[:, :R], 0)
    own = np.zeros(QPAD, dtype=np.uint32)
    own[:Q] = mine.sum(1)
    return plane, own


def grade_block(name, G, r, R):
    """... as the bytes of the exchange block."""
    plane, own = grade_plane(name, G, r, R)
    return np.concatenate([plane.ravel(), own.view(np.uint8)])


def vote_table(name, G, r, ks):
    """Shard r's vote table -> uint32 [nk, C + 1, QPAD]."""
    _, _, _, dl = make(name)
    C = dl.shape[1]
    R = int(ks[-1])
    mine = owner_mask(name, G, r, R)
    lab = dl[ranking(name)[0][:, :R]].astype(np.int64) * mine[:, :, None]           # [Q, R, C]
    cum = np.concatenate([np.zeros((Q, 1, C), np.int64), np.cumsum(lab, axis=1)], axis=1)
    cown = np.concatenate([np.zeros((Q, 1), np.int64), np.cumsum(mine, axis=1)], axis=1)
    tab = np.zeros((len(ks), C + 1, QPAD), dtype=np.uint32)
    for j, k in enumerate(ks):
        tab[j, :C, :Q] = cum[:, k, :].T
        tab[j, C, :Q] = cown[:, k]
    return tab


def merge_grades(blocks):
    """[(plane, own)] -> (plane, own) of the whole database: a slot is non-zero in at most one block."""
    plane = np.zeros_like(blocks[0][0])
    for p, _ in blocks:
        assert not ((plane != 0) & (p != 0)).any()
        plane |= p
    return plane, np.sum([o.astype(np.int64) for _, o in blocks], axis=0)


def merge_votes(tabs):
    return np.sum([t.astype(np.int64) for t in tabs], axis=0)

"""Inputs and brute-force tables for the side metrics of a database-sharded context (tests/test_shard_side_host.py checks the
generators' properties with NumPy, tests/test_shard_side_gpu.py runs them on virtual shards).

Q = 70 gives Qpad = 128: one full 64-query unit and one partly filled, with pad columns.  N = 1031 is prime: uneven shards for every
G > 1 (128 or 129 rows at G = 8).  The multi-hot case carries at most 4 labels on every database row but the LAST one, which carries
11 of the 12 labels of query 7: the whole database has 12 grades -- (b + 1) * 12 > 640, a banded joint pass -- and so has the last
shard, while every other shard has 5 and its joint block is zero-padded in g.
"""
import functools

import numpy as np

Q, N = 70, 1031
GS = (1, 2, 3, 8)
CUTOFFS = (1, 7, 500, N)
CELLS = 640                                              # (distance, grade) cells of a wavefront's column that fit the LDS
SHAPES = {"b8_c10": (8, 10, False), "b64_c10": (64, 10, False), "b100_c10": (100, 10, False), "b64_c81_multihot": (64, 81, True)}
HEAVY_QUERY, HEAVY_QUERY_LABELS, HEAVY_ROW_LABELS, ROW_LABELS_MAX = 7, 12, 11, 4


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (qb, db uint8 {0,1} codes, ql, dl int8 {0,1} labels), read-only."""
    b, C, multihot = SHAPES[name]
    rng = np.random.default_rng(1000 * b + C)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl, ql = np.zeros((N, C), dtype=np.int8), np.zeros((Q, C), dtype=np.int8)
    if multihot:
        for lab, n in ((dl, N), (ql, Q)):
            for i in range(n):
                lab[i, rng.choice(C, int(rng.integers(1, ROW_LABELS_MAX + 1)), replace=False)] = 1
        ql[5] = 0                                        # a query without labels
        heavy = rng.choice(C, HEAVY_QUERY_LABELS, replace=False)
        ql[HEAVY_QUERY] = 0
        ql[HEAVY_QUERY, heavy] = 1
        dl[N - 1] = 0
        dl[N - 1, heavy[:HEAVY_ROW_LABELS]] = 1          # the one row with the most labels: in the last shard for every G
    else:
        dl[np.arange(N), rng.integers(0, C, N)] = 1
        ql[np.arange(Q), rng.integers(0, C, Q)] = 1
    out = (qb, db, ql, dl)
    for a in out:
        a.flags.writeable = False
    return out


def shard_bounds(n_total, world):
    """hashgan_amd.sharded.shard_bounds, restated so that the host test needs nothing but NumPy."""
    per, extra = divmod(int(n_total), int(world))
    out, base = [], 0
    for r in range(world):
        rows = per + (1 if r < extra else 0)
        out.append((base, rows))
        base += rows
    return out


def defined_G(ql, dl):
    return 1 + int(min(ql.sum(1).max(), dl.sum(1).max()))


def bands(b, G):
    return 1 if (b + 1) * G <= CELLS else -(-(b + 1) // (CELLS // G))


def _pairs(qb, db, ql, dl):
    d = (qb[:, None, :] != db[None, :, :]).sum(2)
    g = ql.astype(np.int64) @ dl.astype(np.int64).T
    return d, g


def brute_rel(qb, db, ql, dl):
    """(all, rel) uint32 [b + 1, Q] by the definition."""
    d, g = _pairs(qb, db, ql, dl)
    cols = np.broadcast_to(np.arange(len(qb))[:, None], d.shape)
    all_ = np.zeros((qb.shape[1] + 1, len(qb)), dtype=np.uint32)
    rel = np.zeros_like(all_)
    np.add.at(all_, (d, cols), 1)
    np.add.at(rel, (d[g > 0], cols[g > 0]), 1)
    return all_, rel


def brute_grade(qb, db, ql, dl):
    """uint32 [C + 1, Q] by the definition."""
    _, g = _pairs(qb, db, ql, dl)
    H = np.zeros((ql.shape[1] + 1, len(qb)), dtype=np.uint32)
    np.add.at(H, (g, np.broadcast_to(np.arange(len(qb))[:, None], g.shape)), 1)
    return H


def brute_joint(qb, db, ql, dl, G):
    """uint32 [b + 1, G, Q] by the definition; a grade beyond G - 1 would raise."""
    d, g = _pairs(qb, db, ql, dl)
    J = np.zeros((qb.shape[1] + 1, G, len(qb)), dtype=np.uint32)
    np.add.at(J, (d, g, np.arange(len(qb))[:, None]), 1)
    return J


def pad_grades(J, Gc):
    """[b + 1, Gs, Q] -> [b + 1, Gc, Q] with zero planes for the grades Gs .. Gc - 1: the joint block of the exchange."""
    return np.pad(J, ((0, 0), (0, Gc - J.shape[1]), (0, 0)))

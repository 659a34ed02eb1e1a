"""NumPy statement of the re-ranked Hamming ranking (hg_topr_rerank): row n against query q has d = the Hamming distance of the sign
bits (bit = feature > 0) and s = oracle.real_map.inner_products' float32 inner product of the features; rows are ranked by
(d ascending, s descending, database index ascending) and the top R kept.  Match and AP are oracle.hamming_map's."""
import numpy as np

from oracle import hamming_map as H
from oracle import real_map as RM


def generate(Q, N, b, C, seed, multi_hot=False):
    """Features tanh(prototype[label] + 0.9 normal) with a few duplicated database rows -> (qf, dbf float32; ql, dl int64 {0,1})."""
    rng = np.random.default_rng(seed)
    proto = rng.normal(size=(C, b))
    dcls, qcls = rng.integers(0, C, N), rng.integers(0, C, Q)
    dbf = np.tanh(proto[dcls] + 0.9 * rng.normal(size=(N, b))).astype(np.float32)
    qf = np.tanh(proto[qcls] + 0.9 * rng.normal(size=(Q, b))).astype(np.float32)
    dl = np.zeros((N, C), np.int64)
    ql = np.zeros((Q, C), np.int64)
    dl[np.arange(N), dcls] = 1
    ql[np.arange(Q), qcls] = 1
    if multi_hot:
        dl |= (rng.random((N, C)) < 0.03).astype(np.int64)
        ql |= (rng.random((Q, C)) < 0.03).astype(np.int64)
    dbf[5::97] = dbf[4::97]                               # equal (d, s) against every query: the index decides
    return qf, dbf, ql, dl


def distances(qf, dbf):
    """int64 [Q, N]: Hamming distances of the sign bits."""
    return H.hamming_matrix(H.pack_bits(qf > 0), H.pack_bits(dbf > 0))


def rerank(qf, dbf, ql, dl, R):
    """-> dict idx int64 [Q, R], dist int64 [Q, R], score float32 [Q, R], match bool [Q, R], ap float64 [Q] (NaN: no hit), rel int64 [Q],
    and d [Q, N], s [Q, N] of all pairs."""
    d = distances(qf, dbf)
    s = RM.inner_products(qf, dbf)
    Q, N = d.shape
    idx = np.empty((Q, R), np.int64)
    match = np.empty((Q, R), bool)
    ap = np.full(Q, np.nan)
    rel = np.zeros(Q, np.int64)
    ar = np.arange(N)
    for q in range(Q):
        idx[q] = np.lexsort((ar, -s[q], d[q]))[:R]
        match[q] = H.label_match(ql[q, :], dl[idx[q], :])
        a, r = H.average_precision(match[q], R)
        rel[q] = r
        if a is not None:
            ap[q] = a
    rows = np.arange(Q)[:, None]
    return dict(idx=idx, dist=d[rows, idx], score=s[rows, idx], match=match, ap=ap, rel=rel, d=d, s=s)


def mean_ap(ap):
    return H.mean_ap(ap[~np.isnan(ap)])

"""Product quantisation on the host (hashgan_amd/pq.py) and the argument checks of MAPs(quantised=True): no GPU."""
import types
import warnings

import numpy as np
import pytest

from oracle import real_map as RM
from hashgan_amd import MAPs, metric, pq


def tables(N=300, M=3, K=5, dsub=4, seed=0):
    rng = np.random.default_rng(seed)
    books = np.tanh(rng.standard_normal((M, K, dsub))).astype(np.float32)
    codes = rng.integers(0, K, (N, M)).astype(np.uint8)
    return codes, books


def test_decode_is_the_gather_and_moves_bits_untouched():
    codes, books = tables()
    books[0, 1, 2] = 0.0
    books[1, 0, 0] = -0.0
    books[2, 3, 1] = np.float32(1e-42)                  # a subnormal
    books[2, 4, 3] = -np.float32(3e-45)
    x = pq.decode(codes, books)
    assert x.dtype == np.float32 and x.shape == (300, 12) and x.flags.c_contiguous
    M, K, dsub = books.shape
    want = np.empty_like(x)
    for n in range(x.shape[0]):
        for k in range(x.shape[1]):
            want[n, k] = books[k // dsub, codes[n, k // dsub], k % dsub]
    assert np.array_equal(x.view(np.uint32), want.view(np.uint32))
    assert (x.view(np.uint32) == 0x80000000).any() and (x.view(np.uint32) == np.float32(1e-42).view(np.uint32)).any()


def test_encode_takes_the_lowest_index_on_ties_and_inverts_decode_on_codewords():
    codes, books = tables(K=7)
    books[1, 5] = books[1, 2]                           # two equal codewords: index 2 wins
    books[2, 0] = [0.5, 0.0, 0.0, 0.0]
    books[2, 1] = [-0.5, 0.0, 0.0, 0.0]                 # the origin is equally far from 0 and 1: index 0 wins
    x = pq.decode(codes, books)
    got = pq.encode(x, books)
    assert got.dtype == np.uint8 and got.shape == codes.shape
    assert np.array_equal(pq.decode(got, books).view(np.uint32), x.view(np.uint32))
    assert not (got[:, 1] == 5).any() and (got[:, 1] == 2).sum() == ((codes[:, 1] == 2) | (codes[:, 1] == 5)).sum()
    far = books.copy()
    far[2, 2:] = 9.0                                    # out of the way
    origin = np.zeros((1, 12), np.float32)
    assert pq.encode(origin, far)[0, 2] == 0
    assert np.array_equal(pq.encode(x.astype(np.float64), books), got)


def test_sign_codes_are_the_packed_signs_of_the_decoded_table():
    for M, K, dsub in ((3, 5, 4), (8, 256, 8), (3, 16, 11), (5, 9, 51), (1, 2, 1), (16, 64, 8)):
        codes, books = tables(200, M, K, dsub, seed=M)
        books[0, 0, 0] = 0.0
        books[-1, -1, -1] = -0.0
        assert np.array_equal(pq.sign_codes(codes, books), metric.pack_codes(pq.decode(codes, books) > 0)), (M, K, dsub)


def test_argument_errors():
    codes, books = tables()
    for bad in (books.astype(np.float64), books[0], np.zeros((1, 257, 1), np.float32), np.zeros((16, 2, 16), np.float32),
                np.zeros((0, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            pq.decode(codes[:, :bad.shape[0]] if bad.ndim == 3 else codes, bad)
    for bad in (codes.astype(np.int32), codes[:, :2], codes[0], np.full_like(codes, 5)):
        with pytest.raises(ValueError):
            pq.decode(bad, books)
        with pytest.raises(ValueError):
            pq.sign_codes(bad, books)
    nan = books.copy()
    nan[1, 1, 1] = np.nan
    inf = books.copy()
    inf[0, 0, 0] = -np.inf
    for bad in (nan, inf):
        with pytest.raises(ValueError):
            pq.decode(codes, bad)
        with pytest.raises(ValueError):
            pq.encode(np.zeros((2, 12), np.float32), bad)
    with pytest.raises(ValueError):
        pq.encode(np.zeros((2, 11), np.float32), books)
    with pytest.raises(ValueError):
        pq.encode(np.zeros((2, 12), np.int32), books)
    with pytest.raises(ValueError):
        pq.encode(np.zeros(12, np.float32), books)


def test_maps_quantised_refuses_conflicting_modes_and_misfit_databases():
    for kw in (dict(binarize=True), dict(rerank=True), dict(asymmetric=True)):
        with pytest.raises(ValueError, match="quantised"):
            MAPs(10, quantised=True, **kw)
    m = MAPs(10, quantised=True)
    assert m._mode() == "quantised" and m.quantised
    codes, books = tables()
    lab = np.zeros((300, 2), np.int64)
    q = types.SimpleNamespace(output=np.zeros((4, 12), np.float32), label=np.zeros((4, 2), np.int64))
    # refused before any GPU use: wrong dtypes and shapes of the tables, a query of another width, R beyond N
    with pytest.raises(ValueError):
        m.rank_into(types.SimpleNamespace(codes=codes.astype(np.int64), codebooks=books, label=lab), q, idx=object())
    with pytest.raises(ValueError):
        m.rank_into(types.SimpleNamespace(codes=codes, codebooks=books[:2], label=lab), q, idx=object())
    with pytest.raises(ValueError, match="same b"):
        m.get_maps_at(types.SimpleNamespace(codes=codes, codebooks=books, label=lab),
                      types.SimpleNamespace(output=np.zeros((4, 13), np.float32), label=q.label), [1, 2])
    with pytest.raises(ValueError, match="1..N"):
        m.get_maps_at(types.SimpleNamespace(codes=codes, codebooks=books, label=lab), q, [1, 301])
    with pytest.raises(ValueError, match="resident"):
        m.get_maps_at(None, types.SimpleNamespace(codes=codes[:4], label=q.label), [1, 2])      # SQD with nothing to decode with
    assert MAPs(10)._mode() == "reference" and not MAPs(10).quantised


def test_the_oracle_orders_exact_ties_of_a_decoded_table_by_index():
    """K = 4, M = 2: 16 distinct rows, so every score is shared by whole groups of rows -- the yardstick for the GPU test's tie shape."""
    rng = np.random.default_rng(5)
    N, Q, R = 4000, 6, 700
    books = np.tanh(rng.standard_normal((2, 4, 6))).astype(np.float32)
    codes = rng.integers(0, 4, (N, 2)).astype(np.uint8)
    x = pq.decode(codes, books)
    assert len(np.unique(x, axis=0)) == 16
    qf = np.tanh(rng.standard_normal((Q, 12))).astype(np.float32)
    ql = (rng.random((Q, 4)) < 0.3).astype(np.int8)
    dl = (rng.random((N, 4)) < 0.3).astype(np.int8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, idx, score = RM.map_from_features(qf, x, ql, dl, R)
    assert idx.shape == (Q, R) and score.shape == (Q, R)
    bits = score.view(np.uint32)
    assert (score[:, :-1] >= score[:, 1:]).all()
    same = bits[:, :-1] == bits[:, 1:]
    assert same.mean() > 0.9                                          # long groups of equal scores
    assert (idx[:, 1:][same].astype(np.int64) > idx[:, :-1][same].astype(np.int64)).all(), "ties not in index order"
    # the group at the cut is taken from its lowest indices: of the rows with that score, the first ones by index and no others
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, full_idx, full_score = RM.map_from_features(qf[:1], x, ql[:1], dl, N)
    cut = bits[0, -1]
    group = full_idx[0][full_score[0].view(np.uint32) == cut]
    taken = idx[0][bits[0] == cut]
    assert len(group) > len(taken) > 0 and np.array_equal(taken, np.sort(group)[:len(taken)])

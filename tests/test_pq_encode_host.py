"""The PQ encoder without a GPU: the brute-force oracle (tests/pq_encode_oracle.py) against pq.encode, the tie-case generator's own
conditions, and the argument errors of pq.encode_gpu and MAPs(quantise_queries=True), which come before any GPU use."""
import types

import numpy as np
import pytest

from tests import pq_encode_oracle as O
from hashgan_amd import MAPs, pq

# the issue's five shapes, N scaled down: (N, M, dsub, K)
HOST_SHAPES = [(3000, 8, 8, 256), (2500, 3, 11, 16), (3000, 2, 6, 4), (2000, 1, 1, 2), (600, 5, 51, 256)]


@pytest.mark.parametrize("N,M,dsub,K", HOST_SHAPES)
def test_oracle_equals_pq_encode(N, M, dsub, K):
    rng = np.random.default_rng(N + K)
    x = np.tanh(rng.standard_normal((N, M * dsub))).astype(np.float32)
    books = np.stack([x[rng.choice(N, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)])
    books[:, K - 1] = books[:, 0]                                            # a duplicated codeword: the lowest index wins
    codes, err = O.encode(x, books)
    assert np.array_equal(codes, pq.encode(x, books))
    assert not (codes == K - 1).any() and (codes == 0).any()
    d = (x.astype(np.float64) - pq.decode(codes, books).astype(np.float64)) ** 2
    assert np.allclose(err, d.sum(1), rtol=1e-12, atol=0)                    # (another summation order: not bit for bit)


def test_shared_cases_are_what_they_claim():
    for shape in O.SHAPES:
        assert shape[0] % 64 != 0
    c = O.case(*O.DUPLICATED)
    assert np.array_equal(c.books[:, 2:], c.books[:, :2]) and c.codes.max() <= 1       # K = 4 holds 2 distinct: the lower copy wins
    assert min((c.codes == 0).sum(), (c.codes == 1).sum()) > 1000
    assert np.array_equal(c.codes, pq.encode(c.x, c.books))


def test_tie_generator_self_check():
    t = O.tie_case()
    assert t.pairs == 400 and t.x.shape == (4, 200) and t.books.shape == (4, 100, 2, 2)
    assert t.fused_wrong >= 10                       # a condition on the case: enough pairs that a fused chain would get wrong
    for r in range(t.rows):                          # unfused: exact ties everywhere, the lower index
        codes, _ = O.encode(t.x[r:r + 1], t.books[r])
        assert not codes.any()
        assert not pq.encode(t.x[r:r + 1], t.books[r]).any()


def test_non_finite_rows_in_the_oracle():
    c = O.case(1001, 1, 1, 2)
    x = c.x.copy()
    x[3, 0], x[5, 0], x[7, 0] = np.nan, np.inf, -np.inf
    codes, err = O.encode(x, c.books)
    assert not codes[[3, 5, 7]].any() and np.isnan(err[3]) and err[5] == np.inf and err[7] == np.inf
    keep = np.ones(len(x), bool); keep[[3, 5, 7]] = False
    assert np.array_equal(codes[keep], c.codes[keep])


def no_gpu(monkeypatch):
    from hashgan_amd import _native, metric

    def boom(*a, **k):
        raise AssertionError("the GPU was reached")
    monkeypatch.setattr(_native, "Context", boom)
    monkeypatch.setattr(metric._Pool, "acquire", classmethod(boom))


def test_encode_gpu_argument_errors_need_no_gpu(monkeypatch):
    no_gpu(monkeypatch)
    books = np.zeros((2, 4, 3), np.float32)
    x = np.zeros((5, 6), np.float32)
    for bad_x, bad_books in [(x.astype(np.int32), books), (x[:, :5], books), (x[0], books), (x.astype(np.float64), books),
                             (x, books.astype(np.float64)), (x, books[0]), (x, np.zeros((2, 257, 3), np.float32)),
                             (np.zeros((5, 256), np.float32), np.zeros((2, 4, 128), np.float32)), (x[:0], books)]:
        with pytest.raises(ValueError):
            pq.encode_gpu(bad_x, bad_books)
    nf = books.copy()
    nf[1, 2, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        pq.encode_gpu(x, nf)
    with pytest.raises(AssertionError, match="GPU was reached"):             # (the guard itself: valid arguments do go to the GPU)
        pq.encode_gpu(x, books)


def test_maps_quantise_queries_argument_errors_need_no_gpu(monkeypatch):
    no_gpu(monkeypatch)
    with pytest.raises(ValueError, match="quantised=True"):
        MAPs(10, quantise_queries=True)
    with pytest.raises(ValueError):
        MAPs(10, quantised=True, quantise_queries=True, binarize=True)
    books = np.zeros((2, 4, 3), np.float32)
    lab = np.ones((5, 2), np.int64)
    db = types.SimpleNamespace(output=np.zeros((5, 6), np.float32), codebooks=books, label=lab)
    m = MAPs(3, quantised=True, quantise_queries=True)
    with pytest.raises(ValueError, match="query.output"):                    # a query given as codes has nothing to quantise
        m.get_maps_by_feature(db, types.SimpleNamespace(codes=np.zeros((5, 2), np.uint8), label=lab))
    with pytest.raises(ValueError):                                          # the wrong width
        m.get_maps_by_feature(db, types.SimpleNamespace(output=np.zeros((5, 7), np.float32), label=lab))
    with pytest.raises(ValueError):                                          # integers
        m.get_maps_by_feature(db, types.SimpleNamespace(output=np.zeros((5, 6), np.int32), label=lab))
    with pytest.raises(ValueError, match="resident"):
        m.get_maps_by_feature(None, types.SimpleNamespace(output=np.zeros((5, 6), np.float32), label=lab))
    # a database with neither .codes nor .codebooks: the same refusal as before
    with pytest.raises(ValueError, match="codes / .codebooks"):
        MAPs(3, quantised=True).get_maps_by_feature(types.SimpleNamespace(output=np.zeros((5, 6), np.float32), label=lab),
                                                    types.SimpleNamespace(output=np.zeros((5, 6), np.float32), label=lab))

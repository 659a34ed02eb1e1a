"""Label-free relevance, the parts that need no GPU: the NumPy reductions of hashgan_amd.neighbours on hand-made tables, the argument
errors raised before any GPU call, the new exports, and the oracle helper against a hand-made case."""
import numpy as np
import pytest

from hashgan_amd import _native
from hashgan_amd import neighbours as NB
from tests import neighbour_oracle as NO

NAN = np.nan


def test_recall_from_tables():
    hits = np.array([[1, 2, 4], [0, 0, 0], [0, 3, 3], [1, 1, 2]])
    count = np.array([4, 0, 3, 8])                                           # query 1 has no neighbours: left out of the mean
    want = np.array([(1 / 4 + 0 / 3 + 1 / 8) / 3, (2 / 4 + 3 / 3 + 1 / 8) / 3, (4 / 4 + 3 / 3 + 2 / 8) / 3])
    assert np.allclose(NB.recall_from_tables(hits, count), want, rtol=2.0 ** -50, atol=0)
    assert np.isnan(NB.recall_from_tables(np.zeros((2, 3), int), np.zeros(2, int))).all()      # nobody has neighbours
    assert NB.recall_from_tables(np.zeros((0, 2), int), np.zeros(0, int)).shape == (2,)
    with pytest.raises(ValueError):
        NB.recall_from_tables(hits, count[:3])


def test_std_ap_from_tables():
    ks = (1, 2, 5)
    # query 0: n_q = 2, hits at ranks 1 and 4 -> the reference's AP@5 = (1/1 + 2/4) / 2, the textbook's (1/1 + 2/4) / min(2, 5)
    # query 1: n_q = 0;  query 2: n_q = 7 > k, one hit at rank 2;  query 3: n_q = 3, no hit anywhere
    ap = np.array([[1.0, 1.0, 0.75], [NAN, NAN, NAN], [NAN, 0.5, 0.5], [NAN, NAN, NAN]])
    hits = np.array([[1, 1, 2], [0, 0, 0], [0, 1, 1], [0, 0, 0]])
    count = np.array([2, 0, 7, 3])
    m, per = NB.std_ap_from_tables(ap, hits, count, ks)
    want = np.array([[1.0, 0.5, 0.75], [NAN, NAN, NAN], [0.0, 0.25, 0.1], [0.0, 0.0, 0.0]])
    assert np.allclose(per, want, rtol=2.0 ** -50, atol=0, equal_nan=True)
    assert np.isnan(per[1]).all() and not np.isnan(per[[0, 2, 3]]).any()
    assert np.allclose(m, np.array([1.0 / 3, 0.75 / 3, 0.85 / 3]), rtol=2.0 ** -50, atol=0)
    # k > n_q divides by n_q, k < n_q by k
    assert per[0, 2] == 0.75 * 2 / 2 and per[2, 1] == 0.5 * 1 / 2
    assert np.isnan(NB.std_ap_from_tables(ap[1:2], hits[1:2], count[1:2], ks)[0]).all()
    with pytest.raises(ValueError):
        NB.std_ap_from_tables(ap, hits, count, ks[:2])


def test_metrics_from_tables_conventions():
    ks = (1, 2, 5)
    ap = np.array([[1.0, 1.0, 0.75], [NAN, NAN, NAN], [NAN, 0.5, 0.5]])
    hits = np.array([[1, 1, 2], [0, 0, 0], [0, 1, 1]])
    count = np.array([2, 0, 7])
    out = NB.metrics_from_tables(ap, hits, count, ks)
    assert np.array_equal(out["map"], np.array([1.0, 0.75, 0.625]))          # the reference's mean over the queries with a hit
    assert np.allclose(out["precision"], np.array([1 / 3, 2 / 6, 3 / 15]), rtol=2.0 ** -50, atol=0)     # over ALL queries
    assert np.allclose(out["recall"], np.array([0.25, 0.5 * (1 / 2 + 1 / 7), 0.5 * (1 + 1 / 7)]), rtol=2.0 ** -50, atol=0)
    assert np.array_equal(out["per_query"]["count"], count)
    none = NB.metrics_from_tables(np.full((2, 1), NAN), np.zeros((2, 1), int), np.array([3, 0]), (4,))
    assert np.isnan(none["map"][0]) and none["map_std"][0] == 0.0 and none["recall"][0] == 0.0


def test_argument_errors_need_no_gpu():
    q, db = np.ones((3, 8)), np.ones((20, 8))
    gt = np.arange(12).reshape(3, 4)
    ks = (1, 5)
    with pytest.raises(ValueError, match="rows"):
        NB.neighbour_metrics_at_k(q, db, gt[:2], ks)                         # one row per query
    bad = gt.copy(); bad[1, 2] = -1
    with pytest.raises(ValueError, match="negative"):
        NB.neighbour_metrics_at_k(q, db, bad, ks)
    far = gt.copy(); far[0, 0] = 20
    with pytest.raises(ValueError, match="outside"):
        NB.neighbour_metrics_at_k(q, db, far, ks)
    with pytest.raises(ValueError, match="16384"):
        NB.neighbour_metrics_at_k(q, db, np.zeros((3, 16385), np.int64), ks)
    with pytest.raises(ValueError, match="16384"):
        NB.binary_vs_float(q, db, 16385, ks)
    with pytest.raises(ValueError, match="mode"):
        NB.neighbour_metrics_at_k(q, db, gt, ks, mode="cosine")
    with pytest.raises(ValueError, match="mode"):
        NB.binary_vs_float(q, db, 4, ks, modes=("hamming", "euclid"))
    with pytest.raises(ValueError):
        NB.neighbour_metrics_at_k(q, db, gt.astype(np.float64), ks)          # ids are integers
    with pytest.raises(ValueError):
        NB.neighbour_metrics_at_k(q, db[:, :4], gt, ks)                      # code lengths differ
    with pytest.raises(ValueError):
        NB.neighbour_metrics_at_k(q, db, gt, (5, 1))                         # cut-offs ascend
    with pytest.raises(ValueError):
        NB.neighbour_radius_curves(q, db, gt[:2])
    with pytest.raises(ValueError):
        NB.exact_neighbours(q, db, 21)                                       # G <= N
    pad = gt.copy(); pad[2, 1:] = NB.PAD                                     # the pad value is no id: accepted by the check
    assert NB._check_sets(pad, 3, 20).dtype == np.uint32


def test_new_exports_are_bound():
    new = ("hg_set_neighbours", "hg_neighbours_from_lists", "hg_get_neighbours", "hg_match_neighbours", "hg_nbr_hist", "hg_get_nbr_hist")
    for name in new:
        assert name in _native.EXPORTS and name in _native._SIGNATURES
    for method in ("set_neighbours", "neighbours_from_lists", "get_neighbours", "match_neighbours", "nbr_hist", "get_nbr_hist"):
        assert callable(getattr(_native.Context, method))


def test_oracle_helper_on_a_hand_made_case():
    P = NO.PAD
    gt = np.array([[7, P, 2, 9], [P, P, P, P]], dtype=np.uint32)
    idx = np.array([[2, 5, 9, 1, 0], [3, 4, 5, 6, 7]])
    table, cnt = NO.sorted_table(gt)
    assert table.tolist() == [[2, 7, 9, P], [P, P, P, P]] and cnt.tolist() == [3, 0]
    m = NO.match_bits(idx, gt)
    assert m.tolist() == [[1, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    ap, rel = NO.ap_rows(m)
    assert ap[0] == (1 / 1 + 2 / 3) / 2 and np.isnan(ap[1]) and rel.tolist() == [2, 0]
    ap_k, hits_k = NO.ap_at(m, (1, 3))
    assert hits_k.tolist() == [[1, 2], [0, 0]] and ap_k[0, 0] == 1.0
    w = NO.bitmap_words(np.ones((1, 65), np.uint8))
    assert w.shape == (1, 2) and w[0, 0] == np.uint64(0xFFFFFFFFFFFFFFFF) and w[0, 1] == np.uint64(1)
    qb = np.array([[0, 0, 0]], np.uint8)
    db = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
    h = NO.nbr_hist(qb, db, np.array([[3, 0, P, 2]], np.uint32))
    assert h[:, 0].tolist() == [1, 1, 0, 1]

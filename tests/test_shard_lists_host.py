"""The two list exchange units of a database-sharded context, modelled with NumPy (no GPU): tests/shard_list_cases.py builds every
shard's grade plane and vote table from the canonical ranking by the definitions of hashgan_amd/csrc/hg_list_merge.hpp; here their
merge is held against the whole database's, the owned-slot counts against R and the cut-offs, and the shapes against the properties
tests/test_shard_lists_gpu.py relies on.  This pins the layout the GPU test then reads back from the device."""
import numpy as np
import pytest
from tests import shard_list_cases as L
from tests import shard_side_cases as S

NAMES = list(L.SHAPES)


@pytest.mark.parametrize("ks", [L.KS_LONG, L.KS_SHORT])
@pytest.mark.parametrize("G", L.GS)
@pytest.mark.parametrize("name", NAMES)
def test_the_shards_units_merge_into_the_whole_databases(name, G, ks):
    _, _, ql, dl = L.make(name)
    C, R = dl.shape[1], ks[-1]
    planes = [L.grade_plane(name, G, r, R) for r in range(G)]
    plane, own = L.merge_grades(planes)
    whole_plane, whole_own = L.grade_plane(name, 1, 0, R)
    assert np.array_equal(plane, whole_plane) and np.array_equal(own, whole_own)
    assert (own[:L.Q] == R).all() and (own[L.Q:] == 0).all()
    assert np.array_equal(whole_plane[:, :R], L.grades(name)[:, :R]) and not whole_plane[:, R:].any()
    assert plane.shape == (L.Q, L.rp_of(R)) and L.rp_of(R) % 16 == 0 and 0 <= L.rp_of(R) - R < 16
    assert len(L.grade_block(name, G, 0, R)) == L.Q * L.rp_of(R) + 4 * L.QPAD

    tabs = [L.vote_table(name, G, r, ks) for r in range(G)]
    tab = L.merge_votes(tabs)
    assert np.array_equal(tab, L.vote_table(name, 1, 0, ks))
    assert tabs[0].shape == (len(ks), C + 1, L.QPAD) and tabs[0].nbytes == 4 * len(ks) * (C + 1) * L.QPAD
    for j, k in enumerate(ks):
        assert (tab[j, C, :L.Q] == k).all() and not tab[j, :, L.Q:].any()
        # the whole database's counts by the definition: rows of class c among the first k ranks
        want = dl[L.ranking(name)[0][:, :k]].astype(np.int64).sum(1)
        assert np.array_equal(tab[j, :C, :L.Q].T, want)


@pytest.mark.parametrize("name", NAMES)
def test_the_shapes_have_the_properties_the_gpu_test_relies_on(name):
    b, C, multihot = L.SHAPES[name]
    qb, db, ql, dl = L.make(name)
    assert qb.shape == (L.Q, b) and db.shape == (L.N, b) and ql.shape == (L.Q, C) and dl.shape == (L.N, C)
    idx, dist = L.ranking(name)
    for G in (2, 3, 8):
        # (query, shard) pairs that own no slot of the top 7
        empty = sum(int((L.owner_mask(name, G, r, 7).sum(1) == 0).sum()) for r in range(G))
        assert (1 <= empty <= 33) if G < 8 else (218 <= empty <= 276), (G, empty)
        # queries whose cut at 7 falls inside a Hamming tie group with rows of more than one shard
        starts = np.array([lo for lo, _ in S.shard_bounds(L.N, G)])
        split = 0
        for q in range(L.Q):
            group = idx[q, dist[q] == dist[q, 6]]
            split += int(dist[q, 7] == dist[q, 6] and len(set(np.searchsorted(starts, group, side="right"))) > 1)
        assert 42 <= split <= 70, (G, split)
    g = L.grades(name)
    if name == "b64_c81_multihot":
        assert g.max() == 11 and not ql[5].any()
    if name == L.OWN:
        assert C == 200 and b == 64 and (C + 63) // 64 == 4                      # four label words: the k_match path
        assert g.max() == L.HEAVY_LABELS and g[L.HEAVY_QUERY].max() == L.HEAVY_LABELS
        assert not ql[L.NO_LABEL_QUERY].any() and not g[L.NO_LABEL_QUERY].any()
        assert 1 <= dl.sum(1).min() and dl.sum(1).max() <= L.HEAVY_LABELS and dl[:, C - 1].any() and ql[:, C - 1].any()
        assert all(dl[:, 64 * w:64 * (w + 1)].any() for w in range(4))           # every label word carries votes
    if not multihot:
        assert g.max() == 1


def test_the_cutoffs_meet_the_list_walks_chunk_boundary():
    assert L.KS_LONG[-1] == L.N and 256 in L.KS_LONG and 257 in L.KS_LONG and L.KS_SHORT[-1] == 7
    assert L.rp_of(7) == 16 and L.rp_of(L.N) == 1040

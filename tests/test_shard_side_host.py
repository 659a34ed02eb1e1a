"""Host side of the sharded side metrics (no GPU): the generators of tests/shard_side_cases.py have the properties the GPU tests rely
on, the reductions lifted out of extra_metrics.tie_aware_map / tie_aware_precision_recall_at_k return what the inlined code returned,
and the statement the device merge implements -- the zero-padded per-shard tables add up to the whole database's -- holds by brute force."""
import numpy as np
import pytest
from tests import shard_side_cases as S
from tests import tie_oracle
from hashgan_amd import extra_metrics as X
from hashgan_amd import sharded


def test_shard_bounds_are_the_products_and_every_shard_is_non_empty():
    for G in S.GS:
        bounds = S.shard_bounds(S.N, G)
        assert bounds == sharded.shard_bounds(S.N, G)
        assert all(rows >= 1 for _, rows in bounds) and sum(rows for _, rows in bounds) == S.N
    assert sorted({rows for _, rows in S.shard_bounds(S.N, 8)}) == [128, 129]          # uneven: N is prime
    assert -(-S.Q // 64) * 64 == 128 and S.Q % 64 != 0                                # one full unit, one partly filled


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_generators_are_binary_and_of_the_stated_shape(name):
    b, C, multihot = S.SHAPES[name]
    qb, db, ql, dl = S.make(name)
    assert qb.shape == (S.Q, b) and db.shape == (S.N, b) and ql.shape == (S.Q, C) and dl.shape == (S.N, C)
    for a in (qb, db, ql, dl):
        assert set(np.unique(a)) <= {0, 1}
    if not multihot:
        assert (dl.sum(1) == 1).all() and (ql.sum(1) == 1).all()
        assert S.defined_G(ql, dl) == 2 and S.bands(b, 2) == 1


def test_multihot_case_is_banded_and_only_the_last_shard_has_the_common_grade_count():
    b, C, _ = S.SHAPES["b64_c81_multihot"]
    qb, db, ql, dl = S.make("b64_c81_multihot")
    Gc = S.defined_G(ql, dl)
    assert Gc == 12 >= 11 and (b + 1) * Gc > S.CELLS and S.bands(b, Gc) == 2            # the whole database: banded
    assert ql[5].sum() == 0 and ql[S.HEAVY_QUERY].sum() == S.HEAVY_QUERY_LABELS
    assert dl[:-1].sum(1).max() <= S.ROW_LABELS_MAX and dl[-1].sum() == S.HEAVY_ROW_LABELS
    assert (ql[S.HEAVY_QUERY].astype(int) @ dl[-1].astype(int)) == Gc - 1                # the top grade does occur
    for G in S.GS[1:]:
        own = [S.defined_G(ql, dl[lo:lo + n]) for lo, n in S.shard_bounds(S.N, G)]
        assert own[-1] == Gc and all(g == S.ROW_LABELS_MAX + 1 < Gc for g in own[:-1]), (G, own)
        assert max(own) == Gc                                                           # what the ranks agree on
        assert S.bands(b, own[-1]) == 2 and S.bands(b, own[0]) == 1                      # a banded and an unbanded pass meet in one merge


@pytest.mark.parametrize("name", ["b8_c10", "b64_c81_multihot"])
def test_zero_padded_shard_tables_add_up_to_the_whole_databases(name):
    """The statement k_side_merge implements, by brute force, for every G of the GPU test."""
    qb, db, ql, dl = S.make(name)
    Gc = S.defined_G(ql, dl)
    whole_rel, whole_grade, whole_joint = S.brute_rel(qb, db, ql, dl), S.brute_grade(qb, db, ql, dl), S.brute_joint(qb, db, ql, dl, Gc)
    assert (whole_rel[0].sum(0) == S.N).all() and (whole_grade.sum(0) == S.N).all() and (whole_joint.sum((0, 1)) == S.N).all()
    for G in S.GS:
        all_, rel, grade, joint = 0, 0, 0, 0
        for lo, n in S.shard_bounds(S.N, G):
            a, r = S.brute_rel(qb, db[lo:lo + n], ql, dl[lo:lo + n])
            all_, rel = all_ + a.astype(np.int64), rel + r.astype(np.int64)
            grade = grade + S.brute_grade(qb, db[lo:lo + n], ql, dl[lo:lo + n]).astype(np.int64)
            Gs = S.defined_G(ql, dl[lo:lo + n])
            joint = joint + S.pad_grades(S.brute_joint(qb, db[lo:lo + n], ql, dl[lo:lo + n], Gs), Gc).astype(np.int64)
        assert np.array_equal(all_, whole_rel[0]) and np.array_equal(rel, whole_rel[1]), G
        assert np.array_equal(grade, whole_grade) and np.array_equal(joint, whole_joint), G
        # the column totals the merge checks
        assert (all_.sum(0) == S.N).all() and (grade.sum(0) == S.N).all() and (joint.sum((0, 1)) == S.N).all()


def _recorded_tie_tables():
    """[Q, nR] tables of the shape Context.get_tie_ap returns, from the CPU oracle on the b = 8 case (every cut-off inside a tie group),
    with three columns appended by hand: no query has a hit, every p_hit is 0 or 1 with NaN APs where it is 0, and a single query."""
    qb, db, ql, dl = S.make("b8_c10")
    all_h, rel_h = tie_oracle.tables(qb[:12], db, ql[:12], dl)
    t = tie_oracle.over_queries(tie_oracle.fast, all_h, rel_h, S.CUTOFFS)
    ap, p_hit = t["ap"], t["p_hit"]
    none = np.zeros((12, 1))
    sure = (np.arange(12) % 3 != 0).astype(np.float64)[:, None]
    ap = np.concatenate([ap, np.full((12, 1), np.nan), np.where(sure > 0, 0.25 + np.arange(12)[:, None] / 64.0, np.nan)], axis=1)
    p_hit = np.concatenate([p_hit, none, sure], axis=1)
    return dict(t, ap=ap, p_hit=p_hit), rel_h.sum(1)


def test_lifted_map_reduction_is_the_inlined_code():
    t, total_rel = _recorded_tie_tables()
    assert ((t["p_hit"] > 0) & (t["p_hit"] < 1)).any() and (t["p_hit"][:, -2] == 0).all()      # fractional weights and a dead column are there
    # tie_aware_map's lines as they stood before the helper was lifted out of it
    w = t["p_hit"]
    den = w.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(den > 0, np.where(w > 0, w * t["ap"], 0.0).sum(0) / den, np.nan)
    got = X.map_from_tie_tables(t["ap"], t["p_hit"])
    assert got.dtype == m.dtype and got.tobytes() == m.tobytes()
    assert np.isnan(m[-2]) and np.isfinite(m[:-2]).all()
    out = X.tie_map_from_tables(t, total_rel)
    assert out["map"].tobytes() == m.tobytes() and sorted(out["per_query"]) == sorted(list(t) + ["total_rel"])
    assert all(out["per_query"][k] is t[k] for k in t) and out["per_query"]["total_rel"] is total_rel
    one = X.map_from_tie_tables(t["ap"][:1], t["p_hit"][:1])                                     # a single query: its own AP where it has a hit
    assert np.array_equal(one[t["p_hit"][0] > 0], t["ap"][0][t["p_hit"][0] > 0])


def test_lifted_precision_recall_reduction_is_the_inlined_code():
    t, total_rel = _recorded_tie_tables()
    ks = np.asarray(S.CUTOFFS, dtype=np.int64)
    rel_exp = t["rel_exp"]
    for tr in (total_rel, np.where(np.arange(12) % 4 == 0, 0, total_rel), np.zeros(12, dtype=np.int64)):
        # tie_aware_precision_recall_at_k's lines as they stood
        precision = (rel_exp / ks[None, :]).mean(0)
        ok = tr > 0
        recall = (rel_exp[ok] / tr[ok, None]).mean(0) if ok.any() else np.full(len(ks), np.nan)
        p, r = X.tie_precision_recall_from_tables(rel_exp, tr, ks)
        assert p.tobytes() == precision.tobytes() and r.tobytes() == recall.tobytes()


def test_shard_functions_refuse_bad_arguments_before_any_exchange():
    """A context-shaped object whose every GPU call and a communicator whose every collective would raise: the argument errors come first."""

    class Ctx:
        Q, N, n_total, b, C = S.Q, 129, S.N, 64, 10

        def census(self, which):
            return self.kind

        def __getattr__(self, name):
            raise AssertionError("GPU call %s before the arguments were checked" % name)

    class Comm:
        world, rank = 8, 0

        def __getattr__(self, name):
            raise AssertionError("collective %s before the arguments were checked" % name)

    ctx, comm = Ctx(), Comm()
    ctx.kind = (0, 0, 0, False)
    for fn in (sharded.tie_aware_map_shard, sharded.tie_aware_precision_recall_at_k_shard, sharded.tie_aware_graded_at_k_shard):
        for bad in ((0, 5), (5, 5), (7, 3), (1, S.N + 1), (), (1.5,)):
            with pytest.raises(ValueError):
                fn(ctx, comm, bad)
    with pytest.raises(ValueError):
        sharded.tie_aware_graded_at_k_shard(ctx, comm, (1, 5), gain="cubic")
    ctx.C = 256
    for fn in (sharded.grade_histograms_shard, sharded.distance_grade_histograms_shard):
        with pytest.raises(ValueError):
            fn(ctx, comm)
    with pytest.raises(ValueError):
        sharded.tie_aware_graded_at_k_shard(ctx, comm, (1, 5))
    ctx.C = 10
    ctx.kind = (3, 0, 0, True)                                                       # real-valued entries
    for fn in (sharded.lookup_histograms_shard, sharded.hamming_radius_curves_shard, sharded.grade_histograms_shard,
               sharded.distance_grade_histograms_shard):
        with pytest.raises(ValueError):
            fn(ctx, comm)
    for fn in (sharded.tie_aware_map_shard, sharded.tie_aware_precision_recall_at_k_shard, sharded.tie_aware_graded_at_k_shard):
        with pytest.raises(ValueError):
            fn(ctx, comm, (1, 5))
    ctx.kind = (0, 0, 0, False)
    ctx.n_total = None                                                                # nothing loaded
    with pytest.raises(ValueError):
        sharded.lookup_histograms_shard(ctx, comm)

"""The re-ranked Hamming ranking on the paths tests/test_rerank_gpu.py leaves unrun (needs an MI355X): every k_rr_collect<NW>, the three
routes of k_rr_order (the whole query in LDS; group by group in LDS; radix groups next to LDS groups, the cut inside either kind),
k_rr_score's group walk started in the middle of a list of several groups, the key's index field above bit 15 and above bit 19, chunks
that start inside a 64-query tile, scores of either sign, denormal, zero and +inf, a permuted database, a second-hand context.

The reference is tests/rerank_oracle.py::rerank throughout.  idx, dist and match are compared with ==, score and ap by their bytes, rel
as integers; the three route counters and the record count are the oracle's (rerank_oracle.route).  Every case asserts the premises
that make it reach its route before it runs (tests/test_rerank_host.py holds the same premises without a GPU)."""
import functools

import numpy as np
import pytest

from tests import rerank_oracle as RO
from tests.test_rerank_gpu import OPTS, assert_equals_oracle, bits, new_ctx, outputs

pytestmark = pytest.mark.gpu

STATS = ("rerank_records", "rerank_chunks", "rerank_groups_lds", "rerank_groups_global")


def run(ctx, R):
    got = outputs(ctx, R)
    return got, {k: ctx.get_stat(k) for k in STATS}


def fresh(qf, dbf, ql, dl, R, opts=OPTS):
    ctx = new_ctx(qf, dbf, ql, dl, opts=opts)
    try:
        return run(ctx, R)
    finally:
        ctx.close()


def assert_route(stats, r, chunks=1):
    assert stats == dict(rerank_records=r["records"], rerank_chunks=chunks, rerank_groups_lds=r["groups_lds"], rerank_groups_global=r["groups_global"]), stats


def assert_same_bytes(a, b):
    for k in a:
        assert a[k].dtype == b[k].dtype and bits(a[k]) == bits(b[k]), k


@pytest.mark.parametrize("b", RO.WIDTHS)
def test_every_code_width(b):
    """k_rr_collect<NW> for NW = 1 ... 8 (b = 32 NW - 1: a ragged last word) and two widths that fill their last word."""
    qf, dbf, ql, dl, R, o = RO.width_case(b)
    r = RO.width_premises(qf, dbf, R, o)
    got, stats = fresh(qf, dbf, ql, dl, R)
    assert_equals_oracle(got, o)
    assert_route(stats, r)


def test_group_by_group_in_lds():
    """M_q > 16 384 with every group inside the LDS: rr_sort_lds at off > 0, and k_rr_score's walk over nine groups from the middle."""
    qf, dbf, ql, dl, R, o = RO.lds_groups_case()
    r = RO.lds_groups_premises(R, o)
    got, stats = fresh(qf, dbf, ql, dl, R)
    assert_equals_oracle(got, o)
    assert stats["rerank_groups_global"] == 0
    assert_route(stats, r)


@functools.lru_cache(maxsize=None)
def mixed_run(name):
    qf, dbf, ql, dl, R, o = RO.mixed_case(name)
    return fresh(qf, dbf, ql, dl, R)


@pytest.mark.parametrize("name", list(RO.MIXED_R))
def test_radix_and_lds_groups_in_one_query(name):
    """Four LDS groups, the radix group d = 4 (scores of both signs, indices beyond 2^16, duplicated rows), then -- at the larger R -- an
    LDS group behind it: the cut inside the radix group, and inside the LDS group with the radix group emitted whole."""
    qf, dbf, ql, dl, R, o = RO.mixed_case(name)
    r = RO.mixed_premises(name, o)
    got, stats = mixed_run(name)
    assert_equals_oracle(got, o)
    assert stats["rerank_groups_global"] == len(qf)
    assert_route(stats, r)


@functools.lru_cache(maxsize=None)
def high_index_run():
    qf, dbf, ql, dl, R, o = RO.high_index_case()
    return fresh(qf, dbf, ql, dl, R)


def test_index_bits_20_to_23():
    """One radix group of 1 050 000 rows per query whose best rows are the last ones: nibbles 4 and 5 of the key decide ranks, and
    rr_emit unpacks indices beyond 2^20."""
    qf, dbf, ql, dl, R, o = RO.high_index_case()
    r = RO.high_index_premises(R, o)
    got, stats = high_index_run()
    assert_equals_oracle(got, o)
    assert_route(stats, r)


def test_chunks_that_cut_through_query_tiles():
    """Chunks [0, 84), [84, 168), [168, 200): the second starts inside tile 1 and ends in tile 2 (k_rr_collect's qt0 and live)."""
    qf, dbf, ql, dl, R, o = RO.chunk_case()
    r = RO.chunk_premises(R, o, budget_mb=1)
    ctx = new_ctx(qf, dbf, ql, dl)
    try:
        whole, whole_stats = run(ctx, R)
        ctx.set_option("dense_budget_mb", 1)
        cut, cut_stats = run(ctx, R)
    finally:
        ctx.close()
    assert whole_stats["rerank_chunks"] == 1 and cut_stats["rerank_chunks"] == 3 == r["chunks"]
    assert_same_bytes(whole, cut)
    assert_equals_oracle(whole, o)
    assert_equals_oracle(cut, o)
    assert_route(whole_stats, r)
    assert_route(cut_stats, r, chunks=3)


def test_denormal_and_zero_scores():
    """Scores that are float32 denormals of either sign and +0.0 (no loader and no kernel flushes them; none refuses the table)."""
    qf, dbf, ql, dl, R, o = RO.denormal_case()
    r = RO.denormal_premises(R, o)
    got, stats = fresh(qf, dbf, ql, dl, R)
    assert_equals_oracle(got, o)
    assert_route(stats, r)


def test_overflowing_scores():
    """+inf next to finite scores in one list: the +inf rows lead their group in index order (no loader refuses the table)."""
    qf, dbf, ql, dl, R, o = RO.overflow_case()
    r = RO.overflow_premises(R, o)
    got, stats = fresh(qf, dbf, ql, dl, R)
    assert_equals_oracle(got, o)
    assert_route(stats, r)


def test_the_stored_order_does_not_matter():
    """No two rows tie in (d, s): the permuted database gives the same dist, score, match, ap and rel, and idx through the permutation."""
    (qf, dbf, ql, dl, R, o), (dbf_p, dl_p), perm = RO.untied_case()
    r = RO.untied_premises(R, o)
    got, stats = fresh(qf, dbf, ql, dl, R)
    got_p, stats_p = fresh(qf, dbf_p, ql, dl_p, R)
    assert_equals_oracle(got, o)
    assert_route(stats, r)
    assert stats_p == stats
    for k in ("dist", "score", "match", "ap", "rel"):
        assert bits(got[k]) == bits(got_p[k]), k
    assert (perm[got_p["idx"]] == got["idx"]).all()      # row j of the permuted table is row perm[j] of the other


def test_a_second_hand_context_leaves_the_same_bytes():
    """The largest case, then a small one (no query beyond the LDS: no second buffer asked for), then a radix group again on buffers
    that stayed at the largest case's size: each equals a fresh context's bytes and the oracle."""
    big, small, head = RO.high_index_case(), RO.width_case(31), RO.high_index_head_case()
    RO.high_index_premises(big[4], big[5])
    RO.high_index_head_premises(head[4], head[5])
    ctx = new_ctx(*big[:4])
    try:
        results = [run(ctx, big[4])]
        for qf, dbf, ql, dl, R, _ in (small, head):
            ctx.set_database_f32(dbf, dl)
            ctx.set_queries_f32(qf, ql)
            results.append(run(ctx, R))
    finally:
        ctx.close()
    firsthand = [high_index_run(), fresh(*small[:5]), fresh(*head[:5])]
    for (got, stats), (want, want_stats), case in zip(results, firsthand, (big, small, head)):
        assert_same_bytes(got, want)
        assert stats == want_stats
        assert_equals_oracle(got, case[5])

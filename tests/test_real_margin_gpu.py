"""The 16-bit filter's error margin on inputs that reach it (k_real_thr2's eps, hg_real_bf.hpp): the real-valued, asymmetric and quantised
rankings on the cases of tests/real_margin_cases.py, whose top R holds rows that the filter scores short of the exact chain by nearly all
eps allows -- a margin too small for some row loses that row without a sign, the call still ending at its first attempt with a plausible
list.  tests/test_real_margin_host.py proves the cases sharp on the CPU; here every list, score and AP must be the oracle's bit for bit,
with the filter on (stat real_path bit 0) in the format the case was built for (bit 3: IEEE half), the cut sampled in 16-bit scores or in
exact chains, tightened by the second sample or not.  Nothing is asserted about real_attempts: a cut inside a plateau may overflow slices,
and the ladder then goes deeper."""
import numpy as np
import pytest

from hashgan_amd import _native
from tests import real_margin_cases as MC

pytestmark = pytest.mark.gpu

SAMPLING = [(h, s) for h in (0, 1) for s in (0, 1)]          # (real_sample_half, real_second_sample)


def _case_ids(prefix):
    return [n for n in MC.CASES if n.startswith(prefix)]


def load(ctx, c, scale=0):
    """The case's database (times 2^scale) and queries into ctx -> the ranking calls (topr, map) of its kind."""
    if c.kind == "floats":
        x = c.x if scale == 0 else (c.x.astype(np.float64) * 2.0 ** scale).astype(np.float32)
        assert ctx.set_database_f32(x, c.dl)[1] == 0
        assert ctx.set_queries_f32(c.qf, c.ql)[1] == 0
        return ctx.topr_real, ctx.map_real
    ctx.set_option("keep_query_floats", 1)
    if c.kind == "codes":
        ctx.set_option("keep_floats", 0)
        assert ctx.set_database_f32(c.x, c.dl)[1] == 0
        assert ctx.set_queries_f32(c.qf, c.ql)[1] == 0
        return ctx.topr_asym, ctx.map_asym
    assert ctx.set_database_pq(c.codes, c.books, c.dl)[1] == 0
    assert ctx.set_queries_f32(c.qf, c.ql)[1] == 0
    return ctx.topr_pq, ctx.map_pq


def check(ctx, c, calls, fmt=None, scale=0, what=""):
    """The oracle's lists, scores (times 2^scale: exact) and APs under every way to place the cut; the filter ran, in the format `fmt`."""
    topr, mapr = calls
    fmt = fmt or c.fmt
    score = c.score if scale == 0 else (c.score.astype(np.float64) * 2.0 ** scale).astype(np.float32)
    for half_sample, second in SAMPLING:
        ctx.set_option("real_sample_half", half_sample)
        ctx.set_option("real_second_sample", second)
        tag = (c.name, what, half_sample, second)
        idx, got = topr(c.R)
        path = ctx.get_stat("real_path")
        wrong = np.flatnonzero((idx != c.idx).any(1))
        assert len(wrong) == 0, tag + ("queries with another list", wrong.tolist(),
                                       "short rows missing", [int(np.setdiff1d(c.idx[q][c.short[c.idx[q]]], idx[q]).size) for q in wrong])
        assert np.array_equal(got.view(np.uint32), score.view(np.uint32)), tag
        assert path & 1, tag
        assert ((path >> 3) & 1) == (1 if fmt == "half" else 0), tag
        ap, rel = mapr(c.R)
        assert np.array_equal(ap, c.ap, equal_nan=True), tag
        assert ctx.get_stat("real_path") & 1, tag


def run(name):
    c = MC.case(name)
    ctx = _native.Context(0)
    try:
        check(ctx, c, load(ctx, c))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", _case_ids("a-"))
def test_float_tables_in_half(name):
    """b = 16, 64, 128 and 200 (one query tile per wavefront, the exact sample), plateau norms^2 >= 1."""
    run(name)


@pytest.mark.parametrize("name", _case_ids("b-"))
def test_float_tables_in_bfloat16(name):
    """bfloat16 because the largest norm^2 is below 1, or because features exceed half's range: u = 2^-8 is exactly the rounding bound,
    the short rows reach 0.95 of eps."""
    run(name)


@pytest.mark.parametrize("name", _case_ids("c-"))
def test_the_rows_of_largest_norm_wherever_they_lie(name):
    """The short rows -- the only rows of the largest norm -- in the first 16 rows alone, in the last partial group of 16 alone, in rows no
    sample visits: on a fresh context, and on one that held a database of much smaller norms and one of much larger norms before (the
    norm and the image belong to the database: each new table brings its own)."""
    c = MC.case(name)
    ctx = _native.Context(0)
    try:
        check(ctx, c, load(ctx, c), what="fresh")
        check(ctx, c, load(ctx, c, scale=24), scale=24, what="larger norms")          # (a norm left over from a smaller table loses rows)
        check(ctx, c, load(ctx, c, scale=-20), scale=-20, what="smaller norms")
        check(ctx, c, load(ctx, c), what="after both")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", _case_ids("d-"))
def test_format_boundaries(name):
    """The database's largest |x_k| just below 2^15 (half) and at 2^15 (bfloat16), its largest norm^2 just below 1 (bfloat16) and just above
    (half); a query feature of 32768, of the float32 below it, of 65520 (infinite in half), at index 5, 13 (the other lane-half of the
    query's column) and b - 1: the one wild query keeps every row, the others are filtered as ever, every list is the oracle's."""
    run(name)


@pytest.mark.parametrize("name", _case_ids("e-"))
def test_norms_whose_float32_squares_underflow(name):
    """Features near 2^-80 and 2^-70 against queries near 2^40, and ordinary rows mixed with half-subnormal and float32-subnormal ones.
    Before k_row_norm_max summed in double the first table's norm came out as 0, its margin a hundredth of the filter's error."""
    run(name)


@pytest.mark.parametrize("name", _case_ids("f-"))
def test_codes_and_quantised_tables(name):
    """hg_topr_asym / hg_map_asym on +-1 codes (only the queries round) and hg_topr_pq / hg_map_pq on a plateau of codeword combinations,
    the largest codeword that occurs used by the last row alone and a larger one by none."""
    run(name)

"""The cases of tests/test_real_margin_gpu.py are sharp: proved here on the CPU, for every one of them, with the host model of the 16-bit
filter and the restated margin of tests/real_margin_cases.py against the exact chains of oracle/real_map.py.  A case that misses a premise
is a builder to fix -- none is skipped.

The fractions of eps the short rows must reach: the issue's 0.90 (bfloat16), 0.40 (half) and 0.20 (codes) at KP = 64, and for every other
geometry real_margin_cases.share_of_eps -- the same formula -- with the same relative slack (real_margin_cases.RHO); the paper values are
the table in that module's docstring, pinned below."""
import numpy as np
import pytest

from tests import real_margin_cases as MC

ALL = pytest.mark.parametrize("name", list(MC.CASES))


def _views(c, flush=False, xmax2=None):
    """(chain, approx [Q, N] float64, eps [Q] at the highest cut the plateau allows, eps [Q] at a cut of 0, the queries the filter bounds)"""
    chain = c.chains.astype(np.float64)
    approx = MC.filter_model(c.qf, c.x, c.fmt, flush)
    xm = c.xmax2 if xmax2 is None else xmax2
    top = chain[:, c.plateau].max(1)
    bounded = ~MC.is_wild(c.qf) if c.fmt == "half" else np.ones(c.Q, bool)
    return chain, approx, MC.margin_model(c.qf, xm, c.KP, c.fmt, top), MC.margin_model(c.qf, xm, c.KP, c.fmt, np.zeros(c.Q)), bounded


def test_the_standard_cases_ask_for_the_fractions_of_the_issue():
    assert MC.case("b-bf16-scaled-down").KP == 64 and MC.case("a-half-b64").KP == 64 and MC.case("f-codes-b64").KP == 64
    assert MC.case("b-bf16-scaled-down").f >= 0.90 and MC.case("a-half-b64").f >= 0.40 and MC.case("f-codes-b64").f >= 0.20
    for r in MC.RHO.values():
        assert 0.85 < r < 1.0


@pytest.mark.parametrize("fmt,KP,n,kw,value", [
    ("bf16", 16, 15, {}, 0.990), ("bf16", 64, 63, {}, 0.984), ("bf16", 128, 127, {}, 0.977),
    ("half", 16, 15, {}, 0.465), ("half", 64, 63, {}, 0.456), ("half", 128, 127, {}, 0.443), ("half", 208, 199, {}, 0.428),
    ("half", 32, 32, dict(kind="codes", mism=3), 0.188), ("half", 64, 64, dict(kind="codes", mism=2), 0.214),
    ("half", 128, 128, dict(kind="codes", mism=2), 0.215)])
def test_the_table_of_shares_in_the_case_module(fmt, KP, n, kw, value):
    """The paper values quoted in real_margin_cases' docstring and DESIGN.md: largest norm = the short rows' own, nothing given away."""
    assert abs(MC.share_of_eps(fmt, KP, n, xnorm_ratio=1.0, **kw) - value) < 6e-4


@ALL
def test_the_case_has_the_shape_the_filter_needs(name):
    c = MC.case(name)
    assert 65536 <= c.N <= 70100 and c.N % 16 != 0
    assert 5 <= c.Q <= 12
    assert 8 * c.R <= c.N
    assert c.plateau.sum() >= 4 * c.R
    assert c.plateau_q.any()
    assert c.fmt == c.built, "the database takes another format than the case was built for"
    assert np.isfinite(c.x).all() and np.isfinite(c.qf).all()


@ALL
def test_the_top_r_holds_short_rows_at_their_share_of_eps(name):
    c = MC.case(name)
    for flush in ((False, True) if c.fmt == "half" else (False,)):
        chain, approx, eps, _, _ = _views(c, flush)
        for q in np.flatnonzero(c.plateau_q):
            top = c.idx[q]
            sh = top[c.short[top]]
            assert 8 * len(sh) >= c.R, (name, q, len(sh))
            fall = chain[q, sh] - approx[q, sh]
            assert (fall >= c.f * eps[q]).all(), (name, q, (fall / eps[q]).min(), c.f)
            # all of the plateau lies in a band much narrower than that shortfall, and everything else far from it
            pl = chain[q, c.plateau]
            assert pl.max() - pl.min() < fall.min() / 10, (name, q, (pl.max() - pl.min()) / fall.min())
            other = chain[q, ~c.plateau]
            over = other > pl.max()
            assert over.sum() < c.R and over.sum() <= len(c.above) + 1
            # (the rows above: 2^-5 higher, or a mismatch less -- many eps, unless a single huge row inflates eps itself)
            assert (other[over].min() if over.any() else np.inf) - pl.max() > min(4 * eps[q], 0.02 * pl.max())
            assert pl.min() - other[~over].max() > 4 * eps[q], (name, q, (pl.min() - other[~over].max()) / eps[q])
            if c.kind != "codes":
                assert len(np.unique(c.chains[q, c.plateau])) == c.plateau.sum(), "the plateau's chains are distinct"


@ALL
def test_the_sampled_cut_lands_in_the_plateau(name):
    """Whatever the sample computes -- exact chains or 16-bit scores -- the plateau's exact rows alone outnumber the depth of the cut, and
    the rows above the plateau do not reach it: the first attempt's cut lies in the band (or in its 16-bit image)."""
    c = MC.case(name)
    exact = c.plateau if c.kind == "codes" else c.plateau & ~c.short
    q = int(np.flatnonzero(c.plateau_q)[0])
    over = np.zeros(c.N, bool)
    over[~c.plateau] = c.chains[q, ~c.plateau] > c.chains[q, c.plateau].max()
    for sample_half in (0, 1):
        for second in (0, 1):
            stride, rank = MC.sample_plan(c.N, c.R, c.b, sample_half, second)
            assert exact[::stride].sum() + over[::stride].sum() >= rank + 2, (name, stride, rank, exact[::stride].sum())
            assert over[::stride].sum() < rank


@ALL
def test_the_margin_covers_every_pair(name):
    """|chain - approx| <= eps for every pair the filter bounds, at the smallest eps a call can meet (a cut of 0), half's subnormal
    operands kept or flushed -- with the norm the library computes now, a double sum rounded up."""
    c = MC.case(name)
    for flush in ((False, True) if c.fmt == "half" else (False,)):
        chain, approx, _, eps0, bounded = _views(c, flush)
        err = np.abs(chain - approx)[bounded]
        assert (err <= eps0[bounded][:, None]).all(), (name, flush, (err / eps0[bounded][:, None]).max())


@pytest.mark.parametrize("name", MC.UNDERFLOW)
def test_a_float32_sum_of_squares_loses_the_norm_of_tiny_features(name):
    """Why k_row_norm_max sums in double.  Features near 2^-80: every float32 square is 0, so was the norm, and the margin left was two
    orders of magnitude short of the filter's error.  Near 2^-70: the squares are subnormal, nine bits each, and the float32 norm falls
    short of the truth by 0.09 % -- more than the 1.0001 k_real_thr2 allows for it, though inside the 4 % of air the margin has otherwise."""
    c = MC.case(name)
    old = MC.xmax2_float32(c.x)
    true = float((c.x.astype(np.float64) ** 2).sum(1).max())
    assert float(old) * 1.0001 < true <= float(c.xmax2), "the float32 norm, inflated as k_real_thr2 inflates it, is no upper bound"
    if name == "e-2^-80":
        assert float(old) == 0.0 and float(c.xmax2) == 2.0 ** -149
        chain, approx, eps, _, _ = _views(c, xmax2=old)
        q = int(np.flatnonzero(c.plateau_q)[0])
        top = c.idx[q]
        sh = top[c.short[top]]
        assert ((chain[q, sh] - approx[q, sh]) > 100 * eps[q]).all(), "with the float32 norm these rows fall out of the filter"

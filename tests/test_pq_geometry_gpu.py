"""The quantised ranking's kernels on every code geometry, at filter size (hg_pq.hpp: k_pq_image16, k_pq_rescore, k_pq_expand_rows).

N = 65536 and R = 640 are the smallest sizes at which real_ladder bets (N >= 65536, 8 R <= N), so every case here runs sample, 16-bit
filter and the rescore from the codes -- where tests/test_pq_gpu.py reaches the filter with at most two code dwords per row and with
dsub = 8 alone in the 16-byte form.  A PQ row decodes by pure gather: oracle/real_map.py on pq.decode(codes, codebooks) is the whole
reference, every comparison is array_equal on bits, and every test also asserts the stat that proves its branch ran."""
import functools
import types

import numpy as np
import pytest

from hashgan_amd import pq
from tests.test_pq_gpu import oracle, pq_context, real_context, same_lists

pytestmark = pytest.mark.gpu

N, R, C = 65536, 640, 5
#   (M, dsub, K): what it is there for
GEOMETRIES = {
    (9, 4, 256): "first-wn-reload-3-dwords-G4-every-read-a-new-codeword",
    (12, 5, 7): "3-dwords-no-reload-at-mm-8-G1-K-not-a-power-of-two",
    (13, 3, 256): "4-dwords-3-pad-bytes",
    (16, 8, 16): "4-dwords-KP-128-last-two-tile-width",
    (32, 4, 256): "8-dwords",
    (16, 12, 256): "G4-register-boundary-inside-a-codeword-over-128-features",
    (5, 16, 256): "G4-register-boundary-on-a-codeword-start",
    (3, 20, 256): "G4-image-chunks-straddle-codewords",
    (2, 100, 256): "long-codewords-across-three-registers",
    (64, 1, 256): "dsub-1-16-dwords",
    (40, 2, 3): "dsub-2-K-3",
    (255, 1, 2): "most-subspaces-64-dwords-one-pad-byte",
    (17, 15, 256): "most-features-odd-dsub-5-dwords",
    (1, 64, 256): "M-1",
    (1, 252, 256): "M-1-G4-all-four-registers-252-KB-of-codebooks",
    (4, 4, 1): "K-1-every-score-ties",
}
GEO = pytest.mark.parametrize("geo", list(GEOMETRIES), ids=["%dx%dx%d-%s" % (*g, why) for g, why in GEOMETRIES.items()])


SALT = {}       # (M, dsub, K) -> another draw, where the first one misses a premise of the host-only test below


@functools.lru_cache(maxsize=None)
def geometry(M, dsub, K):
    """test_pq_gpu.case's recipe at this module's shape, the draw chosen per geometry: tanh features, K codewords per subspace drawn from the
    database's own rows, codes = encode, one row duplicated, the oracle's ranking on the decoded table -- computed once, never modified."""
    rng = np.random.default_rng([M, dsub, K, SALT.get((M, dsub, K), 0)])
    b = M * dsub
    Q = 4 if b > 128 else 6
    dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
    dl = (rng.random((N, C)) < 0.25).astype(np.int64)
    ql = (rng.random((Q, C)) < 0.25).astype(np.int64)
    books = np.stack([dbf[rng.choice(N, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    codes = pq.encode(dbf, books)
    codes[N // 3] = codes[N // 3 + 1]                                # a duplicated row: exact tie, index order
    x = pq.decode(codes, books)
    ap, idx, score, match, rel = oracle(qf, x, ql, dl, R)
    # (the decoded table is not kept: sixteen of them are half a gigabyte, and pq.decode gives it back in milliseconds)
    c = types.SimpleNamespace(Q=Q, N=N, M=M, dsub=dsub, K=K, b=b, R=R, C=C, qf=qf, ql=ql, dl=dl, books=books, codes=codes,
                              ap=ap, idx=idx, score=score, match=match, rel=rel)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def top_sets(qf, x, r):
    """The float64 top-r row sets, one sorted row per query."""
    s = qf.astype(np.float64) @ x.astype(np.float64).T
    return np.sort(np.argsort(-s, axis=1, kind="stable")[:, :r], axis=1)


# ------------------------------------------------------------------ the cases themselves (host arithmetic only)
@GEO
def test_the_geometry_has_hits_and_its_far_subspaces_decide_a_list(geo):
    """A wrong code dword behind the second changes the features of subspaces 8 and up: the case notices only if those features move
    some query's top R.  And a list with no hit says nothing about the match bits."""
    c = geometry(*geo)
    assert (c.rel > 0).any(), "no query with a hit"
    x = pq.decode(c.codes, c.books)
    assert np.array_equal(x[N // 3], x[N // 3 + 1])
    if c.M > 8:
        near = x.copy()
        near[:, 8 * c.dsub:] = 0.0
        assert not np.array_equal(top_sets(c.qf, near, R), top_sets(c.qf, x, R)), "subspaces 8 and up decide nothing"


# ------------------------------------------------------------------ 1. every geometry through the filter, and through the expanded rows
@GEO
def test_filter_and_rescore_from_the_codes_equal_the_oracle(geo):
    """Lists, score bits, match bits, APs and hit counts are the oracle's; the first attempt's filter and k_pq_rescore made them, from
    the codes alone; real_mfma = 1 ranks the same lists from the rows k_pq_expand_rows decodes, and back.  (K = 1: one distinct row,
    every score ties and no cut separates R rows from the rest -- the bets run their kernels and lose, any path to the lists will do.)"""
    c = geometry(*geo)
    bet = c.K > 1
    ctx = pq_context(c)

    def first_attempt_from_the_codes(what):
        if bet:
            assert ctx.get_stat("real_path") & 1, what + ": not the filter path"
            assert ctx.get_stat("pq_float_rows") == 0, what
            assert ctx.get_stat("real_attempts") == 1, what

    try:
        same_lists(ctx.topr_pq(R), c)
        assert np.array_equal(ctx.get_match(), c.match)
        first_attempt_from_the_codes("topr_pq")
        ap, rel = ctx.map_pq(R)
        assert np.array_equal(ap, c.ap, equal_nan=True)
        assert np.array_equal(rel, c.rel)
        first_attempt_from_the_codes("map_pq")
        ctx.timing_enable(2)
        same_lists(ctx.topr_pq(R), c, what="timed")
        names = set(ctx.timing_read())
        ctx.timing_enable(0)
        assert "k_pq_rescore" in names and "k_real_rescore" not in names and "k_asym_rescore" not in names, names
        # Up to 128 features the float32 MFMA passes read decoded rows: k_pq_expand_rows over the whole table at this geometry.  Beyond
        # 128 the filter is the only pass whatever real_mfma says (real_select), and the staged sample expands its own rows alone
        # (sampled_rows: k_pq_expand_rows with a row stride) -- by design the whole table is never asked for as floats there.
        wide = c.b > 128
        ctx.set_option("real_mfma", 1)
        same_lists(ctx.topr_pq(R), c, what="real_mfma 1")
        assert ctx.get_stat("pq_float_rows") == (0 if wide else 1)
        assert (ctx.get_stat("real_path") & 1) == (1 if wide else 0)
        ctx.set_option("real_mfma", 2)
        same_lists(ctx.topr_pq(R), c, what="real_mfma 2 again")
        first_attempt_from_the_codes("real_mfma 2 again")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. the filter's format
@functools.lru_cache(maxsize=None)
def scaled(kind):
    """The (8, 8, 256) geometry with its codebooks rescaled codeword by codeword (test_hip_real._adversarial's recipes for the rows
    of a float table): "huge" beyond IEEE half's range, "tiny" below its floor; "unused" one codeword that no row uses at 1e6."""
    base = geometry(8, 8, 256)
    rng = np.random.default_rng(len(kind) * 1000 + 64)
    books, codes, qf = base.books.copy(), base.codes.copy(), base.qf.copy()
    if kind == "huge":
        books *= (10.0 ** rng.integers(0, 7, (base.M, base.K, 1))).astype(np.float32)
    elif kind == "tiny":
        books *= (10.0 ** rng.uniform(-7, -3, (base.M, base.K, 1))).astype(np.float32)
        qf *= (10.0 ** rng.uniform(-6, -2, (base.Q, 1))).astype(np.float32)
    elif kind == "unused":
        codes[codes[:, 3] == 17, 3] = 18
        books[3, 17, :] = 1.0e6
    else:
        raise ValueError(kind)
    x = pq.decode(codes, books)
    ap, idx, score, match, rel = oracle(qf, x, base.ql, base.dl, R)
    c = types.SimpleNamespace(Q=base.Q, N=N, M=base.M, dsub=base.dsub, K=base.K, b=base.b, R=R, C=C, qf=qf, ql=base.ql, dl=base.dl,
                              books=books, codes=codes, x=x, ap=ap, idx=idx, score=score, match=match, rel=rel)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


@pytest.mark.parametrize("kind", ["huge", "tiny", "unused"])
def test_the_scaled_cases_are_what_they_are_meant_to_be(kind):
    """Host arithmetic: every score finite and not all alike, a hit somewhere; the largest row norm^2 on the side of half's window
    [1, 2^30) that the case is named for; the codeword at 1e6 occurs in no row."""
    c = scaled(kind)
    assert np.isfinite(c.score).all() and (c.rel > 0).any()
    assert (c.score[:, 0] != c.score[:, -1]).all()
    norm2 = (c.x.astype(np.float64) ** 2).sum(1).max()
    if kind == "huge":
        assert norm2 >= 2.0 ** 30
    elif kind == "tiny":
        assert norm2 < 1.0
    else:
        assert 1.0 <= norm2 < 2.0 ** 30 and not (c.codes[:, 3] == 17).any() and c.x.max() <= 1.0


@pytest.mark.parametrize("kind", ["huge", "tiny", "unused"])
def test_codebooks_beyond_half_take_the_bfloat16_image(kind):
    """Bit 3 of real_path is the filter's format: bfloat16 (k_pq_image16<false>) when the loader's bound on the rows' norm^2 leaves
    [1, 2^30); the bound runs over the codewords that occur, so a codeword no row uses does not move it."""
    c = scaled(kind)
    ctx = pq_context(c)
    try:
        same_lists(ctx.topr_pq(R), c)
        path = ctx.get_stat("real_path")
        assert path & 1, "not the filter path"
        assert ((path >> 3) & 1) == (1 if kind == "unused" else 0)
        assert ctx.get_stat("pq_float_rows") == 0
        assert np.array_equal(ctx.get_match(), c.match)
        ap, rel = ctx.map_pq(R)
        assert np.array_equal(ap, c.ap, equal_nan=True) and np.array_equal(rel, c.rel)
        path = ctx.get_stat("real_path")
        assert path & 1 and ((path >> 3) & 1) == (1 if kind == "unused" else 0)
    finally:
        ctx.close()


def test_the_huge_codebooks_take_the_path_of_the_decoded_float_table():
    """The loader's bound and k_row_norm_max on the decoded table choose the same format and the same ladder."""
    c = scaled("huge")
    a, r = pq_context(c), real_context(c)
    try:
        idx_a, score_a = a.topr_pq(R)
        idx_r, score_r = r.topr_real(R)
        same_lists((idx_a, score_a), c)
        assert np.array_equal(idx_a, idx_r) and np.array_equal(score_a.view(np.uint32), score_r.view(np.uint32))
        assert a.get_stat("real_path") == r.get_stat("real_path")
        assert a.get_stat("real_path") & 1 and ((a.get_stat("real_path") >> 3) & 1) == 0
        assert a.get_stat("real_attempts") == r.get_stat("real_attempts")
    finally:
        a.close()
        r.close()

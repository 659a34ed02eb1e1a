"""Host proofs for tests/second_hand_cases.py (no GPU): every soil / probe pair crosses the padding boundaries it claims, the probe
inputs hold the edges their references need, and every public method of _native.Context is either in the matrix or excluded by name."""
import numpy as np
import pytest

from oracle import real_map as RM
from tests import brute_refs as B
from tests import second_hand_cases as S
from hashgan_amd import _native

SAME_FAMILY = [p for p in S.PAIRS if p[1] == p[3]]
PROBES = sorted({(p[3], p[4]) for p in S.PAIRS})
# the padded quantities a family's kernels see
USES = {"hamming": ("Qpad", "words32", "words64", "LW", "bitmap_words"), "shard_step": ("Qpad", "words32", "words64", "LW"),
        "lists": ("Qpad", "words32", "words64", "LW", "bitmap_words", "cutoffs"), "neighbours": ("Qpad", "words32", "words64", "LW", "bitmap_words", "G"),
        "rerank": ("Qpad", "bpad", "LW", "bitmap_words"), "real": ("Qpad", "bpad", "LW", "bitmap_words"), "asym": ("Qpad", "bpad", "LW", "bitmap_words"),
        "devmem": ("Qpad", "bpad", "LW", "bitmap_words"), "pq": ("Qpad", "bpad_pq", "LW", "bitmap_words", "pq_tables"),
        "pq_encode": ("Qpad", "bpad_pq", "LW", "bitmap_words", "pq_tables")}


def test_the_two_base_shapes_are_the_issue_s_table():
    big, small = S.padding(S.shape("big")), S.padding(S.shape("small"))
    assert (big["Qpad"], small["Qpad"]) == (192, 64)
    assert (big["words64"], small["words64"]) == (2, 1) and (big["words32"], small["words32"]) == (4, 2)     # k_select_mx4 -> k_select_mx3
    assert (big["LW"], small["LW"]) == (2, 1)
    assert (big["bpad"], small["bpad"]) == (64, 32) and S.BIG["bf"] == 64 and S.SMALL["bf"] == 20              # no pad columns -> 12 of them
    assert (big["bpad_pq"], small["bpad_pq"]) == (64, 32) and S.SMALL["M"] * S.SMALL["dsub"] == 21
    assert (big["cutoffs"], small["cutoffs"]) == (5, 3) and S.SMALL["ks"] == (1, 7, S.SMALL["R"]) and S.BIG["ks"][-1] == S.BIG["R"]
    assert (big["pq_tables"], small["pq_tables"]) == ((8, 256), (3, 16))
    assert (big["G"], small["G"]) == (50, 7)


@pytest.mark.parametrize("pair", SAME_FAMILY, ids=[p[0] for p in SAME_FAMILY])
def test_every_pair_crosses_the_padding_boundaries_of_its_family(pair):
    tag, family, soil_shape, _, probe_shape, _ = pair
    soil, probe = S.shape(soil_shape), S.shape(probe_shape)
    ps, pp = S.padding(soil), S.padding(probe)
    for what in USES[family]:
        if what == "Qpad" and soil_shape.startswith("filter"):
            assert ps[what] == pp[what] and soil.Q != probe.Q        # the one pair inside one query tile (second_hand_cases.SHAPES says why)
            continue
        assert ps[what] != pp[what], (tag, what)
    for s in (soil, probe):
        if s.name.startswith(("bet", "filter")):
            assert s.N in (90000, 70001, 80000, 66000)    # (the bet-sized tables: the sizes the bet's own tests run)
        else:
            assert s.N % 16 != 0 and s.N % 256 != 0 and s.N % 64 != 0, (tag, "N is a multiple of a row batch or of a segment")
        assert all(1 <= k <= s.R for k in s.ks) and list(s.ks) == sorted(set(s.ks))
        assert s.G <= s.R <= s.N
        if s.name.startswith(("bet", "filter")):
            assert s.N >= 65536 and 8 * s.R <= s.N, (tag, "not a shape the bet takes")
        else:
            assert s.N < 65536
    assert (soil.N > probe.N) == (soil.R > probe.R) == (soil.C > probe.C) == (soil.b > probe.b) == (soil.bf > probe.bf)


def test_every_family_runs_both_ways_and_every_switch_shares_a_buffer():
    tags = {p[0] for p in S.PAIRS}
    assert len(tags) == len(S.PAIRS)
    for family in S.FAMILIES:
        own = [p for p in SAME_FAMILY if p[1] == family]
        assert any(S.shape(p[2]).N > S.shape(p[4]).N for p in own), (family, "no larger soil")
        assert any(S.shape(p[2]).N < S.shape(p[4]).N for p in own), (family, "no reverse pair")
    assert {"hamming_bet_" + k for k in S.BET_SELECTS} <= tags and set(S.BET_SELECTS) == {"default", "packed1", "valu"}
    assert {"real_filter", "real_filter_reverse", "hamming_bet_reverse"} <= tags
    assert {(p[1], p[3]) for p in S.PAIRS if p[1] != p[3]} == {("real", "lists"), ("pq", "asym"), ("hamming", "rerank"), ("real", "neighbours")}
    assert S.ROUTES == ("same_context", "trim", "close_and_new")


def _tie_at_the_cut(q0, table, R):
    sc = np.sort(RM.inner_products(q0[None, :], table)[0])[::-1]
    return sc[R - 1:R + 1].view(np.uint32)[0] == sc[R - 1:R + 1].view(np.uint32)[1]


@pytest.mark.parametrize("family,name", PROBES, ids=["%s-%s" % p for p in PROBES])
def test_the_probe_inputs_hold_the_edges_the_references_need(family, name):
    """A query without labels, a row without labels, a duplicated row, and -- where there is a cut -- an exact tie across it."""
    d = S.DATA[family](name)
    s = S.shape(name)
    c = d[0] if isinstance(d, tuple) else getattr(d, "real", d)
    assert (c.ql.sum(1) == 0).any() and (c.dl.sum(1) == 0).any()
    assert (c.rel > 0).any(), "no query with a hit"
    if hasattr(c, "db"):                                                 # binary codes
        assert np.array_equal(c.db[4], c.db[5])
        if s.R < s.N:
            D = np.sort(B.hamming(c.qb, c.db), axis=1)
            assert (D[:, s.R - 1] == D[:, s.R]).any(), "no distance tie across the cut"
        if not name.startswith("bet"):
            assert np.array_equal(c.qb[2], c.db[4]) and c.idx[2, :2].tolist() == [4, 5]      # the duplicates head a list, in index order
    elif family == "rerank":
        assert np.array_equal(c.dbf[5::97], c.dbf[4::97])
        if s.R < s.N:
            inside = [(c.d[q] <= c.dist[q, -1]).sum() > s.R > (c.d[q] < c.dist[q, -1]).sum() for q in range(s.Q)]
            assert any(inside), "no Hamming tie group is cut strictly inside"
    else:                                                                # float tables ranked by inner product
        assert np.array_equal(c.table[s.N // 3], c.table[s.N // 3 + 1])
        if s.R < s.N:
            assert _tie_at_the_cut(c.qf[0], c.table, s.R), "no score tie across the cut"
    if family == "lists":
        l = d[1]
        assert np.isnan(l.ap_at[0][0]).all() and l.nG >= 2 and l.grades.max() >= 2          # the unlabelled query; a pair sharing two labels
        assert (l.votes[1] == -1).any()                                                      # a (q, k) without a vote
    if family == "neighbours":
        n = d[1]
        assert n.gt_sorted[1][0] == 0 and n.match[3].sum() == 0 and n.match.sum() > 0 and (n.gt_sorted[1] < s.G).any()
    if family in ("pq", "pq_encode"):
        assert (c.table.view(np.uint32) == 0x80000000).any(), "the -0.0 codeword does not occur"


# ------------------------------------------------------------------ the completeness guard
def public_methods():
    return sorted(n for n, v in vars(_native.Context).items() if callable(v) and not n.startswith("_"))


def test_every_public_method_is_in_the_matrix_or_excluded_by_name():
    """A feature added later fails here until its entry point is placed in a family of second_hand_cases.FAMILIES (and its job) or in
    EXCLUDED with a reason; a family removed from the matrix leaves its entry points unplaced."""
    in_matrix = set()
    for family, calls in S.FAMILIES.items():
        assert any(p[3] == family for p in S.PAIRS), (family, "a family no pair probes")
        in_matrix |= set(calls)
    public = set(public_methods())
    assert in_matrix <= public and set(S.EXCLUDED) <= public, sorted((in_matrix | set(S.EXCLUDED)) - public)
    assert not in_matrix & set(S.EXCLUDED), sorted(in_matrix & set(S.EXCLUDED))
    unplaced = public - in_matrix - set(S.EXCLUDED)
    assert not unplaced, "neither in the second-hand matrix nor excluded: %s" % sorted(unplaced)
    assert all(isinstance(r, str) and r for r in S.EXCLUDED.values())

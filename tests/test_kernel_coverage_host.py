"""tools/kernel_coverage.py and the committed records of the library's __global__ instantiations (no GPU): the normaliser on both
spellings of a name, the report's text, the list against the in-tree objects, and the two records against the list -- every built
instantiation is either in tools/kernel_coverage_unreachable.txt with the dispatch line that excludes it or in
tools/kernel_coverage_reach.txt with the test that selects it (or `open`, a number that may only fall).  A pull request that adds an
instantiation fails here until its author has decided which.  Below: the host-only premises of tests/test_instantiations_gpu.py."""
import importlib.util
import os
import warnings

import numpy as np
import pytest

from tests.instantiation_refs import rescore_slices_per_wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


KC = _tool()


def _lines(*path):
    return [ln.strip() for ln in open(os.path.join(ROOT, *path), encoding="utf-8") if ln.strip() and not ln.startswith("#")]


def test_both_spellings_of_a_name_normalise_to_one():
    rows = [[p.strip(" ") for p in ln.split(" | ")] for ln in _lines("tests", "golden", "kernel_name_spellings.txt")]
    assert len(rows) >= 12
    for stub, trace, want in rows:
        assert KC.normalise(stub) == want, stub
        assert KC.normalise(trace) == want, trace
    assert KC.family("hg::k_select<8, 0, true>") == "hg::k_select" and KC.family("k_copy_in") == "k_copy_in"
    assert KC.template_args("hg::k_select<8, 0, true>") == ["8", "0", "true"]
    assert KC.template_args("hg::k_run<hg::Pair<int, 2>, hg::Mode<(anonymous namespace)::Tag> >") == ["hg::Pair<int, 2>", "hg::Mode<(anonymous namespace)::Tag>"]
    assert KC.template_args("hg::k_match") == []


def test_a_report_round_trips_through_its_text():
    built = ["hg::k_a<1, true>", "hg::k_a<2, true>", "hg::k_b", "hg::k_c_rescore<16, 1>", "hg::k_c_rescore<16, 2>"]
    text = KC.report_text(built, {"hg::k_a<2, true>", "hg::k_b", "hg::k_c_rescore<16, 2>", "at::native::k_x<3>", "hg::k_gone"}, label="after")
    marks = KC.parse_report("some words\n" + KC.report_text(built, set(), label="parent") + text, "after")
    assert marks == {"hg::k_a<1, true>": False, "hg::k_a<2, true>": True, "hg::k_b": True, "hg::k_c_rescore<16, 1>": False, "hg::k_c_rescore<16, 2>": True}
    assert not any(KC.parse_report(KC.report_text(built, set(), label="parent") + text, "parent").values())
    assert "hg::k_a [0]: 2 | 1" in text and "hg::k_c_rescore <16, .>: 2" in text and "hg::k_gone" in text


def test_the_committed_list_is_what_the_library_builds():
    from hashgan_amd import build
    build.build()                                       # (objects older than their sources, or absent: rebuilt)
    built = KC.static_names()
    listed = _lines("profiles", "kernel_instantiations.txt")
    assert sorted(set(listed)) == listed, "profiles/kernel_instantiations.txt is not sorted and free of repeats"
    new, gone = sorted(set(built) - set(listed)), sorted(set(listed) - set(built))
    assert not new and not gone, ("instantiations the list lacks: %s; listed but no longer built: %s -- run tools/kernel_coverage.py static -o "
                                  "profiles/kernel_instantiations.txt and name the test that launches each new one" % (new, gone))


# ---- premises of tests/test_instantiations_gpu.py that need no GPU ----
@pytest.mark.parametrize("N", [66000, 200000])
def test_without_the_hook_the_far_cases_run_on_32_bit_cursors(N):
    """real_launch_select_bf takes the 64-bit cursors iff (64 crow + L) 4 >= 2^32.  From the geometry code: crow = S cap (real_attempt),
    cap <= (L + 15) & ~15 (place_cut's `whole`; take_every_row: cap = L), S = ceil(N / L) (cut_segments): crow stays near N whatever the
    segment length.  Checked for every L the filter takes (a multiple of 16) up to N: at the cases' sizes the left side stays below an
    eighth of 2^32."""
    from tests.test_instantiations_gpu import far_premise
    worst = 0
    for L in range(16, N + 16, 16):
        S = -(-N // L)
        cap = (L + 15) & ~15
        assert not far_premise(S, cap, L)
        worst = max(worst, (64 * S * cap + L) * 4)
    assert worst < (1 << 32) // 8
    assert far_premise(1, 1 << 24, 1 << 24) and not far_premise(1, (1 << 24) - 16, 64)      # (where the size alone does select them)


def test_the_candidate_set_oracle_is_the_oracle():
    """tests/instantiation_refs.ranked_oracle against oracle.real_map.map_from_features, bit for bit: continuous features, features over
    seven decades, and {0, 1} features whose ties by the hundred straddle the cut."""
    from oracle import real_map as RM
    from tests.instantiation_refs import ranked_oracle
    rng = np.random.default_rng(3)
    for kind, Q, N, b, R in (("tanh", 6, 3000, 20, 700), ("huge", 5, 4000, 33, 500), ("bits", 4, 3000, 16, 400), ("tanh", 3, 500, 1, 40)):
        d = rng.standard_normal((N, b))
        q = np.tanh(rng.standard_normal((Q, b)))
        if kind == "huge":
            d *= 10.0 ** rng.integers(0, 7, (N, 1))
        elif kind == "bits":
            d, q = (rng.random((N, b)) < 0.5).astype(np.float64), (rng.random((Q, b)) < 0.5).astype(np.float64)
        else:
            d = np.tanh(d)
        dbf, qf = d.astype(np.float32), q.astype(np.float32)
        dbf[N // 3] = dbf[N // 3 + 1]
        dl, ql = (rng.random((N, 5)) < 0.25).astype(np.int8), (rng.random((Q, 5)) < 0.25).astype(np.int8)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, ap_ref, idx_ref, score_ref = RM.map_from_features(qf, dbf, ql, dl, R)
            ap, idx, score, ncand = ranked_oracle(qf, dbf, ql, dl, R)
        assert np.array_equal(idx, idx_ref) and np.array_equal(score.view(np.uint32), score_ref.view(np.uint32)), kind
        assert np.array_equal(ap, ap_ref, equal_nan=True), kind
        assert (ncand >= R).all() and (kind == "bits" or (ncand < 2 * R).all()), (kind, ncand)


def test_the_rescore_heuristic_never_picks_three_or_four_slices():
    """Why no case of tests/test_instantiations_gpu.py asks for `<KP, 3>` or `<KP, 4>` of the rescore kernels: over the heuristic's whole domain (rows
    expected per slice, every 0.004 below 64 -- the costs are smooth on the scale of a row --, every half row up to 2500, every 64 rows
    up to 10^6) it returns
    8, 6, 2 or 1; three and four slices lose to six or eight everywhere (by 2.5 % and 0.26 % at the least)."""
    seen = {}
    for i in range(16000):
        seen.setdefault(rescore_slices_per_wave(i * 0.004), i * 0.004)
    for i in range(128, 5000):
        seen.setdefault(rescore_slices_per_wave(i * 0.5), i * 0.5)
    for i in range(40, 16000):
        assert rescore_slices_per_wave(i * 64.0) in (1, 2)
    assert sorted(seen) == [1, 2, 6, 8], seen
    assert seen[2] == 64.0 and 1000 < seen[1] < 1100, seen


def test_the_slice_cases_ask_for_every_count_the_heuristic_can_give():
    """Host arithmetic only: one slice needs 1064 expected rows per slice and gets 1237 (16 features, R = N / 8); two need 64 ... 1063; six
    and eight alternate below."""
    from tests import test_instantiations_gpu as G
    got = {(b, R): G.expected_slices(G.FAR_N, b, R) for b, R in G.SLICE_CASES}
    assert got == {(16, 8250): 1, (16, 4000): 2, (64, 4000): 2, (64, 1500): 6, (64, 900): 8, (128, 4000): 2, (128, 2000): 6}, got
    assert set(got.values()) == {1, 2, 6, 8}
    assert 1.03 * G.place_cut_sample(G.FAR_N, 8250)["expect"] / G.real_segments(G.FAR_N, 16) > 1150        # (clear of the edge at 1064)


# ---- the record: every built instantiation is either unreachable, with the dispatch line that says so, or has a line that names its test ----
OPEN_AT_MOST = 208          # instantiations whose test is not named yet (tools/kernel_coverage_reach.txt, basis `open`): this number only falls


def _record(name, fields):
    rows = {}
    for ln in _lines("tools", name):
        parts = [p.strip() for p in ln.split(" | ")]
        assert len(parts) == fields and all(parts), "%s: %d fields separated by ' | ' -- got %r" % (name, fields, ln)
        assert parts[0] not in rows, "%s: %s twice" % (name, parts[0])
        rows[parts[0]] = parts[1:]
    return rows


def test_every_instantiation_is_recorded_as_unreachable_or_with_the_test_that_reaches_it():
    """A new instantiation fails here until its author writes down which test launches it -- or which dispatch line excludes it.  Neither
    file may name what is not built, no name may be in both, a `case` names a test that exists, and the `open` entries may only get fewer."""
    listed = set(_lines("profiles", "kernel_instantiations.txt"))
    unreachable, reach = _record("kernel_coverage_unreachable.txt", 3), _record("kernel_coverage_reach.txt", 4)
    assert not set(unreachable) - listed, "recorded as unreachable but not built: %s" % sorted(set(unreachable) - listed)
    assert not set(reach) - listed, "recorded with a test but not built: %s" % sorted(set(reach) - listed)
    assert not set(unreachable) & set(reach), "in both records: %s" % sorted(set(unreachable) & set(reach))
    neither = sorted(listed - set(unreachable) - set(reach))
    assert not neither, ("%d instantiations in neither tools/kernel_coverage_unreachable.txt nor tools/kernel_coverage_reach.txt, e.g. %s: name the "
                         "test that launches each, or the dispatch line that excludes it" % (len(neither), neither[:6]))
    for name, (where, why) in unreachable.items():
        path, _, line = where.split(" ")[0].partition(":")
        assert os.path.exists(os.path.join(ROOT, path)) and line.isdigit(), (name, where)
    import re
    n_open = 0
    for name, (basis, test, how) in reach.items():
        assert basis in ("case", "open"), (name, basis)
        if basis == "open":
            n_open += 1
            continue
        path, _, func = test.partition("::")
        func = func.split("[")[0]
        assert re.search(r"(?m)^def %s\(" % re.escape(func), open(os.path.join(ROOT, path), encoding="utf-8").read()), (name, test)
    assert n_open <= OPEN_AT_MOST, "%d instantiations without a named test, %d when this was last lowered" % (n_open, OPEN_AT_MOST)


def test_the_far_cases_take_the_second_sample():
    """What tools/kernel_coverage_reach.txt says of k_real_sample_count and of k_real_sample_h's 16-bit output: at N = 66000, R = 1500
    place_cut takes the second, counting sample and the first one's 1065 rows fit k_real_guess_lds."""
    from tests import test_instantiations_gpu as G
    cut = G.place_cut_sample(G.FAR_N, G.FAR_R)
    assert cut["second"] and cut["M"] == 1065 and cut["M"] <= G.RG_MMAX and cut["stride2"] == 5, cut

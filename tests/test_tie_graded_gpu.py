"""The distance-by-grade histogram on the GPU (hg_joint_hist: k_label_max, k_hist_joint, k_hist_joint_reduce) against brute-force NumPy
-- xor / popcount for the distance, the label AND for the grade, np.add.at for the counts --, its marginals against hg_rel_hist and
hg_grade_hist on the same context, its additivity over shards, its lifetime rules next to the other side metrics and the staged and
split-step sequences, and extra_metrics.tie_aware_graded_at_k on top (needs an MI355X).

Every table is compared with ==.  The one float comparison is the canonical list's DCG against the envelope: both sides are sums of at
most k products gain x discount, the envelope's taken as differences of prefix sums of the discounts per (distance, grade) cell, so the
first-order rounding bound of the two summations is (cells + 8) 2^-52 gain[C] cum[k] with cells = (b + 1) G."""
import functools

import numpy as np
import pytest
from tests import brute_refs, cases
from hashgan_amd import DeviceArray, _native, metric
from hashgan_amd import extra_metrics as X

pytestmark = pytest.mark.gpu

STATE, ARG = _native.HG_ERR_STATE, _native.HG_ERR_ARG
Q, N = 70, 773                                           # two query tiles, Qpad = 128 != Q; with min_segment = 16 several segments, a
OPTS = (("min_segment", 16),)                            # ragged last one and a ragged batch tail
CELLS = 640                                              # (distance, grade) cells of a wavefront's column that fit the LDS


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def raw(x):
    if isinstance(x, dict):
        x = tuple(x[k] for k in sorted(x))
    return tuple(a.tobytes() for a in x) if isinstance(x, tuple) else x.tobytes()


defined_G, brute_joint = brute_refs.defined_G, brute_refs.joint_hist      # (shared with tests/test_second_hand_gpu.py)


def load(ctx, qb, db, ql, dl, idx_base=0, n_total=None):
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1], idx_base, n_total)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))


def new_ctx(qb, db, ql, dl, opts=OPTS, **kw):
    ctx = _native.Context(0)
    for k, v in opts:
        ctx.set_option(k, v)
    load(ctx, qb, db, ql, dl, **kw)
    return ctx


def make(b, C, density, seed, zero_query=False, full_row=False, full_query=False):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    qb = db[rng.integers(0, N, Q)] ^ (rng.random((Q, b)) < 0.1).astype(np.uint8)
    dl = (rng.random((N, C)) < density).astype(np.int8)
    ql = (rng.random((Q, C)) < density).astype(np.int8)
    dl[::9, C - 1] = 1                                   # the last class of the last label word
    ql[:3, C - 1] = 1
    if zero_query:
        ql[5] = 0
    if full_row:
        dl[123] = 1
    if full_query:
        ql[7] = 1
    return qb, db, ql, dl


def plant_band_edges(qb, db, G):
    """Rows of the database replaced by copies of query 0 at chosen distances: the query itself, its complement, and the first and last
    distance of every band of CELLS // G distances.  (Codes only: G, a function of the labels, stays.)"""
    b = qb.shape[1]
    bw = CELLS // G
    ds = {0, b}
    for first in range(0, b + 1, bw):
        ds |= {first, min(first + bw - 1, b)}
    db = db.copy()
    for i, d in enumerate(sorted(ds)):
        row = qb[0].copy()
        row[:d] ^= 1
        db[3 * i + 1] = row
    return db, sorted(ds)


#        b,   C, density, bands expected, extras
CASES = {"b8_c1": (8, 1, 0.5, 1, {}),
         "b33_c10_zero_query_full_row": (33, 10, 0.3, 1, dict(zero_query=True, full_row=True)),
         "b64_c81": (64, 81, 0.04, None, {}),
         "b100_c130_wide": (100, 130, 0.05, None, {}),
         "b255_c255_grade_255": (255, 255, 0.04, 128, dict(full_row=True, full_query=True)),
         "b64_c16_dense": (64, 16, 0.7, 2, {}),
         "b255_c3": (255, 3, 0.6, 2, {})}


@pytest.mark.parametrize("name", list(CASES))
def test_table_equals_brute_force_and_its_marginals(name):
    b, C, density, bands_expected, extras = CASES[name]
    qb, db, ql, dl = make(b, C, density, seed=b * 1000 + C, **extras)
    G = defined_G(ql, dl)
    if name == "b64_c16_dense":
        assert G >= 10
    if name == "b255_c255_grade_255":
        assert G == 256
    ctx = new_ctx(qb, db, ql, dl)
    try:
        assert ctx.get_stat("joint_hist_grades") == 0 and ctx.get_stat("joint_hist_bands") == 0
        raises(STATE, ctx.get_joint_hist)
        ctx.joint_hist()
        assert ctx.get_stat("joint_hist_grades") == G
        bands = ctx.get_stat("joint_hist_bands")
        assert bands == (1 if (b + 1) * G <= CELLS else -(-(b + 1) // (CELLS // G)))
        if bands_expected is not None:
            assert bands == bands_expected
        if bands > 1:                                    # rows on the band edges: the width from the stat, the database loaded again
            db, planted = plant_band_edges(qb, db, ctx.get_stat("joint_hist_grades"))
            assert len(planted) >= bands + 1
            load(ctx, qb, db, ql, dl)
            raises(STATE, ctx.get_joint_hist)
            ctx.joint_hist()
            assert ctx.get_stat("joint_hist_grades") == G and ctx.get_stat("joint_hist_bands") == bands
        J = ctx.get_joint_hist()
        assert J.dtype == np.uint32 and J.shape == (b + 1, G, Q)
        ref = brute_joint(qb, db, ql, dl, G)
        assert np.array_equal(J, ref), np.argwhere(J != ref)[:5]
        if bands > 1:
            assert all(J[d, :, 0].sum() >= 1 for d in planted)
        if extras.get("zero_query"):
            assert J[:, 1:, 5].sum() == 0 and J[:, 0, 5].sum() == N
        if extras.get("full_row"):
            assert J[:, G - 1, :].sum() >= 1                # the row with every label meets the query with the most
        # marginals, on the same context
        ctx.rel_hist()
        all_, rel = ctx.get_rel_hist()
        assert np.array_equal(J.sum(1), all_) and np.array_equal(J[:, 1:, :].sum(1), rel)
        ctx.grade_hist()
        gh = ctx.get_grade_hist()
        assert np.array_equal(J.sum(0), gh[:G]) and gh[G:].sum() == 0
        assert np.array_equal(ctx.get_joint_hist(), ref)     # ... which ended nothing
    finally:
        ctx.close()


def test_the_table_does_not_depend_on_the_segments():
    """A banded pass with one segment per query tile and with two: the same table as brute force gives."""
    qb, db, ql, dl = make(64, 16, 0.7, seed=64016)
    G = defined_G(ql, dl)
    ref = brute_joint(qb, db, ql, dl, G)
    for opts in ((("max_segments", 1),), (("min_segment", 16), ("target_units", 6))):
        ctx = new_ctx(qb, db, ql, dl, opts=opts)
        try:
            ctx.joint_hist()
            assert ctx.get_stat("joint_hist_bands") == 2
            assert np.array_equal(ctx.get_joint_hist(), ref), opts
        finally:
            ctx.close()


def test_additive_over_shards():
    qb, db, ql, dl = make(33, 10, 0.3, seed=33010, full_row=True, full_query=True)   # (the row with every label is in shard 0 only)
    cut = 400
    tables = []
    for lo, hi in ((0, N), (0, cut), (cut, N)):
        ctx = new_ctx(qb, db[lo:hi], ql, dl[lo:hi], idx_base=lo, n_total=N)
        try:
            ctx.joint_hist()
            assert ctx.get_stat("joint_hist_grades") == defined_G(ql, dl[lo:hi])
            tables.append(ctx.get_joint_hist().astype(np.int64))
        finally:
            ctx.close()
    whole, parts = tables[0], tables[1:]
    G = whole.shape[1]
    assert parts[1].shape[1] < G                           # a shard's own G: pad with zeros
    total = sum(np.pad(p, ((0, 0), (0, G - p.shape[1]), (0, 0))) for p in parts)
    assert np.array_equal(total, whole)


# ------------------------------------------------------------------ lifetime (tests/test_side_results_gpu.py's pattern)
GETTERS = ("get_rel_hist", "get_graded", "get_grades", "get_grade_hist", "get_tie_ap", "get_ap_at")
KS, R = (1, 7, 50), 50


def test_reload_and_trim_end_the_table_and_the_pass_ends_nobody_elses():
    qb, db, ql, dl = make(33, 3, 0.4, seed=33003)
    C = 3
    gain, disc = X.gain_table("exp", C), X.discount_table(KS[-1])
    ctx = new_ctx(qb, db, ql, dl)
    try:
        ctx.trim()
        bytes0 = ctx.get_stat("device_bytes")                                    # the tables alone
        ctx.topr(R)
        compute = {"get_rel_hist": ctx.rel_hist, "get_graded": lambda: ctx.graded(KS, gain, disc, keep_grades=True),
                   "get_grade_hist": ctx.grade_hist, "get_tie_ap": lambda: ctx.tie_ap(KS), "get_ap_at": lambda: ctx.ap_at(KS)}
        for fn in compute.values():
            fn()
        want = {name: raw(getattr(ctx, name)()) for name in GETTERS}
        lists, bits = raw(ctx.get_topr()), raw(ctx.get_match())
        ctx.joint_hist()
        J = ctx.get_joint_hist()
        for name in GETTERS:                                                     # the pass ended no other side metric's results
            assert raw(getattr(ctx, name)()) == want[name], name
        assert raw(ctx.get_topr()) == lists and raw(ctx.get_match()) == bits     # ... nor the ranking's
        for fn in compute.values():                                              # and none of theirs ends the table
            fn()
        ctx.topr(R)
        assert np.array_equal(ctx.get_joint_hist(), J)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))           # the same queries again: a new generation
        raises(STATE, ctx.get_joint_hist)
        ctx.joint_hist()
        assert np.array_equal(ctx.get_joint_hist(), J)
        load(ctx, qb, db, ql, dl)                                               # the database again (the queries follow it)
        raises(STATE, ctx.get_joint_hist)
        ctx.joint_hist()
        assert np.array_equal(ctx.get_joint_hist(), J)
        assert ctx.get_stat("device_bytes") > bytes0
        ctx.trim()
        raises(STATE, ctx.get_joint_hist)
        assert ctx.get_stat("device_bytes") == bytes0                            # its buffers are on the context's list
        ctx.joint_hist()
        assert np.array_equal(ctx.get_joint_hist(), J)
        ctx.set_queries(metric.pack_codes(qb[:10]), metric.pack_labels(ql[:10]))   # fewer queries: the table follows
        ctx.joint_hist()
        G10 = defined_G(ql[:10], dl)
        assert np.array_equal(ctx.get_joint_hist(), brute_joint(qb[:10], db, ql[:10], dl, G10))
    finally:
        ctx.close()


def test_256_classes_are_refused():
    rng = np.random.default_rng(256)
    db, qb = rng.integers(0, 2, (300, 32), dtype=np.uint8), rng.integers(0, 2, (5, 32), dtype=np.uint8)
    dl, ql = (rng.random((300, 256)) < 0.1).astype(np.int8), (rng.random((5, 256)) < 0.1).astype(np.int8)
    ctx = new_ctx(qb, db, ql, dl)
    try:
        raises(ARG, ctx.joint_hist)
        raises(STATE, ctx.get_joint_hist)
    finally:
        ctx.close()


def test_a_staged_sequence_interrupted_by_the_pass_finishes_with_the_same_lists():
    qb, db, ql, dl = make(64, 16, 0.7, seed=64016)                               # (a banded pass: the largest LDS request)
    ctx = new_ctx(qb, db, ql, dl)
    try:
        ctx.hist()
        ctx.plan(R)
        ctx.select()
        ctx.match()
        ctx.ap()
        want = raw(ctx.get_topr()), raw(ctx.get_match()), raw(ctx.get_ap())
        hist = ctx.get_hist()
        segments = ctx.get_stat("segments")
        ctx.hist()
        ctx.plan(R)
        ctx.joint_hist()
        assert ctx.get_stat("joint_hist_bands") == 2
        assert ctx.get_stat("segments") == segments                              # the pass's geometry is its own
        ctx.select()
        ctx.match()
        ctx.ap()
        assert (raw(ctx.get_topr()), raw(ctx.get_match()), raw(ctx.get_ap())) == want
        assert np.array_equal(ctx.get_hist(), hist)
        assert np.array_equal(ctx.get_joint_hist().sum(1), hist)
    finally:
        ctx.close()


def test_a_step_in_flight_and_the_licence_to_enqueue_blind_survive_the_pass(case_cache):
    """hg_map_begin's step started before the pass returns the golden APs from hg_map_end, and the pass's first reservations -- made
    while that step is in flight -- move no buffer a blind step touches: the next hg_map_begin is still enqueued blind."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R_ = c["R"]
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        ap, _ = ctx.map(R_)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert ctx.get_stat("last_optimistic") == 1
        n0 = ctx.get_stat("map_async_steps")
        ctx.map_begin(R_)
        assert ctx.get_stat("map_async_steps") == n0 + 1
        ctx.joint_hist()                                                         # first reservations, a step in flight
        ap, _ = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        ctx.map_begin(R_)
        assert ctx.get_stat("map_async_steps") == n0 + 2, "the pass's first reservations ended the licence to enqueue blind"
        ap, _ = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert ctx.get_stat("map_async_redone") == 0
        J = ctx.get_joint_hist()
        assert ctx.get_stat("joint_hist_grades") == 2 and J.shape == (c["b"] + 1, 2, len(c["qbits"]))
        assert (J.sum((0, 1)) == len(c["dbbits"])).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------ the surface: tie_aware_graded_at_k
KS_SURFACE = (1, 5, 50, 300, N)
WORST = {"fraction": 0.0}


@functools.lru_cache(maxsize=None)
def surface_case():
    """C = 10, b = 16: 17 distances for 773 rows, so every cut-off but the last falls inside a tie group."""
    qb, db, ql, dl = make(16, 10, 0.3, seed=16010, zero_query=True)
    G = defined_G(ql, dl)
    J = brute_joint(qb, db, ql, dl, G).transpose(2, 0, 1).astype(np.int64)
    tab, disc = X.gain_table("exp", 10), X.discount_table(N)
    ref = X.tie_graded_from_tables(J, KS_SURFACE, tab[:G], disc)
    for a in (qb, db, ql, dl, J):
        a.flags.writeable = False
    return qb, db, ql, dl, G, ref, tab, disc


def same_dict(got, ref):
    assert raw(got["acg"]) == raw(ref["acg"]) and raw(got["ndcg"]) == raw(ref["ndcg"])
    assert sorted(got["per_query"]) == sorted(ref["per_query"])
    for k, v in ref["per_query"].items():
        assert got["per_query"][k].dtype == v.dtype and raw(got["per_query"][k]) == raw(v), k


def test_surface_equals_the_reduction_of_the_brute_force_table():
    qb, db, ql, dl, G, ref, _, _ = surface_case()
    got = X.tie_aware_graded_at_k(qb, db, ql, dl, KS_SURFACE)
    same_dict(got, ref)
    assert np.array_equal(X.distance_grade_histograms(qb, db, ql, dl), brute_joint(qb, db, ql, dl, G).transpose(2, 0, 1))
    pq = got["per_query"]
    assert np.isnan(pq["ndcg"][5]).all() and (pq["acg_max"][5] == 0).all()       # the query without labels
    inside = np.array(KS_SURFACE[:-1])
    assert (pq["gsum_lo"][:, :4] < pq["gsum_hi"][:, :4]).any(0).all(), inside   # the cut-offs do fall inside tie groups


def test_shuffling_the_database_changes_no_bit():
    qb, db, ql, dl, _, ref, _, _ = surface_case()
    perm = np.random.default_rng(1).permutation(N)
    same_dict(X.tie_aware_graded_at_k(qb, db[perm], ql, dl[perm], KS_SURFACE), ref)


def test_the_canonical_list_lies_inside_the_envelope():
    qb, db, ql, dl, G, ref, tab, disc = surface_case()
    canon = X.graded_relevance_at_k(qb, db, ql, dl, KS_SURFACE)["per_query"]
    pq = ref["per_query"]
    ks = np.array(KS_SURFACE)
    assert (pq["acg_min"] <= canon["acg"]).all() and (canon["acg"] <= pq["acg_max"]).all()
    cum = np.array([disc[:k].sum() for k in ks])
    slack = ((16 + 1) * G + 8) * 2.0 ** -52 * tab[10] * cum[None, :]
    over = np.maximum(np.maximum(pq["dcg_min"] - canon["dcg"], canon["dcg"] - pq["dcg_max"]), 0.0)
    WORST["fraction"] = max(WORST["fraction"], float((over / slack).max()))
    assert (over <= slack).all(), WORST
    assert np.array_equal(canon["idcg"], pq["idcg"])                           # the same ideal ordering
    # k = N: every order holds every row, the grade sums agree with the canonical list's
    assert np.array_equal(pq["gsum_lo"][:, -1] / N, canon["acg"][:, -1])


class Producer:
    """Device memory without a framework: scratch slots of private contexts, filled with memcpy_htod."""

    def __init__(self):
        self.ctxs, self.n = [], 0

    def put(self, host):
        host = np.ascontiguousarray(host)
        if self.n % 4 == 0:
            self.ctxs.append(_native.Context())
        c = self.ctxs[-1]
        ptr = c.scratch(self.n % 4, host.nbytes)
        self.n += 1
        c.memcpy_htod(ptr, host, host.nbytes)
        return ptr

    def close(self):
        for c in self.ctxs:
            c.close()


def test_device_arrays_give_the_same_bits():
    qb, db, ql, dl, _, ref, _, _ = surface_case()
    prod = Producer()
    try:
        d_db = DeviceArray(prod.put(db.astype(np.float32)), db.shape, None, "float32")
        d_dl = DeviceArray(prod.put(dl.astype(np.int32)), dl.shape, None, "int32")
        d_q = DeviceArray(prod.put(qb.astype(np.float32)), qb.shape, None, "float32")
        d_ql = DeviceArray(prod.put(ql.astype(np.bool_)), ql.shape, None, "bool")
        dev = X.tie_aware_graded_at_k(d_q, d_db, d_ql, d_dl, KS_SURFACE)
        mixed = X.tie_aware_graded_at_k(qb, d_db, ql, d_dl, KS_SURFACE)          # database on the device, queries on the host
    finally:
        prod.close()
    same_dict(dev, ref)
    same_dict(mixed, ref)


def test_largest_error_for_the_record():
    """Printed for DESIGN.md: how far the canonical list's DCG left the envelope, as a fraction of the rounding bound (run the whole
    file with -s)."""
    print("largest observed excess over the envelope: %.3g of the bound" % WORST["fraction"])
    assert WORST["fraction"] <= 1.0

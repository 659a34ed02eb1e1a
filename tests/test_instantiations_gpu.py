"""Kernel instantiations that no feature's own cases select (profiles/kernel_instantiations.txt lists the 586 the library builds; the
families below are the ones whose template parameters the other tests' shapes leave partly unvisited), each against the host reference
of its feature.

1. k_real_select_bf<KP, QT, HALF, FAR = true>: the 64-bit-cursor drain that real_launch_select_bf picks only when a wavefront's 64
   record rows span 4 GB (2^24 records per query and more).  The test hook "real_far_cursors" selects it at any size -- the drain is
   valid at every size and must deliver the same bytes as the 32-bit one.  Every filter width KP = 16 ... 256 in both image formats,
   with the hook off and on: all 64 instantiations of the family.
"""
import functools
import types
import warnings

import numpy as np
import pytest

from hashgan_amd import _native, pq
from tests.instantiation_refs import ranked_oracle, rescore_slices_per_wave

pytestmark = pytest.mark.gpu

FAR_N, FAR_R, FAR_C = 66000, 1500, 9
EXACT_WIDTHS = (16, 64, 128, 144)                      # b = KP; two query tiles per wavefront up to 128 features, one beyond


def far_premise(S, cap, L):
    """real_launch_select_bf's own choice: 64-bit cursors iff (64 crow + L) 4 >= 2^32, crow = S cap."""
    return (64 * S * cap + L) * 4 >= 1 << 32


@functools.lru_cache(maxsize=None)
def _tables(kind):
    """One 66000 x 256 table and 70 queries per image format; a case takes its first b features.  half: tanh features; bfloat16: rows
    over seven decades, beyond half's range (the "huge" features of tests/test_hip_real.py)."""
    rng = np.random.default_rng(20 + len(kind))
    d = rng.standard_normal((FAR_N, 256))
    if kind == "bfloat16":
        d *= 10.0 ** rng.integers(0, 7, (FAR_N, 1))
        q = rng.standard_normal((70, 256))
    else:
        d, q = np.tanh(d), np.tanh(rng.standard_normal((70, 256)))
    dl = (rng.random((FAR_N, FAR_C)) < 0.2).astype(np.int8)
    ql = (rng.random((70, FAR_C)) < 0.2).astype(np.int8)
    return d.astype(np.float32), q.astype(np.float32), dl, ql


@functools.lru_cache(maxsize=4)
def far_case(kind, b):
    dbf, qf, dl, ql = _tables(kind)
    dbf, qf = np.ascontiguousarray(dbf[:, :b]), np.ascontiguousarray(qf[:, :b])
    if b > 1:
        dbf[FAR_N // 3] = dbf[FAR_N // 3 + 1]          # a duplicated row: exact tie, index order
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap, idx, score, _ = ranked_oracle(qf, dbf, ql, dl, FAR_R)
    return types.SimpleNamespace(dbf=dbf, qf=qf, dl=dl.astype(np.int64), ql=ql.astype(np.int64), ap=ap, idx=idx, score=score)


def run_both_cursors(load, rank, score_map, ref, Q, half, overflow=False):
    """The call with the hook off, then on -- each on a freshly loaded database (a load resets the widened slices) --: the oracle's
    lists, score bits and APs both times, and the same bytes and the same path and attempts from both."""
    got = {}
    for far in (0, 1):
        ctx = _native.Context(0)
        try:
            ctx.set_option("real_far_cursors", far)
            load(ctx)
            idx, score = rank(ctx)
            path, attempts = ctx.get_stat("real_path"), ctx.get_stat("real_attempts")
            S, cap, N = ctx.get_stat("segments"), ctx.get_stat("slice_cap"), ctx.N
            ap, rel = score_map(ctx)
            got[far] = (idx, score.view(np.uint32), ap, rel, path, attempts, ctx.get_stat("real_path"), ctx.get_stat("real_attempts"),
                        ctx.get_stat("real_cap_boost"))
        finally:
            ctx.close()
        assert path & 1, "not the filter path"
        assert half is None or ((path >> 3) & 1) == (1 if half else 0), "the other image format"
        # (no stat gives the segment length L; N bounds it from above, which only makes the inequality harder to miss)
        assert not far_premise(S, cap, N), "the size alone selects the 64-bit cursors: the hook would prove nothing"
        assert np.array_equal(score.view(np.uint32), ref.score[:Q].view(np.uint32)), far
        assert np.array_equal(idx, ref.idx[:Q]), far
        assert np.array_equal(ap, ref.ap[:Q], equal_nan=True), far
        if overflow:                                   # slices overflowed: the `dropped` branch flagged the queries, and only the ladder's
            assert attempts > 1 and got[far][8] > 1, (attempts, got[far][8])     # retries with WIDER slices raise real_cap_boost (a shallow cut alone does not)
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else np.array_equal(a, b)


def _width_cases():
    out = []
    for kp in range(16, 257, 16):
        b = kp if kp in EXACT_WIDTHS else 255 if kp == 256 else kp - 5     # the other widths: a feature count the image pads; 255 is the loaders' limit
        for kind in ("half", "bfloat16"):
            out.append(pytest.param(kind, b, id="%s-b%d" % (kind, b)))
    return out


@pytest.mark.parametrize("kind,b", _width_cases())
def test_far_cursors_on_every_filter_width_and_image_format(kind, b):
    """N = 66000, R = 1500, Q = 20 and Q = 70 (wavefronts with lanes past Q, and a second query block at two tiles of 32)."""
    c = far_case(kind, b)
    for Q in (20, 70):
        def load(ctx):
            assert ctx.set_database_f32(c.dbf, c.dl)[1] == 0
            assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
        run_both_cursors(load, lambda ctx: ctx.topr_real(FAR_R), lambda ctx: ctx.map_real(FAR_R), c, Q, kind == "half")


@functools.lru_cache(maxsize=None)
def _coded_case(which):
    """The half table's first 64 features behind the two coded row sources: its +-1 table (asymmetric), its PQ decoding (8 x 8, K = 256)."""
    dbf, qf, dl, ql = _tables("half")
    dbf, qf = np.ascontiguousarray(dbf[:, :64]), np.ascontiguousarray(qf[:, :64])
    extra = {}
    if which == "asym":
        x = np.where(dbf > 0, 1, -1).astype(np.float32)
    else:
        rng = np.random.default_rng(5)
        books = np.stack([dbf[rng.choice(FAR_N, 256, replace=False), m * 8:(m + 1) * 8] for m in range(8)]).astype(np.float32)
        codes = pq.encode(dbf, books)
        x = pq.decode(codes, books)
        extra = dict(books=books, codes=codes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap, idx, score, _ = ranked_oracle(qf, x, ql, dl, FAR_R)
    return types.SimpleNamespace(dbf=dbf, qf=qf, dl=dl.astype(np.int64), ql=ql.astype(np.int64), ap=ap, idx=idx, score=score, **extra)


@pytest.mark.parametrize("Q", [20, 70])
def test_far_cursors_behind_the_asymmetric_ranking(Q):
    c = _coded_case("asym")

    def load(ctx):
        ctx.set_option("keep_floats", 0)
        ctx.set_option("keep_query_floats", 1)
        assert ctx.set_database_f32(c.dbf, c.dl)[1] == 0
        assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
    run_both_cursors(load, lambda ctx: ctx.topr_asym(FAR_R), lambda ctx: ctx.map_asym(FAR_R), c, Q, None)


@pytest.mark.parametrize("Q", [20, 70])
def test_far_cursors_behind_the_quantised_ranking(Q):
    c = _coded_case("pq")

    def load(ctx):
        ctx.set_option("keep_query_floats", 1)
        assert ctx.set_database_pq(c.codes, c.books, c.dl)[1] == 0
        assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
    run_both_cursors(load, lambda ctx: ctx.topr_pq(FAR_R), lambda ctx: ctx.map_pq(FAR_R), c, Q, None)


def test_far_cursors_when_the_slices_overflow():
    """The class-sorted database of tests/test_hip_real.py (features that follow the labels, rows stored class by class) at its shape: a
    query's top rows crowd into a tenth of the segments, the sampled cuts lose on slice capacity -- `room` runs out, `dropped` counts,
    the query is flagged and the call is redone with wider slices.  Same lists, same attempts as with the 32-bit cursors."""
    rng = np.random.default_rng(11)
    Q, N, b, R, C = 5, 200000, 64, 4000, 10
    proto = rng.standard_normal((C, b)).astype(np.float32)
    cls, qcls = np.sort(rng.integers(0, C, N)), rng.integers(0, C, Q)
    dbf = np.tanh(0.7 * proto[cls] + rng.standard_normal((N, b), dtype=np.float32)).astype(np.float32)
    qf = np.tanh(0.7 * proto[qcls] + rng.standard_normal((Q, b), dtype=np.float32)).astype(np.float32)
    eye = np.eye(C, dtype=np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap, idx, score, _ = ranked_oracle(qf, dbf, eye[qcls].astype(np.int8), eye[cls].astype(np.int8), R)
    ref = types.SimpleNamespace(ap=ap, idx=idx, score=score)

    def load(ctx):
        assert ctx.set_database_f32(dbf, eye[cls])[1] == 0
        assert ctx.set_queries_f32(qf, eye[qcls])[1] == 0
    run_both_cursors(load, lambda ctx: ctx.topr_real(R), lambda ctx: ctx.map_real(R), ref, Q, True, overflow=True)


# ---- 2. Hamming kernels templated on the code words NW = ceil(b / 32) = 1 ... 8 and the label words LW (1: <= 64 classes, 2: <= 128,
# 0: more -- the match bits come from k_match): every NW x LW corner of k_select (exact and bet), k_select_dense, k_select_mx (eight-byte
# and one-byte records), k_hist_rel and k_hist_joint, at the smallest shapes the features' own tests use, against oracle/hamming_map.py
# and tests/brute_refs.py.
from oracle import hamming_map as O              # noqa: E402
from hashgan_amd import metric                  # noqa: E402
from tests import brute_refs                    # noqa: E402

SEL_VALU, SEL_DENSE, SEL_MX = 1, 2, 3
WORDS = [(nw, 32 * nw - (3 if nw % 2 else 0)) for nw in range(1, 9)]        # (NW, b): full last words and ragged ones; 253 bits for NW = 8
WORDS[7] = (8, 253)
CLASSES = [(1, 10), (2, 100), (0, 150)]                                     # (LW, C)


def _codes(seed, Q, N, b, C):
    rng = np.random.default_rng(seed)
    qb = rng.integers(0, 2, (Q, b), dtype=np.uint8)
    db = rng.integers(0, 2, (N, b), dtype=np.uint8)
    db[::7] = qb[rng.integers(0, Q, len(db[::7]))] ^ (rng.random((len(db[::7]), b)) < 0.1).astype(np.uint8)      # near rows: short distances occur
    dl = (rng.random((N, C)) < 3.0 / C if C > 20 else rng.random((N, C)) < 0.3).astype(np.int8)
    ql = (rng.random((Q, C)) < 3.0 / C if C > 20 else rng.random((Q, C)) < 0.3).astype(np.int8)
    return qb, db, ql, dl


def _load_codes(ctx, qb, db, ql, dl):
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), db.shape[1], dl.shape[1])
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))


def _hamming_ref(qb, db, ql, dl, R):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, im, idx, dist = O.map_from_codes(qb, db, ql, dl, R)
    return ap, im, idx, dist


@pytest.mark.parametrize("lw,C", CLASSES, ids=lambda v: str(v))
@pytest.mark.parametrize("nw,b", WORDS, ids=lambda v: str(v))
def test_exact_sequence_and_side_histograms_on_every_word_count(nw, b, lw, C):
    """Q = 40, N = 1000: the exact two-pass sequence on the vector ALU at R = 100 (k_select<NW, LW, false>) and in the dense regime
    R = N / 2 (k_select_dense<NW, LW>), the vector-ALU histogram (k_hist<NW>), the relevant-row histogram (k_hist_rel<NW, LW>) and the distance-by-grade table
    (k_hist_joint<NW, LW>)."""
    Q, N = 40, 1000
    qb, db, ql, dl = _codes(1000 * nw + C, Q, N, b, C)
    ctx = _native.Context(0)
    try:
        ctx.set_option("select_mfma", 0)
        ctx.set_option("rank_dense", 0)                    # (the byte matrix would take R = N / 2 off the record pass)
        _load_codes(ctx, qb, db, ql, dl)
        for R, variant in ((100, SEL_VALU), (N // 2, SEL_DENSE)):
            ap_ref, im_ref, idx_ref, dist_ref = _hamming_ref(qb, db, ql, dl, R)
            ctx.topr(R)
            assert ctx.get_stat("select_variant") == variant and ctx.get_stat("last_optimistic") == 0, (R, ctx.get_stat("select_variant"))
            idx, dist = ctx.get_topr()
            assert np.array_equal(idx, idx_ref) and np.array_equal(dist, dist_ref), R
            assert np.array_equal(ctx.get_match().astype(bool), im_ref), R
            ap, rel = ctx.map(R)
            assert np.array_equal(ap, ap_ref, equal_nan=True) and np.array_equal(rel, im_ref.sum(1)), R
        ref_all, ref_rel = brute_refs.rel_hist(qb, db, ql, dl)
        ctx.rel_hist()
        a, r = ctx.get_rel_hist()
        assert ctx.get_stat("rel_hist_variant") == 1
        assert np.array_equal(a, ref_all) and np.array_equal(r, ref_rel)
        ctx.set_option("hist_mfma", 0)                     # the vector-ALU histogram pass, k_hist<NW>
        ctx.hist()
        assert ctx.get_stat("hist_variant") == 1
        assert np.array_equal(ctx.get_hist(), ref_all)
        G = brute_refs.defined_G(ql, dl)
        ctx.joint_hist()
        assert ctx.get_stat("joint_hist_grades") == G
        assert np.array_equal(ctx.get_joint_hist(), brute_refs.joint_hist(qb, db, ql, dl, G))
    finally:
        ctx.close()


@pytest.mark.parametrize("lw,C", CLASSES, ids=lambda v: str(v))
@pytest.mark.parametrize("nw,b", WORDS, ids=lambda v: str(v))
def test_the_bet_on_every_word_count_through_the_vector_and_the_one_distance_matrix_select(nw, b, lw, C):
    """Q = 20, N = 66000, R = 1000 (the bet needs N >= 65536, R <= N / 8): k_select<NW, LW, true> (select_mfma = 0) and k_select_mx<NW, LW,
    QT, COMPACT> (select_packed = 1) with eight-byte records (hg_topr: the lists are wanted) and one-byte records (hg_map, <= 128 classes)."""
    Q, N, R = 20, 66000, 1000
    qb, db, ql, dl = _codes(2000 * nw + C, Q, N, b, C)
    ap_ref, im_ref, idx_ref, dist_ref = _hamming_ref(qb, db, ql, dl, R)
    ctx = _native.Context(0)
    try:
        _load_codes(ctx, qb, db, ql, dl)
        for mfma, variant in ((0, SEL_VALU), (1, SEL_MX)):
            ctx.set_option("select_mfma", mfma)
            ctx.set_option("select_packed", 1)
            ctx.set_option("optimistic", 1)
            ap, rel = ctx.map(R)
            assert ctx.get_stat("last_optimistic") == 1 and ctx.get_stat("select_variant") == variant, (mfma, ctx.get_stat("select_variant"))
            assert np.array_equal(ap, ap_ref, equal_nan=True) and np.array_equal(rel, im_ref.sum(1)), mfma
            ctx.topr(R)
            assert ctx.get_stat("last_optimistic") == 1 and ctx.get_stat("select_variant") == variant, (mfma, ctx.get_stat("select_variant"))
            idx, dist = ctx.get_topr()
            assert np.array_equal(idx, idx_ref) and np.array_equal(dist, dist_ref), mfma
            assert np.array_equal(ctx.get_match().astype(bool), im_ref), mfma
    finally:
        ctx.close()


# ---- 3. the real-valued call's other kernels templated on the padded feature count KP (16 ... 128): the sample that leaves float32
# scores (k_real_sample_h<KP, HALF, OUT16 = false>: more than 16384 sampled rows, k_real_guess instead of k_real_guess_lds), the float32
# matrix-core passes (real_mfma = 1: k_real_sample_mx<KP>, k_real_select_mx<KP>) and the vector-ALU passes (real_mfma = 0:
# k_real_sample<KP / 2>, k_real_select<KP / 2, 1>)
RG_MMAX, REAL_SAMPLE_HITS, REAL_SECOND_SAMPLE, REAL_FIRST_HITS_BRACKET, REAL_FIRST_SIGMA = 16384, 64, 4, 24, 5.0     # hg_real_bf.hpp, hg_real.hip


def place_cut_sample(N, R, sigma=REAL_FIRST_SIGMA):
    """place_cut's sample of a first attempt with the default options on up to 128 features (the 16-bit sample applies), restated:
    the strides, the sampled rows M, whether the second, counting sample follows, and the rows a query is expected to keep."""
    stride2 = int(R / (REAL_SAMPLE_HITS * REAL_SECOND_SAMPLE))
    stride = int(R / REAL_FIRST_HITS_BRACKET)
    second = stride2 >= 1 and stride >= 2 * stride2 and -(-N // max(stride, 1)) <= RG_MMAX
    if not second:
        stride = int(R / REAL_SAMPLE_HITS)
    stride = max(stride, 1)
    M = -(-N // stride)
    expect = R * (1.0 + sigma / REAL_SAMPLE_HITS ** 0.5)
    if second:
        fr2 = R * (-(-N // stride2)) / N
        expect = R * (1.0 + sigma / max(fr2, 1.0) ** 0.5)
    return dict(stride=stride, stride2=stride2, M=M, second=second, expect=expect)


def _narrow_cases():
    return [pytest.param(kind, b, id="%s-b%d" % (kind, b)) for kind, b in (p.values for p in _width_cases()) if b <= 128]


@pytest.mark.parametrize("kind,b", _narrow_cases())
def test_a_sample_beyond_the_lds_guess_on_every_filter_width(kind, b):
    """N = 66000, R = 200: every third row is sampled (R / 64 = 3), 22000 rows -- more than k_real_guess_lds holds, so the sample's scores
    leave as float32 and k_real_guess places the cut; no second sample (R / 256 = 0).  The oracle's lists and APs."""
    dbf, qf, dl, ql = _tables(kind)
    Q, R = 20, 200
    dbf, qf = np.ascontiguousarray(dbf[:, :b]), np.ascontiguousarray(qf[:Q, :b])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap_ref, idx_ref, score_ref, _ = ranked_oracle(qf, dbf, ql[:Q], dl, R)
    ctx = _native.Context(0)
    try:
        assert ctx.set_database_f32(dbf, dl.astype(np.int64))[1] == 0
        assert ctx.set_queries_f32(qf, ql[:Q].astype(np.int64))[1] == 0
        cut = place_cut_sample(FAR_N, R)
        assert cut["M"] > RG_MMAX and not cut["second"] and cut["stride"] == 3, cut      # the premise: float32 sample scores, k_real_guess, one sample
        idx, score = ctx.topr_real(R)
        path = ctx.get_stat("real_path")
        assert path & 1 and ((path >> 3) & 1) == (1 if kind == "half" else 0), path
        assert ctx.get_stat("real_attempts") == 1
        assert np.array_equal(score.view(np.uint32), score_ref.view(np.uint32)) and np.array_equal(idx, idx_ref)
        ap, _ = ctx.map_real(R)
        assert np.array_equal(ap, ap_ref, equal_nan=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("kind,b", [p for p in _narrow_cases() if p.values[0] == "half"])
def test_the_exact_pair_passes_on_every_feature_width(kind, b, mode):
    """The bet of the FAR cases (N = 66000, R = 1500, Q = 20) without the filter: every pair on the float32 matrix-core instruction
    (real_mfma = 1) and on the vector ALU (0)."""
    c = far_case(kind, b)
    Q = 20
    ctx = _native.Context(0)
    try:
        ctx.set_option("real_mfma", mode)
        assert ctx.set_database_f32(c.dbf, c.dl)[1] == 0
        assert ctx.set_queries_f32(c.qf[:Q], c.ql[:Q])[1] == 0
        idx, score = ctx.topr_real(FAR_R)
        assert (ctx.get_stat("real_path") & 1) == 0 and ctx.get_stat("real_attempts") == 1
        assert np.array_equal(score.view(np.uint32), c.score[:Q].view(np.uint32)) and np.array_equal(idx, c.idx[:Q])
        ap, _ = ctx.map_real(FAR_R)
        assert np.array_equal(ap, c.ap[:Q], equal_nan=True)
    finally:
        ctx.close()


# ---- 4. the rescore kernels' slices per wavefront (rescore_slices_per_wave: a heuristic on the rows a slice is expected to keep).  Over
# its whole domain it returns 8, 6, 2 or 1, never 3 or 4 (tests/test_kernel_coverage_host.py restates it): 6 and 8 alternate below 64 rows per slice, 2
# from 64, 1 from 1064 -- slices of 8192 rows (16 features, few segments) at R = N / 8.
# max_segments = 3 leaves the plain geometry with three segments, so the real-valued geometry's own cut decides: segments of
# 512 KB of float rows, S = ceil(N / L) -- 9 at 16 features, 33 at 64, 65 at 128.  The slice count each case must get is worked out
# here, on the host, from the restated heuristic and place_cut's expectation; the test checks S through the `segments` stat.
SLICE_CASES = [(16, 8250), (16, 4000), (64, 4000), (64, 1500), (64, 900), (128, 4000), (128, 2000)]       # (b, R) at N = 66000


def real_segments(N, b):
    bp = (b + 15) // 16 * 16
    L = max(64, 512 * 1024 // (bp * 4) // 16 * 16)
    return -(-N // L)


def expected_slices(N, b, R):
    return rescore_slices_per_wave(1.03 * place_cut_sample(N, R)["expect"] / real_segments(N, b))


@pytest.mark.parametrize("source", ["real", "asym", "pq"])
@pytest.mark.parametrize("b,R", SLICE_CASES, ids=lambda v: str(v))
def test_rescore_slice_counts_on_the_three_row_sources(b, R, source):
    max_segments = 3
    dbf, qf, dl, ql = _tables("half")
    Q = 20
    dbf, qf = np.ascontiguousarray(dbf[:, :b]), np.ascontiguousarray(qf[:Q, :b])
    dl64, ql64 = dl.astype(np.int64), ql[:Q].astype(np.int64)
    ctx = _native.Context(0)
    try:
        if max_segments:
            ctx.set_option("max_segments", max_segments)
        if source == "real":
            x = dbf
            assert ctx.set_database_f32(dbf, dl64)[1] == 0
            rank, score_map = ctx.topr_real, ctx.map_real
        elif source == "asym":
            x = np.where(dbf > 0, 1, -1).astype(np.float32)
            ctx.set_option("keep_floats", 0)
            ctx.set_option("keep_query_floats", 1)
            assert ctx.set_database_f32(dbf, dl64)[1] == 0
            rank, score_map = ctx.topr_asym, ctx.map_asym
        else:
            dsub = 4 if b == 16 else 8
            M = b // dsub
            rng = np.random.default_rng(b + R)
            books = np.stack([dbf[rng.choice(FAR_N, 64, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
            codes = pq.encode(dbf, books)
            x = pq.decode(codes, books)
            ctx.set_option("keep_query_floats", 1)
            assert ctx.set_database_pq(codes, books, dl64)[1] == 0
            rank, score_map = ctx.topr_pq, ctx.map_pq
        assert ctx.set_queries_f32(qf, ql64)[1] == 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ap_ref, idx_ref, score_ref, _ = ranked_oracle(qf, x, ql[:Q], dl, R)
        idx, score = rank(R)
        assert ctx.get_stat("real_path") & 1, "not the filter path"
        # the premises of expected_slices: the first attempt held (sigma 5, the sample's own expectation) on the geometry it assumes
        assert ctx.get_stat("real_attempts") == 1 and ctx.get_stat("segments") == real_segments(FAR_N, b), ctx.get_stat("segments")
        assert np.array_equal(score.view(np.uint32), score_ref.view(np.uint32)) and np.array_equal(idx, idx_ref)
        ap, _ = score_map(R)
        assert np.array_equal(ap, ap_ref, equal_nan=True)
    finally:
        ctx.close()

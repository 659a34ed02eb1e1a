"""Label-free relevance on the GPU (needs an MI355X): neighbour sets (hg_set_neighbours, hg_neighbours_from_lists), the match bitmap
from them (hg_match_neighbours) with everything downstream of it, and the neighbour distance histogram (hg_nbr_hist), against the NumPy
statement in tests/neighbour_oracle.py.  Every comparison is == on integers or on the bits of a float64."""
import functools
import types
import warnings

import numpy as np
import pytest

from oracle import hamming_map as H
from oracle import real_map as RM
from tests import cases
from tests import neighbour_oracle as NO
from tests import rerank_oracle as RO
from hashgan_amd import _native, metric, synth
from hashgan_amd import neighbours as NB
from hashgan_amd.devarray import DeviceOut

pytestmark = pytest.mark.gpu

ARG, STATE = _native.HG_ERR_ARG, _native.HG_ERR_STATE
PAD = NO.PAD
Q, N, B, R, C = 37, 3000, 32, 300, 10                    # the base shape: Qpad = 64 != Q, five words of the bitmap, the last one ragged
KS = (1, 7, 64, 300)


def raises(code, fn, *args, **kw):
    with pytest.raises(_native.HashganNativeError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def frozen(**kw):
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return types.SimpleNamespace(**kw)


@functools.lru_cache(maxsize=None)
def codes(Q=Q, N=N, b=B, R=R, seed=0xA5):
    """Planted codes, one-hot labels and the oracle's canonical lists -- computed once, never modified."""
    dl, _ = synth.onehot_labels(seed * 3 + 1, N, C)
    ql, _ = synth.onehot_labels(seed * 3 + 2, Q, C)
    db = synth.planted_codes(seed, dl, b, 0.25)
    qb = synth.planted_codes(seed, ql, b, 0.25) ^ (synth.random_bits(seed + 17, Q, b) & synth.random_bits(seed + 18, Q, b))
    idx, _ = H.topr_from_codes(qb, db, R)
    label_match = (dl[idx].astype(bool) & ql[:, None, :].astype(bool)).any(-1).astype(np.uint8)
    return frozen(Q=Q, N=N, b=b, R=R, qb=qb, db=db, ql=ql, dl=dl, idx=idx, label_match=label_match)


def code_ctx(c, rows=None, **kw):
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(c.db), metric.pack_labels(c.dl), c.b, C, **kw)
    sel = slice(None) if rows is None else rows
    ctx.set_queries(metric.pack_codes(c.qb[sel]), metric.pack_labels(c.ql[sel]))
    return ctx


@functools.lru_cache(maxsize=None)
def sets_for(G):
    """The G sweep's ground truth on the base lists: query 0 has no neighbours, query 1 holds rows 0 and N - 1 (G = 1: query 1 row 0,
    query 2 row N - 1), query 3's whole set lies outside its top R."""
    c = codes()
    gt = NO.random_sets(np.random.default_rng(G), c.idx, N, G, empty=(0,), outside=(3,))
    if G == 1:
        gt[1, 0], gt[2, 0] = 0, N - 1
    else:
        row = np.setdiff1d(NO.members(gt[1]), (0, N - 1))[:G - 2]
        gt[1] = PAD
        gt[1, :row.size + 2] = np.concatenate([(N - 1, 0), row])
    gt.flags.writeable = False
    return gt


def assert_matches_oracle(ctx, idx, gt, ks, what=""):
    """After ctx.match_neighbours(): bits, AP, hits and the cut-off tables against the oracle on the lists idx."""
    want = NO.match_bits(idx, gt)
    assert ctx.get_stat("match_source") == 1, what
    assert np.array_equal(ctx.get_match(), want), what
    ctx.ap()
    ap, rel = ctx.get_ap()
    oap, orel = NO.ap_rows(want)
    assert bits(ap) == bits(oap) and np.array_equal(rel, orel), what
    ctx.ap_at(ks)
    ap_k, hits_k = ctx.get_ap_at()
    oap_k, ohits_k = NO.ap_at(want, ks)
    assert bits(ap_k) == bits(oap_k) and np.array_equal(hits_k, ohits_k), what
    return want, ap_k, hits_k


# ------------------------------------------------------------------ 1. the sets, the bits and what is read from them
@pytest.mark.parametrize("G", (1, 5, 64, 65, 1000))
def test_g_sweep(G):
    c, gt = codes(), sets_for(G)
    ctx = code_ctx(c)
    try:
        ctx.set_neighbours(gt)
        ids, cnt = ctx.get_neighbours()
        oids, ocnt = NO.sorted_table(gt)
        assert np.array_equal(ids, oids) and np.array_equal(cnt, ocnt)
        assert cnt[0] == 0 and (G == 1 or {0, N - 1} <= set(ids[1].tolist()))
        ctx.topr(R)
        assert ctx.get_stat("match_source") == 0
        ctx.match_neighbours()
        want, ap_k, hits_k = assert_matches_oracle(ctx, c.idx, gt, KS)
        ap, rel = ctx.get_ap()
        assert np.isnan(ap[0]) and rel[0] == 0                              # no neighbours: AP NaN
        assert want[3].sum() == 0 and np.isnan(ap[3]) and rel[3] == 0       # every neighbour outside the top R: no hit
        # mean recall leaves the query without neighbours out
        recall = NB.recall_from_tables(hits_k, cnt)
        ok = ocnt > 0
        assert not ok[0] and np.array_equal(recall, (hits_k[ok] / ocnt[ok, None].astype(np.int64)).mean(0))
    finally:
        ctx.close()


@pytest.mark.parametrize("R_", (1, 63, 64, 65))
def test_r_edges_leave_the_pad_bits_zero(R_):
    c = codes()
    rng = np.random.default_rng(R_)
    idx = c.idx[:, :R_]
    gt = NO.random_sets(rng, idx, N, 5)
    gt[:, 0] = idx[:, R_ - 1]                                                # the last rank of every query is a neighbour
    for q in range(Q):                                                       # (and nowhere else in its row)
        gt[q, 1:][gt[q, 1:] == gt[q, 0]] = PAD
    ctx = code_ctx(c)
    try:
        ctx.set_neighbours(gt)
        ctx.topr(R_)
        ctx.match_neighbours()
        ptr, nbytes = ctx.match_buffer()
        RW = (R_ + 63) // 64
        assert nbytes == Q * RW * 8
        words = np.empty((Q, RW), np.uint64)
        ctx.memcpy_dtoh(words, ptr, nbytes)
        want = NO.bitmap_words(NO.match_bits(idx, gt))
        assert np.array_equal(words, want)
        assert ((words[:, -1] >> np.uint64((R_ - 1) % 64)) == 1).all()      # the last rank's bit is the highest one set
    finally:
        ctx.close()


def test_largest_set():
    Q_, N_, R_, G = 3, 40000, 4096, 16384
    rng = np.random.default_rng(16384)
    db, qb = synth.random_bits(11, N_, B), synth.random_bits(12, Q_, B)
    dl, ql = np.ones((N_, 1), np.int8), np.ones((Q_, 1), np.int8)
    idx, _ = H.topr_from_codes(qb, db, R_)
    gt = np.full((Q_, G), PAD, np.uint32)
    gt[0] = rng.choice(N_, G, replace=False)                                 # a full set in random order
    gt[1, rng.permutation(G)[:9000]] = rng.choice(N_, 9000, replace=False)   # a ragged one, pads in between
    gt[2] = np.concatenate([idx[2][::-1], rng.choice(np.setdiff1d(np.arange(N_), idx[2]), G - R_, replace=False)])   # the whole list
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), B, 1)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        ctx.set_neighbours(gt)
        ids, cnt = ctx.get_neighbours()
        oids, ocnt = NO.sorted_table(gt)
        assert np.array_equal(ids, oids) and np.array_equal(cnt, ocnt) and cnt.tolist() == [G, 9000, G]
        ctx.topr(R_)
        ctx.match_neighbours()
        want, _, _ = assert_matches_oracle(ctx, idx, gt, (1, 100, 4096))
        assert want[2].all()
        ctx.nbr_hist()
        nbr, cnt2 = ctx.get_nbr_hist()
        assert np.array_equal(nbr, NO.nbr_hist(qb, db, gt)) and np.array_equal(cnt2, ocnt)
    finally:
        ctx.close()


@pytest.mark.parametrize("b", (1, 33, 64, 65, 128, 255))
def test_nbr_hist_wide_codes(b):
    G = 65
    rng = np.random.default_rng(b)
    db, qb = synth.random_bits(b * 7 + 1, N, b), synth.random_bits(b * 7 + 2, Q, b)
    db[5] = qb[2]; db[6] = 1 - qb[2]                                        # distance 0 and distance b occur
    dl, ql = np.ones((N, 1), np.int8), np.ones((Q, 1), np.int8)
    gt = NO.random_sets(rng, np.tile(np.arange(100), (Q, 1)), N, G, empty=(0,))
    gt[2] = PAD
    gt[2, :2] = (6, 5)
    want = NO.nbr_hist(qb, db, gt)
    assert want[0, 2] == 1 and want[b, 2] == 1 and want[:, 0].sum() == 0
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, 1)
        ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
        ctx.set_neighbours(gt)
        ctx.nbr_hist()
        nbr, cnt = ctx.get_nbr_hist()
        assert nbr.shape == (b + 1, Q)
        assert np.array_equal(nbr, want) and np.array_equal(cnt, NO.sorted_table(gt)[1])
        assert np.array_equal(nbr.sum(0), cnt)
        # the order of a set plays no part
        ctx.set_neighbours(np.ascontiguousarray(gt[:, ::-1]))
        raises(STATE, ctx.get_nbr_hist)                                      # (a new set ends the table of the earlier one)
        ctx.nbr_hist()
        assert bits(ctx.get_nbr_hist()[0]) == bits(nbr)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. self-checks that need no oracle
def test_sets_captured_from_the_lists():
    c = codes()
    ctx = code_ctx(c)
    try:
        for G in (70, R):
            ctx.topr(R)
            idx, _ = ctx.get_topr()
            ctx.neighbours_from_lists(G)
            assert bits(ctx.get_topr()[0]) == bits(idx)                      # the lists are only read
            ctx.match_neighbours()
            m = ctx.get_match()
            assert m[:, :G].all() and not m[:, G:].any()
            table, cnt = ctx.get_neighbours()
            words = ctx.get_match()
            assert (cnt == G).all()
            # the same sets through the host
            ctx.set_neighbours(idx[:, :G])
            t2, c2 = ctx.get_neighbours()
            assert bits(t2) == bits(table) and bits(c2) == bits(cnt)
            ctx.topr(R)
            ctx.match_neighbours()
            assert bits(ctx.get_match()) == bits(words)
        raises(ARG, ctx.neighbours_from_lists, R + 1)                        # G <= R
        raises(ARG, ctx.neighbours_from_lists, 0)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def feats(Q_=Q, N_=N, b=B, seed=5):
    """Real-valued features (tanh of class prototypes + noise, a few duplicated rows) and labels."""
    qf, dbf, ql, dl = RO.generate(Q_, N_, b, C, seed=seed)
    return frozen(Q=Q_, N=N_, b=b, qf=qf, dbf=dbf, ql=ql, dl=dl, pm1=np.where(dbf > 0, 1, -1).astype(np.float32))


def float_ctx(f):
    """Both float tables and the sign() codes on one context: every ranking runs on it."""
    ctx = _native.Context(0)
    ctx.set_option("keep_floats", 1)
    ctx.set_option("keep_query_floats", 1)
    assert ctx.set_database_f32(f.dbf, f.dl)[1] == 0
    assert ctx.set_queries_f32(f.qf, f.ql)[1] == 0
    return ctx


def test_recall_of_the_real_valued_ranking_against_its_own_lists_is_one():
    f, G = feats(), 100
    ctx = float_ctx(f)
    try:
        ctx.topr_real(G, download=False)
        ctx.neighbours_from_lists(G)
        ctx.topr_real(R, download=False)
        ctx.match_neighbours()
        ctx.ap_at((G, R))
        _, hits = ctx.get_ap_at()
        cnt = ctx.get_neighbours(ids=False)[1]
        assert (cnt == G).all() and (hits == G).all()
        assert np.array_equal(NB.recall_from_tables(hits, cnt), np.ones(2))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. every list source
def oracle_lists(f, source, R_):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if source == "topr_real":
            return RM.map_from_features(f.qf, f.dbf, f.ql, f.dl, R_)[2]
        if source == "topr_asym":
            return RM.map_from_features(f.qf, f.pm1, f.ql, f.dl, R_)[2]
        if source == "topr_rerank":
            return RO.rerank(f.qf, f.dbf, f.ql, f.dl, R_)["idx"]
    return H.topr_from_codes((f.qf > 0).astype(np.uint8), (f.dbf > 0).astype(np.uint8), R_)[0]


def staged(ctx, R_):
    ctx.hist()
    ctx.plan(R_)
    ctx.select()


SOURCES = {"topr": lambda ctx, R_: ctx.topr(R_), "staged": staged,
           "topr_real": lambda ctx, R_: ctx.topr_real(R_, download=False),
           "topr_asym": lambda ctx, R_: ctx.topr_asym(R_, download=False),
           "topr_rerank": lambda ctx, R_: ctx.topr_rerank(R_, download=False)}


@pytest.mark.parametrize("source", list(SOURCES))
def test_every_list_source(source):
    f = feats()
    idx = oracle_lists(f, source, R)
    gt = NO.random_sets(np.random.default_rng(len(source)), idx, N, 64, empty=(4,))
    ctx = float_ctx(f)
    try:
        ctx.set_neighbours(gt)
        SOURCES[source](ctx, R)
        ctx.match_neighbours()                                               # (N < 65536: the real-valued rankings take no bet here)
        assert_matches_oracle(ctx, idx, gt, KS, source)
    finally:
        ctx.close()


def test_asymmetric_lists_of_a_bet():
    f = feats(8, 66000, 64, seed=9)
    R_ = 500
    idx = oracle_lists(f, "topr_asym", R_)
    gt = NO.random_sets(np.random.default_rng(66), idx, f.N, 65, empty=(1,))
    ctx = float_ctx(f)
    try:
        ctx.set_neighbours(gt)
        ctx.topr_asym(R_, download=False)
        assert f.N >= 65536 and R_ * 8 <= f.N and ctx.get_stat("real_attempts") == 1     # the ladder's first attempt, a bet, held
        ctx.match_neighbours()
        assert_matches_oracle(ctx, idx, gt, (1, 64, 65, 500))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. downstream
class Arena:
    """Device memory without a framework: one scratch allocation of a context of its own, carved into 256-byte aligned pieces."""

    def __init__(self, nbytes):
        self.ctx = _native.Context(0)
        self.cap, self.top = int(nbytes), 0
        self.base = self.ctx.scratch(0, self.cap)

    def out(self, shape, dtype):
        off = self.top
        self.top = (off + int(np.prod(shape)) * np.dtype(dtype).itemsize + 255) // 256 * 256
        assert self.top <= self.cap
        return DeviceOut(self.base + off, shape, None, dtype)

    def get(self, d):
        host = np.empty(d.shape, dtype=d.dtype)
        self.ctx.memcpy_dtoh(host, d.ptr, host.nbytes)
        return host

    def close(self):
        self.ctx.close()


def test_downstream_of_a_neighbour_match():
    c, gt = codes(), sets_for(64)
    ctx, arena = code_ctx(c), Arena(1 << 20)
    try:
        ctx.set_neighbours(gt)
        ctx.topr(R)
        ctx.ap_at(KS)                                                        # on the label bits
        assert np.array_equal(ctx.get_ap_at()[1][:, -1], c.label_match.sum(1))
        ctx.match_neighbours()
        raises(STATE, ctx.get_ap_at)                                         # the bitmap it walked is gone
        ctx.match()                                                          # hg_match sees the match stage set and returns
        assert ctx.get_stat("match_source") == 1
        ctx.ap()
        dm, da, dh = arena.out((Q, R), "uint8"), arena.out((Q, 1), "float64"), arena.out((Q, 1), "int64")
        ctx.export([("match", dm), ("ap", da), ("hits", dh)])
        ctx.synchronize()
        ap, rel = ctx.get_ap()
        want = NO.match_bits(c.idx, gt)
        assert np.array_equal(arena.get(dm), ctx.get_match()) and np.array_equal(arena.get(dm), want)
        assert bits(arena.get(da)[:, 0]) == bits(ap) and np.array_equal(arena.get(dh)[:, 0], rel)
        # a new ranking brings the label bits back
        ctx.topr(R)
        assert ctx.get_stat("match_source") == 0
        assert np.array_equal(ctx.get_match(), c.label_match)
        ids, _ = ctx.get_neighbours()                                        # ... and leaves the sets
        assert np.array_equal(ids, NO.sorted_table(gt)[0])
    finally:
        ctx.close()
        arena.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_earlier_state():
    c, gt = codes(), sets_for(5)
    ctx = code_ctx(c)
    try:
        raises(STATE, ctx.match_neighbours)                                  # no set, no lists
        ctx.topr(R)
        raises(STATE, ctx.match_neighbours)                                  # no set
        raises(STATE, ctx.nbr_hist)
        raises(STATE, ctx.get_neighbours)
        ctx.set_neighbours(gt)
        ctx.match_neighbours()
        ctx.ap_at(KS)
        ctx.nbr_hist()

        def state():
            return bits(ctx.get_match()), bits(ctx.get_ap_at()[0]), bits(ctx.get_ap_at()[1]), ctx.get_stat("match_source")

        before, nbr = state(), bits(ctx.get_nbr_hist()[0])
        dup = gt.copy(); dup[7, :2] = 11
        far = gt.copy(); far[9, 3] = N
        for bad in (dup, far, gt[:-1], np.zeros((Q, 0), np.uint32), np.zeros((Q, 16385), np.uint32)):
            raises(ARG, ctx.set_neighbours, bad)
            assert state() == before                                         # bitmap, cut-off tables and their source as they were
            raises(STATE, ctx.get_neighbours)                                # a refused call leaves no set
            raises(STATE, ctx.match_neighbours)
            raises(STATE, ctx.get_nbr_hist)
            assert state() == before
            ctx.set_neighbours(gt)
            ctx.nbr_hist()
            assert bits(ctx.get_nbr_hist()[0]) == nbr
        # hg_map writes no lists
        ap, rel = ctx.map(R)
        raises(STATE, ctx.match_neighbours)
        assert ctx.get_stat("match_source") == 0 and np.array_equal(ctx.get_ap()[1], c.label_match.sum(1))
        # reloads and hg_trim end the set
        def queries():
            ctx.set_queries(metric.pack_codes(c.qb), metric.pack_labels(c.ql))

        def database():                                                      # (the queries are set again after a database)
            ctx.set_database(metric.pack_codes(c.db), metric.pack_labels(c.dl), B, C)
            raises(STATE, ctx.get_neighbours)
            queries()

        for event in (queries, database, ctx.trim):
            ctx.set_neighbours(gt)
            ctx.nbr_hist()
            event()
            raises(STATE, ctx.get_neighbours)
            raises(STATE, ctx.get_nbr_hist)
            raises(STATE, ctx.nbr_hist)
            ctx.topr(R)
            raises(STATE, ctx.match_neighbours)
            assert np.array_equal(ctx.get_match(), c.label_match)
    finally:
        ctx.close()


def test_a_shard_context_is_refused():
    c, gt = codes(), sets_for(5)
    ctx = code_ctx(c, idx_base=0, n_total=2 * N)
    try:
        raises(STATE, ctx.set_neighbours, gt)
        ctx.hist(); ctx.plan(R); ctx.select()
        raises(STATE, ctx.neighbours_from_lists, 5)
        raises(STATE, ctx.match_neighbours)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. determinism
def test_same_words_twice_and_for_a_query_alone():
    c, gt = codes(), sets_for(65)
    ctx = code_ctx(c)
    one = code_ctx(c, rows=slice(5, 6))
    try:
        runs = []
        for _ in range(2):
            ctx.set_neighbours(gt)
            ctx.topr(R)
            ctx.match_neighbours()
            ctx.nbr_hist()
            ptr, nbytes = ctx.match_buffer()
            words = np.empty(nbytes // 8, np.uint64)
            ctx.memcpy_dtoh(words, ptr, nbytes)
            runs.append((bits(words), bits(ctx.get_neighbours()[0]), bits(ctx.get_nbr_hist()[0])))
        assert runs[0] == runs[1]
        one.set_neighbours(gt[5:6])
        one.topr(R)
        one.match_neighbours()
        one.nbr_hist()
        assert np.array_equal(one.get_match()[0], ctx.get_match()[5])
        assert np.array_equal(one.get_nbr_hist()[0][:, 0], ctx.get_nbr_hist()[0][:, 5])
    finally:
        ctx.close()
        one.close()


# ------------------------------------------------------------------ 7. the blind step's licence
def test_first_reservations_keep_the_licence_to_enqueue_blind(case_cache):
    """The first hg_set_neighbours and hg_nbr_hist on a context allocate their buffers; none of them is one a blind step touches, so
    the hg_map_begin after them is still enqueued blind (tests/test_side_results_gpu.py's pattern)."""
    c = case_cache("c2_q64")
    g = cases.load_golden("c2_q64")
    R_ = c["R"]
    Q_ = c["qbits"].shape[0]
    gt = np.tile(np.arange(9, dtype=np.uint32), (Q_, 1))
    ctx = _native.Context(0)
    try:
        ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
        ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
        ap, _ = ctx.map(R_)
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert ctx.get_stat("last_optimistic") == 1
        n0 = ctx.get_stat("map_async_steps")
        ctx.set_neighbours(gt)
        ctx.nbr_hist()
        ctx.map_begin(R_)
        assert ctx.get_stat("map_async_steps") == n0 + 1, "the first reservations ended the licence to enqueue blind"
        ctx.nbr_hist()                                                       # beside a step in flight
        nbr, cnt = ctx.get_nbr_hist()
        ap, _ = ctx.map_end()
        assert np.array_equal(ap, g["ap"], equal_nan=True)
        assert ctx.get_stat("map_async_redone") == 0
        assert np.array_equal(nbr, NO.nbr_hist(c["qbits"], c["dbbits"][:9], gt)) and (cnt == 9).all()     # (the sets hold rows 0..8)
    finally:
        ctx.close()


def test_every_buffer_is_on_the_contexts_list():
    c, gt = codes(), sets_for(64)
    ctx = code_ctx(c)
    try:
        ctx.trim()
        bytes0 = ctx.get_stat("device_bytes")
        ctx.set_neighbours(gt)
        ctx.nbr_hist()
        assert ctx.get_stat("device_bytes") > bytes0
        ctx.trim()
        assert ctx.get_stat("device_bytes") == bytes0
        ctx.timing_enable(True)                                              # a timing slot each
        ctx.set_neighbours(gt)
        ctx.topr(R)
        ctx.match_neighbours()
        ctx.nbr_hist()
        t = ctx.timing_read()
        for name in ("k_nbr_sort", "k_nbr_match", "k_nbr_hist"):
            assert t[name][1] == 1, name
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. the public surface
@functools.lru_cache(maxsize=None)
def grid_case():
    """Features on the 1/64 grid: float32 inner products are exact in any summation order."""
    Q_, N_, b = 21, 2000, 32
    qf, dbf = RM.quantised_features(0x51, Q_, b), RM.quantised_features(0x52, N_, b)
    qf[qf == 0] = 1 / 64; dbf[dbf == 0] = -1 / 64                            # (no zero: sign() is a clean bit)
    dbf[40] = dbf[41]
    ql, dl = np.zeros((Q_, 1), np.int64), np.zeros((N_, 1), np.int64)
    return frozen(Q=Q_, N=N_, b=b, qf=qf, dbf=dbf, ql=ql, dl=dl, pm1=np.where(dbf > 0, 1, -1).astype(np.float32))


def direct_metrics(idx, gt, ks):
    """recall, precision, the reference's mAP and the textbook's, computed straight from the lists."""
    m = NO.match_bits(idx, gt).astype(bool)
    n = np.array([NO.members(r).size for r in gt])
    out = {k: [] for k in ("map", "map_std")}
    hits = np.stack([m[:, :k].sum(1) for k in ks], 1)
    out["recall"] = (hits[n > 0] / n[n > 0, None]).mean(0)                   # (a mean over the rows of a [Q, nk] table: NumPy adds row by row)
    out["precision"] = (hits / np.array(ks)[None, :]).mean(0)
    for k in ks:
        ap, rel = NO.ap_rows(m, k)
        out["map"].append(H.mean_ap(ap[rel > 0]) if (rel > 0).any() else np.nan)
        px = np.cumsum(m[:, :k], 1) / np.arange(1, k + 1)
        std = (px * m[:, :k]).sum(1) / np.maximum(np.minimum(n, k), 1)
        out["map_std"].append(std[n > 0].mean())
    return {k: np.array(v) for k, v in out.items()}


MODE_SOURCE = {"hamming": "topr", "rerank": "topr_rerank", "asymmetric": "topr_asym", "features": "topr_real"}


def test_python_surface():
    f = grid_case()
    G, ks = 50, (1, 10, 50, 200)
    truth = oracle_lists(f, "topr_real", G)
    assert np.array_equal(NB.exact_neighbours(f.qf, f.dbf, G), truth)
    out = NB.binary_vs_float(f.qf, f.dbf, G, ks, modes=("hamming", "rerank", "asymmetric", "features"))
    for mode, source in MODE_SOURCE.items():
        idx = oracle_lists(f, source, ks[-1])
        want = direct_metrics(idx, truth, ks)
        m = NO.match_bits(idx, truth)
        oap, ohits = NO.ap_at(m, ks)
        q_in = (f.qf > 0).astype(np.uint8) if mode == "hamming" else f.qf
        d_in = (f.dbf > 0).astype(np.uint8) if mode == "hamming" else f.dbf
        single = NB.neighbour_metrics_at_k(q_in, d_in, truth, ks, mode=mode)
        for got in (out[mode], single):
            assert np.array_equal(got["per_query"]["hits"], ohits), mode
            assert bits(got["per_query"]["ap"]) == bits(oap), mode
            assert (got["per_query"]["count"] == G).all(), mode
            assert np.array_equal(got["recall"], want["recall"]), mode
            assert np.array_equal(got["precision"], want["precision"]), mode
            assert np.array_equal(got["map"], want["map"], equal_nan=True), mode
            # ap * hits / min(n_q, k) rounds three times per query where the direct sum / min(n_q, k) rounds once, and a mean of
            # non-negative terms adds log2(Q) roundings: well inside 16 ulp
            assert np.allclose(got["map_std"], want["map_std"], rtol=2.0 ** -48, atol=0), mode
    assert np.array_equal(out["features"]["recall"][2:], np.ones(2))        # the float ranking recovers its own top G
    # the radius curves: hg_nbr_hist against the definitions
    qb, db = (f.qf > 0).astype(np.uint8), (f.dbf > 0).astype(np.uint8)
    curves = NB.neighbour_radius_curves(qb, db, truth)
    nbr = NO.nbr_hist(qb, db, truth).T.astype(np.int64)
    d = H.hamming_matrix(H.pack_bits(qb), H.pack_bits(db))
    ball = np.stack([(d <= r).sum(1) for r in range(f.b + 1)], 1)
    assert np.array_equal(curves["hit"], np.cumsum(nbr, 1)) and np.array_equal(curves["ball"], ball)
    assert (curves["total_rel"] == G).all() and curves["recall"][-1] == 1.0

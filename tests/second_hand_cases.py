"""Second-hand memory: the shapes, inputs, host references and the family table of tests/test_second_hand_gpu.py (DESIGN.md section 10,
"Second-hand memory: what the suite pins").  Host only: nothing here touches a GPU; tests/test_second_hand_host.py proves what is
claimed about the shapes and the inputs.

A FAMILY is a group of entry points with one job (tests/test_second_hand_gpu.py: JOBS) that runs them all on one context and one host
reference.  A PAIR runs a larger job of a family only to dirty the buffers (the soil), then a smaller one whose results are checked (the
probe) -- and once the other way round, so that buffers grow again and the block cache hands back blocks larger than asked for.  The
references are the ones the per-feature files use: oracle/, tests/brute_refs.py, tests/tie_oracle.py, tests/rerank_oracle.py,
tests/pq_encode_oracle.py, tests/neighbour_oracle.py."""
import functools
import types
import warnings

import numpy as np

from oracle import hamming_map as H
from oracle import real_map as RM
from tests import brute_refs as B
from tests import neighbour_oracle as NO
from tests import pq_encode_oracle as PO
from tests import rerank_oracle as RO
from tests import tie_oracle as T
from hashgan_amd import extra_metrics as X
from hashgan_amd import pq

# ------------------------------------------------------------------ the shapes
# Every padded quantity shrinks across a padding boundary from BIG to SMALL (padding(): proved in tests/test_second_hand_host.py).
#   Q: 64-query tiles; b: Hamming code words (32- and 64-bit; k_select_mx4 takes 65..128 bits, k_select_mx3 up to 64); bf: float features,
#   padded to 16; C: 64-bit label words; N: never a multiple of 16 or of a segment; ks: the cut-off lists; G: the neighbour set size.
# The quantised family's feature count is M * dsub, so its small table has 3 * 7 = 21 features, not bf = 20: the nearest count to 20
# that three codebooks divide (bpad = 32 != b all the same).
BIG = dict(Q=130, b=100, bf=64, C=81, N=4097, R=900, ks=(1, 7, 64, 300, 900), M=8, K=256, dsub=8, G=50)
SMALL = dict(Q=33, b=33, bf=20, C=10, N=1000, R=50, ks=(1, 7, 50), M=3, K=16, dsub=7, G=7)
SHAPES = {
    "big": BIG, "small": SMALL,
    # the one-shot bet (N >= 65536, 8 R <= N)
    "bet_big": dict(BIG, N=90000), "bet_small": dict(SMALL, N=70001),
    # real-valued, every row a record (R = N: no cut) ...
    "nocut_big": dict(BIG, R=BIG["N"]), "nocut_small": dict(SMALL, R=SMALL["N"]),
    # ... and the filter path (sampled cut, 16-bit filter, exact rescoring).  Its reference is a float32 FMA chain emulated on the host
    # over Q x N x bf terms (14 s at Q = 33, N = 80000, bf = 64): this pair alone runs 12 and 9 queries, inside one 64-query tile -- every
    # other pair crosses that boundary -- so that both references stay within seconds.
    "filter_big": dict(BIG, Q=12, N=80000, R=2000), "filter_small": dict(SMALL, Q=9, N=66000, R=300),
}


def shape(name):
    return types.SimpleNamespace(name=name, **SHAPES[name])


def padding(s):
    """The padded sizes of a shape, by the rules of the loaders (hg_tables.hip)."""
    return dict(Qpad=(s.Q + 63) // 64 * 64, words32=(s.b + 31) // 32, words64=(s.b + 63) // 64, LW=(s.C + 63) // 64,
                bpad=(s.bf + 15) // 16 * 16, bpad_pq=(s.M * s.dsub + 15) // 16 * 16, bitmap_words=(s.R + 63) // 64, cutoffs=len(s.ks),
                pq_tables=(s.M, s.K), G=s.G)


# ------------------------------------------------------------------ the families
# name -> the public methods of _native.Context its job calls (tests/test_second_hand_gpu.py checks, through a recording proxy, that the
# job calls exactly these).  The completeness guard (tests/test_second_hand_host.py) places every public method either here or in EXCLUDED.
_LOAD = ("set_database", "set_queries")
_LOAD_F32 = ("set_database_f32", "set_queries_f32")
FAMILIES = {
    "hamming": _LOAD + ("map", "topr", "get_topr", "get_match", "hist", "plan", "select", "match", "ap", "get_ap", "map_begin", "map_end"),
    "lists": _LOAD + ("topr", "ap_at", "get_ap_at", "graded", "get_graded", "get_grades", "votes", "get_votes", "get_vote_pred",
                      "get_vote_confusion", "tie_ap", "get_tie_ap", "rel_hist", "get_rel_hist", "grade_hist", "get_grade_hist",
                      "joint_hist", "get_joint_hist"),
    "rerank": _LOAD_F32 + ("topr_rerank", "map_rerank", "get_topr", "get_rerank_scores", "get_match"),
    "real": _LOAD_F32 + ("topr_real", "map_real", "get_match"),
    "asym": _LOAD_F32 + ("topr_asym", "map_asym", "get_match"),
    "pq": ("set_database_pq", "set_queries_f32", "topr_pq", "map_pq", "get_match"),
    "pq_encode": ("pq_encode", "set_database_pq_f32", "set_queries_f32", "topr_pq", "get_match"),
    "neighbours": _LOAD + ("topr", "get_topr", "neighbours_from_lists", "get_neighbours", "match_neighbours", "get_match", "set_neighbours",
                           "ap", "get_ap", "nbr_hist", "get_nbr_hist"),
    "devmem": ("set_database_dev", "set_queries_dev", "topr", "topr_real", "match", "ap", "export"),
    "shard_step": _LOAD + ("shard_step",),
}
# Options a family's job sets before it loads anything (every job sets ALL of these keys, so that a context another family has used
# is back on known values)
OPTIONS = {"select_mfma": 1, "select_packed": 3, "keep_floats": 2, "keep_query_floats": 0}
FAMILY_OPTIONS = {"rerank": {"keep_floats": 1}, "real": {"keep_floats": 1}, "devmem": {"keep_floats": 1},
                  "asym": {"keep_floats": 0, "keep_query_floats": 1}, "pq": {"keep_query_floats": 1}, "pq_encode": {"keep_query_floats": 1}}
# the bet's three select kernels (tests/test_hip_random_shapes.py::test_random_bet_shapes): default rule, k_select_mx forced, vector ALU
BET_SELECTS = {"default": {}, "packed1": {"select_packed": 1}, "valu": {"select_mfma": 0, "select_packed": 1}}

_PLUMBING = "plumbing of the matrix itself (routes, guards, the producer arena of tests/dev_arena.py), not a result"
_GETTER = "getter of a buffer the matrix reads through another call"
_RCCL = "needs RCCL peers"
_STAGED = "a piece of the multi-rank staged sequences: walked by tests/test_sample_guess_gpu.py and tests/test_shard_*"
EXCLUDED = dict(
    {n: _PLUMBING for n in ("close", "trim", "get_stat", "set_option", "scratch", "memcpy_htod", "memcpy_dtoh", "memcpy_dtod", "synchronize")},
    **{n: _GETTER for n in ("get_packed", "get_hist", "hist_buffer", "match_buffer", "topr_buffers", "census", "get_merged_rel_hist",
                            "get_merged_grade_hist", "get_merged_joint_hist")},
    **{n: "tuning and timing: changes no result" for n in ("set_stream", "preload", "timing_enable", "timing_reset", "timing_read")},
    **{n: _RCCL for n in ("comm_init", "comm_destroy", "comm_info", "allgather", "alltoall", "allgather_topr", "allreduce_max", "barrier")},
    **{n: _STAGED for n in ("bet_eligible", "sample_hist", "guess", "select_candidates", "rank", "select_ranked", "merge_ranked", "merge_ap_part",
                            "unpack_parts", "pack_sample_by_owner", "guess_owned", "guess_finish", "pack_ranked_by_owner", "merge_ap_owned",
                            "bet_verdict", "merge_match", "merge_topr", "pack_side_table", "merge_side_table", "pack_list_table",
                            "merge_list_table")})

# ------------------------------------------------------------------ the matrix: (id, soil family, soil shape, probe family, probe shape, select)
def _pairs():
    out = []
    for fam, big, small in (("hamming", "big", "small"), ("lists", "big", "small"), ("rerank", "big", "small"), ("real", "nocut_big", "nocut_small"),
                            ("real", "filter_big", "filter_small"), ("asym", "big", "small"), ("pq", "big", "small"), ("pq_encode", "big", "small"),
                            ("neighbours", "big", "small"), ("devmem", "big", "small"), ("shard_step", "bet_big", "bet_small")):
        tag = fam + ("_filter" if big.startswith("filter") else "")
        out.append((tag, fam, big, fam, small, "default"))
        out.append((tag + "_reverse", fam, small, fam, big, "default"))
    for sel in BET_SELECTS:
        out.append(("hamming_bet_" + sel, "hamming", "bet_big", "hamming", "bet_small", sel))
    out.append(("hamming_bet_reverse", "hamming", "bet_small", "hamming", "bet_big", "default"))
    # family switches on one context, for the pairs that share buffers (out_idx, the record rows, the float tables)
    out.append(("switch_real_to_lists", "real", "nocut_big", "lists", "small", "default"))
    out.append(("switch_pq_to_asym", "pq", "big", "asym", "small", "default"))
    out.append(("switch_bet_to_rerank", "hamming", "bet_big", "rerank", "small", "default"))
    out.append(("switch_real_to_neighbours", "real", "nocut_big", "neighbours", "small", "default"))
    return out


PAIRS = _pairs()
ROUTES = ("same_context", "trim", "close_and_new")      # (a) the context that just ran the soil, (b) soil -> trim(), (c) soil -> close() -> a new one


# ------------------------------------------------------------------ inputs
def _frozen(**kw):
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return types.SimpleNamespace(**kw)


def _labels(rng, Q, N, C):
    """Multi-hot, about three labels a row; a query and rows without labels, a query with every label."""
    p = min(0.3, 3.0 / C)
    dl = (rng.random((N, C)) < p).astype(np.int64)
    ql = (rng.random((Q, C)) < p).astype(np.int64)
    ql[0] = 0
    dl[::7] = 0
    ql[1] = 1
    return ql, dl


def _seed(name, salt):
    return [salt] + [ord(ch) for ch in name]


@functools.lru_cache(maxsize=None)
def codes(name):
    """Binary codes of SHAPES[name] with the oracle's canonical ranking.  Bet-sized tables are independent bits (what the bet's own tests
    assert last_optimistic on); the others are queries near database rows.  Row 5 is a copy of row 4."""
    s = shape(name)
    rng = np.random.default_rng(_seed(name, 1))
    db = rng.integers(0, 2, (s.N, s.b), dtype=np.uint8)
    db[5] = db[4]
    if name.startswith("bet"):
        qb = rng.integers(0, 2, (s.Q, s.b), dtype=np.uint8)
    else:
        qb = db[rng.integers(0, s.N, s.Q)] ^ (rng.random((s.Q, s.b)) < 0.1).astype(np.uint8)
        qb[2] = db[4]                                     # the duplicated rows head a list: ranks 1 and 2 by index
    ql, dl = _labels(rng, s.Q, s.N, s.C)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, imatch, idx, dist = H.map_from_codes(qb, db, ql, dl, s.R)
    return _frozen(s=s, qb=qb, db=db, ql=ql, dl=dl, ap=ap, imatch=imatch, idx=idx, dist=dist, rel=imatch.sum(1).astype(np.int64))


@functools.lru_cache(maxsize=None)
def lists(name):
    """The list metrics' and histogram passes' references on codes(name), by the brute-force tables of the per-feature files."""
    c = codes(name)
    s = c.s
    order = B.ranked_by(B.hamming(c.qb, c.db))[:, :s.R]
    assert np.array_equal(order, c.idx)                   # two statements of the canonical order
    Gm = B.pair_grades(c.ql, c.dl)
    G = np.take_along_axis(Gm, order, axis=1)
    gain, disc = X.gain_table("linear", s.C), X.discount_table(s.R)
    all_h, rel_h = T.tables(c.qb, c.db, c.ql, c.dl)
    nG = B.defined_G(c.ql, c.dl)
    return _frozen(s=s, gain=gain, disc=disc, grades=G.astype(np.uint8), ap_at=B.ap_at_oracle(c.imatch, s.ks),
                   graded=B.graded_tables(G, s.ks, gain, disc), votes=B.vote_tables(c.dl[order], c.ql, s.ks),
                   tie=T.over_queries(T.fast, all_h, rel_h, s.ks), rel_hist=B.rel_hist(c.qb, c.db, c.ql, c.dl),
                   grade_hist=B.grade_hist(c.ql, c.dl), nG=nG, joint=B.joint_hist(c.qb, c.db, c.ql, c.dl, nG))


def _tie_rows(q0, table, R):
    """The rows at ranks R and R + 1 of query q0 on the float table: copying the first over the second leaves an exact tie at the cut."""
    sc = RM.inner_products(q0[None, :], table)[0]
    order = np.lexsort((np.arange(len(sc)), -sc))
    return int(order[R - 1]), int(order[R])


def _features(name, salt, b):
    s = shape(name)
    rng = np.random.default_rng(_seed(name, salt))
    dbf = np.tanh(rng.standard_normal((s.N, b))).astype(np.float32)
    qf = np.tanh(rng.standard_normal((s.Q, b))).astype(np.float32)
    dbf[s.N // 3] = dbf[s.N // 3 + 1]                      # a duplicated row: exact tie, index order
    ql, dl = _labels(rng, s.Q, s.N, s.C)
    return s, rng, qf, dbf, ql, dl


@functools.lru_cache(maxsize=None)
def real(name):
    """tanh features ranked by float32 inner product: oracle.real_map, bit for bit.  Where R < N, the row ranked R + 1 for query 0 is a
    copy of the row ranked R."""
    s, _, qf, dbf, ql, dl = _features(name, 2, shape(name).bf)
    if s.R < s.N:
        i, j = _tie_rows(qf[0], dbf, s.R)
        dbf[j] = dbf[i]
    ap, idx, score, match, rel = B.real_lists(qf, dbf, ql, dl, s.R)
    return _frozen(s=s, qf=qf, dbf=dbf, table=dbf, ql=ql, dl=dl, ap=ap, idx=idx, score=score, match=match, rel=rel)


@functools.lru_cache(maxsize=None)
def asym(name):
    """Real-valued queries against the database's sign codes read as +-1 (tests/test_asym_gpu.py): oracle.real_map on that table."""
    s, rng, qf, dbf, ql, dl = _features(name, 3, shape(name).bf)
    dbf[rng.integers(0, s.N, 7), rng.integers(0, s.bf, 7)] = 0.0          # exactly zero: a clear bit, read as -1
    pm1 = np.where(dbf > 0, 1, -1).astype(np.float32)
    i, j = _tie_rows(qf[0], pm1, s.R)
    dbf[j] = dbf[i]
    pm1[j] = pm1[i]
    ap, idx, score, match, rel = B.real_lists(qf, pm1, ql, dl, s.R)
    return _frozen(s=s, qf=qf, dbf=dbf, table=pm1, ql=ql, dl=dl, ap=ap, idx=idx, score=score, match=match, rel=rel)


@functools.lru_cache(maxsize=None)
def quantised(name):
    """Features, codebooks drawn from the features' own rows, the encoder oracle's codes and errors (tests/pq_encode_oracle.py), the
    decoded table and oracle.real_map's ranking on it (tests/test_pq_gpu.py).  The feature row ranked R + 1 for query 0 is a copy of the
    one ranked R, so their codes are too."""
    s0 = shape(name)
    b = s0.M * s0.dsub
    s, rng, qf, dbf, ql, dl = _features(name, 4, b)
    books = np.stack([dbf[rng.choice(s.N, s.K, replace=False), m * s.dsub:(m + 1) * s.dsub] for m in range(s.M)]).astype(np.float32)
    books[0, 0, 0] = 0.0
    books[s.M - 1, s.K - 1, s.dsub - 1] = -0.0
    i, j = _tie_rows(qf[0], pq.decode(PO.encode(dbf, books)[0], books), s.R)
    dbf[j] = dbf[i]
    pq_codes, err = PO.encode(dbf, books)
    x = pq.decode(pq_codes, books)
    ap, idx, score, match, rel = B.real_lists(qf, x, ql, dl, s.R)
    return _frozen(s=s, b=b, qf=qf, dbf=dbf, books=books, codes=pq_codes, err=err, table=x, ql=ql, dl=dl, ap=ap, idx=idx, score=score,
                   match=match, rel=rel)


@functools.lru_cache(maxsize=None)
def rerank(name):
    """tests/rerank_oracle.py's generator and ranking at SHAPES[name] with bf features; a query and rows without labels."""
    s = shape(name)
    qf, dbf, ql, dl = RO.generate(s.Q, s.N, s.bf, s.C, seed=sum(_seed(name, 5)), multi_hot=True)
    ql[0] = 0
    dl[::7] = 0
    o = RO.rerank(qf, dbf, ql, dl, s.R)
    # what the call counts on the device (stats rerank_records, rerank_groups_lds): the rows up to the threshold distance of each query,
    # and the distinct distances among them (one tie group each; every query of these shapes is ordered in LDS at once)
    kept = [o["d"][q][o["d"][q] <= o["dist"][q, -1]] for q in range(s.Q)]
    records, groups = int(sum(len(k) for k in kept)), int(sum(len(np.unique(k)) for k in kept))
    return _frozen(s=s, qf=qf, dbf=dbf, ql=ql, dl=dl, d=o["d"], sc=o["s"], records=records, groups=groups,
                   **{k: o[k] for k in ("idx", "dist", "score", "match", "ap", "rel")})


@functools.lru_cache(maxsize=None)
def neighbours(name):
    """Neighbour sets on codes(name)'s lists (tests/neighbour_oracle.py): the first G ranks as sets, then ragged random sets -- query 0
    has none, every neighbour of query 3 lies outside its list."""
    c = codes(name)
    s = c.s
    first = np.ascontiguousarray(c.idx[:, :s.G]).astype(np.uint32)
    gt = NO.random_sets(np.random.default_rng(_seed(name, 6)), c.idx, s.N, s.G, empty=(0,), outside=(3,))
    match = NO.match_bits(c.idx, gt)
    return _frozen(s=s, first=first, first_sorted=NO.sorted_table(first), first_match=NO.match_bits(c.idx, first), gt=gt,
                   gt_sorted=NO.sorted_table(gt), match=match, ap=NO.ap_rows(match), nbr_hist=NO.nbr_hist(c.qb, c.db, gt))


@functools.lru_cache(maxsize=None)
def devmem(name):
    """real(name)'s features as the device-array loaders take them, ranked twice: by the Hamming distance of their sign codes
    (oracle.hamming_map) and by inner product (oracle.real_map)."""
    r = real(name)
    s = r.s
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ap, imatch, idx, dist = H.map_from_codes(r.qf > 0, r.dbf > 0, r.ql, r.dl, s.R)
    return _frozen(s=s, real=r, ap=ap, match=imatch.astype(np.uint8), idx=idx, dist=dist)


DATA = {"hamming": codes, "lists": lambda name: (codes(name), lists(name)), "rerank": rerank, "real": real, "asym": asym, "pq": quantised,
        "pq_encode": quantised, "neighbours": lambda name: (codes(name), neighbours(name)), "devmem": devmem, "shard_step": codes}

"""NumPy statement of the re-ranked Hamming ranking (hg_topr_rerank): row n against query q has d = the Hamming distance of the sign
bits (bit = feature > 0) and s = oracle.real_map.inner_products' float32 inner product of the features; rows are ranked by
(d ascending, s descending, database index ascending) and the top R kept.  Match and AP are oracle.hamming_map's."""
import functools

import numpy as np

from oracle import hamming_map as H
from oracle import real_map as RM


def generate(Q, N, b, C, seed, multi_hot=False):
    """Features tanh(prototype[label] + 0.9 normal) with a few duplicated database rows -> (qf, dbf float32; ql, dl int64 {0,1})."""
    rng = np.random.default_rng(seed)
    proto = rng.normal(size=(C, b))
    dcls, qcls = rng.integers(0, C, N), rng.integers(0, C, Q)
    dbf = np.tanh(proto[dcls] + 0.9 * rng.normal(size=(N, b))).astype(np.float32)
    qf = np.tanh(proto[qcls] + 0.9 * rng.normal(size=(Q, b))).astype(np.float32)
    dl = np.zeros((N, C), np.int64)
    ql = np.zeros((Q, C), np.int64)
    dl[np.arange(N), dcls] = 1
    ql[np.arange(Q), qcls] = 1
    if multi_hot:
        dl |= (rng.random((N, C)) < 0.03).astype(np.int64)
        ql |= (rng.random((Q, C)) < 0.03).astype(np.int64)
    dbf[5::97] = dbf[4::97]                               # equal (d, s) against every query: the index decides
    return qf, dbf, ql, dl


def distances(qf, dbf):
    """int64 [Q, N]: Hamming distances of the sign bits."""
    return H.hamming_matrix(H.pack_bits(qf > 0), H.pack_bits(dbf > 0))


def rerank(qf, dbf, ql, dl, R):
    """-> dict idx int64 [Q, R], dist int64 [Q, R], score float32 [Q, R], match bool [Q, R], ap float64 [Q] (NaN: no hit), rel int64 [Q],
    and d [Q, N], s [Q, N] of all pairs."""
    d = distances(qf, dbf)
    s = RM.inner_products(qf, dbf)
    Q, N = d.shape
    idx = np.empty((Q, R), np.int64)
    match = np.empty((Q, R), bool)
    ap = np.full(Q, np.nan)
    rel = np.zeros(Q, np.int64)
    ar = np.arange(N)
    for q in range(Q):
        idx[q] = np.lexsort((ar, -s[q], d[q]))[:R]
        match[q] = H.label_match(ql[q, :], dl[idx[q], :])
        a, r = H.average_precision(match[q], R)
        rel[q] = r
        if a is not None:
            ap[q] = a
    rows = np.arange(Q)[:, None]
    return dict(idx=idx, dist=d[rows, idx], score=s[rows, idx], match=match, ap=ap, rel=rel, d=d, s=s)


def mean_ap(ap):
    return H.mean_ap(ap[~np.isnan(ap)])


# ---- the cases of tests/test_rerank_routes_gpu.py: inputs, the oracle's result, and the premises that make each case reach its route.
# ---- tests/test_rerank_host.py asserts the premises without a GPU; the GPU module asserts them again before it compares.
RR_LDS_KEYS = 16384                                      # hg_rerank.hpp: keys k_rr_order sorts in LDS.  The kernel's number: a case whose
                                                         # premise fails changes its seed or R, never this


def _onehot(rng, n, C):
    return np.eye(C, dtype=np.int64)[rng.integers(0, C, n)]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def signed_uniform(Q, N, b, C, seed, duplicates):
    """Features = a random sign times uniform(0.05, 1): Hamming distances binomial(b, 1/2), scores of either sign inside every group.
    duplicates: rows 5::97 are copies of rows 4::97, and rows 66000::97 are copies of rows 1000::97 -- equal (d, s) on either side of
    index 2^16, the row of the higher index with the smaller low 16 bits: only bits 16 ... 19 of the key put such a pair in order."""
    rng = np.random.default_rng(seed)
    sign = lambda n: rng.integers(0, 2, (n, b)) * 2.0 - 1.0
    dbf = (sign(N) * rng.uniform(0.05, 1.0, (N, b))).astype(np.float32)
    qf = (sign(Q) * rng.uniform(0.05, 1.0, (Q, b))).astype(np.float32)
    if duplicates:
        dbf[5::97] = dbf[4::97]
        far = dbf[66000::97]
        far[:] = dbf[1000::97][:len(far)]
    return qf, dbf, _onehot(rng, Q, C), _onehot(rng, N, C)


def positive_uniform(Q, N, b, C, seed, top=5):
    """All-positive features uniform(0.05, 1) -- every code equal, one group of N rows per query -- with the last `top` rows 1.0 in every
    feature: the highest scores of every query sit at the highest indices."""
    rng = np.random.default_rng(seed)
    dbf = rng.uniform(0.05, 1.0, (N, b)).astype(np.float32)
    qf = rng.uniform(0.05, 1.0, (Q, b)).astype(np.float32)
    dbf[N - top:] = 1.0
    return qf, dbf, _onehot(rng, Q, C), _onehot(rng, N, C)


def straddling_ties(o, bit):
    """bool [Q, R - 1]: ranks r, r + 1 hold records of equal (d, s) whose indices lie on either side of 2^bit with the low bits the other
    way round -- pairs that bits [bit, 24) of the key alone put in order."""
    idx, low = o["idx"], o["idx"] & ((1 << bit) - 1)
    tie = (o["dist"][:, 1:] == o["dist"][:, :-1]) & (o["score"][:, 1:] == o["score"][:, :-1])
    return (tie & (idx[:, :-1] < 1 << bit) & (idx[:, 1:] >= 1 << bit) & (low[:, 1:] < low[:, :-1]))


def route(o, R):
    """What k_rr_order does with the oracle's groups, as hg_get_stat reports it: per query the threshold t, M_q = #(d <= t) and the sizes
    of the groups d <= t; a query of M_q <= RR_LDS_KEYS is sorted at once (its non-empty groups all count as ordered in LDS), a longer
    one group by group -- in LDS up to RR_LDS_KEYS keys, by the radix passes beyond.
    -> dict t [Q], m [Q], sizes (list of arrays), records, groups_lds, groups_global."""
    d = o["d"]
    t = o["dist"][:, R - 1]
    m, sizes, lds, glob = [], [], 0, 0
    for q in range(len(d)):
        n = np.bincount(d[q], minlength=int(t[q]) + 1)[:int(t[q]) + 1]
        assert n[:-1].sum() < R <= n.sum()
        m.append(int(n.sum()))
        sizes.append(n)
        if m[-1] <= RR_LDS_KEYS:
            lds += int((n > 0).sum())
        else:
            lds += int(((n > 0) & (n <= RR_LDS_KEYS)).sum())
            glob += int((n > RR_LDS_KEYS).sum())
    return dict(t=t, m=np.array(m), sizes=sizes, records=int(sum(m)), groups_lds=lds, groups_global=glob)


# -- case 1: every code width
WIDTHS = [32 * nw - 1 for nw in range(1, 9)] + [128, 192]
WQ, WN, WR, WC = 70, 773, 300, 10


@functools.lru_cache(maxsize=None)
def width_case(b):
    """-> qf, dbf, ql, dl, R, oracle.  Query 11 has no label."""
    qf, dbf, ql, dl = generate(WQ, WN, b, WC, seed=b * 1000 + WC)
    ql[11] = 0
    _freeze(qf, dbf, ql, dl)
    return qf, dbf, ql, dl, WR, rerank(qf, dbf, ql, dl, WR)


def width_premises(qf, dbf, R, o):
    """The threshold group of some query is cut strictly inside, and some query's kept set is not the canonical (distance, index) one."""
    d = o["d"]
    canon, _ = H.topr_from_codes(qf > 0, dbf > 0, R)
    cut_inside = differs = 0
    for q in range(len(d)):
        t = o["dist"][q, -1]
        cut_inside += int((d[q] <= t).sum() > R and (d[q] < t).sum() < R)
        differs += int(set(canon[q].tolist()) != set(o["idx"][q].tolist()))
    print("b=%d: cut inside: %d queries, set differs from hg_topr's: %d queries" % (qf.shape[1], cut_inside, differs))
    assert cut_inside >= 1 and differs >= 1
    assert o["rel"][11] == 0 and np.isnan(o["ap"][11])
    r = route(o, R)
    assert (r["m"] <= RR_LDS_KEYS).all() and r["groups_global"] == 0
    return r


# -- case 2: more than RR_LDS_KEYS records per query, every group inside the LDS
@functools.lru_cache(maxsize=None)
def lds_groups_case():
    R = 20000
    qf, dbf, ql, dl = signed_uniform(3, 40000, 16, 4, seed=216, duplicates=False)
    _freeze(qf, dbf, ql, dl)
    return qf, dbf, ql, dl, R, rerank(qf, dbf, ql, dl, R)


def lds_groups_premises(R, o):
    r = route(o, R)
    print("M_q", r["m"].tolist(), "largest group", [int(n.max()) for n in r["sizes"]], "non-empty groups", [int((n > 0).sum()) for n in r["sizes"]])
    assert (r["m"] > RR_LDS_KEYS).all()
    assert all(n.max() <= RR_LDS_KEYS for n in r["sizes"])
    assert all((n > 0).sum() >= 2 for n in r["sizes"])
    assert r["groups_global"] == 0 and r["groups_lds"] == sum(int((n > 0).sum()) for n in r["sizes"])
    return r


# -- case 3: radix and LDS groups in one query, scores of both signs, the cut inside either kind
MIXED_R = {"cut_in_the_radix_group": (40000, 4), "cut_in_the_lds_group_behind_it": (50000, 5)}       # R, the threshold it must give


@functools.lru_cache(maxsize=None)
def mixed_tables():
    qf, dbf, ql, dl = signed_uniform(3, 70001, 8, 4, seed=308, duplicates=True)
    _freeze(qf, dbf, ql, dl)
    return qf, dbf, ql, dl


@functools.lru_cache(maxsize=None)
def mixed_case(name):
    R, _ = MIXED_R[name]
    return mixed_tables() + (R, rerank(*mixed_tables(), R))


def mixed_premises(name, o):
    R, t_want = MIXED_R[name]
    d, s = o["d"], o["s"]
    Q, N = d.shape
    r = route(o, R)
    for q in range(Q):
        n = np.bincount(d[q], minlength=9)
        print("query %d: groups %s, t = %d, M_q = %d" % (q, n.tolist(), r["t"][q], r["m"][q]))
        assert n[4] > RR_LDS_KEYS and n[3] <= RR_LDS_KEYS and n[5] <= RR_LDS_KEYS
        assert r["t"][q] == t_want
        assert n[:t_want].sum() < R < n[:t_want + 1].sum()            # the cut strictly inside the threshold group
        in4 = d[q] == 4
        assert (s[q][in4] > 0).any() and (s[q][in4] < 0).any()
        assert (np.nonzero(in4)[0] >= 65536).any()
        assert ((o["dist"][q, 1:] == o["dist"][q, :-1]) & (o["score"][q, 1:] == o["score"][q, :-1])).any()
        assert r["m"][q] > 2048                                        # k_rr_score: several blocks per query over several groups
    across = (straddling_ties(o, 16) & (o["dist"][:, 1:] == 4)).sum(1)
    print("pairs of equal (d, s) across index 2^16 that the radix group emits:", across.tolist())
    assert (across >= 1).all()
    # both signs and indices >= 2^16 also among what the radix group emits
    emitted4 = o["dist"] == 4
    assert (o["score"][emitted4] > 0).any() and (o["score"][emitted4] < 0).any() and (o["idx"][emitted4] >= 65536).any()
    assert r["groups_global"] == Q
    assert r["groups_lds"] == sum(int((n[:4] > 0).sum()) + (1 if t_want == 5 else 0) for n in r["sizes"])
    return r


# -- case 4: index bits 20...23
HIGH_R = 900000


@functools.lru_cache(maxsize=None)
def high_index_case():
    qf, dbf, ql, dl = positive_uniform(2, 1050000, 16, 4, seed=420)
    _freeze(qf, dbf, ql, dl)
    return qf, dbf, ql, dl, HIGH_R, rerank(qf, dbf, ql, dl, HIGH_R)


def high_index_premises(R, o, first=5, many=1000):
    N = o["d"].shape[1]
    high = (o["idx"] >= 1 << 20).sum(1)
    print("top R rows with index >= 2^20:", high.tolist(), "first ranks", o["idx"][:, :first].tolist())
    assert (o["d"] == 0).all()
    assert (o["idx"][:, :first] == np.arange(N - first, N)).all() and N - first >= 1 << 20
    assert (high >= many).all()
    across = straddling_ties(o, 20).sum(1)
    print("ranked pairs of equal (d, s) across index 2^20:", across.tolist(), "across 2^16:", straddling_ties(o, 16).sum(1).tolist())
    assert (across >= 1).all()
    r = route(o, R)
    assert r["groups_global"] == len(o["d"]) and r["groups_lds"] == 0 and r["records"] == len(o["d"]) * N
    return r


# -- case 5: chunks that cut through the 64-query tiles
@functools.lru_cache(maxsize=None)
def chunk_case():
    Q, N, b, C = 200, 773, 33, 10
    qf, dbf, ql, dl = generate(Q, N, b, C, seed=533)
    _freeze(qf, dbf, ql, dl)
    return qf, dbf, ql, dl, N, rerank(qf, dbf, ql, dl, N)


def chunk_premises(R, o, budget_mb=1):
    """The chunks run_rerank cuts at 16 bytes per record: a query joins the chunk while the chunk still fits the budget."""
    r = route(o, R)
    assert (r["m"] == R).all()
    chunks, recs = [], None
    for q, m in enumerate(r["m"]):
        if recs is None or (recs + m) * 16 > budget_mb << 20:
            chunks.append([q, q])
            recs = 0
        chunks[-1][1] = q + 1
        recs += int(m)
    print("chunks", chunks)
    assert chunks == [[0, 84], [84, 168], [168, 200]]
    assert any(a % 64 and a // 64 != (e - 1) // 64 for a, e in chunks)       # a chunk starts inside a tile and reaches the next one
    r["chunks"] = len(chunks)
    return r


# -- case 6: the ends of the score range, on case 1's tables of 63 features
ZERO_ROW = 700


@functools.lru_cache(maxsize=None)
def denormal_case():
    """Database features x 2^-70, query features x 2^-60: a product is below 2^-130, a multiple of 2^-149 after the fma's rounding.
    Such a chain does not cancel to zero by chance (63 terms of up to 2^19 quanta each), so row ZERO_ROW is all zeros: its score is
    +0.0 against every query, by construction."""
    qf, dbf, ql, dl, R, _ = width_case(63)
    qf, dbf = qf * np.float32(2.0 ** -60), dbf * np.float32(2.0 ** -70)
    dbf[ZERO_ROW] = 0.0
    _freeze(qf, dbf)
    return qf, dbf, ql, dl, R, rerank(qf, dbf, ql, dl, R)


def denormal_premises(R, o):
    tiny = np.float32(2.0 ** -126)
    sc, di = o["score"], o["dist"]
    pairs = zeros = 0
    for q in range(len(sc)):
        den = (np.abs(sc[q]) < tiny) & (sc[q] != 0)
        pairs += int((den[1:] & den[:-1] & (di[q, 1:] == di[q, :-1]) & (sc[q, 1:] != sc[q, :-1])).any())
        zeros += int(((sc[q] == 0) & ~np.signbit(sc[q])).sum())
    print("queries with distinct denormals next to each other in one group: %d; records of score +0.0: %d; denormal or zero: %d of %d"
          % (pairs, zeros, int((np.abs(sc) < tiny).sum()), sc.size))
    assert pairs >= 1 and zeros >= 1
    assert not np.signbit(o["s"][o["s"] == 0]).any()
    return route(o, R)


@functools.lru_cache(maxsize=None)
def overflow_case():
    """|database features| x 2^62, |query features| x 2^61: a product is about 2^123 |x y|, and a chain of 63 of them crosses 2^128 = +inf
    where sum |x y| reaches 32 -- these tables' sums lie on both sides of it.  (At 2^62 on either side the bar is 16 and every one of the
    54 110 sums is beyond it: nothing finite is left to order.)  No negative term, so no NaN."""
    qf, dbf, ql, dl, R, _ = width_case(63)
    qf, dbf = np.abs(qf) * np.float32(2.0 ** 61), np.abs(dbf) * np.float32(2.0 ** 62)
    _freeze(qf, dbf)
    with np.errstate(all="ignore"):                       # (the float64 model of the fma overflows its float32 cast, as meant)
        return qf, dbf, ql, dl, R, rerank(qf, dbf, ql, dl, R)


def overflow_premises(R, o):
    sc = o["score"]
    both = (np.isposinf(sc).any(1) & np.isfinite(sc).any(1)).sum()
    print("queries with +inf and finite scores in the top R: %d; +inf scores in all: %d of %d" % (both, int(np.isposinf(o["s"]).sum()), o["s"].size))
    assert not np.isnan(o["s"]).any()
    assert both >= 1
    return route(o, R)


# -- case 7: the stored order does not matter
@functools.lru_cache(maxsize=None)
def untied_case():
    """Case 3's tables without the duplicated rows and without the later row of every pair that still ties in (d, s) for some query
    (float32 scores of 19 000 rows of a group collide by chance), then the same rows under a fixed permutation.
    -> (qf, dbf, ql, dl, R, oracle), (dbf[perm], dl[perm]), perm."""
    qf, dbf, ql, dl = mixed_tables()
    R = MIXED_R["cut_in_the_radix_group"][0]
    d, s = distances(qf, dbf), RM.inner_products(qf, dbf)
    keep = np.ones(len(dbf), bool)
    keep[5::97] = False
    for q in range(len(qf)):
        rows = np.nonzero(keep)[0]
        order = rows[np.lexsort((rows, s[q][rows], d[q][rows]))]
        tie = (d[q][order[1:]] == d[q][order[:-1]]) & (s[q][order[1:]] == s[q][order[:-1]])
        keep[order[1:][tie]] = False
    dbf, dl = np.ascontiguousarray(dbf[keep]), np.ascontiguousarray(dl[keep])
    perm = np.random.default_rng(707).permutation(len(dbf))
    dbf_p, dl_p = np.ascontiguousarray(dbf[perm]), np.ascontiguousarray(dl[perm])
    _freeze(dbf, dl, dbf_p, dl_p, perm)
    return (qf, dbf, ql, dl, R, rerank(qf, dbf, ql, dl, R)), (dbf_p, dl_p), perm


def untied_premises(R, o):
    d, s = o["d"], o["s"]
    for q in range(len(d)):
        order = np.lexsort((s[q], d[q]))
        assert not ((d[q][order[1:]] == d[q][order[:-1]]) & (s[q][order[1:]] == s[q][order[:-1]])).any()
        n = np.bincount(d[q], minlength=9)
        assert n[4] > RR_LDS_KEYS and n[:4].sum() < R < n[:5].sum()
    print("rows kept: %d" % d.shape[1])
    assert d.shape[1] > 65536
    r = route(o, R)
    assert r["groups_global"] == len(d)
    return r


# -- case 8: a second-hand context: case 4, then case 1 at 31 features, then the first 70 001 rows of case 4
@functools.lru_cache(maxsize=None)
def high_index_head_case():
    qf, dbf, ql, dl, _, _ = high_index_case()
    n, R = 70001, 40000
    dbf, dl = np.ascontiguousarray(dbf[:n]), np.ascontiguousarray(dl[:n])
    _freeze(dbf, dl)
    return qf, dbf, ql, dl, R, rerank(qf, dbf, ql, dl, R)


def high_index_head_premises(R, o):
    r = route(o, R)
    assert (o["d"] == 0).all() and r["groups_global"] == len(o["d"]) and r["groups_lds"] == 0
    return r


"""Cases that reach the 16-bit filter's error margin (hg_real_bf.hpp: k_real_select_bf keeps approx > thr - eps, k_real_thr2 computes eps),
a host model of the filter's arithmetic, and a restatement of the margin.  NumPy only; not a test.  tests/test_real_margin_host.py proves on
the CPU that every case is sharp, tests/test_real_margin_gpu.py runs them.

What a case is made of (unscaled: every plateau feature is 1 + e 2^-23 for a small integer e; `dexp` and the queries' exponents then scale
the tables by powers of two, which scales every product, every partial sum and every bound exactly):

  query     q0[k] = 1 + (H - 1) 2^-23 for k < n, else 0, H = 2^(23 - p) half a 16-bit unit in the last place of 1.0 (p significant bits): one
            float32 below the rounding midpoint, so the 16-bit image is 1.0 and loses nearly all it can.  Query i is q0 2^i.
            n = 2^m - 1 features are active, so that the plateau's scores lie just below 2^m and float32 resolves them twice as finely.
  short     x[k] = q0[k]: parallel to the query, every product short by (1 + H')^2 - 1 relative.
  exact     the first m_b features 1 + 2 H 2^-23 (the next 16-bit number), the others 1.0, one of them carrying the remainder that
            makes the row's score the short rows' score.
  ladder    both kinds come as a ladder of candidates: candidate t is lower than candidate 0 by t float32 units of the score,
            through `digit` features at the end of the row (their partial sums lie in the score's binade, where one unit less in a
            product is at least one unit less in the chain: a ladder's chains fall strictly).  Float tables take one unit per step from
            one feature at a time, feature after feature (half's budget per feature, H - 2, is 127 units at n = 63); PQ tables, whose
            subspaces have 256 codewords at most, take positional digits in three subspaces.
  plateau   walking down both ladders at once, score rank i takes the next candidate of its kind (short where i % 6 is 1) whose chain
            is below the last one taken: P = 4 R rows, all chains distinct, kinds interleaved by score.  Index slot j takes score rank
            (j g) mod P: interleaved by index too.  A sixth of the rows is short, no more: with all of them lost, R rows still lie above
            a cut 1.3 R deep, so a margin too small ends the call at its first attempt with a wrong list, not with a lost bet.
  above     A rows of 16-bit numbers, 1 + 2^-5 times the plateau, a unit in the last place of bfloat16 apart in feature 0.
  rest      N(0, 0.05^2) features: norms far below the plateau's, scores many eps below it.

The +-1 code cases cannot follow this recipe to the letter: a code row has no low bits, so the plateau is the rows that differ from the
query's sign pattern in exactly m positions -- their chains differ only through the chain's own rounding, ties are ordered by index -- and
every plateau row is `short`, by the query's rounding alone.

Shares of eps the worst case reaches on paper, per 16-bit format and padded feature count KP (share_of_eps: q parallel to x, x the row of
largest norm, nothing given away; tests/test_real_margin_host.py pins the table):

    KP    bfloat16   half     codes (half, the queries alone round; 3 mismatches at 32, else 2)
    16    0.990      0.465    -
    32    -          -        0.188
    64    0.984      0.456    0.214
    128   0.977      0.443    0.215
    208   -          0.428    -

bfloat16's u = 2^-8 is exactly the round-to-nearest bound, so its margin is tight by design; half's u = 2^-10 is twice its bound.  A case
asserts RHO times the paper value for ITS norms, scales and ladder (the above rows' larger norm costs 3 %, the walk down the ladder up to
3 % in bfloat16 and 7 % in half; a single huge row or a norm rounded up to the smallest float costs what it costs: computed), RHO the
relative slack that turns the standard case's value into the 0.90 / 0.40 / 0.20 asked for at KP = 64.
"""
import functools
import math
import types

import numpy as np

from oracle import real_map as RM

FORMATS = {"bf16": dict(p=8, u=2.0 ** -8, eta=0.0), "half": dict(p=11, u=2.0 ** -10, eta=2.0 ** -14)}     # u, eta: as real_launch_select_bf passes them
ULP = 2.0 ** -23
ABOVE = 1.0 + 2.0 ** -5
F64 = {"bf16": 0.90, "half": 0.40, "codes": 0.20}          # the issue's fractions of eps at KP = 64


# ------------------------------------------------------------------ the filter's arithmetic and its margin
def round_bf16(x):
    """float32 -> bfloat16 -> float32, round to nearest even on the bit pattern."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    return r.view(np.float32)


def round_half(x, flush=False):
    """float32 -> IEEE half -> float64; flush: half-subnormal operands read as zero."""
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)
    if flush:
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
    return h


def filter_model(qf, dbf, fmt, flush=False):
    """approx float64 [Q, N]: the 16-bit score of every pair -- features rounded to the format, products summed in float64."""
    if fmt == "bf16":
        q, x = round_bf16(qf).astype(np.float64), round_bf16(dbf).astype(np.float64)
    else:
        q, x = round_half(qf, flush), round_half(dbf, flush)
    with np.errstate(invalid="ignore"):                        # (a query feature that is infinite in half: its scores mean nothing)
        return q @ x.T


def margin_model(qf, xmax2, KP, fmt, t):
    """eps float64 [Q]: k_real_thr2's margin, line by line (xmax2: the float32 the kernel reads; t [Q]: the cuts)."""
    u, eta = FORMATS[fmt]["u"], FORMATS[fmt]["eta"]
    qq = (np.asarray(qf, dtype=np.float64) ** 2).sum(1)
    xx = float(np.float32(xmax2)) * 1.0001
    c = 2.0 * u + u * u + (KP + 2) * 2.0 ** -21
    return (1.0001 * c * np.sqrt(qq * xx) + (KP + 2) * 2.0 ** -21 * np.abs(np.asarray(t, dtype=np.float64))
            + 1.01 * eta * math.sqrt(KP) * (np.sqrt(qq) + math.sqrt(xx)) + KP * eta * eta + 1e-30)


def xmax2_float32(dbf):
    """The largest row norm^2 as a float32 sum of float32 squares, four features at a time: what k_row_norm_max computed before it summed in
    double.  Squares of features below 2^-75 are 0 here."""
    x = np.ascontiguousarray(dbf, dtype=np.float32)
    x = np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))
    s = np.zeros(len(x), np.float32)
    with np.errstate(under="ignore", over="ignore"):
        for k in range(0, x.shape[1], 4):
            v = x[:, k:k + 4]
            s = s + (((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + v[:, 3] * v[:, 3])
    return np.float32(np.inf) if np.isnan(s).any() else s.max()


def xmax2_float(dbf):
    """The smallest float32 that is at least the largest row norm^2 (float64 sums: exact squares, 2^-44 relative in the sum)."""
    with np.errstate(over="ignore"):
        m = float((np.asarray(dbf, dtype=np.float64) ** 2).sum(1).max())
        f = np.float32(m)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < m else f


def format_of(xmax2):
    """The filter's format for a database: IEEE half while 1 <= the largest norm^2 < 2^30 (ensure_filter_image)."""
    return "half" if 1.0 <= float(xmax2) < 2.0 ** 30 else "bf16"


def is_wild(qf):
    """Queries with a feature half cannot hold: the half filter keeps every row of theirs and relies on no bound."""
    return ~(np.abs(np.asarray(qf, dtype=np.float32)) < 32768.0).all(1)


def sample_plan(N, R, b, sample_half, second_sample):
    """place_cut's first attempt restated: (stride of the first sample, the rank of the sampled score that becomes the cut)."""
    bpad = (b + 15) // 16 * 16
    can16 = bpad <= 128 and bool(sample_half)
    stride2, stride = R // 256, R // 24
    second = can16 and bool(second_sample) and stride2 >= 1 and stride >= 2 * stride2 and (N + stride - 1) // stride <= 16384
    if not second:
        stride = R // 64
    stride = max(stride, 1)
    M = (N + stride - 1) // stride
    fr = R * M / N
    return stride, int(math.ceil(fr + 5.0 * math.sqrt(fr))) + 1


def share_of_eps(fmt, KP, n, kind="floats", mism=0, walk=0.0, xnorm_ratio=ABOVE, qscale=1.0, xscale=1.0, xmax2=None):
    """The share of eps a short row's shortfall reaches, on paper: n active features of magnitude 1 (times the scales), the largest norm
    xnorm_ratio times the short rows' (or xmax2 given), `walk` the part of the shortfall the ladder gives away; codes: n = b features,
    `mism` mismatches, only the query rounds."""
    p, u, eta = FORMATS[fmt]["p"], FORMATS[fmt]["u"], FORMATS[fmt]["eta"]
    w = 1.0 + (2.0 ** (23 - p) - 1) * ULP
    if kind == "codes":
        chain, approx, qq, xx = (n - 2 * mism) * w * qscale, (n - 2 * mism) * qscale, n * (w * qscale) ** 2, float(n)
    else:
        chain, approx = n * w * w * qscale * xscale, n * qscale * xscale
        qq, xx = n * (w * qscale) ** 2, n * (w * xscale * xnorm_ratio) ** 2
    if xmax2 is not None:
        xx = float(xmax2)
    xx *= 1.0001
    c = 2.0 * u + u * u + (KP + 2) * 2.0 ** -21
    eps = (1.0001 * c * math.sqrt(qq * xx) + (KP + 2) * 2.0 ** -21 * chain + 1.01 * eta * math.sqrt(KP) * (math.sqrt(qq) + math.sqrt(xx))
           + KP * eta * eta + 1e-30)
    return (chain - approx) * (1.0 - walk) / eps


# the relative slack: what the issue's fractions at KP = 64 leave of the paper value of the standard case of each kind (63 active features,
# eight above rows as the largest norm -- a hair more than the table holds, rounded up -- and the part of the shortfall the ladder gives away)
_X2 = (62 * ABOVE ** 2 + (ABOVE + 8 * 2.0 ** -7) ** 2) * (1 + 1e-6)
WALK = {"bf16": 0.03, "half": 0.07}
RHO = {"bf16": F64["bf16"] / share_of_eps("bf16", 64, 63, walk=WALK["bf16"], xmax2=_X2),
       "half": F64["half"] / share_of_eps("half", 64, 63, walk=WALK["half"], xmax2=_X2),
       "codes": F64["codes"] / share_of_eps("half", 64, 64, "codes", mism=2)}


# ------------------------------------------------------------------ ladders
def _geometry(n, fmt):
    H = 2 ** (23 - FORMATS[fmt]["p"])
    w = 1.0 + (H - 1) * ULP
    eS = int(math.floor(math.log2(n * w * w)))                 # the plateau's scores lie in [2^eS, 2^(eS + 1))
    assert n * w * w < 2.0 ** (eS + 1) and n > 2 ** eS
    return H, 2 ** eS                                          # ... and one float32 unit of them is 2^eS units of a feature near 1.0


def thermometer(n, fmt, L):
    """red int64 [L, n]: candidate t gives away t units, one feature at a time from the last one down, H - 2 feature units at most each."""
    H, uu = _geometry(n, fmt)
    cap = (H - 2) // uu
    red = np.zeros((L, n), np.int64)
    rem = np.arange(L, dtype=np.int64)
    k = n - 1
    while rem.any():
        assert k >= uu, "the ladder's features must lie where the partial sums have reached the score's binade"
        d = np.minimum(rem, cap)
        red[:, k] = d
        rem = rem - d
        k -= 1
    return red


def digits(n, fmt, at):
    """red int64 [L, n]: the candidates in positional digits in the features at[0] (lowest), at[1], at[2].  A step of digit i takes
    weight[i] units, more than all lower digits together can (each rounding of the chain moves a product by half a unit at most), within
    H - 1 feature units per feature; the radix of the middle digit is the one that gives the longest ladder."""
    H, uu = _geometry(n, fmt)
    B = (H - 1) // uu
    assert min(at) >= uu and B >= 64
    best = None
    for r1 in range(2, 32):
        w1 = 30 + 1 + 2
        s2 = 30 + (r1 - 1) * w1
        w2 = s2 + 2 + 2
        if (r1 - 1) * w1 > B:
            break
        r2 = min(B // w2 + 1, 31)
        if best is None or 31 * r1 * r2 > best[0]:
            best = (31 * r1 * r2, r1, r2, w1, w2)
    L, r1, r2, w1, w2 = best
    t = np.arange(L)
    red = np.zeros((L, n), np.int64)
    red[:, at[0]], red[:, at[1]], red[:, at[2]] = t % 31, w1 * (t // 31 % r1), w2 * (t // (31 * r1))
    return red


def plateau_rows(n, fmt, P, red, pattern=lambda i: i % 6 == 1):
    """(rows float32 [P, n] unscaled in score order, highest first; short bool [P]; chains float32 [P] against q0).  red: a ladder."""
    H, uu = _geometry(n, fmt)
    L = len(red)
    mx = red.max(0)                                            # feature units each ladder feature can give away
    short = np.full((L, n), H - 1, np.int64) - red * uu
    m_b = int((n * (H - 1) - int(mx.sum()) * uu) // (2 * H))
    rest = n * (H - 1) - int(mx.sum()) * uu - 2 * H * m_b      # the exact rows' remainder, on a feature of its own
    assert m_b + 1 + np.count_nonzero(mx) <= n and (mx[:m_b + 1] == 0).all()
    exact = np.zeros((L, n), np.int64)
    exact[:, :m_b] = 2 * H
    exact[:, m_b] = rest
    exact += (mx[None, :] - red) * uu
    assert (short.sum(1) == exact.sum(1)).all()
    q0 = np.full((1, n), 1.0 + (H - 1) * ULP, np.float32)
    as_rows = lambda e: (1.0 + e * ULP).astype(np.float32)
    cand = {True: as_rows(short), False: as_rows(exact)}
    chain = {k: RM.inner_products(q0, v)[0] for k, v in cand.items()}
    for k in chain:
        assert (np.diff(chain[k]) < 0).all(), "a ladder's chains must fall strictly"
    rows, kinds, chains, at, last = [], [], [], {True: 0, False: 0}, np.float32(np.inf)
    for i in range(P):
        k = bool(pattern(i))
        while at[k] < L and not chain[k][at[k]] < last:
            at[k] += 1
        assert at[k] < L, "the ladder is too short for the plateau"
        rows.append(cand[k][at[k]]); kinds.append(k); chains.append(chain[k][at[k]])
        last = chain[k][at[k]]
        at[k] += 1
    return np.stack(rows), np.array(kinds), np.array(chains, np.float32)


def above_rows(n, A):
    a = np.full((A, n), ABOVE, np.float32)
    a[:, 0] += np.arange(1, A + 1, dtype=np.float32) * np.float32(2.0 ** -7)
    return a


# ------------------------------------------------------------------ cases
def _freeze(c):
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def _finish(c, seed, C=6):
    """Labels, the oracle's lists on c.x (the float table the ranking is defined on), and the bookkeeping every test reads."""
    rng = np.random.default_rng([seed, 77])
    c.dl = (rng.random((c.N, C)) < 0.25).astype(np.int64)
    c.ql = (rng.random((c.Q, C)) < 0.25).astype(np.int64)
    c.dl[0, 0] = c.ql[0, 0] = 1
    c.chains = RM.inner_products(c.qf, c.x)
    order = np.argsort(-c.chains, axis=1, kind="stable")[:, :c.R]
    c.idx, c.score = order, np.take_along_axis(c.chains, order, 1)
    from oracle import hamming_map as O
    c.ap = np.full(c.Q, np.nan)
    for i in range(c.Q):
        a, _ = O.average_precision(O.label_match(c.ql[i].astype(np.int8), c.dl[order[i]].astype(np.int8)), c.R)
        if a is not None:
            c.ap[i] = a
    c.xmax2 = xmax2_float(c.x) if c.kind == "floats" else c.xmax2
    c.fmt = format_of(c.xmax2)
    c.KP = (c.b + 15) // 16 * 16
    return _freeze(c)


def _positions(N, P, short, place, R, b):
    """Index of every plateau slot (slot order = index order)."""
    pos = (np.arange(P, dtype=np.int64) * N) // P
    if place == "spread":
        return pos
    ns = int(short.sum())
    if place == "first16":
        assert ns <= 16
        free = 16 + (np.arange(P - ns, dtype=np.int64) * (N - 32)) // (P - ns)
        out = np.empty(P, np.int64)
        out[short], out[~short] = np.arange(ns), free
        return out
    if place == "last16":
        assert ns <= N % 16
        free = (np.arange(P - ns, dtype=np.int64) * (N - 32)) // (P - ns)
        out = np.empty(P, np.int64)
        out[short], out[~short] = N - N % 16 + np.arange(ns), free
        return out
    if place == "unsampled":
        strides = {sample_plan(N, R, b, h, s)[0] for h in (0, 1) for s in (0, 1)} | {max(R // 256, 1)}
        assert 1 not in strides, strides
        ok = np.ones(N, bool)
        for s in strides:
            ok[::s] = False
        pos = pos // 2 * 2                                     # exact rows: even rows (every stride here is even or meets them anyway)
        free = np.flatnonzero(ok)
        want = pos[short]
        pos[short] = free[np.minimum(np.searchsorted(free, want), len(free) - 1)]
        assert len(np.unique(pos)) == P
        return pos
    raise ValueError(place)


@functools.lru_cache(maxsize=None)
def float_case(name, fmt, b, R, n=None, N=66003, Q=6, dexp=0, qexp=0, A=8, place="spread", rest="normal", special=None, wild=None, seed=1):
    """A float table with a plateau (module docstring).  dexp, qexp: the database and the queries times 2^dexp, 2^qexp; place: where the
    short rows lie; rest: what the odd background rows hold; special: (row features ..) written over one background row; wild: (query,
    feature, value) written into the queries."""
    rng = np.random.default_rng([seed, b, R])
    n = n or 2 ** int(math.log2(b)) - 1
    P = 4 * R
    H, uu = _geometry(n, fmt)
    if place in ("first16", "last16"):
        ns = 16 if place == "first16" else N % 16
        pattern = lambda i: i % 8 == 4 and i < 8 * ns
    else:
        pattern = lambda i: i % 6 == 1
    rows, kinds, _ = plateau_rows(n, fmt, P, thermometer(n, fmt, 2 * P + 64), pattern)
    g = 389 if place == "spread" or place == "unsampled" else 1
    rank_of_slot = (np.arange(P) * g) % P
    assert math.gcd(g, P) == 1
    short_slot = kinds[rank_of_slot]
    pos = _positions(N, P, short_slot, place, R, b)
    x = (rng.standard_normal((N, b)) * 0.05).astype(np.float32)
    if rest == "half_subnormal":
        x[1::2] = (rng.standard_normal((len(x[1::2]), b)) * 2.0 ** -17).astype(np.float32)
    elif rest == "float_subnormal":
        x[1::2] = (rng.standard_normal((len(x[1::2]), b)) * 2.0 ** -130 / 2.0 ** dexp).astype(np.float32)
    taken = np.zeros(N, bool)
    taken[pos] = True
    x[pos] = 0.0
    x[pos, :n] = rows[rank_of_slot]
    free = np.flatnonzero(~taken)
    above = free[(np.arange(A) * 997 + 40) % len(free)] if A else np.zeros(0, np.int64)
    x[above] = 0.0
    if A:
        x[above, :n] = above_rows(n, A)
    x = (x.astype(np.float64) * 2.0 ** dexp).astype(np.float32)
    if special is not None:
        at = free[len(free) // 2]
        assert at not in above
        x[at] = 0.0
        x[at, b - 1] = special
    q0 = np.zeros(b, np.float32)
    q0[:n] = 1.0 + (H - 1) * ULP
    qf = np.stack([(q0.astype(np.float64) * 2.0 ** (qexp + i)).astype(np.float32) for i in range(Q)])
    plateau_q = np.ones(Q, bool)
    if wild is not None:
        for qi, k, v in wild:
            qf[qi, k] = v
            plateau_q[qi] = False
    short = np.zeros(N, bool)
    short[pos[short_slot]] = True
    plateau = np.zeros(N, bool)
    plateau[pos] = True
    c = types.SimpleNamespace(name=name, kind="floats", N=N, Q=Q, b=b, R=R, n=n, x=x, qf=qf, short=short, plateau=plateau, above=above,
                              plateau_q=plateau_q, dexp=dexp, qexp=qexp, place=place, built=fmt)
    c = _finish(c, seed)
    # the fraction of eps this case must reach: the paper value for its own norms and scales, with the relative slack of KP = 64
    c.f = RHO[c.fmt] * share_of_eps(c.fmt, c.KP, n, walk=WALK[c.fmt], qscale=2.0 ** qexp, xscale=2.0 ** dexp, xmax2=c.xmax2)
    return c


@functools.lru_cache(maxsize=None)
def code_case(name, b, R, N=66003, Q=6, A=8, seed=2):
    """+-1 codes, queries q0 = (sign pattern) x (1 + (H - 1) 2^-23) in half: every row that differs from the pattern in exactly `mism`
    positions is on the plateau, short by the query's rounding alone."""
    rng = np.random.default_rng([seed, b, R])
    mism = 2 if b >= 64 else 3
    P = 4 * R
    H = 2 ** (23 - 11)
    sign = np.where(rng.random(b) < 0.5, -1.0, 1.0)
    x = np.where(rng.random((N, b)) < 0.5, -1.0, 1.0) * sign[None, :]           # (relative to the pattern: +1 agrees)
    low = (x < 0).sum(1) < 3 * mism
    x[low] = -x[low]                                                              # background: far from the pattern
    import itertools
    sets = list(itertools.combinations(range(b), mism))
    assert len(sets) >= P
    pick = [sets[(j * 7919) % len(sets)] for j in range(P)]
    assert len(set(pick)) == P
    pos = (np.arange(P, dtype=np.int64) * N) // P
    x[pos] = 1.0
    for j, s in enumerate(pick):
        x[pos[j], list(s)] = -1.0
    taken = np.zeros(N, bool)
    taken[pos] = True
    free = np.flatnonzero(~taken)
    above = free[(np.arange(A) * 997 + 40) % len(free)]
    x[above] = 1.0
    for i in range(1, A):
        x[above[i], (i * 5) % b] = -1.0                                           # one mismatch; above[0]: none
    x = (x * sign[None, :]).astype(np.float32)
    q0 = (sign * (1.0 + (H - 1) * ULP)).astype(np.float32)
    qf = np.stack([(q0.astype(np.float64) * 2.0 ** i).astype(np.float32) for i in range(Q)])
    plateau = np.zeros(N, bool)
    plateau[pos] = True
    c = types.SimpleNamespace(name=name, kind="codes", N=N, Q=Q, b=b, R=R, n=b, x=x, qf=qf, short=plateau.copy(), plateau=plateau, above=above,
                              plateau_q=np.ones(Q, bool), xmax2=np.float32(b), mism=mism, built="half")
    c = _finish(c, seed)
    c.f = RHO["codes"] * share_of_eps("half", c.KP, b, "codes", mism=mism)
    return c


@functools.lru_cache(maxsize=None)
def pq_case(name, M, dsub, R, N=66003, Q=6, A=8, K=256, dexp=-4, seed=3):
    """PQ codes and codebooks whose decoded table is a float plateau in bfloat16 (largest norm^2 < 1): the plateau's rows are combinations of
    codewords, their ladder three positional digits in the last three subspaces.  The codeword of largest norm in each subspace belongs to
    the last row alone; a still larger one to no row."""
    from hashgan_amd import pq
    rng = np.random.default_rng([seed, M, dsub, R])
    b = M * dsub
    n = b - 1
    fmt = "bf16"
    H, uu = _geometry(n, fmt)
    P = 4 * R
    at = (n - 1, n - 1 - dsub, n - 1 - 2 * dsub)
    rows, kinds, _ = plateau_rows(n, fmt, P, digits(n, fmt, at))
    rank_of_slot = (np.arange(P) * 389) % P
    short_slot = kinds[rank_of_slot]
    pos = (np.arange(P, dtype=np.int64) * (N - 1)) // P
    prow = np.zeros((P, b), np.float32)
    prow[:, :n] = rows[rank_of_slot]
    arow = np.zeros((A, b), np.float32)
    arow[:, :n] = above_rows(n, A)
    nbg = 64
    books = np.zeros((M, K, dsub), np.float32)
    codes = np.empty((N, M), np.uint8)
    for m in range(M):
        sl = slice(m * dsub, (m + 1) * dsub)
        words, inv = np.unique(np.concatenate([prow[:, sl], arow[:, sl]]), axis=0, return_inverse=True)
        nw = len(words)
        assert nw + nbg + 2 <= K, (m, nw)
        books[m, :nw] = words
        books[m, nw:nw + nbg] = (rng.standard_normal((nbg, dsub)) * 0.05).astype(np.float32)
        books[m, K - 2] = ABOVE * 1.001                        # the largest norm that occurs: the last row's alone (1.0323, larger than the above rows' feature 0)
        books[m, K - 2, 0] = 1.1
        books[m, K - 1] = 4.0                                  # larger still, used by no row
        codes[:, m] = nw + rng.integers(0, nbg, N)
        inv = inv.reshape(-1)
        codes[pos, m] = inv[:P]
        taken = np.zeros(N, bool)
        taken[pos] = True
        taken[N - 1] = True
        free = np.flatnonzero(~taken)
        above = free[(np.arange(A) * 997 + 40) % len(free)]
        codes[above, m] = inv[P:]
        codes[N - 1, m] = K - 2
    books = (books.astype(np.float64) * 2.0 ** dexp).astype(np.float32)
    x = pq.decode(codes, books)
    q0 = np.zeros(b, np.float32)
    q0[:n] = 1.0 + (H - 1) * ULP
    qf = np.stack([(q0.astype(np.float64) * 2.0 ** i).astype(np.float32) for i in range(Q)])
    short = np.zeros(N, bool)
    short[pos[short_slot]] = True
    plateau = np.zeros(N, bool)
    plateau[pos] = True
    # the loader's bound: per subspace the largest norm^2 among the codewords that occur, summed in double, rounded up
    bound = sum(max(float((books[m, k].astype(np.float64) ** 2).sum()) for k in np.unique(codes[:, m])) for m in range(M))
    f = np.float32(bound)
    xmax2 = np.nextafter(f, np.float32(np.inf)) if float(f) < bound else f
    c = types.SimpleNamespace(name=name, kind="pq", N=N, Q=Q, b=b, R=R, n=n, x=x, qf=qf, short=short, plateau=plateau, above=above,
                              plateau_q=np.ones(Q, bool), xmax2=xmax2, codes=codes, books=books, M=M, dsub=dsub, K=K, dexp=dexp, built=fmt)
    c = _finish(c, seed)
    c.f = RHO["bf16"] * share_of_eps("bf16", c.KP, n, walk=WALK["bf16"], xscale=2.0 ** dexp, xmax2=c.xmax2)
    return c


BELOW_2_15 = float(np.nextafter(np.float32(32768.0), np.float32(0.0)))
BELOW_1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
ABOVE_1 = float(np.nextafter(np.float32(1.0), np.float32(2.0)))

# name -> (builder, arguments): every case of tests/test_real_margin_gpu.py
CASES = {}


def _add(name, fn, *a, **kw):
    CASES[name] = (fn, (name,) + a, kw)


for _b in (16, 64, 128):                                                           # a: float tables in half
    _add("a-half-b%d" % _b, float_case, "half", _b, 256)
_add("a-half-b200", float_case, "half", 200, 192, n=199)                           # (QT = 1 kernels, the exact sample)
_add("b-bf16-scaled-down", float_case, "bf16", 64, 256, dexp=-4)                   # b: bfloat16 because the largest norm^2 < 1 ...
_add("b-bf16-b16-scaled-down", float_case, "bf16", 16, 256, dexp=-3)
_add("b-bf16-beyond-half", float_case, "bf16", 64, 256, dexp=16, special=40000.0)  # ... or because features exceed half's range
_add("c-first16", float_case, "bf16", 64, 128, dexp=-4, A=0, place="first16")     # c: where the rows of largest norm lie
_add("c-last-group", float_case, "bf16", 64, 88, N=66011, dexp=-4, A=0, place="last16")
_add("c-unsampled", float_case, "bf16", 64, 512, dexp=-4, A=0, place="unsampled")
_add("d-db-below-2^15", float_case, "half", 64, 256, dexp=11, special=BELOW_2_15)  # d: format boundaries of the database ...
_add("d-db-at-2^15", float_case, "bf16", 64, 256, dexp=11, special=32768.0)
_add("d-norm-below-1", float_case, "bf16", 64, 256, dexp=-4, special=BELOW_1)
_add("d-norm-above-1", float_case, "half", 64, 256, dexp=-4, special=ABOVE_1)
for _v, _tag in ((32768.0, "2^15"), (BELOW_2_15, "below-2^15"), (65520.0, "65520")):      # ... and of the queries
    _add("d-query-%s" % _tag, float_case, "half", 64, 256, wild=((2, 5, _v),))
for _k in (13, 63):
    _add("d-query-wild-at-%d" % _k, float_case, "half", 64, 256, wild=((1, _k, 40000.0),))
_add("e-2^-80", float_case, "bf16", 64, 256, dexp=-80, qexp=40)                    # e: norms whose float32 squares underflow
_add("e-2^-70", float_case, "bf16", 64, 256, dexp=-70, qexp=40)
_add("e-half-subnormal-rows", float_case, "half", 64, 256, rest="half_subnormal")
_add("e-float-subnormal-rows", float_case, "half", 64, 256, rest="float_subnormal")
for _b in (32, 64, 128):                                                           # f: codes and PQ
    _add("f-codes-b%d" % _b, code_case, _b, 256)
_add("f-pq-8x8", pq_case, 8, 8, 192)
_add("f-pq-16x8", pq_case, 16, 8, 160)

UNDERFLOW = ("e-2^-80", "e-2^-70")                                                 # the float32 norm is short of the truth here


def case(name):
    fn, a, kw = CASES[name]
    return fn(*a, **kw)

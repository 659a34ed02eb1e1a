"""Oracles for tie-aware AP at the top-R cut (hg_tie_ap), from one query's two table columns -- n[d] rows at Hamming distance d,
r[d] relevant rows among them -- and R.  Nothing here shares code with the library.

  exact(n, r, R)       fractions.Fraction and math.comb throughout, rounded to float once per output
  fast(n, r, R)        the hypergeometric pmf from exact integer binomials (a big-integer quotient is correctly rounded), every
                       other term in float64, every sum by math.fsum
  enumerated(n, r, R)  mean, minimum and maximum of the reference's AP (lib/metric.py:20-23) over every arrangement of the relevant
                       rows inside the tie groups, in Fractions -- tiny structures only
  bound(R, H)          the kernel's first-order rounding bound, relative

Every oracle returns dict(ap, p_hit, ap_min, ap_max, rel_exp, rel_lo, rel_hi, H); ap, ap_min, ap_max are NaN where no order has a hit.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

NAN = float("nan")


def bound(R, H):
    """(1.25 R + 4 H + 32) 2^-52, relative; H = h_hi - h_lo + 1 values the hit count of the cut group can take."""
    return (1.25 * np.asarray(R, dtype=np.float64) + 4.0 * np.asarray(H, dtype=np.float64) + 32.0) * 2.0 ** -52


def cut(n, r, R):
    """-> (whole groups [(P_d, S_d, n_d, r_d)] with n_d > 0, (P, S, n_t, r_t, c) of the cut group)."""
    n = [int(x) for x in n]
    r = [int(x) for x in r]
    assert 1 <= R <= sum(n) and all(0 <= b <= a for a, b in zip(n, r))
    P = S = 0
    whole = []
    for nd, rd in zip(n, r):
        if nd and P + nd >= R:
            return whole, (P, S, nd, rd, R - P)
        if nd:
            whole.append((P, S, nd, rd))
        P += nd
        S += rd
    raise AssertionError("unreachable")


def _tree_sum(xs):
    """Sum of Fractions by halves: the big denominators meet late."""
    xs = list(xs)
    if not xs:
        return Fraction(0)
    while len(xs) > 1:
        xs = [xs[i] + xs[i + 1] if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
    return xs[0]


def _h_range(nt, rt, c):
    return max(0, c - (nt - rt)), min(c, rt)


def _run(n, r, R, exact_mode):
    whole, (P, S, nt, rt, c) = cut(n, r, R)
    if exact_mode:
        num = Fraction
        total = _tree_sum
        out = float
    else:
        num = float
        total = math.fsum
        out = float

    def q(a, b):                       # a / b of two integers
        return Fraction(a, b) if exact_mode else a / b

    # whole groups
    tI, tmax, tmin = [], [], []
    for Pd, Sd, nd, rd in whole:
        if rd == 0:
            continue
        rho = q(rd - 1, nd - 1) if nd > 1 else num(0)
        f = q(rd, nd)
        tI.extend(f * ((Sd + 1 + (i - 1) * rho) / num(Pd + i)) for i in range(1, nd + 1))
        tmax.extend(q(Sd + j, Pd + j) for j in range(1, rd + 1))
        tmin.extend(q(Sd + j, Pd + nd - rd + j) for j in range(1, rd + 1))
    I, Imax, Imin = total(tI), total(tmax), total(tmin)
    T0 = total(q(1, P + i) for i in range(1, c + 1))
    T1 = total(q(i - 1, P + i) for i in range(1, c + 1))
    h_lo, h_hi = _h_range(nt, rt, c)
    den = math.comb(nt, c)

    def pmf(h):
        return q(math.comb(rt, h) * math.comb(nt - rt, c - h), den)

    def B(h):
        if h == 0:
            return num(0)
        slope = q(h - 1, c - 1) if c > 1 else num(0)
        return q(h, c) * ((S + 1) * T0 + slope * T1)

    hs = [h for h in range(h_lo, h_hi + 1) if S + h > 0]
    p_hit = total(pmf(h) for h in hs)
    res = dict(rel_exp=out(S + q(c * rt, nt)), rel_lo=S + h_lo, rel_hi=S + h_hi, H=h_hi - h_lo + 1, p_hit=out(p_hit))
    if not hs:
        res.update(ap=NAN, ap_min=NAN, ap_max=NAN)
        return res
    res["ap"] = out(total(pmf(h) * ((I + B(h)) / num(S + h)) for h in hs) / p_hit)
    # the envelope: Bmax(h) and Bmin(h) as running sums (Bmin by the recurrence, which test_tie_ap_host checks against the
    # definition and against the enumeration)
    best_max = best_min = None
    Bmax, Bmin, U = (num(0), num(0), num(0)) if exact_mode else (_Acc(), _Acc(), _Acc())
    for h in range(0, h_hi + 1):
        if h > 0:
            x = P + c - (h - 1)
            if exact_mode:
                Bmax = Bmax + Fraction(S + h, P + h)
                U = U + Fraction(1, x)
                Bmin = Bmin + Fraction(S, x) + U
            else:
                Bmax.add((S + h) / (P + h))
                U.add(1 / x)
                Bmin.add(S / x, U.hi, U.lo)
        if h >= h_lo and S + h > 0:
            vmax = (Imax + (Bmax if exact_mode else Bmax.hi)) / num(S + h)
            vmin = (Imin + (Bmin if exact_mode else Bmin.hi)) / num(S + h)
            best_max = vmax if best_max is None or vmax > best_max else best_max
            best_min = vmin if best_min is None or vmin < best_min else best_min
    res["ap_max"], res["ap_min"] = out(best_max), out(best_min)
    return res


class _Acc:
    """A running sum kept as two floats, each addition through math.fsum: hi is the correctly rounded sum of everything added
    to (hi, lo) so far, lo what that rounding left over."""

    def __init__(self):
        self.hi = self.lo = 0.0

    def add(self, *xs):
        hi = math.fsum((self.hi, self.lo) + xs)
        self.lo = math.fsum((self.hi, self.lo) + xs + (-hi,))
        self.hi = hi


def exact(n, r, R):
    return _run(n, r, R, True)


def fast(n, r, R):
    return _run(n, r, R, False)


def bmin_by_definition(P, S, c, h):
    return sum((Fraction(S + j, P + c - h + j) for j in range(1, h + 1)), Fraction(0))


def reference_ap(imatch):
    """lib/metric.py:20-23 on one 0/1 list, in Fractions; None where the reference skips the query."""
    rel = sum(imatch)
    if rel == 0:
        return None
    cum = 0
    acc = Fraction(0)
    for k, m in enumerate(imatch, 1):
        cum += m
        if m:
            acc += Fraction(cum, k)
    return acc / rel


def enumerated(n, r, R):
    """Every arrangement of the r_d relevant rows among the n_d places of each group is the image of r_d! (n_d - r_d)! row orders,
    the same number for each: uniform over the arrangements IS uniform over the tie orders."""
    groups = [(int(a), int(b)) for a, b in zip(n, r) if a]
    per_group = []
    for nd, rd in groups:
        per_group.append([tuple(1 if i in pos else 0 for i in range(nd)) for pos in itertools.combinations(range(nd), rd)])
    aps, rels, total = [], [], 0
    for combo in itertools.product(*per_group):
        lst = [m for g in combo for m in g][:R]
        total += 1
        rels.append(sum(lst))
        ap = reference_ap(lst)
        if ap is not None:
            aps.append(ap)
    res = dict(p_hit=float(Fraction(len(aps), total)), rel_exp=float(Fraction(sum(rels), total)), rel_lo=min(rels), rel_hi=max(rels))
    if aps:
        res.update(ap=float(sum(aps, Fraction(0)) / len(aps)), ap_min=float(min(aps)), ap_max=float(max(aps)))
    else:
        res.update(ap=NAN, ap_min=NAN, ap_max=NAN)
    return res


def tables(qb, db, ql, dl):
    """Brute force: the Q x N distance matrix, the label match, a bincount per query -> (all, rel) int64 [Q, b+1]."""
    b = qb.shape[1]
    ip = (2.0 * qb.astype(np.float32) - 1.0) @ (2.0 * db.astype(np.float32) - 1.0).T
    D = ((b - ip) / 2).astype(np.int64)
    rel = (ql.astype(np.int64) @ dl.astype(np.int64).T) > 0
    all_h = np.stack([np.bincount(D[q], minlength=b + 1) for q in range(len(qb))])
    rel_h = np.stack([np.bincount(D[q][rel[q]], minlength=b + 1) for q in range(len(qb))])
    return all_h, rel_h


KEYS = ("ap", "p_hit", "ap_min", "ap_max", "rel_exp", "rel_lo", "rel_hi", "H")


def over_queries(fn, all_h, rel_h, Rs):
    """fn = exact or fast on every (query, R) -> dict of [Q, nR] arrays."""
    Q = len(all_h)
    out = {k: np.empty((Q, len(Rs)), dtype=np.int64 if k in ("rel_lo", "rel_hi", "H") else np.float64) for k in KEYS}
    for qi in range(Q):
        for j, R in enumerate(Rs):
            res = fn(all_h[qi], rel_h[qi], int(R))
            for k in KEYS:
                out[k][qi, j] = res[k]
    return out

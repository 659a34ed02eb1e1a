"""oracle/real_map.py's ranking at N = 66000 and beyond in a second per case: the oracle's own fma chains (RM.inner_products) run on a
per-query candidate set that provably contains the top R, instead of on all Q x N pairs (two minutes at 70 x 66000 x 256).  Not a test.

The candidate set.  The chain ip(q, x) = fl(fl(... fl(q0 x0) + q1 x1 ...)) of bp = b padded to 16 fused multiply-adds in float32 differs
from the exact inner product by at most gamma_bp sum |q_k| |x_k|, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1: every partial sum carries one rounding; the final `+ 0.0` is exact).  The float64 product of the same
tables (BLAS, any order) is within gamma64_b sum |q_k| |x_k| of the exact one, u64 = 2^-53.  With E = (gamma_bp + gamma64_b) * A,
A = |q| . |x| rounded up, every chain score lies in [s64 - E, s64 + E].  Let t be the R-th largest LOWER end: R rows score t or more,
so a row whose UPPER end is below t is not among the top R under (score descending, index ascending); every other row is a candidate.
The candidates keep their index order, so the stable sort breaks ties as the oracle does."""
import numpy as np

from oracle import hamming_map as H
from oracle import real_map as RM


def candidate_rows(s64, A, bp, R):
    u, u64 = 2.0 ** -24, 2.0 ** -53
    gam = bp * u / (1.0 - bp * u) + bp * u64 / (1.0 - bp * u64)
    E = 1.0001 * gam * A + 1e-300                           # (1.0001: A itself is a rounded float64 sum)
    lo = s64 - E
    t = np.partition(lo, len(lo) - R)[len(lo) - R]
    return np.flatnonzero(s64 + E >= t)


def ranked_oracle(qf, x, ql, dl, R):
    """-> (ap float64 [Q] with nan for skipped queries, idx int64 [Q, R], score float32 [Q, R], candidates per query): what
    RM.map_from_features(qf, x, ql, dl, R)[1:] returns, bit for bit (tests/test_kernel_coverage_host.py holds it to that)."""
    qf = np.ascontiguousarray(qf, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    Q, b = qf.shape
    bp = (b + 15) // 16 * 16
    q64, x64 = qf.astype(np.float64), x.astype(np.float64)
    S = q64 @ x64.T
    A = np.abs(q64) @ np.abs(x64).T
    idx = np.empty((Q, R), np.int64)
    score = np.empty((Q, R), np.float32)
    ap = np.full(Q, np.nan)
    ncand = np.empty(Q, np.int64)
    for i in range(Q):
        rows = candidate_rows(S[i], A[i], bp, R)
        ncand[i] = len(rows)
        ips = RM.inner_products(qf[i:i + 1], x[rows])[0]
        o = np.argsort(-ips, kind="stable")[:R]             # ip descending, index ascending (rows are in index order)
        idx[i], score[i] = rows[o], ips[o]
        a, _ = H.average_precision(H.label_match(ql[i, :], dl[idx[i], :]), R)
        if a is not None:
            ap[i] = a
    return ap, idx, score, ncand


def rescore_slices_per_wave(per_slice):
    """hg_real.hip's heuristic restated: the slice count (of 1, 2, 3, 4, 6, 8; 1 or 2 from 64 rows per slice) with the least expected cost."""
    import math
    best, SG = 1e300, 1
    for sg in (1, 2, 3, 4, 6, 8):
        if per_slice >= 64.0 and sg > 2:
            break
        m = per_slice * sg
        sd = math.sqrt(m if m > 1.0 else 1.0)
        rounds = 1.0
        for k in range(1, 65):
            p = 0.5 * math.erfc((64.0 * k - m) / sd * 0.7071067811865476)
            rounds += p
            if p < 1e-6:
                break
        cost = (0.5 + rounds * (1.0 + 0.03 * sg)) / sg
        if cost < best:
            best, SG = cost, sg
    return SG

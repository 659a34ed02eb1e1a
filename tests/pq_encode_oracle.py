"""The PQ encoder's contract restated by brute force in float64 (include/hashgan_amd.h, hg_pq_encode), and the cases its tests share.

For codebooks float32 [M][K][dsub] and a feature row x, per subspace m:
    d_k = 0.0;  for j = 0 .. dsub-1:  t = (double)x[m*dsub+j] - (double)w[m][k][j];  d_k = d_k + t*t     (two roundings per step)
    best = 0;  for k = 1 .. K-1:  if (d_k < d_best) best = k                                                 (strict: the lowest index)
    err(row) = 0.0;  for m = 0 .. M-1:  err += d_best(m)
NumPy evaluates `d + t * t` as a rounded product and a rounded sum -- it has no fused multiply-add -- so the loops below are the
contract itself, vectorised over rows and codewords only.  Not a test: tests/test_pq_encode_host.py and tests/test_pq_encode_gpu.py use it."""
import fractions
import functools
import types

import numpy as np

#          N, M, dsub, K
SHAPES = [(5003, 8, 8, 256),        # register path, 16 KB of float64 codewords per subspace
          (2001, 3, 11, 16),        # odd dsub, b = 33
          (1001, 1, 1, 2),          # the smallest table
          (777, 5, 51, 256),        # b = 255: the generic path, more than one wavefront's tail
          (1030, 16, 8, 64),        # M = 16
          (4097, 2, 6, 4)]          # every codeword duplicated: thousands of rows where the lowest index must win
DUPLICATED = (4097, 2, 6, 4)


def encode(features, codebooks):
    """-> (codes uint8 [N, M], err float64 [N]) by the three lines above; features any float type (widened exactly), non-finite included."""
    with np.errstate(all="ignore"):
        x = np.asarray(features).astype(np.float64)
        w = np.asarray(codebooks, dtype=np.float32).astype(np.float64)
        M, K, dsub = w.shape
        N = x.shape[0]
        assert x.shape == (N, M * dsub)
        codes = np.zeros((N, M), dtype=np.uint8)
        err = np.zeros(N, dtype=np.float64)
        for m in range(M):
            d = np.zeros((N, K), dtype=np.float64)
            for j in range(dsub):
                t = x[:, m * dsub + j, None] - w[m, None, :, j]
                d = d + t * t
            best = np.zeros(N, dtype=np.int64)
            dbest = d[:, 0].copy()
            for k in range(1, K):
                take = d[:, k] < dbest
                best[take] = k
                dbest[take] = d[take, k]
            codes[:, m] = best
            err = err + dbest
    return codes, err


def _frozen(ns):
    for a in vars(ns).values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return ns


@functools.lru_cache(maxsize=None)
def case(N, M, dsub, K):
    """tanh features; codebooks drawn per subspace from the features' own rows (rows that ARE a codeword: distance 0.0), the last
    codeword a duplicate of the first -- for DUPLICATED every codeword of the upper half a duplicate of the lower half; the oracle's
    codes and errors.  Computed once, never modified."""
    rng = np.random.default_rng(1000 * M + 10 * dsub + K)
    b = M * dsub
    x = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    books = np.stack([x[rng.choice(N, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    if (N, M, dsub, K) == DUPLICATED:
        books[:, K // 2:] = books[:, :K // 2]
    else:
        books[:, K - 1] = books[:, 0]
    codes, err = encode(x, books)
    return _frozen(types.SimpleNamespace(N=N, M=M, dsub=dsub, K=K, b=b, x=x, books=books, codes=codes, err=err))


def _rn(q):
    """A rational rounded to the nearest float64 (Python's int / int is correctly rounded)."""
    return q.numerator / q.denominator


@functools.lru_cache(maxsize=None)
def tie_case(pairs=400, per_row=100):
    """The ties a fused multiply-add would break: dsub = 2, K = 2, a subspace per (c, p, r) -- the row's subvector is (c, c), the
    codewords (p, r) and (r, p).  Unfused, d_0 = (c-p)^2 + (c-r)^2 and d_1 = (c-r)^2 + (c-p)^2 are the same two rounded squares added
    in either order: an exact tie, code 0.  A fused chain d = fma(t, t, d) rounds only the first square, so d_0 and d_1 differ whenever
    the two squares round differently -- and then the HIGHER index can win.  c in [0.5, 1), p, r in [1e-3, 2e-3) as float32 from
    default_rng(2); `pairs` of them laid out as pairs / per_row rows of per_row subspaces (b = 2 * per_row <= 255).
    -> x float32 [rows, 2 per_row], books float32 [per_row, 2, 2] per row -- one encode call per row: the codebooks are the row's own --,
    fused_wrong: how many pairs a fused evaluation gets wrong (emulated exactly with fractions.Fraction)."""
    rng = np.random.default_rng(2)
    c = rng.uniform(0.5, 1.0, pairs).astype(np.float32)
    p = rng.uniform(1e-3, 2e-3, pairs).astype(np.float32)
    r = rng.uniform(1e-3, 2e-3, pairs).astype(np.float32)
    rows = pairs // per_row
    assert rows * per_row == pairs
    x = np.repeat(c.reshape(rows, per_row), 2, axis=1)                       # (c, c) per subspace
    books = np.empty((rows, per_row, 2, 2), dtype=np.float32)
    books[:, :, 0, 0] = p.reshape(rows, per_row); books[:, :, 0, 1] = r.reshape(rows, per_row)
    books[:, :, 1, 0] = r.reshape(rows, per_row); books[:, :, 1, 1] = p.reshape(rows, per_row)
    fused_wrong = 0
    F = fractions.Fraction
    for ci, pi, ri in zip(c, p, r):
        tp, tr = float(ci) - float(pi), float(ci) - float(ri)                # float64 differences of float32 values
        sp, sr = tp * tp, tr * tr                                            # the rounded squares
        assert sp + sr == sr + sp
        d0 = _rn(F(tr) * F(tr) + F(sp))                                      # fma(tr, tr, rn(tp^2))
        d1 = _rn(F(tp) * F(tp) + F(sr))                                      # fma(tp, tp, rn(tr^2))
        fused_wrong += d1 < d0
    return _frozen(types.SimpleNamespace(pairs=pairs, rows=rows, M=per_row, x=x, books=books, fused_wrong=int(fused_wrong)))


def bf16_exact(x):
    """float32 values rounded (toward zero) to what bfloat16 holds exactly -> (the float32 values, their uint16 bit patterns)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32), (u >> 16).astype(np.uint16)

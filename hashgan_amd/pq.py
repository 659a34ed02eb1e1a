"""Product quantisation on the host: the tables hg_set_database_pq takes, and what it derives from them.

M disjoint subspaces of dsub features each (b = M * dsub <= 255), K <= 256 codewords per subspace:
    codebooks  float32 [M, K, dsub]
    codes      uint8   [N, M]
A row decodes by pure gather, x[n, k] = codebooks[k // dsub, codes[n, k // dsub], k % dsub] -- no arithmetic, so ranking against the
codes is by definition ranking against decode(codes, codebooks), bit for bit.  encode() is the host's encoder, in float64 on whatever
float type it is given; encode_gpu() is the same contract on float32 features as a HIP kernel (hg_pq_encode / hg_pq_encode_dev), which is
what MAPs(R, quantised=True) uses for a database given as .output + .codebooks and for quantise_queries=True (SQD from features)."""
import numpy as np

MAX_FEATURES = 255
MAX_CODEWORDS = 256


def check_codebooks(codebooks):
    """-> C-contiguous float32 [M, K, dsub]; ValueError on another dtype or shape, or beyond the limits."""
    cb = np.asarray(codebooks)
    if cb.dtype != np.float32:
        raise ValueError("codebooks must be float32 (have %s)" % cb.dtype)
    if cb.ndim != 3 or min(cb.shape) < 1:
        raise ValueError("codebooks must be [M, K, dsub] with M, K, dsub >= 1 (have shape %r)" % (cb.shape,))
    M, K, dsub = cb.shape
    if K > MAX_CODEWORDS:
        raise ValueError("at most %d codewords per subspace (have K=%d)" % (MAX_CODEWORDS, K))
    if M * dsub > MAX_FEATURES:
        raise ValueError("at most %d features (have M * dsub = %d)" % (MAX_FEATURES, M * dsub))
    return np.ascontiguousarray(cb)


def check_tables(codes, codebooks, values=True):
    """-> (codes uint8 [N, M], codebooks float32 [M, K, dsub]), both C-contiguous; ValueError on another dtype or shape; values=True
    also on a code >= K or a non-finite codeword (what hg_set_database_pq refuses itself)."""
    cb = check_codebooks(codebooks)
    c = np.asarray(codes)
    if c.dtype != np.uint8:
        raise ValueError("codes must be uint8 (have %s)" % c.dtype)
    if c.ndim != 2 or c.shape[1] != cb.shape[0]:
        raise ValueError("codes must be [N, M] with the codebooks' M=%d (have shape %r)" % (cb.shape[0], c.shape))
    if values:
        if c.size and int(c.max()) >= cb.shape[1]:
            n, m = np.argwhere(c >= cb.shape[1])[0]
            raise ValueError("code %d at row %d, subspace %d is not below K=%d" % (c[n, m], n, m, cb.shape[1]))
        if not np.isfinite(cb).all():
            raise ValueError("codebooks must be finite")
    return np.ascontiguousarray(c), cb


def decode(codes, codebooks):
    """float32 [N, M * dsub]: the gather, every bit of a codeword untouched (signed zeros, subnormals)."""
    c, cb = check_tables(codes, codebooks)
    M, _, dsub = cb.shape
    return np.ascontiguousarray(cb[np.arange(M)[None, :], c].reshape(c.shape[0], M * dsub))


def encode(features, codebooks):
    """uint8 [N, M]: per subspace the codeword nearest by squared distance in float64, the lowest index on ties."""
    cb = check_codebooks(codebooks)
    x = np.asarray(features)
    M, K, dsub = cb.shape
    if x.dtype.kind != "f":
        raise ValueError("features must be floating point (have %s)" % x.dtype)
    if x.ndim != 2 or x.shape[1] != M * dsub:
        raise ValueError("features must be [N, M * dsub] = [N, %d] (have shape %r)" % (M * dsub, x.shape))
    if not np.isfinite(cb).all():
        raise ValueError("codebooks must be finite")
    out = np.empty((x.shape[0], M), dtype=np.uint8)
    step = max(1, (1 << 20) // K)                       # rows per block: 8 MB of float64 distances at a time
    for m in range(M):
        w = cb[m].astype(np.float64)
        ww = (w * w).sum(1)
        for r0 in range(0, x.shape[0], step):
            xs = x[r0:r0 + step, m * dsub:(m + 1) * dsub].astype(np.float64)
            # A matrix product finds the candidates: |x|^2 - 2 x.w + |w|^2 differs from the sum of squared differences by rounding alone,
            # orders of magnitude below `tol`.  A row with one codeword within `tol` of its smallest has its answer; the others -- ties
            # and near-ties -- get the squared distances themselves, summed feature by feature.
            xx = (xs * xs).sum(1)
            approx = xx[:, None] - 2.0 * (xs @ w.T) + ww[None, :]
            tol = 1e-11 * (dsub + 2) * (xx + ww.max() + 1.0)
            best = approx.argmin(1)
            close = np.flatnonzero((approx <= (approx.min(1) + tol)[:, None]).sum(1) > 1)
            if close.size:
                d = np.zeros((close.size, K))
                for j in range(dsub):
                    t = xs[close, j, None] - w[None, :, j]
                    d += t * t
                best[close] = d.argmin(1)                # (argmin: the first, the lowest index, among equals)
            out[r0:r0 + step, m] = best
    return out


def encode_gpu(features, codebooks, device=0, return_error=False):
    """encode() on the GPU, exactly (include/hashgan_amd.h, hg_pq_encode: per subspace the float64 sum of squared differences feature by
    feature, two roundings per step, the lowest index on ties): features a host array, a torch tensor, an object with
    __cuda_array_interface__ or a devarray.DeviceArray -- float32, or float16 / bfloat16 widened exactly -- [N, M * dsub].  The context
    comes from the pool MAPs objects draw theirs from.  ValueError for what encode() refuses, before any GPU use, and for rows with a
    non-finite feature, after the call.  -> codes uint8 [N, M]; return_error=True: (codes, err float64 [N], the summed squared distance
    to the chosen codewords)."""
    from . import metric
    from .devarray import as_device_array
    cb = check_codebooks(codebooks)
    M, K, dsub = cb.shape
    if not np.isfinite(cb).all():
        raise ValueError("codebooks must be finite")
    x = as_device_array(features)
    if x is None:
        x = np.asarray(features)
        if x.dtype.kind != "f":
            raise ValueError("features must be floating point (have %s)" % x.dtype)
        if x.dtype.itemsize > 4:
            raise ValueError("the GPU encodes float32 (or float16) features: %s would be rounded first -- convert it, or use encode()" % x.dtype)
    elif x.dtype not in ("float32", "float16", "bfloat16"):
        raise ValueError("features must be floating point (have %s)" % x.dtype)
    if x.ndim != 2 or x.shape[1] != M * dsub:
        raise ValueError("features must be [N, M * dsub] = [N, %d] (have shape %r)" % (M * dsub, tuple(x.shape)))
    if x.shape[0] < 1:
        raise ValueError("features must have at least one row")
    eng = metric._Pool.acquire(device)
    try:
        codes, err, bad = eng.ctx.pq_encode(x, cb, want_err=return_error)
    finally:
        metric._Pool.release(eng)
    if bad:
        raise ValueError("%d feature rows are not finite" % bad)
    return (codes, err) if return_error else codes


def sign_codes(codes, codebooks):
    """uint64 [N, ceil(b / 64)]: the packed sign codes hg_set_database_pq derives (bit k = decoded feature k > 0) -- from the codewords'
    sign patterns, like the loader: metric.pack_codes(decode(codes, codebooks) > 0) without the decoded table."""
    c, cb = check_tables(codes, codebooks)
    M, _, dsub = cb.shape
    b = M * dsub
    pos = cb > 0                                         # [M, K, dsub]: the sign patterns
    out = np.zeros((c.shape[0], (b + 63) // 64), dtype=np.uint64)
    for m in range(M):
        for j in range(dsub):
            k = m * dsub + j
            out[:, k // 64] |= pos[m, c[:, m], j].astype(np.uint64) << np.uint64(k % 64)
    return out

"""The identity the asymmetric ranking (hg_topr_asym / hg_map_asym) rests on, checked on the host.

s(q, n) is defined as the float32 fma chain acc = fmaf(q_k, x_nk, acc), k ascending from +0.0, then + 0.0, with x_nk = +-1.0f.  With a
factor of +-1 the product is exact, so each step is one correctly rounded addition: the chain equals the plain running float32 sum
acc = float32(acc + x_k * q_k) bit for bit -- on ordinary values, subnormals, signed zeros and infinities alike.  That is what lets a
kernel read a code bit instead of a float, and what a kernel that adds or subtracts q_k instead of calling fma would be licensed by.

The bit convention is the loaders': bit set <=> feature > 0, so a zero feature is -1 (metric.pack_codes, the host equivalent of
hg_pack_sign_f32)."""
import warnings
import numpy as np
import pytest
from oracle import real_map as RM
from hashgan_amd import metric

Q, N = 6, 64


def _queries(rng, b):
    qf = np.tanh(rng.standard_normal((Q, b))).astype(np.float32)
    qf[1] = (rng.choice([-1, 1], b) * rng.integers(1, 900, b) * 1e-41).astype(np.float32)   # subnormals (1e-41 scale; the smallest normal is 1.2e-38)
    qf[2] = np.where(rng.random(b) < 0.5, np.float32(0.0), np.float32(-0.0))       # +-0.0 only
    qf[3, ::2] = np.where(rng.random(qf[3, ::2].shape) < 0.5, np.float32(0.0), np.float32(-0.0))   # +-0.0 among ordinary values
    qf[4, b // 2] = np.inf                                                         # one infinity
    return qf


def _table(rng, b):
    pm1 = np.where(rng.random((N, b)) < 0.5, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    pm1[0] = -1.0                                                                  # an all-minus row
    pm1[1] = 1.0                                                                   # an all-plus row
    return pm1


def _running_sum(qf, pm1):
    """acc = float32(acc + x_k * q_k), k ascending, from +0.0, then + 0.0: numpy float32 arithmetic, one rounding per step."""
    acc = np.zeros((qf.shape[0], pm1.shape[0]), dtype=np.float32)
    for k in range(qf.shape[1]):
        acc = (acc + pm1[None, :, k] * qf[:, None, k]).astype(np.float32)
    return (acc + np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("b", [1, 33, 64])
def test_fma_chain_with_unit_factors_is_the_running_float32_sum(b):
    rng = np.random.default_rng(100 + b)
    qf, pm1 = _queries(rng, b), _table(rng, b)
    assert np.any((qf[1] != 0) & (np.abs(qf[1]) < np.finfo(np.float32).tiny)), "the subnormal row holds no subnormal"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                            # (inf - inf: the NaNs are the point)
        chain = RM.inner_products(qf, pm1)
        plain = _running_sum(qf, pm1)
    assert chain.dtype == np.float32 and chain.shape == (Q, N)
    # the row with an infinity: finiteness and NaN positions, not payloads
    assert np.array_equal(np.isnan(chain[4]), np.isnan(plain[4]))
    assert np.array_equal(np.isinf(chain[4]), np.isinf(plain[4]))
    ok = ~np.isnan(chain[4])
    assert np.array_equal(chain[4][ok].view(np.uint32), plain[4][ok].view(np.uint32))
    # every other row: bit for bit, the sign of a zero included
    rows = [0, 1, 2, 3, 5]
    assert not np.isnan(chain[rows]).any()
    assert np.array_equal(chain[rows].view(np.uint32), plain[rows].view(np.uint32))
    # the all-minus and all-plus rows are the negated / plain running sum of the query itself
    own = _running_sum(qf, np.stack([-np.ones(b, np.float32), np.ones(b, np.float32)]))
    assert np.array_equal(chain[rows][:, :2].view(np.uint32), own[rows].view(np.uint32))


@pytest.mark.parametrize("b", [1, 33, 64])
def test_bit_convention_bit_set_is_plus_one_and_zero_is_minus_one(b):
    """The table the asymmetric score is defined on is where(code bit, +1, -1) of the loaders' codes: bit k of word k // 64 is
    feature k > 0; a feature of exactly 0.0 (or -0.0) packs to a clear bit and so reads as -1; pad bits are clear."""
    rng = np.random.default_rng(200 + b)
    dbf = np.tanh(rng.standard_normal((N, b))).astype(np.float32)
    dbf[rng.integers(0, N, 9), rng.integers(0, b, 9)] = 0.0
    dbf[5, 0] = -0.0
    dbf[6, b - 1] = 0.0
    words = metric.pack_codes(dbf)
    assert words.dtype == np.uint64 and words.shape == (N, (b + 63) // 64)
    k = np.arange(b)
    bits = (words[:, k // 64] >> (k % 64).astype(np.uint64)) & np.uint64(1)
    pm1 = np.where(bits == 1, np.float32(1.0), np.float32(-1.0))
    assert np.array_equal(pm1, np.where(dbf > 0, 1.0, -1.0).astype(np.float32))
    assert pm1[5, 0] == -1.0 and pm1[6, b - 1] == -1.0
    if b % 64:
        assert not (words[:, -1] >> np.uint64(b % 64)).any(), "pad bits must be clear"
    # and the score on that table is the chain on the signed features with zeros read as -1
    qf = _queries(rng, b)[:1]
    assert np.array_equal(RM.inner_products(qf, pm1).view(np.uint32), _running_sum(qf, pm1).view(np.uint32))

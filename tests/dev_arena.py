"""Device memory without a framework, for the tests of the device-array loaders and of hg_export (tests/test_dev_output_gpu.py,
tests/test_second_hand_gpu.py): one scratch allocation of a producer context, pre-filled with a canary byte.  Not a test."""
import numpy as np

from hashgan_amd import _native
from hashgan_amd.devarray import DeviceArray, DeviceOut

CANARY = 0xA5
NP = {"int64": np.int64, "int32": np.int32, "uint8": np.uint8, "float32": np.float32, "float64": np.float64}


# ------------------------------------------------------------------ device memory without a framework
class Arena:
    """One device allocation (a producer context's scratch slot), filled with the canary byte, from which destinations are carved with
    64 bytes of canary before and after each; read back whole."""

    def __init__(self, nbytes):
        self.ctx = _native.Context()
        self.cap = int(nbytes) + 256
        self.base = self.ctx.scratch(0, self.cap)
        assert self.base % 64 == 0
        self.reset()

    def reset(self, byte=CANARY):
        self.host = np.full(self.cap, byte, np.uint8)
        self.ctx.memcpy_htod(self.base, self.host, self.cap)
        self.top, self.placed = 64, []

    def take(self, nbytes):
        """-> offset of `nbytes` at a multiple of 64, with 64 bytes of canary on either side."""
        off = self.top
        self.top = (off + int(nbytes) + 64 + 63) // 64 * 64
        assert self.top <= self.cap, "arena too small"
        return off

    def out(self, shape, dtype, strides=None, skip=0, stream=None):
        """A destination of `shape`, strides in elements (None: contiguous), its first element `skip` elements behind a 64-byte
        boundary -> DeviceOut."""
        isz = NP[dtype]().itemsize
        rs, cs = strides or (shape[1], 1)
        extent = ((shape[0] - 1) * rs + (shape[1] - 1) * cs + 1 + skip) * isz
        off = self.take(extent) + skip * isz
        return DeviceOut(self.base + off, shape, (rs, cs), dtype, stream)

    def expect(self, dst, want):
        """The bytes `dst` must hold after the export: `want` (shape of dst, its dtype) at the addressed elements."""
        dt = np.dtype(NP[dst.dtype])
        want = np.asarray(want)
        assert want.shape == dst.shape and want.dtype == dt, (want.shape, want.dtype, dst)
        off = dst.ptr - self.base
        extent = ((dst.shape[0] - 1) * dst.strides[0] + (dst.shape[1] - 1) * dst.strides[1] + 1) * dt.itemsize
        typed = self.host[off:off + extent].view(dt)
        view = np.lib.stride_tricks.as_strided(typed, dst.shape, (dst.strides[0] * dt.itemsize, dst.strides[1] * dt.itemsize))
        view[...] = want

    def read(self):
        got = np.empty(self.cap, np.uint8)
        self.ctx.memcpy_dtoh(got, self.base, self.cap)
        return got

    def check(self, what=""):
        """The whole allocation equals the expected image: the addressed elements, and the canary everywhere else."""
        got = self.read()
        if not np.array_equal(got, self.host):
            bad = np.flatnonzero(got != self.host)
            raise AssertionError("%s: %d bytes differ, the first at offset %d (got 0x%02x, expected 0x%02x)"
                                 % (what, bad.size, bad[0], got[bad[0]], self.host[bad[0]]))

    def untouched(self):
        return bool((self.read() == CANARY).all())

    def close(self):
        self.ctx.close()

    def put(self, a, dtype):
        """A host array copied into the arena (64 bytes of canary on either side) -> DeviceArray, contiguous."""
        a = np.ascontiguousarray(a)
        off = self.take(a.nbytes)
        self.host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.ctx.memcpy_htod(self.base + off, a, a.nbytes)
        return DeviceArray(self.base + off, a.shape, None, dtype)

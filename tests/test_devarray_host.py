"""Device-array descriptors without a GPU: devarray.as_device_array on stand-in objects, the routing's refusal of a table split
between host and device, and the host arithmetic of hg_dev_desc.hpp under AddressSanitizer / UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hashgan_amd import MAP
from hashgan_amd.devarray import DeviceArray, as_device_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000001000


class CAI:
    """An object that only has __cuda_array_interface__."""

    def __init__(self, shape, typestr="<f4", strides=None, version=3, ptr=PTR, **extra):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), version=version, strides=strides, **extra)


class FakeDtype:
    def __init__(self, name):
        self.name = name

    def __str__(self):
        return self.name


class FakeTensor:
    """Quacks like a torch tensor as far as as_device_array looks."""

    def __init__(self, shape, stride, dtype="torch.float32", is_cuda=True, ptr=PTR):
        self.shape, self._stride, self.dtype, self.is_cuda, self._ptr = tuple(shape), tuple(stride), FakeDtype(dtype), is_cuda, ptr

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._stride

    def __array__(self, *a, **k):                      # (np.asarray of a device tensor raises, like torch's)
        raise TypeError("can't convert a device tensor to numpy")


def fields(d):
    return d.ptr, d.shape, d.strides, d.dtype, d.stream


def test_cuda_array_interface_versions_and_strides():
    for version in (2, 3):
        d = as_device_array(CAI((37, 33), version=version))                       # strides: None = C-contiguous
        assert fields(d) == (PTR, (37, 33), (33, 1), "float32", None)
        d = as_device_array(CAI((37, 33), strides=(160, 4), version=version))     # a view of a wider allocation
        assert d.strides == (40, 1)
    d = as_device_array(CAI((33, 37), strides=(4, 132)))                          # transposed view of a [37, 33] array
    assert d.shape == (33, 37) and d.strides == (1, 33)
    d = as_device_array(CAI((37, 32), strides=(132, 4), ptr=PTR + 4))             # x[:, 1:]: the base sits 4 bytes off
    assert d.ptr == PTR + 4 and d.ptr % 16 == 4 and d.strides == (33, 1)
    d = as_device_array(CAI((37, 32), typestr="<f2", strides=(66, 2), ptr=PTR + 2))
    assert d.ptr % 4 == 2 and d.strides == (33, 1) and d.dtype == "float16" and d.itemsize == 2
    for typestr, name in (("<i8", "int64"), ("<i4", "int32"), ("|u1", "uint8"), ("|b1", "bool")):
        assert as_device_array(CAI((5, 3), typestr=typestr)).dtype == name


def test_stream_of_the_interface_and_of_the_argument():
    assert as_device_array(CAI((4, 4), stream=0x5550)).stream == 0x5550
    assert as_device_array(CAI((4, 4), stream=None)).stream is None
    assert as_device_array(CAI((4, 4), stream=1)).stream is None                  # 1: the legacy default stream
    assert as_device_array(CAI((4, 4), version=2, stream=0x5550)).stream is None  # (version 2 has no stream key)
    assert as_device_array(CAI((4, 4), stream=0x5550), stream=0x7770).stream == 0x7770
    d = DeviceArray(PTR, (4, 4))
    assert as_device_array(d) is d
    assert as_device_array(d, stream=0x7770).stream == 0x7770 and d.stream is None


def test_duck_typed_tensor_and_bfloat16():
    d = as_device_array(FakeTensor((37, 33), (33, 1), "torch.bfloat16"))
    assert fields(d) == (PTR, (37, 33), (33, 1), "bfloat16", None)
    d = as_device_array(FakeTensor((33, 37), (1, 33), "torch.float16"), stream=0x5550)
    assert d.strides == (1, 33) and d.dtype == "float16" and d.stream == 0x5550
    assert as_device_array(FakeTensor((5, 3), (3, 1), "torch.int64")).dtype == "int64"
    assert as_device_array(FakeTensor((5, 3), (3, 1), "torch.bool")).dtype == "bool"
    t = FakeTensor((5, 3), (3, 1))
    t.__cuda_array_interface__ = None                                             # the tensor route comes first
    assert as_device_array(t).dtype == "float32"


def test_host_data_gives_none():
    assert as_device_array(np.ones((3, 4), np.float32)) is None
    assert as_device_array([[1.0, 2.0]]) is None
    assert as_device_array(FakeTensor((3, 4), (4, 1), is_cuda=False)) is None


@pytest.mark.parametrize("obj, word", [
    (CAI((4, 4), mask=CAI((4, 4), typestr="|b1")), "mask"),
    (CAI((4, 4), strides=(18, 4)), "multiples of the item size"),
    (CAI((4, 4), strides=(-16, 4)), "strides"),
    (CAI((4, 4), strides=(16, 0)), "strides"),
    (CAI((16,)), "2-D"),
    (CAI((2, 2, 4)), "2-D"),
    (CAI((4, 4), typestr="<c8"), "dtype"),
    (CAI((4, 4), typestr="<f8"), "dtype"),
    (CAI((4, 4), version=1), "version"),
    (FakeTensor((4, 4), (-4, 1)), "strides"),
    (FakeTensor((16,), (1,)), "2-D"),
    (FakeTensor((4, 4), (4, 1), "torch.complex64"), "dtype"),
], ids=["mask", "odd-byte-stride", "negative-stride", "zero-stride", "1-D", "3-D", "complex", "float64", "version-1", "tensor-negative-stride",
        "tensor-1-D", "tensor-complex"])
def test_refusals_name_the_problem(obj, word):
    with pytest.raises(ValueError, match=word):
        as_device_array(obj)


def test_a_table_split_between_host_and_device_needs_no_gpu():
    q, d = np.ones((2, 8), np.float32), np.ones((5, 8), np.float32)
    ql, dl = np.ones((2, 3), np.int64), np.ones((5, 3), np.int64)
    d_dev = FakeTensor((5, 8), (8, 1))                                            # (a pointer that is never dereferenced: nothing is launched)
    with pytest.raises(ValueError, match="same side"):
        MAP(q, d_dev, ql, dl, 3)                                                  # database features on the device, labels on the host
    with pytest.raises(ValueError, match="same side"):
        MAP(q, d, FakeTensor((2, 3), (3, 1), "torch.int64"), dl, 3)               # query labels on the device, features on the host
    with pytest.raises(ValueError):
        MAP(q, d_dev, ql, FakeTensor((5, 3), (3, 1), "torch.int64"), 6)           # shapes come from the descriptors: R > N


def test_descriptor_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dev_array_check")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                         os.path.join(ROOT, "hashgan_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "dev_array_check.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "dev array check ok" in run.stdout, run.stdout + run.stderr

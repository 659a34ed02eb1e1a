"""Device-array OUTPUTS without a GPU: devarray.as_device_output on stand-in objects, the declarations of hg_export in the header and
the binding, and the destination arithmetic of hg_dev_desc.hpp under AddressSanitizer / UBSan (a stand-alone program)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hashgan_amd import _native
from hashgan_amd.devarray import ITEMSIZE, DeviceArray, DeviceOut, as_device_array, as_device_output

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000001000


class CAI:
    """An object that only has __cuda_array_interface__."""

    def __init__(self, shape, typestr="<f4", strides=None, version=3, ptr=PTR, readonly=False, **extra):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, readonly), version=version, strides=strides, **extra)


class FakeDtype:
    def __init__(self, name):
        self.name = name

    def __str__(self):
        return self.name


class FakeTensor:
    """Quacks like a torch tensor as far as as_device_output looks."""

    def __init__(self, shape, stride, dtype="torch.float32", is_cuda=True, ptr=PTR):
        self.shape, self._stride, self.dtype, self.is_cuda, self._ptr = tuple(shape), tuple(stride), FakeDtype(dtype), is_cuda, ptr

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._stride


def fields(d):
    return d.ptr, d.shape, d.strides, d.dtype, d.stream


def test_interface_dtypes_strides_and_float64():
    for typestr, name, isz in (("<i8", "int64", 8), ("<i4", "int32", 4), ("|u1", "uint8", 1), ("|b1", "bool", 1), ("<f4", "float32", 4),
                               ("<f8", "float64", 8)):
        d = as_device_output(CAI((5, 3), typestr=typestr))
        assert isinstance(d, DeviceOut) and fields(d) == (PTR, (5, 3), (3, 1), name, None) and d.itemsize == isz
    d = as_device_output(CAI((5, 37), "<i8", strides=(320, 8)))                        # a view of a wider allocation
    assert d.strides == (40, 1)
    d = as_device_output(CAI((37, 5), "<i8", strides=(8, 296)))                        # transposed view of a [5, 37] array
    assert d.shape == (37, 5) and d.strides == (1, 37)
    d = as_device_output(CAI((5, 36), "<f8", strides=(296, 8), ptr=PTR + 8))           # x[:, 1:] of float64: the base sits 8 bytes off
    assert d.ptr % 16 == 8 and d.strides == (37, 1) and d.dtype == "float64"
    assert as_device_output(CAI((5, 3), stream=0x5550)).stream == 0x5550               # the consumer's stream
    assert as_device_output(CAI((5, 3), stream=0x5550), stream=0x7770).stream == 0x7770
    assert as_device_output(CAI((5, 3), stream=1)).stream is None


def test_one_dimensional_arrays_are_columns():
    d = as_device_output(CAI((7,), "<f8"))
    assert fields(d) == (PTR, (7, 1), (1, 1), "float64", None)
    d = as_device_output(CAI((7,), "<f8", strides=(24,)))                              # ap[::3]
    assert d.shape == (7, 1) and d.strides == (3, 1)
    d = as_device_output(FakeTensor((7,), (1,), "torch.float64"))
    assert fields(d) == (PTR, (7, 1), (1, 1), "float64", None)
    d = as_device_output(FakeTensor((7,), (2,), "torch.int64"), stream=0x5550)
    assert d.shape == (7, 1) and d.strides == (2, 1) and d.dtype == "int64" and d.stream == 0x5550


def test_tensors_and_descriptors():
    d = as_device_output(FakeTensor((5, 37), (37, 1), "torch.int64"))
    assert fields(d) == (PTR, (5, 37), (37, 1), "int64", None)
    assert as_device_output(FakeTensor((37, 5), (1, 37), "torch.bool")).strides == (1, 37)
    assert as_device_output(FakeTensor((5, 1), (1, 1), "torch.double")).dtype == "float64"
    o = DeviceOut(PTR, (5, 3), None, "float64")
    assert as_device_output(o) is o and o.itemsize == 8 and "DeviceOut" in repr(o)
    assert as_device_output(o, stream=0x7770).stream == 0x7770 and o.stream is None
    a = DeviceArray(PTR, (5, 3), (4, 1), "int32", 0x5550)
    d = as_device_output(a)                                                            # an input descriptor names the same memory
    assert isinstance(d, DeviceOut) and fields(d) == (PTR, (5, 3), (4, 1), "int32", 0x5550)
    with pytest.raises(ValueError, match="dtype"):
        DeviceOut(PTR, (5, 3), None, "complex64")
    with pytest.raises(ValueError, match="strides"):
        DeviceOut(PTR, (5, 3), (-3, 1), "float64")
    with pytest.raises(ValueError, match="null"):
        DeviceOut(0, (5, 3), None, "float64")


@pytest.mark.parametrize("obj, word", [
    (CAI((4, 4), readonly=True), "read-only"),
    (CAI((4, 4), mask=CAI((4, 4), typestr="|b1")), "mask"),
    (CAI((4, 4), strides=(-16, 4)), "strides"),
    (CAI((4, 4), strides=(16, 0)), "strides"),
    (CAI((4, 4), strides=(18, 4)), "multiples of the item size"),
    (CAI((2, 2, 4)), "2-D"),
    (CAI((4, 4), typestr="<c8"), "dtype"),
    (CAI((4, 4), version=1), "version"),
    (FakeTensor((4, 4), (-4, 1)), "strides"),
    (FakeTensor((4, 4), (4, 0)), "strides"),
    (FakeTensor((2, 2, 4), (8, 4, 1)), "2-D"),
    (FakeTensor((4, 4), (4, 1), "torch.complex64"), "dtype"),
    (np.ones((3, 4), np.float32), "host data"),
    ([[1.0, 2.0]], "host data"),
    (FakeTensor((3, 4), (4, 1), is_cuda=False), "host data"),
], ids=["read-only", "mask", "negative-stride", "zero-stride", "odd-byte-stride", "3-D", "complex", "version-1", "tensor-negative-stride",
        "tensor-zero-stride", "tensor-3-D", "tensor-complex", "numpy", "list", "cpu-tensor"])
def test_refusals_name_the_problem(obj, word):
    with pytest.raises(ValueError, match=word):
        as_device_output(obj)


def test_inputs_still_refuse_float64():
    assert "float64" not in ITEMSIZE and "float64" in DeviceOut.ITEMSIZE
    with pytest.raises(ValueError, match="dtype"):
        as_device_array(CAI((4, 4), typestr="<f8"))                                    # (nobody widens the wrong table)


def test_header_and_binding_declare_the_export():
    src = open(os.path.join(ROOT, "include", "hashgan_amd.h")).read()
    assert re.search(r"\bint\s+hg_export\s*\(\s*hg_ctx\s*\*\s*\w+\s*,\s*const\s+hg_export_item\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s+hg_export_item\s*\{\s*int\s+what\s*;\s*hg_dev_array\s+dst\s*;\s*\}\s*hg_export_item\s*;", src)
    defines = dict((k, int(v)) for k, v in re.findall(r"^#define\s+(HG_OUT_[A-Z]+|HG_F64|HG_U8)\s+(\d+)", src, flags=re.M))
    assert defines == dict(HG_U8=5, HG_F64=6, HG_OUT_IDX=0, HG_OUT_DIST=1, HG_OUT_SCORE=2, HG_OUT_MATCH=3, HG_OUT_AP=4, HG_OUT_HITS=5,
                           HG_OUT_GRADES=6)
    for name, value in defines.items():
        assert getattr(_native, name) == value, name
    assert _native.DEV_DTYPES["float64"] == _native.HG_F64
    assert _native.OUT_ITEMS == dict(idx=0, dist=1, score=2, match=3, ap=4, hits=5, grades=6)
    assert "hg_export" in _native.EXPORTS and hasattr(_native.Context, "export")
    # the struct the binding passes has the header's layout: {int what; hg_dev_array dst}
    assert [f[0] for f in _native.ExportItemStruct._fields_] == ["what", "dst"]
    assert _native.ExportItemStruct.dst.offset == 8 and _native.ExportItemStruct.dst.size == 56       # (an 8-byte aligned struct behind an int)


def test_destination_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dev_out_check")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                         os.path.join(ROOT, "hashgan_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "dev_out_check.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "dev out check ok" in run.stdout, run.stdout + run.stderr

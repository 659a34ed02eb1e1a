"""Arrays that already lie in GPU memory, described without importing the framework that owns them.

A training process produces its features on the GPU the metric runs on (main.py:151-164: forward_all(), then the metric).
`as_device_array` turns what such a caller holds into a `DeviceArray` -- address, shape, strides in ELEMENTS, dtype name, producer
stream -- which the library packs straight out of the caller's memory (hg_set_database_dev / hg_set_queries_dev); host data gives
None and goes the NumPy way.  Nothing here touches the GPU or imports torch.
"""
import re

# dtype name -> item size in bytes: what the library's kernels read (features: the float types; labels: the rest and float32)
ITEMSIZE = {"float32": 4, "float16": 2, "bfloat16": 2, "int64": 8, "int32": 4, "uint8": 1, "bool": 1}
# __cuda_array_interface__ type strings (NumPy's array-interface codes; bfloat16 has none)
_TYPESTR = {"f4": "float32", "f2": "float16", "i8": "int64", "i4": "int32", "u1": "uint8", "b1": "bool"}


class DeviceArray:
    """A 2-D array in device memory: `ptr` (int address), `shape` (rows, cols), `strides` (row, col) in elements, both >= 1,
    `dtype` (a key of ITEMSIZE), `stream` (the producer's hipStream_t as an int; 0 / None = the null stream).

    The library orders its reads behind everything enqueued so far on `stream`, and has copied what it needs when the load
    returns: the memory may be overwritten or freed afterwards."""
    __slots__ = ("ptr", "shape", "strides", "dtype", "stream")

    def __init__(self, ptr, shape, strides=None, dtype="float32", stream=None):
        shape = tuple(int(s) for s in shape)
        if len(shape) != 2:
            raise ValueError("device arrays must be 2-D [n, width] (got %d-D)" % len(shape))
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError("device arrays must have at least one row and one column (got shape %r)" % (shape,))
        dtype = str(dtype)
        if dtype not in ITEMSIZE:
            raise ValueError("unsupported device dtype %r (supported: %s)" % (dtype, ", ".join(sorted(ITEMSIZE))))
        strides = (shape[1], 1) if strides is None else tuple(int(s) for s in strides)
        if len(strides) != 2:
            raise ValueError("device arrays need one stride per dimension (got %r)" % (strides,))
        if strides[0] < 1 or strides[1] < 1:
            # (a one-row or one-column view may carry any stride: it is never applied)
            fixed = tuple(1 if (s < 1 and n == 1) else s for s, n in zip(strides, shape))
            if fixed[0] < 1 or fixed[1] < 1:
                raise ValueError("negative or zero strides %r are not supported: make the array contiguous first" % (strides,))
            strides = fixed
        if not ptr:
            raise ValueError("device array with a null pointer")
        self.ptr, self.shape, self.strides, self.dtype = int(ptr), shape, strides, dtype
        self.stream = int(stream) if stream else None

    @property
    def ndim(self):
        return 2

    @property
    def itemsize(self):
        return ITEMSIZE[self.dtype]

    def __repr__(self):
        return "DeviceArray(ptr=0x%x, shape=%r, strides=%r, dtype=%s, stream=%r)" % (self.ptr, self.shape, self.strides, self.dtype,
                                                                                   self.stream)


class DeviceOut(DeviceArray):
    """A 2-D array in device memory that the library WRITES (Context.export, MAPs.rank_into): DeviceArray's fields and rules, with
    float64 among the dtypes (per-query AP).  `stream` is the CONSUMER's: the library's writes wait for everything enqueued so far
    on it, and whatever is enqueued on it after the call sees the data.  The memory must stay allocated until then."""
    __slots__ = ()
    ITEMSIZE = dict(ITEMSIZE, float64=8)

    def __init__(self, ptr, shape, strides=None, dtype="float32", stream=None):
        dtype = str(dtype)
        if dtype not in self.ITEMSIZE:
            raise ValueError("unsupported device dtype %r (supported: %s)" % (dtype, ", ".join(sorted(self.ITEMSIZE))))
        # (float64 is laid out like int64: the base class checks shape, strides and pointer)
        DeviceArray.__init__(self, ptr, shape, strides, "int64" if dtype == "float64" else dtype, stream)
        self.dtype = dtype

    @property
    def itemsize(self):
        return self.ITEMSIZE[self.dtype]

    def __repr__(self):
        return "DeviceOut" + DeviceArray.__repr__(self)[len("DeviceArray"):]


def _from_cuda_array_interface(obj, cai, stream, out=False):
    """out: a destination -- float64 and 1-D [n] (taken as [n, 1]) are accepted, a read-only array is refused."""
    version = int(cai.get("version", 0))
    if version not in (2, 3):
        raise ValueError("__cuda_array_interface__ version %r is not supported (2 or 3)" % cai.get("version"))
    if cai.get("mask") is not None:
        raise ValueError("masked device arrays are not supported")
    sizes = DeviceOut.ITEMSIZE if out else ITEMSIZE
    typestr = str(cai["typestr"])
    name = _TYPESTR.get(typestr[1:]) if typestr[:1] in "<|=" else None
    if name is None and out and typestr[:1] in "<|=" and typestr[1:] == "f8":
        name = "float64"
    if name is None:
        raise ValueError("unsupported device dtype %r (supported: %s)" % (typestr, ", ".join(sorted(sizes))))
    if out and cai["data"][1]:
        raise ValueError("the device array is read-only: it cannot be written")
    shape = tuple(cai["shape"])
    strides = cai.get("strides")
    if out and len(shape) == 1:
        shape = (shape[0], 1)
        strides = None if strides is None else (strides[0], sizes[name])
    if len(shape) != 2:
        raise ValueError("device arrays must be 2-D [n, width] (got %d-D)" % len(shape))
    isz = sizes[name]
    if strides is not None:
        if any(int(s) % isz for s in strides):
            raise ValueError("byte strides %r are not multiples of the item size %d" % (tuple(strides), isz))
        strides = tuple(int(s) // isz for s in strides)
    ptr = cai["data"][0]
    if stream is None and version >= 3:
        # v3: None = no synchronisation needed, 1 = the legacy default stream, 2 = the per-thread default stream, else a handle
        s = cai.get("stream")
        stream = None if s in (None, 1) else int(s)
    return (DeviceOut if out else DeviceArray)(ptr, shape, strides, name, stream)


def _from_tensor(obj, stream, out=False):
    sizes = DeviceOut.ITEMSIZE if out else ITEMSIZE
    m = re.search(r"(\w+)$", str(obj.dtype))           # 'torch.bfloat16' -> 'bfloat16'
    name = m.group(1) if m else str(obj.dtype)
    name = {"float": "float32", "half": "float16", "long": "int64", "int": "int32", "double": "float64"}.get(name, name)
    if name not in sizes:
        raise ValueError("unsupported device dtype %s (supported: %s)" % (obj.dtype, ", ".join(sorted(sizes))))
    shape, strides = tuple(obj.shape), tuple(obj.stride())
    if out and len(shape) == 1:
        shape, strides = (shape[0], 1), (strides[0], 1)
    if len(shape) != 2:
        raise ValueError("device arrays must be 2-D [n, width] (got %d-D)" % len(shape))
    return (DeviceOut if out else DeviceArray)(obj.data_ptr(), shape, strides, name, stream)


def as_device_array(obj, stream=None):
    """-> DeviceArray for data in GPU memory, None for host data (NumPy arrays, lists, CPU tensors).

    Accepted: a DeviceArray; an object with `__cuda_array_interface__` (version 2 or 3; byte strides must be multiples of the item
    size, `strides: None` means C-contiguous, the `stream` key of version 3 is honoured, a mask is refused); a tensor-like object
    whose `is_cuda` is true, with `data_ptr()`, `stride()`, `shape` and `dtype` -- the dtype is read from `str(dtype)`, which is how
    bfloat16 arrives (it has no array-interface type string).  2-D only, strides >= 1, dtypes of ITEMSIZE; anything else raises
    ValueError naming the problem.

    `stream`: the HIP stream (an int handle) on which the producer's work was enqueued; it overrides the interface's own.  The
    default is the null stream, which is ordered after every BLOCKING stream of the process -- torch's default stream included.
    Work queued on a NON-BLOCKING side stream (torch.cuda.Stream()) is not ordered with the null stream: pass that stream's handle
    (torch.cuda.current_stream().cuda_stream), or synchronise it first."""
    if isinstance(obj, DeviceArray):
        if stream is not None and stream != obj.stream:
            return DeviceArray(obj.ptr, obj.shape, obj.strides, obj.dtype, stream)
        return obj
    if getattr(obj, "is_cuda", None) is True and hasattr(obj, "data_ptr"):
        return _from_tensor(obj, stream)
    if getattr(obj, "is_cuda", None) is False:
        return None                                    # a CPU tensor: np.asarray takes it
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is not None:
        return _from_cuda_array_interface(obj, cai, stream)
    return None


def as_device_output(obj, stream=None):
    """-> DeviceOut for an array in GPU memory that the library is to write.  The spellings of as_device_array: a DeviceOut; an object
    with `__cuda_array_interface__` (refused when its `data` says read-only); a tensor-like object whose `is_cuda` is true.  float64 is
    accepted (per-query AP), and a 1-D array of length n is taken as [n, 1] (torch users hold AP as [Q]).  There is no host route:
    host data raises ValueError, like everything as_device_array refuses.

    `stream`: the CONSUMER's HIP stream (an int handle); it overrides the interface's own.  The library's writes are ordered behind
    what is enqueued on it so far, and what is enqueued on it afterwards sees the data.  The default is the null stream; work on a
    NON-BLOCKING stream (torch.cuda.Stream()) is only ordered if its handle is passed (torch.cuda.current_stream().cuda_stream)."""
    if isinstance(obj, DeviceOut):
        if stream is not None and stream != obj.stream:
            return DeviceOut(obj.ptr, obj.shape, obj.strides, obj.dtype, stream)
        return obj
    if isinstance(obj, DeviceArray):
        return DeviceOut(obj.ptr, obj.shape, obj.strides, obj.dtype, obj.stream if stream is None else stream)
    if getattr(obj, "is_cuda", None) is True and hasattr(obj, "data_ptr"):
        return _from_tensor(obj, stream, out=True)
    cai = None if getattr(obj, "is_cuda", None) is False else getattr(obj, "__cuda_array_interface__", None)
    if cai is not None:
        return _from_cuda_array_interface(obj, cai, stream, out=True)
    raise ValueError("results are written into device memory only: %s is host data (a DeviceOut, a device tensor or an object with "
                     "__cuda_array_interface__ is needed)" % type(obj).__name__)

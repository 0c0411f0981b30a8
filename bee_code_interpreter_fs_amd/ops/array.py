"""``DeviceArray``: a minimal numpy-like array in MI355X HBM, driven by the
hand-written beekern kernels.

Sandboxed user code calls these in place of numpy (BASELINE.json north
star).  The benchmark payload `examples/benchmark-numpy.py:18-22` becomes::

    import beekern as bk
    x = bk.random.rand(10**8)          # Philox kernel, f64, stays in HBM
    result = bk.sum(bk.square(x))      # fused square+sum: one HBM read pass

Comparisons (``x < 0.5``, ``bk.less_equal(a, b)``) return ``bool`` masks, one
byte per element as numpy's; a mask is *lazy* too: ``sum`` / ``mean`` /
``count_nonzero`` / ``any`` / ``all`` of it count in one fused pass over the
operands (no mask written), any other use (``where``, ``x[mask]``, ``&``)
materialises it.

``median`` / ``percentile`` / ``quantile`` / ``histogram`` summarise a whole
array without sorting or copying it (``csrc/kernels/stats.hip``: a radix
select of a few ranks, a histogram counted in LDS); they read a ``.T`` view in
place and return host scalars / ndarrays typed as numpy's.

``sort`` / ``argsort`` (1-D, always stable), ``argmax`` / ``argmin`` (the flat
index) and ``take`` / ``x[idx]`` (1-D, by an int64 index array) order and
reorder arrays on the device (``csrc/kernels/sort.hip``), in numpy's order:
NaNs last, ``-0.0 == +0.0``, ties in index order.

2-D arrays: the binary operations broadcast an ``(R, C)`` array against a
``(C,)``, ``(1, C)`` or ``(R, 1)`` one of the same dtype in one pass, and
``amax`` / ``amin`` / ``var`` / ``std`` (like ``sum`` / ``mean``) reduce along
an axis, with ``keepdims`` (``csrc/kernels/axis.hip``; f32 / f64, ``.T`` views
read in place).

``square`` (and ``x * x`` / ``x ** 2``) returns a *lazy* array: if the only
consumer is a reduction the square is fused into it (no 800 MB temporary);
any other use materialises it with the elementwise kernel.

Kernels run through a driver (``ops/driver.py``): in-process HIP (native) or
the executor's kernel broker (light sandboxes, no HIP context of their own).
"""

from __future__ import annotations

import math
import os
import struct
import threading
import weakref
from typing import Any, Optional, Sequence, Tuple

from ._lazy import is_integer, is_number, np, numpy_loaded, scalar
from ._native import DTYPE_CODES, DTYPE_SIZES, BeekernError, QuotaExceeded  # noqa: F401
from .driver import (DIST_BETA, DIST_CAUCHY, DIST_EXPONENTIAL, DIST_GAMMA, DIST_GUMBEL, DIST_LAPLACE, DIST_LOGISTIC,
                     DIST_LOGNORMAL, DIST_PARETO, DIST_RAYLEIGH, DIST_STUDENT_T, DIST_WEIBULL, RINT_BINOMIAL,
                     RINT_GEOMETRIC, RINT_INTEGERS, RINT_POISSON, make_driver)

Shape = Tuple[int, ...]

_UNARY = {
    "square": 0, "abs": 1, "negative": 2, "sqrt": 3, "exp": 4, "log": 5, "relu": 6,
    "sin": 7, "cos": 8, "tanh": 9, "sigmoid": 10, "copy": 11,
}
_BINARY = {"add": 0, "subtract": 1, "multiply": 2, "divide": 3, "maximum": 4, "minimum": 5, "power": 6}
_REDUCE = {"sum": 0, "square_sum": 1, "abs_sum": 2, "max": 3, "min": 4, "dot": 5, "max_abs_diff": 6}
# (max and min of a mask are any and all, as 0.0 / 1.0)
_COMPARE = {"less": 0, "less_equal": 1, "greater": 2, "greater_equal": 3, "equal": 4, "not_equal": 5}
_FLIPPED = {0: 2, 1: 3, 2: 0, 3: 1, 4: 4, 5: 5}  # s OP x  ==  x FLIPPED[OP] s
_LOGICAL = {"logical_and": 0, "logical_or": 1, "logical_xor": 2, "logical_not": 3}
_SUPPORTED = ("float32", "float64", "bfloat16", "bool", "int64")
_FLOATS = ("float32", "float64", "bfloat16")
# int64 arrays (csrc/kernels/integer.hip): op codes of bk_int_binary / bk_int_reduce
_INT_BINARY = {"add": 0, "subtract": 1, "multiply": 2, "floor_divide": 3, "remainder": 4, "maximum": 5, "minimum": 6}
_INT_REDUCE = {"sum": 0, "max": 1, "min": 2}
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1

_state_lock = threading.Lock()
_driver = None


def normalize_dtype(dtype: Any) -> str:
    if dtype is None:
        return "float64"
    if dtype is bool:
        return "bool"
    if isinstance(dtype, str):
        name = {"bf16": "bfloat16", "f32": "float32", "f64": "float64", "double": "float64", "float": "float64"}.get(
            dtype, dtype
        )
    else:
        name = str(getattr(dtype, "name", None) or np.dtype(dtype).name)
        name = name.replace("torch.", "")
    if name not in _SUPPORTED:
        raise TypeError(f"unsupported dtype {dtype!r}; beekern supports {_SUPPORTED}")
    return name


def init(device: Optional[int] = None, lazy: bool = False) -> int:
    """Initialise the driver (HIP context on ``device``, or a broker session);
    idempotent.  Sandboxes do this while waiting in the warm pool.  ``lazy``
    (broker driver only) defers opening the session to the first request."""
    global _driver
    if _driver is not None:
        return _driver.device
    with _state_lock:
        if _driver is None:
            d = make_driver()
            dev = int(os.environ.get("BEE_DEVICE", "0")) if device is None else int(device)
            if lazy and d.name == "broker":
                d.init(dev, lazy=True)
            else:
                d.init(dev)
            _driver = d
    return _driver.device


def driver():
    if _driver is None:
        init()
    return _driver


def driver_name() -> str:
    return driver().name


def is_initialized() -> bool:
    return _driver is not None


def synchronize() -> None:
    if _driver is not None:
        _driver.sync()


def memory_stats() -> dict:
    return driver().memory_stats()


def set_quota(nbytes: int) -> None:
    driver().set_quota(int(nbytes))


def empty_cache() -> None:
    driver().empty_cache()


def device_info() -> dict:
    return driver().device_info()


class _Buffer:
    """Owns one device allocation (pointer or broker handle)."""

    __slots__ = ("ptr", "nbytes", "_owner", "_drv", "_readers", "__weakref__")

    def __init__(self, nbytes: int, ptr: Optional[int] = None, owner: Any = None) -> None:
        self.nbytes = int(nbytes)
        self._readers = None  # lazy masks that still have to read this buffer (a WeakSet, on first use)
        self._owner = owner
        self._drv = driver()
        self.ptr = int(ptr) if ptr is not None else self._drv.malloc(max(self.nbytes, 1))

    def __del__(self) -> None:
        if self._owner is None and getattr(self, "ptr", 0):
            try:
                self._drv.free(self.ptr)
            except Exception:
                pass


class DeviceArray:
    """Contiguous row-major array in device memory (or a lazy unary view)."""

    __array_priority__ = 1000

    def __init__(self, shape: Sequence[int], dtype: str, buffer: Optional[_Buffer] = None, lazy=None, strides_t=False):
        self.shape: Shape = tuple(int(s) for s in shape)
        self.dtype = normalize_dtype(dtype)
        # until materialised: ("square", src), ("rand", kind, seed, offset,
        # lo, hi) -- a draw whose values are fixed by its counter range -- or
        # ("cmp", op, a, b_or_scalar): a mask of a comparison not yet run
        self._lazy = lazy
        self._transposed = strides_t  # 2-D transposed view of a contiguous buffer
        if buffer is None and lazy is None:
            buffer = _Buffer(self.nbytes)
        self._buf = buffer

    @property
    def size(self) -> int:
        return int(math.prod(self.shape)) if self.shape else 1

    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def itemsize(self) -> int:
        return DTYPE_SIZES[self.dtype]

    @property
    def nbytes(self) -> int:
        return self.size * self.itemsize

    @property
    def ptr(self) -> int:
        self._materialize()
        return self._buf.ptr  # type: ignore[union-attr]

    @property
    def code(self) -> int:
        return DTYPE_CODES[self.dtype]

    def __len__(self) -> int:
        if not self.shape:
            raise TypeError("len() of a 0-d array")
        return self.shape[0]

    def __repr__(self) -> str:
        kind = "lazy " if self._lazy else ""
        return f"DeviceArray({kind}shape={self.shape}, dtype={self.dtype})"

    def _materialize(self) -> "DeviceArray":
        if self._lazy is not None:
            if self._lazy[0] == "rand":
                _, kind, seed, off, lo, hi = self._lazy
                self._buf = _Buffer(self.nbytes)
                driver().rand(kind, self._buf.ptr, self.size, self.code, seed, off, lo, hi)
            elif self._lazy[0] == "cmp":
                _, op, a, b = self._lazy
                self._buf = _Buffer(self.nbytes)
                if isinstance(b, DeviceArray):
                    driver().compare(op, a.code, 0, a.ptr, b.ptr, 0.0, self._buf.ptr, self.size)
                else:
                    driver().compare(op, a.code, 1, a.ptr, 0, b, self._buf.ptr, self.size)
            else:
                op, src = self._lazy
                self._buf = _Buffer(self.nbytes)
                driver().unary(_UNARY[op], self.code, src.ptr, self._buf.ptr, self.size)
            self._lazy = None
        if self._transposed:
            rows, cols = self.shape[1], self.shape[0]  # underlying buffer is (rows, cols)
            src = self._buf
            out = _Buffer(self.nbytes)  # on-device transpose, 2/4/8-byte elements
            driver().transpose(src.ptr, out.ptr, rows, cols, cols, rows, self.code, self.code)
            self._buf = out
            self._transposed = False
        return self

    def numpy(self) -> np.ndarray:
        self._materialize()
        return _download(self._buf, self.shape, self.dtype)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a.astype(dtype) if dtype is not None else a

    # numpy functions and ufuncs on a device array run on the kernels where
    # one computes what numpy would; the rest copy to the host once, with a
    # warning (ops/npinterop.py) -- not silently through __array__
    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        from .npinterop import array_ufunc

        return array_ufunc(_binding(), ufunc, method, inputs, kwargs)

    def __array_function__(self, func, types, args, kwargs):
        from .npinterop import array_function

        return array_function(_binding(), func, types, args, kwargs)

    def tolist(self):
        return self.numpy().tolist()

    def item(self):
        if self.size != 1:
            raise ValueError("item() needs a size-1 array")
        return self.numpy().reshape(()).item()

    def __float__(self) -> float:
        return float(self.item())

    def reshape(self, *shape) -> "DeviceArray":
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        shape = list(shape)
        if -1 in shape:
            known = math.prod(s for s in shape if s != -1)
            shape[shape.index(-1)] = self.size // max(known, 1)
        if math.prod(shape) != self.size:
            raise ValueError(f"cannot reshape {self.shape} to {tuple(shape)}")
        self._materialize()
        return DeviceArray(shape, self.dtype, buffer=self._buf)

    @property
    def T(self) -> "DeviceArray":
        _no_int64("T", self)
        if self.ndim != 2:
            raise ValueError("T needs a 2-D array")
        self._materialize()
        return DeviceArray((self.shape[1], self.shape[0]), self.dtype, buffer=self._buf, strides_t=True)

    def astype(self, dtype) -> "DeviceArray":
        dt = normalize_dtype(dtype)
        if dt == self.dtype:
            return self.copy()
        if "int64" in (dt, self.dtype):
            return _int_astype(self, dt)
        if "bool" in (dt, self.dtype):
            if dt not in ("float32", "float64"):
                raise TypeError(f"beekern astype: {self.dtype} -> {dt} has no kernel (bool converts to float32 / float64)")
            if driver().name == "broker":
                # the broker's CAST frame knows float dtypes only
                # (broker_core.cpp dtype_size): the same values through WHERE
                return where(self, 1.0, 0.0, dtype=dt)
        self._materialize()
        out = DeviceArray(self.shape, dt)
        driver().cast(self.code, out.code, self.ptr, out.ptr, self.size)
        return out

    def copy(self) -> "DeviceArray":
        if self.dtype in ("bool", "int64"):
            out = DeviceArray(self.shape, self.dtype)
            driver().copy(out.ptr, self.ptr, self.nbytes)
            return out
        return _unary("copy", self)

    def any(self) -> bool:
        return any(self)

    def all(self) -> bool:
        return all(self)

    def __getitem__(self, key) -> "DeviceArray":
        """``x[mask]``: the elements where the bool array ``mask`` (of x's
        shape) is true, 1-D in C order.  ``x[idx]`` of a 1-D array: ``take(x, idx)`` for an int64
        DeviceArray or a host integer list / ndarray.  No other indexing on the device."""
        if isinstance(key, DeviceArray) and key.dtype == "int64" and self.ndim == 1:
            return take(self, key)
        if self.ndim == 1 and _is_host_index(key):
            return take(self, key)
        if not isinstance(key, DeviceArray) or key.dtype != "bool":
            raise TypeError("beekern arrays are indexed by a bool DeviceArray of the same shape only")
        if key.shape != self.shape:
            raise TypeError(f"beekern x[mask]: the mask's shape {key.shape} is not the array's {self.shape}")
        count = count_nonzero(key)  # (a lazy mask: the fused count)
        out = DeviceArray((count,), self.dtype)
        if count:
            # (int64 elements move by size, as float64's)
            driver().compress(_bits_code(self), self.ptr, key.ptr, self.size, out.ptr, count)
        return out

    def argsort(self, kind=None) -> "DeviceArray":
        return argsort(self, kind)

    def argmax(self, axis=None):
        return argmax(self, axis)

    def argmin(self, axis=None):
        return argmin(self, axis)

    def sum(self, axis: Optional[int] = None, keepdims: bool = False):
        return sum(self, axis, keepdims)

    def mean(self, axis: Optional[int] = None, keepdims: bool = False):
        return mean(self, axis, keepdims)

    def max(self, axis: Optional[int] = None, keepdims: bool = False):
        if axis is None and not keepdims and self.dtype != "int64":
            return _reduce("max", self)
        return amax(self, axis, keepdims)

    def min(self, axis: Optional[int] = None, keepdims: bool = False):
        if axis is None and not keepdims and self.dtype != "int64":
            return _reduce("min", self)
        return amin(self, axis, keepdims)

    def var(self, axis: Optional[int] = None, ddof=0, keepdims: bool = False):
        return var(self, axis, ddof, keepdims)

    def std(self, axis: Optional[int] = None, ddof=0, keepdims: bool = False):
        return std(self, axis, ddof, keepdims)

    def __add__(self, o): return _binary("add", self, o)
    def __radd__(self, o): return _binary("add", self, o)
    def __sub__(self, o): return _binary("subtract", self, o)
    def __rsub__(self, o): return _binary("subtract", self, o, reversed_=True)
    def __mul__(self, o):
        if o is self and self.dtype != "int64":
            return square(self)
        return _binary("multiply", self, o)
    def __rmul__(self, o): return _binary("multiply", self, o)
    def __truediv__(self, o): return _binary("divide", self, o)
    def __rtruediv__(self, o): return _binary("divide", self, o, reversed_=True)
    def __floordiv__(self, o): return floor_divide(self, o)
    def __rfloordiv__(self, o): return floor_divide(o, self)
    def __mod__(self, o): return remainder(self, o)
    def __rmod__(self, o): return remainder(o, self)
    def __pow__(self, o):
        _no_int64("power", self)
        if isinstance(o, (int, float)) and o == 2:
            return square(self)
        return _binary("power", self, o)
    def __neg__(self): return _unary("negative", self)
    def __abs__(self): return _unary("abs", self)
    def __matmul__(self, o): return matmul(self, o)
    # (== and != stay identity-based, as object's)
    def __lt__(self, o): return less(self, o)
    def __le__(self, o): return less_equal(self, o)
    def __gt__(self, o): return greater(self, o)
    def __ge__(self, o): return greater_equal(self, o)
    def __and__(self, o): return logical_and(self, o)
    def __rand__(self, o): return logical_and(o, self)
    def __or__(self, o): return logical_or(self, o)
    def __ror__(self, o): return logical_or(o, self)
    def __xor__(self, o): return logical_xor(self, o)
    def __rxor__(self, o): return logical_xor(o, self)
    def __invert__(self): return logical_not(self)


_BINDING = []


def _binding():
    """DeviceArray's plug into the numpy protocols (ops/npinterop.py)."""
    if not _BINDING:
        from .npinterop import Binding

        def mine(x):
            return isinstance(x, DeviceArray)

        _BINDING.append(Binding(dev=lambda x: x if mine(x) else None, box=lambda d: d,
                                host=lambda x: x.numpy(), is_mine=mine))
    return _BINDING[0]


def _np_dtype(dtype: str):
    return {"float32": np.float32, "float64": np.float64, "bool": np.bool_, "int64": np.int64}[dtype]


def _np_view_dtype(dtype: str):
    # (a mask's bytes come down as uint8: a buffer may hold any non-zero byte for true)
    return np.uint16 if dtype == "bfloat16" else np.uint8 if dtype == "bool" else _np_dtype(dtype)


def _download(buf: _Buffer, shape: Shape, dtype: str) -> np.ndarray:
    host = np.empty(shape, dtype=_np_view_dtype(dtype))
    driver().d2h(buf.ptr, host)
    if dtype == "bfloat16":
        return (host.astype(np.uint32) << 16).view(np.float32)
    if dtype == "bool":
        return host != 0
    return host


def _upload(host: np.ndarray, dtype: str) -> _Buffer:
    host = np.ascontiguousarray(host)
    buf = _Buffer(host.nbytes)
    driver().h2d(buf.ptr, host)
    return buf


def _f32_bits_to_bf16(u: int) -> int:
    """One f32 bit pattern -> bf16 bits, round to nearest even (NaN -> 0x7FC0),
    as _f32_to_bf16_bits does element-wise."""
    if (u & 0x7F800000) == 0x7F800000 and (u & 0x007FFFFF):
        return 0x7FC0
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def _f32_to_bf16_bits(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    out = rounded.astype(np.uint16)
    nan = np.isnan(a)
    if nan.any():
        out[nan] = 0x7FC0
    return out


# ---- constructors -------------------------------------------------------------------

def empty(shape, dtype="float64") -> DeviceArray:
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return DeviceArray(shape, dtype)


def full(shape, value: float, dtype="float64") -> DeviceArray:
    a = empty(shape, dtype)
    # the fill's bit pattern (no numpy: see ops/_lazy.py)
    if a.dtype == "bool":
        pattern, width = (1 if value else 0), 1
    elif a.dtype == "int64":
        pattern, width = _int64_scalar(value if is_integer(value) else int(value)) & 0xFFFFFFFFFFFFFFFF, 8
    elif a.dtype == "float64":
        pattern, width = struct.unpack("<Q", struct.pack("<d", float(value)))[0], 8
    elif a.dtype == "float32":
        pattern, width = struct.unpack("<I", struct.pack("<f", float(value)))[0], 4
    else:
        pattern, width = _f32_bits_to_bf16(struct.unpack("<I", struct.pack("<f", float(value)))[0]), 2
    driver().fill(a.ptr, a.nbytes, pattern, width)
    return a


def zeros(shape, dtype="float64") -> DeviceArray:
    return full(shape, 0.0, dtype)


def ones(shape, dtype="float64") -> DeviceArray:
    return full(shape, 1.0, dtype)


def asarray(obj, dtype=None) -> DeviceArray:
    if isinstance(obj, DeviceArray):
        return obj if dtype is None or normalize_dtype(dtype) == obj.dtype else obj.astype(dtype)
    if _is_torch_tensor(obj):
        return from_torch(obj) if dtype is None else from_torch(obj).astype(dtype)
    host = np.asarray(obj)
    # (integer host data becomes float64 unless int64 is asked for)
    dt = normalize_dtype(dtype if dtype is not None else (host.dtype if host.dtype.kind == "f" else "float64"))
    if dt == "bfloat16":
        buf = _upload(_f32_to_bf16_bits(host.astype(np.float32)), "bfloat16")
    else:
        buf = _upload(host.astype(_np_dtype(dt), copy=False), dt)
    return DeviceArray(host.shape, dt, buffer=buf)


from_numpy = asarray
array = asarray


def _is_torch_tensor(x) -> bool:
    t = type(x)
    return t.__module__.startswith("torch") and t.__name__ in ("Tensor", "Parameter")


def from_torch(t) -> DeviceArray:
    """Zero-copy view of a contiguous HIP torch tensor when this process owns
    the HIP context; a host copy in broker mode."""
    dt = normalize_dtype(str(t.dtype).replace("torch.", ""))
    if t.is_cuda and driver().name == "native":
        t = t.contiguous()
        return DeviceArray(tuple(t.shape), dt, buffer=_Buffer(t.numel() * t.element_size(), ptr=t.data_ptr(), owner=t))
    host = t.detach().cpu()
    if dt == "bfloat16":
        import torch

        return asarray(host.to(torch.float32).numpy(), "bfloat16")
    return asarray(host.numpy(), dt)


def to_torch(a: DeviceArray):
    import torch

    host = a.numpy()
    dt = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}[a.dtype]
    return torch.from_numpy(host).to(device="cuda", dtype=dt)


# ---- elementwise / reductions ------------------------------------------------------

def _as_operand(x) -> DeviceArray:
    return x if isinstance(x, DeviceArray) else asarray(x)


def _no_masks(what: str, *arrays) -> None:
    for a in arrays:
        if a.dtype == "bool":
            raise TypeError(f"beekern {what}: no kernel for bool arrays (masks take logical_* / where / astype)")


def _unary(op: str, x) -> DeviceArray:
    x = _as_operand(x)
    if x.dtype == "int64":
        return _int_unary(op, x)
    _no_masks(op, x)
    x._materialize()
    out = DeviceArray(x.shape, x.dtype)
    driver().unary(_UNARY[op], x.code, x.ptr, out.ptr, x.size)
    return out


def square(x) -> DeviceArray:
    """Lazy x**2: fused into a following reduction, else materialised.  A
    still-lazy uniform draw stays lazy underneath (sum(square(rand)) is one
    fused Philox->square->reduce kernel)."""
    x = _as_operand(x)
    if x.dtype == "int64":
        return _int_binary("multiply", x, x, False)
    if not _lazy_uniform(x):
        x = x._materialize()
    return DeviceArray(x.shape, x.dtype, lazy=("square", x))


def _vector_kind(matrix: DeviceArray, v: DeviceArray) -> Optional[int]:
    """How ``v`` runs along the 2-D ``matrix`` under numpy's broadcasting:
    0 for one element per column (shapes (C,) and (1, C)), 1 for one per row
    ((R, 1)), None if it is no such vector."""
    if matrix.ndim != 2:
        return None
    rows, cols = matrix.shape
    if v.shape in ((cols,), (1, cols)):
        return 0
    if v.shape == (rows, 1):
        return 1
    return None


def _broadcast_shape(s: Shape, t: Shape) -> Optional[Shape]:
    """numpy's broadcast of two shapes, or None if they do not broadcast."""
    n = max(len(s), len(t))
    s, t = (1,) * (n - len(s)) + tuple(s), (1,) * (n - len(t)) + tuple(t)
    out = []
    for p, q in zip(s, t):
        if p != q and 1 not in (p, q):
            return None
        out.append(q if p == 1 else p)
    return tuple(out)


def _broadcast(op: str, matrix: DeviceArray, v: DeviceArray, kind: int, swapped: bool) -> DeviceArray:
    """``matrix op v`` (``v op matrix`` if swapped) with ``v`` along one axis
    (bk_broadcast).  A ``.T`` view is read in place: its buffer takes the vector
    along the other axis and the result is a ``.T`` view again."""
    if matrix._lazy is not None:
        matrix._materialize()
    v._materialize()
    rows, cols = matrix.shape
    if matrix._transposed:  # the buffer is (cols, rows)
        rows, cols, kind = cols, rows, 1 - kind
    out = _Buffer(matrix.nbytes)
    if matrix.size:
        driver().broadcast(_BINARY[op], matrix.code, kind, swapped, matrix._buf.ptr, v.ptr, out.ptr,  # type: ignore[union-attr]
                           rows, cols, cols, cols)
    return DeviceArray(matrix.shape, matrix.dtype, buffer=out, strides_t=matrix._transposed)


def _binary_unequal(op: str, a: DeviceArray, b: DeviceArray, reversed_: bool) -> Optional[DeviceArray]:
    """``a op b`` (``b op a`` if reversed) for two arrays of one float dtype
    whose shapes differ but broadcast to one of them; None if they do not."""
    if a.ndim > 2 or b.ndim > 2:
        return None
    if a.size == b.size:  # e.g. (C,) with (1, C): the same elements in the same order
        shape = _broadcast_shape(a.shape, b.shape)
        if shape not in (a.shape, b.shape):
            return None
        a._materialize()
        b._materialize()
        if reversed_:
            a, b = b, a
        out = DeviceArray(shape, a.dtype)
        driver().binary(_BINARY[op], a.code, 0, a.ptr, b.ptr, 0.0, out.ptr, a.size)
        return out
    if a.dtype not in ("float32", "float64"):
        return None  # (bk_broadcast has no bf16 form)
    kind = _vector_kind(a, b)
    if kind is not None:
        return _broadcast(op, a, b, kind, reversed_)
    kind = _vector_kind(b, a)
    if kind is not None:
        return _broadcast(op, b, a, kind, not reversed_)
    return None


def _binary(op: str, a, b, reversed_: bool = False) -> DeviceArray:
    if _is_int64(a) or _is_int64(b):
        return _int_binary(op, a, b, reversed_)
    a = _as_operand(a)
    _no_masks(op, a)
    if is_number(b):
        a._materialize()
        out = DeviceArray(a.shape, a.dtype)
        driver().binary(_BINARY[op], a.code, 2 if reversed_ else 1, a.ptr, 0, float(b), out.ptr, a.size)
        return out
    b = _as_operand(b)
    _no_masks(op, b)
    if b.shape != a.shape or b.dtype != a.dtype:
        if b.size == 1:
            return _binary(op, a, float(b.item()), reversed_)
        res = _binary_unequal(op, a, b, reversed_) if b.dtype == a.dtype else None
        if res is None:
            raise ValueError(f"beekern {op}: shapes/dtypes must match ({a.shape} {a.dtype} vs {b.shape} {b.dtype})")
        return res
    a._materialize()
    b._materialize()
    if reversed_:
        a, b = b, a
    out = DeviceArray(a.shape, a.dtype)
    driver().binary(_BINARY[op], a.code, 0, a.ptr, b.ptr, 0.0, out.ptr, a.size)
    return out


def _reduce(op: str, x: DeviceArray, y: Optional[DeviceArray] = None) -> np.float64:
    return scalar(driver().reduce(_REDUCE[op], x.code, x.ptr, y.ptr if y is not None else 0, x.size))


def _lazy_uniform(x: DeviceArray) -> bool:
    # fused reductions exist for the f64 / f32 streams (bf16 draws materialise)
    return x._lazy is not None and x._lazy[0] == "rand" and x._lazy[1] == 0 and x.dtype != "bfloat16"


def _rand_reduce(op: str, x: DeviceArray) -> np.float64:
    """Reduce a still-lazy uniform draw in one fused Philox->reduce kernel
    (bk_rand_reduce): the values are the ones materialising x would store."""
    _, _, seed, off, lo, hi = x._lazy
    return scalar(driver().rand_reduce(_REDUCE[op], x.code, x.size, seed, off, lo, hi))


def _reduce_axis(op: str, x: DeviceArray, axis: int):
    """sum / mean of a 2-D array along ``axis`` (numpy semantics: axis 0
    collapses the rows -> one value per column).  f64 in -> f64 out; f32 and
    bf16 in -> f32 out; f64 accumulation (bk_reduce_axis)."""
    if x.ndim == 1:
        if axis not in (0, -1):
            raise ValueError(f"axis {axis} is out of bounds for a 1-D array")
        return sum(x) if op == "sum" else mean(x)  # numpy: a scalar
    if x.ndim != 2:
        raise ValueError("axis reductions support 1-D and 2-D arrays")
    axis = axis + 2 if axis < 0 else axis
    if axis not in (0, 1):
        raise ValueError(f"axis {axis} is out of bounds for a 2-D array")
    if x._lazy is not None:
        x._materialize()
    rows, cols = x.shape
    if x._transposed:  # a .T view: the buffer is (cols, rows) -- reduce the other way
        rows, cols, axis = cols, rows, 1 - axis
    out = DeviceArray((cols if axis == 0 else rows,), "float64" if x.dtype == "float64" else "float32")
    driver().reduce_axis(0 if op == "sum" else 1, x.code, x._buf.ptr, out.ptr, rows, cols, cols, axis)  # type: ignore[union-attr]
    return out


def _kept(res, x: DeviceArray, axis: Optional[int]):
    """``res`` with the reduced axis kept as length one (numpy's
    ``keepdims=True``): a reshape of an axis result, a one-element array of a
    whole-array one."""
    if isinstance(res, DeviceArray):
        return res.reshape(1, res.size) if (axis + 2 if axis < 0 else axis) == 0 else res.reshape(res.size, 1)
    return full((1,) * x.ndim, float(res), x.dtype)


def sum(x, axis: Optional[int] = None, keepdims: bool = False):  # noqa: A001 - numpy-compatible name
    x = _as_operand(x)
    if x.dtype == "int64":
        return _int_reduce("sum", x, axis, keepdims)
    if keepdims:
        if x.dtype == "bool":
            raise TypeError("beekern sum: keepdims of a bool array's count has no kernel")
        return _kept(sum(x, axis), x, axis)
    if x.dtype == "bool":
        if axis is not None and not (x.ndim == 1 and axis in (0, -1)):
            raise TypeError("beekern sum: axis sums of a bool array have no kernel")
        count = count_nonzero(x)
        m = numpy_loaded()
        return m.int64(count) if m is not None else count
    if axis is not None:
        return _reduce_axis("sum", x, int(axis))
    if x._lazy is not None and x._lazy[0] == "square":
        base = x._lazy[1]
        if _lazy_uniform(base):
            return _rand_reduce("square_sum", base)  # neither the draw nor x**2 materialised
        return _reduce("square_sum", base)  # fused: x**2 never materialised
    if _lazy_uniform(x):
        return _rand_reduce("sum", x)
    return _reduce("sum", x._materialize())


def square_sum(x) -> np.float64:
    x = _as_operand(x)
    if _lazy_uniform(x):
        return _rand_reduce("square_sum", x)
    return _reduce("square_sum", x._materialize())


def mean(x, axis: Optional[int] = None, keepdims: bool = False):
    """np.mean.  Of an int64 array: the exact (int64) sum divided once by the size, as a float64."""
    x = _as_operand(x)
    if x.dtype == "int64":
        if x.size == 0:
            _int_reduce("sum", x, axis, keepdims)
            return scalar(float("nan"))
        return scalar(float(_int_reduce("sum", x, axis, keepdims)) / x.size)
    if keepdims:
        if x.dtype == "bool":
            raise TypeError("beekern mean: keepdims of a bool array's mean has no kernel")
        return _kept(mean(x, axis), x, axis)
    if x.dtype == "bool":
        if axis is not None and not (x.ndim == 1 and axis in (0, -1)):
            raise TypeError("beekern mean: axis means of a bool array have no kernel")
        return scalar(count_nonzero(x) / x.size) if x.size else scalar(float("nan"))
    if axis is not None:
        return _reduce_axis("mean", x, int(axis))
    return sum(x) / x.size


def dot(a, b):
    a, b = _as_operand(a), _as_operand(b)
    _no_int64("dot", a, b)
    if a.ndim == 2 or b.ndim == 2:
        return matmul(a, b)  # (.T views stay views: the GEMMs read them in place)
    a, b = a._materialize(), b._materialize()
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("dot: 1-D operands must match in shape and dtype")
    return _reduce("dot", a, b)


def max_abs_diff(a, b) -> np.float64:
    """max(|a - b|) in one pass (no a - b array): e.g. a result against its
    reference.  Same shape and dtype."""
    a, b = _as_operand(a)._materialize(), _as_operand(b)._materialize()
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("max_abs_diff: operands must match in shape and dtype")
    return _reduce("max_abs_diff", a, b)


# ---- per-axis max / min / var / std (csrc/kernels/axis.hip) --------------------------

_STAT = {"max": 0, "min": 1, "var": 2, "std": 3}
MAX_AXIS0_COLUMNS = 1 << 18  # = BK_MAX_AXIS0_COLUMNS (csrc/kernels/beekern.h): the column form's workspace


def _stat_axis(what: str, x: DeviceArray, axis) -> Optional[int]:
    """The axis (0 or 1) of a 2-D array that ``what`` reduces along, or None
    for the whole array (no axis, or the one axis of a 1-D array)."""
    if axis is None:
        return None
    if not is_integer(axis):
        raise TypeError(f"beekern {what}: axis is an int or None, got {type(axis).__name__}")
    axis = int(axis)
    if x.ndim == 1:
        if axis not in (0, -1):
            raise ValueError(f"axis {axis} is out of bounds for a 1-D array")
        return None
    if x.ndim != 2:
        raise ValueError("axis reductions support 1-D and 2-D arrays")
    if axis not in (0, 1, -1, -2):
        raise ValueError(f"axis {axis} is out of bounds for a 2-D array")
    return axis % 2


def _axis_stat(what: str, x: DeviceArray, axis: int, ddof=0) -> DeviceArray:
    """max / min / var / std of a 2-D f32 / f64 array along ``axis`` in the
    array's dtype (bk_axis_stat: f64 arithmetic, the variance in two passes
    about an f64 mean).  A ``.T`` view reduces along the other axis of its
    buffer."""
    if x.dtype not in ("float32", "float64"):
        raise TypeError(f"beekern {what}: axis reductions take float32 / float64 arrays, got {x.dtype}")
    if x._lazy is not None:
        x._materialize()
    rows, cols = x.shape
    if x._transposed:  # the buffer is (cols, rows)
        rows, cols, axis = cols, rows, 1 - axis
    n = rows if axis == 0 else cols
    if n == 0 or x.size == 0:
        raise ValueError(f"beekern {what}: the reduced axis (or the array) is empty")
    divisor = 1.0
    if what in ("var", "std"):
        divisor = float(n - ddof)
        if not divisor > 0.0:
            raise ValueError(f"beekern {what}: ddof {ddof} leaves no degrees of freedom along an axis of {n}")
    if axis == 0 and cols > MAX_AXIS0_COLUMNS:
        raise ValueError(f"beekern {what}: at most {MAX_AXIS0_COLUMNS} columns along axis 0 of the buffer, got {cols}")
    out = DeviceArray((cols if axis == 0 else rows,), x.dtype)
    driver().axis_stat(_STAT[what], x.code, x._buf.ptr, out.ptr, rows, cols, cols, axis, divisor)  # type: ignore[union-attr]
    return out


def _extremum(what: str, x, axis, keepdims: bool):
    x = _as_operand(x)
    if x.dtype == "int64":
        return _int_reduce(what, x, axis, keepdims)
    ax = _stat_axis(what, x, axis)
    if ax is None:
        res = _reduce(what, x._materialize())
    else:
        res = _axis_stat(what, x, ax)
    return _kept(res, x, ax) if keepdims else res


def amax(x, axis: Optional[int] = None, keepdims: bool = False):
    return _extremum("max", x, axis, keepdims)


def amin(x, axis: Optional[int] = None, keepdims: bool = False):
    return _extremum("min", x, axis, keepdims)


def _spread(what: str, x, axis, ddof, keepdims: bool):
    x = _as_operand(x)
    if x.dtype not in ("float32", "float64"):
        raise TypeError(f"beekern {what}: float32 / float64 arrays only, got {x.dtype}")
    if isinstance(ddof, bool) or not isinstance(ddof, (int, float)):
        raise TypeError(f"beekern {what}: ddof is a number, got {type(ddof).__name__}")
    ax = _stat_axis(what, x, axis)
    if ax is None:
        n = x.size
        if not n - ddof > 0:
            raise ValueError(f"beekern {what}: ddof {ddof} leaves no degrees of freedom for {n} elements")
        m = float(mean(x))
        v = float(square_sum(_binary("subtract", x, m))) / (n - ddof)  # two passes, as numpy
        res = _result_type(x.dtype)(math.sqrt(v) if what == "std" else v)
    else:
        res = _axis_stat(what, x, ax, ddof)
    return _kept(res, x, ax) if keepdims else res


def var(x, axis: Optional[int] = None, ddof=0, keepdims: bool = False):
    """np.var: the whole array (a scalar of the array's dtype) or one axis of
    a 2-D array; two passes in f64, as numpy's."""
    return _spread("var", x, axis, ddof, keepdims)


def std(x, axis: Optional[int] = None, ddof=0, keepdims: bool = False):
    """np.std; see :func:`var`."""
    return _spread("std", x, axis, ddof, keepdims)


def _make_unary(name):
    def fn(x):
        return _unary(name, x)

    fn.__name__ = name
    return fn


abs = _make_unary("abs")  # noqa: A001
negative = _make_unary("negative")
sqrt = _make_unary("sqrt")
exp = _make_unary("exp")
log = _make_unary("log")
relu = _make_unary("relu")
sin = _make_unary("sin")
cos = _make_unary("cos")
tanh = _make_unary("tanh")
sigmoid = _make_unary("sigmoid")


def add(a, b): return _binary("add", a, b)
def subtract(a, b): return _binary("subtract", a, b)
def multiply(a, b): return _binary("multiply", a, b)
def divide(a, b): return _binary("divide", a, b)
def maximum(a, b): return _binary("maximum", a, b)
def minimum(a, b): return _binary("minimum", a, b)
def power(a, b): return _binary("power", a, b)


def floor_divide(a, b):
    """``a // b`` of int64 operands (Python's floor; 0 for a zero divisor, as numpy)."""
    return _int_binary("floor_divide", a, b, False)


def remainder(a, b):
    """``a % b`` of int64 operands (the divisor's sign; 0 for a zero divisor, as numpy)."""
    return _int_binary("remainder", a, b, False)


mod = remainder


# ---- int64 arrays (csrc/kernels/integer.hip) --------------------------------------------
#
# + - * // % maximum minimum, unary - and abs give int64 between int64 arrays of
# one shape and with integer scalars that fit int64 (OverflowError otherwise, as
# numpy 2).  A float scalar or a float32 / float64 array on the other side casts
# the int64 side (and a float32 array: numpy's result is float64) to float64
# and the float kernel runs; / always does.  Comparisons give ordinary bool
# masks.  No broadcasting, .T, axis reductions, ** or matmul.

def _is_int64(x) -> bool:
    return isinstance(x, DeviceArray) and x.dtype == "int64"


def _no_int64(what: str, *arrays) -> None:
    for a in arrays:
        if _is_int64(a):
            raise TypeError(f"beekern {what}: no kernel for int64 arrays")


def _bits_code(x: DeviceArray) -> int:
    """The dtype code the kernels that move elements by size (compress, where) take for x."""
    return DTYPE_CODES["float64"] if x.dtype == "int64" else x.code


def _int64_scalar(v) -> int:
    v = int(v)
    if not _I64_MIN <= v <= _I64_MAX:
        raise OverflowError(f"Python integer {v} out of bounds for int64")
    return v


def _is_int_scalar(v) -> bool:
    return is_integer(v) or (numpy_loaded() is not None and isinstance(v, np.bool_))


def _is_float_scalar(v) -> bool:
    return is_number(v) and not is_integer(v)


def _int_astype(x: DeviceArray, dt: str) -> DeviceArray:
    """int64 <-> float32 / float64 / bool (bk_int_cast; to bool: ``x != 0``)."""
    if "bfloat16" in (dt, x.dtype):
        raise TypeError(f"beekern astype: {x.dtype} -> {dt} has no kernel (int64 converts to and from float32 / "
                        "float64 / bool)")
    if dt == "bool":
        return _int_compare(_COMPARE["not_equal"], x, 0)
    out = DeviceArray(x.shape, dt)
    driver().int_cast(x.code, out.code, x.ptr, out.ptr, x.size)
    return out


def _as_float64(v):
    """An operand of a mixed int64 / float operation as float64: arrays cast, scalars float()."""
    if isinstance(v, DeviceArray):
        if v.dtype not in ("int64", "float32", "float64"):
            raise TypeError(f"beekern: no kernel for int64 with {v.dtype} arrays")
        return v if v.dtype == "float64" else v.astype("float64")
    return float(v)


def _int_operand(what: str, v):
    """An operand of an int64 operation: an int64 DeviceArray or an int that fits, or None if it is a float
    operand (a float scalar, a float32 / float64 array or host data of floats)."""
    if isinstance(v, DeviceArray):
        if v.dtype == "int64":
            return v
        if v.dtype in ("float32", "float64"):
            return None
        raise TypeError(f"beekern {what}: no kernel for int64 with {v.dtype} arrays")
    if _is_int_scalar(v):
        return _int64_scalar(v)
    if _is_float_scalar(v):
        return None
    host = np.asarray(v)
    if host.dtype.kind in "iub":
        return asarray(host, "int64")
    if host.dtype.kind == "f":
        return None
    raise TypeError(f"beekern {what}: cannot combine an int64 DeviceArray with {type(v).__name__}")


def _same_shape(what: str, a: DeviceArray, b: DeviceArray) -> None:
    if a.shape != b.shape:
        raise TypeError(f"beekern {what}: int64 arrays do not broadcast ({a.shape} vs {b.shape})")


def _int_binary(op: str, a, b, reversed_: bool) -> DeviceArray:
    lhs, rhs = (b, a) if reversed_ else (a, b)
    if not (_is_int64(lhs) or _is_int64(rhs)):
        raise TypeError(f"beekern {op}: int64 arrays only")
    if op == "power":
        raise TypeError("beekern power: no kernel for int64 arrays")
    il, ir = _int_operand(op, lhs), _int_operand(op, rhs)
    if op == "divide" or il is None or ir is None:
        if op not in _BINARY:
            raise TypeError(f"beekern {op}: no kernel for int64 with float operands")
        fl = _as_float64(lhs if isinstance(lhs, DeviceArray) or is_number(lhs) else asarray(lhs))
        fr = _as_float64(rhs if isinstance(rhs, DeviceArray) or is_number(rhs) else asarray(rhs))
        if isinstance(fl, DeviceArray):
            if isinstance(fr, DeviceArray):
                _same_shape(op, fl, fr)
            return _binary(op, fl, fr)
        return _binary(op, fr, fl, reversed_=True)
    code = _INT_BINARY[op]
    if isinstance(il, DeviceArray) and isinstance(ir, DeviceArray):
        if ir.size == 1 and il.shape != ir.shape:
            ir = int(ir.item())
        elif il.size == 1 and il.shape != ir.shape:
            il = int(il.item())
        else:
            _same_shape(op, il, ir)
            out = DeviceArray(il.shape, "int64")
            driver().int_binary(code, 0, il.ptr, ir.ptr, 0, out.ptr, il.size)
            return out
    arr, sc, mode = (il, ir, 1) if isinstance(il, DeviceArray) else (ir, il, 2)
    out = DeviceArray(arr.shape, "int64")
    driver().int_binary(code, mode, arr.ptr, 0, sc, out.ptr, arr.size)
    return out


def _int_unary(op: str, x: DeviceArray) -> DeviceArray:
    if op == "negative":
        return _int_binary("subtract", 0, x, False)
    if op == "abs":  # (INT64_MIN stays, as numpy's)
        return _int_binary("maximum", x, _int_binary("subtract", 0, x, False), False)
    if op == "copy":
        return x.copy()
    raise TypeError(f"beekern {op}: no kernel for int64 arrays")


def _const_mask(shape, value: bool) -> DeviceArray:
    return full(shape, value, "bool")


def _int_compare(code: int, a, b) -> DeviceArray:
    """A comparison with an int64 array on one side at least (a is a DeviceArray): a materialised bool mask."""
    if not _is_int64(a):  # a float array against an int64 one
        return _compare_code(code, _as_float64(a), _as_float64(b))
    if _is_int_scalar(b):
        v = int(b)
        if not _I64_MIN <= v <= _I64_MAX:  # numpy 2: the exact comparison
            true = {0: v > 0, 1: v > 0, 2: v < 0, 3: v < 0, 4: False, 5: True}[code]
            return _const_mask(a.shape, true)
        out = DeviceArray(a.shape, "bool")
        driver().int_compare(code, 1, a.ptr, 0, v, out.ptr, a.size)
        return out
    ib = _int_operand("compare", b)
    if ib is None:
        fb = _as_float64(b if isinstance(b, DeviceArray) or is_number(b) else asarray(b))
        return _compare_code(code, _as_float64(a), fb)
    _same_shape("compare", a, ib)
    out = DeviceArray(a.shape, "bool")
    driver().int_compare(code, 0, a.ptr, ib.ptr, 0, out.ptr, a.size)
    return out


def _compare_code(code: int, a, b) -> DeviceArray:
    name = next(k for k, v in _COMPARE.items() if v == code)
    return _compare(name, a, b)


def _int_reduce(what: str, x: DeviceArray, axis=None, keepdims: bool = False):
    """sum (wrapping, as numpy's) / max / min of a whole int64 array as ``np.int64``."""
    x._materialize()
    if keepdims or not (axis is None or (x.ndim == 1 and is_integer(axis) and int(axis) in (0, -1))):
        raise TypeError(f"beekern {what}: no axis or keepdims reductions of int64 arrays")
    if what != "sum" and x.size == 0:
        raise ValueError(f"zero-size array to reduction operation {what} which has no identity")
    v = driver().int_reduce(_INT_REDUCE[what], x.ptr, x.size)
    m = numpy_loaded()  # (np.int64 when numpy is loaded, else the same value as an int: ops/_lazy.py)
    return m.int64(v) if m is not None else v


# ---- boolean masks -------------------------------------------------------------------

def _is_numpy_scalar(s) -> bool:
    m = numpy_loaded()
    return m is not None and isinstance(s, (m.floating, m.integer, m.bool_))


def _round_to(s: float, dtype: str) -> float:
    """A Python scalar as the array's dtype would hold it (numpy 2: Python
    numbers are weak and take the array's dtype), as a double."""
    if dtype == "float64":
        return s
    try:
        bits = struct.unpack("<I", struct.pack("<f", s))[0]  # RNE
    except OverflowError:  # past float32's range: +-inf, as numpy's cast
        return math.copysign(math.inf, s)
    if dtype == "bfloat16":
        bits = _f32_bits_to_bf16(bits) << 16
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _compare_scalar(s, dtype: str) -> float:
    """The double the comparison kernel compares every (widened) element
    with.  A Python number is rounded to the array's dtype first; a numpy
    scalar goes unrounded -- where it would promote (np.float64 against an
    f32 array) the kernel's f64 comparison is numpy's promoted one, and where
    it would not, it is exact in the dtype already."""
    if _is_numpy_scalar(s):
        return float(s)
    return _round_to(float(s), dtype)


def _scalar_keeps_dtype(s, dtype: str) -> bool:
    """Whether numpy's result stays in ``dtype`` when ``s`` meets such an array."""
    if not _is_numpy_scalar(s):
        return True
    return dtype != "bfloat16" and np.result_type(np.dtype(dtype), s) == np.dtype(dtype)


def _compare(op: str, a, b) -> DeviceArray:
    code = _COMPARE[op]
    if not isinstance(a, DeviceArray):
        if not isinstance(b, DeviceArray):
            raise TypeError(f"beekern {op}: one operand must be a DeviceArray")
        a, b, code = b, a, _FLIPPED[code]  # scalar OP array: the flipped operator
    if a.dtype == "int64" or _is_int64(b):
        return _int_compare(code, a, b)
    if a.dtype not in _FLOATS:
        raise TypeError(f"beekern {op}: float arrays only, got {a.dtype}")
    if not (a._lazy is None and not a._transposed):
        a._materialize()
    if isinstance(b, DeviceArray):
        if b.shape != a.shape or b.dtype != a.dtype:
            if b.size == 1 and b.dtype in _FLOATS:
                return _compare(op, a, float(b.item()))
            raise ValueError(f"beekern {op}: shapes/dtypes must match ({a.shape} {a.dtype} vs {b.shape} {b.dtype})")
        b._materialize()
        other = b
    elif is_number(b) or _is_numpy_scalar(b):
        other = _compare_scalar(b, a.dtype)
    else:
        raise TypeError(f"beekern {op}: cannot compare a DeviceArray with {type(b).__name__}")
    mask = DeviceArray(a.shape, "bool", lazy=("cmp", code, a, other))
    for src in (a, other):
        if isinstance(src, DeviceArray):
            if src._buf._readers is None:
                src._buf._readers = weakref.WeakSet()
            src._buf._readers.add(mask)
    return mask


def _before_write(target: DeviceArray) -> None:
    """An in-place write into ``target`` is about to be enqueued: the lazy
    masks that still have to read its buffer run first (they are snapshots
    of the values at the time of the comparison)."""
    readers = target._buf._readers if target._buf is not None else None
    if readers:
        for m in list(readers):
            m._materialize()
        readers.clear()


def less(a, b): return _compare("less", a, b)
def less_equal(a, b): return _compare("less_equal", a, b)
def greater(a, b): return _compare("greater", a, b)
def greater_equal(a, b): return _compare("greater_equal", a, b)
def equal(a, b): return _compare("equal", a, b)
def not_equal(a, b): return _compare("not_equal", a, b)


def _is_lazy_mask(m: DeviceArray) -> bool:
    return m._lazy is not None and m._lazy[0] == "cmp"


def count_nonzero(x) -> int:
    """The number of true (non-zero) elements.  A lazy mask, or a float array
    (``x != 0``), is counted in one fused pass with no mask written."""
    x = _as_operand(x)
    if x.dtype == "int64":
        x = _int_compare(_COMPARE["not_equal"], x, 0)
    if x.dtype != "bool":
        x = _compare("not_equal", x, 0.0)
    if _is_lazy_mask(x):
        _, op, a, b = x._lazy
        if isinstance(b, DeviceArray):
            return int(driver().compare_count(op, a.code, 0, a.ptr, b.ptr, 0.0, x.size))
        return int(driver().compare_count(op, a.code, 1, a.ptr, 0, b, x.size))
    return int(driver().reduce(_REDUCE["sum"], x.code, x.ptr, 0, x.size))


def _mask_operand(what: str, m) -> DeviceArray:
    if not isinstance(m, DeviceArray) or m.dtype != "bool":
        raise TypeError(f"beekern {what}: bool DeviceArrays only, got "
                        f"{m.dtype if isinstance(m, DeviceArray) else type(m).__name__}")
    return m


def any(x) -> bool:  # noqa: A001 - numpy-compatible name
    x = _mask_operand("any", x)
    if _is_lazy_mask(x):
        return count_nonzero(x) > 0
    return driver().reduce(_REDUCE["max"], x.code, x.ptr, 0, x.size) != 0.0


def all(x) -> bool:  # noqa: A001 - numpy-compatible name
    x = _mask_operand("all", x)
    if _is_lazy_mask(x):
        return count_nonzero(x) == x.size
    return driver().reduce(_REDUCE["min"], x.code, x.ptr, 0, x.size) != 0.0


def _logical(op: str, a, b=None) -> DeviceArray:
    a = _mask_operand(op, a)
    if b is not None:
        b = _mask_operand(op, b)
        if b.shape != a.shape:
            raise ValueError(f"beekern {op}: shapes must match ({a.shape} vs {b.shape})")
    out = DeviceArray(a.shape, "bool")
    driver().mask_logical(_LOGICAL[op], a.ptr, b.ptr if b is not None else 0, out.ptr, a.size)
    return out


def logical_and(a, b): return _logical("logical_and", a, b)
def logical_or(a, b): return _logical("logical_or", a, b)
def logical_xor(a, b): return _logical("logical_xor", a, b)
def logical_not(a): return _logical("logical_not", a)


def where(mask, a, b, dtype=None) -> DeviceArray:
    """``mask ? a : b`` elementwise.  ``a`` and ``b``: device arrays of the
    mask's shape (one float dtype), or scalars; a Python number takes the
    arrays' dtype, two scalars give float64 (or ``dtype``).  Array values are
    moved as bits (NaN payloads and -0.0 survive)."""
    mask = _mask_operand("where", mask)
    if _is_int64(a) or _is_int64(b) or (dtype is not None and normalize_dtype(dtype) == "int64"):
        return _int_where(mask, a, b)
    arrays = [v for v in (a, b) if isinstance(v, DeviceArray)]
    for v in (a, b):
        if not isinstance(v, DeviceArray) and not (is_number(v) or _is_numpy_scalar(v)):
            raise TypeError(f"beekern where: operands are DeviceArrays or numbers, got {type(v).__name__}")
    if arrays:
        dt = arrays[0].dtype
        for v in arrays:
            if v.dtype != dt or v.dtype not in _FLOATS:
                raise TypeError(f"beekern where: arrays of one float dtype, got {[x.dtype for x in arrays]}")
            if v.shape != mask.shape:
                raise ValueError(f"beekern where: shapes must match the mask's ({v.shape} vs {mask.shape})")
        if dtype is not None and normalize_dtype(dtype) != dt:
            raise TypeError("beekern where: dtype= is for two scalars")
    else:
        dt = normalize_dtype(dtype) if dtype is not None else "float64"
        if dt not in _FLOATS:
            raise TypeError(f"beekern where: float results only, got {dt}")
    for v in (a, b):
        if not isinstance(v, DeviceArray) and arrays and not _scalar_keeps_dtype(v, dt):
            raise TypeError(f"beekern where: a {type(v).__name__} scalar would promote the {dt} result")
    flags = (0 if isinstance(a, DeviceArray) else 1) | (0 if isinstance(b, DeviceArray) else 2)
    out = DeviceArray(mask.shape, dt)
    driver().where(DTYPE_CODES[dt], mask.ptr, flags, a.ptr if not flags & 1 else 0, b.ptr if not flags & 2 else 0,
                   float(a) if flags & 1 else 0.0, float(b) if flags & 2 else 0.0, out.ptr, mask.size)
    return out


def _int_where(mask: DeviceArray, a, b) -> DeviceArray:
    """``where`` with an int64 side.  Two int64 operands (arrays of the mask's shape, integers that fit) give
    int64: scalars become arrays (``full``) and the values move as bits through the float64 form of the
    kernel.  A float operand casts the int64 side to float64, as numpy's result is."""
    sides = []
    for v in (a, b):
        if not isinstance(v, DeviceArray) and not (is_number(v) or _is_numpy_scalar(v)):
            raise TypeError(f"beekern where: operands are DeviceArrays or numbers, got {type(v).__name__}")
        sides.append(_int_operand("where", v))
    if sides[0] is None or sides[1] is None:
        return where(mask, _as_float64(a), _as_float64(b))
    arrays = []
    for v in sides:
        if not isinstance(v, DeviceArray):
            v = full(mask.shape, v, "int64")
        if v.shape != mask.shape:
            raise ValueError(f"beekern where: shapes must match the mask's ({v.shape} vs {mask.shape})")
        arrays.append(v)
    out = DeviceArray(mask.shape, "int64")
    driver().where(DTYPE_CODES["float64"], mask.ptr, 0, arrays[0].ptr, arrays[1].ptr, 0.0, 0.0, out.ptr, mask.size)
    return out


# ---- sorting, arg-reductions, gather (csrc/kernels/sort.hip) -------------------------
# numpy's order: floats numerically with -0.0 == +0.0 a tie and NaNs last, int64 signed, ties in index order (the
# sort is always stable).  np.sort / np.argsort / np.argmax / np.argmin / np.take of a device array are not routed
# here yet: they stay host fallbacks that warn (ops/npinterop.py).
MAX_SORT_N = 0x7FFFFFFF  # = BK_MAX_SORT_N (csrc/kernels/beekern.h), driver.MAX_SORT_N
_SORTABLE = ("float32", "float64", "bfloat16", "int64")


def _sort_operand(what: str, x, one_d: bool) -> DeviceArray:
    x = _as_operand(x)
    if x.dtype not in _SORTABLE:
        raise TypeError(f"beekern {what}: float32 / float64 / bfloat16 / int64 arrays only, got {x.dtype}")
    if one_d and x.ndim != 1:
        raise TypeError(f"beekern {what}: 1-D arrays only, got ndim {x.ndim} (no axis sorts yet)")
    if x._transposed:
        raise TypeError(f"beekern {what}: not on a .T view (copy it first: its C-order elements are not in the buffer's order)")
    x._materialize()
    return x


def _sort(what: str, x, want_sorted: bool, want_index: bool):
    from .driver import sort_workspace_bytes

    x = _sort_operand(what, x, True)
    n = x.size
    if n > MAX_SORT_N:
        raise TypeError(f"beekern {what}: at most {MAX_SORT_N} elements a call (BK_MAX_SORT_N), got {n}")
    out = DeviceArray((n,), x.dtype) if want_sorted else None
    index = DeviceArray((n,), "int64") if want_index else None
    if n:
        ws = _Buffer(sort_workspace_bytes(x.code, n, want_index))
        driver().sort(x.code, x.ptr, n, out.ptr if out is not None else 0, index.ptr if index is not None else 0, ws.ptr)
    return out, index


def sort(x, kind=None) -> DeviceArray:  # noqa: A001 - numpy-compatible name
    """np.sort(x) of a 1-D array, in x's dtype (``kind`` is accepted and ignored: the sort is stable)."""
    return _sort("sort", x, True, False)[0]


def argsort(x, kind=None) -> DeviceArray:
    """np.argsort(x, kind="stable") of a 1-D array as an int64 array."""
    return _sort("argsort", x, False, True)[1]


def _arg_reduce(what: str, x, axis):
    if axis is not None:
        raise TypeError(f"beekern {what}: axis= is not there yet (the flat index of the whole array only)")
    x = _sort_operand(what, x, False)
    if x.size == 0:
        raise ValueError(f"attempt to get {what} of an empty sequence")
    v = driver().arg_reduce(0 if what == "argmax" else 1, x.code, x.ptr, x.size)
    m = numpy_loaded()
    return m.int64(v) if m is not None else v


def argmax(x, axis=None):
    """np.argmax(x): the flat C-order index of the first maximum (the first NaN if there is one) as ``np.int64``."""
    return _arg_reduce("argmax", x, axis)


def argmin(x, axis=None):
    """np.argmin(x): the flat C-order index of the first minimum (the first NaN if there is one) as ``np.int64``."""
    return _arg_reduce("argmin", x, axis)


def _is_host_index(key) -> bool:
    """A non-empty list or ndarray of integers (not bools): what ``x[key]`` gathers by."""
    m = numpy_loaded()
    if isinstance(key, list):
        return len(key) > 0 and not [k for k in key if isinstance(k, bool) or not is_integer(k)]
    return m is not None and isinstance(key, m.ndarray) and key.dtype.kind in "iu"


def _index_operand(x: DeviceArray, idx) -> DeviceArray:
    """``idx`` as an int64 device array: one as it is; a host integer list / ndarray checked against x's length
    (numpy's IndexError, before anything is uploaded) and uploaded."""
    if isinstance(idx, DeviceArray):
        if idx.dtype != "int64":
            raise TypeError(f"beekern take: the index is an int64 array, got {idx.dtype}")
        if idx._transposed:
            raise TypeError("beekern take: not by a .T view")
        idx._materialize()
        return idx
    host = np.asarray(idx)
    if host.size == 0:
        host = host.astype(np.int64)  # (an empty list is float64 to numpy)
    if host.dtype.kind not in "iu":
        raise TypeError(f"beekern take: integer indices only, got {host.dtype}")
    if host.dtype.kind == "u" and host.size and int(host.max()) > _I64_MAX:
        raise IndexError(f"index {int(host.max())} is out of bounds for axis 0 with size {x.size}")
    host = host.astype(np.int64)
    bad = (host < -x.size) | (host >= x.size)
    if bad.any():
        raise IndexError(f"index {int(host[bad].flat[0])} is out of bounds for axis 0 with size {x.size}")
    return asarray(host, dtype="int64")


def take(x, idx) -> DeviceArray:
    """np.take(x, idx) of a 1-D array: ``x[idx]`` for an int64 index array (a DeviceArray, or a host integer list /
    ndarray), negative indices from the end, in idx's shape.  IndexError if an index is outside [-len(x), len(x))."""
    x = _as_operand(x)
    if x.ndim != 1:
        raise TypeError(f"beekern take: 1-D arrays only, got ndim {x.ndim}")
    if x.dtype not in _SUPPORTED:
        raise TypeError(f"beekern take: no kernel for {x.dtype} arrays")
    x._materialize()
    idx = _index_operand(x, idx)
    out = DeviceArray(idx.shape, x.dtype)
    bad = driver().take(_bits_code(x), x.ptr, x.size, idx.ptr, idx.size, out.ptr)
    if bad:
        raise IndexError(f"index out of bounds for axis 0 with size {x.size} ({bad} of the {idx.size} indices)")
    return out


# ---- order statistics and histograms (csrc/kernels/stats.hip) ------------------------

_SELECT_Q = 16  # quantiles per select call: two neighbouring ranks each, 32 ranks a call
MAX_HISTOGRAM_BINS = 4096  # = BK_MAX_BINS (csrc/kernels/beekern.h), driver.MAX_BINS


def _stats_operand(what: str, x) -> DeviceArray:
    """The array whose elements ``what`` looks at, in whatever order the
    buffer holds them: a lazy draw gets its buffer, a ``.T`` view is read in
    place (neither order statistics nor counts depend on element order)."""
    x = _as_operand(x)
    if x.dtype not in _FLOATS:
        raise TypeError(f"beekern {what}: float arrays only, got {x.dtype}")
    if x._lazy is not None:
        x._materialize()
    return x


def _result_type(dtype: str):
    return np.float64 if dtype == "float64" else np.float32  # (bf16 results are float32)


def _lerp(a: float, b: float, g: float) -> float:
    """a + (b - a) * g in f64, from whichever end is nearer as numpy's
    quantile does (``_lerp``: b - (b - a) * (1 - g) for g >= 0.5)."""
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


def _quantiles(x: DeviceArray, qs: Sequence[float]) -> list:
    """numpy's "linear" quantiles of the whole array, as f64 Python floats
    (NaN for every one if x holds a NaN)."""
    n = x.size
    out: list = []
    for i in range(0, len(qs), _SELECT_Q):
        part = qs[i:i + _SELECT_Q]
        ranks, gammas = [], []
        for q in part:
            virtual = (n - 1) * q
            lo = min(max(int(math.floor(virtual)), 0), n - 1)
            ranks += [lo, min(lo + 1, n - 1)]
            gammas.append(virtual - lo)
        values, nans = driver().select(x.code, x._buf.ptr, n, ranks)  # type: ignore[union-attr]
        if nans:
            return [math.nan] * len(qs)
        out += [_lerp(values[2 * j], values[2 * j + 1], g) for j, g in enumerate(gammas)]
    return out


def _quantile(what: str, x, q, scale: float):
    x = _stats_operand(what, x)
    if x.size == 0:
        raise ValueError(f"beekern {what}: the array is empty")
    qa = np.asarray(q, dtype=np.float64)
    if qa.ndim > 1:
        raise ValueError(f"beekern {what}: q is a scalar or a 1-D sequence")
    qs = [float(v) / scale for v in qa.reshape(-1)]
    for v in qs:
        if not 0.0 <= v <= 1.0:  # (a NaN too)
            raise ValueError("Percentiles must be in the range [0, 100]" if scale == 100.0
                             else "Quantiles must be in the range [0, 1]")
    res = _quantiles(x, qs)
    if qa.ndim == 0:
        return _result_type(x.dtype)(res[0])
    return np.array(res, np.float64)


def percentile(x, q):
    """np.percentile(x, q) of the whole array (method "linear"): a scalar of
    the array's dtype for a scalar ``q`` (float32 for bf16), a host float64
    ndarray for a 1-D sequence.  No sort: a radix select of the neighbouring
    ranks, interpolated in f64 and rounded once."""
    return _quantile("percentile", x, q, 100.0)


def quantile(x, q):
    """np.quantile(x, q) of the whole array; see :func:`percentile`."""
    return _quantile("quantile", x, q, 1.0)


def median(x):
    """np.median(x) of the whole array: the middle element, or the mean of the
    middle two in the array's dtype as numpy takes it; NaN if x holds one."""
    x = _stats_operand("median", x)
    n = x.size
    if n == 0:
        raise ValueError("beekern median: the array is empty")
    rt = _result_type(x.dtype)
    values, nans = driver().select(x.code, x._buf.ptr, n, [(n - 1) // 2, n // 2])  # type: ignore[union-attr]
    if nans:
        return rt(math.nan)
    return np.mean(np.array(values if n % 2 == 0 else values[:1], rt))


def histogram(x, bins=10, range=None, density=False):  # noqa: A002 - numpy's parameter name
    """np.histogram(x, bins, range, density=density) of the whole array:
    (counts, edges) as host ndarrays.  ``bins``: an int or a 1-D sequence of
    edges, at most 4096 bins.  The edges are numpy's own
    (``np.histogram_bin_edges`` on the array's [min, max] or ``range``, in the
    array's dtype); the counts follow numpy's bin rule exactly."""
    x = _stats_operand("histogram", x)
    rt = _result_type(x.dtype)
    if is_integer(bins):
        if int(bins) > MAX_HISTOGRAM_BINS:
            raise ValueError(f"beekern histogram: at most {MAX_HISTOGRAM_BINS} bins, got {int(bins)}")
        if range is not None:
            ends = np.array([range[0], range[1]], rt)  # (numpy looks at the data's dtype only)
        elif x.size:
            lo, hi = (driver().reduce(_REDUCE[op], x.code, x._buf.ptr, 0, x.size) for op in ("min", "max"))  # type: ignore[union-attr]
            ends = np.array([lo, hi], rt)
        else:
            ends = np.array([], rt)
        edges = np.histogram_bin_edges(ends, int(bins), range=range)  # (numpy's errors for a bad bins / range)
    else:
        if isinstance(bins, str):
            raise TypeError("beekern histogram: bins is an int or a sequence of edges (no estimator names)")
        edges = np.histogram_bin_edges(np.array([], rt), bins, range=range)
        if edges.size - 1 > MAX_HISTOGRAM_BINS:
            raise ValueError(f"beekern histogram: at most {MAX_HISTOGRAM_BINS} bins, got {edges.size - 1}")
        if not np.isfinite(edges).all():
            raise ValueError("beekern histogram: the edges must be finite")
    if edges.size < 2 or x.size == 0:
        counts = np.zeros(max(edges.size - 1, 0), np.int64)
    else:
        counts = driver().histogram(x.code, x._buf.ptr, x.size, edges.astype(np.float64))  # type: ignore[union-attr]
    if density:
        db = np.array(np.diff(edges), float)
        return counts / db / counts.sum(), edges
    return counts, edges


# ---- matmul --------------------------------------------------------------------------

# The [K][N] kernel (bk_gemm_bf16_nn) reads B in place; the alternative is a
# transpose pass (4*K*N bytes of HBM traffic) then the TN kernel, which runs
# 7-10% faster than the [K][N] one.  The pass costs ~600/M of the GEMM, so
# reading in place wins below M ~ 6k.  Measured on MI355X, TFLOP/s, [K][N]
# kernel vs transpose + TN (hipBLASLt's NN in brackets,
# profiles/archive/r2_s3_gemm_nn_sweep.log):
#   M=N=4096,  K=512..4096: 715/949/1132/1229/1298 vs 574/771/1029/1154/1218
#                           (659/935/1140/1256/1302)
#   2048x8192x2048: 1211 vs 1014 (1195)
#   M=N=8192,  K=1024..8192: 1081/1242/1286/1298 vs 1091/1252/1328/1325
#   16384x4096x1024: 1104 vs 1108
# BEE_GEMM_NN: auto (M below _NN_MAX_M), 1 (whenever the shape allows), 0 (never)
_GEMM_NN = os.environ.get("BEE_GEMM_NN", "auto")
_NN_MAX_M = 6144


def _use_nn(M: int) -> bool:
    return _GEMM_NN == "1" or (_GEMM_NN == "auto" and M < _NN_MAX_M)


def _fp_dtype(x) -> bool:
    return x.dtype in ("float32", "float64")


# f32 products take the six-piece bf16 split (csrc/kernels/gemm_fp.hip
# bk_gemm_f32x6: f32-level error at the bf16 MFMA's rate) above 2^33
# multiply-adds with M, N >= 256; smaller ones, and any product whose
# workspace the HBM quota refuses, run on the f32 MFMA.  Measured medians,
# split vs f32 kernel (profiles/r6_gemm_fp_sweep.jsonl, f32 kernel with the
# buffer loads): 1024^3 81 vs 26 us, 1536^3 113 vs 80, 2048^3 (= 2^33) 153
# vs 138, 4000x3000x1000 153 vs 191, 3072^3 426 vs 424 (level), 4096^3 696
# vs 1005.  BEE_GEMM_F32X6: auto | 1 (whenever the shape allows) | 0 (never).
_F32X6 = os.environ.get("BEE_GEMM_F32X6", "auto")
_F32X6_MIN_MACS = (1 << 33) + 1


def f32x6_workspace_bytes(M: int, N: int, K: int) -> int:
    """Workspace of the split product: a 256-byte header, then A' [M][6 Kp]
    and B' [N][6 Kp] in bf16, Kp = K rounded up to 64 (broker_core.hpp)."""
    return 256 + 12 * ((K + 63) // 64 * 64) * (M + N)


def _use_f32x6(M: int, N: int, K: int) -> bool:
    if _F32X6 == "0" or 6 * ((K + 63) // 64 * 64) > (1 << 22):
        return False
    return _F32X6 == "1" or (min(M, N) >= 256 and M * N * K >= _F32X6_MIN_MACS)


def matmul_fp(a, b) -> DeviceArray:
    """C = A @ B in numpy's precision: f64 operands on the f64 MFMA
    (``v_mfma_f64_16x16x4_f64``), f32 on the exact f32 MFMA
    (``v_mfma_f32_16x16x4_f32``) or, for large products, on the bf16 MFMA
    through the six-piece split (f32-level error, :func:`f32x6_workspace_bytes`),
    mixed f32/f64 promoted to f64 as numpy does (``csrc/kernels/gemm_fp.hip``).  numpy's 1-D rules: a 1-D ``a`` is
    a row vector, a 1-D ``b`` a column, and that axis is dropped from the
    result.  ``.T`` views are read in place (no transpose pass)."""
    a = _as_operand(a)
    b = _as_operand(b)
    if not (_fp_dtype(a) and _fp_dtype(b)) or a.ndim not in (1, 2) or b.ndim not in (1, 2):
        raise ValueError(f"matmul_fp: f32/f64 operands of 1 or 2 dimensions, got {a.shape} {a.dtype} @ {b.shape} {b.dtype}")
    dt = "float64" if "float64" in (a.dtype, b.dtype) else "float32"
    a1, b1 = a.ndim == 1, b.ndim == 1
    if a1:
        a = a.reshape(1, a.shape[0])
    if b1:
        b = b.reshape(b.shape[0], 1)
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"matmul: incompatible shapes {a.shape} @ {b.shape}")
    if a.dtype != dt:
        a = a.astype(dt)
    if b.dtype != dt:
        b = b.astype(dt)
    M, K = a.shape
    N = b.shape[1]
    out_shape = tuple(s for s, drop in ((M, a1), (N, b1)) if not drop)
    if M == 0 or N == 0 or K == 0:
        return zeros(out_shape, dt)  # (numpy: an empty product, or zeros for K == 0)
    # a .T view is never lazy (T materialises first): its buffer is the
    # row-major transpose, read as is with the transposed-operand flag
    ta, tb = a._transposed, b._transposed
    a_ptr = a._buf.ptr if ta else a.ptr  # type: ignore[union-attr]
    b_ptr = b._buf.ptr if tb else b.ptr  # type: ignore[union-attr]
    c = DeviceArray((M, N), dt)
    lda, ldb = (M if ta else K), (K if tb else N)
    ws = None
    if dt == "float32" and _use_f32x6(M, N, K):
        nbytes = f32x6_workspace_bytes(M, N, K)
        try:
            ws = DeviceArray((nbytes // 2,), "bfloat16")
        except QuotaExceeded:
            ws = None  # (no room for the split operands: the f32 MFMA needs none)
    if ws is not None:
        driver().gemm_f32x6(ta, tb, a_ptr, b_ptr, c.ptr, M, N, K, lda, ldb, N, ws.ptr, nbytes)
        del ws  # (freed in stream order)
    else:
        driver().gemm_fp(DTYPE_CODES[dt], ta, tb, a_ptr, b_ptr, c.ptr, M, N, K, lda, ldb, N)
    return c.reshape(out_shape) if out_shape != (M, N) else c


def matmul(a, b, out_dtype: Optional[str] = None) -> DeviceArray:
    """C = A @ B.

    f32 / f64 operands (and no ``out_dtype``): numpy's precision on the
    full-precision MFMA GEMM (:func:`matmul_fp`).  A bf16 operand or an
    explicit ``out_dtype``: the bf16 MFMA GEMM (f32 accumulate; f32 / f64
    operands are rounded to bf16), bf16 result by default.

    On the bf16 path ``b.T`` views of a row-major [N, K] buffer are used as
    is (the TN kernels); a plain row-major bf16 ``b`` is read in place by the
    [K][N] kernel for tile-multiple shapes with M below ~6k (BEE_GEMM_NN),
    else transposed once on device (15 us at 4096^2) for the TN kernel; an
    f32/f64 ``b`` is converted and transposed in the same pass.
    """
    a = _as_operand(a)
    b = _as_operand(b)
    _no_int64("matmul", a, b)
    if out_dtype is None:
        if _fp_dtype(a) and _fp_dtype(b):
            return matmul_fp(a, b)
        out_dtype = "bfloat16"
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[0]:
        raise ValueError(f"matmul: incompatible shapes {a.shape} @ {b.shape}")
    M, K = a.shape
    N = b.shape[1]
    if a.dtype != "bfloat16":
        a = a.astype("bfloat16")
    a._materialize()
    if b._transposed and b.dtype == "bfloat16" and b._lazy is None:
        bt_ptr = b._buf.ptr  # the underlying buffer already is Bt[N, K]
        keep = b
    elif b._transposed and b.dtype in ("float32", "float64") and b._lazy is None:
        # the underlying buffer is Bt[N, K] already: only the conversion
        keep = DeviceArray((N, K), "bfloat16")
        driver().cast(b.code, DTYPE_CODES["bfloat16"], b._buf.ptr, keep.ptr, N * K)
        bt_ptr = keep.ptr
    elif b.dtype in ("float32", "float64") and not b._transposed and K % 8 == 0 and N % 8 == 0 and \
            (driver().name == "broker" or b.ptr % 16 == 0):
        # one pass: f32/f64 B[K, N] -> bf16 Bt[N, K] (broker handles are allocation bases: 16-B aligned)
        keep = DeviceArray((N, K), "bfloat16")
        driver().transpose(b.ptr, keep.ptr, K, N, N, K, DTYPE_CODES[b.dtype])
        bt_ptr = keep.ptr
    else:
        if b.dtype != "bfloat16":
            b = b.astype("bfloat16")
        b._materialize()
        out_dtype = normalize_dtype(out_dtype)
        from .driver import nn_shape_ok

        d = driver()
        if _use_nn(M) and hasattr(d, "gemm_nn") and nn_shape_ok(M, N, K, K, N, N, out_dtype == "bfloat16") and \
                (d.name == "broker" or (a.ptr % 16 == 0 and b.ptr % 16 == 0)):
            # B[K, N] read in place through transposed LDS reads: no transpose pass
            c = DeviceArray((M, N), out_dtype)
            d.gemm_nn(a.ptr, b.ptr, c.ptr, M, N, K, K, N, N, 1.0, 0.0, DTYPE_CODES[out_dtype])
            return c
        keep = DeviceArray((N, K), "bfloat16")
        driver().transpose(b.ptr, keep.ptr, K, N, N, K)
        bt_ptr = keep.ptr
    out_dtype = normalize_dtype(out_dtype)
    c = DeviceArray((M, N), out_dtype)
    driver().gemm(a.ptr, bt_ptr, c.ptr, M, N, K, K, K, N, 1.0, 0.0, DTYPE_CODES[out_dtype])
    del keep
    return c


def gemm_bf16_tn(a: DeviceArray, bt: DeviceArray, out_dtype: str = "bfloat16", alpha: float = 1.0) -> DeviceArray:
    """Raw C = alpha * A . Bt^T with both operands already bf16 [M,K] / [N,K]."""
    M, K = a.shape
    N = bt.shape[0]
    out_dtype = normalize_dtype(out_dtype)
    c = DeviceArray((M, N), out_dtype)
    driver().gemm(a.ptr, bt.ptr, c.ptr, M, N, K, K, K, N, float(alpha), 0.0, DTYPE_CODES[out_dtype])
    return c


# ---- random ----------------------------------------------------------------------------

_LAZY_RANDOM = os.environ.get("BEE_LAZY_RANDOM", "1") != "0"


def set_lazy_random(enabled: bool) -> bool:
    """Uniform draws are lazy by default: generated on first use, and fused
    into a reduction that consumes them directly.  ``False`` materialises
    every draw in HBM at once (numpy's data movement: the reference
    payload's 800 MB array).  Returns the previous setting."""
    global _LAZY_RANDOM
    prev, _LAZY_RANDOM = _LAZY_RANDOM, bool(enabled)
    return prev


class Generator:
    """Counter-based Philox4x32-10 stream on the device (numpy.random subset)."""

    def __init__(self, seed: Optional[int] = None) -> None:
        self.seed(seed)

    def seed(self, seed: Optional[int] = None) -> None:
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._offset = 0

    def _advance(self, n: int, per_call: int) -> int:
        off = self._offset
        self._offset += (n + per_call - 1) // per_call
        return off

    def random(self, size=None, dtype="float64") -> DeviceArray:
        return self.uniform(0.0, 1.0, size, dtype)

    def rand(self, *shape, dtype="float64") -> DeviceArray:
        return self.uniform(0.0, 1.0, shape or (1,), dtype)

    def _draw(self, kind: int, a: float, b: float, size, dtype) -> DeviceArray:
        shape = _shape_of(size)
        dt = normalize_dtype(dtype)
        if dt == "bfloat16" and kind != 0:
            return self._draw(kind, a, b, shape, "float32").astype("bfloat16")
        per = 2 if dt == "float64" else 4  # bf16 uniforms are the f32 stream, rounded
        n = int(math.prod(shape)) if shape else 1
        off = self._advance(n, per)
        if kind == 0 and _LAZY_RANDOM:
            # generated on first use; a reduction consuming it directly fuses
            # the generator into the reduction (sum, square_sum)
            return DeviceArray(shape, dt, lazy=("rand", 0, self._seed, off, float(a), float(b)))
        out = DeviceArray(shape, dt)
        driver().rand(kind, out.ptr, out.size, out.code, self._seed, off, float(a), float(b))
        return out

    def uniform(self, low=0.0, high=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._draw(0, low, high, size, dtype)

    def randn(self, *shape, dtype="float64") -> DeviceArray:
        return self.normal(0.0, 1.0, shape or (1,), dtype)

    def standard_normal(self, size=None, dtype="float64") -> DeviceArray:
        return self.normal(0.0, 1.0, size, dtype)

    def normal(self, loc=0.0, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._draw(1, loc, scale, size, dtype)

    # ---- the distributions of bk_rand_dist (csrc/kernels/random.hip): numpy's names and defaults --------
    def _dist(self, kind: int, p0: float, p1: float, size, dtype, per: int = 0) -> DeviceArray:
        """A materialised draw of distribution ``kind``.  per: elements a counter yields -- 0 for the
        packing of the uniform draws (2 f64 / 4 f32), 1 for the rejection family (a substream each)."""
        shape = _shape_of(size)
        dt = normalize_dtype(dtype)
        if dt == "bfloat16":  # the f32 draw, rounded
            return self._dist(kind, p0, p1, shape, "float32", per).astype("bfloat16")
        if dt not in ("float32", "float64"):
            raise TypeError(f"random draws are float32, float64 or bfloat16, not {dt}")
        n = int(math.prod(shape)) if shape else 1
        off = self._advance(n, per or (2 if dt == "float64" else 4))
        out = DeviceArray(shape, dt)
        driver().rand_dist(kind, out.ptr, out.size, out.code, self._seed, off, float(p0), float(p1))
        return out

    def exponential(self, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_EXPONENTIAL, _param("scale", scale, 0), 0.0, size, dtype)

    def standard_exponential(self, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_EXPONENTIAL, 1.0, 0.0, size, dtype)

    def laplace(self, loc=0.0, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_LAPLACE, _param("loc", loc), _param("scale", scale, 0), size, dtype)

    def logistic(self, loc=0.0, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_LOGISTIC, _param("loc", loc), _param("scale", scale, 0), size, dtype)

    def gumbel(self, loc=0.0, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_GUMBEL, _param("loc", loc), _param("scale", scale, 0), size, dtype)

    def rayleigh(self, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_RAYLEIGH, _param("scale", scale, 0), 0.0, size, dtype)

    def weibull(self, a, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_WEIBULL, _param("a", a, 1), 0.0, size, dtype)

    def pareto(self, a, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_PARETO, _param("a", a, 1), 0.0, size, dtype)

    def standard_cauchy(self, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_CAUCHY, 0.0, 1.0, size, dtype)

    def lognormal(self, mean=0.0, sigma=1.0, size=None, dtype="float64") -> DeviceArray:
        """exp of the ``normal(mean, sigma)`` draw at the same seed and counter."""
        return self._dist(DIST_LOGNORMAL, _param("mean", mean), _param("sigma", sigma, 0), size, dtype)

    def gamma(self, shape, scale=1.0, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_GAMMA, _param("shape", shape, 1), _param("scale", scale, 0), size, dtype, per=1)

    def standard_gamma(self, shape, size=None, dtype="float64") -> DeviceArray:
        return self.gamma(shape, 1.0, size, dtype)

    def chisquare(self, df, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_GAMMA, 0.5 * _param("df", df, 1), 2.0, size, dtype, per=1)

    def beta(self, a, b, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_BETA, _param("a", a, 1), _param("b", b, 1), size, dtype, per=1)

    def standard_t(self, df, size=None, dtype="float64") -> DeviceArray:
        return self._dist(DIST_STUDENT_T, _param("df", df, 1), 0.0, size, dtype, per=1)

    # ---- the integer-valued draws of bk_rand_int (csrc/kernels/integer.hip): int64, numpy's names and defaults ----
    def _rint(self, kind: int, a: int, b: int, p: float, size, per: int) -> DeviceArray:
        """A draw of ``kind``.  per: elements a counter yields (1: a substream each)."""
        shape = _shape_of(size)
        n = int(math.prod(shape)) if shape else 1
        off = self._advance(n, per)
        out = DeviceArray(shape, "int64")
        driver().rand_int(kind, out.ptr, out.size, self._seed, off, a, b, float(p))
        return out

    def integers(self, low, high=None, size=None, endpoint: bool = False) -> DeviceArray:
        """Uniform integers of [low, high) ([0, low) without ``high``; ``endpoint``: [low, high])."""
        if high is None:
            low, high = 0, low
        low, high = _int_param("low", low), _int_param("high", high)
        if endpoint:
            high += 1
        if not low < high <= _I64_MAX:
            raise ValueError("low >= high" if low >= high else "high is out of bounds for int64")
        return self._rint(RINT_INTEGERS, low, high, 0.0, size, 4 if high - low <= (1 << 32) else 2)

    def randint(self, low, high=None, size=None) -> DeviceArray:
        return self.integers(low, high, size)

    def poisson(self, lam=1.0, size=None) -> DeviceArray:
        lam = _param("lam", lam, 0)
        if lam > 9007199254740992.0:
            raise ValueError("lam value too large")
        return self._rint(RINT_POISSON, 0, 0, lam, size, 1)

    def binomial(self, n, p, size=None) -> DeviceArray:
        n, p = _int_param("n", n), _param("p", p)
        if n < 0:
            raise ValueError("n < 0")
        if n >= 1 << 53:
            raise ValueError("n too large")
        if not 0.0 <= p <= 1.0:
            raise ValueError("p < 0, p > 1 or p is NaN")
        return self._rint(RINT_BINOMIAL, n, 0, p, size, 1)

    def geometric(self, p, size=None) -> DeviceArray:
        p = _param("p", p)
        if not 0.0 < p <= 1.0:
            raise ValueError("p <= 0, p > 1 or p contains NaNs")
        return self._rint(RINT_GEOMETRIC, 0, 0, p, size, 2)


def _int_param(name: str, v) -> int:
    """An integer parameter of a draw that fits int64 (ValueError otherwise)."""
    if not is_integer(v):
        f = float(v)
        if not math.isfinite(f) or f != math.floor(f):
            raise ValueError(f"{name} must be an integer")
        v = int(f)
    v = int(v)
    if not _I64_MIN <= v <= _I64_MAX:
        raise ValueError(f"{name} is out of bounds for int64")
    return v


def _param(name: str, v, rule: int = -1) -> float:
    """A distribution's parameter as a finite float; rule 0: >= 0, 1: > 0 (ValueError in numpy's words)."""
    f = float(v)
    if not math.isfinite(f):
        raise ValueError(f"{name} must be finite")
    if rule == 0 and f < 0.0:
        raise ValueError(f"{name} < 0")
    if rule == 1 and f <= 0.0:
        raise ValueError(f"{name} <= 0")
    return f


def _shape_of(size) -> Shape:
    if size is None:
        return (1,)
    if is_integer(size):
        return (int(size),)
    if len(size) == 1 and isinstance(size[0], (tuple, list)):
        return tuple(int(s) for s in size[0])
    return tuple(int(s) for s in size)


class _RandomModule:
    """``bk.random`` — module-level functions on a default generator."""

    def __init__(self) -> None:
        self._gen: Optional[Generator] = None

    @property
    def gen(self) -> Generator:
        if self._gen is None:
            self._gen = Generator()
        return self._gen

    def seed(self, seed=None): self.gen.seed(seed)
    def default_rng(self, seed=None) -> Generator: return Generator(seed)
    def rand(self, *shape, dtype="float64"): return self.gen.rand(*shape, dtype=dtype)
    def randn(self, *shape, dtype="float64"): return self.gen.randn(*shape, dtype=dtype)
    def random(self, size=None, dtype="float64"): return self.gen.random(size, dtype)
    def uniform(self, low=0.0, high=1.0, size=None, dtype="float64"): return self.gen.uniform(low, high, size, dtype)
    def normal(self, loc=0.0, scale=1.0, size=None, dtype="float64"): return self.gen.normal(loc, scale, size, dtype)
    def standard_normal(self, size=None, dtype="float64"): return self.gen.standard_normal(size, dtype)
    def exponential(self, scale=1.0, size=None, dtype="float64"): return self.gen.exponential(scale, size, dtype)
    def standard_exponential(self, size=None, dtype="float64"): return self.gen.standard_exponential(size, dtype)
    def laplace(self, loc=0.0, scale=1.0, size=None, dtype="float64"): return self.gen.laplace(loc, scale, size, dtype)
    def gumbel(self, loc=0.0, scale=1.0, size=None, dtype="float64"): return self.gen.gumbel(loc, scale, size, dtype)
    def rayleigh(self, scale=1.0, size=None, dtype="float64"): return self.gen.rayleigh(scale, size, dtype)
    def weibull(self, a, size=None, dtype="float64"): return self.gen.weibull(a, size, dtype)
    def pareto(self, a, size=None, dtype="float64"): return self.gen.pareto(a, size, dtype)
    def standard_cauchy(self, size=None, dtype="float64"): return self.gen.standard_cauchy(size, dtype)
    def lognormal(self, mean=0.0, sigma=1.0, size=None, dtype="float64"):
        return self.gen.lognormal(mean, sigma, size, dtype)

    def logistic(self, loc=0.0, scale=1.0, size=None, dtype="float64"):
        return self.gen.logistic(loc, scale, size, dtype)

    def gamma(self, shape, scale=1.0, size=None, dtype="float64"): return self.gen.gamma(shape, scale, size, dtype)
    def standard_gamma(self, shape, size=None, dtype="float64"): return self.gen.standard_gamma(shape, size, dtype)
    def chisquare(self, df, size=None, dtype="float64"): return self.gen.chisquare(df, size, dtype)
    def beta(self, a, b, size=None, dtype="float64"): return self.gen.beta(a, b, size, dtype)
    def standard_t(self, df, size=None, dtype="float64"): return self.gen.standard_t(df, size, dtype)

    def integers(self, low, high=None, size=None, endpoint=False):
        return self.gen.integers(low, high, size, endpoint)

    def randint(self, low, high=None, size=None): return self.gen.randint(low, high, size)
    def poisson(self, lam=1.0, size=None): return self.gen.poisson(lam, size)
    def binomial(self, n, p, size=None): return self.gen.binomial(n, p, size)
    def geometric(self, p, size=None): return self.gen.geometric(p, size)


random = _RandomModule()


class Timer:
    """Device timing: HIP events (native) or synced wall clock (broker)."""

    def __enter__(self):
        self._tok = driver().timer_start()
        return self

    def __exit__(self, *exc):
        self.ms = driver().timer_stop(self._tok)
        return False

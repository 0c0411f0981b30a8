"""numpy's dispatch protocols for beekern arrays (NEP 13 ``__array_ufunc__``,
NEP 18 ``__array_function__``).

A numpy call on a device array runs on the gfx950 kernels when one computes
what numpy would (same dtype rules, same shape):

* ufuncs: square, negative, absolute, sqrt, exp, log, sin, cos, tanh, add,
  subtract, multiply, divide, maximum, minimum, power -- elementwise kernels
  (``ops/array.py`` ``_unary`` / ``_binary``); ``np.square`` stays lazy, so
  ``np.sum(np.square(x))`` is the fused one-pass square-sum; the binary ones
  also broadcast a 2-D ``(R, C)`` operand against a ``(C,)``, ``(1, C)`` or
  ``(R, 1)`` one of the same dtype, on either side (``X - X.mean(axis=0)``:
  one pass of ``csrc/kernels/axis.hip``, ``.T`` views read in place);
* comparisons ``less`` / ``less_equal`` / ``greater`` / ``greater_equal`` /
  ``equal`` / ``not_equal`` of two device arrays or an array and a scalar
  (either side): a device ``bool`` mask, lazy until something other than a
  count needs it, so ``np.sum(x * x + y * y <= 1.0)`` is one fused
  compare-count pass (``csrc/kernels/mask.hip``); a Python number is rounded
  to the array's dtype first and a numpy scalar that would promote compares
  in f64, as numpy 2 does;
* on ``bool`` masks: ``logical_and`` / ``logical_or`` / ``logical_xor`` /
  ``logical_not`` and ``bitwise_and`` / ``bitwise_or`` / ``bitwise_xor`` /
  ``invert`` (``&``, ``|``, ``^``, ``~``);
* ufunc reductions ``np.add.reduce`` / ``np.maximum.reduce`` /
  ``np.minimum.reduce`` (whole array, or ``axis=0|1`` of a 2-D array);
* functions: ``sum`` / ``mean``, ``max`` / ``min`` / ``amax`` / ``amin``,
  ``var`` / ``std`` (``ddof`` too; two passes in f64, as numpy) of the whole
  array or along one axis (``0``, ``1``, ``-1``, ``-2``) of a 2-D array, with
  ``keepdims`` -- the axis forms of max / min / var / std take f32 / f64 and
  run on ``csrc/kernels/axis.hip``; results are typed as numpy types them (an
  array in the input dtype, a numpy scalar for a whole or 1-D array);
  ``out=``, ``dtype=``, ``where=``, ``initial=``, tuple axes, ``mean=`` /
  ``correction=`` and arrays of more than two dimensions go to the host;
* ``dot`` of 1-D vectors, ``linalg.norm`` (fused square-sum), ``copy`` /
  ``reshape`` / ``ravel``, and the metadata functions ``shape`` / ``ndim`` /
  ``size``;
* masks: ``sum`` (``np.int64``) / ``mean`` / ``count_nonzero`` (also of a
  float array: the fused ``!= 0`` count) / ``any`` / ``all`` of a whole
  array, and the three-argument ``where(mask, x, y)``;
* order statistics and histograms of a whole f32 / f64 array (or axis 0 of a
  1-D one): ``median``, ``percentile`` / ``quantile`` (method "linear", ``q``
  a host scalar, list or ndarray) and ``histogram`` (int ``bins`` or host
  edges, at most 4096 bins, ``range``, ``density``) -- a radix select of the
  ranks a quantile needs and a histogram counted against numpy's own edges
  (``csrc/kernels/stats.hip``), typed as numpy types them; ``out``,
  ``overwrite_input=True``, ``keepdims=True``, ``weights``, other methods, an
  axis of a 2-D array, string ``bins``, ``q`` out of range, bf16 / bool and
  empty arrays go to numpy on the host;
* ``matmul`` / ``dot`` / ``@`` of 1-D and 2-D operands: f32 / f64 on the
  full-precision MFMA GEMM in numpy's result dtype (``ops/array.py``
  ``matmul_fp``, ``csrc/kernels/gemm_fp.hip``; ``.T`` views read in place),
  bf16 on the bf16 MFMA GEMM.  A host ndarray operand of a product with a
  device array is uploaded once and the result stays on the device
  (``BEE_NUMPY_OFFLOAD_MATMUL=bf16`` rounds f32 / f64 products to the bf16
  GEMM instead, as before).

* on ``int64`` arrays (``csrc/kernels/integer.hip``): ``add`` / ``subtract`` /
  ``multiply`` / ``floor_divide`` / ``remainder`` (``mod``) / ``true_divide`` /
  ``maximum`` / ``minimum`` / ``negative`` / ``absolute`` and the six
  comparisons, with an int64 array of the same shape, an integer scalar that
  fits (int64 results) or a float scalar / f32 / f64 array (float64 results,
  as numpy's); ``sum`` / ``max`` / ``min`` (``np.int64``), ``mean``
  (``np.float64``) and ``count_nonzero`` of a whole array; ``where(mask, a,
  b)``.  Keyword forms (``out=``, ``dtype=``, ``axis=``) and every other
  function of an int64 array go to the host.

Everything else copies the operands to the host (``__array__``) and runs
numpy there, with one ``HostFallbackWarning`` per function per process
(``BEE_OFFLOAD_WARN=0`` silences it).  ``np.sum(device_array)`` used to
take that copy silently for every call (the class had only ``__array__``).

The reference has no GPU path at all; this is the in-sandbox half of the
north star's "sandboxed code calls the HIP kernels in place of numpy"
(BASELINE.json), opt-in through ``ops/numpy_offload.py``.
"""

from __future__ import annotations

import math
import os
import warnings
from typing import Any, Callable, Optional

from ._lazy import np


def _array_module():
    # (the package exports a function named `array`: reach the module itself)
    import importlib

    return importlib.import_module(__package__ + ".array")


class HostFallbackWarning(UserWarning):
    """A numpy call on a device array ran on the host (operands copied)."""


_WARNED: set = set()


def warn_fallback(what: str) -> None:
    if what in _WARNED or os.environ.get("BEE_OFFLOAD_WARN", "1") == "0":
        return
    _WARNED.add(what)
    warnings.warn(f"beekern: numpy.{what} has no GPU kernel for these operands; they were copied to the host",
                  HostFallbackWarning, stacklevel=4)


_UNARY = {"square": "square", "negative": "negative", "absolute": "abs", "sqrt": "sqrt", "exp": "exp", "log": "log",
          "sin": "sin", "cos": "cos", "tanh": "tanh"}
_BINARY = {"add": "add", "subtract": "subtract", "multiply": "multiply", "divide": "divide",
           "true_divide": "divide", "maximum": "maximum", "minimum": "minimum", "power": "power"}
_REDUCE = {"add": "sum", "maximum": "amax", "minimum": "amin"}
_COMPARE = ("less", "less_equal", "greater", "greater_equal", "equal", "not_equal")
# on bool masks the bitwise ufuncs are the logical ones
_LOGICAL = {"logical_and": "logical_and", "logical_or": "logical_or", "logical_xor": "logical_xor",
            "logical_not": "logical_not", "bitwise_and": "logical_and", "bitwise_or": "logical_or",
            "bitwise_xor": "logical_xor", "invert": "logical_not"}


class Binding:
    """How one array class plugs into the dispatch: ``dev(x)`` -> the
    device array behind ``x`` (or None if ``x`` is not device-resident),
    ``box(d)`` -> a result device array as the caller's class, ``host(x)`` ->
    the ndarray for a host fallback, ``scalar(v, dtype)`` -> a reduction's
    result as numpy would type it."""

    def __init__(self, dev: Callable, box: Callable, host: Callable, is_mine: Callable) -> None:
        self.dev, self.box, self.host, self.is_mine = dev, box, host, is_mine


def _weak_scalar_ok(s, dtype_name: str) -> bool:
    """A scalar operand keeps the array's dtype (numpy 2 / NEP 50): Python
    int / float / bool are weak; a numpy scalar must not promote."""
    if isinstance(s, (np.floating, np.integer, np.bool_)):  # (np.float64 is also a Python float)
        if dtype_name == "bfloat16":
            return False
        return np.result_type(np.dtype(dtype_name), s) == np.dtype(dtype_name)
    if isinstance(s, (bool, int, float)):
        return not isinstance(s, int) or abs(s) < 2**53
    return False


def _as_result_scalar(v, dtype_name: str):
    """numpy types a full reduction by the array's dtype (f32 -> float32); of
    a bool mask: a count is int64, a mean float64, any / all bool."""
    if dtype_name == "bool":
        if isinstance(v, (bool, np.bool_)):
            return np.bool_(v)
        return np.int64(v) if isinstance(v, (int, np.integer)) else np.float64(v)
    if dtype_name == "int64":  # sum / max / min are int64, a mean float64
        return np.int64(v) if isinstance(v, (int, np.integer)) else np.float64(v)
    if dtype_name == "float32":
        return np.float32(v)
    return np.float64(v)


def _host_args(b: Binding, obj):
    if b.is_mine(obj):
        return b.host(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_host_args(b, o) for o in obj)
    if isinstance(obj, dict):
        return {k: _host_args(b, v) for k, v in obj.items()}
    return obj


def _any_on_device(b: Binding, objs) -> bool:
    """Whether a host fallback moves anything off the device (arrays already
    on the host -- an offloaded array after its first host operation -- are
    plain numpy from then on: no warning)."""
    for o in objs:
        if b.dev(o) is not None:
            return True
        if isinstance(o, (list, tuple)) and _any_on_device(b, o):
            return True
    return False


_FP = ("float32", "float64")


def _matmul(b: Binding, A, x, y, name: str = "matmul"):
    """The device result of numpy's ``matmul`` / ``dot`` of ``x`` and ``y``
    (numpy's dtype rules and 1-D semantics), or None for a host fallback.

    One operand may be a host ndarray (or list) when the other is on the
    device: it is uploaded once -- a product with a device array is worth one
    host-to-device copy of the other operand -- and the result stays on the
    device.  N-D (batched) operands, integer results and shape errors go to
    numpy on the host (which raises numpy's own error for the last)."""
    dx, dy = b.dev(x), b.dev(y)
    if dx is None and dy is None:
        return None
    if (dx is None and b.is_mine(x)) or (dy is None and b.is_mine(y)):
        return None  # a host-resident offload array: everything stays on the host
    if "int64" in (getattr(dx, "dtype", None), getattr(dy, "dtype", None)):
        return None  # (no integer product on the device)
    if "bfloat16" in (getattr(dx, "dtype", None), getattr(dy, "dtype", None)):
        if dx is None or dy is None or dx.dtype != dy.dtype or dx.ndim != 2 or dy.ndim != 2 or \
                dx.shape[1] != dy.shape[0]:
            return None
        return A.matmul(dx, dy)

    def np_dtype(obj, d):
        if d is not None:
            return np.dtype(d.dtype)
        h = np.asarray(obj)
        return h.dtype if h.dtype.kind in "biuf" and h.ndim in (1, 2) and h.size else None

    tx, ty = np_dtype(x, dx), np_dtype(y, dy)
    if tx is None or ty is None:
        return None
    rt = np.result_type(tx, ty)
    if rt.name not in _FP:
        return None
    shapes = [d.shape if d is not None else np.shape(o) for o, d in ((x, dx), (y, dy))]
    if any(len(s) not in (1, 2) for s in shapes):
        return None
    if name == "dot" and len(shapes[0]) == 1 and len(shapes[1]) == 1:
        return None  # (1-D . 1-D is the reduction path)
    kx = shapes[0][-1]
    ky = shapes[1][0]
    if kx != ky:
        return None
    if dx is None:
        dx = A.asarray(np.asarray(x), rt.name)
    if dy is None:
        dy = A.asarray(np.asarray(y), rt.name)
    if os.environ.get("BEE_NUMPY_OFFLOAD_MATMUL", "") == "bf16" and dx.ndim == 2 and dy.ndim == 2:
        return A.matmul(dx, dy, out_dtype="float32").astype(rt.name)
    return A.matmul_fp(dx, dy)


def array_ufunc(b: Binding, ufunc, method: str, inputs, kwargs):
    A = _array_module()

    out = kwargs.get("out")
    extra = {k for k in kwargs if k != "out"}
    name = ufunc.__name__
    res = _try_ufunc(b, A, ufunc, name, method, inputs, kwargs, extra)
    if res is not None:
        if out is not None:
            target = b.dev(out[0])
            A._before_write(target)  # (lazy masks of the old values run first)
            A.driver().unary(A._UNARY["copy"], target.code, res.ptr, target.ptr, target.size)
            return out[0]
        return b.box(res) if isinstance(res, A.DeviceArray) else res
    if _any_on_device(b, inputs):
        warn_fallback(name if method == "__call__" else f"{name}.{method}")
    return getattr(ufunc, method)(*_host_args(b, inputs), **_host_args(b, kwargs))


def _try_ufunc(b, A, ufunc, name, method, inputs, kwargs, extra) -> Optional[Any]:
    """The GPU result (DeviceArray or numpy scalar), or None for a host fallback."""
    out = kwargs.get("out")
    if method == "__call__":
        if extra - {"dtype"}:
            return None
        if name == "matmul":
            if len(inputs) != 2 or out is not None or kwargs.get("dtype") is not None:
                return None
            return _matmul(b, A, inputs[0], inputs[1])
        devs = [b.dev(x) for x in inputs]
        arrays = [d for d in devs if d is not None]
        if not arrays or any(b.is_mine(x) and d is None for x, d in zip(inputs, devs)):
            return None  # a host-resident operand: everything stays on the host
        if any(d.dtype == "int64" for d in arrays):
            return None if (out is not None or extra) else _try_int_ufunc(A, name, inputs, devs)
        dt = arrays[0].dtype
        if kwargs.get("dtype") is not None and np.dtype(kwargs["dtype"]).name != dt:
            return None
        if any(d.dtype != dt for d in arrays):
            return None
        if name in _COMPARE or name in _LOGICAL or dt == "bool":
            if out is not None or kwargs.get("dtype") is not None:
                return None
            return _try_mask_ufunc(A, name, inputs, devs, dt)
        if out is not None:
            if len(out) != 1 or b.dev(out[0]) is None:
                return None
            o = b.dev(out[0])
            shape = arrays[0].shape if len(arrays) == 1 else A._broadcast_shape(arrays[0].shape, arrays[1].shape)
            if o.dtype != dt or o.shape != shape or o._transposed:
                return None
            o._materialize()  # (a lazy draw gets its buffer: the result is written into it)
        if name in _UNARY and len(inputs) == 1:
            x = devs[0]
            return A.square(x) if name == "square" else A._unary(_UNARY[name], x)
        if name in _BINARY and len(inputs) == 2:
            x, y = devs
            if x is not None and y is not None:
                if x.shape != y.shape:
                    # a matrix against a vector along one axis, or two shapes of the same elements
                    return None if 1 in (x.size, y.size) else A._binary_unequal(_BINARY[name], x, y, False)
                if name == "multiply" and inputs[0] is inputs[1]:
                    return A.square(x)
                return A._binary(_BINARY[name], x, y)
            arr, s, rev = (x, inputs[1], False) if x is not None else (y, inputs[0], True)
            if not _weak_scalar_ok(s, dt):
                return None
            if name == "power" and not rev and float(s) == 2.0:
                return A.square(arr)
            return A._binary(_BINARY[name], arr, float(s), reversed_=rev)
        return None
    if method == "reduce" and name in _REDUCE and len(inputs) == 1 and out is None:
        if extra - {"axis", "dtype"}:
            return None
        x = b.dev(inputs[0])
        if x is None or (kwargs.get("dtype") is not None and np.dtype(kwargs["dtype"]).name != x.dtype):
            return None
        axis = kwargs.get("axis", 0)
        if axis is None or (x.ndim == 1 and axis in (0, -1)):
            return _full_reduce(A, _REDUCE[name], x)
        if x.dtype == "int64":
            return None  # (no axis reductions of int64 arrays)
        if x.ndim == 2 and _is_axis(axis, (0, 1, -1, -2)):
            if name == "add":
                return A.sum(x, axis=axis)
            if x.dtype in _FP:
                return _axis_result(lambda: A.amax(x, axis) if name == "maximum" else A.amin(x, axis))
        return None
    return None


_INT_BINARY = {"add": "add", "subtract": "subtract", "multiply": "multiply", "floor_divide": "floor_divide",
               "remainder": "remainder", "mod": "remainder", "true_divide": "divide", "divide": "divide",
               "maximum": "maximum", "minimum": "minimum"}
_INT_UNARY = {"negative": "negative", "absolute": "abs"}
_INT_FUNCTIONS = ("sum", "mean", "max", "min", "amax", "amin", "count_nonzero")
_ANY_DTYPE_FUNCTIONS = ("shape", "ndim", "size", "copy", "reshape", "ravel")


def _try_int_ufunc(A, name, inputs, devs) -> Optional[Any]:
    """A ufunc with an int64 device array among its inputs (no ``out=``, no keywords): the device result
    under the rules of ``ops/array.py``'s int64 section, or None for a host fallback.  An integer scalar that
    does not fit int64 raises OverflowError, as numpy 2 does."""
    operands = []
    for x, d in zip(inputs, devs):
        if d is not None:
            if d.dtype not in ("int64", "float32", "float64"):
                return None
            operands.append(d)
        elif isinstance(x, (bool, int, float, np.floating, np.integer, np.bool_)) and getattr(x, "itemsize", 8) <= 8:
            operands.append(x)
        else:
            return None  # (a host array or something else: numpy decides)
    try:
        if name in _INT_UNARY and len(operands) == 1:
            return A._unary(_INT_UNARY[name], operands[0])
        if len(operands) != 2:
            return None
        x, y = operands
        if isinstance(x, A.DeviceArray) and isinstance(y, A.DeviceArray) and x.shape != y.shape:
            return None
        if name in _INT_BINARY:
            return A._int_binary(_INT_BINARY[name], x, y, False)
        if name in _COMPARE:
            return A._compare(name, x, y)
    except (TypeError, ValueError):
        return None
    return None


def _try_int_function(b, A, name, args, kwargs, x):
    """A numpy function whose first argument is the int64 device array ``x``: sum / max / min / mean /
    count_nonzero of the whole array, or _NO."""
    if name not in _INT_FUNCTIONS:
        return _NO
    got = _bind(name, args, kwargs, ("a",))
    if got is None or set(got) != {"a"}:
        return _NO  # (axis=, dtype=, out=, keepdims=, ...: numpy's own answer)
    if name == "count_nonzero":
        return A.count_nonzero(x)
    if name in ("max", "min", "amax", "amin") and x.size == 0:
        return _NO
    fn = {"sum": A.sum, "mean": A.mean, "max": A.amax, "amax": A.amax, "min": A.amin, "amin": A.amin}[name]
    return _as_result_scalar(fn(x), "int64")


def _is_axis(axis, allowed) -> bool:
    return isinstance(axis, (int, np.integer)) and not isinstance(axis, (bool, np.bool_)) and axis in allowed


def _axis_result(fn):
    """An axis reduction's device result, or None where the ops layer refuses
    it (an empty axis, too many columns, ddof >= n): numpy decides, on the host."""
    try:
        return fn()
    except (ValueError, TypeError):
        return None


def _try_mask_ufunc(A, name, inputs, devs, dt) -> Optional[Any]:
    """A comparison of float arrays, or mask logic on bool arrays: the device
    mask, or None for a host fallback."""
    if name in _COMPARE and len(inputs) == 2 and dt != "bool":
        x, y = devs
        if x is not None and y is not None:
            return A._compare(name, x, y) if x.shape == y.shape else None
        arr, s, rev = (x, inputs[1], False) if x is not None else (y, inputs[0], True)
        if isinstance(s, (np.floating, np.integer, np.bool_)):
            # weak or strong, the kernel compares in f64: a promoting numpy
            # scalar (np.float64 against f32) goes unrounded -- numpy's
            # promoted comparison (wider than f64: numpy on the host)
            if s.dtype.itemsize > 8:
                return None
        elif not _weak_scalar_ok(s, dt):
            return None
        return A._compare(name, s, arr) if rev else A._compare(name, arr, s)
    if name in _LOGICAL and dt == "bool":
        if any(d is None for d in devs):
            return None  # (a scalar or host operand)
        if len(devs) == 1 and _LOGICAL[name] == "logical_not":
            return A.logical_not(devs[0])
        if len(devs) == 2 and _LOGICAL[name] != "logical_not" and devs[0].shape == devs[1].shape:
            return A._logical(_LOGICAL[name], devs[0], devs[1])
    return None


def _full_reduce(A, what: str, x):
    if x.dtype == "bool":  # numpy: add.reduce counts (int64), max / min are any / all
        return _as_result_scalar(A.sum(x) if what == "sum" else A.any(x) if what == "amax" else A.all(x), "bool")
    v = A.sum(x) if what == "sum" else A.amax(x) if what == "amax" else A.amin(x)
    return _as_result_scalar(v, x.dtype)


_NOVALUE_NAMES = ("_NoValue", "_NoValueType")


def _given(v) -> bool:
    """An optional argument the caller actually passed (numpy forwards its
    ``np._NoValue`` sentinel for the ones left out)."""
    return v is not None and type(v).__name__ not in _NOVALUE_NAMES


def _kw_only(kwargs, allowed) -> bool:
    return all(k in allowed or not _given(v) or (k == "keepdims" and v is False) for k, v in kwargs.items())


def _keepdims(got) -> Optional[bool]:
    """The call's ``keepdims`` (False when left out); None if it is no bool."""
    k = got.get("keepdims", False)
    if not _given(k):
        return False
    return bool(k) if isinstance(k, (bool, np.bool_)) else None


def _bind(func_name: str, args, kwargs, params):
    """Positional + keyword arguments of ``func_name`` as a dict (the numpy
    signature's leading parameters ``params``); None if they do not fit."""
    if len(args) > len(params):
        return None
    got = dict(zip(params, args))
    for k, v in kwargs.items():
        if k in got:
            return None
        got[k] = v
    return got


def array_function(b: Binding, func, types, args, kwargs):
    A = _array_module()

    name = getattr(func, "__name__", str(func))
    mod = getattr(func, "__module__", "") or ""
    res = _try_function(b, A, name, mod, args, kwargs)
    if res is not _NO:
        return res
    if _any_on_device(b, args) or _any_on_device(b, tuple(kwargs.values())):
        warn_fallback(name if not mod.endswith("linalg") else f"linalg.{name}")
    return func(*_host_args(b, args), **_host_args(b, kwargs))


_NO = object()


def _host_numbers(b: Binding, v, max_len: int):
    """A host scalar, list / tuple or ndarray (0-D or 1-D, at most ``max_len``
    long) of real numbers as a float64 ndarray, else None."""
    if b.is_mine(v) or isinstance(v, (str, bytes, bool, np.bool_)):
        return None
    if not isinstance(v, (int, float, np.integer, np.floating, list, tuple, np.ndarray)):
        return None
    try:
        a = np.asarray(v)
    except Exception:
        return None
    if a.dtype.kind not in "iuf" or a.ndim > 1 or a.size > max_len or (a.ndim == 1 and isinstance(v, (list, tuple))
                                                                        and len(v) != a.size):
        return None
    return a.astype(np.float64)


def _try_quantile(b: Binding, A, name: str, args, kwargs):
    """np.median / np.percentile / np.quantile of a whole f32 / f64 device
    array, method "linear": numpy's value and type, or _NO."""
    if name == "median":
        got = _bind(name, args, kwargs, ("a", "axis", "out", "overwrite_input", "keepdims"))
        allowed = {"a", "axis"}
    else:
        got = _bind(name, args, kwargs, ("a", "q", "axis", "out", "overwrite_input", "method", "keepdims"))
        allowed = {"a", "q", "axis", "method"}
    if got is None:
        return _NO
    if got.get("overwrite_input") is False:
        del got["overwrite_input"]
    if not _kw_only(got, allowed) or (_given(got.get("method")) and got["method"] != "linear"):
        return _NO
    x = b.dev(got["a"])
    if x is None or x.dtype not in _FP or x.size == 0:
        return _NO
    axis = got.get("axis")
    if _given(axis) and not (x.ndim == 1 and isinstance(axis, (int, np.integer)) and not isinstance(axis, bool)
                             and axis in (0, -1)):
        return _NO
    if name == "median":
        return _as_result_scalar(A.median(x), x.dtype)
    if "q" not in got:
        return _NO
    q = _host_numbers(b, got["q"], 1 << 20)
    top = 100.0 if name == "percentile" else 1.0
    if q is None or not bool(np.all((q >= 0.0) & (q <= top))):  # (out of range, NaN: numpy's own error)
        return _NO
    res = A.percentile(x, q) if name == "percentile" else A.quantile(x, q)
    # numpy's result dtype follows q too (a list of Python numbers is a strong
    # float64 / int64 array, a Python scalar is weak): ask numpy, on one element
    like = getattr(np, name)(np.zeros(1, np.dtype(x.dtype)), got["q"])
    return like.dtype.type(res) if q.ndim == 0 else res.astype(like.dtype)


def _try_histogram(b: Binding, A, args, kwargs):
    """np.histogram of a whole f32 / f64 device array: (int64 counts -- or the
    density -- and numpy's edges), host ndarrays, or _NO."""
    got = _bind("histogram", args, kwargs, ("a", "bins", "range", "density", "weights"))
    if got is None or not _kw_only(got, {"a", "bins", "range", "density"}):
        return _NO
    x = b.dev(got["a"])
    if x is None or x.dtype not in _FP or x.size == 0:
        return _NO
    bins = got.get("bins", 10)
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_)):
        if not 1 <= int(bins) <= A.MAX_HISTOGRAM_BINS:
            return _NO
        bins = int(bins)
    else:
        e = _host_numbers(b, bins, A.MAX_HISTOGRAM_BINS + 1)
        if e is None or e.ndim != 1 or e.size < 2 or not np.isfinite(e).all() or bool(np.any(e[:-1] > e[1:])):
            return _NO
    rng = got.get("range")
    if rng is not None:
        r = _host_numbers(b, rng, 2) if isinstance(rng, (list, tuple, np.ndarray)) else None
        if r is None or r.shape != (2,) or not np.isfinite(r).all() or r[0] > r[1]:
            return _NO
        rng = (rng[0], rng[1])
    density = got.get("density")
    if density is not None and not isinstance(density, (bool, np.bool_)):
        return _NO
    return A.histogram(x, bins, range=rng, density=bool(density))


def _try_function(b, A, name, mod, args, kwargs):
    first = b.dev(args[0]) if args else None
    if first is not None and first.dtype == "int64" and name not in _ANY_DTYPE_FUNCTIONS:
        return _try_int_function(b, A, name, args, kwargs, first)
    if name in ("shape", "ndim", "size") and args and b.dev(args[0]) is not None and len(args) + len(kwargs) == 1:
        d = b.dev(args[0])
        return {"shape": d.shape, "ndim": d.ndim, "size": d.size}[name]
    if name in ("sum", "mean"):
        got = _bind(name, args, kwargs, ("a", "axis", "dtype", "out", "keepdims"))
        if got is None or not _kw_only(got, {"a", "axis", "keepdims"}):
            return _NO
        x = b.dev(got["a"])
        keep = _keepdims(got)
        if x is None or keep is None:
            return _NO
        fn = A.sum if name == "sum" else A.mean
        axis = got.get("axis")
        if axis is None or (x.ndim == 1 and _is_axis(axis, (0, -1))):
            if keep:  # a one-element array of the input's dimensions
                return _NO if x.dtype == "bool" or x.ndim > 2 else b.box(fn(x, None, True))
            return _as_result_scalar(fn(x), x.dtype)
        if x.dtype == "bool":
            return _NO
        if x.ndim == 2 and _is_axis(axis, (0, 1, -1, -2)):
            return b.box(fn(x, int(axis), keep))
        return _NO
    if name in ("max", "min", "amax", "amin"):
        got = _bind(name, args, kwargs, ("a", "axis", "out", "keepdims"))
        if got is None or not _kw_only(got, {"a", "axis", "keepdims"}):
            return _NO
        x = b.dev(got["a"])
        keep = _keepdims(got)
        if x is None or keep is None:
            return _NO
        what = "amax" if name in ("max", "amax") else "amin"
        axis = got.get("axis")
        if not _given(axis) or (x.ndim == 1 and _is_axis(axis, (0, -1))):
            if not keep:
                return _full_reduce(A, what, x)
            axis = None
        elif not (x.ndim == 2 and _is_axis(axis, (0, 1, -1, -2))):
            return _NO
        if x.dtype not in _FP or x.ndim > 2:
            return _NO
        res = _axis_result(lambda: getattr(A, what)(x, None if axis is None else int(axis), keep))
        return _NO if res is None else b.box(res)
    if name in ("var", "std"):
        got = _bind(name, args, kwargs, ("a", "axis", "dtype", "out", "ddof", "keepdims"))
        if got is None or not _kw_only(got, {"a", "axis", "ddof", "keepdims"}):
            return _NO
        x = b.dev(got["a"])
        keep = _keepdims(got)
        ddof = got.get("ddof", 0) if _given(got.get("ddof")) else 0
        if x is None or keep is None or x.dtype in ("bfloat16", "bool") or isinstance(ddof, bool) or \
                not isinstance(ddof, (int, float)):
            return _NO
        axis = got.get("axis")
        if _given(axis) and not (x.ndim == 1 and _is_axis(axis, (0, -1))):
            if not (x.ndim == 2 and _is_axis(axis, (0, 1, -1, -2))):
                return _NO
            res = _axis_result(lambda: getattr(A, name)(x, int(axis), ddof, keep))
            return _NO if res is None else b.box(res)
        n = x.size
        if n - ddof <= 0 or (keep and x.ndim > 2):
            return _NO
        m = float(A.mean(x))
        v = float(A.square_sum(A._binary("subtract", x, m))) / (n - ddof)  # two passes, as numpy
        v = _as_result_scalar(math.sqrt(v) if name == "std" else v, x.dtype)
        return b.box(A._kept(v, x, None)) if keep else v
    if name == "norm" and mod.endswith("linalg"):
        got = _bind(name, args, kwargs, ("x", "ord", "axis", "keepdims"))
        if got is None or not _kw_only(got, {"x"}):
            return _NO
        x = b.dev(got["x"])
        if x is None or x.dtype == "bool":
            return _NO
        return _as_result_scalar(math.sqrt(float(A.square_sum(x))), x.dtype)
    if name in ("dot", "vdot", "inner"):
        if len(args) != 2 or not _kw_only(kwargs, ()):
            return _NO
        x, y = b.dev(args[0]), b.dev(args[1])
        if x is not None and y is not None and x.ndim == 1 and y.ndim == 1 and x.shape == y.shape and \
                x.dtype == y.dtype and x.dtype != "bool":
            return _as_result_scalar(A.dot(x, y), x.dtype)
        if name == "dot":
            r = _matmul(b, A, args[0], args[1], "dot")
            return _NO if r is None else b.box(r)
        return _NO
    if name in ("count_nonzero", "any", "all"):
        params = ("a", "axis") if name == "count_nonzero" else ("a", "axis", "out")
        got = _bind(name, args, kwargs, params)
        if got is None or not _kw_only(got, {"a"}):
            return _NO
        x = b.dev(got["a"])
        if x is None:
            return _NO
        if name == "count_nonzero":  # (of a float array: the fused != 0 count)
            return A.count_nonzero(x)
        count = A.count_nonzero(x) if x.dtype != "bool" else None
        if name == "any":
            return np.bool_(count > 0 if count is not None else A.any(x))
        return np.bool_(count == x.size if count is not None else A.all(x))
    if name == "where":
        if len(args) != 3 or kwargs:
            return _NO  # (the one-argument form is nonzero(): host)
        cond = b.dev(args[0])
        if cond is None or cond.dtype != "bool":
            return _NO
        vals = []
        for v in args[1:]:
            if b.is_mine(v):
                d = b.dev(v)
                if d is None:
                    return _NO  # a host-resident operand: everything stays on the host
                vals.append(d)
            elif isinstance(v, (bool, int, float, np.floating, np.integer, np.bool_)):
                vals.append(v)
            else:
                return _NO
        arrays = [v for v in vals if isinstance(v, A.DeviceArray)]
        dtype = None
        if arrays:
            if not all(_weak_scalar_ok(v, arrays[0].dtype) for v in vals if not isinstance(v, A.DeviceArray)):
                return _NO
        else:
            dtype = np.result_type(*vals).name
            if dtype not in _FP:
                return _NO  # (two integers: an integer result, numpy's on the host)
        try:
            return b.box(A.where(cond, vals[0], vals[1], dtype=dtype))
        except (TypeError, ValueError):
            return _NO
    if name in ("median", "percentile", "quantile"):
        return _try_quantile(b, A, name, args, kwargs)
    if name == "histogram":
        return _try_histogram(b, A, args, kwargs)
    if name == "copy" and len(args) == 1 and not kwargs:
        x = b.dev(args[0])
        return _NO if x is None else b.box(x.copy())
    if name in ("reshape", "ravel"):
        params = ("a", "shape") if name == "reshape" else ("a",)
        kw = dict(kwargs)
        if name == "reshape" and "newshape" in kw:  # numpy < 2.1's name, deprecated but still accepted
            if "shape" in kw or len(args) > 1:
                return _NO
            kw["shape"] = kw.pop("newshape")
        got = _bind(name, args, kw, params + ("order",))
        # anything else (copy=..., unknown keywords): numpy decides, on the host
        if got is None or set(got) - set(params) - {"order"} or got.get("order", "C") not in ("C", None):
            return _NO
        if name == "reshape" and "shape" not in got:
            return _NO
        x = b.dev(got["a"])
        if x is None:
            return _NO
        shape = got.get("shape", -1) if name == "reshape" else -1
        try:
            return b.box(x.reshape(shape))
        except (ValueError, TypeError):
            return _NO
    return _NO

"""2-D broadcasting and the axis reductions above the kernels, on CPU:
``ops/array.py`` (``_binary`` against a vector, amax / amin / var / std,
keepdims), the numpy protocols (``ops/npinterop.py``) and the offload
(``ops/numpy_offload.py``) over the numpy model of the two kernels
(tests/host_driver_axis.py), which records the launches.  These tests check the
Python layers against numpy on the same host data: which operand is the
vector, kinds and flags, ``.T`` views, shapes, result types, fallbacks.  The
kernels themselves: tests/test_axis_gpu.py."""

import os
import runpy
import warnings

import numpy as np
import pytest

from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops import npinterop, numpy_offload
from bee_code_interpreter_fs_amd.ops.npinterop import HostFallbackWarning
from bee_code_interpreter_fs_amd.ops.numpy_offload import OffloadArray

from .host_driver_axis import use_axis_host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, C = 7, 5
DTYPES = ["float64", "float32"]


@pytest.fixture
def drv(monkeypatch):
    d = use_axis_host_driver(monkeypatch)
    monkeypatch.setattr(npinterop, "_WARNED", set())
    return d


@pytest.fixture
def offload(drv, monkeypatch):
    monkeypatch.setattr(numpy_offload, "MIN_ELEMENTS", 1 << 12)
    monkeypatch.setattr(numpy_offload, "_GEN", [])
    numpy_offload.patch_numpy_random(np.random, setter=lambda o, k, v: monkeypatch.setattr(o, k, v, raising=False))
    return drv


def kernels(drv):
    return [op[0] for op in drv.launches if op[0] != "d2h"]


def table(dtype, rows=R, cols=C, seed=0):
    return (np.random.default_rng(seed).standard_normal((rows, cols)) + 2.0).astype(dtype)


# ---- broadcasting ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vshape,kind", [((C,), 0), ((1, C), 0), ((R, 1), 1)])
def test_matrix_against_a_vector_on_either_side(drv, dtype, vshape, kind):
    h = table(dtype)
    hv = (np.random.default_rng(1).standard_normal(vshape) + 3.0).astype(dtype)
    x, v = ops.asarray(h, dtype), ops.asarray(hv, dtype)
    cases = [(ops.subtract, np.subtract, 1), (ops.divide, np.divide, 3), (lambda a, b: a - b, np.subtract, 1),
             (lambda a, b: a / b, np.divide, 3), (lambda a, b: a + b, np.add, 0), (lambda a, b: a * b, np.multiply, 2),
             (lambda a, b: a ** b, np.power, 6), (ops.maximum, np.maximum, 4), (ops.minimum, np.minimum, 5)]
    for fn, ref, code in cases:
        for (a, b), (ha, hb), swapped in (((x, v), (h, hv), False), ((v, x), (hv, h), True)):
            del drv.launches[:]
            got = fn(a, b)
            assert drv.launches == [("broadcast", code, kind, swapped, R, C)]
            with np.errstate(all="ignore"):  # (a negative base to a fractional power: NaN on both sides)
                want = ref(ha, hb)
            assert got.shape == want.shape == (R, C) and got.dtype == dtype
            np.testing.assert_array_equal(got.numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reflected_operators_with_a_host_vector(drv, dtype):
    # ndarray - DeviceArray: __array_priority__ hands it to __rsub__
    h = table(dtype)
    hv = np.arange(1.0, C + 1).astype(dtype)
    x = ops.asarray(h, dtype)
    del drv.launches[:]
    got = x.__rsub__(ops.asarray(hv, dtype))
    assert drv.launches == [("broadcast", 1, 0, True, R, C)]
    np.testing.assert_array_equal(got.numpy(), hv - h)
    np.testing.assert_array_equal(x.__rtruediv__(ops.asarray(hv, dtype)).numpy(), hv / h)


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_sizes_take_the_plain_kernel(drv, dtype):
    hv, hw = np.arange(1.0, C + 1).astype(dtype), np.linspace(2, 3, C).astype(dtype).reshape(1, C)
    v, w = ops.asarray(hv, dtype), ops.asarray(hw, dtype)
    for a, b, ha, hb in ((v, w, hv, hw), (w, v, hw, hv)):
        del drv.launches[:]
        got = ops.subtract(a, b)
        assert kernels(drv) == ["binary"]
        assert got.shape == (1, C)
        np.testing.assert_array_equal(got.numpy(), ha - hb)
    col = ops.asarray(hv.reshape(C, 1), dtype)
    assert (col / ops.asarray(hv.reshape(C, 1) + 1, dtype)).shape == (C, 1)
    # a single element keeps its shortcut: the scalar form of the plain kernel, the other operand's shape
    del drv.launches[:]
    got = ops.asarray(table(dtype), dtype) - ops.asarray(np.array([[2.0]], dtype), dtype)
    assert kernels(drv) == ["binary"] and got.shape == (R, C)
    one = ops.asarray(np.array([3.0], dtype), dtype)
    assert (one - ops.asarray(np.array([[2.0]], dtype), dtype)).shape == (1,)
    assert (ops.asarray(np.full((1, 1, 1), 5.0, dtype), dtype) * one).numpy().tolist() == [[[15.0]]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_matrix_operand(drv, dtype):
    h = table(dtype)  # (R, C): h.T is (C, R)
    x = ops.asarray(h, dtype)
    for hv in (np.arange(1.0, R + 1).astype(dtype), np.arange(1.0, R + 1).astype(dtype).reshape(1, R),
               np.arange(1.0, C + 1).astype(dtype).reshape(C, 1)):
        v = ops.asarray(hv, dtype)
        for fn in (lambda a, b: a - b, lambda a, b: b / a):
            del drv.launches[:]
            got = fn(x.T, v)
            want = fn(h.T, hv)
            assert got.shape == want.shape == (C, R)
            np.testing.assert_array_equal(got.numpy(), want)
            # the buffer is read in place with the vector along its other axis
            assert [k for k in kernels(drv) if k in ("broadcast", "transpose")][0] == "broadcast"
            launch = [op for op in drv.launches if op[0] == "broadcast"][0]
            assert launch[2] == (1 if hv.shape != (C, 1) else 0) and launch[4:] == (R, C)
    # the result of a .T operand is usable as any other array
    z = x.T - ops.asarray(np.ones(R, dtype), dtype)
    np.testing.assert_array_equal((z + z).numpy(), (h.T - 1) + (h.T - 1))
    np.testing.assert_array_equal(ops.sum(z, axis=0).numpy(), (h.T - 1).astype(np.float64).sum(axis=0).astype(dtype))


def test_shapes_that_do_not_broadcast_raise(drv):
    x = ops.asarray(table("float64"))
    with pytest.raises(ValueError):
        ops.asarray(np.ones((R, 1))) - ops.asarray(np.ones((1, C)))
    with pytest.raises(ValueError):
        x - ops.asarray(np.ones(R))
    with pytest.raises(ValueError):
        x - ops.asarray(np.ones((C, 1)))
    with pytest.raises(ValueError):
        x - ops.asarray(np.ones(C, np.float32), "float32")
    with pytest.raises(ValueError):
        ops.asarray(np.ones((2, R, C))) - ops.asarray(np.ones(C))
    # bf16 has the equal-shape kernel only
    xb = ops.asarray(table("float64"), "bfloat16")
    for vb in (np.ones(C), np.ones((1, C)), np.ones((R, 1))):
        with pytest.raises(ValueError):
            ops.subtract(xb, ops.asarray(vb, "bfloat16"))
        with pytest.raises(ValueError):
            ops.asarray(vb, "bfloat16") / xb
    with pytest.raises(TypeError):
        x - (ops.asarray(np.ones(C)) > 0.0)
    with pytest.raises(TypeError):
        (x > 0.0) + ops.asarray(np.ones(C))
    assert "broadcast" not in kernels(drv)
    # a square matrix takes a 1-D vector along its rows, as numpy
    hs = table("float64", C, C)
    np.testing.assert_array_equal((ops.asarray(hs) - ops.asarray(np.arange(C, dtype=float))).numpy(),
                                  hs - np.arange(C, dtype=float))


# ---- reductions ---------------------------------------------------------------------------

def f64_stat(h, what, axis, ddof=0, keepdims=False):
    """The kernels' contract: f64 arithmetic on the widened data, rounded once."""
    w = h.astype(np.float64)
    kw = dict(axis=axis, keepdims=keepdims)
    r = {"amax": lambda: w.max(**kw), "amin": lambda: w.min(**kw), "var": lambda: w.var(ddof=ddof, **kw),
         "std": lambda: w.std(ddof=ddof, **kw)}[what]()
    return r.astype(h.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1, -1, -2])
def test_axis_reductions(drv, dtype, axis):
    h = table(dtype, seed=3)
    x = ops.asarray(h, dtype)
    for what, code in (("amax", 0), ("amin", 1), ("var", 2), ("std", 3)):
        for keep in (False, True):
            del drv.launches[:]
            got = getattr(ops, what)(x, axis=axis, keepdims=keep)
            n = h.shape[axis]
            assert drv.launches == [("axis_stat", code, axis % 2, R, C, float(n) if code >= 2 else 1.0)]
            want = f64_stat(h, what, axis, keepdims=keep)
            assert got.shape == want.shape and got.dtype == dtype
            tol = 4 * np.finfo(dtype).eps if code >= 2 else 0  # (numpy's pairwise sums against the model's)
            np.testing.assert_allclose(got.numpy(), want, rtol=tol, atol=0)
    for what in ("var", "std"):
        got = getattr(ops, what)(x, axis=axis, ddof=1)
        assert drv.launches[-1][5] == float(h.shape[axis] - 1)
        np.testing.assert_allclose(got.numpy(), f64_stat(h, what, axis, ddof=1), rtol=4 * np.finfo(dtype).eps)
    # the methods, sum and mean with keepdims
    np.testing.assert_array_equal(x.max(axis=axis).numpy(), h.max(axis=axis))
    np.testing.assert_array_equal(x.min(axis, keepdims=True).numpy(), h.min(axis=axis, keepdims=True))
    assert x.var(axis=axis, ddof=1).shape == x.std(axis).shape == h.var(axis=axis).shape
    for fn in ("sum", "mean"):
        got = getattr(x, fn)(axis=axis, keepdims=True)
        want = getattr(h.astype(np.float64), fn)(axis=axis, keepdims=True)
        assert got.shape == want.shape and got.dtype == dtype
        np.testing.assert_allclose(got.numpy(), want.astype(dtype), rtol=4 * np.finfo(dtype).eps)
        assert getattr(ops, fn)(x, axis, True).shape == want.shape


@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_views_reduce_the_buffer_the_other_way(drv, dtype):
    h = table(dtype, seed=4)
    x = ops.asarray(h, dtype)
    for axis in (0, 1):
        del drv.launches[:]
        np.testing.assert_array_equal(ops.amax(x.T, axis=axis).numpy(), h.T.max(axis=axis))
        np.testing.assert_allclose(ops.std(x.T, axis=axis, ddof=1, keepdims=True).numpy(),
                                   f64_stat(h.T, "std", axis, 1, True), rtol=4 * np.finfo(dtype).eps)
        assert kernels(drv) == ["axis_stat", "axis_stat"]
        assert all(op[2] == 1 - axis and op[3:5] == (R, C) for op in drv.launches if op[0] == "axis_stat")


def test_reduction_errors(drv):
    h = table("float64")
    x = ops.asarray(h)
    for bad in (ops.asarray(h, "bfloat16"), x > 0.0):
        for fn in (ops.amax, ops.amin, ops.var, ops.std):
            with pytest.raises(TypeError):
                fn(bad, axis=0)
    for fn in (ops.var, ops.std):
        with pytest.raises(ValueError):
            fn(x, axis=0, ddof=R)
        with pytest.raises(ValueError):
            fn(x, axis=1, ddof=C + 1)
        with pytest.raises(ValueError):
            fn(x, ddof=R * C)
    with pytest.raises(ValueError):
        ops.amax(x, axis=2)
    with pytest.raises(ValueError):
        ops.var(ops.asarray(np.ones((2, 3, 4))), axis=0)
    with pytest.raises(ValueError, match="columns"):
        ops.amax(ops.zeros((1, (1 << 18) + 1)), axis=0)
    assert "axis_stat" not in kernels(drv)
    assert ops.amax(ops.zeros((1, (1 << 18) + 1)), axis=1).shape == (1,)  # (wide rows are fine)
    assert ops.var(x, axis=1, ddof=C - 1).shape == (R,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_dimensional_arrays_give_scalars(drv, dtype):
    h = np.random.default_rng(6).standard_normal(50).astype(dtype)
    x = ops.asarray(h, dtype)
    for axis in (0, -1, None):
        assert ops.amax(x, axis=axis) == h.max() and ops.amin(x, axis=axis) == h.min()
        assert np.ndim(ops.amax(x, axis=axis)) == 0
        v, s = ops.var(x, axis=axis, ddof=1), ops.std(x, axis=axis)
        assert type(v) is type(s) is np.dtype(dtype).type
        np.testing.assert_allclose(v, h.astype(np.float64).var(ddof=1), rtol=4 * np.finfo(dtype).eps)
        np.testing.assert_allclose(s, h.astype(np.float64).std(), rtol=4 * np.finfo(dtype).eps)
        assert ops.amax(x, axis=axis, keepdims=True).shape == (1,)
    with pytest.raises(ValueError):
        ops.amax(x, axis=1)
    assert "axis_stat" not in kernels(drv)
    # the whole of a 2-D array
    h2 = table(dtype)
    x2 = ops.asarray(h2, dtype)
    assert ops.amax(x2) == h2.max() and x2.min() == h2.min()
    np.testing.assert_allclose(ops.var(x2), h2.astype(np.float64).var(), rtol=4 * np.finfo(dtype).eps)
    assert ops.std(x2, keepdims=True).shape == ops.sum(x2, keepdims=True).shape == (1, 1)


# ---- the numpy protocols -----------------------------------------------------------------

def same(got, want, rtol=0.0):
    """numpy's type, dtype and shape; a device array or a numpy scalar."""
    if np.ndim(want) == 0:
        assert type(got) is type(want), (type(got), type(want))
    else:
        assert isinstance(got, ops.DeviceArray), type(got)
        assert got.shape == want.shape and np.dtype(got.dtype) == want.dtype
        got = got.numpy()
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_protocol_forms_stay_on_the_device(drv, dtype):
    h = table(dtype, seed=8)
    x = ops.asarray(h, dtype)
    hc, hr = h.mean(axis=0), h.max(axis=1, keepdims=True)
    c, r = ops.asarray(hc, dtype), ops.asarray(hr, dtype)
    eps = 4 * np.finfo(dtype).eps
    with warnings.catch_warnings():
        warnings.simplefilter("error", HostFallbackWarning)
        # binary ufuncs
        for fn in (np.subtract, np.divide, np.add, np.multiply, np.maximum, np.minimum, np.power):
            with np.errstate(all="ignore"):  # (a negative base to a fractional power: NaN on both sides)
                wants = fn(h, hc), fn(hc, h), fn(h, hr), fn(hr, h)
            for got, want in zip((fn(x, c), fn(c, x), fn(x, r), fn(r, x)), wants):
                same(got, want)
        same(x - c.reshape(1, C), h - hc.reshape(1, C))
        same(np.subtract(c, c.reshape(1, C)), hc - hc.reshape(1, C))
        same(x.T / r.reshape(R), h.T / hr.reshape(R))
        out = ops.empty((R, C), dtype)
        assert np.subtract(x, c, out=out) is out
        np.testing.assert_array_equal(out.numpy(), h - hc)
        # max / min
        for fn in (np.max, np.min, np.amax, np.amin):
            for axis in (0, 1, -1, -2):
                same(fn(x, axis=axis), fn(h, axis=axis))
                same(fn(x, axis, keepdims=True), fn(h, axis, keepdims=True))
            same(fn(x), fn(h))
            same(fn(x, keepdims=True), fn(h, keepdims=True))
        same(np.maximum.reduce(x, axis=0), np.maximum.reduce(h, axis=0))
        same(np.maximum.reduce(x), np.maximum.reduce(h))  # (axis 0 by default)
        same(np.minimum.reduce(x, axis=1), np.minimum.reduce(h, axis=1))
        # var / std
        for fn in (np.var, np.std):
            for axis in (0, 1, -1, -2):
                same(fn(x, axis=axis), fn(h.astype(np.float64), axis=axis).astype(dtype), eps)
                same(fn(x, axis, ddof=1, keepdims=True),
                     fn(h.astype(np.float64), axis, ddof=1, keepdims=True).astype(dtype), eps)
                same(fn(x, axis=axis, ddof=0.5), fn(h.astype(np.float64), axis=axis, ddof=0.5).astype(dtype), eps)
            same(fn(x, ddof=1), np.dtype(dtype).type(fn(h.astype(np.float64), ddof=1)), eps)
            same(fn(x, keepdims=True), fn(h.astype(np.float64), keepdims=True).astype(dtype), eps)
            same(fn(x, ddof=2.5, keepdims=True), fn(h.astype(np.float64), ddof=2.5, keepdims=True).astype(dtype), eps)
        # sum / mean
        for fn in (np.sum, np.mean):
            for axis in (0, 1, -1, -2):
                same(fn(x, axis=axis, keepdims=True), fn(h.astype(np.float64), axis=axis, keepdims=True).astype(dtype),
                     eps)
            same(fn(x, keepdims=True), fn(h.astype(np.float64), keepdims=True).astype(dtype), eps)
            assert fn(x, keepdims=True).shape == (1, 1)
        # 1-D inputs: numpy scalars
        v = ops.asarray(hc, dtype)
        for fn in (np.max, np.min, np.var, np.std):
            same(fn(v, axis=0), np.dtype(dtype).type(fn(hc.astype(np.float64), axis=0)), eps)
            assert fn(v, axis=-1, keepdims=True).shape == (1,)
    assert "broadcast" in kernels(drv) and "axis_stat" in kernels(drv)


def test_still_falls_back(drv, monkeypatch):
    h = table("float64", seed=9)
    x = ops.asarray(h)
    c = ops.asarray(h.mean(axis=0))

    def fresh(fn, want=None):
        monkeypatch.setattr(npinterop, "_WARNED", set())
        del drv.launches[:]
        with pytest.warns(HostFallbackWarning):
            got = fn()
        assert "axis_stat" not in kernels(drv) and "broadcast" not in kernels(drv)
        if want is not None:
            np.testing.assert_array_equal(np.asarray(got), want)
        return got

    fresh(lambda: np.max(x, axis=0, out=np.empty(C)), h.max(axis=0))
    fresh(lambda: np.max(x, axis=0, initial=100.0), np.full(C, 100.0))
    fresh(lambda: np.min(x, axis=1, where=h > 0, initial=9.0), h.min(axis=1, where=h > 0, initial=9.0))
    fresh(lambda: np.max(x, axis=(0, 1)), h.max())
    fresh(lambda: np.var(x, axis=0, dtype=np.float32), h.var(axis=0, dtype=np.float32))
    fresh(lambda: np.std(x, axis=0, out=np.empty(C)), h.std(axis=0))
    fresh(lambda: np.var(x, axis=(0, 1)), h.var())
    fresh(lambda: np.var(x, axis=0, mean=h.mean(axis=0, keepdims=True)), h.var(axis=0))
    fresh(lambda: np.std(x, axis=0, correction=1), h.std(axis=0, ddof=1))
    fresh(lambda: np.sum(x, axis=0, keepdims=True, dtype=np.float32), h.sum(axis=0, keepdims=True, dtype=np.float32))
    fresh(lambda: np.mean(x, axis=(0, 1), keepdims=True), h.mean(keepdims=True))
    fresh(lambda: np.maximum.reduce(x, axis=0, keepdims=True), h.max(axis=0, keepdims=True))
    # dtypes and dimensions without a kernel
    xb = ops.asarray(h, "bfloat16")
    fresh(lambda: np.max(xb, axis=0))
    fresh(lambda: np.var(xb, axis=1))
    m = x > 2.0
    fresh(lambda: np.max(m, axis=0), (h > 2.0).max(axis=0))
    fresh(lambda: np.std(m, axis=0))
    x3 = ops.asarray(np.arange(24.0).reshape(2, 3, 4))
    fresh(lambda: np.max(x3, axis=0), np.arange(24.0).reshape(2, 3, 4).max(axis=0))
    fresh(lambda: np.var(x3, axis=2))
    fresh(lambda: np.sum(x3, keepdims=True))
    fresh(lambda: np.subtract(x3, ops.asarray(np.arange(4.0))), np.arange(24.0).reshape(2, 3, 4) - np.arange(4.0))
    # shapes and dtypes that do not go to the broadcast kernel
    fresh(lambda: np.subtract(ops.asarray(np.ones((R, 1))), ops.asarray(np.ones((1, C)))), np.zeros((R, C)))
    fresh(lambda: np.subtract(x, ops.asarray(np.ones(C, np.float32), "float32")), h - 1)
    cb = ops.asarray(np.arange(1.0, C + 1), "bfloat16")  # (exact in bf16)
    for vb, hb in ((cb, np.arange(1.0, C + 1, dtype=np.float32)), (cb.reshape(1, C), np.arange(1.0, C + 1, dtype=np.float32))):
        fresh(lambda: np.subtract(xb, vb), xb.numpy() - hb)
        fresh(lambda: np.divide(vb, xb), hb / xb.numpy())
    fresh(lambda: np.less(x, c), h < h.mean(axis=0))
    fresh(lambda: np.logical_and(x > 2.0, (c > 2.0)), (h > 2.0) & (h.mean(axis=0) > 2.0))
    fresh(lambda: np.subtract(x, c, out=ops.empty((1, R, C))))  # (out= of another shape than the result's)
    # ddof that leaves nothing: numpy's own warning and result, on the host
    monkeypatch.setattr(npinterop, "_WARNED", set())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = np.var(x, axis=0, ddof=R)
    assert any(issubclass(i.category, HostFallbackWarning) for i in w) and np.asarray(got).shape == (C,)
    # sort, cumsum and argmax stay host fallbacks
    fresh(lambda: np.sort(x, axis=0), np.sort(h, axis=0))
    fresh(lambda: np.cumsum(x, axis=1), np.cumsum(h, axis=1))
    fresh(lambda: np.argmax(x, axis=0), np.argmax(h, axis=0))
    # the accepted forms beside them stay on the device
    monkeypatch.setattr(npinterop, "_WARNED", set())
    with warnings.catch_warnings():
        warnings.simplefilter("error", HostFallbackWarning)
        np.max(x, axis=0, keepdims=False), np.var(x, axis=-1, ddof=0, dtype=None, out=None), np.subtract(x, c)
        np.sum(x, axis=None, keepdims=True), np.std(x, 1, None, None, 1, True)


# ---- the offload and the example --------------------------------------------------------

def test_offload_arrays_share_the_paths(offload):
    with warnings.catch_warnings():
        warnings.simplefilter("error", HostFallbackWarning)
        x = np.random.normal(1.0, 2.0, (1000, 8))
        assert isinstance(x, OffloadArray) and x.on_device
        z = (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
        top = x.max(axis=1, keepdims=True)
        lo = x.min(axis=0)
        v = x.var(axis=1)
        t = x.T - x.mean(axis=1)
        assert all(isinstance(a, OffloadArray) and a.on_device for a in (z, top, lo, v, t))
        assert z.shape == (1000, 8) and top.shape == (1000, 1) and lo.shape == (8,) and t.shape == (8, 1000)
    h = np.asarray(x)
    np.testing.assert_allclose(np.asarray(z), (h - h.mean(axis=0)) / h.std(axis=0, ddof=1), rtol=1e-12)
    np.testing.assert_array_equal(np.asarray(top), h.max(axis=1, keepdims=True))
    np.testing.assert_array_equal(np.asarray(lo), h.min(axis=0))
    np.testing.assert_allclose(np.asarray(v), h.var(axis=1), rtol=1e-12)
    np.testing.assert_allclose(np.asarray(t), h.T - h.mean(axis=1), rtol=1e-12)


def test_the_example_never_leaves_the_device(offload, capsys):
    with warnings.catch_warnings():
        warnings.simplefilter("error", HostFallbackWarning)
        g = runpy.run_path(os.path.join(ROOT, "examples", "standardize_softmax.py"))
    assert isinstance(g["Z"], OffloadArray) and g["Z"].on_device
    assert isinstance(g["X"], OffloadArray) and g["X"].on_device and g["P"].on_device
    ks = kernels(offload)
    assert "broadcast" in ks and "axis_stat" in ks and "gemm_fp" in ks and "transpose" not in ks
    z = np.asarray(g["Z"])
    assert z.shape == (200000, 32)
    assert np.abs(z.mean(axis=0)).max() < 1e-9 and np.abs(z.std(axis=0) - 1).max() < 1e-9
    np.testing.assert_allclose(np.asarray(g["P"]).sum(axis=1), 1.0, rtol=1e-12)
    out = capsys.readouterr().out
    for label in ("Largest |column mean|:", "Column std range:", "Softmax row sums:", "Correlation diagonal:"):
        assert label in out
    lo, hi = (float(t) for t in out.split("Correlation diagonal:")[1].split()[:2])
    assert abs(lo - 1) < 1e-9 and abs(hi - 1) < 1e-9

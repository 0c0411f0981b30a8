"""The sort family above the kernels, on CPU: ``bk.sort`` / ``argsort`` /
``argmax`` / ``argmin`` / ``take`` / ``x[idx]`` (``ops/array.py``) over the numpy
model of the three driver calls (tests/host_driver_sort.py, tests/sort_ref.py),
which records the launches.  Results against numpy, every refusal, the bool-mask
``__getitem__`` unchanged, and numpy's own functions of these names still host
fallbacks that warn.  The kernels themselves: tests/test_sort_gpu.py."""

import os
import warnings

import numpy as np
import pytest

from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops import driver as drvmod
from bee_code_interpreter_fs_amd.ops import npinterop
from bee_code_interpreter_fs_amd.ops.npinterop import HostFallbackWarning

from . import sort_ref as R
from .host_driver_sort import use_sort_host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.array([3.5, -0.0, np.nan, 0.0, -np.inf, 7.25, 3.5, np.inf, -2.0, np.nan, 1e-310, 3.5])
I = np.array([5, -7, 0, R.I64_MAX, R.I64_MIN, 3, 5, -1, 0, 5], np.int64)


@pytest.fixture
def drv(monkeypatch):
    d = use_sort_host_driver(monkeypatch)
    monkeypatch.setattr(npinterop, "_WARNED", set())
    return d


def launches(drv):
    return [op for op in drv.launches if op[0] != "d2h"]


def host(name, values):
    return R.bf16_bits(values) if name == "bfloat16" else np.asarray(values, name)


def as_float(name, a):
    return R.bf16_floats(a) if name == "bfloat16" else a


# ---- the reference itself ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "f64", "bf16", "i64"])
def test_the_reference_order_is_numpys(name):
    rng = np.random.Generator(np.random.PCG64(3))
    if name == "i64":
        a = rng.integers(R.I64_MIN, R.I64_MAX, 5000, dtype=np.int64, endpoint=True)
        a[::7] = rng.integers(-3, 3, a[::7].size)
    else:
        v = rng.standard_normal(5000) * 10.0 ** rng.integers(-30, 30, 5000)
        v[::5] = rng.integers(-2, 2, v[::5].size)
        v[::11], v[3::13], v[5::17], v[7::19] = np.nan, -0.0, np.inf, -np.inf
        a = R.bf16_bits(v) if name == "bf16" else v.astype(R.NP_DTYPES[name])
    vals = R.as_values(a, name)
    np.testing.assert_array_equal(R.argsort(a, name), np.argsort(vals, kind="stable"))
    np.testing.assert_array_equal(R.sort(a, name), np.sort(vals))
    assert R.argmax(a, name) == np.argmax(vals) and R.argmin(a, name) == np.argmin(vals)
    clean = a[~np.isnan(vals)] if name != "i64" else a
    assert R.argmax(clean, name) == np.argmax(R.as_values(clean, name))
    assert R.argmin(clean, name) == np.argmin(R.as_values(clean, name))


def test_the_reference_take_wraps_and_counts():
    x = np.arange(10.0) + 1
    got, bad = R.take(x, [0, -1, 9, -10, 10, -11, R.I64_MIN, R.I64_MAX])
    assert bad == 4 and got.tolist() == [1.0, 10.0, 10.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    got, bad = R.take(x, np.array([[1, 2], [-1, -2]]))
    assert bad == 0 and np.array_equal(got, np.take(x, [[1, 2], [-1, -2]]))


def test_the_scratch_formula_grows_with_n_and_the_index():
    f = drvmod.sort_workspace_bytes
    assert f(0, 0, False) == f(0, 0, True) == 256 + 1024 + 512 * 1024
    assert f(0, 5, False) - f(0, 0, False) == 2 * 32 and f(0, 5, True) - f(0, 5, False) == 2 * 32
    assert f(1, 1000, True) - f(1, 0, True) == 2 * 8000 + 2 * 4000
    assert f(2, 1001, False) - f(2, 0, False) == 2 * 2016
    assert [f(dt, 10, True) for dt in (3, 4, 6, 7, -1)] == [0] * 5
    assert f(0, -1, True) == 0 == f(0, drvmod.MAX_SORT_N + 1, True) and f(5, drvmod.MAX_SORT_N, True) > 0
    assert ops.array  # noqa: B015
    import importlib

    assert importlib.import_module("bee_code_interpreter_fs_amd.ops.array").MAX_SORT_N == drvmod.MAX_SORT_N == 0x7FFFFFFF


# ---- sort / argsort -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["float32", "float64", "bfloat16", "int64"])
def test_sort_and_argsort_are_numpys(drv, name):
    h = I if name == "int64" else (F.astype(np.float32) if name != "float64" else F)
    x = ops.asarray(h, dtype=name)
    want = as_float(name, host(name, h))
    del drv.launches[:]
    s = ops.sort(x)
    assert launches(drv) == [("sort", x.code, h.size, True, False)]
    assert s.dtype == name and s.shape == (h.size,)
    np.testing.assert_array_equal(np.asarray(as_float(name, s.numpy() if name != "bfloat16" else R.bf16_bits(s.numpy()))),
                                  np.sort(want))
    del drv.launches[:]
    order = ops.argsort(x)
    assert launches(drv) == [("sort", x.code, h.size, False, True)]
    assert order.dtype == "int64" and np.array_equal(order.numpy(), np.argsort(want, kind="stable"))
    assert np.array_equal(x.argsort().numpy(), order.numpy())
    for kind in ("stable", "quicksort", "mergesort", None):
        assert np.array_equal(ops.argsort(x, kind=kind).numpy(), order.numpy())
        assert ops.sort(x, kind=kind).numpy().tobytes() == s.numpy().tobytes()


def test_sort_of_nothing_one_element_and_a_lazy_operand(drv):
    e = ops.asarray(np.zeros(0), dtype="float64")
    del drv.launches[:]
    assert ops.sort(e).shape == (0,) and ops.argsort(e).dtype == "int64" and launches(drv) == []
    one = ops.asarray([4.0])
    assert ops.sort(one).numpy().tolist() == [4.0] and ops.argsort(one).numpy().tolist() == [0]
    x = ops.asarray(F)
    sq = ops.square(x)  # lazy until used
    want = np.square(F)
    np.testing.assert_array_equal(ops.sort(sq).numpy(), np.sort(want))
    assert np.array_equal(ops.argsort(ops.square(x)).numpy(), np.argsort(want, kind="stable"))
    assert ops.argmax(ops.square(x)) == np.argmax(want)
    assert np.array_equal(ops.sort([3.0, 1.0, 2.0]).numpy(), [1.0, 2.0, 3.0])  # host data is uploaded, as for other ops


def test_sort_refusals(drv, monkeypatch):
    m = ops.asarray(np.arange(6.0).reshape(2, 3))
    for fn in (ops.sort, ops.argsort):
        with pytest.raises(TypeError, match="1-D arrays only, got ndim 2"):
            fn(m)
        with pytest.raises(TypeError, match="ndim 0"):
            fn(ops.asarray(3.0))
        with pytest.raises(TypeError, match="got bool"):
            fn(ops.asarray(F) > 0)
    import importlib

    A = importlib.import_module("bee_code_interpreter_fs_amd.ops.array")
    monkeypatch.setattr(A, "MAX_SORT_N", 4)
    del drv.launches[:]
    for fn in (ops.sort, ops.argsort):
        with pytest.raises(TypeError, match=r"at most 4 elements a call \(BK_MAX_SORT_N\)"):
            fn(ops.asarray(np.arange(5.0)))
    assert launches(drv) == []
    assert ops.sort(ops.asarray(np.arange(4.0)[::-1].copy())).numpy().tolist() == [0.0, 1.0, 2.0, 3.0]


# ---- argmax / argmin ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["float32", "float64", "bfloat16", "int64"])
def test_argmax_and_argmin_are_numpys(drv, name):
    h = I if name == "int64" else (F.astype(np.float32) if name != "float64" else F)
    for hh in (h, h[[0, 1, 3, 5, 6, 8]], h[:1], h.reshape(2, -1)):
        x = ops.asarray(hh, dtype=name)
        want = as_float(name, host(name, hh))
        del drv.launches[:]
        got = ops.argmax(x)
        assert launches(drv) == [("arg_reduce", 0, x.code, hh.size)]
        assert got == np.argmax(want) and isinstance(got, np.int64)
        got = x.argmin()
        assert launches(drv)[-1] == ("arg_reduce", 1, x.code, hh.size)
        assert got == np.argmin(want) and isinstance(got, np.int64) and x.argmax() == np.argmax(want)


def test_arg_reduce_refusals(drv):
    e = ops.asarray(np.zeros(0))
    with pytest.raises(ValueError, match="attempt to get argmax of an empty sequence"):
        ops.argmax(e)
    with pytest.raises(ValueError, match="attempt to get argmin of an empty sequence"):
        e.argmin()
    m = ops.asarray(np.arange(6.0).reshape(2, 3))
    with pytest.raises(TypeError, match=r"\.T view"):
        ops.argmax(m.T)
    for call in (lambda: ops.argmax(m, axis=0), lambda: m.argmin(axis=1), lambda: ops.argmin(m, 0)):
        with pytest.raises(TypeError, match="axis= is not there yet"):
            call()
    with pytest.raises(TypeError, match="got bool"):
        ops.argmax(m > 2)
    assert launches(drv) == [] or all(op[0] != "arg_reduce" for op in launches(drv))


# ---- take / x[idx] -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["float32", "float64", "bfloat16", "int64", "bool"])
def test_take_is_numpys(drv, name):
    h = (I if name == "int64" else F.astype(np.float32) if name != "float64" else F)
    x = ops.asarray(h, dtype=name) if name != "bool" else ops.asarray(F) > 0
    hx = x.numpy()
    n = hx.size
    for idx in ([0, -1, 3, 3, -n, n - 1], np.arange(n)[::-1].copy(), np.array([[1, 2], [-1, -2]]), np.zeros(0, np.int64), []):
        del drv.launches[:]
        got = ops.take(x, idx)
        ih = np.asarray(idx, np.int64)
        assert launches(drv)[-1] == ("take", 1 if name == "int64" else x.code, n, ih.size)
        assert got.dtype == name and got.shape == ih.shape
        assert got.numpy().tobytes() == np.take(hx, ih).tobytes()
        d_idx = ops.asarray(ih, dtype="int64")
        assert ops.take(x, d_idx).numpy().tobytes() == np.take(hx, ih).tobytes()
    order = ops.argsort(x) if name != "bool" else ops.asarray(np.arange(n)[::-1].copy(), dtype="int64")
    assert x[order].numpy().tobytes() == hx[order.numpy()].tobytes()
    assert x[[1, 0, -1]].numpy().tobytes() == hx[[1, 0, -1]].tobytes()
    assert x[np.array([2, 2])].numpy().tobytes() == hx[[2, 2]].tobytes()


def test_take_refusals(drv):
    x = ops.asarray(F)
    n = F.size
    del drv.launches[:]
    for bad, shown in (([0, n], n), ([-n - 1], -n - 1), (np.array([1, 2 ** 62]), 2 ** 62)):
        with pytest.raises(IndexError, match=f"index {shown} is out of bounds for axis 0 with size {n}"):
            ops.take(x, bad)
        with pytest.raises(IndexError, match="out of bounds for axis 0"):
            x[bad]
    assert launches(drv) == []  # host indices are checked before anything is uploaded
    with pytest.raises(IndexError, match=f"out of bounds for axis 0 with size {n} \\(2 of the 3 indices\\)"):
        ops.take(x, ops.asarray([0, n, R.I64_MIN], dtype="int64"))
    with pytest.raises(IndexError):
        x[ops.asarray([n], dtype="int64")]
    with pytest.raises(TypeError, match="integer indices only"):
        ops.take(x, [0.5])
    with pytest.raises(TypeError, match="int64 array, got float64"):
        ops.take(x, ops.asarray([0.0]))
    with pytest.raises(TypeError, match="1-D arrays only, got ndim 2"):
        ops.take(ops.asarray(np.zeros((2, 2))), [0])


def test_getitem_keeps_the_mask_path_and_its_type_error(drv):
    x = ops.asarray(F)
    del drv.launches[:]
    got = x[x > 1.0]
    assert "compress" in [op[0] for op in launches(drv)] and "take" not in [op[0] for op in launches(drv)]
    np.testing.assert_array_equal(got.numpy(), F[F > 1.0])
    i = ops.asarray(I, dtype="int64")
    np.testing.assert_array_equal(i[i > 0].numpy(), I[I > 0])
    m2 = ops.asarray(np.arange(6.0).reshape(2, 3))
    np.testing.assert_array_equal(m2[m2 > 2].numpy(), np.arange(6.0)[3:])
    for key in (0, slice(0, 2), (0, 1), None, 1.5, "a", [True, False], [], [0.5], np.array([True] * F.size), ops.asarray(F),
                Ellipsis):
        with pytest.raises(TypeError, match="indexed by a bool DeviceArray of the same shape only"):
            x[key]
    with pytest.raises(TypeError, match="indexed by a bool DeviceArray"):
        m2[ops.asarray([0, 1], dtype="int64")]  # (x[idx] gathers from 1-D arrays only)
    with pytest.raises(TypeError, match="indexed by a bool DeviceArray"):
        m2[[0, 1]]


# ---- numpy's own functions stay on the host ----------------------------------------------------------------------

def test_numpy_functions_of_these_names_still_fall_back_with_a_warning(drv):
    x, i = ops.asarray(F), ops.asarray(I, dtype="int64")
    cases = [("sort", lambda: np.sort(x), lambda: np.sort(F)), ("argsort", lambda: np.argsort(x), lambda: np.argsort(F)),
             ("argmax", lambda: np.argmax(x), lambda: np.argmax(F)), ("argmin", lambda: np.argmin(i), lambda: np.argmin(I)),
             ("take", lambda: np.take(x, [0, 1]), lambda: np.take(F, [0, 1]))]
    for name, call, ref in cases:
        del drv.launches[:]
        with pytest.warns(HostFallbackWarning, match=name):
            got, want = call(), ref()
        assert not isinstance(got, ops.DeviceArray) and launches(drv) == [], name
        np.testing.assert_array_equal(got, want)


def test_offload_arrays_resolve_argmax_as_before(drv):
    """``OffloadArray.argmax()`` is ndarray's on the host copy, with the fallback warning: DeviceArray.argmax
    changes nothing there."""
    from bee_code_interpreter_fs_amd.ops.numpy_offload import OffloadArray

    assert "argmax" not in vars(OffloadArray) and "argsort" not in vars(OffloadArray)
    o = OffloadArray(ops.asarray(F))
    del drv.launches[:]
    with pytest.warns(HostFallbackWarning, match="argmax"):
        assert o.argmax() == np.argmax(F)
    assert launches(drv) == [] and not o.on_device
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert o.argmax() == np.argmax(F)  # (already on the host: no warning)


# ---- the example ----------------------------------------------------------------------------------------------------

def test_the_example_runs_on_the_model_without_a_fallback(drv, monkeypatch, capsys, tmp_path):
    """examples/top_claims.py over the numpy model: its printed lines equal numpy's on the draws it made."""
    import runpy
    import sys

    monkeypatch.setitem(sys.modules, "beekern", ops)
    src = open(os.path.join(ROOT, "examples", "top_claims.py")).read().replace("n = 2_000_000", "n = 20_000")
    path = tmp_path / "top_claims.py"
    path.write_text(src)
    with warnings.catch_warnings():
        warnings.simplefilter("error", HostFallbackWarning)
        g = runpy.run_path(str(path))
    out = capsys.readouterr().out.strip().splitlines()
    s, r = g["severity"].numpy(), g["region"].numpy()
    o = np.argsort(s, kind="stable")
    lines = []
    g["report"](lambda *a: lines.append(" ".join(str(v) for v in a)), s[o[-10:]][::-1].tolist(), o[-10:][::-1].tolist(),
                int(np.argmax(s)), float(s.max()), r[o[-10:]][::-1].tolist(), float(np.sort(s)[s.size // 2]))
    assert len(out) == 5 and out == lines
    assert [op[0] for op in launches(drv)].count("sort") == 1 and "arg_reduce" in [op[0] for op in launches(drv)]

"""Quantiles and histograms above the kernels, on CPU: ``ops/array.py``
(median / percentile / quantile / histogram), the numpy protocols
(``ops/npinterop.py``) and the offload (``ops/numpy_offload.py``) over the
numpy model of the two kernels (tests/host_driver_stats.py), which records the
launches.  The model sorts, so these tests check the Python layers against
numpy on the same host data: rank arithmetic, interpolation, result types,
edges, fallbacks.  The kernels themselves: tests/test_stats_gpu.py."""

import os
import runpy
import warnings

import numpy as np
import pytest

from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops import npinterop, numpy_offload
from bee_code_interpreter_fs_amd.ops.numpy_offload import OffloadArray

from .host_driver_stats import use_stats_host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = [0, 0.1, 1, 5, 25, 33.3, 50, 75, 95, 99.9, 100]
NS = [1, 2, 3, 17, 255, 4097]


@pytest.fixture
def drv(monkeypatch):
    d = use_stats_host_driver(monkeypatch)
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


@pytest.mark.parametrize("n", NS)
def test_rank_arithmetic_is_numpys_linear_method(drv, n):
    h = np.random.default_rng(n).standard_normal(n)
    x = ops.asarray(h)
    want = np.percentile(h, QS)
    got = ops.percentile(x, QS)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(QS),)
    np.testing.assert_array_equal(got, want)  # (the same lerp, from the same two neighbours)
    np.testing.assert_array_equal(np.percentile(x, QS), want)
    np.testing.assert_array_equal(np.quantile(x, np.array(QS) / 100), np.quantile(h, np.array(QS) / 100))
    for q in QS:
        assert ops.percentile(x, q) == np.percentile(h, q)
        assert ops.quantile(x, q / 100) == np.quantile(h, q / 100)
    assert ops.median(x) == np.median(h) and np.median(x) == np.median(h)


@pytest.mark.parametrize("n", NS)
def test_f32_results_are_the_f64_interpolation_rounded_once(drv, n):
    h = np.random.default_rng(100 + n).standard_normal(n).astype(np.float32)
    x = ops.asarray(h, "float32")
    want = np.percentile(h.astype(np.float64), QS)
    got = np.percentile(x, QS)  # (a list of Python numbers: numpy's result is float64)
    assert got.dtype == np.percentile(h, QS).dtype == np.float64
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ops.percentile(x, QS), want)
    q32 = np.array(QS, np.float32)
    got = np.percentile(x, q32)
    assert got.dtype == np.percentile(h, q32).dtype == np.float32
    np.testing.assert_array_equal(got, np.percentile(h.astype(np.float64), q32.astype(np.float64)).astype(np.float32))
    for q in QS:
        assert np.percentile(x, q) == np.float32(np.percentile(h.astype(np.float64), q))
    assert np.median(x) == np.median(h)  # (numpy's own f32 mean of the middle pair)


def test_result_types(drv):
    h64 = np.linspace(-1.0, 2.0, 101)
    for h, scalar_t in ((h64, np.float64), (h64.astype(np.float32), np.float32)):
        x = ops.asarray(h, h.dtype.name)
        for fn, q in ((np.percentile, 30), (np.quantile, 0.3)):
            s = fn(x, q)
            assert type(s) is scalar_t and type(s) is type(fn(h, q))
            assert type(fn(x, np.float64(q))) is type(fn(h, np.float64(q)))
            assert type(fn(x, np.array(q))) is type(fn(h, np.array(q)))  # 0-D
            assert type(fn(x, np.array(q, h.dtype))) is scalar_t
            a = fn(x, [q, q])
            # (numpy's dtype follows q as well: a list of Python numbers is float64)
            assert isinstance(a, np.ndarray) and a.dtype == fn(h, [q, q]).dtype and a.shape == (2,)
            q_arr = np.array([q], h.dtype)
            assert fn(x, q_arr).shape == (1,) and fn(x, q_arr).dtype == fn(h, q_arr).dtype == h.dtype
        assert type(np.median(x)) is scalar_t
        # beekern's own functions: a sequence gives float64 whatever the array
        assert type(ops.percentile(x, 30)) is scalar_t and ops.percentile(x, [30]).dtype == np.float64
        assert type(ops.quantile(x, 0.3)) is scalar_t and type(ops.median(x)) is scalar_t
    b = ops.asarray(h64, "bfloat16")
    assert type(ops.median(b)) is np.float32 and type(ops.percentile(b, 10)) is np.float32
    assert ops.percentile(b, (10, 20)).dtype == np.float64


def test_errors(drv):
    x = ops.asarray(np.arange(5.0))
    for bad in (-0.1, 100.1, float("nan"), [50, 101]):
        with pytest.raises(ValueError, match="Percentiles must be in the range"):
            ops.percentile(x, bad)
    with pytest.raises(ValueError, match="Quantiles must be in the range"):
        ops.quantile(x, 1.5)
    empty = ops.asarray(np.zeros(0))
    for fn in (ops.median, lambda a: ops.percentile(a, 50), lambda a: ops.quantile(a, 0.5)):
        with pytest.raises(ValueError, match="empty"):
            fn(empty)
    with pytest.raises(TypeError):
        ops.median(x > 2.0)
    with pytest.raises(ValueError, match="4096"):
        ops.histogram(x, bins=4097)
    with pytest.raises(ValueError, match="4096"):
        ops.histogram(x, bins=np.arange(4098.0))
    assert not drv.launches or "select" not in kernels(drv)


def test_nan_propagates(drv):
    h = np.arange(100.0)
    h[37] = np.nan
    x = ops.asarray(h)
    assert np.isnan(np.median(x)) and np.isnan(np.percentile(x, 10)) and np.isnan(np.quantile(x, [0.1, 0.9])).all()
    assert type(np.median(ops.asarray(h.astype(np.float32), "float32"))) is np.float32
    with pytest.raises(ValueError, match="autodetected range"):
        np.histogram(x, bins=5)
    c, e = np.histogram(x, bins=5, range=(0, 100))  # (a NaN counts nowhere)
    wc, we = np.histogram(h, bins=5, range=(0, 100))
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_array_equal(e, we)


def test_transposed_views_and_lazy_draws(drv):
    h = np.random.default_rng(5).standard_normal((37, 53))
    x = ops.asarray(h)
    del drv.launches[:]
    assert np.median(x.T) == np.median(h) and np.percentile(x.T, 12.5) == np.percentile(h, 12.5)
    c, e = np.histogram(x.T, bins=7)
    wc, we = np.histogram(h.T, bins=7)
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_array_equal(e, we)
    assert "transpose" not in kernels(drv) and "select" in kernels(drv) and "histogram" in kernels(drv)
    assert np.median(x) == np.median(h)  # any shape
    # a lazy draw is materialised first, once
    r = ops.random.default_rng(3).random(5000)
    assert r._lazy is not None
    m = ops.median(r)
    assert r._lazy is None and m == np.median(r.numpy())


def test_select_calls_carry_up_to_16_quantiles(drv):
    h = np.random.default_rng(8).standard_normal(1000)
    x = ops.asarray(h)
    del drv.launches[:]
    q16 = list(np.linspace(0, 100, 16))
    np.testing.assert_array_equal(np.percentile(x, q16), np.percentile(h, q16))
    assert kernels(drv) == ["select"]
    assert len(drv.launches[0][2]) == 32
    del drv.launches[:]
    q40 = list(np.linspace(0, 100, 40))
    np.testing.assert_array_equal(np.percentile(x, q40), np.percentile(h, q40))
    assert kernels(drv) == ["select"] * 3
    assert [len(op[2]) for op in drv.launches if op[0] == "select"] == [32, 32, 16]
    del drv.launches[:]
    np.median(x)
    assert kernels(drv) == ["select"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_histogram_edges_and_counts_are_numpys(drv, dtype):
    h = (np.random.default_rng(9).standard_normal(5000) * 3).astype(dtype)
    x = ops.asarray(h, dtype)
    cases = [dict(), dict(bins=1), dict(bins=50), dict(bins=4096), dict(bins=np.int64(7)),
             dict(bins=[-2.0, -0.5, 0.0, 0.25, 4.0]), dict(bins=np.array([-1, 0, 0, 2])), dict(bins=(0.0, 1.0)),
             dict(bins=20, range=(-1.0, 1.0)), dict(bins=5, range=(10.0, 20.0)), dict(bins=3, range=(2, 2)),
             dict(bins=50, density=True), dict(bins=[-3.0, -1.0, 0.0, 5.0], density=True),
             dict(bins=10, range=(-1, 1), density=False)]
    for kw in cases:
        wc, we = np.histogram(h, **kw)
        for c, e in (np.histogram(x, **kw), ops.histogram(x, **kw)):
            assert isinstance(c, np.ndarray) and isinstance(e, np.ndarray)
            assert c.dtype == wc.dtype and e.dtype == we.dtype, kw
            np.testing.assert_array_equal(e, we)
            np.testing.assert_array_equal(c, wc)
    assert np.histogram(x)[0].dtype == np.int64
    assert np.histogram(x)[1].dtype == np.dtype(dtype)
    # positional arguments bind like numpy's
    np.testing.assert_array_equal(np.histogram(x, 12, (-1, 1))[0], np.histogram(h, 12, (-1, 1))[0])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_histogram_of_constant_data(drv, dtype):
    h = np.full(300, 2.5, dtype)
    x = ops.asarray(h, dtype)
    for kw in (dict(bins=10), dict(bins=1), dict(bins=4, range=(2.5, 2.5))):
        wc, we = np.histogram(h, **kw)
        c, e = np.histogram(x, **kw)
        np.testing.assert_array_equal(e, we)
        np.testing.assert_array_equal(c, wc)
        assert e.dtype == we.dtype


def _warns(fn):
    with pytest.warns(npinterop.HostFallbackWarning):
        return fn()


def test_everything_else_still_falls_back(drv, monkeypatch):
    h = np.random.default_rng(11).standard_normal(64)
    x = ops.asarray(h)
    h2 = h.reshape(8, 8)
    x2 = ops.asarray(h2)

    def fresh(fn):
        monkeypatch.setattr(npinterop, "_WARNED", set())
        del drv.launches[:]
        r = _warns(fn)
        assert "select" not in kernels(drv) and "histogram" not in kernels(drv)
        return r

    with pytest.warns(npinterop.HostFallbackWarning, match="sort"):
        np.sort(x)
    # dtypes without the protocol path
    xb = ops.asarray(h, "bfloat16")
    fresh(lambda: np.median(xb))
    fresh(lambda: np.percentile(xb, 50))
    fresh(lambda: np.histogram(xb, bins=4))
    m = x > 0.0
    fresh(lambda: np.median(m))
    fresh(lambda: np.histogram(m, bins=2))
    # arguments without a kernel
    assert fresh(lambda: np.median(x, keepdims=True)).shape == (1,)
    fresh(lambda: np.median(x, out=np.empty(())))
    fresh(lambda: np.median(x, overwrite_input=True))
    fresh(lambda: np.percentile(x, 50, out=np.empty(())))
    fresh(lambda: np.percentile(x, 50, overwrite_input=True))
    assert fresh(lambda: np.percentile(x, 50, keepdims=True)).shape == (1,)
    assert fresh(lambda: np.quantile(x, 0.5, method="nearest")) == np.quantile(h, 0.5, method="nearest")
    fresh(lambda: np.percentile(x, 50, method="lower"))
    fresh(lambda: np.quantile(x, 0.5, method="inverted_cdf", weights=np.ones(64)))
    assert fresh(lambda: np.median(x2, axis=0)).shape == (8,)
    assert fresh(lambda: np.percentile(x2, 50, axis=1)).shape == (8,)
    fresh(lambda: np.quantile(x2, 0.5, axis=(0, 1)))
    fresh(lambda: np.histogram(x, bins="auto"))
    fresh(lambda: np.histogram(x, bins=4, weights=np.ones(64)))
    assert fresh(lambda: np.histogram(x, bins=4097))[0].shape == (4097,)
    assert fresh(lambda: np.histogram(x, bins=np.linspace(-3, 3, 4098)))[0].shape == (4097,)
    # numpy raises its own errors, on the host
    for bad in (lambda: np.percentile(x, 101), lambda: np.quantile(x, [-0.5]), lambda: np.percentile(x, float("nan"))):
        monkeypatch.setattr(npinterop, "_WARNED", set())
        with pytest.warns(npinterop.HostFallbackWarning), pytest.raises(ValueError, match="must be in the range"):
            bad()
    monkeypatch.setattr(npinterop, "_WARNED", set())
    with pytest.warns(npinterop.HostFallbackWarning), pytest.raises(ValueError):
        np.histogram(x, bins=[1.0, 0.0])
    # size-0 arrays: numpy's NaN and warning
    e = ops.asarray(np.zeros(0))
    monkeypatch.setattr(npinterop, "_WARNED", set())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert np.isnan(np.median(e))
    assert any(issubclass(i.category, npinterop.HostFallbackWarning) for i in w)
    assert fresh(lambda: np.histogram(e, bins=3))[0].tolist() == [0, 0, 0]
    # the accepted forms stay on the device
    monkeypatch.setattr(npinterop, "_WARNED", set())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        np.median(x, axis=0), np.median(x, axis=-1, keepdims=False), np.median(x2, axis=None)
        np.percentile(x, 50, method="linear", overwrite_input=False), np.quantile(x, np.float32(0.5), axis=None)
        np.histogram(x, bins=4, range=None, density=None)


def test_offload_arrays_share_the_paths(offload):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = np.random.normal(0.0, 1.0, 5000)
        assert isinstance(r, OffloadArray)
        p = np.percentile(r, [1, 5])
        med = np.median(r)
        c, e = np.histogram(r, bins=50)
        r32 = np.random.default_rng(1).standard_normal(5000, dtype=np.float32)
        assert isinstance(r32, OffloadArray) and np.histogram(r32)[1].dtype == np.float32
        assert type(np.median(r32)) is np.float32
        assert r.on_device and r32.on_device
    h = np.asarray(r)
    np.testing.assert_array_equal(p, np.percentile(h, [1, 5]))
    assert med == np.median(h) and isinstance(p, np.ndarray) and type(med) is np.float64
    np.testing.assert_array_equal(c, np.histogram(h, bins=50)[0])
    np.testing.assert_array_equal(e, np.histogram(h, bins=50)[1])


def test_the_var_example_never_leaves_the_device(offload, capsys):
    with warnings.catch_warnings():
        warnings.simplefilter("error", npinterop.HostFallbackWarning)
        g = runpy.run_path(os.path.join(ROOT, "examples", "monte_carlo_var.py"))
    assert isinstance(g["r"], OffloadArray) and g["r"].on_device
    assert kernels(offload).count("select") == 2 and kernels(offload).count("histogram") == 1
    h = np.asarray(g["r"])
    out = capsys.readouterr().out
    assert f"VaR 1%: {np.percentile(h, 1)}" in out and f"Median: {np.median(h)}" in out
    wc, we = np.histogram(h, bins=50)
    assert f"count {wc.max()}" in out

"""Boolean masks above the kernels, on CPU: ``ops/array.py`` (comparisons,
lazy masks, where, x[mask]), the numpy protocols (``ops/npinterop.py``) and
the offload (``ops/numpy_offload.py``) over the numpy model of the mask
kernels (tests/host_driver_masks.py), which records the launches.  The
kernels themselves: tests/test_masks_gpu.py."""

import warnings

import numpy as np
import pytest

from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops import npinterop, numpy_offload
from bee_code_interpreter_fs_amd.ops.numpy_offload import OffloadArray

from .host_driver import _bf16_bits, _bf16_f32
from .host_driver_masks import use_mask_host_driver

N = 1 << 13
_OPS = {"less": np.less, "less_equal": np.less_equal, "greater": np.greater, "greater_equal": np.greater_equal,
        "equal": np.equal, "not_equal": np.not_equal}


@pytest.fixture
def drv(monkeypatch):
    d = use_mask_host_driver(monkeypatch)
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


def host_values(dtype, seed=0, n=1000):
    """Values with ties and specials, representable in ``dtype``; and the
    ndarray numpy compares (bf16: the f32 values of the rounded bits)."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-3, 4, n).astype(np.float64) / 4
    h[:6] = [np.nan, 0.0, -0.0, np.inf, -np.inf, 0.5]
    if dtype == "bfloat16":
        return _bf16_f32(_bf16_bits(h.astype(np.float32)))
    return h.astype(dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64", "bfloat16"])
@pytest.mark.parametrize("op", sorted(_OPS))
def test_comparisons_match_numpy_in_both_operand_forms(drv, dtype, op):
    ha, hb = host_values(dtype, 1), host_values(dtype, 2)
    a, b = ops.asarray(ha, dtype), ops.asarray(hb, dtype)
    with np.errstate(invalid="ignore"):
        m = getattr(ops, op)(a, b)
        assert m.dtype == "bool" and m.shape == a.shape
        got = m.numpy()
        assert got.dtype == np.bool_
        np.testing.assert_array_equal(got, _OPS[op](ha, hb))
        np.testing.assert_array_equal(getattr(ops, op)(a, 0.5).numpy(), _OPS[op](ha, ha.dtype.type(0.5)))
        # a scalar on the left: the flipped operator
        np.testing.assert_array_equal(getattr(ops, op)(0.25, a).numpy(), _OPS[op](ha.dtype.type(0.25), ha))
        np.testing.assert_array_equal(_OPS[op](a, b).numpy(), _OPS[op](ha, hb))  # the ufunc
        np.testing.assert_array_equal(_OPS[op](0.25, a).numpy(), _OPS[op](ha.dtype.type(0.25), ha))


def test_operators_and_errors(drv):
    h = host_values("float64", 3)
    x = ops.asarray(h)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal((x < 0.25).numpy(), h < 0.25)
        np.testing.assert_array_equal((x <= 0.25).numpy(), h <= 0.25)
        np.testing.assert_array_equal((x > 0.25).numpy(), h > 0.25)
        np.testing.assert_array_equal((x >= 0.25).numpy(), h >= 0.25)
        np.testing.assert_array_equal((0.25 > x).numpy(), 0.25 > h)
    assert (x == x) is True and (x != x) is False  # identity, as before
    with pytest.raises(ValueError):
        ops.less(x, ops.asarray(h[:10]))
    with pytest.raises(ValueError):
        ops.less(x, ops.asarray(h.astype(np.float32)))
    with pytest.raises(TypeError):
        ops.less(x, "a")
    with pytest.raises(TypeError):
        ops.less(x < 0.0, x < 1.0)  # masks are not ordered
    with pytest.raises(TypeError):
        x & x
    with pytest.raises(TypeError):
        ~x
    with pytest.raises(TypeError):
        ops.add(x < 0.0, 1.0)
    with pytest.raises(TypeError):
        x[0]
    with pytest.raises(TypeError):
        x[ops.asarray(h[:10]) < 0.0]


def test_weak_and_strong_scalars_compare_as_numpy_does(drv):
    h = np.array([np.float32(0.1), 0.0, 1.0, np.nextafter(np.float32(0.1), np.float32(1))], np.float32)
    x = ops.asarray(h)
    weak, strong = (x > 0.1).numpy(), (x > np.float64(0.1)).numpy()
    np.testing.assert_array_equal(weak, h > 0.1)  # 0.1 rounds to float32(0.1): not greater
    np.testing.assert_array_equal(strong, h > np.float64(0.1))  # promoted: float32(0.1) > 0.1 in f64
    assert not weak[0] and strong[0]
    np.testing.assert_array_equal(np.greater(x, 0.1).numpy(), weak)
    np.testing.assert_array_equal(np.greater(x, np.float64(0.1)).numpy(), strong)
    np.testing.assert_array_equal(np.less(np.float64(0.1), x).numpy(), strong)
    # bf16: the Python scalar is rounded to bf16 first
    hb = _bf16_f32(_bf16_bits(np.array([0.1, 0.2], np.float32)))
    xb = ops.asarray(hb, "bfloat16")
    np.testing.assert_array_equal((xb >= 0.1).numpy(), [True, True])
    np.testing.assert_array_equal((xb >= np.float64(0.1)).numpy(), hb.astype(np.float64) >= 0.1)
    # past float32's range a Python scalar is +-inf, as numpy's conversion
    np.testing.assert_array_equal((x < 1e60).numpy(), [True] * 4)


def test_counts_of_a_lazy_mask_are_fused(drv):
    rng = np.random.default_rng(5)
    hx, hy = rng.random(N), rng.random(N)
    x, y = ops.asarray(hx), ops.asarray(hy)
    want = hx * hx + hy * hy <= 1.0
    drv.launches.clear()
    inside = x * x + y * y <= 1.0
    assert kernels(drv) == ["unary", "unary", "binary"], drv.launches  # the comparison has not run
    s = np.sum(inside)
    assert isinstance(s, np.int64) and s == want.sum()
    m = np.mean(inside)
    assert isinstance(m, np.float64) and m == want.mean()
    c = np.count_nonzero(inside)
    assert type(c) is int and c == want.sum()
    assert isinstance(np.any(inside), np.bool_) and np.any(inside) and not np.all(inside)
    assert ops.any(inside) is True and ops.all(inside) is False
    assert isinstance(ops.sum(inside), np.int64) and isinstance(ops.mean(inside), np.float64)
    assert type(ops.count_nonzero(inside)) is int
    assert "compare" not in kernels(drv) and kernels(drv).count("compare_count") == 11, drv.launches
    # every other use materialises it, once
    drv.launches.clear()
    np.testing.assert_array_equal((~inside).numpy(), ~want)
    np.testing.assert_array_equal(inside.numpy(), want)
    assert np.sum(inside) == want.sum() and np.any(inside) and not np.all(inside)
    assert kernels(drv).count("compare") == 1 and "compare_count" not in kernels(drv), drv.launches
    assert kernels(drv).count("reduce") == 3
    # of a float array: the fused != 0 count
    drv.launches.clear()
    assert np.count_nonzero(ops.asarray(np.array([0.0, -0.0, 2.0, np.nan]))) == 2
    assert kernels(drv) == ["compare_count"]


def test_mask_reductions_on_materialised_masks(drv):
    for h in (np.zeros(100, bool), np.ones(100, bool), np.arange(100) % 3 == 0, np.zeros(0, bool)):
        m = ops.asarray(h, dtype="bool")
        assert m.dtype == "bool"
        assert ops.sum(m) == h.sum() and ops.count_nonzero(m) == h.sum()
        assert ops.any(m) is bool(h.any()) and ops.all(m) is bool(h.all())
        assert m.any() is bool(h.any()) and m.all() is bool(h.all())
        assert np.max(m) == h.any() if h.size else True
        assert isinstance(np.add.reduce(m), np.int64)
    assert np.isnan(ops.mean(ops.asarray(np.zeros(0, bool), dtype="bool")))


def test_bool_creation_and_astype(drv):
    h = np.arange(50) % 4 == 1
    m = ops.asarray(h, dtype=bool)
    np.testing.assert_array_equal(m.numpy(), h)
    assert ops.asarray(h).dtype == "float64"  # no explicit dtype: converted, as before
    assert ops.normalize_dtype(np.bool_) == "bool" and ops.normalize_dtype("bool") == "bool"
    np.testing.assert_array_equal(ops.zeros(7, "bool").numpy(), np.zeros(7, bool))
    np.testing.assert_array_equal(ops.ones((2, 3), "bool").numpy(), np.ones((2, 3), bool))
    assert ops.empty(5, "bool").nbytes == 5
    for dt in ("float32", "float64"):
        f = m.astype(dt)
        assert f.dtype == dt
        np.testing.assert_array_equal(f.numpy(), h.astype(dt))
    np.testing.assert_array_equal(m.copy().numpy(), h)
    with pytest.raises(TypeError):
        m.astype("bfloat16")
    with pytest.raises(TypeError):
        ops.asarray(np.ones(3)).astype("bool")


def test_mask_logic(drv):
    ha, hb = np.arange(300) % 2 == 0, np.arange(300) % 3 == 0
    a, b = ops.asarray(ha, dtype="bool"), ops.asarray(hb, dtype="bool")
    for got, want in [(a & b, ha & hb), (a | b, ha | hb), (a ^ b, ha ^ hb), (~a, ~ha),
                      (ops.logical_and(a, b), ha & hb), (ops.logical_or(a, b), ha | hb),
                      (ops.logical_xor(a, b), ha ^ hb), (ops.logical_not(b), ~hb),
                      (np.logical_and(a, b), ha & hb), (np.logical_or(a, b), ha | hb),
                      (np.logical_xor(a, b), ha ^ hb), (np.logical_not(a), ~ha),
                      (np.bitwise_and(a, b), ha & hb), (np.bitwise_or(a, b), ha | hb),
                      (np.bitwise_xor(a, b), ha ^ hb), (np.invert(a), ~ha)]:
        assert isinstance(got, ops.DeviceArray) and got.dtype == "bool"
        np.testing.assert_array_equal(got.numpy(), want)
    with pytest.raises(ValueError):
        a & ops.asarray(ha[:5], dtype="bool")


@pytest.mark.parametrize("dtype", ["float32", "float64", "bfloat16"])
def test_where_array_and_scalar_forms(drv, dtype):
    ha, hb = host_values(dtype, 7), host_values(dtype, 8)
    a, b = ops.asarray(ha, dtype), ops.asarray(hb, dtype)
    hm = np.arange(ha.size) % 3 != 0
    m = ops.asarray(hm, dtype="bool")
    bits = np.uint32 if ha.dtype == np.float32 else np.uint64

    def same(got, want):
        assert got.dtype == dtype
        np.testing.assert_array_equal(got.numpy().view(bits), np.asarray(want, ha.dtype).view(bits))

    same(ops.where(m, a, b), np.where(hm, ha, hb))
    same(ops.where(m, a, -0.0), np.where(hm, ha, ha.dtype.type(-0.0)))
    same(ops.where(m, 2.5, b), np.where(hm, ha.dtype.type(2.5), hb))
    same(np.where(m, a, b), np.where(hm, ha, hb))
    same(np.where(m, a, 1.5), np.where(hm, ha, ha.dtype.type(1.5)))
    with pytest.raises(ValueError):
        ops.where(m, a, ops.asarray(hb[:3], dtype))
    with pytest.raises(TypeError):
        ops.where(a, a, b)  # the condition is a mask


def test_where_scalar_scalar_and_dtype_rules(drv):
    hm = np.arange(100) % 2 == 0
    m = ops.asarray(hm, dtype="bool")
    r = ops.where(m, 1.0, 0.25)
    assert r.dtype == "float64"
    np.testing.assert_array_equal(r.numpy(), np.where(hm, 1.0, 0.25))
    r = np.where(m, 2.0, -1.0)
    assert isinstance(r, ops.DeviceArray) and r.dtype == "float64"
    np.testing.assert_array_equal(r.numpy(), np.where(hm, 2.0, -1.0))
    # f32 scalars are rounded once (RNE)
    x = ops.asarray(np.zeros(100, np.float32))
    np.testing.assert_array_equal(ops.where(m, x, 0.1).numpy(), np.where(hm, np.float32(0), np.float32(0.1)))
    with pytest.raises(TypeError):
        ops.where(m, x, ops.asarray(np.zeros(100)))  # mixed float dtypes
    with pytest.raises(TypeError):
        ops.where(m, x, np.float64(0.1))  # would promote
    # numpy's answer for the forms without a kernel, on the host
    with pytest.warns(npinterop.HostFallbackWarning):
        r = np.where(m, 1, 0)
    assert isinstance(r, np.ndarray) and r.dtype.kind == "i"
    (idx,) = np.where(m)
    np.testing.assert_array_equal(idx, np.where(hm)[0])


@pytest.mark.parametrize("dtype", ["float32", "float64", "bfloat16", "bool"])
def test_selection_keeps_order(drv, dtype):
    n = 777
    if dtype == "bool":
        h = np.arange(n) % 5 < 2
        x = ops.asarray(h, dtype="bool")
    else:
        h = host_values(dtype, 9, n)
        h[:6] = np.arange(6)
        x = ops.asarray(h, dtype)
    for hm in (np.arange(n) % 3 == 1, np.zeros(n, bool), np.ones(n, bool)):
        drv.launches.clear()
        got = x[ops.asarray(hm, dtype="bool")]
        assert got.dtype == dtype and got.shape == (int(hm.sum()),)
        np.testing.assert_array_equal(got.numpy(), h[hm])
        if not hm.any():
            assert "compress" not in kernels(drv)  # a zero-length result: nothing to launch
    # a lazy mask: the fused count sizes the result, then the mask is materialised
    if dtype != "bool":
        drv.launches.clear()
        with np.errstate(invalid="ignore"):
            got, want = x[x > 0.0], h[h > 0.0]
        np.testing.assert_array_equal(got.numpy(), want)
        assert kernels(drv) == ["compare_count", "compare", "compress"], drv.launches


def test_selection_of_2d_and_transposed_views(drv):
    h = np.arange(12.0).reshape(3, 4)
    x = ops.asarray(h)
    np.testing.assert_array_equal(x[x > 4.0].numpy(), h[h > 4.0])
    t = x.T
    np.testing.assert_array_equal(t[t > 4.0].numpy(), h.T[h.T > 4.0])  # C order of the view


def test_lazy_mask_is_a_snapshot_of_its_operands(offload):
    x = np.random.rand(N)
    assert isinstance(x, OffloadArray)
    before = np.asarray(ops.asarray(x._dev).numpy()).copy()
    m = x > 0.5
    assert isinstance(m, OffloadArray) and m.on_device and m._dev._lazy is not None
    x += 1.0  # in place, after the comparison
    assert x.on_device
    assert np.sum(m) == (before > 0.5).sum()
    np.testing.assert_array_equal(np.asarray(m), before > 0.5)
    assert np.sum(x > 0.5) == N


def test_offload_masks_stay_on_the_device(offload):
    x, y = np.random.rand(N), np.random.rand(N)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = x < y
        assert isinstance(m, OffloadArray) and m.on_device and m.dtype == np.dtype(bool)
        both = (x < 0.5) & ~(y >= 0.5) | (x > 2.0) ^ (y > 2.0)
        assert both.on_device and both.dtype == np.dtype(bool)
        assert isinstance(m.any(), np.bool_) and m.any() and not m.all()
        f = m.astype(np.float64)
        assert isinstance(f, OffloadArray) and f.on_device and f.dtype == np.float64
        sel = x[m]
        assert isinstance(sel, OffloadArray) and sel.on_device and sel.shape == (int(np.sum(m)),)
        w = np.where(m, x, y)
        assert isinstance(w, OffloadArray) and w.on_device
        assert x.on_device and y.on_device
    hx, hy = np.asarray(x), np.asarray(y)
    np.testing.assert_array_equal(np.asarray(sel), hx[hx < hy])
    np.testing.assert_array_equal(np.asarray(w), np.minimum(hx, hy))
    np.testing.assert_array_equal(np.asarray(both), (hx < 0.5) & ~(hy >= 0.5))
    # a host-resident operand keeps everything on the host
    z = np.random.rand(N)
    z[0] = 0.25  # (moves z to the host for good)
    r = z < x
    assert isinstance(r, np.ndarray) and r.dtype == bool


def test_the_pi_payload_never_leaves_the_device(offload):
    n = N
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x = np.random.rand(n)
        y = np.random.rand(n)
        inside = x**2 + y**2 <= 1.0
        pi = 4 * np.sum(inside) / n
        mean_inside = x[inside].mean()
    assert x.on_device and y.on_device and inside.on_device
    assert "compare_count" in kernels(offload) and "compress" in kernels(offload)
    hx, hy = np.asarray(x), np.asarray(y)
    want = hx**2 + hy**2 <= 1.0
    assert pi == 4 * want.sum() / n
    assert mean_inside == pytest.approx(hx[want].mean(), rel=1e-12)


def test_pinned_fallbacks_still_warn(drv):
    h = np.array([3.0, 1.0, 2.0])
    x = ops.asarray(h)
    with pytest.warns(npinterop.HostFallbackWarning, match="sort"):
        np.sort(x)
    with pytest.warns(npinterop.HostFallbackWarning):
        np.cumsum(x)
    o = OffloadArray(ops.asarray(h))
    with pytest.warns(npinterop.HostFallbackWarning):
        assert o.argmax() == 0
    x32 = ops.asarray(h.astype(np.float32))
    with pytest.warns(npinterop.HostFallbackWarning):
        z = np.multiply(x32, np.float64(2.0))
    assert isinstance(z, np.ndarray) and z.dtype == np.float64
    # the mask forms without a kernel fall back too
    m = x > 1.5
    with pytest.warns(npinterop.HostFallbackWarning):
        assert np.sum(m, dtype=np.float32) == 2.0
    with pytest.warns(npinterop.HostFallbackWarning):
        r = np.less(x, 1.5, out=np.empty(3, bool))
    np.testing.assert_array_equal(r, h < 1.5)

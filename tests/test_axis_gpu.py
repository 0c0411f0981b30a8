"""The broadcast and the axis statistics (csrc/kernels/axis.hip) on the MI355X,
native driver.  Broadcasts are compared bit for bit with beekern's own
equal-shape binary kernel on the expanded vector (the same arithmetic, so
equality is the condition); max / min with numpy exactly; var / std with
``h.astype(float64).var(axis, ddof=ddof)`` on the downloaded operand.  Then
through the service: the plain-numpy example under the offload, and both new
ops once in a broker sandbox.  CPU twins: test_axis_cpu.py,
test_broker_axis_cpu.py.

Tolerances of var / std.  f64: rtol 1e-9 -- f64 accumulation over at most
140000 terms is bounded by n * 2^-53 ~ 1.6e-11, the margin is that of
test_sum_mean_along_axis.  f32: rtol 2.5e-7, about 2 f32 ulp -- the result is
an f64-accurate value rounded once (6e-8), which an f32-rounded mean between
the two passes misses on data near 1000 (up to 4e-3).  A constant line of
value c gives at most 1e-18 c^2."""

import os
import tempfile

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops.array import driver as _driver  # (ops.driver is the submodule)

from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float64", "float32"]
UINT = {"float32": np.uint32, "float64": np.uint64}
# the smallest shapes at which the paths differ: single elements and lines;
# rows far wider / tables far taller than a block's tile; odd columns (rows not
# 16-byte aligned: the one-element paths); 16-byte paths with ragged column
# strips; more than one row chunk of the 16-byte column kernel, the last ragged;
# a tall table narrower than that kernel's strip (fewer column lanes, more row lanes)
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 70000), (70000, 3), (2, 140000), (1000, 300), (257, 1023), (777, 4104),
          (4100, 64), (70000, 8)]
CASES = [(dt, s) for dt in DTYPES for s in SHAPES]
OPS = ["add", "subtract", "multiply", "divide", "maximum", "minimum", "power"]


def bits(a):
    return np.ascontiguousarray(a).view(UINT[a.dtype.name])


def same_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} vs {want.ravel()[bad[:4]]}"


def same_values(got, want, what=""):
    """Against numpy: the same bits, but for NaNs (a GPU and a CPU differ in the
    sign and payload of the NaN an invalid operation makes)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    same_bits(np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(want.dtype), what)


def table(dtype, shape, seed=0, specials=True):
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    h = rng.standard_normal(shape) * 2.0
    if specials and h.size >= 16:  # signed zeros, infinities and a NaN among the operands
        flat = h.reshape(-1)
        flat[rng.choice(h.size, 6, replace=False)] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0]
    return h.astype(dtype)


# ---- broadcast ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,shape", CASES)
def test_broadcast_equals_the_binary_kernel_on_the_expanded_vector(gpu, dtype, shape):
    rows, cols = shape
    h = table(dtype, shape)
    x = gpu.asarray(h, dtype)
    d = _driver()
    for kind, n in ((0, cols), (1, rows)):
        hv = table(dtype, (1, n), seed=1 + kind).reshape(n)
        v = gpu.asarray(hv if kind == 0 else hv.reshape(n, 1), dtype)
        wide = gpu.asarray(np.ascontiguousarray(np.broadcast_to(hv[None, :] if kind == 0 else hv[:, None], shape)), dtype)
        for name in OPS:
            fn = getattr(gpu, name)
            for swapped in (False, True):
                got = fn(v, x) if swapped else fn(x, v)
                want = fn(wide, x) if swapped else fn(x, wide)
                # (two single elements: the scalar shortcut, which keeps its first operand's shape)
                same_bits(got.numpy().reshape(shape) if h.size == 1 else got.numpy(), want.numpy(),
                          f"{name} kind {kind} swapped {swapped}")
                # in place: y is a
                y = x.copy()
                d.broadcast(OPS.index(name), x.code, kind, swapped, y.ptr, v.ptr, y.ptr, rows, cols, cols, cols)
                same_bits(y.numpy(), want.numpy(), f"in place {name} kind {kind} swapped {swapped}")
        same_bits(v.numpy().reshape(n), hv, "the vector")
    same_bits(x.numpy(), h, "the matrix")  # the operands are only read


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,ld", [(257, 1019, 1023), (300, 4096, 4104), (70, 6, 8)])
def test_broadcast_with_row_strides(gpu, dtype, rows, cols, ld):
    """Rows further apart than they are long: the gaps of y keep their bytes."""
    h = table(dtype, (rows, ld))
    x = gpu.asarray(h, dtype)
    d = _driver()
    for kind, n in ((0, cols), (1, rows)):
        hv = table(dtype, (1, n), seed=5, specials=False).reshape(n)
        v = gpu.asarray(hv, dtype)
        y = gpu.full((rows, ld), -7.0, dtype)
        d.broadcast(1, x.code, kind, False, x.ptr, v.ptr, y.ptr, rows, cols, ld, ld)
        want = np.full((rows, ld), -7.0, dtype)
        with np.errstate(all="ignore"):
            want[:, :cols] = h[:, :cols] - (hv[None, :] if kind == 0 else hv[:, None])
        same_values(y.numpy(), want, f"kind {kind}")
        # a contiguous output of a strided matrix
        z = gpu.empty((rows, cols), dtype)
        d.broadcast(3, x.code, kind, True, x.ptr, v.ptr, z.ptr, rows, cols, ld, cols)
        with np.errstate(all="ignore"):
            same_values(z.numpy(), ((hv[None, :] if kind == 0 else hv[:, None]) / h[:, :cols]).astype(dtype), f"kind {kind}")
        # the statistics read the same strided matrix
        out = gpu.empty((cols if kind == 0 else rows,), dtype)
        d.axis_stat(0, x.code, x.ptr, out.ptr, rows, cols, ld, kind, 1.0)
        np.testing.assert_array_equal(out.numpy(), h[:, :cols].max(axis=kind))
        clean = np.nan_to_num(h[:, :cols].astype(np.float64), nan=0.5, posinf=2.0, neginf=-2.0)
        xc = np.zeros((rows, ld), dtype)
        xc[:, :cols] = clean
        dxc = gpu.asarray(xc, dtype)
        d.axis_stat(2, x.code, dxc.ptr, out.ptr, rows, cols, ld, kind, clean.shape[kind] - 1)
        np.testing.assert_allclose(out.numpy(), xc[:, :cols].astype(np.float64).var(axis=kind, ddof=1),
                                   rtol=1e-9 if dtype == "float64" else 2.5e-7, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 1), (3, 70000), (1000, 300), (257, 1023), (4100, 64)])
def test_broadcast_of_a_transposed_view(gpu, dtype, shape):
    h = table(dtype, shape)
    x = gpu.asarray(h, dtype)
    rows, cols = shape
    for hv in (table(dtype, (1, rows), 3).reshape(rows), table(dtype, (1, cols), 4).reshape(cols, 1)):
        if hv.size == 1:
            continue  # (a single element is the scalar form of the plain kernel)
        v = gpu.asarray(hv, dtype)
        with np.errstate(all="ignore"):
            same_values((x.T - v).numpy(), h.T - hv, "x.T - v")  # (IEEE subtraction and division: numpy's bits)
            same_values((v / x.T).numpy(), hv / h.T, "v / x.T")
            same_values(np.subtract(x.T, v).numpy(), h.T - hv, "np.subtract")
    same_bits(x.numpy(), h, "the matrix")


def test_broadcast_refuses_what_it_cannot_run(gpu):
    from bee_code_interpreter_fs_amd.ops import BeekernError

    x, v = gpu.zeros((8, 8)), gpu.zeros((8,))
    d = _driver()
    with pytest.raises(BeekernError):
        d.broadcast(1, x.code, 0, False, x.ptr, x.ptr, x.ptr, 8, 8, 8, 8)  # y overlaps v
    with pytest.raises(BeekernError):
        d.broadcast(1, x.code, 0, False, x.ptr, v.ptr, x.ptr + 8, 7, 7, 8, 8)  # y overlaps a, shifted
    with pytest.raises(BeekernError):
        d.broadcast(7, x.code, 0, False, x.ptr, v.ptr, x.ptr, 8, 8, 8, 8)
    with pytest.raises(BeekernError):
        d.broadcast(1, 2, 0, False, x.ptr, v.ptr, x.ptr, 8, 8, 8, 8)  # bf16
    with pytest.raises(BeekernError):
        d.axis_stat(0, 6, x.ptr, v.ptr, 8, 8, 8, 0, 1.0)  # bool
    with pytest.raises(BeekernError):
        d.axis_stat(2, x.code, x.ptr, v.ptr, 8, 8, 8, 0, 0.0)
    with pytest.raises(BeekernError):
        d.axis_stat(0, x.code, x.ptr, v.ptr, 1, (1 << 18) + 1, (1 << 18) + 1, 0, 1.0)  # wider than the column workspace
    with pytest.raises(ValueError):
        gpu.amax(gpu.zeros((1, (1 << 18) + 1)), axis=0)


# ---- max / min ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,shape", CASES)
def test_max_min_are_numpys(gpu, dtype, shape):
    h = table(dtype, shape, seed=7, specials=False)
    x = gpu.asarray(h, dtype)
    for axis in (0, 1):
        np.testing.assert_array_equal(gpu.amax(x, axis=axis).numpy(), h.max(axis=axis))
        np.testing.assert_array_equal(gpu.amin(x, axis=axis).numpy(), h.min(axis=axis))
        got = np.max(x, axis=axis, keepdims=True)
        assert got.shape == h.max(axis=axis, keepdims=True).shape and got.dtype == dtype
        np.testing.assert_array_equal(np.min(x.T, axis=axis).numpy(), h.T.min(axis=axis))


@pytest.mark.parametrize("dtype,shape", CASES)
def test_a_nan_is_its_lines_max_and_min_only(gpu, dtype, shape):
    rows, cols = shape
    base = table(dtype, shape, seed=8, specials=False)
    for axis in (0, 1):
        n, lines = shape[axis], shape[1 - axis]
        line = lines // 2
        for at in sorted({0, n // 2, n - 1}):
            h = base.copy()
            if axis == 0:
                h[at, line] = np.nan
            else:
                h[line, at] = np.nan
            x = gpu.asarray(h, dtype)
            for fn, ref in ((gpu.amax, np.max), (gpu.amin, np.min)):
                got = fn(x, axis=axis).numpy()
                assert np.isnan(got[line]) and np.isnan(got).sum() == 1, (axis, at, np.flatnonzero(np.isnan(got))[:5])
                np.testing.assert_array_equal(got, ref(h, axis=axis))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 5), (70000, 3), (257, 1023), (777, 4104)])
def test_infinities_are_ordinary_values(gpu, dtype, shape):
    h = table(dtype, shape, seed=9, specials=False)
    rng = np.random.default_rng(10)
    h.reshape(-1)[rng.choice(h.size, min(h.size, 64), replace=False)] = rng.choice([np.inf, -np.inf], min(h.size, 64))
    h[0, :] = -np.inf  # lines of one infinity only, and lines holding both
    h[:, 0] = np.inf
    x = gpu.asarray(h, dtype)
    for axis in (0, 1):
        np.testing.assert_array_equal(gpu.amax(x, axis=axis).numpy(), h.max(axis=axis))
        np.testing.assert_array_equal(gpu.amin(x, axis=axis).numpy(), h.min(axis=axis))


# ---- var / std -----------------------------------------------------------------------------

def spread_data(dtype, shape, offset):
    rng = np.random.default_rng([11, shape[0], shape[1]])
    return (rng.uniform(-1.0, 1.0, shape) + offset).astype(dtype)


@pytest.mark.parametrize("dtype,shape", CASES)
def test_var_std_against_f64_numpy(gpu, dtype, shape):
    rtol = 1e-9 if dtype == "float64" else 2.5e-7
    for offset in ((0.0, 1e6) if dtype == "float64" else (0.0, 1e3)):
        h = spread_data(dtype, shape, offset)
        x = gpu.asarray(h, dtype)
        w = h.astype(np.float64)
        for axis in (0, 1):
            for ddof in (0, 1):
                if shape[axis] - ddof <= 0:
                    with pytest.raises(ValueError):
                        gpu.var(x, axis=axis, ddof=ddof)
                    continue
                var, std = gpu.var(x, axis=axis, ddof=ddof), gpu.std(x, axis=axis, ddof=ddof)
                assert var.dtype == std.dtype == dtype and var.shape == std.shape == (shape[1 - axis],)
                want_var, want_std = w.var(axis=axis, ddof=ddof), w.std(axis=axis, ddof=ddof)
                got_var, got_std = var.numpy().astype(np.float64), std.numpy().astype(np.float64)
                err_var = np.max(np.abs(got_var - want_var) / np.maximum(np.abs(want_var), 1e-300), initial=0.0)
                err_std = np.max(np.abs(got_std - want_std) / np.maximum(np.abs(want_std), 1e-300), initial=0.0)
                print(f"{dtype} {shape} offset {offset} axis {axis} ddof {ddof}: var {err_var:.3g} std {err_std:.3g}")
                np.testing.assert_allclose(got_var, want_var, rtol=rtol, atol=0)
                np.testing.assert_allclose(got_std, want_std, rtol=rtol, atol=0)
                # the same bits twice, and through a .T view and the protocols
                same_bits(gpu.var(x, axis=axis, ddof=ddof).numpy(), var.numpy(), "var, again")
                same_bits(gpu.std(x, axis=axis, ddof=ddof).numpy(), std.numpy(), "std, again")
            same_bits(np.var(x.T, axis=1 - axis).numpy(), gpu.var(x, axis=axis).numpy(), "x.T")
            kept = np.std(x, axis=axis, ddof=0.5, keepdims=True)
            assert kept.shape == w.std(axis=axis, keepdims=True).shape
            np.testing.assert_allclose(kept.numpy().astype(np.float64), w.std(axis=axis, ddof=0.5, keepdims=True),
                                       rtol=rtol, atol=0)


@pytest.mark.parametrize("dtype,shape", CASES)
def test_constant_lines_have_no_variance(gpu, dtype, shape):
    for c in ((0.1, 1e6 + 0.1) if dtype == "float64" else (0.1, 1000.1)):
        c = float(np.dtype(dtype).type(c))
        x = gpu.full(shape, c, dtype)
        for axis in (0, 1):
            assert float(np.max(gpu.var(x, axis=axis).numpy())) <= 1e-18 * c * c
            assert float(np.max(gpu.std(x, axis=axis).numpy())) <= 1e-9 * c


# ---- through the service ---------------------------------------------------------------

@pytest.fixture(scope="module")
def asvc():
    ensure_native_executor()
    h = ServiceHarness(tempfile.mkdtemp(prefix="bee-axis-"), gpu_ids=[0], workers_per_gpu_target=1,
                       default_timeout=120.0)
    h.start()
    yield h
    h.stop()


def test_standardize_softmax_under_the_offload(asvc):
    """Plain numpy, Execute(numpy_offload=True): every line of the example runs
    on the sandbox's GPU (no HostFallbackWarning)."""
    src = open(os.path.join(ROOT, "examples", "standardize_softmax.py")).read()
    r = asvc.call(asvc.ctx.code_executor.execute(source_code=src, numpy_offload=True, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert "HostFallbackWarning" not in r.stderr, r.stderr

    def numbers(label, count):
        return [float(t) for t in r.stdout.split(label)[1].split()[:count]]

    assert abs(numbers("Largest |column mean|:", 1)[0]) < 1e-9, r.stdout
    assert all(abs(v - 1.0) < 1e-9 for v in numbers("Column std range:", 2)), r.stdout
    assert all(abs(v - 1.0) < 1e-12 for v in numbers("Softmax row sums:", 2)), r.stdout
    assert all(abs(v - 1.0) < 1e-9 for v in numbers("Correlation diagonal:", 2)), r.stdout


def test_broadcast_and_axis_stat_in_a_broker_sandbox(asvc):
    code = (
        "import beekern as bk, numpy as np\n"
        "h = np.random.default_rng(5).standard_normal((1025, 33)) + 3.0\n"
        "x = bk.asarray(h)\n"
        "assert bk.driver_name() == 'broker'\n"
        "c, r = bk.asarray(h.mean(axis=0)), bk.asarray(h.max(axis=1, keepdims=True))\n"
        "assert ((x - c).numpy() == h - h.mean(axis=0)).all()                        # BROADCAST\n"
        "assert ((r / x).numpy() == h.max(axis=1, keepdims=True) / h).all()\n"
        "assert ((x.T * c.reshape(33, 1)).numpy() == h.T * h.mean(axis=0).reshape(33, 1)).all()\n"
        "for axis in (0, 1):                                                        # AXIS_STAT\n"
        "    assert (bk.amax(x, axis=axis).numpy() == h.max(axis=axis)).all()\n"
        "    assert (np.min(x, axis=axis, keepdims=True).numpy() == h.min(axis=axis, keepdims=True)).all()\n"
        "    np.testing.assert_allclose(bk.var(x, axis=axis, ddof=1).numpy(), h.var(axis=axis, ddof=1), rtol=1e-9)\n"
        "    np.testing.assert_allclose(np.std(x, axis=axis).numpy(), h.std(axis=axis), rtol=1e-9)\n"
        "h32 = h.astype(np.float32)\n"
        "x32 = bk.asarray(h32, 'float32')\n"
        "assert (bk.amin(x32, axis=0).numpy() == h32.min(axis=0)).all()\n"
        "np.testing.assert_allclose(bk.std(x32, axis=1).numpy(), h32.astype(np.float64).std(axis=1), rtol=2.5e-7)\n"
        "print('axis ok', bk.driver_name())\n"
    )
    r = asvc.call(asvc.ctx.code_executor.execute(source_code=code, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert r.stdout.split() == ["axis", "ok", "broker"], r.stdout

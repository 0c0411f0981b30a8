"""The host model of the elementwise kernels (tests/host_driver.py) against
numpy in the kernels' compute type.

bk_binary converts a scalar operand once to its compute type (f32 for f32 and
bf16 arrays) and works there -- numpy 2's rule for a Python scalar against an
f32 array.  The model computes in f64 and rounds, which gives the same bits
only if it rounds the scalar to f32 first: ``x + 0.1`` differs in 4.7 % of
standard-normal f32 values otherwise.  tests/test_elementwise_gpu.py holds the
kernels to the same reference, so the two sides cannot drift apart.
"""

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops.array import _BINARY, _UNARY, _f32_to_bf16_bits

from .host_driver import HostDriver

F32, F64, BF16 = 0, 1, 2
SCALARS = [0.1, 1 / 3, 3.0, -0.0, 1e39]
_NP_BINARY = {"add": np.add, "subtract": np.subtract, "multiply": np.multiply, "divide": np.divide,
              "maximum": np.maximum, "minimum": np.minimum, "power": np.power}


def _specials_f32() -> np.ndarray:
    fi = np.finfo(np.float32)
    one = np.float32(1)
    mags = [0.0, np.inf, 1.0, fi.smallest_subnormal, fi.smallest_normal - fi.smallest_subnormal, fi.smallest_normal,
            fi.max, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 0.5, 2.0, 3.0]
    return np.array([s * m for m in mags for s in (1, -1)] + [np.nan], np.float32)


def _inputs(dt: int) -> np.ndarray:
    """10^5 standard-normal values plus the specials, as the array's stored bits."""
    x = np.concatenate([np.random.default_rng(7).standard_normal(100_000).astype(np.float32), _specials_f32()])
    return _f32_to_bf16_bits(x) if dt == BF16 else x


def _as_f32(stored: np.ndarray, dt: int) -> np.ndarray:
    return (stored.astype(np.uint32) << 16).view(np.float32) if dt == BF16 else stored


def _run_binary(op: int, dt: int, mode: int, stored: np.ndarray, sc: float) -> np.ndarray:
    drv = HostDriver()
    a, y = drv.malloc(stored.nbytes), drv.malloc(stored.nbytes)
    drv.h2d(a, stored)
    drv.binary(op, dt, mode, a, 0, sc, y, stored.size)
    out = np.empty_like(stored)
    drv.d2h(y, out)
    return out


def _run_unary(op: int, dt: int, stored: np.ndarray) -> np.ndarray:
    drv = HostDriver()
    x, y = drv.malloc(stored.nbytes), drv.malloc(stored.nbytes)
    drv.h2d(x, stored)
    drv.unary(op, dt, x, y, stored.size)
    out = np.empty_like(stored)
    drv.d2h(y, out)
    return out


def _assert_same_bits(got: np.ndarray, ref_f32: np.ndarray, dt: int, what: str) -> None:
    """Bit for bit; where the reference is NaN only NaN is required."""
    ref = _f32_to_bf16_bits(ref_f32) if dt == BF16 else ref_f32
    nan = np.isnan(ref_f32)
    assert np.isnan(_as_f32(got, dt)[nan]).all(), what
    uint = np.uint16 if dt == BF16 else np.uint32
    bad = np.flatnonzero((got.view(uint) != ref.view(uint)) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}"


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(_BINARY))
def test_scalar_operand_is_rounded_to_the_compute_type(name, mode, dt):
    stored = _inputs(dt)
    x = _as_f32(stored, dt)
    for s in SCALARS:
        with np.errstate(all="ignore"):
            s32 = np.float32(s)
            ref = _NP_BINARY[name](x, s32) if mode == 1 else _NP_BINARY[name](s32, x)
        assert ref.dtype == np.float32
        _assert_same_bits(_run_binary(_BINARY[name], dt, mode, stored, s), ref, dt, f"{name} mode {mode} scalar {s!r}")


def test_add_point_one_differs_from_the_f64_scalar():
    """The case the model got wrong: adding the double 0.1 and rounding is not
    adding float32(0.1)."""
    x = _inputs(F32)[:100_000]
    wrong = (x.astype(np.float64) + 0.1).astype(np.float32)
    right = x + np.float32(0.1)
    assert (wrong != right).mean() > 0.01
    np.testing.assert_array_equal(_run_binary(_BINARY["add"], F32, 1, x, 0.1), right)


def test_f64_scalar_is_used_as_given():
    x = np.random.default_rng(8).standard_normal(4099)
    np.testing.assert_array_equal(_run_binary(_BINARY["add"], F64, 1, x, 0.1), x + 0.1)
    np.testing.assert_array_equal(_run_binary(_BINARY["subtract"], F64, 2, x, 1 / 3), 1 / 3 - x)


@pytest.mark.parametrize("dt", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
def test_abs_and_relu_contract(dt):
    """abs clears the sign bit (abs(-0.0) is +0.0); relu is maximum(x, 0): NaN
    stays NaN, both zeros and every negative give +0.0."""
    vals = np.array([-0.0, 0.0, -1.5, 1.5, -np.inf, np.inf, np.nan, -np.nan], np.float64 if dt == F64 else np.float32)
    stored = _f32_to_bf16_bits(vals) if dt == BF16 else vals
    sign = {F32: 31, F64: 63, BF16: 15}[dt]
    uint = {F32: np.uint32, F64: np.uint64, BF16: np.uint16}[dt]

    def value(a):
        return _as_f32(a, dt).astype(np.float64)

    got = _run_unary(_UNARY["abs"], dt, stored)
    assert ((got.view(uint) >> sign)[:6] == 0).all(), "abs leaves a sign bit"
    np.testing.assert_array_equal(value(got)[:6], [0.0, 0.0, 1.5, 1.5, np.inf, np.inf])
    assert np.isnan(value(got)[6:]).all()

    got = _run_unary(_UNARY["relu"], dt, stored)
    assert ((got.view(uint) >> sign)[:6] == 0).all(), "relu returns a negative zero"
    np.testing.assert_array_equal(value(got)[:6], [0.0, 0.0, 0.0, 1.5, 0.0, np.inf])
    assert np.isnan(value(got)[6:]).all(), "relu(NaN) must stay NaN"

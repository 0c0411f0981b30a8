"""bk_unary / bk_binary / bk_cast / bk_fill (csrc/kernels/elementwise.hip) and
bk_rand_normal against numpy, at the values, lengths and paths where such
kernels go wrong.

Run on an MI355X: ``python -m pytest tests/test_elementwise_gpu.py -m gpu``.

The kernels are called through the driver on buffers the test owns: every
output buffer is longer than the n elements asked for and pre-filled with a
sentinel, and every test asserts that the bytes past element n are untouched.
Pointers are used as the allocator returns them (the kernels assume 16-byte
alignment).

The reference is numpy in the kernel's *compute* type on the same input bits:
f64 for f64, f32 for f32 and bf16; a bf16 result is the f32 result rounded once
(``_f32_to_bf16_bits``); a scalar operand is ``np.float32(s)`` for f32 / bf16.

* square abs negative sqrt relu copy, add subtract multiply divide: bit for bit,
  sign of zero and denormals included; where the reference is NaN only NaN is
  required (payload and sign are the hardware's).  relu's contract: +0.0 for
  both zeros and every negative, NaN for NaN.
* maximum minimum: bit for bit, a zero result compared as a value (numpy's
  choice between +0.0 and -0.0 is not specified); NaN in either operand: NaN.
* exp log sin cos tanh sigmoid power: inf / NaN / zero references must match
  exactly (the zero's sign for power and tanh); elsewhere f64 and f32 hold
  ``|got - ref| <= 4 tol |ref| + m`` with the project's tol (1e-12 / 2e-6) and
  m the smallest normal of the compute type (what 1 / (1 + exp(-x)) loses
  below the normal range), sin and cos of large arguments (|x| >= 1e4, where
  the result's scale is 1 and its relative error is the argument reduction's)
  ``4 tol`` absolute;
  bf16 is within one bf16 ulp of the rounded reference -- the kernel rounds an
  f32 result a few f32 ulps off, so it can only land on the other side of a tie.

Each inexact case prints its worst error in ulps of the dtype (``ULP ...``
lines, ``pytest -s``); the figures are recorded, the tolerance is asserted.
"""

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops.array import _BINARY, _UNARY, _f32_to_bf16_bits

from .philox_ref import normal_f32, normal_f64

pytestmark = pytest.mark.gpu

F32, F64, BF16, BOOL = 0, 1, 2, 6
DTYPES = {"float64": F64, "float32": F32, "bfloat16": BF16}
STORE = {F32: np.float32, F64: np.float64, BF16: np.uint16}
COMPUTE = {F32: np.float32, F64: np.float64, BF16: np.float32}
UINT = {F32: np.uint32, F64: np.uint64, BF16: np.uint16}
TOL = {F64: 1e-12, F32: 2e-6}
PAD = 256  # sentinel bytes kept after every output
K_BAD_ARGUMENT = 1

EXACT_UNARY = ("square", "abs", "negative", "sqrt", "relu", "copy")
EXACT_BINARY = ("add", "subtract", "multiply", "divide")
_PERIOD = ((np.arange(251) * 151 + 89) & 0xFF).astype(np.uint8)  # (a prime period: no element size divides it)


def _sentinel(nbytes: int) -> np.ndarray:
    return np.resize(_PERIOD, nbytes)


class _Device:
    """Device buffers of one test, freed when it ends."""

    def __init__(self, drv) -> None:
        self.drv = drv
        self.ptrs: list = []

    def put(self, host: np.ndarray) -> int:
        p = self.drv.malloc(host.nbytes)
        self.ptrs.append(p)
        self.drv.h2d(p, np.ascontiguousarray(host))
        return p

    def run(self, n: int, store, launch) -> np.ndarray:
        """The n elements ``launch(y)`` wrote to a sentinel-filled buffer,
        after checking that nothing past them changed."""
        nbytes = n * np.dtype(store).itemsize
        before = _sentinel(nbytes + PAD)
        y = self.put(before)
        launch(y)
        after = np.empty_like(before)
        self.drv.d2h(y, after)
        assert np.array_equal(after[nbytes:], before[nbytes:]), f"bytes past element {n} were written"
        return after[:nbytes].view(store)

    def free(self) -> None:
        for p in self.ptrs:
            self.drv.free(p)
        self.ptrs = []


@pytest.fixture
def dev(gpu):
    from bee_code_interpreter_fs_amd.ops.array import driver

    d = _Device(driver())
    yield d
    d.drv.sync()
    d.free()


# ---- values -----------------------------------------------------------------------------------------

def _to_store(x: np.ndarray, dt: int) -> np.ndarray:
    return _f32_to_bf16_bits(x) if dt == BF16 else np.ascontiguousarray(x, STORE[dt])


def _values(stored: np.ndarray, dt: int) -> np.ndarray:
    """Stored elements in the compute type."""
    return (stored.astype(np.uint32) << 16).view(np.float32) if dt == BF16 else stored


def _representable(x, dt: int) -> np.ndarray:
    with np.errstate(all="ignore"):
        x = np.asarray(x, np.float64).astype(COMPUTE[dt])
    return _values(_f32_to_bf16_bits(x), dt) if dt == BF16 else x


def _specials(dt: int) -> np.ndarray:
    """+-0, +-inf, NaN, +-1 and its neighbours, the ends of the subnormal and
    normal ranges of the dtype, and the arguments that push each function to
    its limits; the most telling ones first (the scalar tail holds few)."""
    ct = COMPUTE[dt]
    if dt == BF16:
        bits = np.array([0x0001, 0x007F, 0x0080, 0x7F7F, 0x3F7F, 0x3F81], np.uint32) << 16
        mags = [float(v) for v in bits.view(np.float32)]
    else:
        fi, one = np.finfo(ct), ct(1)
        mags = [float(v) for v in (fi.smallest_subnormal, fi.smallest_normal - fi.smallest_subnormal,
                                   fi.smallest_normal, fi.max, np.nextafter(one, ct(0)), np.nextafter(one, ct(2)))]
    overflow = float(np.log(np.float64(np.finfo(ct).max)))  # exp's threshold in the compute type
    mags += [overflow - 1, overflow + 1, 20.0, 100.0, 1000.0, 1e-5, 1e6, 1e-8, 0.5, 2.0, 3.0]
    if dt == F64:
        mags.append(1e22)
    vals = [-0.0, np.nan, -np.inf, np.inf, -1.0, 0.0, 1.0] + [s * m for m in mags for s in (1.0, -1.0)]
    return _representable(vals, dt)


def _vec(dt: int) -> int:
    return 16 // np.dtype(STORE[dt]).itemsize


def _all_loops_length(dt: int) -> int:
    """Two full chunks of 4 x 256 vectors, five leftover vectors, a scalar tail."""
    N = _vec(dt)
    return 2 * 1024 * N + 5 * N + (N - 1)


def _place(base: np.ndarray, special: np.ndarray, dt: int) -> np.ndarray:
    """``special`` in each of the kernels' three loops: the first chunk, the
    leftover vectors and the scalar tail (as many as each holds)."""
    N = _vec(dt)
    x = base.copy()
    first = min(special.size, 1024 * N)
    x[:first] = special[:first]
    mid = min(special.size, 5 * N)
    x[2 * 1024 * N: 2 * 1024 * N + mid] = special[:mid]
    tail = min(special.size, N - 1)
    x[x.size - tail:] = special[:tail]
    return x


def _random(dt: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return _representable(rng.standard_normal(n) * rng.choice([1e-3, 1.0, 10.0], n), dt)


# ---- references and comparisons ---------------------------------------------------------------------

def _unary_ref(name: str, x: np.ndarray) -> np.ndarray:
    ct = x.dtype.type
    with np.errstate(all="ignore"):
        if name == "relu":  # the contract: NaN stays NaN, zeros and negatives give +0.0
            return np.where(np.isnan(x), x, np.where(x > 0, x, ct(0)))
        if name == "sigmoid":
            return ct(1) / (ct(1) + np.exp(-x))
        if name == "copy":
            return x.copy()
        return {"square": np.square, "abs": np.abs, "negative": np.negative, "sqrt": np.sqrt, "exp": np.exp,
                "log": np.log, "sin": np.sin, "cos": np.cos, "tanh": np.tanh}[name](x)


_NP_BINARY = {"add": np.add, "subtract": np.subtract, "multiply": np.multiply, "divide": np.divide,
              "maximum": np.maximum, "minimum": np.minimum, "power": np.power}


def _binary_ref(name: str, a, b) -> np.ndarray:
    with np.errstate(all="ignore"):
        return _NP_BINARY[name](a, b)


def _scalar(s: float, dt: int):
    """The kernel converts a scalar operand once to its compute type."""
    with np.errstate(over="ignore"):
        return np.float64(s) if dt == F64 else np.float32(s)


def _report(what: str, bad: np.ndarray, got, ref, x=None) -> str:
    i = np.flatnonzero(bad)[:6]
    rows = [f"[{k}] got {got[k]!r} ref {ref[k]!r}" + (f" x {x[k]!r}" if x is not None else "") for k in i]
    return f"{what}: {int(bad.sum())} of {bad.size} differ: " + "; ".join(rows)


def _check_exact(what: str, got: np.ndarray, ref: np.ndarray, dt: int, zero_by_value: bool = False) -> None:
    assert ref.dtype == COMPUTE[dt] and got.shape == ref.shape, what
    g = _values(got, dt)
    want = _to_store(ref, dt)
    nan = np.isnan(ref)
    assert np.isnan(g[nan]).all(), f"{what}: a NaN result came out as a number"
    same = got.view(UINT[dt]) == want.view(UINT[dt])
    if zero_by_value:
        w = _values(want, dt)
        same |= (w == 0) & (g == 0)
    bad = ~same & ~nan
    assert not bad.any(), _report(what, bad, g, _values(want, dt))


def _ordered(bits: np.ndarray) -> np.ndarray:
    """bf16 bit patterns as integers in value order (+-0 both 0, inf next to the largest finite)."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def _check_inexact(what: str, got: np.ndarray, ref: np.ndarray, dt: int, x=None, signed_zero: bool = False,
                   large_abs: bool = False, ref_hi=None) -> None:
    """The rules of the module docstring for exp log sin cos tanh sigmoid power;
    prints the worst error in ulps of the dtype before asserting."""
    assert ref.dtype == COMPUTE[dt] and got.shape == ref.shape, what
    g = _values(got, dt)
    nan, inf, zero = np.isnan(ref), np.isinf(ref), ref == 0
    rest = ~(nan | inf | zero)
    if dt == BF16:
        dist = np.abs(_ordered(got) - _ordered(_f32_to_bf16_bits(ref)))
        worst = int(dist[rest].max()) if rest.any() else 0
        ok = dist <= 1
    else:
        g64, r64 = g.astype(np.float64), ref.astype(np.float64)
        with np.errstate(all="ignore"):
            err = np.abs(g64 - r64)
            bound = 4 * TOL[dt] * np.abs(r64) + float(np.finfo(COMPUTE[dt]).smallest_normal)
            if large_abs:
                bound = np.where(np.abs(x) >= 1e4, 4 * TOL[dt], bound)
            ulps = err / np.spacing(np.abs(ref)).astype(np.float64)
        worst = float(np.nanmax(ulps[rest])) if rest.any() else 0.0
        ok = err <= bound  # (a NaN where a number belongs compares false)
    line = f"ULP {what} max_ulp_vs_reference={worst:.4g}"
    if ref_hi is not None and rest.any():
        # the same figure against the function evaluated in f64 and rounded once: numpy's f32 routines are
        # themselves a few ulps off
        if dt == BF16:
            hi = np.abs(_ordered(got) - _ordered(_f32_to_bf16_bits(ref_hi)))[rest].max()
        else:
            with np.errstate(all="ignore"):
                ulps_hi = (np.abs(g.astype(np.float64) - ref_hi.astype(np.float64))
                           / np.spacing(np.abs(ref_hi)).astype(np.float64))
                hi = np.nanmax(ulps_hi[rest & np.isfinite(ref_hi) & (ref_hi != 0)])
        line += f" max_ulp_vs_f64_rounded={float(hi):.4g}"
    print(line)
    assert np.isnan(g[nan]).all(), f"{what}: a NaN result came out as a number"
    bad = inf & (g != ref)
    assert not bad.any(), _report(what + " (infinite reference)", bad, g, ref, x)
    bad = zero & (g != 0)
    assert not bad.any(), _report(what + " (zero reference)", bad, g, ref, x)
    if signed_zero:
        bad = zero & (np.signbit(g) != np.signbit(ref))
        assert not bad.any(), _report(what + " (sign of zero)", bad, g, ref, x)
    bad = rest & ~ok
    assert not bad.any(), _report(what, bad, g, ref, x)


def _check(name: str, what: str, got, ref, dt: int, x=None, ref_hi=None) -> None:
    if name in EXACT_UNARY or name in EXACT_BINARY:
        _check_exact(what, got, ref, dt)
    elif name in ("maximum", "minimum"):
        _check_exact(what, got, ref, dt, zero_by_value=True)
    else:
        _check_inexact(what, got, ref, dt, x=x, signed_zero=name in ("power", "tanh"),
                       large_abs=name in ("sin", "cos"), ref_hi=ref_hi)


def _unary_ref_hi(name: str, x: np.ndarray):
    """f32 / bf16 only: the function in f64, rounded once to f32."""
    if x.dtype == np.float64 or name in EXACT_UNARY:
        return None
    with np.errstate(all="ignore"):
        return _unary_ref(name, x.astype(np.float64)).astype(np.float32)


# ---- unary ------------------------------------------------------------------------------------------

def _unary_input(dt: int) -> np.ndarray:
    n = _all_loops_length(dt)
    return _place(_random(dt, n, 100 + dt), _specials(dt), dt)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(_UNARY))
def test_unary_every_op_special_values_every_loop(dev, name, dtype):
    dt = DTYPES[dtype]
    x = _unary_input(dt)
    n = x.size
    xp = dev.put(_to_store(x, dt))
    got = dev.run(n, STORE[dt], lambda y: dev.drv.unary(_UNARY[name], dt, xp, y, n))
    _check(name, f"unary {name} {dtype}", got, _unary_ref(name, x), dt, x=x, ref_hi=_unary_ref_hi(name, x))


@pytest.mark.parametrize("name", list(_UNARY))
def test_unary_every_bf16_bit_pattern(dev, name):
    stored = np.arange(1 << 16, dtype=np.uint16)
    x = _values(stored, BF16)
    xp = dev.put(stored)
    got = dev.run(stored.size, np.uint16, lambda y: dev.drv.unary(_UNARY[name], BF16, xp, y, stored.size))
    _check(name, f"unary {name} every-bf16", got, _unary_ref(name, x), BF16, x=x, ref_hi=_unary_ref_hi(name, x))


# ---- binary -----------------------------------------------------------------------------------------

_POWER_PAIRS = [(np.nan, 0.0), (1.0, np.nan), (-8.0, 1 / 3), (-2.0, 3.0), (0.0, -1.0), (-0.0, -1.0), (-0.0, 3.0),
                (2.0, 1024.0), (np.inf, -1.0)]


def _binary_inputs(dt: int):
    """Operand pairs: power's edge pairs first, then every special against the
    specials rotated by 0, 3, 6, ... places."""
    sp = _specials(dt)
    rolls = range(0, sp.size, 3)
    pa = np.concatenate([_representable([p[0] for p in _POWER_PAIRS], dt)] + [sp for _ in rolls])
    pb = np.concatenate([_representable([p[1] for p in _POWER_PAIRS], dt)] + [np.roll(sp, r) for r in rolls])
    n = _all_loops_length(dt)
    return _place(_random(dt, n, 200 + dt), pa, dt), _place(_random(dt, n, 300 + dt), pb, dt)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(_BINARY))
def test_binary_every_op_and_mode_special_values_every_loop(dev, name, mode, dtype):
    dt = DTYPES[dtype]
    a, b = _binary_inputs(dt)
    n = a.size
    ap = dev.put(_to_store(a, dt))
    if mode == 0:
        bp = dev.put(_to_store(b, dt))
        got = dev.run(n, STORE[dt], lambda y: dev.drv.binary(_BINARY[name], dt, 0, ap, bp, 0.0, y, n))
        _check(name, f"binary {name} mode 0 {dtype}", got, _binary_ref(name, a, b), dt)
        return
    for s in (0.1, -3.0):
        got = dev.run(n, STORE[dt], lambda y: dev.drv.binary(_BINARY[name], dt, mode, ap, 0, s, y, n))
        sc = _scalar(s, dt)
        ref = _binary_ref(name, a, sc) if mode == 1 else _binary_ref(name, sc, a)
        _check(name, f"binary {name} mode {mode} scalar {s} {dtype}", got, ref, dt, x=a)


@pytest.mark.parametrize("name", ["multiply", "add"])
def test_binary_every_bf16_bit_pattern_against_itself_reversed(dev, name):
    sa = np.arange(1 << 16, dtype=np.uint16)
    sb = sa[::-1].copy()
    ap, bp = dev.put(sa), dev.put(sb)
    got = dev.run(sa.size, np.uint16, lambda y: dev.drv.binary(_BINARY[name], BF16, 0, ap, bp, 0.0, y, sa.size))
    _check_exact(f"binary {name} every-bf16", got, _binary_ref(name, _values(sa, BF16), _values(sb, BF16)), BF16)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_denormals_are_kept(dev, dtype):
    """smallest_normal * 0.5 and largest_subnormal + smallest_subnormal, bit
    for bit: a flush-to-zero build returns 0 for the first and loses the second."""
    dt = DTYPES[dtype]
    ct = COMPUTE[dt]
    fi = np.finfo(ct)
    N = _vec(dt)
    n = 1024 * N + N + 1  # a chunk, a vector and a scalar element
    a = np.full(n, fi.smallest_normal, ct)
    ap = dev.put(a)
    got = dev.run(n, ct, lambda y: dev.drv.binary(_BINARY["multiply"], dt, 1, ap, 0, 0.5, y, n))
    ref = a * ct(0.5)
    assert (ref > 0).all() and (ref < fi.smallest_normal).all()
    _check_exact(f"smallest normal * 0.5 {dtype}", got, ref, dt)
    big, small = np.full(n, fi.smallest_normal - fi.smallest_subnormal, ct), np.full(n, fi.smallest_subnormal, ct)
    bp, sp = dev.put(big), dev.put(small)
    got = dev.run(n, ct, lambda y: dev.drv.binary(_BINARY["add"], dt, 0, bp, sp, 0.0, y, n))
    assert ((big + small) == fi.smallest_normal).all()
    _check_exact(f"largest subnormal + smallest subnormal {dtype}", got, big + small, dt)
    got = dev.run(n, ct, lambda y: dev.drv.unary(_UNARY["negative"], dt, sp, y, n))
    _check_exact(f"-smallest subnormal {dtype}", got, -small, dt)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_lengths_around_one_vector_and_one_chunk(dev, dtype):
    dt = DTYPES[dtype]
    N = _vec(dt)
    for n in sorted({1, N - 1, N, N + 1, 1024 * N - 1, 1024 * N, 1024 * N + 1}):
        a, b = _random(dt, n, n), _random(dt, n, n + 1)
        ap, bp = dev.put(_to_store(a, dt)), dev.put(_to_store(b, dt))
        got = dev.run(n, STORE[dt], lambda y: dev.drv.unary(_UNARY["negative"], dt, ap, y, n))
        _check_exact(f"negative {dtype} n={n}", got, -a, dt)
        got = dev.run(n, STORE[dt], lambda y: dev.drv.binary(_BINARY["divide"], dt, 0, ap, bp, 0.0, y, n))
        _check_exact(f"divide {dtype} n={n}", got, _binary_ref("divide", a, b), dt)


# ---- the grid-stride loops and the non-temporal variants --------------------------------------------

def _one_block_per_cu(dev, monkeypatch) -> None:
    """A 256-block grid: the library reads the cap from the environment on
    every launch (stream_grid, bk_common.hpp)."""
    if dev.drv.name != "native":
        pytest.skip("the grid cap is read by the process that launches: the native driver only")
    monkeypatch.setenv("BK_STREAM_BLOCKS_PER_CU", "1")


def test_blocks_go_round_the_chunk_loop_again(dev, monkeypatch):
    """513 chunks on 256 blocks: the first block takes three chunks, the rest two."""
    _one_block_per_cu(dev, monkeypatch)
    n = 2 * (513 * 1024) + 3
    a = np.arange(n, dtype=np.float64) * 0.5 - 1000.0
    b = (np.arange(n) % 1021).astype(np.float64) + 0.25
    ap, bp = dev.put(a), dev.put(b)
    got = dev.run(n, np.float64, lambda y: dev.drv.unary(_UNARY["negative"], F64, ap, y, n))
    _check_exact("negative f64, 3 chunks a block", got, -a, F64)
    got = dev.run(n, np.float64, lambda y: dev.drv.binary(_BINARY["add"], F64, 0, ap, bp, 0.0, y, n))
    _check_exact("add f64, 3 chunks a block", got, a + b, F64)


def test_cast_lanes_stride_the_grid(dev, monkeypatch):
    """200 003 elements on 65 536 lanes: every lane takes three or four."""
    _one_block_per_cu(dev, monkeypatch)
    n = 200_003
    x = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    xp = dev.put(x)
    got = dev.run(n, np.uint16, lambda y: dev.drv.cast(F32, BF16, xp, y, n))
    np.testing.assert_array_equal(got, _f32_to_bf16_bits(x))


@pytest.mark.parametrize("name", ["negative", "add"])
def test_non_temporal_variants(dev, name):
    """268.5 MB an array: past the 256 MiB at which the kernels switch to
    non-temporal loads and stores, and past the 16 384-block grid cap."""
    n = (1 << 25) + 2051
    a = np.arange(n, dtype=np.float64) * 0.5 - 1e6
    ap = dev.put(a)
    if name == "negative":
        got = dev.run(n, np.float64, lambda y: dev.drv.unary(_UNARY["negative"], F64, ap, y, n))
        ref = -a
    else:
        b = (np.arange(n) % 1021).astype(np.float64) + 0.25
        bp = dev.put(b)
        got = dev.run(n, np.float64, lambda y: dev.drv.binary(_BINARY["add"], F64, 0, ap, bp, 0.0, y, n))
        ref = a + b
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


# ---- casts ------------------------------------------------------------------------------------------

def _cast(dev, src: int, dst: int, stored: np.ndarray, store_out) -> np.ndarray:
    xp = dev.put(stored)
    return dev.run(stored.size, store_out, lambda y: dev.drv.cast(src, dst, xp, y, stored.size))


def _assert_bits(got: np.ndarray, want: np.ndarray, nan: np.ndarray, got_nan: np.ndarray, what: str) -> None:
    assert got_nan[nan].all(), f"{what}: a NaN came out as a number"
    bad = (got != want) & ~nan
    assert not bad.any(), _report(what, bad, got, want)


def test_cast_f32_to_bf16_every_tie_and_neighbour(dev):
    """Every upper half with the lower half at 0, just above it, just below
    the tie, the tie and just above the tie: round to nearest even, the top
    finite value's overflow to inf, denormals, NaNs."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    bits = np.concatenate([hi | lo for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001)]).astype(np.uint32)
    x = bits.view(np.float32)
    got = _cast(dev, F32, BF16, x, np.uint16)
    _assert_bits(got, _f32_to_bf16_bits(x), np.isnan(x), np.isnan(_values(got, BF16)), "f32 -> bf16")


def _f64_cast_inputs() -> np.ndarray:
    rng = np.random.default_rng(9)
    sp = _specials(F64)
    named = [1e39, -1e39, 1e-40, -1e-40, 1e-46, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 3 * 2.0 ** -24,
             1 + 2.0 ** -8 + 2.0 ** -40, float(np.finfo(np.float32).max) * (1 + 2.0 ** -25), 3.3895313892515355e38]
    f32_specials = _specials(F32).astype(np.float64)
    # f64 values a hair off an f32 -> bf16 tie: through f32 they land on the tie, directly they do not
    upper = rng.integers(0x0080, 0x7F00, 4000).astype(np.uint32)
    tie = ((upper << 16) | 0x8000).view(np.float32).astype(np.float64)
    near_tie = tie * (1 + rng.choice([-1.0, 1.0], tie.size) * 2.0 ** -40) * rng.choice([-1.0, 1.0], tie.size)
    spread = rng.standard_normal(4000) * 10.0 ** rng.integers(-45, 39, 4000)
    return np.concatenate([sp, named, f32_specials, near_tie, spread])


def test_cast_f64_to_f32(dev):
    x = _f64_cast_inputs()
    with np.errstate(all="ignore"):
        want = x.astype(np.float32)
    assert np.isinf(want[x == 1e39]).all() and (want[x == 1e-40] > 0).all()
    got = _cast(dev, F64, F32, x, np.float32)
    _assert_bits(got.view(np.uint32), want.view(np.uint32), np.isnan(x), np.isnan(got), "f64 -> f32")


def test_cast_f64_to_bf16_rounds_through_f32(dev):
    """astype(f32) then bf16, not one direct rounding: 1 + 2^-8 + 2^-40 is
    0x3F80 through f32 (a tie, to even) and 0x3F81 directly."""
    x = _f64_cast_inputs()
    with np.errstate(all="ignore"):
        want = _f32_to_bf16_bits(x.astype(np.float32))
    assert want[x == 1 + 2.0 ** -8 + 2.0 ** -40].tolist() == [0x3F80]
    got = _cast(dev, F64, BF16, x, np.uint16)
    _assert_bits(got, want, np.isnan(x), np.isnan(_values(got, BF16)), "f64 -> bf16")


def test_casts_that_widen_are_exact(dev):
    x32 = np.concatenate([_specials(F32), np.random.default_rng(10).standard_normal(4099).astype(np.float32)])
    got = _cast(dev, F32, F64, x32, np.float64)
    wide = x32.astype(np.float64)
    _assert_bits(got.view(np.uint64), wide.view(np.uint64), np.isnan(x32), np.isnan(got), "f32 -> f64")
    every = np.arange(1 << 16, dtype=np.uint16)
    v = _values(every, BF16)
    got = _cast(dev, BF16, F32, every, np.float32)
    _assert_bits(got.view(np.uint32), v.view(np.uint32), np.isnan(v), np.isnan(got), "bf16 -> f32")
    got = _cast(dev, BF16, F64, every, np.float64)
    with np.errstate(invalid="ignore"):  # (signalling NaN patterns)
        wide = v.astype(np.float64)
    _assert_bits(got.view(np.uint64), wide.view(np.uint64), np.isnan(v), np.isnan(got), "bf16 -> f64")


@pytest.mark.parametrize("dst", ["float32", "float64"])
def test_cast_bool_any_nonzero_byte_is_one(dev, dst):
    for n in (1, 15, 16, 17, 4099):
        x = np.resize(np.array([2, 0, 0x80, 1, 0xFF, 0, 0], np.uint8), n)
        got = _cast(dev, BOOL, DTYPES[dst], x, STORE[DTYPES[dst]])
        np.testing.assert_array_equal(got, (x != 0).astype(got.dtype), err_msg=f"bool -> {dst} n={n}")


def test_bad_arguments_are_refused_before_any_launch(dev):
    """Unsupported pairs, ops, modes and widths and null pointers return
    kBadArgument (the entry points check them on the host) and write nothing."""
    from bee_code_interpreter_fs_amd.ops import _native

    if dev.drv.name != "native":
        pytest.skip("raw entry points: the native driver only")
    lib, stream = _native.lib(), dev.drv.stream
    src = dev.put(np.ones(64, np.float64))
    before = _sentinel(1024)
    dst = dev.put(before)
    F16, I32 = 3, 4
    for s, d in [(F32, F32), (F64, F64), (BF16, BF16), (BOOL, BF16), (BOOL, BOOL), (F32, BOOL), (F16, F32), (F32, F16),
                 (I32, F32), (F64, 7), (-1, F32)]:
        assert lib.bk_cast(s, d, src, dst, 16, stream) == K_BAD_ARGUMENT, (s, d)
    assert lib.bk_cast(F32, F64, None, dst, 16, stream) == K_BAD_ARGUMENT
    assert lib.bk_cast(F32, F64, src, None, 16, stream) == K_BAD_ARGUMENT
    assert lib.bk_cast(F32, F64, src, dst, -1, stream) == K_BAD_ARGUMENT
    for op, d in [(-1, F32), (len(_UNARY), F32), (0, BOOL), (0, F16)]:
        assert lib.bk_unary(op, d, src, dst, 16, stream) == K_BAD_ARGUMENT, (op, d)
    assert lib.bk_unary(0, F32, None, dst, 16, stream) == K_BAD_ARGUMENT
    for op, d, mode in [(len(_BINARY), F32, 0), (0, BOOL, 0), (0, F32, 3), (0, F32, -1)]:
        assert lib.bk_binary(op, d, mode, src, src, 0.0, dst, 16, stream) == K_BAD_ARGUMENT, (op, d, mode)
    assert lib.bk_binary(0, F32, 0, src, None, 0.0, dst, 16, stream) == K_BAD_ARGUMENT
    for width in (0, 3, 16):
        assert lib.bk_fill(dst, 64, 0x0102030405060708, width, stream) == K_BAD_ARGUMENT, width
    assert lib.bk_fill(None, 64, 0, 4, stream) == K_BAD_ARGUMENT
    after = np.empty_like(before)
    dev.drv.d2h(dst, after)
    np.testing.assert_array_equal(after, before)


# ---- fill -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_fill_every_width_byte_for_byte(dev, width):
    pattern = 0x0807060504030201 & ((1 << (8 * width)) - 1)
    unit = np.frombuffer(pattern.to_bytes(width, "little"), np.uint8)
    per = 16 // width
    for count in sorted({1, per - 1, per, per + 1, 4099} - {0}):
        nbytes = count * width
        got = dev.run(nbytes, np.uint8, lambda y: dev.drv.fill(y, nbytes, pattern, width))
        np.testing.assert_array_equal(got, np.resize(unit, nbytes), err_msg=f"width {width}, {count} elements")


def test_full(gpu):
    n = 4099
    assert (gpu.full(n, 0.1, "float64").numpy() == 0.1).all()
    assert (gpu.full(n, 0.1, "float32").numpy() == np.float32(0.1)).all()
    rounded = _values(_f32_to_bf16_bits(np.array([0.1], np.float32)), BF16)[0]
    assert rounded != np.float32(0.1)
    assert (gpu.full(n, 0.1, "bfloat16").numpy() == rounded).all()
    t, f = gpu.full(n, True, "bool").numpy(), gpu.full(n, False, "bool").numpy()
    assert t.shape == f.shape == (n,) and t.all() and not f.any()


# ---- normal draws -----------------------------------------------------------------------------------

_SEED = 0x5EED_0F_B0C5_11
_MAX_F32_NORMAL_ERR = [0.0]


def _normal_bound(dtype: str, mean: float, std: float) -> float:
    # f64: the project's f64 tolerance at the scale of the result.  f32: structural -- the kernel's fast log and
    # sincos are within it, another draw is not (two independent normals come this close 0.06 % of the time)
    return 4e-12 * (abs(mean) + 8 * std) if dtype == "float64" else 1e-3 * std


def _assert_normal(got: np.ndarray, ref: np.ndarray, dtype: str, mean: float, std: float, what: str) -> None:
    assert got.shape == ref.shape and got.dtype == np.dtype(dtype), what
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.nanmax(err)) if err.size else 0.0
    if dtype == "float32":
        _MAX_F32_NORMAL_ERR[0] = max(_MAX_F32_NORMAL_ERR[0], worst / std)
        print(f"NORMAL_F32 {what} max_err_over_std={worst / std:.4g} (so far {_MAX_F32_NORMAL_ERR[0]:.4g})")
    else:
        print(f"NORMAL_F64 {what} max_err_over_bound={worst / _normal_bound(dtype, mean, std):.4g}")
    bad = ~(err <= _normal_bound(dtype, mean, std))
    assert not bad.any(), _report(what, bad, got, ref)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (2.0, 3.0)])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099, 1 << 20])
def test_normal_draws_match_host_box_muller(gpu, n, mean, std, dtype):
    """Element by element against the host reference of the same Philox
    words, and a second draw continues at the counter after the first."""
    ref_fn, per = (normal_f64, 2) if dtype == "float64" else (normal_f32, 4)
    g = gpu.random.default_rng(_SEED)
    first = g.normal(mean, std, n, dtype=dtype).numpy()
    second = g.normal(mean, std, n, dtype=dtype).numpy()
    _assert_normal(first, ref_fn(n, _SEED, 0, mean, std), dtype, mean, std, f"normal {dtype} n={n}")
    _assert_normal(second, ref_fn(n, _SEED, (n + per - 1) // per, mean, std), dtype, mean, std,
                   f"normal {dtype} n={n}, second draw")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_normal_draws_in_two_parts_equal_one_draw(gpu, dtype):
    g = gpu.random.default_rng(_SEED)
    a, b = g.normal(0.0, 1.0, 1000, dtype=dtype).numpy(), g.normal(0.0, 1.0, 1000, dtype=dtype).numpy()
    assert not np.array_equal(a, b)
    whole = gpu.random.default_rng(_SEED).normal(0.0, 1.0, 2000, dtype=dtype).numpy()
    np.testing.assert_array_equal(np.concatenate([a, b]), whole)


@pytest.mark.parametrize("n", [5, 4099])
def test_bf16_normal_draw_is_the_f32_draw_rounded(gpu, n):
    f32 = gpu.random.default_rng(_SEED).normal(2.0, 3.0, n, dtype="float32").numpy()
    bf16 = gpu.random.default_rng(_SEED).normal(2.0, 3.0, n, dtype="bfloat16").numpy()
    np.testing.assert_array_equal(bf16, _values(_f32_to_bf16_bits(f32), BF16))

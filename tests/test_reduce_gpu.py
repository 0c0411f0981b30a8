"""bk_reduce, bk_rand_reduce and bk_reduce_axis (csrc/kernels/reduce.hip) against
host references, at the values, lengths and layouts where such kernels go wrong.

Run on an MI355X: ``python -m pytest tests/test_reduce_gpu.py -m gpu -s``.

Buffers are allocated through the driver and freed when the test ends; the
kernels are called through ``driver().reduce`` / ``rand_reduce`` / ``reduce_axis``
or, where a status code is the point, through the ``_native`` entry points.
Lengths, grids and bounds come from tests/reduce_inputs.py, which derives them
from the kernels' loops; tests/test_reduce_cpu.py checks those premises without a
GPU.

* **Exact sums.**  The input is small integers (``exact_ints``), exactly
  representable in bf16, f32 and f64; sums of x, x^2, |x| and a.b stay far below
  2^53, so every partial sum of every order is exact and the assertion is ``==``
  against the host's integer sum.  One dropped, repeated or misconverted element
  changes the result.  The same holds for max / min / max_abs_diff with one
  planted extreme, and for the axis sums; an axis mean is the exact sum times
  1 / n in f64, rounded once to the output type, in the kernel and in the reference.
* **Rounded data** (normals, Philox streams, squares of bf16 values): the
  reference is ``math.fsum`` of the widened terms and the bound is
  ``D * 2^-53 * sum |terms|``, D the longest chain of f64 additions a term can pass
  through: all the elements of a lane (ceil(nvec / stride) vectors and one tail
  element), the 15 merges of the 16 accumulators, 6 + 6 cross-lane steps in the
  block, 8 chained partials a trip of the fold and 6 + 6 steps again
  (``reduce_inputs.depth``).  On the default 512-block grid at the all-loops
  length that is 23 N + 48: 94 for f64, 140 for f32, 232 for bf16.  Where the
  terms are products of f64 values D is one more: the kernel may fuse the
  multiplication into the addition, the reference rounds it.  D is never fitted
  to what the kernel returns.  Each such case prints ``RED ... err/bound=`` under
  ``pytest -s``; the figure is recorded, the bound is asserted.
* **Edge values** are compared with numpy in f64 on the widened input: NaN where
  numpy gives NaN, the same infinity, and ``==`` for finite results (the cases
  are built so that numpy's result does not depend on the order either).
* Every output buffer of the axis kernels ends in a sentinel that must stay
  untouched, and their inputs are padded to ``ld > cols`` with NaN that must not
  show in any result.
"""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops.array import _REDUCE, _f32_to_bf16_bits

from . import reduce_inputs as R
from .philox_ref import uniform_f32, uniform_f64
from .reduce_inputs import ABS_SUM, BF16, DOT, DTYPES, F32, F64, MAX, MAX_ABS_DIFF, MIN, SQUARE_SUM, STORE, SUM, U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"sum": SUM, "square_sum": SQUARE_SUM, "abs_sum": ABS_SUM, "max": MAX, "min": MIN, "dot": DOT,
       "max_abs_diff": MAX_ABS_DIFF}
assert OPS == _REDUCE  # the codes of ops/array.py
SUMS = ("sum", "square_sum", "abs_sum", "dot")
PAD = 256  # sentinel bytes kept after every output
K_OK, K_BAD_ARGUMENT = 0, 1
WS_REDUCE_AXIS = 1  # enum BkWorkspace
MAX_AXIS0_COLUMNS = 1 << 18  # BK_MAX_AXIS0_COLUMNS
_SEED = 0x5EED_0F_B0C5_11
_PERIOD = ((np.arange(251) * 151 + 89) & 0xFF).astype(np.uint8)


class _Device:
    """Device buffers of one test, freed when it ends."""

    def __init__(self, drv) -> None:
        self.drv = drv
        self.ptrs: list = []

    def alloc(self, nbytes: int) -> int:
        p = self.drv.malloc(nbytes)
        self.ptrs.append(p)
        return p

    def put(self, host: np.ndarray) -> int:
        p = self.alloc(host.nbytes)
        self.drv.h2d(p, np.ascontiguousarray(host))
        return p

    def poke(self, p: int, dt: int, index: int, value) -> None:
        """One element of a stored array."""
        self.drv.h2d(p, _store(np.array([value], np.float64), dt), offset=index * np.dtype(STORE[dt]).itemsize)

    def reduce(self, op: str, dt: int, a: int, b: int, n: int) -> float:
        return self.drv.reduce(OPS[op], dt, a, b, n)

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


def _store(x: np.ndarray, dt: int) -> np.ndarray:
    """f64 values in the storage type, rounded to nearest even."""
    with np.errstate(over="ignore"):
        x32 = x.astype(np.float32)
    return x if dt == F64 else x32 if dt == F32 else _f32_to_bf16_bits(x32)


def _same(got: float, ref: float) -> bool:
    return (math.isnan(got) and math.isnan(ref)) or got == ref


@functools.lru_cache(maxsize=4)
def _exact(n: int):
    """(a, b, their exact sums) as int64 arrays that nobody writes to."""
    a, b = R.exact_ints(n, 0), R.exact_ints(n, 1)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, R.exact_sums(a, b)


def _positions(dt: int) -> dict:
    """One element in each region of reduce_1pass at the all-loops length on the default grid
    (stride S = 131072 vectors: vectors [0, 16 S) go through the 16-in-flight loop, [16 S, 20 S) through
    the 4-in-flight loop, [20 S, nvec) one at a time, then the tail)."""
    N, S = R.vec(dt), R.RED_BLOCKS * R.RED_BLOCK
    n = R.all_loops_length(N)
    nvec = n // N
    return {"first vector": N - 1, "16 in flight": (7 * S + 12345) * N + 1, "4 in flight": (17 * S + 777) * N,
            "one at a time": (22 * S + 3) * N + N - 1, "scalar tail": nvec * N, "last element": n - 1}


# ---- exact sums ---------------------------------------------------------------------------------------

def _check_exact_sums(dev, gpu, dt: int, dtype: str, n: int) -> None:
    a, b, want = _exact(n)
    pa, pb = dev.put(R.to_store(a, dt)), dev.put(R.to_store(b, dt))
    for op in SUMS:
        got = dev.reduce(op, dt, pa, pb if op == "dot" else 0, n)
        assert got == want[OPS[op]], f"{op} {dtype} n={n}: got {got!r}, exactly {want[OPS[op]]}"
    x = gpu.asarray(a.astype(np.float64), dtype)
    got = float(gpu.sum(gpu.square(x)))  # the fused route of ops.sum
    assert got == want[SQUARE_SUM], f"sum(square(x)) {dtype} n={n}: got {got!r}, exactly {want[SQUARE_SUM]}"
    dev.drv.sync()
    dev.free()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_exact_sums_around_one_vector_and_one_block(dev, gpu, dtype):
    dt = DTYPES[dtype]
    N = R.vec(dt)
    for n in sorted({1, N - 1, N, N + 1, 256 * N - 1, 256 * N, 256 * N + 1}):
        _check_exact_sums(dev, gpu, dt, dtype, n)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_exact_sums_every_loop_of_the_default_grid(dev, gpu, dtype):
    dt = DTYPES[dtype]
    _check_exact_sums(dev, gpu, dt, dtype, R.all_loops_length(R.vec(dt)))


def test_exact_dot_past_the_non_temporal_switch(dev):
    """Two f64 operands of 128 MiB and 16 KiB each: together past the 256 MiB at which launch_reduce
    takes the non-temporal kernels."""
    n = (1 << 24) + 2051
    assert 2 * n * 8 >= R.NT_BYTES > n * 8
    a, b, want = _exact(n)
    pa, pb = dev.put(R.to_store(a, F64)), dev.put(R.to_store(b, F64))
    got = dev.reduce("dot", F64, pa, pb, n)
    assert got == want[DOT], f"dot: got {got!r}, exactly {want[DOT]}"
    got = dev.reduce("max_abs_diff", F64, pa, pb, n)
    assert got == int(np.abs(a - b).max())
    got = dev.reduce("sum", F64, pa, 0, n)  # one operand: still below the switch
    assert got == want[SUM]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_planted_extreme_is_found_in_every_loop(dev, dtype):
    """max, min and max_abs_diff find one extreme element wherever it sits."""
    dt = DTYPES[dtype]
    n = R.all_loops_length(R.vec(dt))
    a, b, _ = _exact(n)
    pa, pb = dev.put(R.to_store(a, dt)), dev.put(R.to_store(b, dt))
    assert dev.reduce("max", dt, pa, 0, n) == 128 and dev.reduce("min", dt, pa, 0, n) == -128
    assert dev.reduce("max_abs_diff", dt, pa, pb, n) == int(np.abs(a - b).max()) <= 253
    for where, k in _positions(dt).items():
        dev.poke(pa, dt, k, 300.0)
        assert dev.reduce("max", dt, pa, 0, n) == 300.0, f"max {dtype}, extreme in the {where}"
        dev.poke(pb, dt, k, -300.0)
        assert dev.reduce("max_abs_diff", dt, pa, pb, n) == 600.0, f"max_abs_diff {dtype}, extreme in the {where}"
        dev.poke(pa, dt, k, -300.0)
        assert dev.reduce("min", dt, pa, 0, n) == -300.0, f"min {dtype}, extreme in the {where}"
        dev.poke(pa, dt, k, float(a[k]))
        dev.poke(pb, dt, k, float(b[k]))
    assert dev.reduce("max", dt, pa, 0, n) == 128 and dev.reduce("min", dt, pa, 0, n) == -128


# ---- rounded data -------------------------------------------------------------------------------------

def _terms(op: str, wa: np.ndarray, wb) -> np.ndarray:
    return {"sum": lambda: wa, "square_sum": lambda: wa * wa, "fused": lambda: wa * wa, "abs_sum": lambda: np.abs(wa),
            "dot": lambda: wa * wb}[op]()


def _check_bound(what: str, got: float, terms: np.ndarray, D: int) -> None:
    ref = R.fsum(terms)
    bound = D * U * float(np.abs(terms).sum())
    err = abs(got - ref)
    print(f"RED {what} D={D} err/bound={err / bound if bound else 0.0:.4g}")
    assert err <= bound, f"{what}: got {got!r}, fsum {ref!r}, error {err:.3g} > bound {bound:.3g}"


@functools.lru_cache(maxsize=1)
def _normals(dt: int, scale: float):
    n = R.all_loops_length(R.vec(dt))
    rng = np.random.default_rng(1000 * dt + int(scale * 1000))
    sa, sb = _store(rng.standard_normal(n) * scale, dt), _store(rng.standard_normal(n) * scale, dt)
    return n, sa, sb, R.widen(sa, dt), R.widen(sb, dt)


@pytest.mark.parametrize("dtype,scale,op", [(d, s, o) for d in DTYPES for s in (1e-3, 1.0, 10.0)
                                            for o in SUMS + ("fused",)])
def test_rounded_sums_stay_within_the_derived_bound(dev, gpu, dtype, scale, op):
    dt = DTYPES[dtype]
    n, sa, sb, wa, wb = _normals(dt, scale)
    D = R.depth(n, R.vec(dt), R.RED_BLOCKS) + (1 if dt == F64 and op in ("square_sum", "fused", "dot") else 0)
    if op == "fused":
        got = float(gpu.sum(gpu.square(gpu.asarray(wa, dtype))))
    else:
        pa = dev.put(sa)
        got = dev.reduce(op, dt, pa, dev.put(sb) if op == "dot" else 0, n)
    _check_bound(f"normals {dtype} x{scale:g} {op} n={n}", got, _terms(op, wa, wb), D)


# ---- edge values --------------------------------------------------------------------------------------

def _numpy_all_ops(wa: np.ndarray, wb: np.ndarray) -> dict:
    with np.errstate(all="ignore"):
        return {"sum": float(wa.sum()), "square_sum": float((wa * wa).sum()), "abs_sum": float(np.abs(wa).sum()),
                "max": float(wa.max()), "min": float(wa.min()), "dot": float((wa * wb).sum()),
                "max_abs_diff": float(np.abs(wa - wb).max())}


_NO_PRODUCTS = ("sum", "square_sum", "abs_sum", "max", "min")


def _edge_cases(dt: int) -> list:
    """(name, [(operand, place, value)], ops).  Every reference is order-independent: an infinity or a NaN
    decides the result alone, and a huge finite value absorbs the small integers around it exactly."""
    inf, nan = np.inf, np.nan
    long_, tail = "16 in flight", "scalar tail"
    cases = []
    for p, q in ((long_, tail), (tail, long_)):
        cases += [(f"+inf in the {p}", [("a", p, inf)], tuple(OPS)),
                  (f"+inf in the {p}, -inf in the {q}", [("a", p, inf), ("a", q, -inf)], tuple(OPS)),
                  (f"NaN in the {p}", [("a", p, nan)], tuple(OPS)),
                  (f"NaN in the second operand, {p}", [("b", p, nan)], ("dot", "max_abs_diff"))]
        if dt == F64:
            big = float(np.finfo(np.float64).max)
            cases.append((f"f64 max in the {p} and the {q}", [("a", p, big), ("a", q, big)], _NO_PRODUCTS))
        else:
            cases.append((f"3e38 in the {p}", [("a", p, 3e38)], tuple(OPS)))
    return cases


_EDGE = [(dtype, name) for dtype in DTYPES for name, _, _ in _edge_cases(DTYPES[dtype])]


@pytest.mark.parametrize("dtype,case", _EDGE)
def test_edge_values_in_a_long_loop_vector_and_in_the_tail(dev, dtype, case):
    dt = DTYPES[dtype]
    n = R.all_loops_length(R.vec(dt))
    a, b, _ = _exact(n)
    host = {"a": a.astype(np.float64), "b": b.astype(np.float64)}
    ptr = {"a": dev.put(R.to_store(a, dt)), "b": dev.put(R.to_store(b, dt))}
    pos = _positions(dt)
    (pokes, ops), = [(p, o) for name, p, o in _edge_cases(dt) if name == case]
    for operand, place, value in pokes:
        k = pos[place]
        stored = _store(np.array([value], np.float64), dt)
        host[operand][k] = R.widen(stored, dt)[0]
        dev.drv.h2d(ptr[operand], stored, offset=k * stored.itemsize)
    ref = _numpy_all_ops(host["a"], host["b"])
    if case.startswith("3e38"):
        v = host["a"][pos[pokes[0][1]]]
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(v) * np.float32(v)) and ref["square_sum"] == v * v < np.inf
    for op in ops:
        got = dev.reduce(op, dt, ptr["a"], ptr["b"] if op in ("dot", "max_abs_diff") else 0, n)
        assert _same(got, ref[op]), f"{dtype}, {case}: {op} gave {got!r}, numpy {ref[op]!r}"


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_subnormal_inputs_are_summed_not_flushed(dev, dtype):
    dt = DTYPES[dtype]
    tiny = {F64: 2.0 ** -1074, F32: 2.0 ** -149, BF16: 2.0 ** -133}[dt]  # the smallest subnormal of the dtype
    stored = _store(np.full(1000, tiny), dt)
    assert (R.widen(stored, dt) == tiny).all() and tiny > 0
    p = dev.put(stored)
    assert dev.reduce("sum", dt, p, 0, 1000) == 1000 * tiny  # (exact: a multiple of the f64 subnormal unit)
    assert dev.reduce("abs_sum", dt, p, 0, 1000) == 1000 * tiny
    assert dev.reduce("max", dt, p, 0, 1000) == tiny == dev.reduce("min", dt, p, 0, 1000)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_zeros_of_both_signs_and_an_all_minus_inf_array(dev, dtype):
    dt = DTYPES[dtype]
    n = 1024 * R.vec(dt) + R.vec(dt) - 1  # whole vectors and a tail
    zeros = _store(np.where(R.exact_ints(n) & 1, 0.0, -0.0), dt)
    assert np.signbit(R.widen(zeros, dt)).any() and not np.signbit(R.widen(zeros, dt)).all()
    p = dev.put(zeros)
    for op in ("max", "min", "sum", "abs_sum", "square_sum"):
        assert dev.reduce(op, dt, p, 0, n) == 0.0, op  # (by value: the sign of a zero result is not specified)
    p = dev.put(_store(np.full(n, -np.inf), dt))
    assert dev.reduce("max", dt, p, 0, n) == -np.inf == dev.reduce("min", dt, p, 0, n)
    assert dev.reduce("abs_sum", dt, p, 0, n) == np.inf == dev.reduce("square_sum", dt, p, 0, n)


def test_bf16_conversion_every_pattern_of_twenty_binades(dev):
    stored = R.bf16_binades()
    x = R.widen(stored, BF16)
    n = stored.size
    p = dev.put(stored)
    assert dev.reduce("sum", BF16, p, 0, n) == 0.0 == float(x.sum())
    assert dev.reduce("abs_sum", BF16, p, 0, n) == float(np.abs(x).sum())
    assert dev.reduce("max", BF16, p, 0, n) == x.max() and dev.reduce("min", BF16, p, 0, n) == x.min()
    _check_bound("bf16 binades square_sum n=5120", dev.reduce("square_sum", BF16, p, 0, n), x * x,
                 R.depth(n, 8, R.grid_blocks(n, 8)))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_empty_input_gives_the_identity_and_leaves_the_workspace_usable(dev, dtype):
    """n = 0 on valid pointers: kOk, the op's identity in *out, and the next reduction on the same
    workspace is right (the ticket was re-armed)."""
    from bee_code_interpreter_fs_amd.ops import _native

    if dev.drv.name != "native":
        pytest.skip("raw entry points: the native driver only")
    import ctypes

    vp = ctypes.c_void_p
    dt = DTYPES[dtype]
    lib, stream, ws = _native.lib(), dev.drv.stream, dev.drv.workspaces[0]
    n = 256 * R.vec(dt) + 1
    a, b, want = _exact(n)
    pa, pb = dev.put(R.to_store(a, dt)), dev.put(R.to_store(b, dt))
    out = dev.put(np.array([123.0]))
    identity = {"sum": 0.0, "square_sum": 0.0, "abs_sum": 0.0, "dot": 0.0, "max": -np.inf, "min": np.inf,
                "max_abs_diff": 0.0}
    got = np.empty(1)
    for op, ident in identity.items():
        dev.drv.h2d(out, np.array([123.0]))
        assert lib.bk_reduce(OPS[op], dt, vp(pa), vp(pb), 0, vp(ws), vp(out), stream) == K_OK, op
        dev.drv.d2h(out, got)
        assert got[0] == ident, f"{op} of nothing: {got[0]!r}"
        assert lib.bk_reduce(OPS["dot"], dt, vp(pa), vp(pb), n, vp(ws), vp(out), stream) == K_OK
        dev.drv.d2h(out, got)
        assert got[0] == want[DOT], f"dot after an empty {op}: {got[0]!r}"
    assert lib.bk_reduce(OPS["sum"], dt, vp(pa), None, -1, vp(ws), vp(out), stream) == K_BAD_ARGUMENT


# ---- fused draws --------------------------------------------------------------------------------------

_STREAM = {"float64": (uniform_f64, 2), "float32": (uniform_f32, 4)}


def _check_rand_reduce(dev, dtype: str, n: int, offset: int, lo: float, hi: float) -> None:
    fn, per = _STREAM[dtype]
    x = fn(n, _SEED, offset, lo, hi).astype(np.float64)
    assert x.size == n
    blocks = R.rand_blocks(n, per)
    for op in ("sum", "square_sum"):
        got = dev.drv.rand_reduce(OPS[op], DTYPES[dtype], n, _SEED, offset, lo, hi)
        # (+1: the square of an f64 draw is rounded by the reference, maybe fused by the kernel)
        D = R.rand_depth(n, per, blocks) + (1 if op == "square_sum" and dtype == "float64" else 0)
        _check_bound(f"rand_reduce {dtype} {op} n={n} offset={offset} [{lo:g}, {hi:g}) blocks={blocks}", got,
                     _terms(op, x, None), D)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [2, 6, 1001, 1002])
def test_fused_draws_short(dev, dtype, n):
    """[0, 1) and [-1, 1): spans for which lo + span * u rounds once, fused or not, so the host stream
    has the kernel's bits.  1002 and 6 leave half a counter unused in f32 (n % 4 == 2), 1001 in both."""
    _check_rand_reduce(dev, dtype, n, 0, 0.0, 1.0)
    _check_rand_reduce(dev, dtype, n, 7, -1.0, 1.0)


@pytest.mark.parametrize("dtype,n", [("float64", 8_388_608 + 3), ("float32", 16_777_216 + 3)])
def test_fused_draws_on_the_capped_grid(dev, dtype, n):
    """One counter more than 2048 blocks x 256 lanes x 8 counters: the grid is capped and the lanes
    stride it; the odd n leaves the last counter partly used."""
    assert R.rand_blocks(n, _STREAM[dtype][1]) == R.RANDRED_BLOCKS
    _check_rand_reduce(dev, dtype, n, 0, 0.0, 1.0)


@pytest.mark.parametrize("offset", [2 ** 32 - 3, 2 ** 33 + 1])
def test_counter_offsets_carry_into_the_high_word(dev, offset):
    """offset + p crosses 2^32 (or starts above it) within the draw: the counter's high word changes.
    The fused reductions and the materialised streams of all three dtypes, the latter bit for bit."""
    for dtype in ("float64", "float32"):
        _check_rand_reduce(dev, dtype, 1001, offset, 0.0, 1.0)
        _check_rand_reduce(dev, dtype, 1001, offset, -1.0, 1.0)
    n = 4099
    for dtype, host in (("float64", uniform_f64(n, _SEED, offset, -1.0, 1.0)),
                        ("float32", uniform_f32(n, _SEED, offset, -1.0, 1.0)),
                        ("bfloat16", _f32_to_bf16_bits(uniform_f32(n, _SEED, offset, -1.0, 1.0)))):
        before = np.resize(_PERIOD, host.nbytes + PAD)
        p = dev.put(before)
        dev.drv.rand(0, p, n, DTYPES[dtype], _SEED, offset, -1.0, 1.0)
        after = np.empty_like(before)
        dev.drv.d2h(p, after)
        assert np.array_equal(after[host.nbytes:], before[host.nbytes:]), f"{dtype}: bytes past element {n} were written"
        assert np.array_equal(after[:host.nbytes], host.view(np.uint8)), f"{dtype} stream at offset {offset}"


# ---- axis sums ----------------------------------------------------------------------------------------

def _axis_shapes(dt: int) -> dict:
    """name -> (rows, cols, pad, pointer offset in elements), from the loops of colsum_tile_v,
    colsum_1pass, rowsum_v and rowsum; V = elements of a 16-byte vector."""
    V = R.vec(dt)
    return {
        # 3 strips x 3 chunks of 709, 709 and 707 rows: two trips of the 4-deep loop (256 rows each), then
        # single steps of 64 rows, the last of them partial
        "vector columns, 3 ragged chunks": (2125, 3 * 16 * V, V, 0),
        "vector columns, rows < 64": (37, 2 * 16 * V, 2 * V, 0),
        "scalar columns, two column blocks": (77, 257, 5, 0),
        "scalar columns, pointer off by one element": (37, 2 * 16 * V, 2 * V, 1),
        # 325 vectors a row: every lane one 4-deep trip (256), one single step (64), five lanes one more
        "vector rows": (5, V * (256 + 64 + 5), V, 0),
        "scalar rows": (5, V * (256 + 64 + 5) + 1, 3, 0),
        # f64: 8192 strips > kAxisTickets, the scalar kernel; f32: exactly 4096 strips; bf16: 2048
        "the widest matrix": (3, MAX_AXIS0_COLUMNS, V, 0),
    }


def _run_axis(dev, dt: int, wide: np.ndarray, pad: int, offset: int, op: int, axis: int) -> np.ndarray:
    """bk_reduce_axis on ``wide`` (f64 values the dtype holds exactly) stored with row stride
    cols + pad, the padding (and the ``offset`` elements before the matrix) NaN."""
    rows, cols = wide.shape
    ld = cols + pad
    full = np.full((rows, ld), np.nan)
    full[:, :cols] = wide
    stored = R.to_store(np.concatenate([np.full(offset, np.nan), full.ravel()]), dt)
    base = dev.put(stored)
    out_t = np.float64 if dt == F64 else np.float32
    count = cols if axis == 0 else rows
    nbytes = count * np.dtype(out_t).itemsize
    before = np.resize(_PERIOD, nbytes + PAD)
    y = dev.put(before)
    dev.drv.reduce_axis(op, dt, base + offset * stored.itemsize, y, rows, cols, ld, axis)
    after = np.empty_like(before)
    dev.drv.d2h(y, after)
    assert np.array_equal(after[nbytes:], before[nbytes:]), f"bytes past output element {count} were written"
    return after[:nbytes].view(out_t)


def _axis_ref(wide: np.ndarray, op: int, axis: int, out_t) -> np.ndarray:
    with np.errstate(all="ignore"):
        s = wide.sum(axis=axis)  # exact for the integer columns and rows; inf / NaN where one was planted
        return (s if op == 0 else s * (1.0 / wide.shape[axis])).astype(out_t)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", list(_axis_shapes(F64)))
def test_axis_sums_exact_with_padded_rows(dev, dtype, shape):
    dt = DTYPES[dtype]
    rows, cols, pad, offset = _axis_shapes(dt)[shape]
    wide = R.exact_ints(rows * cols).reshape(rows, cols).astype(np.float64)
    out_t = np.float64 if dt == F64 else np.float32
    for axis in (0, 1):
        assert np.abs(wide.sum(axis=axis)).max() < 2 ** 24  # exact in an f32 output too
        for op in (0, 1):
            got = _run_axis(dev, dt, wide, pad, offset, op, axis)
            ref = _axis_ref(wide, op, axis, out_t)
            assert not np.isnan(got).any(), f"{shape} {dtype} axis {axis}: the padding leaked into the result"
            bad = np.flatnonzero(got != ref)
            assert bad.size == 0, (f"{shape} {dtype} axis {axis} op {op}: {bad.size} differ, first at {bad[0]}: "
                                   f"got {got[bad[0]]!r}, exactly {ref[bad[0]]!r}")
        dev.drv.sync()
        dev.free()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", ["vector columns, 3 ragged chunks", "scalar columns, two column blocks"])
def test_axis_sums_keep_inf_and_nan_in_their_own_column_and_row(dev, dtype, shape):
    dt = DTYPES[dtype]
    rows, cols, pad, offset = _axis_shapes(dt)[shape]
    wide = R.exact_ints(rows * cols).reshape(rows, cols).astype(np.float64)
    wide[rows // 3, cols - 2] = np.inf
    wide[rows - 1, 1] = np.nan
    out_t = np.float64 if dt == F64 else np.float32
    for axis in (0, 1):
        ref = _axis_ref(wide, 0, axis, out_t)
        assert np.isnan(ref).sum() == 1 and np.isinf(ref).sum() == 1
        got = _run_axis(dev, dt, wide, pad, offset, 0, axis)
        assert np.array_equal(got, ref, equal_nan=True), f"{shape} {dtype} axis {axis}"


def test_axis_one_column_past_the_limit_is_refused(dev):
    from bee_code_interpreter_fs_amd.ops import _native

    if dev.drv.name != "native":
        pytest.skip("raw entry points: the native driver only")
    import ctypes

    vp = ctypes.c_void_p
    lib, cols = _native.lib(), MAX_AXIS0_COLUMNS + 1
    x = dev.put(np.ones(cols))
    before = np.resize(_PERIOD, cols * 8)
    y = dev.put(before)
    ws = dev.drv._workspace(WS_REDUCE_AXIS)
    for dt in (F64, F32, BF16):
        assert lib.bk_reduce_axis(0, dt, vp(x), 1, cols, cols, 0, vp(y), vp(ws), dev.drv.stream) == K_BAD_ARGUMENT
    assert lib.bk_reduce_axis(0, F64, vp(x), 1, cols - 1, cols - 2, 0, vp(y), vp(ws), dev.drv.stream) == K_BAD_ARGUMENT
    after = np.empty_like(before)
    dev.drv.d2h(y, after)
    assert np.array_equal(after, before)


# ---- the lab layouts and grid knobs: one child process each -----------------------------------------------
# BK_REDUCE_LAYOUT, BK_REDUCE_BLOCKS and BK_REDUCE_UNROLL are read once into statics (launch_reduce), so each
# setting needs a fresh interpreter.  The child runs the exact-integer checks above on the lengths at which
# every loop of the selected kernel runs (tests/reduce_inputs.py) and prints "ok".

LAB_CHILD = r"""
import os
import numpy as np
from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops.array import driver
from tests import reduce_inputs as R

layout = os.environ.get("BK_REDUCE_LAYOUT", "")
blocks = int(os.environ.get("BK_REDUCE_BLOCKS", R.RED_BLOCKS))
unroll = os.environ.get("BK_REDUCE_UNROLL")
two_operands = not layout.startswith("ldsdma")  # reduce_ldsdma: single-operand ops; dot goes to reduce_1pass
ops.init(0)
d = driver()
assert d.name == "native"


def lengths(N):
    if unroll:  # reduce_1pass<U = 4 / 8>: the non-temporal path only
        return [R.unroll_length()]
    if blocks > 2048:  # the fold's loop goes round twice
        return [R.fold_twice_length(N, blocks)]
    out = [R.all_loops_length(N, blocks)]  # reduce_1pass and reduce_chunked: every loop on `blocks` blocks
    if layout.startswith("ldsdma"):
        out += R.ldsdma_lengths(N, blocks)  # idle waves, short waves, 27-piece waves
    return out


def poke(p, dt, k, value):
    d.h2d(p, R.to_store(np.array([value]), dt), offset=k * np.dtype(R.STORE[dt]).itemsize)


for dt in (R.F64,) if unroll else (R.F64, R.F32, R.BF16):
    N = R.vec(dt)
    for n in lengths(N):
        assert R.grid_blocks(n, N, blocks) <= blocks
        a, b = R.exact_ints(n, 0), R.exact_ints(n, 1)
        want = R.exact_sums(a, b)
        pa = d.malloc(n * 16 // N)
        d.h2d(pa, R.to_store(a, dt))
        for op in (R.SUM, R.SQUARE_SUM, R.ABS_SUM):
            got = d.reduce(op, dt, pa, 0, n)
            assert got == want[op], (dt, n, op, got, want[op])
        if two_operands:
            pb = d.malloc(n * 16 // N)
            d.h2d(pb, R.to_store(b, dt))
            got = d.reduce(R.DOT, dt, pa, pb, n)
            assert got == want[R.DOT], (dt, n, "dot", got, want[R.DOT])
            got = d.reduce(R.MAX_ABS_DIFF, dt, pa, pb, n)
            assert got == int(np.abs(a - b).max()), (dt, n, "max_abs_diff", got)
            d.free(pb)
        assert d.reduce(R.MAX, dt, pa, 0, n) == a.max() and d.reduce(R.MIN, dt, pa, 0, n) == a.min(), (dt, n)
        for k in sorted({0, (n // N // 2) * N + N - 1, (n // N) * N - 1, n - 1}):  # vectors and the tail
            poke(pa, dt, k, 300)
            assert d.reduce(R.MAX, dt, pa, 0, n) == 300, (dt, n, "max", k)
            poke(pa, dt, k, -300)
            assert d.reduce(R.MIN, dt, pa, 0, n) == -300, (dt, n, "min", k)
            poke(pa, dt, k, a[k])
        assert d.reduce(R.SUM, dt, pa, 0, n) == want[R.SUM], (dt, n, "sum again")
        d.sync()
        d.free(pa)
print("ok")
"""

LAB_SETTINGS = ([{"BK_REDUCE_LAYOUT": layout, **extra} for layout in ("chunk", "ldsdma", "ldsdma_stride")
                 for extra in ({}, {"BK_REDUCE_BLOCKS": "3"})]
                + [{"BK_REDUCE_BLOCKS": b} for b in ("1", "3", "640", "2049")]
                + [{"BK_REDUCE_UNROLL": u} for u in ("4", "8")])


@pytest.mark.parametrize("setting", LAB_SETTINGS, ids=lambda s: ",".join(f"{k[3:].lower()}={v}" for k, v in s.items()))
def test_lab_layouts_and_grid_knobs_in_a_child_process(gpu, setting):
    env = {k: v for k, v in os.environ.items()
           if k not in ("BK_REDUCE_LAYOUT", "BK_REDUCE_BLOCKS", "BK_REDUCE_UNROLL", "BEE_BROKER_SOCK")}
    env.update(setting)
    p = subprocess.run([sys.executable, "-c", LAB_CHILD], capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), f"{setting}: exit {p.returncode}\n{p.stdout}{p.stderr[-3000:]}"


RANDRED_CHILD = r"""
import os
import numpy as np
from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops.array import driver
from tests import reduce_inputs as R
from tests.philox_ref import uniform_f32, uniform_f64

knob = int(os.environ["BK_RANDRED_BLOCKS"])
seed = 0x5EED0FB0C511
ops.init(0)
d = driver()
assert d.name == "native"
for dt, stream, per in ((R.F64, uniform_f64, 2), (R.F32, uniform_f32, 4)):
    n = 3 * 8 * 256 * knob * per + per + 1  # three times the counters the capped grid takes at 8 a lane, and a partial one
    assert R.rand_blocks(n, per, knob) == knob < R.rand_blocks(n, per)
    x = stream(n, seed, 5, 0.0, 1.0).astype(np.float64)
    for op, terms in ((R.SUM, x), (R.SQUARE_SUM, x * x)):
        got = d.rand_reduce(op, dt, n, seed, 5, 0.0, 1.0)
        D = R.rand_depth(n, per, knob) + 1
        err, bound = abs(got - R.fsum(terms)), D * R.U * float(np.abs(terms).sum())
        print(f"RED rand_reduce blocks={knob} dtype={dt} op={op} n={n} D={D} err/bound={err / bound:.4g}")
        assert err <= bound, (dt, op, got, err, bound)
print("ok")
"""


@pytest.mark.parametrize("blocks", ["3"])
def test_rand_reduce_grid_knob_in_a_child_process(gpu, blocks):
    """BK_RANDRED_BLOCKS below 256 used to give a launch with no blocks; 3 blocks make every lane go
    round the loops of rand_reduce_f64 and rand_reduce_f32 several times on a few thousand counters."""
    env = {k: v for k, v in os.environ.items() if k not in ("BK_RANDRED_BLOCKS", "BEE_BROKER_SOCK")}
    env["BK_RANDRED_BLOCKS"] = blocks
    p = subprocess.run([sys.executable, "-c", RANDRED_CHILD], capture_output=True, text=True, timeout=240, cwd=ROOT,
                       env=env)
    print(p.stdout, end="")
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), f"exit {p.returncode}\n{p.stdout}{p.stderr[-3000:]}"

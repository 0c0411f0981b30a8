"""The int64 kernels (csrc/kernels/integer.hip) on the GPU, native driver.

Arithmetic, comparisons and casts are bit-exact against numpy at the sizes
where the kernels change path (the vector tail, one block, several blocks,
whole chunks), from 16-byte aligned pointers and from pointers one element
off, in every mode and in place, over the edge values.  The reduction is exact
whatever the grid.  The draws equal the reference model (tests/int_ref.py)
element by element -- the seeds are such that the model's smallest decision
margin exceeds 1e-9 (asserted here and in tests/test_int_cpu.py), a million
times the difference between two f64 log / lgamma implementations -- do not
depend on the grid, and pass a chi-square test against the exact pmf at 2^20
draws.  CPU twins: test_int_cpu.py, test_broker_int_cpu.py.
"""

import ctypes
import math
import os
import re
import tempfile

import numpy as np
import pytest

from . import int_ref as R
from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MAX = R.I64_MIN, R.I64_MAX
EDGES = [0, 1, -1, MIN, MAX, MIN + 1, MAX - 1, (1 << 53) + 1, (1 << 53) - 1, -(1 << 53) - 1, 7, -7, 3, -3, 2, -2]
# n = 5003: two whole chunks of kStreamUnroll x 256 vectors, then vectors, then an odd element
NS = [0, 1, 2, 3, 255, 256, 257, 5003]
_vp = ctypes.c_void_p


def _constant(path, name):
    text = open(os.path.join(ROOT, "csrc", "kernels", path)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


# the elements one block of bk_int_reduce covers before the grid grows: read from the kernel's own constants
BLOCK_SPAN = _constant("bk_ticket.hpp", "kRedBlock") * _constant("integer.hip", "kIntRedVecsPerLane") * 2
RED_BLOCKS = _constant("bk_ticket.hpp", "kRedBlocks")


def operands(n, salt=0):
    """Two int64 arrays of n elements: random over the whole range with the edge values sprinkled so that the
    pairs of edges meet."""
    rng = np.random.Generator(np.random.PCG64(1000 + n + salt))
    a = rng.integers(MIN, MAX, n, dtype=np.int64, endpoint=True)
    b = rng.integers(-50, 50, n, dtype=np.int64)
    b[::2] = rng.integers(MIN, MAX, (n + 1) // 2, dtype=np.int64, endpoint=True)
    L = len(EDGES)
    i = np.arange(n)
    ea, eb = np.array(EDGES, np.int64)[i % L], np.array(EDGES, np.int64)[(i // L) % L]
    pick = i % 3 != 2 if n >= L * L else np.ones(n, bool)
    a[pick], b[pick] = ea[pick], eb[pick]
    return a, b


def np_binary(op, a, b):
    fn = [np.add, np.subtract, np.multiply, np.floor_divide, np.remainder, np.maximum, np.minimum][op]
    with np.errstate(all="ignore"):
        return fn(a, b)


def np_compare(op, a, b):
    return [np.less, np.less_equal, np.greater, np.greater_equal, np.equal, np.not_equal][op](a, b)


class Dev:
    """n elements of a numpy dtype in device memory behind `lead` elements of padding, so that the array
    starts 16-byte aligned (lead 0) or one element off it."""

    def __init__(self, gpu, host, lead):
        self.host = np.ascontiguousarray(host)
        self.lead, self.n = lead, self.host.size
        self.item = self.host.dtype.itemsize
        self.fence = np.frombuffer(b"\xa5" * self.item, self.host.dtype)[0]
        padded = np.concatenate([np.full(lead, self.fence, self.host.dtype), self.host,
                                 np.full(3, self.fence, self.host.dtype)])
        self.arr = gpu.empty((padded.nbytes + 1) // 2, "bfloat16")  # raw bytes
        assert self.arr.ptr % 16 == 0
        from bee_code_interpreter_fs_amd.ops.array import driver

        self.d = driver()
        self.d.h2d(self.arr.ptr, padded)
        self.ptr = self.arr.ptr + lead * self.item

    def read(self):
        """The n elements; the padding around them must be untouched."""
        out = np.empty(self.lead + self.n + 3, self.host.dtype)
        self.d.d2h(self.arr.ptr, out)
        raw = out.view(np.uint8).reshape(-1, self.item)
        fence = np.frombuffer(self.fence.tobytes(), np.uint8)
        assert (raw[:self.lead] == fence).all() and (raw[self.lead + self.n:] == fence).all(), "wrote out of bounds"
        return out[self.lead:self.lead + self.n]


# ---- arithmetic ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset-8"])
@pytest.mark.parametrize("op", range(7), ids=["add", "subtract", "multiply", "floor_divide", "remainder", "max", "min"])
def test_binary_is_bit_exact_in_every_mode(gpu, op, lead):
    for n in NS:
        a, b = operands(n)
        for scalar in (0, -1, 3, MIN, MAX):
            for mode in (1, 2):
                x, y = Dev(gpu, a, lead), Dev(gpu, np.zeros(n, np.int64), lead)
                x.d.int_binary(op, mode, x.ptr, 0, scalar, y.ptr, n)
                s = np.int64(scalar)
                want = np_binary(op, a, s) if mode == 1 else np_binary(op, s, a)
                np.testing.assert_array_equal(y.read(), want, err_msg=f"op {op} mode {mode} n {n} scalar {scalar}")
            if n > 300:
                break  # (one scalar at the large size: the paths are the same)
        x, w, y = Dev(gpu, a, lead), Dev(gpu, b, lead), Dev(gpu, np.zeros(n, np.int64), lead)
        x.d.int_binary(op, 0, x.ptr, w.ptr, 0, y.ptr, n)
        np.testing.assert_array_equal(y.read(), np_binary(op, a, b), err_msg=f"op {op} arrays n {n}")
        # in place: y = a, then y = b
        x.d.int_binary(op, 0, x.ptr, w.ptr, 0, x.ptr, n)
        np.testing.assert_array_equal(x.read(), np_binary(op, a, b), err_msg=f"op {op} in place (a) n {n}")
        x2 = Dev(gpu, a, lead)
        x.d.int_binary(op, 0, x2.ptr, w.ptr, 0, w.ptr, n)
        np.testing.assert_array_equal(w.read(), np_binary(op, a, b), err_msg=f"op {op} in place (b) n {n}")


def test_binary_with_operands_of_different_alignment(gpu):
    """a 16-byte aligned, b and y one element off (and the other way round): the element-wise path."""
    n = 1031
    a, b = operands(n, salt=5)
    for la, lb, ly in ((0, 1, 1), (1, 0, 0), (0, 0, 1)):
        x, w, y = Dev(gpu, a, la), Dev(gpu, b, lb), Dev(gpu, np.zeros(n, np.int64), ly)
        for op in (0, 3, 4):
            x.d.int_binary(op, 0, x.ptr, w.ptr, 0, y.ptr, n)
            np.testing.assert_array_equal(y.read(), np_binary(op, a, b))
        m = Dev(gpu, np.zeros(n, np.uint8), 0)
        x.d.int_compare(0, 0, x.ptr, w.ptr, 0, m.ptr, n)
        np.testing.assert_array_equal(m.read() != 0, a < b)


def test_every_pair_of_edge_values(gpu):
    """Division and remainder by 0 and -1, INT64_MIN on either side, mixed signs, wrapping products."""
    e = np.array(EDGES, np.int64)
    a, b = np.repeat(e, e.size), np.tile(e, e.size)
    for op in range(7):
        x, w, y = Dev(gpu, a, 0), Dev(gpu, b, 0), Dev(gpu, np.zeros(a.size, np.int64), 0)
        x.d.int_binary(op, 0, x.ptr, w.ptr, 0, y.ptr, a.size)
        got = y.read()
        np.testing.assert_array_equal(got, np_binary(op, a, b), err_msg=f"op {op}")
        np.testing.assert_array_equal(got, R.binary(op, a, b), err_msg=f"op {op} (the reference semantics)")


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset-8"])
def test_compare_is_bit_exact(gpu, lead):
    for n in NS:
        a, b = operands(n)
        b[::5] = a[::5]  # equal pairs
        for op in range(6):
            for mask_lead in (0, 1):  # the mask's own alignment: 2-byte stores or byte stores
                x, w = Dev(gpu, a, lead), Dev(gpu, b, lead)
                m = Dev(gpu, np.full(n, 7, np.uint8), mask_lead)
                x.d.int_compare(op, 0, x.ptr, w.ptr, 0, m.ptr, n)
                np.testing.assert_array_equal(m.read(), np_compare(op, a, b).astype(np.uint8), err_msg=f"op {op} n {n}")
                for scalar in (0, MIN, MAX, int(a[n // 2]) if n else 5):
                    m = Dev(gpu, np.full(n, 7, np.uint8), mask_lead)
                    x.d.int_compare(op, 1, x.ptr, 0, scalar, m.ptr, n)
                    np.testing.assert_array_equal(m.read(), np_compare(op, a, np.int64(scalar)).astype(np.uint8),
                                                  err_msg=f"op {op} n {n} scalar {scalar}")


def test_a_mask_of_int64_feeds_the_mask_kernels(gpu):
    n = 70001
    h = np.random.Generator(np.random.PCG64(3)).integers(-9, 10, n)
    x = gpu.asarray(h, dtype="int64")
    m = x > 2
    assert m.dtype == "bool" and gpu.sum(m) == (h > 2).sum() and gpu.mean(m) == (h > 2).mean()
    both = m & (x < 7)
    np.testing.assert_array_equal(both.numpy(), (h > 2) & (h < 7))
    np.testing.assert_array_equal(x[both].numpy(), h[(h > 2) & (h < 7)])
    np.testing.assert_array_equal(gpu.where(m, x, -x).numpy(), np.where(h > 2, h, -h))
    np.testing.assert_array_equal(gpu.where(m, x, 0).numpy(), np.where(h > 2, h, 0))
    assert gpu.any(m) and not gpu.all(m) and gpu.count_nonzero(x) == np.count_nonzero(h)


CAST_FLOATS = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.0 ** 63, -2.0 ** 63, 2.0 ** 63 * (1 - 2.0 ** -53), -2.0 ** 63 * (1 + 2.0 ** -52),
               float("nan"), float("inf"), float("-inf"), 1e300, -1e300, 2.0 ** 53 + 2, 16777217.0, -3.999, 1e-320]


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset-8"])
def test_casts_are_numpys(gpu, lead):
    for n in NS:
        a, _ = operands(n)
        a[1::7] = (1 << 24) + 1  # rounds to even in float32
        a[2::7] = (1 << 53) + 1  # and in float64
        for dst, code in ((np.float64, R.F64), (np.float32, R.F32)):
            x, y = Dev(gpu, a, lead), Dev(gpu, np.zeros(n, dst), lead)
            x.d.int_cast(R.I64, code, x.ptr, y.ptr, n)
            want = a.astype(dst)
            assert y.read().tobytes() == want.tobytes(), f"int64 -> {dst.__name__} n {n}"
        rng = np.random.Generator(np.random.PCG64(n))
        for src, code in ((np.float64, R.F64), (np.float32, R.F32)):
            f = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 22, n)).astype(src)
            k = min(n, len(CAST_FLOATS))
            with np.errstate(all="ignore"):
                f[:k] = np.array(CAST_FLOATS[:k]).astype(src)
                want = f.astype(np.int64)
            x, y = Dev(gpu, f, lead), Dev(gpu, np.zeros(n, np.int64), lead)
            x.d.int_cast(code, R.I64, x.ptr, y.ptr, n)
            got = y.read()
            np.testing.assert_array_equal(got, R.float_to_int64(f), err_msg=f"{src.__name__} -> int64 n {n}")
            np.testing.assert_array_equal(got, want, err_msg=f"{src.__name__} -> int64 n {n} (numpy's astype)")
        bits = rng.integers(0, 3, n).astype(np.uint8) * 127  # 0, 127, 254: any non-zero byte is true
        x, y = Dev(gpu, bits, lead), Dev(gpu, np.zeros(n, np.int64), lead)
        x.d.int_cast(R.BOOL, R.I64, x.ptr, y.ptr, n)
        np.testing.assert_array_equal(y.read(), (bits != 0).astype(np.int64))


# ---- reductions ------------------------------------------------------------------------------------------

RED_NS = [0, 1, BLOCK_SPAN - 1, BLOCK_SPAN, BLOCK_SPAN + 1, BLOCK_SPAN + 2, 5 * BLOCK_SPAN + 3,
          RED_BLOCKS * BLOCK_SPAN * 2 + BLOCK_SPAN + 3]  # the last: every lane loops, the 8-vector loop included


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset-8"])
def test_reduce_is_exact_whatever_the_grid(gpu, lead):
    assert BLOCK_SPAN == 2048
    for n in RED_NS:
        rng = np.random.Generator(np.random.PCG64(n))
        a = rng.integers(MIN // 4, MAX // 4, n, dtype=np.int64)  # the sum wraps many times over
        x = Dev(gpu, a, lead)
        for op in range(3):
            assert x.d.int_reduce(op, x.ptr, n) == R.reduce(op, a), f"op {op} n {n}"
        if n:
            assert R.reduce(0, a) == int(a.sum())  # numpy's own wrapping sum
        small = rng.integers(-1000, 1000, n, dtype=np.int64)
        for at in sorted({0, n - 1, min(BLOCK_SPAN - 1, n - 1), min(BLOCK_SPAN, n - 1)} if n else ()):
            for op, v in ((1, MAX), (2, MIN), (1, 1000), (2, -1001)):
                b = small.copy()
                b[at] = v
                y = Dev(gpu, b, lead)
                assert y.d.int_reduce(op, y.ptr, n) == v, f"op {op} extremum at {at} of {n}"


def test_an_overflowing_sum_wraps_like_numpys(gpu):
    a = np.array([MAX, 1, MAX, 5, MIN, MIN, -3], np.int64)
    x = gpu.asarray(a, dtype="int64")
    with np.errstate(all="ignore"):
        assert gpu.sum(x) == a.sum() and isinstance(gpu.sum(x), np.int64)
    assert x.max() == MAX and x.min() == MIN and isinstance(x.max(), np.int64)


def test_two_launches_back_to_back_on_one_workspace(gpu):
    """No wait between them: the first leaves the ticket re-armed and its partials are dead by then."""
    from bee_code_interpreter_fs_amd.ops.array import driver

    d = driver()
    rng = np.random.Generator(np.random.PCG64(8))
    a = rng.integers(MIN // 4, MAX // 4, 7 * BLOCK_SPAN + 5, dtype=np.int64)
    b = rng.integers(MIN // 4, MAX // 4, 3 * BLOCK_SPAN + 1, dtype=np.int64)
    x, y, out = Dev(gpu, a, 0), Dev(gpu, b, 1), Dev(gpu, np.zeros(4, np.int64), 0)
    ws = d.workspaces[0]
    for i, (op, v) in enumerate(((0, x), (1, y), (0, y), (2, x))):
        rc = d.lib.bk_int_reduce(op, _vp(v.ptr), v.n, _vp(ws), _vp(out.ptr + 8 * i), d.stream)
        assert rc == 0
    d.sync()
    assert out.read().tolist() == [R.reduce(0, a), R.reduce(1, b), R.reduce(0, b), R.reduce(2, a)]
    assert d.reduce(0, 1, gpu.ones(1000).ptr, 0, 1000) == 1000.0  # the float reductions share the workspace


# ---- draws --------------------------------------------------------------------------------------------------

def device_draw(g, kind, a, b, p, n):
    if kind == R.INTEGERS:
        return g.integers(a, b, n)
    if kind == R.POISSON:
        return g.poisson(p, n)
    if kind == R.BINOMIAL:
        return g.binomial(a, p, n)
    return g.geometric(p, n)


def case_id(c):
    kind, a, b, p = c
    return f"{R.NAMES[kind]}-{a}-{b}-{p}"


@pytest.mark.parametrize("low,high", R.INTEGER_CASES, ids=[f"span-{h - lo}" for lo, h in R.INTEGER_CASES])
def test_integers_match_the_model(gpu, low, high):
    n = R.INTEGER_N
    g = gpu.random.default_rng(R.EXACT_SEED)
    got = g.integers(low, high, n)
    assert got.dtype == "int64" and got.shape == (n,) and g._offset == R.counters(R.INTEGERS, n, low, high)
    want, attempts = R.integers(n, R.EXACT_SEED, 0, low, high)
    print(f"INT_ATTEMPTS integers [{low}, {high}) most attempts {attempts}")
    h = got.numpy()
    np.testing.assert_array_equal(h, want)
    assert h.min() >= low and h.max() < high
    nxt = g.integers(low, high, 259).numpy()  # the next draw continues at the next counter
    np.testing.assert_array_equal(nxt, R.integers(259, R.EXACT_SEED, R.counters(R.INTEGERS, n, low, high), low, high)[0])
    # from a pointer one element off a 16-byte boundary
    y = Dev(gpu, np.zeros(1001, np.int64), 1)
    y.d.rand_int(R.INTEGERS, y.ptr, 1001, R.EXACT_SEED, 0, low, high, 0.0)
    np.testing.assert_array_equal(y.read(), want[:1001])


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=[case_id(c) for c in R.EXACT_CASES])
def test_poisson_binomial_geometric_match_the_model(gpu, case):
    kind, a, b, p = case
    n = R.EXACT_N
    if kind == R.POISSON:
        want, margin, attempts = R.poisson(n, R.EXACT_SEED, 0, p)
    elif kind == R.BINOMIAL:
        want, margin, attempts = R.binomial(n, R.EXACT_SEED, 0, a, p)
    else:
        (want, margin), attempts = R.geometric(n, R.EXACT_SEED, 0, p), 1
    print(f"INT_MARGIN {case_id(case)} smallest decision margin {margin.min():.3g}, most attempts {attempts}")
    assert margin.min() > 1e-9 and attempts <= 16
    g = gpu.random.default_rng(R.EXACT_SEED)
    got = device_draw(g, kind, a, b, p, n)
    assert got.dtype == "int64" and g._offset == R.counters(kind, n)
    np.testing.assert_array_equal(got.numpy(), want)


@pytest.mark.parametrize("case", [(R.INTEGERS, 1, 7, 0.0), (R.INTEGERS, 0, 1 << 40, 0.0), (R.POISSON, 0, 0, 3.0),
                                  (R.POISSON, 0, 0, 50.0), (R.BINOMIAL, 10, 0, .5), (R.BINOMIAL, 1000, 0, .3),
                                  (R.GEOMETRIC, 0, 0, .2)], ids=case_id)
def test_a_draw_does_not_depend_on_the_grid(gpu, case):
    """A prefix of an n-element draw is the shorter draw (n no multiple of 4), also across many blocks."""
    kind, a, b, p = case
    for n, m in ((1003, 501), (300007, 2051)):
        long = device_draw(gpu.random.default_rng(5), kind, a, b, p, n).numpy()
        short = device_draw(gpu.random.default_rng(5), kind, a, b, p, m).numpy()
        np.testing.assert_array_equal(long[:m], short)


@pytest.mark.parametrize("case", R.CHI_CASES, ids=[case_id(c) for c in R.CHI_CASES])
def test_chi_square_against_the_exact_pmf(gpu, case):
    """At 2^20 draws, cells with an expected count below 5 pooled: the statistic stays below the chi-square
    1 - 1e-6 quantile (Wilson-Hilferty).  A condition, not a measurement."""
    kind, a, b, p = case
    x = device_draw(gpu.random.default_rng(0x1D7 + kind), kind, a, b, p, R.CHI_N).numpy()
    stat, df = R.chi_square(kind, x, a, b, p)
    print(f"INT_CHI2 {case_id(case)} statistic {stat:.2f} df {df} bound {R.chi_square_bound(df):.2f}")
    assert df >= 5 and stat <= R.chi_square_bound(df)


def test_the_entry_points_refuse_bad_arguments(gpu):
    """kBadArgument before any launch (the driver raises); n = 0 is fine."""
    from bee_code_interpreter_fs_amd.ops.array import BeekernError, driver

    d = driver()
    x, m = gpu.zeros(64, "int64"), gpu.zeros(64, "bool")
    nan = float("nan")
    d.rand_int(R.POISSON, x.ptr, 0, 1, 0, 0, 0, 3.0)
    d.int_binary(0, 0, x.ptr, x.ptr, 0, x.ptr, 0)
    d.int_compare(0, 1, x.ptr, 0, 0, m.ptr, 0)
    d.int_cast(R.I64, R.F64, x.ptr, x.ptr, 0)
    bad = [
        lambda: d.rand_int(4, x.ptr, 8, 1, 0, 0, 6, 0.5), lambda: d.rand_int(-1, x.ptr, 8, 1, 0, 0, 6, 0.5),
        lambda: d.rand_int(R.INTEGERS, 0, 8, 1, 0, 0, 6, 0.0), lambda: d.rand_int(R.INTEGERS, x.ptr, -1, 1, 0, 0, 6, 0.0),
        lambda: d.rand_int(R.INTEGERS, x.ptr, 8, 1, 0, 6, 6, 0.0), lambda: d.rand_int(R.INTEGERS, x.ptr, 8, 1, 0, 7, 6, 0.0),
        lambda: d.rand_int(R.POISSON, x.ptr, 8, 1, 0, 0, 0, -1.0), lambda: d.rand_int(R.POISSON, x.ptr, 8, 1, 0, 0, 0, nan),
        lambda: d.rand_int(R.POISSON, x.ptr, 8, 1, 0, 0, 0, 2.0 ** 54),
        lambda: d.rand_int(R.BINOMIAL, x.ptr, 8, 1, 0, -1, 0, 0.5), lambda: d.rand_int(R.BINOMIAL, x.ptr, 8, 1, 0, 1 << 53, 0, 0.5),
        lambda: d.rand_int(R.BINOMIAL, x.ptr, 8, 1, 0, 5, 0, 1.5), lambda: d.rand_int(R.BINOMIAL, x.ptr, 8, 1, 0, 5, 0, nan),
        lambda: d.rand_int(R.GEOMETRIC, x.ptr, 8, 1, 0, 0, 0, 0.0), lambda: d.rand_int(R.GEOMETRIC, x.ptr, 8, 1, 0, 0, 0, 1.5),
        lambda: d.int_binary(7, 0, x.ptr, x.ptr, 0, x.ptr, 8), lambda: d.int_binary(-1, 0, x.ptr, x.ptr, 0, x.ptr, 8),
        lambda: d.int_binary(0, 3, x.ptr, x.ptr, 0, x.ptr, 8), lambda: d.int_binary(0, 0, x.ptr, 0, 0, x.ptr, 8),
        lambda: d.int_binary(0, 1, 0, 0, 0, x.ptr, 8), lambda: d.int_binary(0, 1, x.ptr, 0, 0, x.ptr, -1),
        lambda: d.int_compare(6, 1, x.ptr, 0, 0, m.ptr, 8), lambda: d.int_compare(0, 2, x.ptr, 0, 0, m.ptr, 8),
        lambda: d.int_compare(0, 0, x.ptr, 0, 0, m.ptr, 8), lambda: d.int_compare(0, 1, x.ptr, 0, 0, 0, 8),
        lambda: d.int_reduce(3, x.ptr, 8), lambda: d.int_reduce(0, 0, 8), lambda: d.int_reduce(0, x.ptr, -1),
        lambda: d.int_cast(R.I64, R.I64, x.ptr, x.ptr, 8), lambda: d.int_cast(R.I64, 2, x.ptr, x.ptr, 8),
        lambda: d.int_cast(2, R.I64, x.ptr, x.ptr, 8), lambda: d.int_cast(R.I64, R.BOOL, x.ptr, m.ptr, 8),
        lambda: d.int_cast(R.F64, R.F32, x.ptr, x.ptr, 8), lambda: d.int_cast(R.I64, R.F64, x.ptr, x.ptr, -1),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(BeekernError):
            call()
            pytest.fail(f"call {i} was accepted")
    gpu.synchronize()
    assert (x.numpy() == 0).all() and not m.numpy().any()
    with pytest.raises(ValueError):
        gpu.random.poisson(-1.0, 8)
    with pytest.raises(ValueError):
        gpu.random.integers(5, 5, 8)


# ---- through the service -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dsvc():
    ensure_native_executor()
    h = ServiceHarness(tempfile.mkdtemp(prefix="bee-int-"), gpu_ids=[0], workers_per_gpu_target=1, default_timeout=120.0)
    h.start()
    yield h
    h.stop()


def test_dice_and_counts_in_a_broker_sandbox(dsvc):
    """examples/dice_and_counts.py through the kernel broker.  Each printed share is a binomial proportion of
    n = 2e6 draws, within 6 standard errors of its exact value; each mean within 6 standard errors of the
    distribution's mean; the Poisson figures at the printed rate (the frailty's sample mean)."""
    src = open(os.path.join(ROOT, "examples", "dice_and_counts.py")).read()
    r = dsvc.call(dsvc.ctx.code_executor.execute(source_code=src, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert "HostFallbackWarning" not in r.stderr, r.stderr
    labels = ("P(total is 7):", "Mean total:", "Largest total:", "Claim rate:", "Mean claims per policy:",
              "Share with two or more claims:", "Mean heads in ten flips:", "Share with eight or more heads:", "Total heads:")
    got = {label: float(r.stdout.split(label)[1].split()[0]) for label in labels}
    n = 2e6

    def se(p):
        return (p * (1 - p) / n) ** 0.5

    assert abs(got["P(total is 7):"] - 1 / 6) < 6 * se(1 / 6), got
    assert abs(got["Mean total:"] - 7.0) < 6 * (35 / 6 / n) ** 0.5, got  # two dice: variance 35 / 6
    assert got["Largest total:"] == 12
    lam = got["Claim rate:"]
    assert abs(lam - 1.0) < 6 * (0.5 / n) ** 0.5, got  # gamma(2, 1/2): mean 1, variance 1/2
    assert abs(got["Mean claims per policy:"] - lam) < 6 * (lam / n) ** 0.5, got
    two = 1 - math.exp(-lam) * (1 + lam)
    assert abs(got["Share with two or more claims:"] - two) < 6 * se(two), got
    assert abs(got["Mean heads in ten flips:"] - 5.0) < 6 * (2.5 / n) ** 0.5, got
    eight = 56 / 1024
    assert abs(got["Share with eight or more heads:"] - eight) < 6 * se(eight), got
    assert got["Total heads:"] == pytest.approx(got["Mean heads in ten flips:"] * n, rel=1e-12)
    assert [6 * se(1 / 6), 6 * se(two), 6 * se(eight)] == pytest.approx([0.00158, 0.00187, 0.00096], rel=0.03)

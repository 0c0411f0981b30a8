"""The fused entry points of csrc/kernels on the MI355X: an axis reduction with
a second, converted output (bk_reduce_axis_cast), and a producer that closes
with the scalar reduction of its output (bk_reduce_axis_tail,
bk_gemm_bf16_tn_tail).

Each is compared bit for bit with the two launches it replaces (bk_reduce_axis
or bk_gemm_bf16_tn, then bk_cast or bk_reduce), and with numpy:

* axis sums against the f64 sum of the stored inputs, within 1e-9 of the sum of
  their magnitudes (test_workspace_gpu.py's bound for an axis; the f64
  accumulation of at most 2050 terms errs by far less) plus, for an f32
  output, its one rounding, 2^-24 of the value;
* a cast against numpy's conversion of the stored output (exact; bf16 by
  round-to-nearest-even through f32);
* a closing sum within 1e-10 of the sum of magnitudes (test_workspace_gpu.py's
  bound for bk_reduce); max and max |a - b| exactly, from the stored values.

Shapes are the smallest that reach each path: two column strips with the
second ragged and three row chunks (the ticket fold runs); the scalar kernels;
17 row blocks, more than the 8 XCDs; the closing reduction's single-block
limit and one vector past it.  Every tail runs twice on one workspace, so a
ticket that is not re-armed shows."""

import ctypes
import struct

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops import _native
from bee_code_interpreter_fs_amd.ops.array import _f32_to_bf16_bits
from bee_code_interpreter_fs_amd.ops.array import driver as _driver

pytestmark = pytest.mark.gpu

WS_REDUCE, WS_REDUCE_AXIS = 0, 1  # enum BkWorkspace
F32, F64, BF16 = 0, 1, 2
NAME = {F32: "float32", F64: "float64", BF16: "bfloat16"}
SUM, SQUARE_SUM, ABS_SUM, MAX, MIN, DOT, MAX_ABS_DIFF = range(7)
BAD_ARGUMENT = 1
_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def ws(gpu):
    """One workspace of each kind for the module, from dirty blocks."""
    d, lib = _driver(), _native.lib()
    made = {}
    for kind in (WS_REDUCE, WS_REDUCE_AXIS):
        nbytes = lib.bk_workspace_bytes(kind)
        made[kind] = d.malloc(nbytes)
        d.fill(made[kind], nbytes, 0xA5, 1)
        _native.check(lib.bk_workspace_init(kind, _vp(made[kind]), d.stream), "bk_workspace_init")
    yield made
    d.sync()
    for p in made.values():
        d.free(p)


def _matrix(gpu, rows, cols, dtype, seed):
    """A device matrix and the f64 values it really holds."""
    h = np.random.default_rng(seed).uniform(-1, 1, (rows, cols))
    x = gpu.asarray(h, NAME[dtype])
    return x, x.numpy().astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _axis(lib, d, ws, x, rows, cols, axis, op, out):
    _native.check(lib.bk_reduce_axis(op, x.code, _vp(x.ptr), rows, cols, cols, axis, _vp(out.ptr), _vp(ws[WS_REDUCE_AXIS]),
                                     d.stream), "bk_reduce_axis")


def _reduce(lib, d, ws, op, dt, a, b, n, scalar):
    _native.check(lib.bk_reduce(op, dt, _vp(a), _vp(b) if b else None, n, _vp(ws[WS_REDUCE]), _vp(scalar.ptr), d.stream),
                  "bk_reduce")
    return struct.pack("<d", scalar.numpy()[0])


def _check_axis_sum(got, h, axis, op, out_dt):
    want = h.sum(axis=axis) if op == 0 else h.mean(axis=axis)
    scale = 1.0 if op == 0 else 1.0 / h.shape[axis]
    tol = 1e-9 * np.abs(h).sum(axis=axis) * scale + (2.0 ** -24 * np.abs(want) if out_dt == F32 else 0.0)
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol)


def _host_cast(stored, cdt):
    if cdt == BF16:
        return (_f32_to_bf16_bits(stored.astype(np.float32)).astype(np.uint32) << 16).view(np.float32)
    return stored.astype(np.float64 if cdt == F64 else np.float32)


# (rows, cols, input dtype): the 16-byte column kernel in bf16, f32 and f64 -- two strips, the second ragged, three
# row chunks -- and the scalar column kernel
COLUMN_SHAPES = [(2050, 136, BF16), (2050, 68, F32), (2050, 34, F64), (70, 37, F32), (70, 37, BF16), (70, 37, F64)]
# the 16-byte row kernel (17 blocks, the last ragged) and the scalar one
ROW_SHAPES = [(67, 520, F32), (67, 520, BF16), (67, 37, F32), (67, 37, F64)]


@pytest.mark.parametrize("op", [0, 1], ids=["sum", "mean"])
@pytest.mark.parametrize("rows,cols,dt,axis", [(*s, 0) for s in COLUMN_SHAPES] + [(*s, 1) for s in ROW_SHAPES])
def test_axis_reduction_with_cast(gpu, ws, rows, cols, dt, axis, op):
    d, lib = _driver(), _native.lib()
    x, h = _matrix(gpu, rows, cols, dt, 11)
    n = cols if axis == 0 else rows
    out_dt = F64 if dt == F64 else F32
    plain = gpu.empty((n,), NAME[out_dt])
    _axis(lib, d, ws, x, rows, cols, axis, op, plain)
    _check_axis_sum(plain.numpy(), h, axis, op, out_dt)
    for cdt in (F32, F64, BF16):  # every supported pair, and the one that is none
        fused, cast_plain, cast_fused = gpu.empty((n,), NAME[out_dt]), gpu.empty((n,), NAME[cdt]), gpu.empty((n,), NAME[cdt])
        rc = lib.bk_reduce_axis_cast(op, x.code, _vp(x.ptr), rows, cols, cols, axis, _vp(fused.ptr), cdt, _vp(cast_fused.ptr),
                                     _vp(ws[WS_REDUCE_AXIS]), d.stream)
        if cdt == out_dt:
            assert rc == BAD_ARGUMENT  # bk_cast has no such pair either
            continue
        _native.check(rc, "bk_reduce_axis_cast")
        _native.check(lib.bk_cast(out_dt, cdt, _vp(plain.ptr), _vp(cast_plain.ptr), n, d.stream), "bk_cast")
        assert _bits(fused.numpy()) == _bits(plain.numpy())
        assert _bits(cast_fused.numpy()) == _bits(cast_plain.numpy())
        assert _bits(cast_fused.numpy()) == _bits(_host_cast(plain.numpy(), cdt))


def _tail_axis(lib, d, ws, x, rows, cols, axis, out, top, a, b, n, scalar):
    return lib.bk_reduce_axis_tail(0, x.code, _vp(x.ptr), rows, cols, cols, axis, _vp(out.ptr), _vp(ws[WS_REDUCE_AXIS]), top,
                                   _vp(a), _vp(b) if b else None, n, _vp(ws[WS_REDUCE]), _vp(scalar.ptr), d.stream)


def _check_scalar(top, got, a, b):
    """got against the stored operands (f64 arrays)."""
    if top == SUM:
        assert abs(got - a.sum()) <= 1e-10 * np.abs(a).sum()
    elif top == SQUARE_SUM:
        assert abs(got - (a * a).sum()) <= 1e-10 * (a * a).sum()
    elif top == DOT:
        assert abs(got - (a * b).sum()) <= 1e-10 * np.abs(a * b).sum()
    elif top == MAX:
        assert got == a.max()
    elif top == MAX_ABS_DIFF:
        assert got == np.abs(a - b).max()


@pytest.mark.parametrize("top", [SUM, MAX, SQUARE_SUM, MAX_ABS_DIFF, DOT])
@pytest.mark.parametrize("rows,cols,dt,axis", [(*s, 1) for s in ROW_SHAPES] + [(2050, 136, BF16, 0), (2050, 34, F64, 0),
                                                                                 (70, 37, F32, 0)])
def test_axis_reduction_with_closing_reduce(gpu, ws, rows, cols, dt, axis, top):
    d, lib = _driver(), _native.lib()
    x, h = _matrix(gpu, rows, cols, dt, 12)
    n = cols if axis == 0 else rows
    out_dt = F64 if dt == F64 else F32
    plain, fused, scalar = gpu.empty((n,), NAME[out_dt]), gpu.empty((n,), NAME[out_dt]), gpu.empty((1,))
    other = gpu.asarray(np.random.default_rng(13).uniform(-1, 1, n), NAME[out_dt])
    two = top in (DOT, MAX_ABS_DIFF)
    _axis(lib, d, ws, x, rows, cols, axis, 0, plain)
    for swapped in ([False, True] if two else [False]):  # the produced operand as a, then as b
        pa, pb = (other.ptr, plain.ptr) if swapped else (plain.ptr, other.ptr if two else 0)
        fa, fb = (other.ptr, fused.ptr) if swapped else (fused.ptr, other.ptr if two else 0)
        want = _reduce(lib, d, ws, top, out_dt, pa, pb, n, scalar)
        for _ in range(2):  # the second run finds the tickets re-armed
            d.fill(fused.ptr, n * (8 if out_dt == F64 else 4), 0xA5, 1)
            _native.check(_tail_axis(lib, d, ws, x, rows, cols, axis, fused, top, fa, fb, n, scalar), "bk_reduce_axis_tail")
            got = scalar.numpy()[0]
            assert struct.pack("<d", got) == want
            assert _bits(fused.numpy()) == _bits(plain.numpy())
        a64, b64 = plain.numpy().astype(np.float64), other.numpy().astype(np.float64)
        _check_scalar(top, got, *((b64, a64) if swapped else (a64, b64)))
    # and bk_reduce still finds its workspace as it needs it
    assert _reduce(lib, d, ws, top, out_dt, plain.ptr, other.ptr if two else 0, n, scalar) == \
        _reduce(lib, d, ws, top, out_dt, fused.ptr, other.ptr if two else 0, n, scalar)


@pytest.mark.parametrize("dt,limit", [(F32, 4 * 1024 + 3), (F64, 2 * 1024 + 1)])
def test_closing_reduce_stops_at_the_single_block_limit(gpu, ws, dt, limit):
    """bk_reduce runs one block up to 1024 16-byte vectors and the scalar rest;
    one vector more is two blocks, and no tail."""
    d, lib = _driver(), _native.lib()
    per = 16 // (8 if dt == F64 else 4)
    rows = limit - (per - 1) + per  # one vector past
    x, h = _matrix(gpu, rows, 8, dt, 14)
    plain, fused, scalar = gpu.empty((rows,), NAME[dt]), gpu.empty((rows,), NAME[dt]), gpu.empty((1,))
    _axis(lib, d, ws, x, limit, 8, 1, 0, plain)
    want = _reduce(lib, d, ws, SUM, dt, plain.ptr, 0, limit, scalar)
    for _ in range(2):
        _native.check(_tail_axis(lib, d, ws, x, limit, 8, 1, fused, SUM, fused.ptr, 0, limit, scalar), "bk_reduce_axis_tail")
        assert struct.pack("<d", scalar.numpy()[0]) == want
    assert _bits(fused.numpy()[:limit]) == _bits(plain.numpy()[:limit])
    _check_scalar(SUM, scalar.numpy()[0], plain.numpy()[:limit].astype(np.float64), None)
    assert _tail_axis(lib, d, ws, x, rows, 8, 1, fused, SUM, fused.ptr, 0, rows, scalar) == BAD_ARGUMENT
    # nor a tail over part of the output, or over another buffer
    assert _tail_axis(lib, d, ws, x, limit, 8, 1, fused, SUM, fused.ptr, 0, limit - 1, scalar) == BAD_ARGUMENT
    assert _tail_axis(lib, d, ws, x, limit, 8, 1, fused, SUM, plain.ptr, 0, limit, scalar) == BAD_ARGUMENT


def test_closing_max_propagates_nan_like_bk_reduce(gpu, ws):
    d, lib = _driver(), _native.lib()
    h = np.random.default_rng(15).uniform(-1, 1, (67, 37))
    h[5, 7] = np.nan
    x = gpu.asarray(h, "float32")
    plain, fused, scalar = gpu.empty((67,), "float32"), gpu.empty((67,), "float32"), gpu.empty((1,))
    _axis(lib, d, ws, x, 67, 37, 1, 0, plain)
    want = _reduce(lib, d, ws, MAX, F32, plain.ptr, 0, 67, scalar)
    _native.check(_tail_axis(lib, d, ws, x, 67, 37, 1, fused, MAX, fused.ptr, 0, 67, scalar), "bk_reduce_axis_tail")
    assert struct.pack("<d", scalar.numpy()[0]) == want and np.isnan(scalar.numpy()[0])


@pytest.mark.parametrize("top", [MAX_ABS_DIFF, SUM, MAX, DOT])
@pytest.mark.parametrize("odt", [F32, BF16])
@pytest.mark.parametrize("M,K,N", [(260, 64, 1), (1030, 512, 3)])
def test_skinny_product_with_closing_reduce(gpu, ws, M, K, N, odt, top):
    d, lib = _driver(), _native.lib()
    A, _ = _matrix(gpu, M, K, BF16, 16)
    Bt, _ = _matrix(gpu, N, K, BF16, 17)
    n = M * N
    plain, fused, scalar = gpu.empty((n,), NAME[odt]), gpu.empty((n,), NAME[odt]), gpu.empty((1,))
    other = gpu.asarray(np.random.default_rng(18).uniform(-4, 4, n), NAME[odt])
    two = top in (DOT, MAX_ABS_DIFF)
    assert lib.bk_gemm_bf16_pick(_vp(A.ptr), _vp(Bt.ptr), _vp(plain.ptr), M, N, K, K, K, N, odt) == 8  # the skinny kernel
    _native.check(lib.bk_gemm_bf16_tn(_vp(A.ptr), _vp(Bt.ptr), _vp(plain.ptr), M, N, K, K, K, N, 1.0, 0.0, odt, d.stream),
                  "bk_gemm_bf16_tn")
    for swapped in ([False, True] if two else [False]):
        pa, pb = (other.ptr, plain.ptr) if swapped else (plain.ptr, other.ptr if two else 0)
        fa, fb = (other.ptr, fused.ptr) if swapped else (fused.ptr, other.ptr if two else 0)
        want = _reduce(lib, d, ws, top, odt, pa, pb, n, scalar)
        for _ in range(2):
            d.fill(fused.ptr, n * (2 if odt == BF16 else 4), 0xA5, 1)
            _native.check(lib.bk_gemm_bf16_tn_tail(_vp(A.ptr), _vp(Bt.ptr), _vp(fused.ptr), M, N, K, K, K, N, 1.0, 0.0, odt, top,
                                                   _vp(fa), _vp(fb) if fb else None, n, _vp(ws[WS_REDUCE]), _vp(scalar.ptr),
                                                   d.stream), "bk_gemm_bf16_tn_tail")
            got = scalar.numpy()[0]
            assert struct.pack("<d", got) == want
            assert _bits(fused.numpy()) == _bits(plain.numpy())
        a64, b64 = plain.numpy().astype(np.float64), other.numpy().astype(np.float64)
        _check_scalar(top, got, *((b64, a64) if swapped else (a64, b64)))
    # products the skinny kernel does not take, or that read C, have no tail
    tail = (top, _vp(fused.ptr), _vp(other.ptr) if two else None, n, _vp(ws[WS_REDUCE]), _vp(scalar.ptr), d.stream)
    assert lib.bk_gemm_bf16_tn_tail(_vp(A.ptr), _vp(Bt.ptr), _vp(fused.ptr), M, N, K, K, K, N, 1.0, 0.5, odt, *tail) == BAD_ARGUMENT
    assert lib.bk_gemm_bf16_tn_tail(_vp(A.ptr), _vp(Bt.ptr), _vp(fused.ptr), M, N, K, K, K, N + 1, 1.0, 0.0, odt,
                                    *tail) == BAD_ARGUMENT

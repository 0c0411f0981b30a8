"""The ticketed scratch workspaces (bk_workspace_bytes / bk_workspace_init of
csrc/kernels/beekern.h) on the MI355X, native driver.

Production hands a workspace out of the caching allocator, so a fresh one holds
whatever its last owner left.  Every kind is therefore allocated at exactly
bk_workspace_bytes(kind), filled with the byte 0xA5, initialised, and its op
run twice in a row on it through the ``_native`` entry point: the second run
shows that the first re-armed the tickets and left the tables as it found
them.  Both results are compared with numpy on the host under the tolerances
of the op's own test (test_kernels_gpu.py, test_masks_gpu.py,
test_stats_gpu.py, test_axis_gpu.py): sums to 1e-10 of sum |x| (1e-9 along an
axis), variances to rtol 1e-9, everything else exactly.

Shapes: the smallest at which more than one block takes a ticket."""

import ctypes

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops import _native
from bee_code_interpreter_fs_amd.ops.array import driver as _driver  # (ops.driver is the submodule)

pytestmark = pytest.mark.gpu

# enum BkWorkspace of csrc/kernels/beekern.h
REDUCE, REDUCE_AXIS, AXIS_STAT, COMPRESS, SELECT, HISTOGRAM = range(6)
N = 100003
ROWS, COLS = 4099, 67
_vp = ctypes.c_void_p


@pytest.fixture
def fresh_workspace(gpu):
    """kind -> a workspace of that kind made from a dirty block; freed after the test."""
    d, lib, made = _driver(), _native.lib(), []

    def make(kind):
        nbytes = lib.bk_workspace_bytes(kind)
        assert nbytes > 0
        ws = d.malloc(nbytes)
        made.append(ws)
        d.fill(ws, nbytes, 0xA5, 1)
        _native.check(lib.bk_workspace_init(kind, _vp(ws), d.stream), "bk_workspace_init")
        return ws

    yield make
    d.sync()
    for ws in made:
        d.free(ws)


def twice(run):
    return run(), run()


def test_reduce(gpu, fresh_workspace):
    d, lib = _driver(), _native.lib()
    h = np.random.default_rng(1).uniform(-1, 1, N)
    x, out = gpu.asarray(h), gpu.empty((1,))
    ws = fresh_workspace(REDUCE)

    def run():
        _native.check(lib.bk_reduce(0, x.code, _vp(x.ptr), None, N, _vp(ws), _vp(out.ptr), d.stream), "bk_reduce")
        return float(out.numpy()[0])

    for got in twice(run):
        assert abs(got - h.sum()) <= 1e-10 * np.abs(h).sum()


def test_compress(gpu, fresh_workspace):
    d, lib = _driver(), _native.lib()
    rng = np.random.default_rng(2)
    h, hm = rng.standard_normal(N).astype(np.float32), rng.random(N) < 0.5
    x, m = gpu.asarray(h, "float32"), gpu.asarray(hm, dtype="bool")
    count = int(hm.sum())
    ws = fresh_workspace(COMPRESS)

    def run():
        out = gpu.full((count,), -7.0, "float32")
        _native.check(lib.bk_compress(x.code, _vp(x.ptr), _vp(m.ptr), N, _vp(out.ptr), count, _vp(ws), d.stream),
                      "bk_compress")
        return out.numpy()

    for got in twice(run):
        np.testing.assert_array_equal(got.view(np.uint32), h[hm].view(np.uint32))


def test_select(gpu, fresh_workspace):
    d, lib = _driver(), _native.lib()
    h = np.random.default_rng(3).standard_normal(N).astype(np.float32)
    x, out = gpu.asarray(h, "float32"), gpu.empty((5,))
    ranks = [0, (N - 1) // 2, N // 2, N - 1]
    karr = (ctypes.c_int64 * len(ranks))(*ranks)
    ws = fresh_workspace(SELECT)

    def run():
        _native.check(lib.bk_select(x.code, _vp(x.ptr), N, karr, len(ranks), _vp(out.ptr), _vp(ws), d.stream),
                      "bk_select")
        return out.numpy()

    for got in twice(run):
        np.testing.assert_array_equal(got[:4], np.sort(h)[ranks].astype(np.float64))
        assert got[4] == 0  # no NaNs


def test_histogram(gpu, fresh_workspace):
    d, lib = _driver(), _native.lib()
    h = np.random.default_rng(4).standard_normal(N)
    want, edges = np.histogram(h, bins=50)
    x, e = gpu.asarray(h), gpu.asarray(edges)
    counts = d.malloc(50 * 8)
    ws = fresh_workspace(HISTOGRAM)

    def run():
        _native.check(lib.bk_histogram(x.code, _vp(x.ptr), N, _vp(e.ptr), 50, _vp(counts), _vp(ws), d.stream),
                      "bk_histogram")
        got = np.zeros(50, np.uint64)
        d.d2h(counts, got)
        return got

    try:
        for got in twice(run):
            np.testing.assert_array_equal(got.astype(np.int64), want)
    finally:
        d.free(counts)


@pytest.mark.parametrize("axis", [0, 1])
def test_reduce_axis(gpu, fresh_workspace, axis):
    d, lib = _driver(), _native.lib()
    h = np.random.default_rng(5).uniform(-1, 1, (ROWS, COLS))
    x, out = gpu.asarray(h), gpu.empty((h.shape[1 - axis],))
    ws = fresh_workspace(REDUCE_AXIS)

    def run():
        _native.check(lib.bk_reduce_axis(0, x.code, _vp(x.ptr), ROWS, COLS, COLS, axis, _vp(out.ptr), _vp(ws), d.stream),
                      "bk_reduce_axis")
        return out.numpy()

    for got in twice(run):
        np.testing.assert_allclose(got, h.sum(axis=axis), rtol=1e-9, atol=1e-9 * h.shape[axis])


@pytest.mark.parametrize("axis", [0, 1])
def test_axis_stat(gpu, fresh_workspace, axis):
    d, lib = _driver(), _native.lib()
    h = np.random.default_rng(6).uniform(-1, 1, (ROWS, COLS))
    x, out = gpu.asarray(h), gpu.empty((h.shape[1 - axis],))
    ws = fresh_workspace(AXIS_STAT)

    def run():
        _native.check(lib.bk_axis_stat(2, x.code, _vp(x.ptr), ROWS, COLS, COLS, axis, float(h.shape[axis] - 1),
                                       _vp(out.ptr), _vp(ws), d.stream), "bk_axis_stat")
        return out.numpy()

    for got in twice(run):
        np.testing.assert_allclose(got, h.var(axis=axis, ddof=1), rtol=1e-9, atol=0)

"""The sort family (csrc/kernels/sort.hip) on the GPU, native driver: bk_sort,
bk_arg_reduce and bk_take against tests/sort_ref.py and numpy on the host.

``index_out`` is compared with exact equality against the reference order (and
the reference against ``np.argsort(kind="stable")``), ``sorted_out`` with
``assert_array_equal`` against ``np.sort``.  Sizes sit around the kernels' own
constants, read from sort.hip.  CPU twins: test_sort_cpu.py,
test_broker_sort_cpu.py.
"""

import ctypes
import os
import re
import tempfile

import numpy as np
import pytest

from . import sort_ref as R
from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = ctypes.c_void_p
NAMES = ["f32", "f64", "bf16", "i64"]


def _constant(path, name):
    text = open(os.path.join(ROOT, "csrc", "kernels", path)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


T = _constant("sort.hip", "kSortTile")
B = _constant("sort.hip", "kSortMaxBlocks")
ARG_BLOCKS = _constant("sort.hip", "kArgMaxBlocks")
ARG_VECS = _constant("sort.hip", "kArgVecsPerLane")
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, B * T + T + 1]
MAX_SORT_N = 0x7FFFFFFF


def data(name, n, seed=0, few=False):
    """n elements of the dtype: random over a wide range (few: four distinct values, so most elements tie)."""
    rng = np.random.Generator(np.random.PCG64(77 + seed + n))
    if name == "i64":
        return (rng.integers(-2, 2, n, dtype=np.int64) if few
                else rng.integers(R.I64_MIN, R.I64_MAX, n, dtype=np.int64, endpoint=True))
    v = rng.integers(-2, 2, n).astype(np.float64) if few else rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
    if name == "bf16":
        return R.bf16_bits(v)
    return v.astype(R.NP_DTYPES[name])


def edge_values(name):
    if name == "i64":
        return np.array([R.I64_MIN, -1, 0, R.I64_MAX, R.I64_MIN + 1, R.I64_MAX - 1, 1], np.int64)
    if name == "f64":
        return np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, np.finfo(np.float64).max,
                         -np.finfo(np.float64).max, 1.0, -1.0]
                        ).astype(np.float64).view(np.uint64).tolist() + [0x7FF8000000000000, 0xFFF8000000000001,
                                                                         0x7FF0000000000001]
    if name == "f32":
        return np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1e-38, np.finfo(np.float32).max,
                         -np.finfo(np.float32).max, 1.0, -1.0], np.float32).view(np.uint32).tolist() + [0x7FC00000, 0xFFC00001,
                                                                                                    0x7F800001]
    return [0x0000, 0x8000, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x0080, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80, 0x7FC0, 0xFFC1, 0x7F81]


def with_edges(name, n, seed=0):
    """Random data with the dtype's edge values tiled in, value k every 37 + k elements."""
    a = data(name, n, seed)
    ev = edge_values(name)
    if name == "i64":
        for k, v in enumerate(ev):
            a[k::37 + k] = v
        return a
    bits = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    for k, v in enumerate(ev):
        bits[k::37 + k] = v
    return a


class Dev:
    """A host array in device memory behind `lead` elements of padding and ahead of 3 more: 16-byte aligned
    (lead 0) or one element off."""

    def __init__(self, gpu, host, lead=0):
        from bee_code_interpreter_fs_amd.ops.array import driver

        self.host = np.ascontiguousarray(host)
        self.lead, self.n, self.item = lead, self.host.size, self.host.dtype.itemsize
        self.fence = np.frombuffer(b"\xa5" * self.item, self.host.dtype)[0]
        padded = np.concatenate([np.full(lead, self.fence, self.host.dtype), self.host,
                                 np.full(3, self.fence, self.host.dtype)])
        self.arr = gpu.empty((padded.nbytes + 1) // 2, "bfloat16")  # raw bytes
        assert self.arr.ptr % 16 == 0
        self.d = driver()
        self.d.h2d(self.arr.ptr, padded)
        self.ptr = self.arr.ptr + lead * self.item

    def read(self):
        out = np.empty(self.lead + self.n + 3, self.host.dtype)
        self.d.d2h(self.arr.ptr, out)
        raw = out.view(np.uint8).reshape(-1, self.item)
        fence = np.frombuffer(self.fence.tobytes(), np.uint8)
        assert (raw[:self.lead] == fence).all() and (raw[self.lead + self.n:] == fence).all(), "wrote out of bounds"
        return out[self.lead:self.lead + self.n]


class Scratch:
    def __init__(self, gpu, nbytes):
        self.arr = gpu.empty(max(nbytes, 2) // 2 + 1, "bfloat16")
        self.ptr, self.nbytes = self.arr.ptr, nbytes


def gpu_sort(gpu, a, name, lead=0, want_sorted=True, want_index=True, ws=None):
    """(sorted or None, index or None, x read back) of one bk_sort call."""
    from bee_code_interpreter_fs_amd.ops import driver as drv

    n = a.size
    x = Dev(gpu, a, lead)
    s = Dev(gpu, np.zeros(n, a.dtype), lead) if want_sorted else None
    i = Dev(gpu, np.zeros(n, np.int64), lead) if want_index else None
    ws = ws or Scratch(gpu, drv.sort_workspace_bytes(R.DTYPES[name], n, want_index))
    x.d.sort(R.DTYPES[name], x.ptr, n, s.ptr if s else 0, i.ptr if i else 0, ws.ptr)
    return (s.read() if s else None), (i.read() if i else None), x.read()


def check_sort(gpu, a, name, lead=0, msg=""):
    got_sorted, got_index, x_after = gpu_sort(gpu, a, name, lead)
    want = R.argsort(a, name)
    np.testing.assert_array_equal(want, np.argsort(R.as_values(a, name), kind="stable"), err_msg="the reference order")
    assert np.array_equal(got_index, want), f"{name} {msg} n {a.size}: index_out"
    np.testing.assert_array_equal(R.as_values(got_sorted, name), np.sort(R.as_values(a, name)),
                                  err_msg=f"{name} {msg} n {a.size}: sorted_out")
    assert x_after.tobytes() == np.ascontiguousarray(a).tobytes(), "x was written"


# ---- bk_sort --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("name", NAMES)
def test_sort_at_every_size(gpu, name, lead):
    """Around a wave, a tile, and past the block cap, where blocks own several tiles, unevenly."""
    for n in SIZES:
        check_sort(gpu, data(name, n, few=n % 2 == 1 and n < 3 * T), name, lead, "sizes")


@pytest.mark.parametrize("name", NAMES)
def test_every_pass_reads_its_own_byte(gpu, name):
    """For every pass p: data whose keys differ only in byte p -- all 256 digit values, shuffled, repeated past
    one tile (among the floats a few such keys belong to NaN bit patterns, which all share the last key)."""
    size = R.NP_DTYPES[name]().itemsize
    U = {2: np.uint16, 4: np.uint32, 8: np.uint64}[size]
    n = T + 256 + 17
    rng = np.random.Generator(np.random.PCG64(5))
    sign = 1 << (8 * size - 1)
    for p in range(size):
        digits = np.resize(np.arange(256, dtype=np.uint64), n)
        rng.shuffle(digits)
        rest = 0x3C3C3C3C3C3C3C3C & ((1 << 8 * size) - 1) & ~(0xFF << (8 * p))
        key = (digits << np.uint64(8 * p)) | np.uint64(rest)
        # the element whose key this is: the key transform inverted
        if name == "i64":
            a = (key ^ np.uint64(sign)).view(np.int64)
        else:
            bits = np.where(key & np.uint64(sign) != 0, key ^ np.uint64(sign), ~key & np.uint64((1 << 8 * size) - 1))
            a = bits.astype(U).view(R.NP_DTYPES[name])
        got = R.keys(a, name).astype(np.uint64)
        assert (got == key).mean() > 0.9 and len(np.unique(got >> np.uint64(8 * p) & np.uint64(0xFF))) >= 250
        check_sort(gpu, a, name, 0, f"byte {p}")


@pytest.mark.parametrize("name", NAMES)
def test_ties_keep_index_order(gpu, name):
    n = 3 * T + 5
    mk = (lambda v: np.asarray(v, np.int64)) if name == "i64" else (
        (lambda v: R.bf16_bits(v)) if name == "bf16" else (lambda v: np.asarray(v, R.NP_DTYPES[name])))
    rng = np.random.Generator(np.random.PCG64(9))
    check_sort(gpu, mk(rng.integers(0, 3, n) - 1), name, 0, "three values")
    check_sort(gpu, mk(np.full(n, 7)), name, 0, "all equal")
    ramp = np.arange(n) // 5 - n // 10  # runs of five equal values, ascending
    check_sort(gpu, mk(ramp), name, 0, "sorted")
    check_sort(gpu, mk(ramp[::-1]), name, 0, "reversed")


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("name", NAMES)
def test_edge_values(gpu, name, lead):
    """+-0.0 tie, +-inf, NaNs of both signs last (in index order), denormals, the largest finite values;
    INT64_MIN, -1, 0, INT64_MAX."""
    check_sort(gpu, with_edges(name, 2 * T + 77), name, lead, "edges")


@pytest.mark.parametrize("name", NAMES)
def test_outputs_alone_and_together_and_a_shared_scratch(gpu, name):
    from bee_code_interpreter_fs_amd.ops import driver as drv

    a, b = with_edges(name, T + 300, 1), data(name, 3 * T + 1, 2, few=True)
    both_s, both_i, _ = gpu_sort(gpu, a, name)
    only_s, none_i, _ = gpu_sort(gpu, a, name, want_index=False)
    none_s, only_i, _ = gpu_sort(gpu, a, name, want_sorted=False)
    assert none_i is None and none_s is None
    assert both_s.tobytes() == only_s.tobytes() and np.array_equal(both_i, only_i)
    assert np.array_equal(both_i, R.argsort(a, name))
    # two different sorts back to back on the stream, one scratch: nothing is read between them
    ws = Scratch(gpu, max(drv.sort_workspace_bytes(R.DTYPES[name], v.size, True) for v in (a, b)))
    xa, xb = Dev(gpu, a), Dev(gpu, b)
    ia, sb, ib = Dev(gpu, np.zeros(a.size, np.int64)), Dev(gpu, np.zeros(b.size, b.dtype)), Dev(gpu, np.zeros(b.size, np.int64))
    xa.d.sort(R.DTYPES[name], xa.ptr, a.size, 0, ia.ptr, ws.ptr)
    xa.d.sort(R.DTYPES[name], xb.ptr, b.size, sb.ptr, ib.ptr, ws.ptr)
    assert np.array_equal(ia.read(), R.argsort(a, name)) and np.array_equal(ib.read(), R.argsort(b, name))
    np.testing.assert_array_equal(R.as_values(sb.read(), name), np.sort(R.as_values(b, name)))


@pytest.mark.parametrize("name", ["f32", "f64", "bf16"])
def test_sort_agrees_with_select(gpu, name):
    a = with_edges(name, 2 * T + 9, 3)
    got_sorted, _, _ = gpu_sort(gpu, a, name, want_index=False)
    x = Dev(gpu, a)
    ranks = [0, 1, T - 1, T, a.size // 2, a.size - 1]
    vals, nans = x.d.select(R.DTYPES[name], x.ptr, a.size, ranks)
    np.testing.assert_array_equal(R.as_values(got_sorted, name)[ranks].astype(np.float64), np.array(vals))
    assert nans == int(np.isnan(R.as_values(a, name)).sum())


# ---- bk_arg_reduce ----------------------------------------------------------------------------------------

def _plain(name, n, rng):
    """Values strictly inside (-100, 100), no NaN: an extremum can be planted outside."""
    v = rng.integers(-99, 100, n)
    return v.astype(np.int64) if name == "i64" else (R.bf16_bits(v) if name == "bf16" else v.astype(R.NP_DTYPES[name]))


def _put(name, a, at, value):
    a[at] = R.bf16_bits([value])[0] if name == "bf16" else value


@pytest.mark.parametrize("name", NAMES)
def test_arg_reduce_finds_the_first_extremum(gpu, name):
    vec = 16 // R.NP_DTYPES[name]().itemsize
    span = 256 * ARG_VECS * vec  # the elements of one block before the grid grows
    rng = np.random.Generator(np.random.PCG64(11))
    for n in (1, 2, 65, span - 1, span, span + 1, 2 * span + 3, ARG_BLOCKS * span + span + 5):
        places = sorted({0, n - 1, min(span - 1, n - 1), min(span, n - 1), n // 2})
        for lead in (0, 1):
            for op, big in ((0, 1000.0), (1, -1000.0)):
                for at in places:
                    a = _plain(name, n, rng)
                    _put(name, a, at, big)
                    dup = min(at + span + 1, n - 1)
                    _put(name, a, dup, big)  # a later duplicate: the first occurrence wins
                    x = Dev(gpu, a, lead)
                    got = x.d.arg_reduce(op, R.DTYPES[name], x.ptr, n)
                    vals = R.as_values(a, name)
                    want = int(np.argmax(vals) if op == 0 else np.argmin(vals))
                    assert want == (R.argmax if op == 0 else R.argmin)(a, name) == at
                    assert got == want, f"{name} op {op} n {n} at {at} lead {lead}"
            if n > 3 * span:
                break  # (one alignment at the largest size)


@pytest.mark.parametrize("name", ["f32", "f64", "bf16"])
def test_arg_reduce_returns_the_first_nan(gpu, name):
    """A NaN first, last, and two of them (the second negative): both ops return the first one's index."""
    n = 3 * 256 * ARG_VECS * (16 // R.NP_DTYPES[name]().itemsize) + 7
    rng = np.random.Generator(np.random.PCG64(12))
    for places in ([0], [n - 1], [n // 3, n - 2], [5, 4]):
        a = _plain(name, n, rng)
        _put(name, a, 1, np.inf)
        _put(name, a, 2, -np.inf)
        for at in places:
            _put(name, a, at, np.nan)
        if len(places) > 1:
            a.view(np.uint8).reshape(n, -1)[places[1], -1] |= 0x80  # the sign bit (little endian)
        vals = R.as_values(a, name)
        assert np.isnan(vals).sum() == len(places)
        x = Dev(gpu, a)
        for op in (0, 1):
            want = int(np.argmax(vals) if op == 0 else np.argmin(vals))
            assert want == min(places) == (R.argmax if op == 0 else R.argmin)(a, name)
            assert x.d.arg_reduce(op, R.DTYPES[name], x.ptr, n) == want, (name, op, places)


@pytest.mark.parametrize("name", NAMES)
def test_arg_reduce_on_edge_values(gpu, name):
    a = with_edges(name, 5003, 4)
    if name != "i64":  # without the NaNs: +-0.0 tie, the infinities win
        vals = R.as_values(a, name)
        a = a[~np.isnan(vals)]
    x = Dev(gpu, a, 1)
    vals = R.as_values(a, name)
    assert x.d.arg_reduce(0, R.DTYPES[name], x.ptr, a.size) == int(np.argmax(vals)) == R.argmax(a, name)
    assert x.d.arg_reduce(1, R.DTYPES[name], x.ptr, a.size) == int(np.argmin(vals)) == R.argmin(a, name)
    zeros = a.copy()
    zeros[:] = 0
    if name != "i64":
        zeros.view(np.uint8)[-1] = 0x80  # -0.0 last: still index 0 for both
    z = Dev(gpu, zeros)
    assert z.d.arg_reduce(0, R.DTYPES[name], z.ptr, zeros.size) == 0 == z.d.arg_reduce(1, R.DTYPES[name], z.ptr, zeros.size)


# ---- bk_take ---------------------------------------------------------------------------------------------

TAKE_TYPES = [("f32", 0, np.float32), ("f64", 1, np.float64), ("bf16", 2, np.uint16), ("bool", 6, np.uint8),
              ("i64", 5, np.int64)]


@pytest.mark.parametrize("case", TAKE_TYPES, ids=[c[0] for c in TAKE_TYPES])
def test_take_gathers_and_counts_bad_indices(gpu, case):
    _, dt, npdt = case
    rng = np.random.Generator(np.random.PCG64(13))
    n = 1000
    xh = rng.integers(1, 2 if dt == 6 else 250, n).astype(npdt)  # (never zero: a zeroed element shows)
    if dt == 6:
        xh[::3] = 0
    indices = {
        "identity": np.arange(n), "reversed": np.arange(n)[::-1], "all same": np.full(300, 17),
        "negative": -1 - np.arange(n), "random with repeats": rng.integers(-n, n, 4 * n + 3),
        "one": np.array([n - 1]), "a tile": rng.integers(0, n, 256), "a tile and one": rng.integers(0, n, 257),
        "none": np.zeros(0, np.int64),
    }
    for lead in (0, 1):
        x = Dev(gpu, xh, lead)
        for what, ih in indices.items():
            ih = ih.astype(np.int64)
            idx, out = Dev(gpu, ih, lead), Dev(gpu, np.full(ih.size, 0x5A, np.uint8).repeat(npdt().itemsize).view(npdt), lead)
            bad = x.d.take(dt, x.ptr, n, idx.ptr, ih.size, out.ptr)
            want, want_bad = R.take(xh, ih)
            assert bad == want_bad == 0, what
            assert out.read().tobytes() == want.tobytes() == xh[ih].tobytes(), what
        ih = rng.integers(-n, n, 2 * n + 1).astype(np.int64)
        ih[[0, 5, 77, 1500, 2 * n]] = [n, -n - 1, R.I64_MIN, R.I64_MAX, n + 1]
        idx, out = Dev(gpu, ih, lead), Dev(gpu, np.full(ih.size, 0x5A, np.uint8).repeat(npdt().itemsize).view(npdt), lead)
        want, want_bad = R.take(xh, ih)
        assert x.d.take(dt, x.ptr, n, idx.ptr, ih.size, out.ptr) == want_bad == 5
        got = out.read()
        assert got.tobytes() == want.tobytes() and not got[[0, 5, 77, 1500, 2 * n]].any()


# ---- arguments ----------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(gpu):
    from bee_code_interpreter_fs_amd.ops import driver as drv

    a = data("f32", 100)
    x, s, i = Dev(gpu, a), Dev(gpu, np.zeros(100, np.float32)), Dev(gpu, np.zeros(100, np.int64))
    d, lib = x.d, x.d.lib
    need = lib.bk_sort_workspace_bytes(0, 100, 1)
    assert need == drv.sort_workspace_bytes(0, 100, True) > 0
    for dt in (0, 1, 2, 5):
        for n in (0, 1, 4097, 10 ** 8, MAX_SORT_N):
            for wi in (0, 1):
                assert lib.bk_sort_workspace_bytes(dt, n, wi) == drv.sort_workspace_bytes(dt, n, bool(wi)) > 0
    assert [lib.bk_sort_workspace_bytes(dt, n, 1) for dt, n in ((3, 10), (4, 10), (6, 10), (7, 10), (-1, 10), (0, -1),
                                                                 (0, MAX_SORT_N + 1))] == [0] * 7
    ws = Scratch(gpu, need)
    st = d.stream

    def sort(dt=0, xp=x.ptr, n=100, sp=s.ptr, ip=i.ptr, wp=ws.ptr, wb=need):
        return lib.bk_sort(dt, _vp(xp) if xp else None, n, _vp(sp) if sp else None, _vp(ip) if ip else None,
                           _vp(wp) if wp else None, wb, st)

    assert sort() == 0
    assert sort(n=0, xp=0, wp=0, wb=0) == 0  # nothing to do, nothing launched
    for rc in (sort(dt=3), sort(dt=4), sort(dt=6), sort(dt=9), sort(dt=-1), sort(n=-1), sort(n=MAX_SORT_N + 1),
               sort(xp=0), sort(sp=0, ip=0), sort(wp=0), sort(wb=need - 1), sort(wb=0), sort(xp=x.ptr + 2),
               sort(wp=ws.ptr + 8, wb=need), sort(ip=i.ptr + 4)):
        assert rc == 1
    wsr = d.workspaces[drv.WS_REDUCE]

    def arg(op=0, dt=0, xp=x.ptr, n=100, wp=wsr, op_=d.scalar):
        return lib.bk_arg_reduce(op, dt, _vp(xp) if xp else None, n, _vp(wp) if wp else None, _vp(op_) if op_ else None, st)

    assert arg() == 0
    for rc in (arg(op=2), arg(op=-1), arg(dt=3), arg(dt=6), arg(dt=8), arg(xp=0), arg(n=0), arg(n=-5), arg(wp=0), arg(op_=0)):
        assert rc == 1
    idx, out = Dev(gpu, np.arange(100, dtype=np.int64)), Dev(gpu, np.zeros(100, np.float32))

    def take(dt=0, xp=x.ptr, n=100, ip=idx.ptr, m=100, op_=out.ptr, wp=wsr, bp=d.scalar):
        p = lambda v: _vp(v) if v else None  # noqa: E731
        return lib.bk_take(dt, p(xp), n, p(ip), m, p(op_), p(wp), p(bp), st)

    assert take() == 0
    for rc in (take(dt=3), take(dt=4), take(dt=7), take(xp=0), take(n=-1), take(ip=0), take(m=-1), take(op_=0), take(wp=0),
               take(bp=0)):
        assert rc == 1
    d.sync()
    # the refused calls wrote nothing and left the workspace ready
    assert d.arg_reduce(0, 0, x.ptr, 100) == int(np.argmax(a))
    assert np.array_equal(i.read(), R.argsort(a, "f32"))


# ---- the public API and the example, in a broker sandbox -----------------------------------------------------

def test_public_api_on_the_gpu(gpu):
    import bee_code_interpreter_fs_amd.ops as bk

    rng = np.random.Generator(np.random.PCG64(21))
    h = rng.standard_normal(3 * T + 11)
    h[::97] = np.nan
    x = bk.array(h, dtype="float64")
    order = bk.argsort(x)
    assert order.dtype == "int64" and np.array_equal(order.numpy(), np.argsort(h, kind="stable"))
    np.testing.assert_array_equal(bk.sort(x).numpy(), np.sort(h))
    np.testing.assert_array_equal(x[order].numpy(), np.sort(h))
    assert bk.argmax(x) == np.argmax(h) and bk.argmin(x) == np.argmin(h) and isinstance(bk.argmax(x), np.int64)
    np.testing.assert_array_equal(bk.take(x, [0, -1, 5]).numpy(), h[[0, -1, 5]])
    with pytest.raises(IndexError):
        bk.take(x, [h.size])
    d = bk.array(rng.integers(1, 7, 5000), dtype="int64")
    assert np.array_equal(bk.sort(d).numpy(), np.sort(d.numpy())) and d.argmax() == np.argmax(d.numpy())


@pytest.fixture(scope="module")
def dsvc():
    ensure_native_executor()
    h = ServiceHarness(tempfile.mkdtemp(prefix="bee-sort-"), gpu_ids=[0], workers_per_gpu_target=1, default_timeout=120.0)
    h.start()
    yield h
    h.stop()


CHECK_TOP_CLAIMS = """
import numpy as _np
_s, _r = severity.numpy(), region.numpy()
_o = _np.argsort(_s, kind="stable")
report(lambda *a: print("numpy", *a), [float(v) for v in _s[_o[-10:]][::-1]], [int(v) for v in _o[-10:][::-1]],
       int(_np.argmax(_s)), float(_s[_np.argmax(_s)]), [int(v) for v in _r[_o[-10:]][::-1]], float(_np.sort(_s)[len(_s) // 2]))
"""


def test_top_claims_in_a_broker_sandbox(dsvc):
    """examples/top_claims.py through the kernel broker.  The test appends a few lines that download the two
    draws and print numpy's figures for them in the example's format: the two printouts are equal."""
    src = open(os.path.join(ROOT, "examples", "top_claims.py")).read() + CHECK_TOP_CLAIMS
    r = dsvc.call(dsvc.ctx.code_executor.execute(source_code=src, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert "HostFallbackWarning" not in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    ours = [ln for ln in lines if not ln.startswith("numpy ")]
    theirs = [ln[len("numpy "):] for ln in lines if ln.startswith("numpy ")]
    assert len(ours) >= 5 and ours == theirs, r.stdout

"""The radix select and the histogram (csrc/kernels/stats.hip) on the MI355X,
native driver, against numpy on the downloaded operands: selected values equal
``np.sort(h)[k]`` exactly, NaN counts and histogram counts as integers, the
input unchanged bit for bit.  Then the same through the service: the
plain-numpy value-at-risk payload under the offload, and both new ops once in
a broker sandbox.  CPU twins: test_stats_cpu.py, test_broker_stats_cpu.py.

Interpolated percentiles are checked against
``np.percentile(h.astype(np.float64), q)``: both sides evaluate
``a + (b - a) g`` in f64 with a few roundings, so an f64 result may differ by
at most 2 ulp of max(|a|, |b|) (a plain f64 evaluation sat at most 1.0 ulp
from numpy on these sizes and kinds), and an f32 result is that value rounded
to f32, within 1 f32 ulp.  numpy on the f32 array itself is NOT the reference
for interpolated values: its f32 path rounds g to f32 and sat up to 19 f32 ulp
from its own f64 answer on the same inputs."""

import functools
import os
import statistics
import tempfile

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops import driver as drvmod
from bee_code_interpreter_fs_amd.ops.array import driver as _driver  # (ops.driver is the submodule)

from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float64", "float32", "bfloat16"]
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
# one block's tile: 4 x 256 16-byte vectors (kUnroll x kBlock of stats.hip), in elements
TILE = {"float64": 2048, "float32": 4096, "bfloat16": 8192}
# below, at and above a wave and a block; around the tile (per dtype, added
# below); more than one block with a ragged tail
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, (1 << 20) + 3]
KINDS = ["uniform", "normal", "equal", "two", "ascending", "descending", "lowbits", "specials", "specials_nan"]
FINITE = KINDS[:7]
QS = [0, 0.1, 1, 5, 25, 33.3, 50, 75, 95, 99.9, 100]


def sizes_for(dtype):
    return SIZES[:-1] + [TILE[dtype] - 1, TILE[dtype] + 1, SIZES[-1]]


CASES = [(dt, n) for dt in DTYPES for n in sizes_for(dt)]


def _from_bits(bits, dtype):
    """Host values (f32 for bf16) from the dtype's bit patterns."""
    if dtype == "bfloat16":
        return (np.asarray(bits, np.uint32) << 16).view(np.float32)
    return np.asarray(bits, UINT[np.dtype(dtype).itemsize]).view(dtype)


def _to_dtype(h, dtype):
    """f64 values rounded into ``dtype`` (bf16: representable f32 values, by truncation)."""
    if dtype == "bfloat16":
        u = np.ascontiguousarray(h, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
        return u.view(np.float32)
    return h.astype(dtype)


def _specials(dtype):
    """+-0, +-inf, the smallest and largest denormals, the smallest normal and the extremes."""
    if dtype == "bfloat16":
        pos = [0x0000, 0x7F80, 0x0001, 0x007F, 0x0080, 0x7F7F]
        bits = pos + [b | 0x8000 for b in pos]
    elif dtype == "float32":
        pos = [0x00000000, 0x7F800000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF]
        bits = pos + [b | 0x80000000 for b in pos]
    else:
        pos = [0, 0x7FF0 << 48, 1, (1 << 52) - 1, 1 << 52, (0x7FF0 << 48) - 1]
        bits = pos + [b | (1 << 63) for b in pos]
    return _from_bits(bits, dtype)


def _nans(dtype):
    """Quiet and payload NaNs of both signs."""
    if dtype == "bfloat16":
        return _from_bits([0x7FC0, 0xFFC0, 0x7F81, 0xFFFF], dtype)
    if dtype == "float32":
        return _from_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype)
    return _from_bits([0x7FF8 << 48, 0xFFF8 << 48, (0x7FF0 << 48) + 1, (1 << 64) - 1], dtype)


@functools.lru_cache(maxsize=None)
def _host(dtype, n, kind):
    rng = np.random.default_rng(n % 9973 + 17 * KINDS.index(kind))
    if kind == "uniform":
        h = _to_dtype(rng.random(n), dtype)
    elif kind in ("normal", "specials", "specials_nan"):
        h = _to_dtype(rng.standard_normal(n), dtype).copy()
        tiled = {"normal": [], "specials": _specials(dtype),
                 "specials_nan": np.concatenate([_specials(dtype), _nans(dtype)])}[kind]
        for k, v in enumerate(tiled):  # (every 37 + k elements: every lane and vector position)
            h[k::37 + k] = v
    elif kind == "equal":
        h = _to_dtype(np.full(n, 0.3), dtype)
    elif kind == "two":
        h = _to_dtype(np.where(rng.random(n) < 0.4, -1.5, 2.25), dtype)
    elif kind in ("ascending", "descending"):
        h = _to_dtype(np.arange(n, dtype=np.float64) / 8 - 1000.0, dtype)
        h = h[::-1].copy() if kind == "descending" else h
    else:  # lowbits: only the lowest mantissa bits differ, so the last pass decides
        base = {"bfloat16": 0x3FC0, "float32": 0x3FC00000, "float64": 0x3FF8 << 48}[dtype]
        h = _from_bits(base + rng.integers(0, 64 if dtype == "bfloat16" else 256, n).astype(np.uint64), dtype)
    h = np.ascontiguousarray(h)
    h.setflags(write=False)
    return h


def _device_bits(d):
    raw = np.empty(d.size, UINT[d.itemsize])
    _driver().d2h(d._buf.ptr, raw)
    return raw


def _same(got, want):
    """==, with NaN equal to NaN (a selected NaN is some NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def _ranks(n, h, kind):
    ranks = [0, n - 1, (n - 1) // 2, n // 2]
    if kind == "two":  # the boundary between the two values
        below = int((h == h.min()).sum())
        ranks += [min(max(below - 1, 0), n - 1), min(below, n - 1)]
    return ranks


@pytest.mark.parametrize("dtype,n", CASES)
def test_select_matches_sort(gpu, dtype, n):
    for kind in KINDS:
        x = gpu.asarray(_host(dtype, n, kind), dtype)
        h = x.numpy()  # the downloaded operand (bf16: widened to f32)
        before = _device_bits(x)
        s = np.sort(h).astype(np.float64)
        nan_count = int(np.isnan(h).sum())
        ranks = _ranks(n, h, kind)
        values, nans = _driver().select(x.code, x._buf.ptr, n, ranks)
        assert nans == nan_count, (kind, nans, nan_count)
        assert _same(values, s[ranks]), (kind, ranks, values, s[ranks])
        # 32 ranks at once, with duplicates, in no order
        many = [int(k) for k in np.random.default_rng(n).integers(0, n, 24)] + ranks[:4] + [ranks[0]] * 4
        values, nans = _driver().select(x.code, x._buf.ptr, n, many)
        assert len(values) == 32 and nans == nan_count
        assert _same(values, s[many]), (kind, many, values, s[many])
        # the median is numpy's, exactly (bf16: beekern's own function, numpy's f32 arithmetic)
        with np.errstate(all="ignore"):
            want = np.median(h)
        got = gpu.median(x) if dtype == "bfloat16" else np.median(x)
        assert type(got) is type(want) and _same(got, want), (kind, got, want)
        np.testing.assert_array_equal(_device_bits(x), before)  # x is only read


@pytest.mark.parametrize("dtype,n", [c for c in CASES if c[0] != "bfloat16"])
def test_percentiles_within_the_interpolation_bound(gpu, dtype, n):
    for kind in FINITE:
        x = gpu.asarray(_host(dtype, n, kind), dtype)
        h64 = x.numpy().astype(np.float64)
        s = np.sort(h64)
        ref = np.percentile(h64, QS)
        got = gpu.percentile(x, QS)  # f64, before any rounding to the dtype
        for q, g, r in zip(QS, got, ref):
            lo = int(np.floor((n - 1) * (q / 100)))
            scale = max(abs(s[lo]), abs(s[min(lo + 1, n - 1)]))
            if dtype == "float64":
                err = abs(g - r) / np.spacing(scale)
                print(f"{kind} n={n} q={q}: {err:.2f} f64 ulp")
                assert err <= 2.0, (kind, q, g, r)
            else:
                g32, r32 = np.float32(g), np.float32(r)
                err = abs(float(g32) - float(r32)) / float(np.spacing(np.float32(scale)))
                print(f"{kind} n={n} q={q}: {err:.2f} f32 ulp")
                assert err <= 1.0, (kind, q, g32, r32)
                assert np.percentile(x, q) == g32  # the protocol rounds that value once
        assert _same(np.percentile(x, QS), got)
    hn = _host(dtype, n, "specials_nan")
    if np.isnan(hn).any():  # (n = 1 holds the first special only)
        nan = gpu.asarray(hn, dtype)
        assert np.isnan(np.percentile(nan, 50)) and np.isnan(np.quantile(nan, [0.0, 1.0])).all()


def _garbage_counts():
    """Fill the native driver's count scratch, so stale contents would show."""
    d = _driver()
    d.fill(d._stats_scratch() + drvmod._STATS_COUNTS_AT, drvmod.MAX_BINS * 8, 0xA5A5A5A5DEADBEEF, 8)


HIST_SIZES = {dt: [1, 257, TILE[dt] + 1, (1 << 20) + 3] for dt in DTYPES}


@pytest.mark.parametrize("dtype,n", [(dt, n) for dt in DTYPES for n in HIST_SIZES[dt]])
def test_histogram_counts_are_numpys(gpu, dtype, n):
    hist = gpu.histogram if dtype == "bfloat16" else np.histogram  # (bf16 has no numpy protocol path)
    for kind in ("uniform", "normal", "equal", "lowbits", "specials", "specials_nan"):
        x = gpu.asarray(_host(dtype, n, kind), dtype)
        h = x.numpy()
        uneven = [-2.0, -1.5, -0.25, 0.0, 0.0, 0.3, 1.0, 1.5, 1.5000001, 64.0]
        cases = [dict(bins=50, range=(-3.0, 3.0)), dict(bins=4096, range=(-1.0, 1.0)), dict(bins=uneven),
                 dict(bins=7, range=(10.0, 20.0)),  # a range that excludes the data
                 dict(bins=1, range=(-0.5, 0.5)), dict(bins=2, range=(0.0, 2.0))]
        if kind in FINITE:  # the automatic range: min and max on the device
            cases += [dict(bins=b) for b in (1, 2, 50, 4096)]
        for kw in cases:
            _garbage_counts()
            try:
                wc, we = np.histogram(h, **kw)
            except ValueError:  # (4096 bins over a range a few ulps wide: numpy's error, ours too)
                with pytest.raises(ValueError, match="Too many bins"):
                    hist(x, **kw)
                continue
            c, e = hist(x, **kw)
            assert c.dtype == np.int64 and e.dtype == we.dtype
            np.testing.assert_array_equal(e, we, err_msg=f"{kind} {kw}")
            np.testing.assert_array_equal(c, wc, err_msg=f"{kind} {kw}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_histogram_elements_on_and_beside_every_edge(gpu, dtype):
    if dtype == "bfloat16":
        edges = np.arange(-6.0, 6.5, 0.25, dtype=np.float32)  # exact in bf16
        bits = (edges.view(np.uint32) >> 16).astype(np.int64)
        beside = [_from_bits(np.clip(bits + d, 0, 0xFFFF), dtype) for d in (-1, 1)]
    else:
        t = np.dtype(dtype).type
        edges = np.histogram_bin_edges(np.array([-1.0, 2.0], dtype), 50)
        beside = [np.nextafter(edges, t(-np.inf)), np.nextafter(edges, t(np.inf))]
    h = np.tile(np.concatenate([edges] + beside), 40)
    x = gpu.asarray(h, dtype)
    h = x.numpy()
    hist = gpu.histogram if dtype == "bfloat16" else np.histogram
    for kw in (dict(bins=edges), dict(bins=edges.size - 1, range=(float(edges[0]), float(edges[-1]))),
               dict(bins=edges[::3]), dict(bins=4096, range=(float(edges[0]), float(edges[-1])))):
        _garbage_counts()
        c, e = hist(x, **kw)
        wc, we = np.histogram(h, **kw)
        np.testing.assert_array_equal(e, we)
        np.testing.assert_array_equal(c, wc)
    assert np.histogram(h, bins=edges)[0].sum() == edges.size * 40 + 2 * (edges.size - 1) * 40  # (the case is not vacuous)


def test_transposed_view_and_density(gpu):
    h = np.random.default_rng(2).standard_normal((300, 41))
    x = gpu.asarray(h)
    assert np.median(x.T) == np.median(h) and np.percentile(x.T, 5) == np.percentile(h, 5)
    d, e = np.histogram(x.T, bins=20, density=True)
    wd, we = np.histogram(h, bins=20, density=True)
    np.testing.assert_array_equal(d, wd)
    np.testing.assert_array_equal(e, we)


# ---- through the service ---------------------------------------------------------------

@pytest.fixture(scope="module")
def ssvc():
    ensure_native_executor()
    h = ServiceHarness(tempfile.mkdtemp(prefix="bee-stats-"), gpu_ids=[0], workers_per_gpu_target=1,
                       default_timeout=120.0)
    h.start()
    yield h
    h.stop()


def test_monte_carlo_var_under_the_offload(ssvc):
    """Plain numpy, Execute(numpy_offload=True): percentiles, median and the
    histogram stay on the sandbox's GPU.  A sample quantile of n draws has
    standard error sqrt(p (1 - p) / n) / pdf(z_p): each printed quantile
    within 6 of those of the standard normal's (n = 2e6: 0.016, 0.0090 and
    0.0053 for p = 0.01, 0.05, 0.5)."""
    src = open(os.path.join(ROOT, "examples", "monte_carlo_var.py")).read()
    r = ssvc.call(ssvc.ctx.code_executor.execute(source_code=src, numpy_offload=True, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert "HostFallbackWarning" not in r.stderr, r.stderr
    nd, n = statistics.NormalDist(), 2e6
    bounds = []
    for label, p in (("VaR 1%:", 0.01), ("VaR 5%:", 0.05), ("Median:", 0.5)):
        z = nd.inv_cdf(p)
        bound = 6 * (p * (1 - p) / n) ** 0.5 / nd.pdf(z)
        bounds.append(bound)
        got = float(r.stdout.split(label)[1].split()[0])
        assert abs(got - z) < bound, (label, got, z, bound)
    assert bounds == pytest.approx([0.016, 0.0090, 0.0053], rel=0.03)
    lo, hi = (float(v) for v in r.stdout.split("Mode bin:")[1].split()[:2])
    assert lo < 0.5 and hi > -0.5, r.stdout  # the mode bin is next to 0


def test_select_and_histogram_in_a_broker_sandbox(ssvc):
    code = (
        "import beekern as bk, numpy as np\n"
        "n = 16385\n"
        "h = np.random.default_rng(3).standard_normal(n)\n"
        "h[::7] = 0.25\n"
        "x = bk.asarray(h)\n"
        "assert bk.driver_name() == 'broker'\n"
        "s = np.sort(h)\n"
        "ranks = [0, n - 1, n // 2, 4000, 4001] + list(range(100, 127))\n"
        "from bee_code_interpreter_fs_amd.ops.array import driver\n"
        "vals, nans = driver().select(x.code, x.ptr, n, ranks)\n"
        "assert nans == 0 and (np.array(vals) == s[ranks]).all()                    # SELECT\n"
        "assert bk.median(x) == np.median(h)\n"
        "assert (bk.percentile(x, [1, 5, 50]) == np.percentile(h, [1, 5, 50])).all()\n"
        "for kw in (dict(bins=50), dict(bins=4096), dict(bins=[-1.0, 0.25, 0.25, 3.0]), dict(bins=9, range=(0, 1))):\n"
        "    c, e = bk.histogram(x, **kw)                                           # HISTOGRAM\n"
        "    wc, we = np.histogram(h, **kw)\n"
        "    assert (c == wc).all() and (e == we).all() and c.dtype == np.int64\n"
        "h32 = h.astype(np.float32)\n"
        "assert bk.median(bk.asarray(h32, 'float32')) == np.median(h32)\n"
        "print('stats ok', bk.driver_name())\n"
    )
    r = ssvc.call(ssvc.ctx.code_executor.execute(source_code=code, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert r.stdout.split() == ["stats", "ok", "broker"], r.stdout

"""Kernel microbench on one MI355X: beekern vs torch (hipBLASLt / torch eager).

Prints one JSON line per kernel with device time (HIP events, median of
repeats) and the achieved HBM GB/s or TFLOP/s.  Random operands throughout
(zero-filled inputs read high on MI355X: cdna_hip_programming §5.4 rule 25).
"""

import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from bee_code_interpreter_fs_amd import ops as bk  # noqa: E402


def timed(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    bk.synchronize()
    times = []
    for _ in range(reps):
        with bk.Timer() as t:
            fn()
        times.append(t.ms)
    return statistics.median(times), min(times)


def torch_timed(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times), min(times)


def spread(fn, timer, reps=20, warmup=3):
    """median, min and max of `reps` timed calls (timer: timed / torch_timed's loop)."""
    for _ in range(warmup):
        fn()
    bk.synchronize()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if timer == "bk":
            with bk.Timer() as t:
                fn()
            times.append(t.ms)
        else:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e))
    return statistics.median(times), min(times), max(times)


def mask_rows():
    """The mask kernels (csrc/kernels/mask.hip) against torch eager, n = 1e8
    f64 random data: `python tools/bench_kernels.py masks`
    (profiles/mask_kernels.jsonl).  The fused compare-count reads the bytes
    bk.sum reads with the same stream shape: it is also set against bk.sum
    of the same array in the same run."""
    from bee_code_interpreter_fs_amd.ops.array import driver

    bk.init()
    emit(kernel="device", **bk.device_info())
    n = 10**8
    x = bk.random.rand(n)._materialize()
    y = bk.random.rand(n)._materialize()
    tx = torch.empty(n, dtype=torch.float64, device="cuda").uniform_()
    ty = torch.empty(n, dtype=torch.float64, device="cuda").uniform_()

    def row(kernel, fn, timer, nbytes, **kw):
        ms, mn, mx = spread(fn, timer)
        emit(kernel=kernel, n=n, ms=ms, min_ms=mn, max_ms=mx, GBps=nbytes / ms / 1e6, **kw)
        return ms, mn, mx

    row("compare_le f64 (array <= 0.5 -> mask)", lambda: bk.less_equal(x, 0.5)._materialize(), "bk", n * 9)
    row("torch.le f64", lambda: torch.le(tx, 0.5), "torch", n * 9)
    row("compare_le f64 (array <= array -> mask)", lambda: bk.less_equal(x, y)._materialize(), "bk", n * 17)
    row("torch.le f64 (array, array)", lambda: torch.le(tx, ty), "torch", n * 17)

    s_ms, s_mn, s_mx = row("sum_f64 (incl. 8B readback)", lambda: bk.sum(x), "bk", n * 8)
    c_ms, _, _ = row("compare_count f64 fused (x <= 0.5, incl. 8B readback)",
                     lambda: bk.count_nonzero(bk.less_equal(x, 0.5)), "bk", n * 8)
    emit(kernel="compare_count vs sum_f64", ratio=c_ms / s_ms, inside_sum_spread=bool(s_mn <= c_ms <= s_mx))
    # the same two at the driver: the timed span of the rows above starts
    # before the Python that builds the lazy mask, these hold the launch only
    drv = driver()
    s_ms, s_mn, s_mx = row("sum_f64 (driver call, incl. 8B readback)", lambda: drv.reduce(0, x.code, x.ptr, 0, n),
                           "bk", n * 8)
    c_ms, _, _ = row("compare_count f64 fused (driver call, incl. 8B readback)",
                     lambda: drv.compare_count(1, x.code, 1, x.ptr, 0, 0.5, n), "bk", n * 8)
    emit(kernel="compare_count vs sum_f64 (driver calls)", ratio=c_ms / s_ms,
         inside_sum_spread=bool(s_mn <= c_ms <= s_mx))
    row("torch.count_nonzero(tx <= 0.5) f64", lambda: torch.count_nonzero(tx <= 0.5).item(), "torch", n * 8)

    m = bk.less_equal(x, 0.5)._materialize()
    tm = tx <= 0.5
    row("where f64 (mask, array, array)", lambda: bk.where(m, x, y), "bk", n * 25)
    row("torch.where f64", lambda: torch.where(tm, tx, ty), "torch", n * 25)

    count = bk.count_nonzero(m)
    row("compress f64, 50% (x[mask]: count + 2 launches)", lambda: x[m], "bk", n * 10 + count * 8, density=count / n)
    out = bk.empty(count, "float64")
    row("compress f64, 50% (kernels only, count known)",
        lambda: drv.compress(x.code, x.ptr, m.ptr, n, out.ptr, count), "bk", n * 10 + count * 8)
    row("torch tx[tm] f64, 50%", lambda: tx[tm], "torch", n * 10 + count * 8)


def stats_rows():
    """The radix select and the histogram (csrc/kernels/stats.hip), n = 1e8 f64
    and f32, uniform / normal / all-equal data, each beside bk.sum of the same
    array (how many array reads it costs) and its torch counterpart on the same
    buffer: `python tools/bench_kernels.py stats` (profiles/stats_kernels.jsonl).
    A select reads the array once per byte of the dtype."""
    from bee_code_interpreter_fs_amd.ops.array import driver

    bk.init()
    emit(kernel="device", **bk.device_info())
    drv = driver()
    n = 10**8
    for dtype, esize in (("float64", 8), ("float32", 4)):
        for data in ("uniform", "normal", "equal"):
            if data == "uniform":
                x = bk.random.uniform(0.0, 1.0, n, dtype=dtype)._materialize()
            elif data == "normal":
                x = bk.random.normal(0.0, 1.0, n, dtype=dtype)._materialize()
            else:
                x = bk.full(n, 0.3, dtype)
            tx = bk.to_torch(x)
            tag = f"{dtype} {data}"

            def row(kernel, fn, timer, reads=1, reps=10, **kw):
                ms, mn, mx = spread(fn, timer, reps=reps, warmup=2)
                emit(kernel=f"{kernel} [{tag}]", n=n, ms=ms, min_ms=mn, max_ms=mx, GBps=reads * n * esize / ms / 1e6, **kw)
                return ms, mn, mx

            s_ms, s_mn, s_mx = row("sum (driver call, incl. 8B readback)", lambda: drv.reduce(0, x.code, x.ptr, 0, n), "bk")
            pair = [(n - 1) // 2, n // 2]
            ten = [int(q * (n - 1)) for q in (0.001, 0.01, 0.05, 0.25, 0.4, 0.5, 0.75, 0.95, 0.99, 0.999)]
            for name, ranks in (("select median pair", pair), ("select 10 ranks", ten)):
                ms, _, _ = row(f"{name} ({esize} passes, incl. readback)", lambda: drv.select(x.code, x.ptr, n, ranks),
                               "bk", reads=esize)
                emit(kernel=f"{name} vs passes x sum [{tag}]", sums=ms / s_ms, passes=esize,
                     within_passes_plus_spread=bool(ms <= esize * s_ms + (s_mx - s_mn)))
            ms, _, _ = row("np.percentile(x, [1, 5, 50, 95, 99]) end to end", lambda: np.percentile(x, [1, 5, 50, 95, 99]),
                           "bk", reads=esize)
            emit(kernel=f"percentile vs sum [{tag}]", sums=ms / s_ms)
            med_ms, _, _ = row("np.median(x) end to end", lambda: np.median(x), "bk", reads=esize)
            t_ms, _, _ = row("torch.median", lambda: torch.median(tx).item(), "torch", reps=5)
            emit(kernel=f"median vs torch.median [{tag}]", ratio=med_ms / t_ms)
            row("torch.kthvalue(n // 2)", lambda: torch.kthvalue(tx, n // 2).values.item(), "torch", reps=5)
            lo, hi = (0.0, 1.0) if data != "normal" else (-6.0, 6.0)
            for bins in (50, 4096):
                edges = np.linspace(lo, hi, bins + 1)
                ms, _, _ = row(f"histogram {bins} bins (driver call, incl. edges up / counts back)",
                               lambda: drv.histogram(x.code, x.ptr, n, edges), "bk")
                emit(kernel=f"histogram {bins} vs sum [{tag}]", sums=ms / s_ms)
                if dtype == "float32":
                    t_ms, _, _ = row(f"torch.histc {bins} bins", lambda: torch.histc(tx, bins=bins, min=lo, max=hi)[0].item(),
                                     "torch", reps=5)
                    emit(kernel=f"histogram {bins} vs torch.histc [{tag}]", ratio=ms / t_ms)
                try:
                    t_ms, _, _ = row(f"torch.histogram {bins} bins",
                                     lambda: torch.histogram(tx, bins=bins, range=(lo, hi))[0][0].item(), "torch", reps=5)
                    emit(kernel=f"histogram {bins} vs torch.histogram [{tag}]", ratio=ms / t_ms)
                except Exception as exc:  # (no device kernel in this torch build)
                    emit(kernel=f"torch.histogram {bins} bins [{tag}]", error=type(exc).__name__)
            del tx, x


def axis_rows():
    """The broadcast and the axis statistics (csrc/kernels/axis.hip) on
    10000 x 10000 f64 and f32 and a tall 10^7 x 8 f64 table, uniform data:
    `python tools/bench_kernels.py axis` (profiles/axis_kernels.jsonl).  Each
    new operation beside a yardstick measured in the same run: X - v beside
    bk.subtract of two equal-shape arrays (which moves half as much again),
    max(axis) beside bk.sum(axis) of the same matrix (the same bytes read),
    var(axis) beside two such sums; and beside its torch counterpart."""
    bk.init()
    emit(kernel="device", **bk.device_info())
    for dtype, esize, shape in (("float64", 8, (10000, 10000)), ("float32", 4, (10000, 10000)),
                                ("float64", 8, (10**7, 8))):
        rows, cols = shape
        n = rows * cols
        tdt = torch.float64 if dtype == "float64" else torch.float32
        x = bk.random.uniform(0.0, 1.0, shape, dtype=dtype)._materialize()
        y = bk.random.uniform(0.0, 1.0, shape, dtype=dtype)._materialize()
        vc = bk.random.uniform(0.0, 1.0, (cols,), dtype=dtype)._materialize()
        vr = bk.random.uniform(0.0, 1.0, (rows, 1), dtype=dtype)._materialize()
        tx = torch.empty(shape, dtype=tdt, device="cuda").uniform_()
        tvc = torch.empty(cols, dtype=tdt, device="cuda").uniform_()
        tvr = torch.empty((rows, 1), dtype=tdt, device="cuda").uniform_()
        tag = f"{dtype} {rows}x{cols}"

        def row(kernel, fn, timer, nbytes, **kw):
            ms, mn, mx = spread(fn, timer, reps=10, warmup=2)
            emit(kernel=f"{kernel} [{tag}]", rows=rows, cols=cols, ms=ms, min_ms=mn, max_ms=mx,
                 GBps=nbytes / ms / 1e6, **kw)
            return ms, mn, mx

        e_ms, e_mn, e_mx = row("subtract (X - Y, equal shapes)", lambda: bk.subtract(x, y), "bk", 3 * n * esize)
        for name, v, tv in (("row vector v[c]", vc, tvc), ("column vector v[r]", vr, tvr)):
            ms, _, _ = row(f"broadcast subtract (X - {name})", lambda: bk.subtract(x, v), "bk", 2 * n * esize)
            t_ms, _, _ = row(f"torch X - {name}", lambda: tx - tv, "torch", 2 * n * esize)
            emit(kernel=f"broadcast {name} vs equal-shape subtract [{tag}]", ratio=ms / e_ms,
                 no_longer_than_subtract=bool(ms <= e_ms), vs_torch=ms / t_ms)
        for axis in (0, 1):
            s_ms, s_mn, s_mx = row(f"sum(axis={axis})", lambda: bk.sum(x, axis=axis), "bk", n * esize)
            ms, _, _ = row(f"max(axis={axis})", lambda: bk.amax(x, axis=axis), "bk", n * esize)
            t_ms, _, _ = row(f"torch.amax(dim={axis})", lambda: torch.amax(tx, dim=axis), "torch", n * esize)
            emit(kernel=f"max(axis={axis}) vs sum(axis={axis}) [{tag}]", ratio=ms / s_ms,
                 within_sum_plus_spread=bool(ms <= s_ms + (s_mx - s_mn)), vs_torch=ms / t_ms)
            ms, _, _ = row(f"var(axis={axis}) (two passes)", lambda: bk.var(x, axis=axis), "bk", 2 * n * esize)
            t_ms, _, _ = row(f"torch.var(dim={axis})", lambda: torch.var(tx, dim=axis, unbiased=False), "torch",
                             2 * n * esize)
            emit(kernel=f"var(axis={axis}) vs 2 x sum(axis={axis}) [{tag}]", sums=ms / s_ms,
                 within_two_sums_plus_spread=bool(ms <= 2 * s_ms + (s_mx - s_mn)), vs_torch=ms / t_ms)
        del x, y, vc, vr, tx, tvc, tvr


def dist_rows():
    """The continuous distributions (csrc/kernels/random.hip bk_rand_dist), n = 1e8,
    f64 and f32, driver calls into one buffer: `python tools/bench_kernels.py dist`
    (profiles/dist_kernels.jsonl).  Each beside a yardstick measured in the same
    run: the one-uniform transforms beside bk_rand_uniform of the dtype (the
    write-bound floor), lognormal and the rejection kinds beside bk_rand_normal;
    torch's device samplers on a buffer of the same size are the outside reference."""
    from bee_code_interpreter_fs_amd.ops import driver as D
    from bee_code_interpreter_fs_amd.ops.array import driver

    bk.init()
    emit(kernel="device", **bk.device_info())
    drv = driver()
    n = 10**8
    one_uniform = [("exponential", D.DIST_EXPONENTIAL, 2.0, 0.0), ("laplace", D.DIST_LAPLACE, 1.0, 0.5),
                   ("logistic", D.DIST_LOGISTIC, -1.0, 2.0), ("gumbel", D.DIST_GUMBEL, 0.5, 1.5),
                   ("rayleigh", D.DIST_RAYLEIGH, 1.5, 0.0), ("weibull(1.7)", D.DIST_WEIBULL, 1.7, 0.0),
                   ("pareto(3)", D.DIST_PARETO, 3.0, 0.0), ("cauchy", D.DIST_CAUCHY, 0.0, 1.0)]
    rejection = [("gamma(2.5)", D.DIST_GAMMA, 2.5, 1.0), ("gamma(0.3)", D.DIST_GAMMA, 0.3, 1.0),
                 ("beta(2, 5)", D.DIST_BETA, 2.0, 5.0), ("student_t(5)", D.DIST_STUDENT_T, 5.0, 0.0)]
    for dtype, esize in (("float64", 8), ("float32", 4)):
        x = bk.empty(n, dtype)
        tx = torch.empty(n, dtype=torch.float64 if esize == 8 else torch.float32, device="cuda")

        def row(kernel, fn, timer="bk", **kw):
            ms, mn, mx = spread(fn, timer, reps=10, warmup=2)
            emit(kernel=f"{kernel} [{dtype}]", n=n, ms=ms, min_ms=mn, max_ms=mx, GBps=n * esize / ms / 1e6, **kw)
            return ms, mn, mx

        u_ms, u_mn, u_mx = row("rand_uniform", lambda: drv.rand(0, x.ptr, n, x.code, 1, 0, 0.0, 1.0))
        n_ms, n_mn, n_mx = row("rand_normal", lambda: drv.rand(1, x.ptr, n, x.code, 1, 0, 0.0, 1.0))
        for name, kind, p0, p1 in one_uniform:
            ms, _, _ = row(name, lambda: drv.rand_dist(kind, x.ptr, n, x.code, 1, 0, p0, p1))
            emit(kernel=f"{name} vs rand_uniform [{dtype}]", ratio=ms / u_ms, within_uniform_spread=bool(ms <= u_mx))
        ms, _, _ = row("lognormal", lambda: drv.rand_dist(D.DIST_LOGNORMAL, x.ptr, n, x.code, 1, 0, 0.0, 1.0))
        emit(kernel=f"lognormal vs rand_normal [{dtype}]", ratio=ms / n_ms, within_normal_spread=bool(ms <= n_mx))
        for name, kind, p0, p1 in rejection:
            ms, _, _ = row(name, lambda: drv.rand_dist(kind, x.ptr, n, x.code, 1, 0, p0, p1))
            emit(kernel=f"{name} vs rand_normal [{dtype}]", ratio=ms / n_ms)
        row("torch exponential_", lambda: tx.exponential_(), "torch")
        row("torch log_normal_", lambda: tx.log_normal_(), "torch")
        alpha = torch.full_like(tx, 2.5)
        row("torch._standard_gamma(2.5)", lambda: torch._standard_gamma(alpha), "torch")
        del alpha, tx, x


def int_rows():
    """The int64 kernels (csrc/kernels/integer.hip), n = 1e8, driver calls, medians
    of 10: `python tools/bench_kernels.py int` (profiles/int_kernels.jsonl).  Each
    beside a yardstick measured in the same run: the integers draws beside
    bk_rand_uniform f64 (the same bytes written), bk_int_binary add beside
    bk_binary f64 add, bk_int_reduce sum beside bk_reduce f64 sum (the same bytes
    moved), poisson and binomial beside bk_rand_dist gamma(2.5) (the other
    rejection sampler with a substream per element)."""
    from bee_code_interpreter_fs_amd.ops import driver as D
    from bee_code_interpreter_fs_amd.ops.array import driver

    bk.init()
    emit(kernel="device", **bk.device_info())
    drv = driver()
    n = 10**8
    x, y, z = bk.empty(n, "int64"), bk.empty(n, "int64"), bk.empty(n, "int64")
    f, g, h = bk.random.rand(n)._materialize(), bk.random.rand(n)._materialize(), bk.empty(n, "float64")

    def row(kernel, fn, nbytes=n * 8, **kw):
        ms, mn, mx = spread(fn, "bk", reps=10, warmup=2)
        emit(kernel=kernel, n=n, ms=ms, min_ms=mn, max_ms=mx, GBps=nbytes / ms / 1e6, **kw)
        return ms, mn, mx

    def versus(name, ms, yard, y_ms, y_mn, y_mx):
        emit(kernel=f"{name} vs {yard}", ratio=ms / y_ms, inside_yardstick_spread=bool(y_mn <= ms <= y_mx))

    u = row("rand_uniform f64", lambda: drv.rand(0, h.ptr, n, h.code, 1, 0, 0.0, 1.0))
    for name, lo, hi in (("integers(0, 6)", 0, 6), ("integers(0, 2^40)", 0, 1 << 40)):
        ms, _, _ = row(name, lambda: drv.rand_int(D.RINT_INTEGERS, x.ptr, n, 1, 0, lo, hi, 0.0))
        versus(name, ms, "rand_uniform f64", *u)
    drv.rand_int(D.RINT_INTEGERS, x.ptr, n, 1, 0, -(1 << 40), 1 << 40, 0.0)
    drv.rand_int(D.RINT_INTEGERS, y.ptr, n, 2, 0, -(1 << 40), 1 << 40, 0.0)
    a = row("binary add f64", lambda: drv.binary(0, f.code, 0, f.ptr, g.ptr, 0.0, h.ptr, n), nbytes=n * 24)
    ms, _, _ = row("int_binary add", lambda: drv.int_binary(0, 0, x.ptr, y.ptr, 0, z.ptr, n), nbytes=n * 24)
    versus("int_binary add", ms, "binary add f64", *a)
    ms, _, _ = row("int_binary floor_divide", lambda: drv.int_binary(3, 0, x.ptr, y.ptr, 0, z.ptr, n), nbytes=n * 24)
    versus("int_binary floor_divide", ms, "binary add f64", *a)
    ms, _, _ = row("int_compare less (array, array -> mask)", lambda: drv.int_compare(0, 0, x.ptr, y.ptr, 0, z.ptr, n),
                   nbytes=n * 17)
    c = row("compare less f64 (array, array -> mask)", lambda: drv.compare(0, f.code, 0, f.ptr, g.ptr, 0.0, h.ptr, n),
            nbytes=n * 17)
    versus("int_compare less", ms, "compare less f64", *c)
    s = row("reduce sum f64 (incl. 8B readback)", lambda: drv.reduce(0, f.code, f.ptr, 0, n))
    ms, _, _ = row("int_reduce sum (incl. 8B readback)", lambda: drv.int_reduce(0, x.ptr, n))
    versus("int_reduce sum", ms, "reduce sum f64", *s)
    ms, _, _ = row("int_cast int64 -> f64", lambda: drv.int_cast(5, 1, x.ptr, h.ptr, n), nbytes=n * 16)
    versus("int_cast int64 -> f64", ms, "binary add f64 (24 against 16 bytes an element)", *a)
    ga = row("rand_dist gamma(2.5) f64", lambda: drv.rand_dist(D.DIST_GAMMA, h.ptr, n, h.code, 1, 0, 2.5, 1.0))
    for name, kind, trials, p in (("poisson(3)", D.RINT_POISSON, 0, 3.0), ("poisson(50)", D.RINT_POISSON, 0, 50.0),
                                  ("binomial(10, 0.5)", D.RINT_BINOMIAL, 10, 0.5),
                                  ("binomial(1000, 0.3)", D.RINT_BINOMIAL, 1000, 0.3),
                                  ("geometric(0.2)", D.RINT_GEOMETRIC, 0, 0.2)):
        ms, _, _ = row(name, lambda: drv.rand_int(kind, x.ptr, n, 1, 0, trials, 0, p))
        versus(name, ms, "rand_dist gamma(2.5) f64", *ga)
    tx = torch.empty(n, dtype=torch.int64, device="cuda")
    for name, fn in (("torch random_(0, 6) int64", lambda: tx.random_(0, 6)),
                     ("torch.poisson(3) f64", lambda: torch.poisson(torch.full((n,), 3.0, dtype=torch.float64, device="cuda")))):
        ms, mn, mx = spread(fn, "torch", reps=10, warmup=2)
        emit(kernel=name, n=n, ms=ms, min_ms=mn, max_ms=mx, GBps=n * 8 / ms / 1e6)


def sort_rows():
    """The sort family (csrc/kernels/sort.hip), n = 1e8, medians of 10 with min and max:
    `python tools/bench_kernels.py sort` (profiles/sort_kernels.jsonl).  bk.sort and bk.argsort of f32, f64 and
    int64 on uniform, normal, all-equal and dice data, each beside torch.sort of the same data and bk.sum of the
    same array as the unit (the bytes model: two reads and one write of the keys per pass, so about 3 sums a pass
    for keys only); bk.argmax beside bk.sum and torch.argmax; bk.take with a random permutation and with a sorted
    index beside bk_binary add of equal size and torch's x[idx]."""
    from bee_code_interpreter_fs_amd.ops.array import driver

    bk.init()
    emit(kernel="device", **bk.device_info())
    drv = driver()
    n = 10**8
    rng = bk.random.default_rng(5)

    def row(kernel, fn, timer="bk", **kw):
        ms, mn, mx = spread(fn, timer, reps=10, warmup=2)
        emit(kernel=kernel, n=n, ms=ms, min_ms=mn, max_ms=mx, **kw)
        return ms

    def make(dtype, dist):
        if dtype == "int64":
            if dist == "uniform":
                return rng.integers(-(1 << 62), 1 << 62, n)
            if dist == "normal":
                return (rng.standard_normal(n) * 1e6).astype("int64")
            return rng.integers(1, 7, n) if dist == "dice" else bk.full(n, 1.0, "float64").astype("int64")
        if dist == "uniform":
            x = rng.random(n, dtype=dtype)
        elif dist == "normal":
            x = rng.standard_normal(n, dtype=dtype)
        elif dist == "dice":
            x = rng.integers(1, 7, n).astype(dtype)
        else:
            x = bk.full(n, 1.0, dtype)
        return x._materialize()

    for dtype in ("float32", "float64", "int64"):
        passes = 4 if dtype == "float32" else 8
        for dist in ("uniform", "normal", "all-equal", "dice"):
            x = make(dtype, dist)
            tx = bk.to_torch(x) if dtype != "int64" else torch.from_numpy(x.numpy()).cuda()
            unit = row(f"sum {dtype} {dist}", lambda: bk.sum(x))
            ms = row(f"sort {dtype} {dist}", lambda: bk.sort(x), passes=passes)
            emit(kernel=f"sort {dtype} {dist} vs sum", sums=ms / unit, sums_per_pass=ms / unit / passes, model_sums_per_pass=3.0)
            ms_a = row(f"argsort {dtype} {dist}", lambda: bk.argsort(x), passes=passes)
            emit(kernel=f"argsort {dtype} {dist} vs sum", sums=ms_a / unit, sums_per_pass=ms_a / unit / passes)
            ms_t = row(f"torch.sort {dtype} {dist}", lambda: torch.sort(tx), timer="torch")
            emit(kernel=f"sort {dtype} {dist} vs torch.sort", ratio=ms / ms_t, argsort_ratio=ms_a / ms_t)
            if dist == "normal":
                ms = row(f"argmax {dtype} (incl. 8B readback)", lambda: bk.argmax(x))
                ms_t = row(f"torch.argmax {dtype} (incl. readback)", lambda: int(torch.argmax(tx)), timer="torch")
                emit(kernel=f"argmax {dtype} vs sum", ratio=ms / unit, vs_torch=ms / ms_t)
            del x, tx
    x = rng.random(n)._materialize()
    y, z = rng.random(n)._materialize(), bk.empty(n, "float64")
    tx = bk.to_torch(x)
    add = row("binary add f64", lambda: drv.binary(0, x.code, 0, x.ptr, y.ptr, 0.0, z.ptr, n))
    perm = torch.randperm(n, device="cuda")
    for name, tidx in (("random permutation", perm), ("sorted index", torch.arange(n, device="cuda"))):
        idx = bk.asarray(tidx.cpu().numpy(), dtype="int64")
        ms = row(f"take f64, {name} (incl. 8B readback)", lambda: bk.take(x, idx))
        ms_t = row(f"torch x[idx] f64, {name}", lambda: tx[tidx], timer="torch")
        emit(kernel=f"take f64, {name} vs binary add", ratio=ms / add, vs_torch=ms / ms_t)
        del idx


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    bk.init()
    info = bk.device_info()
    emit(kernel="device", **info)
    n = 10**8
    # draws are lazy (generated on first use, fused into a consuming
    # reduction): materialise explicitly to time the generator + HBM write
    x = bk.random.rand(n)._materialize()
    ms, mn = timed(lambda: bk.random.rand(n)._materialize())
    emit(kernel="philox_uniform_f64", n=n, ms=ms, min_ms=mn, GBps=n * 8 / ms / 1e6)
    tx = torch.empty(n, dtype=torch.float64, device="cuda")
    ms_t, _ = torch_timed(lambda: tx.uniform_())
    emit(kernel="torch.uniform_ f64", n=n, ms=ms_t, GBps=n * 8 / ms_t / 1e6)

    ms, mn = timed(lambda: bk.square(x)._materialize())
    emit(kernel="square_f64", n=n, ms=ms, min_ms=mn, GBps=n * 16 / ms / 1e6)
    ms_t, _ = torch_timed(lambda: torch.square(tx))
    emit(kernel="torch.square f64", n=n, ms=ms_t, GBps=n * 16 / ms_t / 1e6)

    ms, mn = timed(lambda: bk.sum(x))
    emit(kernel="sum_f64 (incl. 8B readback)", n=n, ms=ms, min_ms=mn, GBps=n * 8 / ms / 1e6)
    ms, mn = timed(lambda: bk.sum(bk.square(x)))
    emit(kernel="square_sum_f64 fused", n=n, ms=ms, min_ms=mn, GBps=n * 8 / ms / 1e6)
    ms_t, _ = torch_timed(lambda: torch.sum(torch.square(tx)))
    emit(kernel="torch.sum(square) f64", n=n, ms=ms_t, GBps=n * 8 / ms_t / 1e6)

    # the payload's lowering: sum(square(rand(n))) as ONE fused
    # Philox->square->reduce kernel (no HBM traffic; compute-bound generator)
    ms, mn = timed(lambda: bk.sum(bk.square(bk.random.rand(n))))
    emit(kernel="fused rand->square->sum f64 (no HBM)", n=n, ms=ms, min_ms=mn, Gdraws_per_s=n / ms / 1e6)

    # whole benchmark-numpy payload on device (host wall clock, includes readback)
    for _ in range(3):
        bk.sum(bk.square(bk.random.rand(n)))
    t0 = time.perf_counter()
    for _ in range(10):
        r = bk.sum(bk.square(bk.random.rand(n)))
    emit(kernel="benchmark-numpy payload (host wall)", ms=(time.perf_counter() - t0) * 100, result=float(r))

    for size in (4096, 8192):
        a = bk.random.uniform(-1, 1, (size, size), dtype="bfloat16")
        b = bk.random.uniform(-1, 1, (size, size), dtype="bfloat16")
        bt = b.T  # Bt view: kernel reads the buffer as [N, K]
        flops = 2 * size**3
        c_probe = bk.empty((size, size), "bfloat16")
        from bee_code_interpreter_fs_amd.ops import _native

        emit(kernel="gemm dispatch", size=size, variant=_native.lib().bk_gemm_bf16_pick(
            a.ptr, b.ptr, c_probe.ptr, size, size, size, size, size, size, 2), a_mod=a.ptr % 256, c_mod=c_probe.ptr % 256)
        ms, mn = timed(lambda: bk.gemm_bf16_tn(a, b, "bfloat16"), reps=20)
        emit(kernel=f"gemm_bf16_tn {size}^3", ms=ms, min_ms=mn, TFLOPs=flops / ms / 1e9, TFLOPs_best=flops / mn / 1e9)
        bt_buf = bk.empty((size * size + 8,), "bfloat16")
        from bee_code_interpreter_fs_amd.ops.array import driver

        drv = driver()
        ms_tr, mn_tr = timed(lambda: drv.transpose(b.ptr, bt_buf.ptr, size, size, size, size), reps=20)
        emit(kernel=f"transpose_bf16 {size}^2", ms=ms_tr, min_ms=mn_tr, GBps=4 * size * size / ms_tr / 1e6)
        # same copy through the LDS-tiled fallback (taken for a destination
        # that is not 16-B aligned)
        ms_tr, mn_tr = timed(lambda: drv.transpose(b.ptr, bt_buf.ptr + 2, size, size, size, size), reps=20)
        emit(kernel=f"transpose_bf16 tiled fallback {size}^2", ms=ms_tr, min_ms=mn_tr, GBps=4 * size * size / ms_tr / 1e6)
        del bt_buf
        ms2, _ = timed(lambda: bk.matmul(a, b), reps=10)
        emit(kernel=f"bk.matmul (transpose+gemm) {size}^3", ms=ms2, TFLOPs=flops / ms2 / 1e9)
        b32 = b.astype("float32")
        ms3, _ = timed(lambda: bk.matmul(a, b32), reps=10)
        emit(kernel=f"bk.matmul f32 b (fused convert+transpose, gemm) {size}^3", ms=ms3, TFLOPs=flops / ms3 / 1e9)
        from bee_code_interpreter_fs_amd.ops._native import DTYPE_CODES

        bt16 = bk.empty((size, size), "bfloat16")
        ms4, _ = timed(lambda: drv.transpose(b32.ptr, bt16.ptr, size, size, size, size, DTYPE_CODES["float32"]), reps=20)
        emit(kernel=f"transpose_to_bf16 from f32 {size}^2", ms=ms4, GBps=6 * size * size / ms4 / 1e6)
        del b32, bt16
        ta = torch.empty(size, size, dtype=torch.bfloat16, device="cuda").uniform_(-1, 1)
        tb = torch.empty(size, size, dtype=torch.bfloat16, device="cuda").uniform_(-1, 1)
        ms_t, mn_t = torch_timed(lambda: ta @ tb.T, reps=20)
        emit(kernel=f"torch.matmul (hipBLASLt) {size}^3", ms=ms_t, TFLOPs=flops / ms_t / 1e9, TFLOPs_best=flops / mn_t / 1e9)
        del bt


if __name__ == "__main__":
    modes = {"masks": mask_rows, "stats": stats_rows, "axis": axis_rows, "dist": dist_rows, "int": int_rows, "sort": sort_rows}
    modes[sys.argv[1]]() if len(sys.argv) == 2 and sys.argv[1] in modes else main()

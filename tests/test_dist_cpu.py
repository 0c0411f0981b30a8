"""The continuous distributions above the kernels, on CPU: ``bk.random``
(``ops/array.py``), the numpy offload's legacy functions and Generator methods
(``ops/numpy_offload.py``) over the numpy model of ``bk_rand_dist``
(tests/host_driver_dist.py, tests/dist_ref.py), which records the launches.
Which kind and parameters reach the driver, shapes and dtypes, counters,
fallbacks, errors; and the reference model's own distributions
(Kolmogorov-Smirnov, the bounds of tests/test_dist_gpu.py) at 2^18 elements.
The kernels themselves: tests/test_dist_gpu.py."""

import os
import runpy
import warnings

import numpy as np
import pytest

from bee_code_interpreter_fs_amd import ops
from bee_code_interpreter_fs_amd.ops import npinterop, numpy_offload
from bee_code_interpreter_fs_amd.ops.npinterop import HostFallbackWarning
from bee_code_interpreter_fs_amd.ops.numpy_offload import OffloadArray

from . import dist_ref as D
from .host_driver_dist import use_dist_host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 12  # the offload threshold of these tests

# numpy's name -> (arguments ahead of size, the launch's kind, p0, p1)
CALLS = {
    "exponential": ((2.5,), D.EXPONENTIAL, 2.5, 0.0),
    "standard_exponential": ((), D.EXPONENTIAL, 1.0, 0.0),
    "laplace": ((1.0, 0.5), D.LAPLACE, 1.0, 0.5),
    "logistic": ((-2.0, 3.0), D.LOGISTIC, -2.0, 3.0),
    "gumbel": ((0.5, 2.0), D.GUMBEL, 0.5, 2.0),
    "rayleigh": ((1.5,), D.RAYLEIGH, 1.5, 0.0),
    "weibull": ((1.7,), D.WEIBULL, 1.7, 0.0),
    "pareto": ((3.0,), D.PARETO, 3.0, 0.0),
    "standard_cauchy": ((), D.CAUCHY, 0.0, 1.0),
    "lognormal": ((0.25, 0.75), D.LOGNORMAL, 0.25, 0.75),
    "standard_gamma": ((2.5,), D.GAMMA, 2.5, 1.0),
    "gamma": ((0.3, 2.0), D.GAMMA, 0.3, 2.0),
    "chisquare": ((5.0,), D.GAMMA, 2.5, 2.0),
    "beta": ((2.0, 5.0), D.BETA, 2.0, 5.0),
    "standard_t": ((5.0,), D.STUDENT_T, 5.0, 0.0),
}
DEFAULTS = {"exponential": (D.EXPONENTIAL, 1.0, 0.0), "laplace": (D.LAPLACE, 0.0, 1.0),
            "logistic": (D.LOGISTIC, 0.0, 1.0), "gumbel": (D.GUMBEL, 0.0, 1.0), "rayleigh": (D.RAYLEIGH, 1.0, 0.0),
            "lognormal": (D.LOGNORMAL, 0.0, 1.0)}


@pytest.fixture
def drv(monkeypatch):
    d = use_dist_host_driver(monkeypatch)
    monkeypatch.setattr(npinterop, "_WARNED", set())
    return d


@pytest.fixture
def offload(drv, monkeypatch):
    monkeypatch.setattr(numpy_offload, "MIN_ELEMENTS", N)
    monkeypatch.setattr(numpy_offload, "_GEN", [])
    numpy_offload.patch_numpy_random(np.random, setter=lambda o, k, v: monkeypatch.setattr(o, k, v, raising=False))
    return drv


def launches(drv):
    return [op for op in drv.launches if op[0] != "d2h"]


def host_rng():
    return np.random.Generator(np.random.PCG64(3))  # (never the patched default_rng)


# ---- bk.random -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("dtype", ["float64", "float32", "bfloat16"])
def test_bk_random_methods_launch_their_kind(drv, name, dtype):
    args, kind, p0, p1 = CALLS[name]
    g = ops.random.default_rng(5)
    x = getattr(g, name)(*args, (3, 70), dtype)
    assert isinstance(x, ops.DeviceArray) and x.shape == (3, 70) and x.dtype == dtype
    got = launches(drv)
    assert got[0] == ("rand_dist", kind, 210, p0, p1) and [op[0] for op in got[1:]] == ["cast"] * (dtype == "bfloat16")
    want = D.draw(kind, 210, "float64" if dtype == "float64" else "float32", 5, 0, p0, p1).reshape(3, 70)
    if dtype == "bfloat16":
        want = ops.asarray(want, "float32").astype("bfloat16").numpy()
    np.testing.assert_array_equal(x.numpy(), want)
    # the module-level function on the default generator: the same launch
    del drv.launches[:]
    y = getattr(ops.random, name)(*args, size=16)
    assert y.shape == (16,) and y.dtype == "float64" and launches(drv) == [("rand_dist", kind, 16, p0, p1)]


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_bk_random_defaults_are_numpys(drv, name):
    getattr(ops.random.default_rng(1), name)(size=8)
    assert launches(drv) == [("rand_dist", *DEFAULTS[name][:1], 8, *DEFAULTS[name][1:])]


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_seeded_draws_repeat_and_successive_draws_continue(drv, name, dtype):
    args = CALLS[name][0]
    a = getattr(ops.random.default_rng(9), name)(*args, 1001, dtype).numpy()
    b = getattr(ops.random.default_rng(9), name)(*args, 1001, dtype).numpy()
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, getattr(ops.random.default_rng(10), name)(*args, 1001, dtype).numpy())
    # counters advance by ceil(n / 2), ceil(n / 4) or n: two draws of whole counters are one draw of the sum
    g = ops.random.default_rng(9)
    first, second = getattr(g, name)(*args, 400, dtype).numpy(), getattr(g, name)(*args, 601, dtype).numpy()
    np.testing.assert_array_equal(np.concatenate([first, second]), a)
    kind = CALLS[name][1]
    assert g._offset == D.counters(kind, 400, dtype) + D.counters(kind, 601, dtype)
    h = ops.random.default_rng(9)
    getattr(h, name)(*args, 3, dtype)  # a ragged draw still consumes whole counters
    assert h._offset == D.counters(kind, 3, dtype) == (3 if kind >= D.GAMMA else 1 if dtype == "float32" else 2)


def test_lognormal_is_exp_of_the_normal_counters(drv):
    g, h = ops.random.default_rng(4), ops.random.default_rng(4)
    g.lognormal(0.0, 1.0, 1000)
    h.normal(0.0, 1.0, 1000)
    assert g._offset == h._offset == 500


def test_invalid_parameters_raise_numpys_errors(drv):
    g = ops.random
    for call, text in [(lambda: g.exponential(-1.0, 8), "scale < 0"), (lambda: g.laplace(0.0, -1.0, 8), "scale < 0"),
                       (lambda: g.lognormal(0.0, -0.5, 8), "sigma < 0"), (lambda: g.weibull(0.0, 8), "a <= 0"),
                       (lambda: g.pareto(-1.0, 8), "a <= 0"), (lambda: g.gamma(-1.0, 1.0, 8), "shape <= 0"),
                       (lambda: g.gamma(0.0, 1.0, 8), "shape <= 0"), (lambda: g.gamma(1.0, -1.0, 8), "scale < 0"),
                       (lambda: g.beta(0.0, 1.0, 8), "a <= 0"), (lambda: g.beta(1.0, -2.0, 8), "b <= 0"),
                       (lambda: g.standard_t(0.0, 8), "df <= 0"), (lambda: g.chisquare(-3.0, 8), "df <= 0"),
                       (lambda: g.rayleigh(float("nan"), 8), "scale must be finite"),
                       (lambda: g.gumbel(float("inf"), 1.0, 8), "loc must be finite"),
                       (lambda: g.standard_gamma(float("inf"), 8), "shape must be finite")]:
        with pytest.raises(ValueError, match=text):
            call()
    with pytest.raises(TypeError):
        g.exponential(1.0, 8, dtype="bool")
    assert launches(drv) == []
    assert (g.exponential(0.0, 8).numpy() == 0.0).all() and (g.gamma(2.0, 0.0, 8).numpy() == 0.0).all()


# ---- the numpy offload --------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CALLS))
def test_legacy_functions_draw_on_the_device(offload, name):
    args, kind, p0, p1 = CALLS[name]
    want = getattr(host_rng(), name)(*args, (2, N))
    x = getattr(np.random, name)(*args, (2, N))
    assert isinstance(x, OffloadArray) and x.on_device
    assert x.shape == want.shape and x.dtype == want.dtype == np.float64
    assert launches(offload) == [("rand_dist", kind, 2 * N, p0, p1)]
    y = getattr(np.random, name)(*args, size=N)  # size by keyword
    assert isinstance(y, OffloadArray) and y.shape == (N,) and launches(offload)[1][:3] == ("rand_dist", kind, N)
    assert x.on_device and y.on_device


@pytest.mark.parametrize("name", sorted(CALLS))
def test_generator_methods_draw_on_the_device(offload, name):
    args, kind, p0, p1 = CALLS[name]
    want = getattr(host_rng(), name)(*args, (N, 2))
    rng = np.random.default_rng(12)
    x = getattr(rng, name)(*args, (N, 2))
    assert isinstance(rng, np.random.Generator) and isinstance(x, OffloadArray) and x.on_device
    assert x.shape == want.shape and x.dtype == want.dtype
    assert launches(offload) == [("rand_dist", kind, 2 * N, p0, p1)]
    again = getattr(np.random.default_rng(12), name)(*args, (N, 2))
    np.testing.assert_array_equal(np.asarray(x), np.asarray(again))


def test_generator_dtype_method_and_out_keywords(offload):
    rng = np.random.default_rng(2)
    for call, dtype in [(lambda: rng.standard_exponential(N, dtype=np.float32), np.float32),
                        (lambda: rng.standard_exponential(N, np.float64, "inv"), np.float64),
                        (lambda: rng.standard_exponential(size=N, method="zig"), np.float64),
                        (lambda: rng.standard_gamma(2.0, N, np.float32), np.float32),
                        (lambda: rng.standard_gamma(shape=0.5, size=N, dtype="float64", out=None), np.float64)]:
        x = call()
        assert isinstance(x, OffloadArray) and x.dtype == dtype and x.shape == (N,)
    assert [op[0] for op in launches(offload)] == ["rand_dist"] * 5
    del offload.launches[:]
    out = np.empty(N)
    assert rng.standard_exponential(N, out=out) is out and rng.standard_gamma(2.0, out=out) is out
    assert isinstance(rng.standard_exponential(N, method="box"), np.ndarray)  # any other method: numpy's business
    with pytest.raises(TypeError):
        rng.standard_gamma(2.0, N, dtype=np.int32)
    assert launches(offload) == []


def test_fallbacks_are_numpys_own_calls(offload):
    rng = np.random.default_rng(3)
    plain = [
        np.random.exponential(1.0, N - 1), rng.exponential(1.0, N - 1), np.random.exponential(2.0), rng.gamma(2.0),  # small
        np.random.gamma(np.full(N, 2.0), 1.0, N), rng.gamma(2.0, np.ones(N)), np.random.exponential(np.ones(N)),  # arrays
        rng.beta([2.0] * N, 5.0), np.random.lognormal(np.zeros(N), 1.0, N), rng.standard_t(np.full(N, 3.0), N),
        np.random.gamma(0.0, 1.0, N), rng.standard_gamma(0.0, N),  # shape == 0: numpy's zeros
        np.random.poisson(3.0, N), np.random.binomial(10, 0.5, N), rng.integers(0, 10, N), rng.poisson(2.0, N),
        rng.choice(5, N), np.random.randint(0, 5, N), np.random.standard_t(True, N),
    ]
    for r in plain:
        assert not isinstance(r, OffloadArray)
    assert (plain[10] == 0).all() and (plain[11] == 0).all() and plain[12].dtype.kind == "i"
    # what numpy refuses, it refuses itself
    for bad in (lambda: np.random.exponential(-1.0, N), lambda: rng.exponential(-1.0, N), lambda: np.random.gamma(-1.0, 1.0, N),
                lambda: rng.beta(0.0, 1.0, N), lambda: np.random.weibull(-1.0, N), lambda: rng.standard_t(-2.0, N),
                lambda: np.random.lognormal(0.0, -1.0, N), lambda: rng.pareto(0.0, N), lambda: np.random.chisquare(0.0, N)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        np.random.exponential(1.0, N, np.float32)  # (the legacy functions take no dtype)
    with pytest.raises(TypeError):
        rng.weibull(size=N)
    assert np.isnan(np.random.exponential(float("nan"), N)).all()  # numpy's own NaNs
    assert launches(offload) == []


def test_numpy_seed_repeats_the_device_draws(offload):
    np.random.seed(21)
    a, b = np.random.gamma(2.0, 1.0, N), np.random.exponential(1.0, N)
    np.random.seed(21)
    c, d = np.random.gamma(2.0, 1.0, N), np.random.exponential(1.0, N)
    np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
    np.testing.assert_array_equal(np.asarray(b), np.asarray(d))
    assert not np.array_equal(np.asarray(a), np.asarray(np.random.gamma(2.0, 1.0, N)))


def test_the_claims_example_never_leaves_the_device(offload, capsys):
    with warnings.catch_warnings():
        warnings.simplefilter("error", HostFallbackWarning)
        g = runpy.run_path(os.path.join(ROOT, "examples", "monte_carlo_claims.py"))
    for name in ("frailty", "severity", "wait", "claimed", "paid"):
        assert isinstance(g[name], OffloadArray) and g[name].on_device, name
    n = g["n"]
    kinds = [op[1] for op in launches(offload) if op[0] == "rand_dist"]
    assert kinds == [D.GAMMA, D.LOGNORMAL, D.EXPONENTIAL]
    assert max((op[1] for op in offload.launches if op[0] == "d2h"), default=0) <= 64  # scalars only came back
    severity, claimed = np.asarray(g["severity"]), np.asarray(g["claimed"])
    out = capsys.readouterr().out
    assert f"Claim frequency: {claimed.mean()}" in out and f"Largest claim: {severity[claimed].max()}" in out
    assert f"99% paid claim: {np.percentile(severity[claimed], 99)}" in out
    # the model's draws have the distributions' means (the intervals of tests/test_dist_gpu.py)
    assert abs(claimed.mean() - 5 / 9) < 0.003 and abs(severity[claimed].mean() - np.exp(0.5)) < 0.02


# ---- the reference model's own distributions ---------------------------------------------------

M = 1 << 18
ONE_SAMPLE = [(D.EXPONENTIAL, 2.0, 0.0), (D.LAPLACE, 1.0, 0.5), (D.LOGISTIC, -1.0, 2.0), (D.GUMBEL, 0.5, 1.5),
              (D.RAYLEIGH, 1.5, 0.0), (D.WEIBULL, 1.7, 0.0), (D.PARETO, 3.0, 0.0), (D.CAUCHY, 0.0, 1.0),
              (D.LOGNORMAL, 0.25, 0.75)]
TWO_SAMPLE = [(D.GAMMA, 0.05, 1.0), (D.GAMMA, 0.3, 1.0), (D.GAMMA, 1.0, 1.0), (D.GAMMA, 2.5, 1.0), (D.GAMMA, 20.0, 1.0),
              (D.GAMMA, 1e6, 1.0), (D.BETA, 0.5, 0.5), (D.BETA, 2.0, 5.0), (D.STUDENT_T, 3.0, 0.0),
              (D.STUDENT_T, 30.0, 0.0)]


def numpy_sample(kind, p0, p1, n):
    rng = np.random.Generator(np.random.PCG64(20261))
    if kind == D.GAMMA:
        return rng.gamma(p0, p1, n)
    return rng.beta(p0, p1, n) if kind == D.BETA else rng.standard_t(p0, n)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind,p0,p1", ONE_SAMPLE, ids=[D.NAMES[k[0]] for k in ONE_SAMPLE])
def test_model_matches_the_closed_form_cdf(kind, p0, p1, dtype):
    x = D.draw(kind, M, dtype, 0xD157 + kind, 0, p0, p1)
    assert np.isfinite(x).all()
    # (an f32 sample is compared at its own rounded parameters' CDF: the difference is far below the bound)
    d = D.ks_one_sample(x, lambda s: D.cdf(kind, s, p0, p1))
    print(f"KS_MODEL {D.NAMES[kind]} {dtype} D={d:.5f} bound={D.KS_ONE_BOUND(M):.5f}")
    assert d <= D.KS_ONE_BOUND(M)


@pytest.mark.parametrize("kind,p0,p1", TWO_SAMPLE, ids=[f"{D.NAMES[k[0]]}-{k[1]}-{k[2]}" for k in TWO_SAMPLE])
def test_model_matches_numpys_sampler(kind, p0, p1):
    x, margin, attempts = D.reject(kind, M, 0xD157 + kind, 0, p0, p1)
    assert np.isfinite(x).all() and attempts <= 8 and margin.min() > 0
    d = D.ks_two_sample(x, numpy_sample(kind, p0, p1, M))
    print(f"KS_MODEL {D.NAMES[kind]}({p0}, {p1}) D={d:.5f} bound={D.KS_TWO_BOUND(M):.5f} attempts={attempts}")
    assert d <= D.KS_TWO_BOUND(M)

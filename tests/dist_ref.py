"""Host (numpy) model of ``bk_rand_dist`` (csrc/kernels/random.hip), on the
Philox words of tests/philox_ref.py.

* kinds 0-7: one transform of an open-interval uniform -- the 53-bit / 24-bit
  integer of the uniform draws with its low bit set, so u is in (0, 1) -- on
  the tags ``TAG_DIST_F64`` / ``TAG_DIST_F32``, a counter per 2 f64 / 4 f32
  elements.  The f32 family runs in f32 arithmetic as the kernel does;
  ``wide=True`` evaluates the same 24-bit uniforms in f64 (what the f32
  kernel approximates).
* lognormal: exp of philox_ref's Box-Muller normal.
* gamma / beta / student t: Marsaglia-Tsang in f64.  Element i owns the
  substream (offset + i, tag, attempt j).  One attempt is one Philox call:
  words 0, 1 -> the open 53-bit uniform of the Box-Muller radius, word 2 ->
  the angle, (w + 1/2) 2^-32 turns (cosine branch), word 3 -> the acceptance
  uniform (w + 1/2) 2^-32.  A shape below 1 draws at shape + 1 and multiplies
  by U^(1 / shape), U the open 53-bit uniform of words 0, 1 at attempt 0 on
  the tag ``TAG_BOOST`` above the gamma's.  ``reject`` also returns every
  element's smallest acceptance margin |lhs - rhs| over the comparisons that
  decided it, so a test can tell a robust decision from a coin toss between
  two log implementations.
"""

from __future__ import annotations

import math

import numpy as np

from .philox_ref import _MASK, normal_f32, normal_f64, philox4x32_10

(EXPONENTIAL, LAPLACE, LOGISTIC, GUMBEL, RAYLEIGH, WEIBULL, PARETO, CAUCHY, LOGNORMAL, GAMMA, BETA, STUDENT_T,
 COUNT) = range(13)
NAMES = ("exponential", "laplace", "logistic", "gumbel", "rayleigh", "weibull", "pareto", "cauchy", "lognormal",
         "gamma", "beta", "student_t")
TAG_DIST_F64, TAG_DIST_F32 = 0x64697374, 0x64697375
TAG_GAMMA_X, TAG_GAMMA_Y, TAG_STUDENT_N, TAG_BOOST = 0x67616D30, 0x67616D31, 0x67616D32, 0x10
MAX_ATTEMPTS = 64
_TINY = 2.2250738585072014e-308


def params_ok(kind: int, p0: float, p1: float) -> bool:
    """The entry point's domain rule: both finite; scale, sigma >= 0; shape, a, b, df > 0."""
    if not (math.isfinite(p0) and math.isfinite(p1)):
        return False
    if kind in (EXPONENTIAL, RAYLEIGH):
        return p0 >= 0
    if kind in (LAPLACE, LOGISTIC, GUMBEL, CAUCHY, LOGNORMAL):
        return p1 >= 0
    if kind in (WEIBULL, PARETO, STUDENT_T):
        return p0 > 0
    if kind == GAMMA:
        return p0 > 0 and p1 >= 0
    return kind == BETA and p0 > 0 and p1 > 0


def _words(ctr: np.ndarray, tag: int, attempt, seed: int):
    return philox4x32_10(ctr & _MASK, ctr >> np.uint64(32), np.full(ctr.size, tag), attempt, seed & 0xFFFFFFFF,
                         (seed >> 32) & 0xFFFFFFFF)


def _open53(a, b):
    return ((a >> 5).astype(np.float64) * 67108864.0 + ((b >> 6) | 1).astype(np.float64)) * (1.0 / 9007199254740992.0)


def _open32(w):
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def open_uniforms(n: int, dtype, seed: int, offset: int, wide: bool = False) -> np.ndarray:
    """The uniforms on (0, 1) behind kinds 0-7: f64 from 53 bits, f32 from 24
    (as f64 values with ``wide``: every one is exact in both types)."""
    f64 = np.dtype(dtype) == np.float64
    per = 2 if f64 else 4
    count = (n + per - 1) // per
    ctr = np.arange(offset, offset + count, dtype=np.uint64)
    r = _words(ctr, TAG_DIST_F64 if f64 else TAG_DIST_F32, np.zeros(count), seed)
    out = np.empty(per * count, np.float64 if (f64 or wide) else np.float32)
    if f64:
        out[0::2], out[1::2] = _open53(r[0], r[1]), _open53(r[2], r[3])
    else:
        for j in range(4):
            out[j::4] = ((r[j] >> 8) | 1).astype(out.dtype) * out.dtype.type(1.0 / 16777216.0)
    return out[:n]


def transform(kind: int, u: np.ndarray, p0: float, p1: float) -> np.ndarray:
    """The kernel's formula for kinds 0-7 in u's own precision (numpy's legacy
    formulas with its 1 - U our u)."""
    T = u.dtype.type
    p0, p1 = T(p0), T(p1)
    with np.errstate(all="ignore"):
        if kind == LAPLACE:
            return np.where(u >= T(0.5), p0 - p1 * np.log(T(2) - T(2) * u), p0 + p1 * np.log(T(2) * u)).astype(u.dtype)
        if kind == LOGISTIC:
            return p0 + p1 * np.log(u / (T(1) - u))
        if kind == CAUCHY:
            # tan(pi (u - 1/2)), as 1 / tan(pi (1/2 - |x|)) near the poles
            x = u - T(0.5)
            ax = np.abs(x)
            inner = ax <= T(0.25)
            t = np.tan(T(np.pi) * np.where(inner, ax, T(0.5) - ax))
            return p0 + p1 * np.copysign(np.where(inner, t, T(1) / t), x)
        e = -np.log1p(-u)
        if kind == EXPONENTIAL:
            return p0 * e
        if kind == GUMBEL:
            return p0 - p1 * np.log(e)
        if kind == RAYLEIGH:
            return p0 * np.sqrt(T(2) * e)
        if kind == WEIBULL:
            return np.power(e, T(1) / p0)
        assert kind == PARETO
        return np.expm1(e / p0)


def one_uniform(kind: int, n: int, dtype, seed: int, offset: int, p0: float, p1: float, wide: bool = False):
    """Kinds 0-7.  wide: the f32 draw's exact value -- its 24-bit uniforms and
    its f32 parameters, evaluated in f64."""
    if wide and np.dtype(dtype) == np.float32:
        p0, p1 = float(np.float32(p0)), float(np.float32(p1))
    return transform(kind, open_uniforms(n, dtype, seed, offset, wide), p0, p1)


def lognormal(n: int, dtype, seed: int, offset: int, mean: float, sigma: float) -> np.ndarray:
    """exp of the Box-Muller normal at the same (seed, offset); for f32 the f64
    evaluation of the f32 draw (philox_ref.normal_f32)."""
    fn = normal_f64 if np.dtype(dtype) == np.float64 else normal_f32
    return np.exp(fn(n, seed, offset, mean, sigma))


def _attempt_normal(r):
    return np.sqrt(-2.0 * np.log(_open53(r[0], r[1]))) * np.cos(2.0 * np.pi * _open32(r[2]))


def _gamma(ctr: np.ndarray, tag: int, seed: int, shape: float):
    """(d v of the accepted attempt, log of the boost factor, margins, attempts used) per element."""
    s = shape + 1.0 if shape < 1.0 else shape
    d = s - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    n = ctr.size
    base = np.full(n, d)  # the value at x = 0, kept after MAX_ATTEMPTS rejections
    margin = np.full(n, np.inf)
    used = np.zeros(n, np.int64)
    live = np.arange(n)
    for j in range(MAX_ATTEMPTS):
        if not live.size:
            break
        r = _words(ctr[live], tag, np.full(live.size, j), seed)
        x, u = _attempt_normal(r), _open32(r[3])
        t = 1.0 + c * x
        v = t * t * t
        x2 = x * x
        squeeze = 1.0 - 0.0331 * (x2 * x2)
        with np.errstate(all="ignore"):
            full_l, full_r = np.log(u), 0.5 * x2 + d * (1.0 - v + np.log(v))
        pos = t > 0.0
        ok = pos & ((u < squeeze) | (full_l < full_r))
        m = np.minimum(np.abs(t), np.abs(u - squeeze))
        m = np.where(pos, np.minimum(m, np.abs(full_l - full_r)), m)
        margin[live] = np.minimum(margin[live], m)
        used[live] = j + 1
        base[live[ok]] = d * v[ok]
        live = live[~ok]
    logboost = np.zeros(n)
    if shape < 1.0:
        r = _words(ctr, tag + TAG_BOOST, np.zeros(n), seed)
        logboost = np.log(_open53(r[0], r[1])) * (1.0 / shape)
    return base, logboost, margin, used


def reject(kind: int, n: int, seed: int, offset: int, p0: float, p1: float):
    """Kinds 9-11 in f64: (values, each element's smallest acceptance margin,
    the most attempts any element used).  The f32 draw is ``values.astype(float32)``."""
    ctr = np.arange(offset, offset + n, dtype=np.uint64)
    if kind == GAMMA:
        base, lb, margin, used = _gamma(ctr, TAG_GAMMA_X, seed, p0)
        vals = base * np.exp(lb) * p1 if p0 < 1.0 else base * p1
    elif kind == BETA:
        bx, lx, mx, ux = _gamma(ctr, TAG_GAMMA_X, seed, p0)
        by, ly, my, uy = _gamma(ctr, TAG_GAMMA_Y, seed, p1)
        x = bx * np.exp(lx) if p0 < 1.0 else bx
        y = by * np.exp(ly) if p1 < 1.0 else by
        with np.errstate(all="ignore"):
            vals = np.where(x + y > 0.0, x / (x + y), 1.0 / (1.0 + np.exp((np.log(by) + ly) - (np.log(bx) + lx))))
        margin, used = np.minimum(mx, my), np.maximum(ux, uy)
    else:
        assert kind == STUDENT_T
        base, lb, margin, used = _gamma(ctr, TAG_GAMMA_X, seed, 0.5 * p0)
        g = np.maximum(base * np.exp(lb) if 0.5 * p0 < 1.0 else base, _TINY)
        nrm = _attempt_normal(_words(ctr, TAG_STUDENT_N, np.zeros(n), seed))
        vals = nrm * np.sqrt(p0 / (2.0 * g))
    return vals, margin, int(used.max()) if n else 0


def counters(kind: int, n: int, dtype) -> int:
    """Counters a draw of n elements consumes."""
    if kind >= GAMMA:
        return n
    per = 2 if np.dtype(dtype) == np.float64 else 4
    return (n + per - 1) // per


def draw(kind: int, n: int, dtype, seed: int, offset: int, p0: float, p1: float) -> np.ndarray:
    """What bk_rand_dist writes, in ``dtype`` (f32 / f64)."""
    dtype = np.dtype(dtype)
    if kind <= CAUCHY:
        return one_uniform(kind, n, dtype, seed, offset, p0, p1).astype(dtype)
    if kind == LOGNORMAL:
        return lognormal(n, dtype, seed, offset, mean=p0, sigma=p1).astype(dtype)
    return reject(kind, n, seed, offset, p0, p1)[0].astype(dtype)


# ---- Kolmogorov-Smirnov statistics (a sort each) -------------------------------------------------

def cdf(kind: int, x: np.ndarray, p0: float, p1: float) -> np.ndarray:
    """The closed-form CDF of kinds 0-8 at x."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if kind == EXPONENTIAL:
            return -np.expm1(-x / p0)
        if kind == LAPLACE:
            z = (x - p0) / p1
            return np.where(z < 0, 0.5 * np.exp(z), 1.0 - 0.5 * np.exp(-z))
        if kind == LOGISTIC:
            return 1.0 / (1.0 + np.exp(-(x - p0) / p1))
        if kind == GUMBEL:
            return np.exp(-np.exp(-(x - p0) / p1))
        if kind == RAYLEIGH:
            return -np.expm1(-x * x / (2.0 * p0 * p0))
        if kind == WEIBULL:
            return -np.expm1(-np.power(x, p0))
        if kind == PARETO:
            return -np.expm1(-p0 * np.log1p(x))
        if kind == CAUCHY:
            return 0.5 + np.arctan((x - p0) / p1) / np.pi
        assert kind == LOGNORMAL
        z = (np.log(x) - p0) / (p1 * math.sqrt(2.0))
        return 0.5 * (1.0 + np.array([math.erf(v) for v in z.tolist()]))


def ks_one_sample(x: np.ndarray, F) -> float:
    """sup |empirical CDF of x - F|."""
    s = np.sort(np.asarray(x, np.float64))
    n = s.size
    f = F(s)
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - f), np.max(f - (i - 1) / n)))


def ks_two_sample(a: np.ndarray, b: np.ndarray) -> float:
    """sup |empirical CDF of a - empirical CDF of b|."""
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    pts = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, pts, side="right") / a.size
                               - np.searchsorted(b, pts, side="right") / b.size)))


KS_ONE_BOUND = lambda n: math.sqrt(math.log(2 / 1e-6) / (2 * n))  # noqa: E731 -- 0.00263 at 2^20
KS_TWO_BOUND = lambda n: math.sqrt(math.log(2 / 1e-6) / n)  # noqa: E731 -- 0.00372 at 2^20 (two samples of n)

"""Host (numpy) model of the int64 kernels (csrc/kernels/integer.hip).

* ``binary`` / ``compare`` / ``reduce`` / ``cast``: the reference semantics of
  the arithmetic as small numpy functions -- wrapping add / subtract /
  multiply, Python's floor division and remainder with 0 for a zero divisor
  and the ``INT64_MIN`` / ``-1`` cases, the float -> int64 rule (truncate; NaN,
  inf and anything outside [-2^63, 2^63) give ``INT64_MIN``).
* ``draw``: ``bk_rand_int`` on the Philox words of tests/philox_ref.py, vectorised
  over the elements with a loop over the attempts.  For poisson, binomial and
  geometric it also returns every element's smallest decision margin -- the
  distance by which the comparisons that decided it were decided -- so a test
  can tell a robust decision from a coin toss between two log / lgamma
  implementations.
* the exact pmfs (from ``math.lgamma``) and the pooled chi-square statistic
  with its Wilson-Hilferty bound.

No scipy.
"""

from __future__ import annotations

import math

import numpy as np

from .philox_ref import _MASK, philox4x32_10

INTEGERS, POISSON, BINOMIAL, GEOMETRIC, COUNT = range(5)
NAMES = ("integers", "poisson", "binomial", "geometric")
TAG_INT_SMALL, TAG_INT_LARGE = 0x696E7430, 0x696E7431
TAG_POISSON, TAG_BINOMIAL, TAG_GEOMETRIC = 0x706F6973, 0x62696E6F, 0x67656F6D
MAX_ATTEMPTS = 64
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# The element-by-element cases of tests/test_int_gpu.py, (kind, a, b, p) at (EXACT_SEED, offset 0), EXACT_N
# elements each: both sides of every branch.  tests/test_int_cpu.py asserts that the model's smallest decision
# margin over exactly these exceeds 1e-9, so every decision on the device is the model's.
EXACT_SEED, EXACT_N = 2024, 1 << 16
EXACT_CASES = [(POISSON, 0, 0, lam) for lam in (0.0, 3.0, 9.999, 10.0, 50.0, 1e4)] + \
              [(BINOMIAL, nt, 0, p) for nt, p in ((10, .5), (1, .5), (40, .25), (1000, .3), (30, .9), (5, 0.0), (5, 1.0))] + \
              [(GEOMETRIC, 0, 0, p) for p in (.5, .01, 1.0)]
# (low, high) of the integers cases: spans 1, 6, 2^31 + 1 (rejection rate near 1/2), 2^32, 2^32 + 1, 2^63, 2^64 - 1
INTEGER_CASES = [(-3, -2), (1, 7), (-5, (1 << 31) - 4), (0, 1 << 32), (-1, 1 << 32), (-(1 << 62), 1 << 62),
                 (I64_MIN, I64_MAX)]
INTEGER_N = (1 << 16) + 3
# the chi-square cases at CHI_N draws: (kind, a, b, p)
CHI_N = 1 << 20
CHI_CASES = [(INTEGERS, 0, 6, 0.0), (POISSON, 0, 0, 3.0), (POISSON, 0, 0, 50.0), (BINOMIAL, 20, 0, .5),
             (BINOMIAL, 1000, 0, .3), (GEOMETRIC, 0, 0, .2)]

ADD, SUBTRACT, MULTIPLY, FLOOR_DIVIDE, REMAINDER, MAXIMUM, MINIMUM, BINARY_COUNT = range(8)
F32, F64, I64, BOOL = 0, 1, 5, 6
CAST_PAIRS = ((I64, F64), (I64, F32), (F64, I64), (F32, I64), (BOOL, I64))


# ---- arithmetic -------------------------------------------------------------------------------

def binary(op: int, a, b) -> np.ndarray:
    """a OP b elementwise on int64 arrays (or scalars), as bk_int_binary computes it."""
    a, b = np.broadcast_arrays(np.asarray(a, np.int64), np.asarray(b, np.int64))
    ua, ub = a.astype(np.uint64), b.astype(np.uint64)  # (two's complement reinterpretation)
    with np.errstate(all="ignore"):
        if op == ADD:
            return (ua + ub).astype(np.int64)
        if op == SUBTRACT:
            return (ua - ub).astype(np.int64)
        if op == MULTIPLY:
            return (ua * ub).astype(np.int64)
        if op == MAXIMUM:
            return np.maximum(a, b)
        if op == MINIMUM:
            return np.minimum(a, b)
        # Python's own integers: floor, the remainder takes the divisor's sign
        out = np.empty(a.shape, np.int64)
        flat_a, flat_b, flat_o = a.ravel().tolist(), b.ravel().tolist(), out.reshape(-1)
        for i, (x, y) in enumerate(zip(flat_a, flat_b)):
            if y == 0:
                r = 0
            elif op == FLOOR_DIVIDE:
                r = x // y
                if r > I64_MAX:  # INT64_MIN // -1
                    r = I64_MIN
            else:
                assert op == REMAINDER
                r = x % y
            flat_o[i] = r
        return out


_CMP = [np.less, np.less_equal, np.greater, np.greater_equal, np.equal, np.not_equal]


def compare(op: int, a, b) -> np.ndarray:
    return _CMP[op](np.asarray(a, np.int64), np.asarray(b, np.int64))


def reduce(op: int, a) -> int:
    """0 sum (wrapping), 1 max, 2 min; the identities for an empty array."""
    a = np.asarray(a, np.int64)
    if op == 0:
        return int(a.astype(np.uint64).sum(dtype=np.uint64).astype(np.int64)) if a.size else 0
    if op == 1:
        return int(a.max()) if a.size else I64_MIN
    assert op == 2
    return int(a.min()) if a.size else I64_MAX


def float_to_int64(x) -> np.ndarray:
    """Truncate toward zero; NaN, +-inf and anything outside [-2^63, 2^63) give INT64_MIN."""
    x = np.asarray(x)
    ok = (x >= -9223372036854775808.0) & (x < 9223372036854775808.0)
    out = np.full(x.shape, I64_MIN, np.int64)
    with np.errstate(all="ignore"):
        out[ok] = np.trunc(x[ok].astype(np.float64)).astype(np.int64)
    return out


def cast(src: int, dst: int, x) -> np.ndarray:
    assert (src, dst) in CAST_PAIRS, (src, dst)
    x = np.asarray(x)
    if src == I64:
        return x.astype(np.float64 if dst == F64 else np.float32)  # round to nearest even
    if src == BOOL:
        return (x.view(np.uint8) != 0).astype(np.int64)
    return float_to_int64(x)


# ---- draws --------------------------------------------------------------------------------------

def params_ok(kind: int, a: int, b: int, p: float) -> bool:
    """The entry point's domain rule."""
    if kind == INTEGERS:
        return I64_MIN <= a < b <= I64_MAX
    if kind == POISSON:
        return 0.0 <= p <= 9007199254740992.0
    if kind == BINOMIAL:
        return 0 <= a < (1 << 53) and 0.0 <= p <= 1.0
    return kind == GEOMETRIC and 0.0 < p <= 1.0


def counters(kind: int, n: int, a: int = 0, b: int = 0) -> int:
    """Counters a draw of n elements consumes."""
    if kind == INTEGERS:
        per = 4 if b - a <= (1 << 32) else 2
        return (n + per - 1) // per
    if kind == GEOMETRIC:
        return (n + 1) // 2
    return n


def _words(ctr: np.ndarray, tag: int, attempt, seed: int):
    return philox4x32_10(ctr & _MASK, ctr >> np.uint64(32), np.full(ctr.size, tag), attempt, seed & 0xFFFFFFFF,
                         (seed >> 32) & 0xFFFFFFFF)


def _open53(a, b):
    return ((a >> 5).astype(np.float64) * 67108864.0 + ((b >> 6) | 1).astype(np.float64)) * (1.0 / 9007199254740992.0)


def _open32(w):
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def _lgamma(x: np.ndarray) -> np.ndarray:
    return np.array([math.lgamma(v) for v in np.asarray(x, np.float64).tolist()], np.float64).reshape(np.shape(x))


def integers(n: int, seed: int, offset: int, low: int, high: int):
    """(values, the most attempts any element used)."""
    s = high - low
    assert 1 <= s < (1 << 64)
    small = s <= (1 << 32)
    per = 4 if small else 2
    count = (n + per - 1) // per
    ctr = np.repeat(np.arange(offset, offset + count, dtype=np.uint64), per)[:n]
    lane = (np.arange(n) % per)
    out = np.zeros(n, np.uint64)
    live = np.arange(n)
    used = 0
    thresh = ((1 << 32) % s) if small else ((1 << 64) % s)
    for j in range(MAX_ATTEMPTS):
        if not live.size:
            break
        used = j + 1
        r = _words(ctr[live], TAG_INT_SMALL if small else TAG_INT_LARGE, np.full(live.size, j), seed)
        r = np.stack([np.asarray(w, np.uint64) for w in r])
        ln = lane[live]
        idx = np.arange(live.size)
        if small:
            w = r[ln, idx]
            m = w * np.uint64(s)  # < 2^64: w < 2^32, s <= 2^32
            hi, lo = m >> np.uint64(32), m & _MASK
        else:
            w = (r[2 * ln, idx] << np.uint64(32)) | r[2 * ln + 1, idx]
            prod = [int(v) * s for v in w.tolist()]  # the 128-bit product
            hi = np.array([v >> 64 for v in prod], np.uint64)
            lo = np.array([v & ((1 << 64) - 1) for v in prod], np.uint64)
        out[live] = hi
        ok = lo >= np.uint64(thresh)
        live = live[~ok]
    vals = (out + np.uint64(low & ((1 << 64) - 1))).astype(np.int64)  # wraps into [low, high)
    return vals, used


def poisson(n: int, seed: int, offset: int, lam: float):
    """(values, margins, the most attempts any element used)."""
    ctr = np.arange(offset, offset + n, dtype=np.uint64)
    vals = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    if lam == 0.0 or n == 0:
        return vals, margin, 0
    live = np.arange(n)
    used = 0
    if lam < 10.0:
        enlam = math.exp(-lam)
        prod = np.ones(n)
        for j in range(MAX_ATTEMPTS):
            if not live.size:
                break
            used = j + 1
            r = _words(ctr[live], TAG_POISSON, np.full(live.size, j), seed)
            pos = np.arange(live.size)  # r is indexed by position in this attempt's live set
            for e in range(4):
                u = _open32(np.asarray(r[e], np.uint64)[pos])
                prod[live] = prod[live] * u
                margin[live] = np.minimum(margin[live], np.abs(prod[live] - enlam) / enlam)
                done = prod[live] <= enlam
                vals[live[~done]] += 1
                live, pos = live[~done], pos[~done]
        return vals, margin, used
    slam = math.sqrt(lam)
    loglam = math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    log_invalpha = math.log(1.1239 + 1.1328 / (b - 3.4))
    vr = 0.9277 - 3.6224 / (b - 2.0)
    for j in range(MAX_ATTEMPTS):
        if not live.size:
            break
        used = j + 1
        r = _words(ctr[live], TAG_POISSON, np.full(live.size, j), seed)
        U = _open53(r[0], r[1]) - 0.5
        V = _open53(r[2], r[3])
        us = 0.5 - np.abs(U)
        k = np.floor((2.0 * a / us + b) * U + lam + 0.43)
        vals[live] = np.maximum(k, 0.0).astype(np.int64)
        fast = (us >= 0.07) & (V <= vr)
        rej = ~fast & ((k < 0.0) | ((us < 0.013) & (V > us)))
        full = ~fast & ~rej
        with np.errstate(all="ignore"):
            lhs = np.log(V) + log_invalpha - np.log(a / (us * us) + b)
            kk = np.where(full, k, 0.0)
            rhs = -lam + kk * loglam - _lgamma(kk + 1.0)
        ok = fast | (full & (lhs <= rhs))
        m = np.where(full, np.abs(lhs - rhs), np.inf)
        margin[live] = np.minimum(margin[live], m)
        live = live[~ok]
    return vals, margin, used


def binomial(n: int, seed: int, offset: int, trials: int, p: float):
    """(values, margins, the most attempts any element used)."""
    ctr = np.arange(offset, offset + n, dtype=np.uint64)
    k_out = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    flip = p > 0.5
    pp = 1.0 - p if flip else p
    q = 1.0 - pp
    nt = float(trials)
    used = 0
    if not (trials == 0 or pp == 0.0 or n == 0):
        npq = nt * pp
        live = np.arange(n)
        if npq < 10.0:
            qn = math.exp(nt * math.log1p(-pp))
            bound = min(nt, npq + 10.0 * math.sqrt(npq * q + 1.0))
            for j in range(MAX_ATTEMPTS):
                if not live.size:
                    break
                used = j + 1
                r = _words(ctr[live], TAG_BINOMIAL, np.full(live.size, j), seed)
                u = _open53(r[0], r[1])
                px = np.full(live.size, qn)
                x = np.zeros(live.size)
                walking = np.ones(live.size, bool)  # still in `while (u > px)`
                restart = np.zeros(live.size, bool)
                mg = np.full(live.size, np.inf)
                while walking.any():
                    w = np.nonzero(walking)[0]
                    mg[w] = np.minimum(mg[w], np.abs(u[w] - px[w]) / px[w])
                    go = u[w] > px[w]
                    walking[w[~go]] = False
                    w = w[go]
                    x[w] += 1.0
                    over = x[w] > bound
                    restart[w[over]] = True
                    walking[w[over]] = False
                    w = w[~over]
                    u[w] = u[w] - px[w]
                    px[w] = ((nt - x[w] + 1.0) * pp * px[w]) / (x[w] * q)
                margin[live] = np.minimum(margin[live], mg)
                k_out[live] = np.minimum(x, nt).astype(np.int64)
                live = live[restart]
        else:
            spq = math.sqrt(npq * q)
            b = 1.15 + 2.53 * spq
            a = -0.0873 + 0.0248 * b + 0.01 * pp
            c = npq + 0.5
            vr = 0.92 - 4.2 / b
            alpha = (2.83 + 5.1 / b) * spq
            m = math.floor((nt + 1.0) * pp)
            h = math.lgamma(m + 1.0) + math.lgamma(nt - m + 1.0)
            lpq = math.log(pp / q)
            for j in range(MAX_ATTEMPTS):
                if not live.size:
                    break
                used = j + 1
                r = _words(ctr[live], TAG_BINOMIAL, np.full(live.size, j), seed)
                U = _open53(r[0], r[1]) - 0.5
                V = _open53(r[2], r[3])
                us = 0.5 - np.abs(U)
                k = np.floor((2.0 * a / us + b) * U + c)
                k_out[live] = np.clip(k, 0.0, nt).astype(np.int64)
                fast = (us >= 0.07) & (V <= vr)
                rej = ~fast & ((k < 0.0) | (k > nt))
                full = ~fast & ~rej
                kk = np.where(full, k, 0.0)
                with np.errstate(all="ignore"):
                    lhs = np.log(V * alpha / (a / (us * us) + b))
                    rhs = h - _lgamma(kk + 1.0) - _lgamma(nt - kk + 1.0) + (kk - m) * lpq
                ok = fast | (full & (lhs <= rhs))
                margin[live] = np.minimum(margin[live], np.where(full, np.abs(lhs - rhs), np.inf))
                live = live[~ok]
    vals = trials - k_out if flip else k_out
    return vals, margin, used


def geometric(n: int, seed: int, offset: int, p: float):
    """(values, margins): the margin is the quotient's distance from the nearest integer."""
    pairs = (n + 1) // 2
    ctr = np.arange(offset, offset + pairs, dtype=np.uint64)
    r = _words(ctr, TAG_GEOMETRIC, np.zeros(pairs), seed)
    u = np.empty(2 * pairs)
    u[0::2], u[1::2] = _open53(r[0], r[1]), _open53(r[2], r[3])
    u = u[:n]
    if p == 1.0:
        return np.ones(n, np.int64), np.full(n, np.inf)
    quot = np.log1p(-u) / math.log1p(-p)
    k = np.ceil(quot)
    margin = np.abs(quot - np.rint(quot))
    vals = np.where(k >= 9223372036854775808.0, np.float64(I64_MAX), np.maximum(k, 1.0))
    out = np.full(n, I64_MAX, np.int64)
    fits = vals < 9223372036854775808.0
    out[fits] = vals[fits].astype(np.int64)
    return out, margin


def draw(kind: int, n: int, seed: int, offset: int, a: int, b: int, p: float) -> np.ndarray:
    """What bk_rand_int writes."""
    assert params_ok(kind, a, b, p), (kind, a, b, p)
    if kind == INTEGERS:
        return integers(n, seed, offset, a, b)[0]
    if kind == POISSON:
        return poisson(n, seed, offset, p)[0]
    if kind == BINOMIAL:
        return binomial(n, seed, offset, a, p)[0]
    return geometric(n, seed, offset, p)[0]


# ---- exact pmfs and the chi-square condition --------------------------------------------------

def pmf(kind: int, ks, a: int, b: int, p: float) -> np.ndarray:
    """P(X = k) for every k of ``ks``, from math.lgamma."""
    out = []
    for k in ks:
        if kind == INTEGERS:
            out.append(1.0 / (b - a) if a <= k < b else 0.0)
        elif kind == POISSON:
            out.append(math.exp(-p + k * math.log(p) - math.lgamma(k + 1.0)) if k >= 0 else 0.0)
        elif kind == BINOMIAL:
            if not 0 <= k <= a:
                out.append(0.0)
            else:
                out.append(math.exp(math.lgamma(a + 1.0) - math.lgamma(k + 1.0) - math.lgamma(a - k + 1.0)
                                    + k * math.log(p) + (a - k) * math.log1p(-p)))
        else:
            out.append(p * math.exp((k - 1) * math.log1p(-p)) if k >= 1 else 0.0)
    return np.array(out)


def chi_square(kind: int, x: np.ndarray, a: int, b: int, p: float):
    """(statistic, degrees of freedom) of the sample against the exact pmf.  Cells run over the
    sample's range widened to where the expected count falls below 1e-3; neighbours with an
    expected count below 5 are pooled, and both tails form a cell each."""
    x = np.asarray(x, np.int64)
    n = x.size
    lo_support = {INTEGERS: a, POISSON: 0, BINOMIAL: 0, GEOMETRIC: 1}[kind]
    hi_support = {INTEGERS: b - 1, BINOMIAL: a}.get(kind)
    mean = (a + b - 1) / 2 if kind == INTEGERS else p if kind == POISSON else a * p if kind == BINOMIAL else 1.0 / p
    lo = hi = int(round(mean))
    lo, hi = max(lo, lo_support), max(hi, lo_support)
    if hi_support is not None:
        lo, hi = min(lo, hi_support), min(hi, hi_support)
    while lo > lo_support and n * pmf(kind, [lo], a, b, p)[0] >= 1e-3:
        lo -= 1
    while (hi_support is None or hi < hi_support) and n * pmf(kind, [hi], a, b, p)[0] >= 1e-3:
        hi += 1
    ks = np.arange(lo, hi + 1)
    expected = n * pmf(kind, ks.tolist(), a, b, p)
    observed = np.bincount(np.clip(x, lo, hi) - lo, minlength=ks.size).astype(np.float64)
    # the mass beyond hi (an unbounded support's upper tail, below 1e-3 counts a cell) belongs to the last cell
    if hi_support is None:
        expected[-1] += max(n - expected.sum(), 0.0)
    # pool from the left, then fold a short last cell into its neighbour
    cells_e, cells_o = [], []
    acc_e = acc_o = 0.0
    for e, o in zip(expected.tolist(), observed.tolist()):
        acc_e += e
        acc_o += o
        if acc_e >= 5.0:
            cells_e.append(acc_e), cells_o.append(acc_o)
            acc_e = acc_o = 0.0
    if acc_e > 0.0 or acc_o > 0.0:
        if cells_e:
            cells_e[-1] += acc_e
            cells_o[-1] += acc_o
        else:
            cells_e.append(acc_e), cells_o.append(acc_o)
    e, o = np.array(cells_e), np.array(cells_o)
    return float(((o - e) ** 2 / e).sum()), e.size - 1


def chi_square_bound(df: int) -> float:
    """The chi-square 1 - 1e-6 quantile by Wilson-Hilferty."""
    return df * (1.0 - 2.0 / (9.0 * df) + 4.7534 * math.sqrt(2.0 / (9.0 * df))) ** 3

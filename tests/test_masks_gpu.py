"""The mask kernels (csrc/kernels/mask.hip) on the MI355X, native driver:
comparisons, the fused compare-count, mask reductions and logic, where,
stream compaction and the bool casts, against numpy on the downloaded
operands -- masks byte for byte, counts as integers, values bit for bit.
Then the same through the service: the plain-numpy Monte Carlo payload under
the offload, and every new op once in a broker sandbox.  CPU twins:
test_masks_cpu.py, test_broker_masks_cpu.py."""

import functools
import math
import os
import tempfile

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops.array import driver as _driver  # (ops.driver is the submodule)

from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the 16-byte vector tail, the chunk edge (4 x 256 vectors of f64 = 2048
# elements, of bf16 = 8192; 16384 is a whole number of both), more than one
# tile of the compaction (4096 elements) with a ragged last one
SIZES = [1, 7, 15, 16, 17, 255, 16383, 16384, 16385, (1 << 20) + 3]
DTYPES = ["float32", "float64", "bfloat16"]
OPS = {"less": np.less, "less_equal": np.less_equal, "greater": np.greater, "greater_equal": np.greater_equal,
       "equal": np.equal, "not_equal": np.not_equal}
THRESHOLD = 0.5  # exact in every dtype
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    out = (bits << 16).view(np.float32)
    out[np.isnan(a)] = np.nan
    return out


def _neighbours(dtype):
    """The two values of ``dtype`` next to THRESHOLD."""
    if dtype == "bfloat16":
        bits = np.array([THRESHOLD], np.float32).view(np.uint32)[0]
        return [float(np.array([bits - 0x10000], np.uint32).view(np.float32)[0]),
                float(np.array([bits + 0x10000], np.uint32).view(np.float32)[0])]
    t = np.dtype(dtype).type
    return [float(np.nextafter(t(THRESHOLD), t(0))), float(np.nextafter(t(THRESHOLD), t(1)))]


@functools.lru_cache(maxsize=None)
def _host(dtype, n, seed):
    """Random values in [0, 1) with a block of specials tiled in (every 37
    elements, so they land at every lane and vector position)."""
    rng = np.random.default_rng(1000 * seed + n % 997)
    h = rng.random(n)
    specials = [np.nan, 0.0, -0.0, np.inf, -np.inf, THRESHOLD] + _neighbours(dtype)
    for k, v in enumerate(specials):
        h[k::37 + k] = v
    h = _bf16_round(h.astype(np.float32)) if dtype == "bfloat16" else h.astype(dtype)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def _host_mask(kind, n):
    if kind == "none":
        m = np.zeros(n, bool)
    elif kind == "all":
        m = np.ones(n, bool)
    elif kind == "alternating":
        m = np.arange(n) % 2 == 0
    elif kind == "last":
        m = np.zeros(n, bool)
        m[-1] = True
    else:
        m = np.random.default_rng(n).random(n) < 0.5
    m.setflags(write=False)
    return m


MASK_KINDS = ["none", "all", "alternating", "last", "random"]


def _raw_mask(gpu, m):
    """The bytes of a device mask exactly as the kernel wrote them."""
    raw = np.empty(m.size, np.uint8)
    _driver().d2h(m.ptr, raw)
    return raw


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def _device_bits(gpu, d):
    """The device array's elements as unsigned integers of its size (bf16: the stored 16 bits)."""
    raw = np.empty(d.size, UINT[d.itemsize])
    _driver().d2h(d.ptr, raw)
    return raw


def _host_bits(h, dtype):
    """What the device stores for the host values ``h`` (bf16: the upper half of the f32)."""
    if dtype == "bfloat16":
        return (np.ascontiguousarray(h, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return _bits(h)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", sorted(OPS))
def test_compare_and_fused_count_match_numpy(gpu, op, dtype, n):
    a, b = gpu.asarray(_host(dtype, n, 1), dtype), gpu.asarray(_host(dtype, n, 2), dtype)
    ha, hb = a.numpy(), b.numpy()  # the downloaded operands
    with np.errstate(invalid="ignore"):
        want_ab = OPS[op](ha, hb)
        want_as = OPS[op](ha, ha.dtype.type(THRESHOLD))
    m_ab, m_as = getattr(gpu, op)(a, b), getattr(gpu, op)(a, THRESHOLD)
    # the fused count first (the masks are still lazy), twice: the same value
    c1, c2 = gpu.count_nonzero(m_ab), gpu.count_nonzero(m_ab)
    assert m_ab._lazy is not None and c1 == c2 == int(want_ab.sum())
    assert gpu.count_nonzero(m_as) == int(want_as.sum())
    np.testing.assert_array_equal(_raw_mask(gpu, m_ab), want_ab.astype(np.uint8))
    np.testing.assert_array_equal(_raw_mask(gpu, m_as), want_as.astype(np.uint8))
    # and the count of the materialised mask (bk_reduce on kBool)
    assert m_ab._lazy is None and gpu.count_nonzero(m_ab) == c1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", MASK_KINDS)
def test_mask_reductions_match_numpy(gpu, kind, n):
    h = _host_mask(kind, n)
    m = gpu.asarray(h, dtype="bool")
    s = gpu.sum(m)
    assert isinstance(s, np.int64) and s == h.sum()
    assert gpu.any(m) is bool(h.any()) and gpu.all(m) is bool(h.all())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ["logical_and", "logical_or", "logical_xor", "logical_not"])
def test_mask_logic_matches_numpy(gpu, op, n):
    ha, hb = _host_mask("random", n), _host_mask("alternating", n)
    a, b = gpu.asarray(ha, dtype="bool"), gpu.asarray(hb, dtype="bool")
    if op == "logical_not":
        got, want = gpu.logical_not(a), ~ha
    else:
        got, want = getattr(gpu, op)(a, b), getattr(np, op)(ha, hb)
    np.testing.assert_array_equal(_raw_mask(gpu, got), want.astype(np.uint8))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["array_array", "array_scalar", "scalar_array", "scalar_scalar"])
def test_where_is_bit_exact(gpu, form, dtype, n):
    ha, hb, hm = _host(dtype, n, 3), _host(dtype, n, 4), _host_mask("random", n)
    a, b, m = gpu.asarray(ha, dtype), gpu.asarray(hb, dtype), gpu.asarray(hm, dtype="bool")
    sa, sb = 0.1, -0.0  # 0.1 rounds (RNE) in f32 and bf16; the zero keeps its sign
    t = np.float32 if dtype == "bfloat16" else np.dtype(dtype).type
    ra = _bf16_round(np.array([sa], np.float32))[0] if dtype == "bfloat16" else t(sa)
    rb = t(sb)
    if form == "array_array":
        got, want = gpu.where(m, a, b), np.where(hm, ha, hb)
    elif form == "array_scalar":
        got, want = gpu.where(m, a, sb), np.where(hm, ha, rb)
    elif form == "scalar_array":
        got, want = gpu.where(m, sa, b), np.where(hm, ra, hb)
    else:
        got, want = gpu.where(m, sa, sb, dtype=dtype), np.where(hm, ra, rb)
    assert got.dtype == dtype
    np.testing.assert_array_equal(_device_bits(gpu, got), _host_bits(want, dtype))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES + ["bool"])
@pytest.mark.parametrize("kind", MASK_KINDS)
def test_compress_is_bit_exact_and_in_order(gpu, kind, dtype, n):
    hm = _host_mask(kind, n)
    if dtype == "bool":
        hx = _host_mask("random", n + 1)[1:]
        x = gpu.asarray(hx, dtype="bool")
        want = hx[hm].astype(np.uint8)
    else:
        hx = _host(dtype, n, 5)
        x = gpu.asarray(hx, dtype)
        want = _host_bits(hx[hm], dtype)
    got = x[gpu.asarray(hm, dtype="bool")]
    assert got.dtype == dtype and got.shape == (int(hm.sum()),)
    if got.size:
        np.testing.assert_array_equal(_device_bits(gpu, got), want)


@pytest.mark.parametrize("n", [16385, (1 << 20) + 3])
def test_compress_never_writes_past_cap(gpu, n):
    hx, hm = _host("float64", n, 6), _host_mask("random", n)
    x, m = gpu.asarray(hx), gpu.asarray(hm, dtype="bool")
    count = int(hm.sum())
    cap = count // 2
    out = gpu.full((count + 64,), -7.0)  # a deliberately larger buffer of sentinels
    _driver().compress(x.code, x.ptr, m.ptr, n, out.ptr, cap)
    got = out.numpy()
    np.testing.assert_array_equal(_bits(got[:cap]), _bits(hx[hm][:cap]))
    assert (got[cap:] == -7.0).all()


def test_any_non_zero_byte_is_true(gpu):
    n = 16385
    raw = np.tile(np.array([0, 1, 2, 255], np.uint8), n // 4 + 1)[:n]
    truth = raw != 0
    m = gpu.empty(n, "bool")
    _driver().h2d(m.ptr, raw)  # what a sandbox can upload through the broker's WRITE
    assert gpu.sum(m) == truth.sum() and gpu.any(m) and not gpu.all(m)
    hx = _host("float64", n, 7)
    x = gpu.asarray(hx)
    np.testing.assert_array_equal(_bits(gpu.where(m, x, -1.0).numpy()), _bits(np.where(truth, hx, -1.0)))
    np.testing.assert_array_equal(_bits(x[m].numpy()), _bits(hx[truth]))
    np.testing.assert_array_equal(_raw_mask(gpu, gpu.logical_not(m)), (~truth).astype(np.uint8))
    np.testing.assert_array_equal(_raw_mask(gpu, gpu.logical_and(m, m)), truth.astype(np.uint8))
    np.testing.assert_array_equal(m.astype("float32").numpy(), truth.astype(np.float32))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_bool_casts(gpu, dtype, n):
    h = _host_mask("random", n)
    got = gpu.asarray(h, dtype="bool").astype(dtype)
    assert got.dtype == dtype
    np.testing.assert_array_equal(got.numpy(), h.astype(dtype))


def test_float_entry_points_refuse_masks(gpu):
    m = gpu.asarray(_host_mask("random", 256), dtype="bool")
    out = gpu.empty(256, "float64")
    d, code = _driver(), m.code
    assert code == 6
    for call in (lambda: d.unary(0, code, m.ptr, out.ptr, 256),
                 lambda: d.binary(0, code, 1, m.ptr, 0, 1.0, out.ptr, 256),
                 lambda: d.rand(0, out.ptr, 256, code, 1, 0, 0.0, 1.0),
                 lambda: d.transpose(m.ptr, out.ptr, 16, 16, 16, 16, code, code),
                 lambda: d.reduce_axis(0, code, m.ptr, out.ptr, 16, 16, 16, 0),
                 lambda: d.gemm_fp(code, False, False, m.ptr, m.ptr, out.ptr, 4, 4, 4, 4, 4, 4),
                 lambda: d.reduce(1, code, m.ptr, 0, 256),
                 lambda: d.compare(0, code, 1, m.ptr, 0, 0.5, out.ptr, 256),
                 lambda: d.where(code, m.ptr, 3, 0, 0, 1.0, 0.0, out.ptr, 256)):
        with pytest.raises(gpu.BeekernError, match="bad argument"):
            call()


def test_numpy_protocols_on_the_kernels(gpu):
    """np.* on device arrays: the lazy mask's counts are the fused kernel's."""
    n = 16385
    hx, hy = _host("float64", n, 8), _host("float64", n, 9)
    x, y = gpu.asarray(hx), gpu.asarray(hy)
    with np.errstate(invalid="ignore"):
        want = hx * hx + hy * hy <= 1.0
        inside = x * x + y * y <= 1.0
    s = np.sum(inside)
    assert isinstance(s, np.int64) and s == want.sum()
    assert np.mean(inside) == want.mean() and np.count_nonzero(inside) == want.sum()
    np.testing.assert_array_equal(_bits(np.where(inside, x, y).numpy()), _bits(np.where(want, hx, hy)))
    np.testing.assert_array_equal(_bits(x[inside].numpy()), _bits(hx[want]))
    np.testing.assert_array_equal((inside & ~(x > THRESHOLD)).numpy(), want & ~(hx > THRESHOLD))


# ---- through the service ---------------------------------------------------------------

@pytest.fixture(scope="module")
def msvc():
    ensure_native_executor()
    h = ServiceHarness(tempfile.mkdtemp(prefix="bee-masks-"), gpu_ids=[0], workers_per_gpu_target=1,
                       default_timeout=120.0)
    h.start()
    yield h
    h.stop()


def test_monte_carlo_pi_under_the_offload(msvc):
    """Plain numpy, Execute(numpy_offload=True): comparison, count and
    selection stay on the sandbox's GPU.  |Pi - pi| < 6 sigma with
    sigma = 4 sqrt(p (1 - p) / n), p = pi / 4, n = 4e6: 4.9e-3."""
    src = open(os.path.join(ROOT, "examples", "monte_carlo_pi.py")).read()
    r = msvc.call(msvc.ctx.code_executor.execute(source_code=src, numpy_offload=True, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    p, n = math.pi / 4, 4e6
    sigma = 4 * math.sqrt(p * (1 - p) / n)
    assert 6 * sigma == pytest.approx(4.9e-3, rel=0.02)
    assert abs(float(r.stdout.split("Pi:")[1].split()[0]) - math.pi) < 6 * sigma, r.stdout
    assert "HostFallbackWarning" not in r.stderr, r.stderr


def test_every_mask_op_in_a_broker_sandbox(msvc):
    code = (
        "import beekern as bk, numpy as np\n"
        "n = 16385\n"
        "rng = np.random.default_rng(3)\n"
        "hx, hy = rng.random(n), rng.random(n)\n"
        "hx[::5] = 0.5\n"
        "x, y = bk.asarray(hx), bk.asarray(hy)\n"
        "assert bk.driver_name() == 'broker'\n"
        "lazy = x <= y\n"
        "assert bk.sum(lazy) == (hx <= hy).sum()                                  # COMPARE_COUNT\n"
        "assert (lazy.numpy() == (hx <= hy)).all()                                # COMPARE\n"
        "m = x > 0.5\n"
        "assert bk.count_nonzero(m) == (hx > 0.5).sum() and bk.any(m) and not bk.all(m)\n"
        "assert ((m & ~lazy).numpy() == ((hx > 0.5) & ~(hx <= hy))).all()         # MASK_LOGICAL\n"
        "assert bk.sum(m) == (hx > 0.5).sum() and bk.any(m) and not bk.all(m)    # REDUCE on a mask\n"
        "assert (bk.where(m, x, 0.25).numpy() == np.where(hx > 0.5, hx, 0.25)).all()  # WHERE\n"
        "assert (x[m].numpy() == hx[hx > 0.5]).all()                              # COMPRESS\n"
        "assert (m.astype('float32').numpy() == (hx > 0.5).astype(np.float32)).all()\n"
        "up = bk.asarray(hx > 0.25, dtype='bool')\n"
        "assert (y[up].numpy() == hy[hx > 0.25]).all()\n"
        "print('masks ok', bk.driver_name())\n"
    )
    r = msvc.call(msvc.ctx.code_executor.execute(source_code=code, timeout=120), timeout=300)
    assert r.exit_code == 0, r.stderr
    assert r.stdout.split() == ["masks", "ok", "broker"], r.stdout

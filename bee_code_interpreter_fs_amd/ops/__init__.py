"""beekern — hand-written CDNA4 (gfx950) kernels behind a numpy-like API.

Exposed to sandboxed code as the top-level module ``beekern`` (see
``runtime/sandbox_modules/beekern.py``).  Kernels: Philox RNG, elementwise
(square & friends), deterministic reductions (sum, fused square-sum, dot,
min/max), boolean masks (comparisons, fused counts, where, x[mask]), order statistics and
histograms (median / percentile / quantile by radix select, np.histogram), 2-D broadcasting and
per-axis max / min / var / std, int64 arrays and the integer-valued draws (integers, poisson, binomial,
geometric), bf16 MFMA GEMM and f64 / f32 MFMA GEMM at numpy's precision — source in ``csrc/kernels``.
"""

from ._native import BeekernError, QuotaExceeded, library_path  # noqa: F401
from .array import (  # noqa: F401
    DeviceArray,
    Generator,
    Timer,
    abs,
    add,
    all,
    amax,
    amin,
    any,
    array,
    asarray,
    cos,
    count_nonzero,
    device_info,
    divide,
    dot,
    driver_name,
    empty,
    empty_cache,
    equal,
    exp,
    floor_divide,
    from_numpy,
    from_torch,
    full,
    gemm_bf16_tn,
    greater,
    greater_equal,
    histogram,
    init,
    is_initialized,
    less,
    less_equal,
    log,
    logical_and,
    logical_not,
    logical_or,
    logical_xor,
    matmul,
    matmul_fp,
    max_abs_diff,
    maximum,
    mean,
    median,
    memory_stats,
    minimum,
    mod,
    multiply,
    negative,
    normalize_dtype,
    not_equal,
    ones,
    percentile,
    power,
    quantile,
    random,
    relu,
    remainder,
    set_lazy_random,
    set_quota,
    sigmoid,
    sin,
    sqrt,
    square,
    square_sum,
    std,
    subtract,
    sum,
    synchronize,
    tanh,
    to_torch,
    var,
    where,
    zeros,
)

float32 = "float32"
float64 = "float64"
bfloat16 = "bfloat16"
bool_ = "bool"
int64 = "int64"

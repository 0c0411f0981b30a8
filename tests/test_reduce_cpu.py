"""The premises of tests/test_reduce_gpu.py, checked without a GPU: the inputs
it calls exact are exact (so `==` against the host sum is the right assertion
for any summation order), and its lengths reach the loops they are meant to
reach (tests/reduce_inputs.py)."""

import numpy as np
import pytest

from . import reduce_inputs as R

LONGEST = R.unroll_length()  # the longest array any exact test sums


def _pairwise(x: np.ndarray) -> float:
    x = x.copy()
    while x.size > 1:
        if x.size & 1:
            x = np.append(x, 0.0)
        x = x[0::2] + x[1::2]
    return float(x[0])


def _agree(terms: np.ndarray, want: int) -> None:
    """Forward, reversed, pairwise and numpy's own f64 sums all equal the integer sum."""
    assert abs(want) < 2 ** 53 and int(np.abs(terms).sum()) < 2 ** 53
    f = terms.astype(np.float64)
    assert float(np.cumsum(f)[-1]) == want            # strictly forward
    assert float(np.cumsum(f[::-1])[-1]) == want      # strictly reversed
    assert _pairwise(f) == want
    assert float(f.sum()) == want


@pytest.mark.parametrize("n", [R.all_loops_length(8), LONGEST])
def test_exact_inputs_sum_exactly_in_any_order(n):
    a, b = R.exact_ints(n, 0), R.exact_ints(n, 1)
    assert a.min() >= -128 and a.max() <= 128 and b.min() >= -128 and b.max() <= 128
    assert a.min() < -100 and a.max() > 100 and len(np.unique(a)) == 257
    want = R.exact_sums(a, b)
    assert want[R.SUM] == sum(int(v) for v in a[:100000]) + int(a[100000:].sum())
    _agree(a, want[R.SUM])
    _agree(a * a, want[R.SQUARE_SUM])
    _agree(np.abs(a), want[R.ABS_SUM])
    _agree(a * b, want[R.DOT])


def test_exact_inputs_round_trip_through_every_dtype():
    vals = np.concatenate([np.arange(-128, 129), [300, -300, 600]])  # the inputs and the planted extremes
    for dt in (R.F64, R.F32, R.BF16):
        assert np.array_equal(R.widen(R.to_store(vals, dt), dt), vals.astype(np.float64)), dt
    low = np.ascontiguousarray(vals, np.float32).view(np.uint32) & 0xFFFF
    assert not low.any()  # bf16 holds them exactly: nothing is cut off


def test_bf16_binades_sum_exactly():
    stored = R.bf16_binades()
    x = R.widen(stored, R.BF16)
    assert stored.size == 5120 == len(np.unique(stored)) and np.isfinite(x).all()
    assert np.abs(x).min() == 2.0 ** -10 and np.abs(x).max() < 2.0 ** 10
    scaled = x * 2.0 ** 17  # every value is a multiple of 2^-17
    assert np.array_equal(scaled, np.round(scaled)) and np.abs(scaled).sum() < 2.0 ** 40
    _agree(scaled.astype(np.int64), 0)
    _agree(np.abs(scaled).astype(np.int64), int(np.abs(scaled).sum()))


@pytest.mark.parametrize("N", [2, 4, 8])
def test_lengths_reach_the_loops(N):
    for blocks in (1, 3, 512, 640):
        n = R.all_loops_length(N, blocks)
        nvec, stride = n // N, blocks * 256
        assert nvec + 3 >= 4 * 256 * blocks  # the knob sizes the grid
        per_lane = [len(range(t, nvec, stride)) for t in (0, 4, 5, stride - 1)]
        assert per_lane == [23, 23, 22, 22] and n % N == N - 1
    n = R.fold_twice_length(N, 2049)
    assert [len(range(t, n // N, 2049 * 256)) for t in (0, 4, 5)] == [5, 5, 4]
    assert R.all_loops_length(N) * (16 // N) < R.NT_BYTES  # the cached path; unroll_length() is past it
    # one depth bound covers every length of the default grid that the tests use
    assert R.depth(R.all_loops_length(N), N, 512) == 23 * N + 1 + 15 + 12 + 8 + 12 < 256


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("knob", [3, 512])
def test_ldsdma_lengths_give_idle_short_and_long_waves(knob, strided):
    for N in (2, 4, 8):
        counts = [R.ldsdma_wave_pieces(n, N, knob, strided) for n in R.ldsdma_lengths(N, knob)]
        seen = {c for per_wave in counts for c in per_wave}
        assert 0 in seen and any(0 < c < 16 for c in seen) and 27 in seen and max(seen) == 27
        for n, per_wave in zip(R.ldsdma_lengths(N, knob), counts):
            assert sum(per_wave) == n // (64 * N) and n % (64 * N) == 37 * N + N - 1


def test_rand_lengths_reach_the_capped_grid():
    assert R.rand_blocks(8_388_608 + 3, 2) == 2048 and R.rand_blocks(8_388_608 - 16, 2) == 2048
    assert R.rand_blocks(16_777_216 + 3, 4) == 2048
    assert R.rand_blocks(1001, 2) == 1 and R.rand_blocks(1001, 4) == 1

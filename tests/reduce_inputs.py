"""Inputs, lengths and error bounds of the reduction tests
(tests/test_reduce_gpu.py, its child processes and tests/test_reduce_cpu.py),
derived from the loops and launch arithmetic of csrc/kernels/reduce.hip.
Nothing here needs a GPU."""

import math

import numpy as np

F32, F64, BF16 = 0, 1, 2  # bk::DType
DTYPES = {"float64": F64, "float32": F32, "bfloat16": BF16}
STORE = {F32: np.float32, F64: np.float64, BF16: np.uint16}
SUM, SQUARE_SUM, ABS_SUM, MAX, MIN, DOT, MAX_ABS_DIFF = range(7)  # bk::ReduceOp

RED_BLOCK = 256        # kRedBlock
RED_BLOCKS = 512       # kRedBlocks: the default grid of bk_reduce
RANDRED_BLOCKS = 2048  # kRandRedMaxBlocks: the grid cap of bk_rand_reduce
NT_BYTES = 256 << 20   # kStreamNtBytes: operands of this many bytes together take non-temporal loads
U = 2.0 ** -53         # unit roundoff of f64


def vec(dt: int) -> int:
    """Elements of one 16-byte vector."""
    return 16 // np.dtype(STORE[dt]).itemsize


# ---- exact inputs -----------------------------------------------------------------------------------
# Integers in [-128, 128]: exactly representable in bf16 (8 significant bits), f32 and f64.  Over at most
# 3.6e7 of them |sum x|, sum |x| <= 4.7e9 and sum x^2, |sum a b| <= 5.9e11, far below 2^53, so every partial
# sum of every summation order is an exact f64 and the result does not depend on the order.

def exact_ints(n: int, which: int = 0) -> np.ndarray:
    """x[i] = (i * 2654435761) % 257 - 128 (which = 0) or a second, differently ordered sequence (1)."""
    i = np.arange(n, dtype=np.int64)
    if which == 0:
        return (i * 2654435761) % 257 - 128
    return ((i + 11) * 40503) % 251 - 125


def to_store(ints: np.ndarray, dt: int) -> np.ndarray:
    """Small integers (or any values bf16 holds exactly) in the device's storage type."""
    if dt == BF16:
        bits = np.ascontiguousarray(ints, np.float32).view(np.uint32)
        return (bits >> 16).astype(np.uint16)  # exact: the low 16 bits are zero (test_reduce_cpu.py)
    return np.ascontiguousarray(ints, STORE[dt])


def widen(stored: np.ndarray, dt: int) -> np.ndarray:
    """Stored elements as f64, exactly."""
    if dt == BF16:
        return (stored.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return stored.astype(np.float64)


def bf16_binades() -> np.ndarray:
    """Every finite bf16 bit pattern with 2^-10 <= |x| < 2^10, once each, in a fixed shuffled order:
    20 binades x 128 significands x 2 signs = 5120 values, each a multiple of 2^-17, every partial sum
    below 2^23 -- sums of x and |x| are exact in any order."""
    exp = np.arange(-10, 10) + 127
    bits = (exp[:, None] << 7 | np.arange(128)[None, :]).ravel()
    both = np.concatenate([bits, bits | 0x8000]).astype(np.uint16)
    return both[np.random.default_rng(16).permutation(both.size)]


def exact_sums(a: np.ndarray, b: np.ndarray) -> dict:
    """op -> the result as a Python int, from int64 arithmetic."""
    return {SUM: int(a.sum()), SQUARE_SUM: int((a * a).sum()), ABS_SUM: int(np.abs(a).sum()), DOT: int((a * b).sum())}


# ---- lengths ----------------------------------------------------------------------------------------

def grid_blocks(n: int, N: int, knob: int = RED_BLOCKS) -> int:
    """launch_reduce: a block for every 256 lanes of 4 vectors, at most the knob, at least one."""
    lanes = (n // N + 3) // 4
    return max(1, min((lanes + RED_BLOCK - 1) // RED_BLOCK, knob))


def all_loops_length(N: int, blocks: int = RED_BLOCKS) -> int:
    """The length at which every loop of reduce_1pass runs on a grid of ``blocks``.

    With stride = blocks * 256 vectors and nvec = 22 * stride + 5, lane t starts at i = t:
      * 16 in flight: runs while i + 15 stride < nvec -- once (t + 15 stride < nvec, t + 31 stride is not);
      * 4 in flight:  then i = t + 16 stride, i + 3 stride < nvec -- once (t + 23 stride is not);
      * one at a time: i = t + 20 stride, t + 21 stride, and t + 22 stride for the lanes t < 5;
      * scalar tail: the N - 1 elements after the last whole vector.
    nvec / 4 lanes need 22 blocks for each one of the grid, so the knob, not the work, sizes the grid.
    reduce_chunked on the same length: 22 blocks + 1 stripes of 256 vectors, 23 a block -- one trip of 16
    stripes and 7 single ones; the last stripe is 5 vectors wide, the last blocks own nothing, and the
    grid's last block takes the tail."""
    n = (22 * blocks * RED_BLOCK + 5) * N + (N - 1)
    assert grid_blocks(n, N, blocks) == blocks
    return n


def fold_twice_length(N: int, blocks: int) -> int:
    """For a grid of more than 2048 blocks (the fold of `finish` takes 8 x 256 partials a trip, so
    its loop goes round again): 4 vectors a lane is the least that needs them; with 5 more and a tail
    every lane runs the 4-in-flight loop, five lanes the one-at-a-time loop."""
    n = (4 * blocks * RED_BLOCK + 5) * N + (N - 1)
    assert grid_blocks(n, N, blocks) == blocks
    return n


def unroll_length() -> int:
    """f64 past 256 MiB (the BK_REDUCE_UNROLL variants exist on the non-temporal path only), on the
    default grid: stride = 131072 vectors, nvec = 134 stride + 5.  134 = 16 * 8 + 4 + 2: with 8 in
    flight 16 trips, one trip of the 4-in-flight loop and two single vectors; 134 = 33 * 4 + 2: with 4 in
    flight 33 trips and two single vectors (the 4-in-flight loop has the same bound and never runs);
    five lanes take one more vector, and one scalar element remains."""
    n = (134 * RED_BLOCKS * RED_BLOCK + 5) * 2 + 1
    assert n * 8 >= NT_BYTES
    return n


def ldsdma_wave_pieces(n: int, N: int, knob: int, strided: bool) -> list:
    """The number of 1-KiB pieces each wave of reduce_ldsdma streams (4 waves a block)."""
    pieces = n // (N * 64)
    waves = 4 * grid_blocks(n, N, knob)
    if strided:
        return [(pieces - w + waves - 1) // waves if w < pieces else 0 for w in range(waves)]
    per = (pieces + waves - 1) // waves
    return [min(min(w * per, pieces) + per, pieces) - min(w * per, pieces) for w in range(waves)]


def ldsdma_lengths(N: int, knob: int) -> list:
    """Lengths for reduce_ldsdma on a grid of at most ``knob`` blocks.  A wave with np pieces issues
    min(np, 16), runs the steady-state loop while j + 20 <= np (j += 4), reads back what is in flight
    and loads the up to three pieces never issued directly.  Together the lengths give waves with no
    piece, with fewer than 16, and with 27 (two steady trips, 16 read back, 3 direct); each has a
    partial last piece of 37 vectors and a scalar tail, summed by the grid's last block."""
    waves = 4 * knob
    tail = 37 * N + (N - 1)
    return [tail,                                  # less than one piece: every wave idle
            (waves + 1) * 64 * N + tail,           # a few pieces a wave (the grid is what the work needs)
            (27 * waves - 3) * 64 * N + tail]      # 27 pieces in the first waves


# ---- the error bound of a rounded sum -----------------------------------------------------------------

def depth(n: int, N: int, blocks: int) -> int:
    """D: the longest chain of f64 additions one term can pass through in reduce_1pass on ``blocks``
    blocks, from the launch arithmetic.

      * a lane's accumulator: a lane loads ceil(nvec / stride) vectors of N elements and at most one tail
        element; counted as if all went through one accumulator (acc[0] takes the 4-in-flight loop's first
        vector, the single vectors and the tail on top of its share of the 16-in-flight loop);
      * 15 merges of the 16 accumulators;
      * 6 cross-lane steps of the wave, then 6 more over the block's wave partials in LDS (2 of them
        add non-zero terms);
      * the fold: a lane chains 8 partials a trip, ceil(blocks / 2048) trips, then 6 + 6 steps again.
    """
    nvec = n // N
    stride = blocks * RED_BLOCK
    lane = -(-nvec // stride) * N + 1
    fold = 8 * -(-blocks // (8 * RED_BLOCK))
    return lane + 15 + 6 + 6 + fold + 6 + 6


def rand_depth(n: int, per_counter: int, blocks: int) -> int:
    """The same for bk_rand_reduce (rand_reduce_f64: per_counter 2; rand_reduce_f32: 4): every value of
    every counter a lane takes, one merge of its two accumulators, block and fold as above."""
    units = -(-n // per_counter)
    lane = -(-units // (blocks * RED_BLOCK)) * per_counter
    fold = 8 * -(-blocks // (8 * RED_BLOCK))
    return lane + 1 + 6 + 6 + fold + 6 + 6


def rand_blocks(n: int, per_counter: int, knob: int = RANDRED_BLOCKS) -> int:
    """bk_rand_reduce: a block for every 256 lanes of 8 counters, at most the knob."""
    units = -(-n // per_counter)
    return max(1, min(((units + 7) // 8 + RED_BLOCK - 1) // RED_BLOCK, knob))


def fsum(terms: np.ndarray) -> float:
    """The correctly rounded sum of f64 terms (math.fsum), a million elements at a time."""
    flat = np.ascontiguousarray(terms, np.float64).ravel()
    step = 1 << 20
    return math.fsum(v for k in range(0, flat.size, step) for v in flat[k:k + step].tolist())

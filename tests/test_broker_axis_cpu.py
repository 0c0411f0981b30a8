"""The kernel broker's BROADCAST and AXIS_STAT ops against well-formed and
hostile frames, on CPU: the protocol core over the host-memory device of
``bee-broker-fuzz`` under ASan + UBSan (tests/test_broker_fuzz_cpu.py has the
harness's story).  The host device computes real answers from every element
the frame addresses, so results read back with READ are checked against numpy
and a wrong bound in the core is a sanitizer report."""

from __future__ import annotations

import struct

import numpy as np
import pytest

from .test_broker_fuzz_cpu import (ALLOC_AT, BAD_HANDLE, OK, PROTOCOL, READ, WRITE, _finish, _serve, frame, fuzz_bin,  # noqa: F401
                                   run)

BROADCAST, AXIS_STAT = 29, 30
ROWS, COLS, LD = 5, 4, 6
# client handles (f64 sizes): the matrix with row stride LD, a contiguous
# output, a vector of max(ROWS, COLS), and each one element short
A, Y, V, A_SHORT, Y_SHORT, V_SHORT = 1, 2, 3, 4, 5, 6
SPAN = (ROWS - 1) * LD + COLS
RNG = np.random.default_rng(12)
DATA = RNG.standard_normal(SPAN) + 2.0
VEC = RNG.standard_normal(ROWS) + 3.0
M = np.lib.stride_tricks.as_strided(DATA, (ROWS, COLS), (LD * 8, 8))


def broadcast(op, dt, kind, swapped, a, v, y, rows=ROWS, cols=COLS, lda=LD, ldy=COLS):
    return frame(BROADCAST, struct.pack("<IIIIQQQqqqq", op, dt, kind, swapped, a, v, y, rows, cols, lda, ldy))


def axis_stat(op, dt, x, y, axis, divisor=1.0, rows=ROWS, cols=COLS, ld=LD, pad=0):
    return frame(AXIS_STAT, struct.pack("<IIQQqqqIId", op, dt, x, y, rows, cols, ld, axis, pad, divisor))


def read(h, nbytes):
    """READ frames of at most 64 bytes (the harness echoes those)."""
    return [frame(READ, struct.pack("<QQQ", h, off, min(64, nbytes - off))) for off in range(0, nbytes, 64)]


def setup_frames():
    sizes = {A: SPAN, Y: ROWS * COLS, V: ROWS, A_SHORT: SPAN - 1, Y_SHORT: ROWS * COLS - 1, V_SHORT: COLS - 1}
    return [frame(ALLOC_AT, struct.pack("<QQ", h, n * 8)) for h, n in sizes.items()] + [
        frame(WRITE, struct.pack("<QQ", A, 0) + DATA.tobytes()), frame(WRITE, struct.pack("<QQ", V, 0) + VEC.tobytes())]


def rows_of(fuzz_bin, frames):
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[:8]] == [OK] * 8
    return rows[8:]


def read_back(rows, count, dtype=np.float64):
    return np.frombuffer(b"".join(r[4] for r in rows), dtype)[:count]


_NP_OPS = [np.add, np.subtract, np.multiply, np.divide, np.maximum, np.minimum, np.power]


def test_well_formed_broadcast_frames_reproduce_numpy(fuzz_bin):
    cases = [(op, kind, swapped) for op in range(7) for kind in (0, 1) for swapped in (0, 1)]
    frames = []
    for op, kind, swapped in cases:
        frames += [broadcast(op, 1, kind, swapped, A, V, Y)] + read(Y, ROWS * COLS * 8)
    per = 1 + len(read(Y, ROWS * COLS * 8))
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames), [(i, r[1]) for i, r in enumerate(rows) if r[1] != OK]
    for i, (op, kind, swapped) in enumerate(cases):
        got = read_back(rows[i * per + 1:(i + 1) * per], ROWS * COLS).reshape(ROWS, COLS)
        w = VEC[:COLS][None, :] if kind == 0 else VEC[:, None]
        with np.errstate(all="ignore"):
            want = _NP_OPS[op](w, M) if swapped else _NP_OPS[op](M, w)
        if op == 6:  # the C library's pow and numpy's agree to an ulp, not to the bit
            np.testing.assert_allclose(got, want, rtol=2.0 ** -52, atol=0)
        else:
            np.testing.assert_array_equal(got, want)


def test_broadcast_in_place_and_into_a_strided_output(fuzz_bin):
    frames = [broadcast(1, 1, 0, 0, A, V, A, ldy=LD)] + read(A, SPAN * 8)  # y is a
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames)
    got = read_back(rows[1:], SPAN)
    want = DATA.copy()
    np.lib.stride_tricks.as_strided(want, (ROWS, COLS), (LD * 8, 8))[...] = M - VEC[:COLS]
    np.testing.assert_array_equal(got, want)  # (the gaps between the rows keep their bytes)
    # the same bytes as f32: twice the elements fit
    frames = [broadcast(0, 0, 1, 0, A, V, Y, rows=ROWS, cols=2 * COLS, lda=2 * LD, ldy=2 * COLS)] + read(Y, ROWS * COLS * 8)
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames)
    m32 = np.lib.stride_tricks.as_strided(DATA.view(np.float32), (ROWS, 2 * COLS), (LD * 8, 4))
    with np.errstate(all="ignore"):
        want32 = m32 + VEC.view(np.float32)[:ROWS, None]
    np.testing.assert_array_equal(read_back(rows[1:], 2 * ROWS * COLS, np.float32).reshape(ROWS, 2 * COLS), want32)


def test_well_formed_axis_stat_frames_reproduce_numpy(fuzz_bin):
    cases = [(op, axis, ddof) for op in range(4) for axis in (0, 1) for ddof in ((0, 1) if op >= 2 else (0,))]
    frames = []
    for op, axis, ddof in cases:
        n = M.shape[axis]
        frames += [axis_stat(op, 1, A, Y, axis, float(n - ddof))] + read(Y, 64)
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames), [(i, r[1]) for i, r in enumerate(rows) if r[1] != OK]
    for i, (op, axis, ddof) in enumerate(cases):
        count = COLS if axis == 0 else ROWS
        got = read_back(rows[2 * i + 1:2 * i + 2], count)
        want = [M.max(axis=axis), M.min(axis=axis), M.var(axis=axis, ddof=ddof), M.std(axis=axis, ddof=ddof)][op]
        np.testing.assert_allclose(got, want, rtol=1e-14 if op >= 2 else 0, atol=0)
    # a NaN in a line is that line's max and min; f32 operands
    nan_data = DATA.copy()
    nan_data[LD + 1] = np.nan  # row 1, column 1
    frames = [frame(WRITE, struct.pack("<QQ", A, 0) + nan_data.tobytes()), axis_stat(0, 1, A, Y, 0)] + read(Y, COLS * 8) + [
        axis_stat(1, 1, A, Y, 1)] + read(Y, ROWS * 8) + [
        frame(WRITE, struct.pack("<QQ", A, 0) + DATA.tobytes()),
        axis_stat(3, 0, A, Y, 1, float(2 * COLS - 1), cols=2 * COLS, ld=2 * LD)] + read(Y, ROWS * 4)
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames)
    nan_m = np.lib.stride_tricks.as_strided(nan_data, (ROWS, COLS), (LD * 8, 8))
    np.testing.assert_array_equal(read_back(rows[2:3], COLS), nan_m.max(axis=0))
    np.testing.assert_array_equal(read_back(rows[4:5], ROWS), nan_m.min(axis=1))
    m32 = np.lib.stride_tricks.as_strided(DATA.view(np.float32), (ROWS, 2 * COLS), (LD * 8, 4))
    with np.errstate(all="ignore"):
        want32 = m32.astype(np.float64).std(axis=1, ddof=1).astype(np.float32)
    np.testing.assert_allclose(read_back(rows[7:8], ROWS, np.float32), want32, rtol=2.5e-7, atol=0)


def test_hostile_frames_are_refused(fuzz_bin):
    nan, inf = float("nan"), float("inf")
    frames = [
        # rows * ld wrapping, negative and zero sizes
        broadcast(1, 1, 0, 0, A, V, Y, rows=(1 << 61) + 1, cols=1, lda=1, ldy=1),
        broadcast(1, 1, 0, 0, A, V, Y, rows=(1 << 62), cols=4, lda=4, ldy=4),
        broadcast(1, 1, 1, 0, A, V, Y, rows=2, cols=1, lda=(1 << 63) - 1, ldy=1),
        broadcast(1, 1, 0, 0, A, V, Y, rows=-1), broadcast(1, 1, 0, 0, A, V, Y, cols=-1),
        broadcast(1, 1, 0, 0, A, V, Y, rows=0), broadcast(1, 1, 0, 0, A, V, Y, cols=0),
        axis_stat(0, 1, A, Y, 0, rows=(1 << 61) + 1, cols=1, ld=1), axis_stat(0, 1, A, Y, 1, rows=1 << 62, cols=4, ld=4),
        axis_stat(2, 1, A, Y, 0, 1.0, rows=2, cols=1, ld=(1 << 63) - 1),
        axis_stat(0, 1, A, Y, 0, rows=-1), axis_stat(0, 1, A, Y, 0, cols=-1), axis_stat(0, 1, A, Y, 0, rows=0),
        axis_stat(0, 1, A, Y, 1, cols=0),
        # a row stride below the row length
        broadcast(1, 1, 0, 0, A, V, Y, lda=COLS - 1), broadcast(1, 1, 0, 0, A, V, Y, ldy=COLS - 1),
        axis_stat(0, 1, A, Y, 0, ld=COLS - 1),
        # a matrix, vector or output one element short
        broadcast(1, 1, 0, 0, A_SHORT, V, Y), broadcast(1, 1, 0, 0, A, V, Y_SHORT), broadcast(1, 1, 0, 0, A, V_SHORT, Y),
        broadcast(1, 1, 1, 0, A, V_SHORT, Y), broadcast(1, 1, 0, 0, A, V, A_SHORT, ldy=LD),
        broadcast(0, 0, 0, 0, A, V, Y, cols=2 * COLS + 1, lda=2 * LD + 1, ldy=2 * COLS + 1),
        axis_stat(0, 1, A_SHORT, Y, 0), axis_stat(0, 1, A, V_SHORT, 0), axis_stat(0, 1, A, V_SHORT, 1),
        axis_stat(0, 1, A, A_SHORT, 1, rows=SPAN, cols=1, ld=1),
        # y overlapping v; y the matrix itself with another stride; the statistic written over its input
        broadcast(1, 1, 0, 0, A, Y, Y), broadcast(1, 1, 1, 0, A, Y, Y), broadcast(1, 1, 0, 0, A, A, A, ldy=LD),
        broadcast(1, 1, 0, 0, A, V, A, cols=3, lda=4, ldy=3), axis_stat(0, 1, A, A, 0),
        # unknown ops, dtypes (bf16 and bool too), kinds, flags and axes
        broadcast(7, 1, 0, 0, A, V, Y), broadcast((1 << 32) - 1, 1, 0, 0, A, V, Y),
        broadcast(1, 2, 0, 0, A, V, Y), broadcast(1, 3, 0, 0, A, V, Y), broadcast(1, 6, 0, 0, A, V, Y),
        broadcast(1, 99, 0, 0, A, V, Y), broadcast(1, 1, 2, 0, A, V, Y), broadcast(1, 1, (1 << 32) - 1, 0, A, V, Y),
        broadcast(1, 1, 0, 2, A, V, Y), broadcast(1, 1, 0, 1 << 31, A, V, Y),
        axis_stat(4, 1, A, Y, 0), axis_stat((1 << 32) - 1, 1, A, Y, 0), axis_stat(0, 2, A, Y, 0), axis_stat(0, 3, A, Y, 0),
        axis_stat(0, 6, A, Y, 0), axis_stat(0, 99, A, Y, 0), axis_stat(0, 1, A, Y, 2), axis_stat(0, 1, A, Y, (1 << 32) - 1),
        # a divisor of zero, negative, NaN or infinite
        axis_stat(2, 1, A, Y, 0, 0.0), axis_stat(2, 1, A, Y, 0, -0.0), axis_stat(3, 1, A, Y, 1, -1.0),
        axis_stat(2, 1, A, Y, 0, nan), axis_stat(3, 1, A, Y, 0, inf), axis_stat(2, 1, A, Y, 0, -inf),
        axis_stat(0, 1, A, Y, 0, 0.0), axis_stat(1, 1, A, Y, 1, nan),
        # missing handles
        broadcast(1, 1, 0, 0, 999, V, Y), broadcast(1, 1, 0, 0, A, 999, Y), broadcast(1, 1, 0, 0, A, V, 999),
        axis_stat(0, 1, 999, Y, 0), axis_stat(0, 1, A, 999, 0),
    ]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [BAD_HANDLE] * len(frames), [(i, r[1]) for i, r in enumerate(rows) if r[1] != BAD_HANDLE]


def test_short_frames_are_protocol_errors(fuzz_bin):
    whole = [broadcast(1, 1, 0, 0, A, V, Y), axis_stat(2, 1, A, Y, 0, 4.0)]
    frames = []
    for f in whole:
        op, _, length = struct.unpack_from("<IIQ", f)
        frames += [frame(op, f[16:16 + cut]) for cut in (0, 3, 8, 23, 24, 40, length - 8, length - 1)]
    rows = rows_of(fuzz_bin, whole + frames)
    assert [r[1] for r in rows[:2]] == [OK, OK]  # (whole, they run)
    assert [r[1] for r in rows[2:]] == [PROTOCOL] * len(frames), [r[1] for r in rows]


def _random_axis_frames(seed: int, count: int):
    import random

    rnd = random.Random(seed)
    handles = [A, Y, V, A_SHORT, Y_SHORT, V_SHORT, 999]
    sizes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 24, 25, 2**31, 2**61 + 1, 2**62, 2**63 - 1, 2**64 - 1]

    def num():
        return rnd.choice(sizes) if rnd.random() < 0.85 else rnd.getrandbits(64)

    small = lambda: rnd.choice([0, 1, 0, 1, 2, 3, 6, 7, 2**32 - 1])  # noqa: E731
    out = []
    for _ in range(count):
        # half the frames start from a shape that fits the buffers, then any field may turn hostile
        fits = rnd.random() < 0.5
        rows, cols = (rnd.randrange(1, 6), rnd.randrange(1, 5)) if fits else (num(), num())
        ld = cols + rnd.choice([0, 0, 1, 2]) if fits else num()
        if rnd.random() < 0.3:
            rows, cols, ld = rnd.choice([(num(), cols, ld), (rows, num(), ld), (rows, cols, num())])
        if rnd.random() < 0.5:
            ldy = cols if fits and rnd.random() < 0.8 else num()
            payload = struct.pack("<IIIIQQQQQQQ", small(), rnd.choice([0, 1, 1, 2, 6]), small(), small(),
                                  rnd.choice(handles), rnd.choice(handles), rnd.choice(handles), rows, cols, ld, ldy)
            op = BROADCAST
        else:
            payload = struct.pack("<IIQQQQQIId", small(), rnd.choice([0, 1, 1, 2, 6]), rnd.choice(handles),
                                  rnd.choice(handles), rows, cols, ld, small(), 0,
                                  rnd.choice([1.0, 4.0, 0.0, -1.0, float("nan"), float("inf"), 1e-300]))
            op = AXIS_STAT
        if rnd.random() < 0.05:
            payload = payload[: rnd.randrange(0, len(payload) + 1)]
        out.append(frame(op, payload))
    return out


@pytest.mark.parametrize("seed", [31, 32])
def test_random_axis_frames_no_sanitizer_findings(fuzz_bin, seed):
    rows = rows_of(fuzz_bin, _random_axis_frames(seed, 4000))
    assert len(rows) == 4000
    ran = {op for op, st, *_ in rows if st == OK}
    assert {BROADCAST, AXIS_STAT} <= ran  # the stream reaches the device models


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_client_methods_speak_the_protocol(fuzz_bin, tmp_path, monkeypatch, dtype):
    """The real BrokerDriver's two methods against the daemon's frame reader
    and the protocol core: results read back and checked against numpy."""
    from bee_code_interpreter_fs_amd.ops.driver import BeekernError, BrokerDriver

    monkeypatch.chdir(tmp_path)  # (a relative socket name: sun_path holds 108 bytes)
    p = _serve(fuzz_bin, "s.sock")
    d = BrokerDriver("s.sock")
    d.init(0)
    rows, cols = 33, 17
    h = (np.random.default_rng(7).standard_normal((rows, cols)) + 2.0).astype(dtype)
    hv, hr = h.mean(axis=0), h.max(axis=1)
    dt = 1 if dtype == "float64" else 0
    x, y, v, r = d.malloc(h.nbytes), d.malloc(h.nbytes), d.malloc(hv.nbytes), d.malloc(hr.nbytes)
    d.h2d(x, h), d.h2d(v, hv), d.h2d(r, hr)
    got = np.empty_like(h)
    d.broadcast(1, dt, 0, False, x, v, y, rows, cols, cols, cols)
    d.d2h(y, got)
    np.testing.assert_array_equal(got, h - hv)
    d.broadcast(3, dt, 1, True, x, r, y, rows, cols, cols, cols)
    d.d2h(y, got)
    np.testing.assert_array_equal(got, hr[:, None] / h)
    d.broadcast(2, dt, 1, False, y, r, y, rows, cols, cols, cols)  # in place
    d.d2h(y, got)
    np.testing.assert_array_equal(got, (hr[:, None] / h) * hr[:, None])
    out0, out1 = np.empty(cols, dtype), np.empty(rows, dtype)
    tol = 4 * np.finfo(dtype).eps
    d.axis_stat(0, dt, x, v, rows, cols, cols, 0, 1.0)
    d.d2h(v, out0)
    np.testing.assert_array_equal(out0, h.max(axis=0))
    d.axis_stat(1, dt, x, r, rows, cols, cols, 1, 1.0)
    d.d2h(r, out1)
    np.testing.assert_array_equal(out1, h.min(axis=1))
    d.axis_stat(2, dt, x, v, rows, cols, cols, 0, rows - 1)
    d.d2h(v, out0)
    np.testing.assert_allclose(out0, h.astype(np.float64).var(axis=0, ddof=1).astype(dtype), rtol=tol)
    d.axis_stat(3, dt, x, r, rows, cols, cols, 1, cols)
    d.d2h(r, out1)
    np.testing.assert_allclose(out1, h.astype(np.float64).std(axis=1).astype(dtype), rtol=tol)
    d.broadcast(1, dt, 0, False, x, y, y, rows, cols, cols, cols)  # y is v: refused at the next reply
    with pytest.raises(BeekernError, match="bad handle"):
        d.sync()
    d.axis_stat(2, dt, x, v, rows, cols, cols, 0, 0.0)
    with pytest.raises(BeekernError, match="bad handle"):
        d.sync()
    d.sync()
    d.sock.close()
    assert _finish(p)["live"] == "0"

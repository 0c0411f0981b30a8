"""The kernel broker's mask ops (COMPARE, COMPARE_COUNT, MASK_LOGICAL, WHERE,
COMPRESS; REDUCE on a bool mask) against well-formed and hostile frames, on
CPU: the protocol core over the host-memory device of ``bee-broker-fuzz``
under ASan + UBSan (tests/test_broker_fuzz_cpu.py has the harness's story).
The host device touches n * size bytes of every float operand, n of every
mask and cap * size of a compress output, so a wrong bound in the core is a
sanitizer report here."""

from __future__ import annotations

import random
import struct

import pytest

from .test_broker_fuzz_cpu import (ALLOC, ALLOC_AT, BAD_HANDLE, NO_REPLY, OK, PROTOCOL, READ, REDUCE, SECOND, U64, WRITE,
                                   _finish, _serve, frame, fuzz_bin, run)  # noqa: F401 - fuzz_bin is a fixture

COMPARE, COMPARE_COUNT, MASK_LOGICAL, WHERE, COMPRESS = range(22, 27)
N = 64
X, Y, M, M2, OUT, SHORT_M, SHORT_OUT = 1, 2, 3, 4, 5, 6, 7  # client handles


def compare(op, dt, mode, a, b, y, n, flags=0):
    return frame(COMPARE, struct.pack("<IIIIQQdQq", op, dt, mode, 0, a, b, 0.5, y, n), flags)


def compare_count(op, dt, mode, a, b, n):
    return frame(COMPARE_COUNT, struct.pack("<IIIIQQdq", op, dt, mode, 0, a, b, 0.5, n))


def logical(op, a, b, y, n):
    return frame(MASK_LOGICAL, struct.pack("<IIQQQq", op, 0, a, b, y, n))


def where(dt, flags, m, a, b, y, n):
    return frame(WHERE, struct.pack("<IIQQQddQq", dt, flags, m, a, b, 1.0, 2.0, y, n))


def compress(dt, x, m, n, y, cap):
    return frame(COMPRESS, struct.pack("<IIQQqQq", dt, 0, x, m, n, y, cap))


def setup_frames():
    """f64 operands X, Y and OUT of N elements, masks M, M2 of N bytes, a mask
    one byte short and an output one element short."""
    sizes = {X: N * 8, Y: N * 8, M: N, M2: N, OUT: N * 8, SHORT_M: N - 1, SHORT_OUT: (N - 1) * 8}
    return [frame(ALLOC_AT, struct.pack("<QQ", h, nbytes)) for h, nbytes in sizes.items()]


def statuses(fuzz_bin, frames):
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[:7]] == [OK] * 7
    return rows[7:]


def test_well_formed_frames_run(fuzz_bin):
    frames = [
        compare(1, 1, 0, X, Y, M, N),            # array <= array
        compare(5, 1, 1, X, 0, M2, N),           # array != scalar: b is not looked up
        compare(0, 0, 1, X, 0, M, N),            # f32: N * 4 bytes of X
        compare(0, 2, 0, X, Y, M, N),            # bf16
        compare_count(3, 1, 0, X, Y, N),
        compare_count(4, 1, 1, X, 999, N),
        logical(0, M, M2, M, N), logical(1, M, M2, M2, N), logical(2, M, M2, SHORT_OUT, N),
        logical(3, M, 999, M2, N),               # not: b is not looked up
        where(1, 0, M, X, Y, OUT, N), where(1, 1, M, 999, Y, OUT, N), where(1, 2, M, X, 999, OUT, N),
        where(1, 3, M, 0, 0, OUT, N), where(2, 0, M, X, Y, OUT, N),
        compress(1, X, M, N, OUT, N), compress(1, X, M, N, SHORT_OUT, N - 1), compress(1, X, M, N, OUT, 0),
        compress(6, M, M2, N, OUT, N),           # a mask selected by a mask
        frame(REDUCE, struct.pack("<IIQQq", 0, 6, M, 0, N)),
        frame(REDUCE, struct.pack("<IIQQq", 3, 6, M, 0, N)),
        frame(REDUCE, struct.pack("<IIQQq", 4, 6, M, 0, N)),
        compare(0, 1, 0, X, Y, M, 0),            # n = 0
        compress(1, X, M, 0, OUT, 0),
    ]
    rows = statuses(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames), [r[1] for r in rows]
    assert len(rows[4][4]) == 8 and len(rows[5][4]) == 8  # COMPARE_COUNT replies one f64, like REDUCE
    assert len(rows[19][4]) == 8


def test_hostile_frames_are_refused(fuzz_bin):
    n_wrap = (1 << 61) + 2  # * 8 (f64) wraps to 16
    frames = [
        # n * size overflow
        compare(0, 1, 0, X, Y, M, n_wrap), compare_count(0, 1, 0, X, Y, n_wrap), where(1, 0, M, X, Y, OUT, n_wrap),
        compress(1, X, M, n_wrap, OUT, 1), compress(1, X, M, N, OUT, n_wrap), logical(0, M, M2, M, (1 << 63) - 1),
        # negative sizes
        compare(0, 1, 0, X, Y, M, -1), compress(1, X, M, N, OUT, -1), compress(1, X, M, -1, OUT, 0),
        # a mask buffer one byte short
        compare(0, 1, 0, X, Y, SHORT_M, N), logical(0, M, SHORT_M, M2, N), logical(3, M, 0, SHORT_M, N),
        where(1, 0, SHORT_M, X, Y, OUT, N), compress(1, X, SHORT_M, N, OUT, N),
        frame(REDUCE, struct.pack("<IIQQq", 0, 6, SHORT_M, 0, N)),
        # an operand or output one element short
        compare(0, 1, 0, X, SHORT_OUT, M, N), compare_count(0, 1, 1, SHORT_OUT, 0, N),
        where(1, 0, M, X, Y, SHORT_OUT, N), where(1, 2, M, SHORT_OUT, 0, OUT, N),
        # cap larger than the output
        compress(1, X, M, N, SHORT_OUT, N), compress(1, X, M, N, M2, 9),
        # a compress output aliasing its inputs; a compare mask aliasing an operand
        compress(1, X, M, N, X, N), compress(6, M2, M, N, M, N), compress(1, X, M, N, X, 0),
        compare(0, 0, 0, X, Y, X, N),
        # unknown op, mode, dtype, flag values
        compare(6, 1, 0, X, Y, M, N), compare(0, 1, 2, X, Y, M, N), compare(0, 3, 0, X, Y, M, N),
        compare(0, 6, 0, X, Y, M, N), compare_count(9, 1, 0, X, Y, N), compare_count(0, 1, 7, X, Y, N),
        logical(4, M, M2, M, N), where(1, 4, M, X, Y, OUT, N), where(6, 0, M, X, Y, OUT, N),
        where(3, 0, M, X, Y, OUT, N), compress(3, X, M, N, OUT, 1), compress(5, X, M, N, OUT, 1),
        # missing handles
        compare(0, 1, 0, X, 999, M, N), where(1, 0, M, 999, Y, OUT, N), compress(1, X, 999, N, OUT, 1),
        # bool reduce: sum, any, all only
        frame(REDUCE, struct.pack("<IIQQq", 1, 6, M, 0, N)), frame(REDUCE, struct.pack("<IIQQq", 5, 6, M, M2, N)),
        frame(REDUCE, struct.pack("<IIQQq", 0, 6, M, 0, N + 1)),
    ]
    rows = statuses(fuzz_bin, frames)
    assert [r[1] for r in rows] == [BAD_HANDLE] * len(frames), [(i, r[1]) for i, r in enumerate(rows) if r[1] != BAD_HANDLE]


def test_short_frames_are_protocol_errors(fuzz_bin):
    whole = [compare(0, 1, 0, X, Y, M, N), compare_count(0, 1, 0, X, Y, N), logical(0, M, M2, M, N),
             where(1, 0, M, X, Y, OUT, N), compress(1, X, M, N, OUT, N)]
    frames = []
    for f in whole:
        op, _, length = struct.unpack_from("<IIQ", f)
        frames += [frame(op, f[16:16 + cut]) for cut in (0, 3, length - 8, length - 1)]
    rows = statuses(fuzz_bin, frames)
    assert [r[1] for r in rows] == [PROTOCOL] * len(frames), [r[1] for r in rows]


def test_compress_output_is_scrubbed_not_trusted_as_written(fuzz_bin):
    """COMPRESS writes only the mask's count of elements: the rest of a fresh
    output must read back scrubbed, never as the allocator's stale bytes."""
    frames = [
        frame(WRITE, struct.pack("<QQ", X, 0) + b"\x11" * (N * 8)),
        frame(WRITE, struct.pack("<QQ", M, 0) + b"\x00" * N),   # nothing selected
        compress(1, X, M, N, OUT, 0),
        frame(READ, struct.pack("<QQQ", OUT, 0, N * 8)),
    ]
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[7:]] == [OK] * 4
    assert rows[-1][2] == N * 8


def _random_mask_frames(seed: int, n: int):
    rnd = random.Random(seed)
    handles = [1 << 62, (1 << 62) + 1, 5, 6, 7]
    interesting = [0, 1, 2, 7, 8, 15, 16, 255, 256, 257, 4095, 4096, 4097, 1 << 20, 2**31 - 1, 2**31, 2**32 + 1,
                   2**61 + 2, 2**62, 2**63 - 1, U64 - 7, U64]

    def num():
        return rnd.choice(interesting) if rnd.random() < 0.7 else rnd.getrandbits(64)

    def h():
        return rnd.choice(handles) if rnd.random() < 0.85 else num()

    def count():  # mostly sizes that fit the buffers, so the kernels' models run
        return rnd.choice([0, 1, 16, 31, 32, 256, 512, 4096]) if rnd.random() < 0.6 else num()

    small = lambda: rnd.choice([0, 1, 2, 3, 5, 6, 99, 2**32 - 1])  # noqa: E731
    out = [frame(ALLOC, struct.pack("<Q", 4096)), frame(ALLOC, struct.pack("<Q", 1 << 16)),
           frame(ALLOC_AT, struct.pack("<QQ", 5, 256)), frame(ALLOC_AT, struct.pack("<QQ", 6, 8192)),
           frame(ALLOC_AT, struct.pack("<QQ", 7, 31))]
    for _ in range(n):
        op = rnd.randrange(COMPARE, COMPRESS + 1) if rnd.random() < 0.9 else rnd.choice([REDUCE, READ])
        flags = NO_REPLY if rnd.random() < 0.3 else 0
        flags |= SECOND if rnd.random() < 0.1 else 0
        if op == COMPARE:
            payload = struct.pack("<IIIIQQdQQ", small(), small(), small(), 0, h(), h(), 0.5, h(), count())
        elif op == COMPARE_COUNT:
            payload = struct.pack("<IIIIQQdQ", small(), small(), small(), 0, h(), h(), 0.5, count())
        elif op == MASK_LOGICAL:
            payload = struct.pack("<IIQQQQ", small(), 0, h(), h(), h(), count())
        elif op == WHERE:
            payload = struct.pack("<IIQQQddQQ", small(), small(), h(), h(), h(), 1.0, 2.0, h(), count())
        elif op == COMPRESS:
            payload = struct.pack("<IIQQQQQ", small(), 0, h(), h(), count(), h(), count())
        elif op == REDUCE:
            payload = struct.pack("<IIQQQ", small(), 6, h(), h(), count())
        else:
            payload = struct.pack("<QQQ", h(), 0, count() % 10000)
        if rnd.random() < 0.05:
            payload = payload[: rnd.randrange(0, len(payload) + 1)]
        out.append(frame(op, payload, flags))
    return out


@pytest.mark.parametrize("seed", [11, 12])
def test_random_mask_frames_no_sanitizer_findings(fuzz_bin, seed):
    rows = run(fuzz_bin, _random_mask_frames(seed, 3000), budget=32 << 20, quota=24 << 20)
    assert len(rows) > 3000
    ran = {op for op, st, *_ in rows if st == OK}
    assert {COMPARE, COMPARE_COUNT, MASK_LOGICAL, WHERE, COMPRESS} <= ran  # the stream reaches the device models


def test_client_methods_speak_the_protocol(fuzz_bin, tmp_path, monkeypatch):
    """The real BrokerDriver's mask methods, once each, against the daemon's
    frame reader and the protocol core."""
    import numpy as np

    from bee_code_interpreter_fs_amd.ops.driver import BeekernError, BrokerDriver

    monkeypatch.chdir(tmp_path)  # (a relative socket name: sun_path holds 108 bytes)
    path = "m.sock"
    p = _serve(fuzz_bin, path)
    d = BrokerDriver(path)
    d.init(0)
    n = 1000
    x, y, out = d.malloc(n * 8), d.malloc(n * 8), d.malloc(n * 8)
    m, m2 = d.malloc(n), d.malloc(n)
    d.h2d(x, np.ones(n))
    d.h2d(y, np.zeros(n))
    d.compare(1, 1, 0, x, y, 0.0, m, n)
    d.compare(2, 1, 1, x, 0, 0.5, m2, n)
    assert isinstance(d.compare_count(1, 1, 0, x, y, 0.0, n), float)
    assert isinstance(d.compare_count(1, 1, 1, x, 0, 0.5, n), float)
    d.mask_logical(0, m, m2, m, n)
    d.mask_logical(3, m, 0, m2, n)
    d.where(1, m, 0, x, y, 0.0, 0.0, out, n)
    d.where(1, m, 3, 0, 0, 1.0, 2.0, out, n)
    d.compress(1, x, m, n, out, n)
    assert isinstance(d.reduce(0, 6, m, 0, n), float)
    assert isinstance(d.reduce(3, 6, m, 0, n), float) and isinstance(d.reduce(4, 6, m, 0, n), float)
    d.sync()  # nothing deferred: every frame above was accepted
    d.compress(1, x, m, n, x, n)  # the output aliases its input: refused, reported by the next reply
    with pytest.raises(BeekernError, match="bad handle"):
        d.sync()
    d.sock.close()
    stats = _finish(p)
    assert stats["live"] == "0"

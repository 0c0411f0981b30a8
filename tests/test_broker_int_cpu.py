"""The kernel broker's int64 ops (RAND_INT, INT_BINARY, INT_COMPARE, INT_REDUCE,
INT_CAST) against well-formed and hostile frames, on CPU: the protocol core
over the host-memory device of ``bee-broker-fuzz`` under ASan + UBSan
(tests/test_broker_fuzz_cpu.py has the harness's story).  The host device
computes real integer arithmetic, comparisons, reductions and casts, so
read-backs are checked against the reference semantics (tests/int_ref.py);
every refusal is checked against a Python model of the core's validation, and
a wrong bound in the core is a sanitizer report."""

from __future__ import annotations

import random
import struct

import numpy as np
import pytest

from . import int_ref as R
from .test_broker_fuzz_cpu import (ALLOC_AT, BAD_ARG, BAD_HANDLE, OK, PROTOCOL, READ, WRITE, _finish, _serve,  # noqa: F401
                                   frame, fuzz_bin, run)

RAND_INT, INT_BINARY, INT_COMPARE, INT_REDUCE, INT_CAST = 32, 33, 34, 35, 36
N = 8  # elements: 64 bytes, what one echoed READ returns
A, B, Y, SHORT, MASK, F32, F64 = 1, 2, 3, 4, 5, 6, 7  # client handles
SIZES = {A: N * 8, B: N * 8, Y: N * 8, SHORT: (N - 1) * 8, MASK: N, F32: N * 4, F64: N * 8}
MIN, MAX = R.I64_MIN, R.I64_MAX
HA = np.array([5, -7, 0, MIN, MAX, 3, -1, 1 << 53], np.int64)
HB = np.array([3, 2, 0, -1, -1, -3, MIN, 7], np.int64)
SEED = 0xB10C_1D7


def rand_int(kind, h, n, a, b, p, seed=SEED, off=0):
    return frame(RAND_INT, struct.pack("<IIQqQQqqd", kind, 0, h, n, seed, off, a, b, p))


def int_binary(op, mode, a, b, sc, y, n):
    return frame(INT_BINARY, struct.pack("<IIQQqQq", op, mode, a, b, sc, y, n))


def int_compare(op, mode, a, b, sc, y, n):
    return frame(INT_COMPARE, struct.pack("<IIQQqQq", op, mode, a, b, sc, y, n))


def int_reduce(op, a, n):
    return frame(INT_REDUCE, struct.pack("<IIQq", op, 0, a, n))


def int_cast(s, d, x, y, n):
    return frame(INT_CAST, struct.pack("<IIQQq", s, d, x, y, n))


def write(h, host):
    return frame(WRITE, struct.pack("<QQ", h, 0) + np.ascontiguousarray(host).tobytes())


def read(h, nbytes=64):
    return frame(READ, struct.pack("<QQQ", h, 0, nbytes))


def setup_frames():
    return [frame(ALLOC_AT, struct.pack("<QQ", h, size)) for h, size in SIZES.items()]


def rows_of(fuzz_bin, frames):
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[:len(SIZES)]] == [OK] * len(SIZES)
    return rows[len(SIZES):]


# ---- results through the fake device ---------------------------------------------------------------------

def test_arithmetic_in_every_mode(fuzz_bin):
    frames, want = [write(A, HA), write(B, HB)], []
    for op in range(7):
        frames += [int_binary(op, 0, A, B, 0, Y, N), read(Y), int_binary(op, 1, A, 0, -3, Y, N), read(Y),
                   int_binary(op, 2, A, 999, 7, Y, N), read(Y)]
        want += [R.binary(op, HA, HB), R.binary(op, HA, -3), R.binary(op, 7, HA)]
    frames += [int_binary(R.SUBTRACT, 0, A, B, 0, A, N), read(A), int_binary(R.FLOOR_DIVIDE, 1, B, 0, 0, B, N), read(B)]  # in place
    want += [R.binary(R.SUBTRACT, HA, HB), np.zeros(N, np.int64)]
    rows = rows_of(fuzz_bin, frames)[2:]
    assert [r[1] for r in rows] == [OK] * len(rows)
    for i, w in enumerate(want):
        np.testing.assert_array_equal(np.frombuffer(rows[2 * i + 1][4], np.int64), w, err_msg=f"result {i}")


def test_comparisons_reductions_and_casts(fuzz_bin):
    f64 = np.array([1.5, -2.5, np.nan, np.inf, -np.inf, 2.0 ** 63, -2.0 ** 63, 16777217.0])
    bits = np.array([0, 1, 2, 255, 0, 0, 7, 128], np.uint8)
    frames = [write(A, HA), write(B, HB)]
    for op in range(6):
        frames += [int_compare(op, 0, A, B, 0, MASK, N), read(MASK, N), int_compare(op, 1, A, 0, 3, MASK, N), read(MASK, N)]
    frames += [int_reduce(op, A, N) for op in range(3)] + [int_reduce(op, A, 0) for op in range(3)]
    frames += [int_cast(R.I64, R.F64, A, F64, N), read(F64), int_cast(R.I64, R.F32, A, F32, N), read(F32, 32),
               write(F64, f64), int_cast(R.F64, R.I64, F64, Y, N), read(Y),
               write(F32, f64.astype(np.float32)), int_cast(R.F32, R.I64, F32, Y, N), read(Y),
               write(MASK, bits), int_cast(R.BOOL, R.I64, MASK, Y, N), read(Y)]
    rows = rows_of(fuzz_bin, frames)[2:]
    assert [r[1] for r in rows] == [OK] * len(rows)
    for op in range(6):
        np.testing.assert_array_equal(np.frombuffer(rows[4 * op + 1][4], np.uint8), R.compare(op, HA, HB))
        np.testing.assert_array_equal(np.frombuffer(rows[4 * op + 3][4], np.uint8), R.compare(op, HA, 3))
    red = rows[24:30]
    assert [struct.unpack("<q", r[4])[0] for r in red] == [R.reduce(op, HA) for op in range(3)] + [0, MIN, MAX]
    rest = rows[30:]
    assert rest[1][4] == HA.astype(np.float64).tobytes() and rest[3][4] == HA.astype(np.float32).tobytes()
    np.testing.assert_array_equal(np.frombuffer(rest[6][4], np.int64), R.float_to_int64(f64))
    np.testing.assert_array_equal(np.frombuffer(rest[9][4], np.int64), R.float_to_int64(f64.astype(np.float32)))
    np.testing.assert_array_equal(np.frombuffer(rest[12][4], np.int64), (bits != 0).astype(np.int64))


def test_draws_fill_the_support(fuzz_bin):
    cases = [(R.INTEGERS, 1, 7, 0.0), (R.INTEGERS, MIN, MAX, 0.0), (R.INTEGERS, -5, -4, 0.0), (R.POISSON, 0, 0, 3.0),
             (R.POISSON, 0, 0, 0.0), (R.POISSON, 0, 0, 2.0 ** 53), (R.BINOMIAL, 10, 0, 0.5), (R.BINOMIAL, 0, 0, 1.0),
             (R.BINOMIAL, (1 << 53) - 1, 0, 0.0), (R.GEOMETRIC, 0, 0, 0.25), (R.GEOMETRIC, 0, 0, 1.0)]
    frames = []
    for kind, a, b, p in cases:
        frames += [rand_int(kind, Y, N, a, b, p), read(Y), rand_int(kind, SHORT, N - 1, a, b, p), rand_int(kind, Y, 0, a, b, p)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(rows)
    for i, (kind, a, b, p) in enumerate(cases):
        v = np.frombuffer(rows[4 * i + 1][4], np.int64)
        lo, hi = {R.INTEGERS: (a, b - 1), R.POISSON: (0, MAX), R.BINOMIAL: (0, a), R.GEOMETRIC: (1, MAX)}[kind]
        assert v.min() >= lo and v.max() <= hi, (kind, v)
    # a partial write of a fresh buffer is preceded by its lazy scrub: zeros behind the draw
    rows = rows_of(fuzz_bin, [rand_int(R.GEOMETRIC, Y, 3, 0, 0, 0.5), read(Y)])
    v = np.frombuffer(rows[1][4], np.int64)
    assert (v[:3] >= 1).all() and not v[3:].any()


# ---- refusals against a model of the validation ---------------------------------------------------------------

def _i64(u):
    return u - (1 << 64) if u >= 1 << 63 else u


def _fits(h, n, esize):
    """The core's bounds rule: n >= 0, n * esize without overflow, the handle known and large enough."""
    return 0 <= n and n * esize < 1 << 64 and h in SIZES and n * esize <= SIZES[h]


def _cast_sizes(s, d):
    size = {R.F32: 4, R.F64: 8, R.I64: 8, R.BOOL: 1}
    return (size[s], size[d]) if (s, d) in R.CAST_PAIRS else None


def model_status(op, payload):
    """The status the protocol core gives a frame (csrc/executor/broker_core.cpp): a short payload is a protocol
    error; codes and parameters are judged before handles; then handles and sizes."""
    full = {RAND_INT: 64, INT_BINARY: 48, INT_COMPARE: 48, INT_REDUCE: 24, INT_CAST: 32}[op]
    if len(payload) < full:
        return PROTOCOL
    if op == RAND_INT:
        kind, _, h, n, _, _, a, b, p = struct.unpack_from("<IIQqQQqqd", payload)
        if kind >= 4 or not R.params_ok(kind, a, b, p):
            return BAD_ARG
        return OK if _fits(h, n, 8) else BAD_HANDLE
    if op in (INT_BINARY, INT_COMPARE):
        code, mode, a, b, _, y, n = struct.unpack_from("<IIQQqQq", payload)
        if op == INT_BINARY:
            if code >= 7 or mode > 2:
                return BAD_ARG
            ok = _fits(a, n, 8) and _fits(y, n, 8) and (mode != 0 or _fits(b, n, 8))
        else:
            if code > 5 or mode > 1:
                return BAD_ARG
            ok = _fits(a, n, 8) and (mode != 0 or _fits(b, n, 8)) and _fits(y, n, 1) and y != a and (mode != 0 or y != b)
        return OK if ok else BAD_HANDLE
    if op == INT_REDUCE:
        code, _, a, n = struct.unpack_from("<IIQq", payload)
        if code >= 3:
            return BAD_ARG
        return OK if _fits(a, n, 8) else BAD_HANDLE
    s, d, x, y, n = struct.unpack_from("<IIQQq", payload)
    sizes = _cast_sizes(s, d)
    if sizes is None:
        return BAD_ARG
    return OK if _fits(x, n, sizes[0]) and _fits(y, n, sizes[1]) and x != y else BAD_HANDLE


def check_against_model(fuzz_bin, frames):
    rows = rows_of(fuzz_bin, frames)
    assert len(rows) == len(frames)
    want = [model_status(struct.unpack_from("<I", f)[0], f[16:]) for f in frames]
    got = [r[1] for r in rows]
    assert got == want, [(i, g, w, frames[i][16:].hex()) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    for r, w in zip(rows, want):  # a reduce that ran replies its one i64, the others nothing (a refusal: its text)
        assert w != OK or r[2] == (8 if r[0] == INT_REDUCE else 0)
    return want


def test_hostile_frames_get_the_documented_status(fuzz_bin):
    nan, inf = float("nan"), float("inf")
    n_wrap = (1 << 61) + 1  # * 8 wraps to 8
    bad_arg = [
        rand_int(4, Y, N, 0, 6, 0.5), rand_int((1 << 32) - 1, Y, N, 0, 6, 0.5), rand_int(R.INTEGERS, Y, N, 6, 6, 0.0),
        rand_int(R.INTEGERS, Y, N, 7, 6, 0.0), rand_int(R.INTEGERS, Y, N, MAX, MIN, 0.0), rand_int(R.POISSON, Y, N, 0, 0, -1e-300),
        rand_int(R.POISSON, Y, N, 0, 0, nan), rand_int(R.POISSON, Y, N, 0, 0, inf), rand_int(R.POISSON, Y, N, 0, 0, 2.0 ** 53 + 2),
        rand_int(R.BINOMIAL, Y, N, -1, 0, 0.5), rand_int(R.BINOMIAL, Y, N, 1 << 53, 0, 0.5), rand_int(R.BINOMIAL, Y, N, 5, 0, -0.1),
        rand_int(R.BINOMIAL, Y, N, 5, 0, 1.0000001), rand_int(R.BINOMIAL, Y, N, 5, 0, nan), rand_int(R.GEOMETRIC, Y, N, 0, 0, 0.0),
        rand_int(R.GEOMETRIC, Y, N, 0, 0, -0.5), rand_int(R.GEOMETRIC, Y, N, 0, 0, 1.5), rand_int(R.GEOMETRIC, Y, N, 0, 0, nan),
        rand_int(R.POISSON, 999, -1, 0, 0, -1.0),  # the parameters are judged before the handle
        int_binary(7, 0, A, B, 0, Y, N), int_binary((1 << 32) - 1, 0, A, B, 0, Y, N), int_binary(0, 3, A, B, 0, Y, N),
        int_compare(6, 0, A, B, 0, MASK, N), int_compare(0, 2, A, B, 0, MASK, N), int_reduce(3, A, N), int_reduce(1 << 31, A, N),
        int_cast(R.I64, R.I64, A, Y, N), int_cast(R.I64, 2, A, Y, N), int_cast(2, R.I64, A, Y, N), int_cast(R.I64, R.BOOL, A, MASK, N),
        int_cast(R.F64, R.F32, F64, F32, N), int_cast(R.BOOL, R.F64, MASK, F64, N), int_cast(4, R.I64, A, Y, N), int_cast(3, R.I64, A, Y, N),
    ]
    bad_handle = [
        rand_int(R.INTEGERS, SHORT, N, 0, 6, 0.0), rand_int(R.INTEGERS, Y, N + 1, 0, 6, 0.0), rand_int(R.POISSON, Y, -1, 0, 0, 3.0),
        rand_int(R.POISSON, Y, n_wrap, 0, 0, 3.0), rand_int(R.POISSON, 999, N, 0, 0, 3.0), rand_int(R.POISSON, MASK, 2, 0, 0, 3.0),
        int_binary(0, 0, A, SHORT, 0, Y, N), int_binary(0, 0, SHORT, B, 0, Y, N), int_binary(0, 0, A, B, 0, SHORT, N),
        int_binary(0, 0, A, 999, 0, Y, N), int_binary(0, 1, A, 0, 0, Y, -1), int_binary(0, 2, A, 0, 0, Y, n_wrap),
        int_binary(0, 1, MASK, 0, 0, Y, 2),
        int_compare(0, 0, A, B, 0, A, N), int_compare(0, 0, A, B, 0, B, N), int_compare(0, 1, A, 0, 0, A, N),
        int_compare(0, 0, A, SHORT, 0, MASK, N), int_compare(0, 1, A, 0, 0, MASK, N + 1), int_compare(0, 1, A, 0, 0, 999, N),
        int_compare(0, 1, A, 0, 0, MASK, -1), int_compare(0, 1, A, 0, 0, MASK, n_wrap),
        int_reduce(0, SHORT, N), int_reduce(0, A, -1), int_reduce(0, A, n_wrap), int_reduce(0, 999, 0), int_reduce(0, MASK, 2),
        int_cast(R.I64, R.F64, A, A, N), int_cast(R.I64, R.F64, SHORT, F64, N), int_cast(R.I64, R.F32, A, F32, N + 1),
        int_cast(R.BOOL, R.I64, MASK, SHORT, N), int_cast(R.F32, R.I64, F32, Y, N + 1), int_cast(R.F64, R.I64, F64, Y, -1),
        int_cast(R.F64, R.I64, F64, Y, n_wrap), int_cast(R.BOOL, R.I64, 999, Y, N),
    ]
    want = check_against_model(fuzz_bin, bad_arg + bad_handle)
    assert want == [BAD_ARG] * len(bad_arg) + [BAD_HANDLE] * len(bad_handle)
    # the ops that take a mode-1 / mode-2 scalar ignore the b handle; a mask may not be an operand's buffer only
    ok = [int_binary(0, 1, A, 999, 0, Y, N), int_binary(0, 2, A, SHORT, 0, A, N), int_compare(0, 1, A, MASK, 0, MASK, N),
          int_cast(R.I64, R.F32, A, Y, N), int_reduce(2, SHORT, N - 1)]
    assert check_against_model(fuzz_bin, ok) == [OK] * len(ok)


def test_no_other_op_takes_int64(fuzz_bin):
    """dtype 5 stays refused by every float op; the int ops take no dtype at all."""
    unary, binary, cast, reduce_, compare = 7, 8, 9, 11, 22
    frames = [frame(unary, struct.pack("<IIQQq", 0, 5, A, Y, N)), frame(binary, struct.pack("<IIIIQQdQq", 0, 5, 0, 0, A, B, 0.0, Y, N)),
              frame(cast, struct.pack("<IIQQq", 5, 1, A, Y, N)), frame(cast, struct.pack("<IIQQq", 1, 5, A, Y, N)),
              frame(reduce_, struct.pack("<IIQQq", 0, 5, A, 0, N)),
              frame(compare, struct.pack("<IIIIQQdQq", 0, 5, 1, 0, A, 0, 0.0, MASK, N))]
    rows = rows_of(fuzz_bin, frames)
    assert all(r[1] in (BAD_ARG, BAD_HANDLE) for r in rows), [r[1] for r in rows]


def test_short_frames_are_protocol_errors(fuzz_bin):
    whole = {RAND_INT: rand_int(R.POISSON, Y, N, 0, 0, 3.0), INT_BINARY: int_binary(0, 0, A, B, 0, Y, N),
             INT_COMPARE: int_compare(0, 0, A, B, 0, MASK, N), INT_REDUCE: int_reduce(0, A, N),
             INT_CAST: int_cast(R.I64, R.F64, A, F64, N)}
    frames = [frame(op, f[16:16 + cut]) for op, f in whole.items() for cut in (0, 3, 4, 8, 16, 23, len(f) - 17)]
    want = check_against_model(fuzz_bin, frames)
    assert want == [PROTOCOL] * len(frames)
    longer = [frame(op, f[16:] + b"\0" * 8) for op, f in whole.items()]  # trailing bytes are ignored, as by the other ops
    assert check_against_model(fuzz_bin, longer) == [OK] * len(longer)


def _random_int_frames(seed: int, count: int):
    rnd = random.Random(seed)
    handles = list(SIZES) + [999, 0]
    sizes = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 64, 2**31, 2**61, 2**61 + 1, 2**62 + 4, 2**63 - 1, 2**63, 2**64 - 1]
    ints = [0, 1, -1, 5, 6, 7, 10, MIN, MAX, 1 << 53, (1 << 53) - 1, -(1 << 53), 1 << 32, (1 << 32) + 1]
    probs = [0.0, -0.0, 0.5, 1.0, 0.25, 3.0, 10.0, 1e4, 2.0 ** 53, 2.0 ** 54, 1e-300, -1e-300, -1.0, 1.0000001,
             float("nan"), float("inf"), -float("inf")]
    codes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 2**31, 2**32 - 1]
    out = []
    for _ in range(count):
        op = rnd.choice([RAND_INT, INT_BINARY, INT_COMPARE, INT_REDUCE, INT_CAST])
        n = rnd.choice(sizes) if rnd.random() < 0.85 else rnd.getrandbits(64)
        h = lambda: rnd.choice(handles)  # noqa: E731
        if op == RAND_INT:
            payload = struct.pack("<IIQQQQqqd", rnd.choice(codes[:6] * 3 + codes), rnd.getrandbits(32), h(), n,
                                  rnd.getrandbits(64), rnd.getrandbits(64), rnd.choice(ints), rnd.choice(ints),
                                  rnd.choice(probs) if rnd.random() < 0.8 else rnd.uniform(-0.5, 1.5))
        elif op in (INT_BINARY, INT_COMPARE):
            payload = struct.pack("<IIQQqQQ", rnd.choice(codes), rnd.choice([0, 0, 1, 1, 2, 3, 2**32 - 1]), h(), h(),
                                  rnd.choice(ints), h(), n)
        elif op == INT_REDUCE:
            payload = struct.pack("<IIQQ", rnd.choice(codes), rnd.getrandbits(32), h(), n)
        else:
            s, d = rnd.choice(R.CAST_PAIRS) if rnd.random() < 0.7 else (rnd.choice(codes), rnd.choice(codes))
            payload = struct.pack("<IIQQQ", s, d, h(), h(), n)
        if rnd.random() < 0.05:
            payload = payload[: rnd.randrange(0, len(payload) + 1)]
        out.append(frame(op, payload))
    return out


@pytest.mark.parametrize("seed", [41, 42])
def test_random_int_frames_match_the_model_with_no_sanitizer_findings(fuzz_bin, seed):
    want = check_against_model(fuzz_bin, _random_int_frames(seed, 3000))
    assert len(want) == 3000 and {OK, BAD_ARG, BAD_HANDLE, PROTOCOL} <= set(want)
    assert want.count(OK) > 100  # the stream reaches the device model often


def test_a_refused_op_leaves_its_output_to_the_lazy_scrub(fuzz_bin):
    # a fresh buffer holds another tenant's bytes; a refused op writes nothing, so a read scrubs first
    frames = [rand_int(R.POISSON, Y, N, 0, 0, -1.0), int_binary(9, 0, A, B, 0, Y, N), int_cast(R.I64, R.BOOL, A, Y, N), read(Y)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [BAD_ARG] * 3 + [OK] and rows[3][4] == bytes(64)


def test_client_methods_speak_the_protocol(fuzz_bin, tmp_path, monkeypatch):
    """The real BrokerDriver's five methods against the daemon's frame reader and the protocol core."""
    from bee_code_interpreter_fs_amd.ops import driver as drv_mod
    from bee_code_interpreter_fs_amd.ops.driver import BeekernError, BrokerDriver

    assert (drv_mod.RAND_INT, drv_mod.INT_BINARY, drv_mod.INT_COMPARE, drv_mod.INT_REDUCE, drv_mod.INT_CAST) == \
        (RAND_INT, INT_BINARY, INT_COMPARE, INT_REDUCE, INT_CAST)
    monkeypatch.chdir(tmp_path)  # (a relative socket name: sun_path holds 108 bytes)
    p = _serve(fuzz_bin, "i.sock")
    d = BrokerDriver("i.sock")
    d.init(0)
    n = 5003
    rng = np.random.Generator(np.random.PCG64(2))
    ha = rng.integers(MIN, MAX, n, dtype=np.int64, endpoint=True)
    hb = rng.integers(-9, 10, n, dtype=np.int64)
    a, b, y, m, f = d.malloc(n * 8), d.malloc(n * 8), d.malloc(n * 8), d.malloc(n), d.malloc(n * 4)
    d.h2d(a, ha), d.h2d(b, hb)
    got = np.empty(n, np.int64)
    for op in range(7):
        d.int_binary(op, 0, a, b, 0, y, n)
        d.d2h(y, got)
        np.testing.assert_array_equal(got, R.binary(op, ha, hb))
    d.int_binary(R.REMAINDER, 2, b, 0, MIN, y, n)
    d.d2h(y, got)
    np.testing.assert_array_equal(got, R.binary(R.REMAINDER, MIN, hb))
    mask = np.empty(n, np.uint8)
    d.int_compare(0, 1, b, 0, -2, m, n)
    d.d2h(m, mask)
    np.testing.assert_array_equal(mask, hb < -2)
    assert [d.int_reduce(op, a, n) for op in range(3)] == [R.reduce(op, ha) for op in range(3)]
    assert isinstance(d.int_reduce(0, a, 0), int) and d.int_reduce(1, a, 0) == MIN
    f32 = np.empty(n, np.float32)
    d.int_cast(R.I64, R.F32, a, f, n)
    d.d2h(f, f32)
    assert f32.tobytes() == ha.astype(np.float32).tobytes()
    d.rand_int(R.INTEGERS, y, n, SEED, 3, -5, 5, 0.0)
    d.d2h(y, got)
    assert got.min() >= -5 and got.max() < 5 and len(set(got.tolist())) == 10
    d.rand_int(R.POISSON, y, n, SEED, 0, 0, 0, -1.0)  # fire-and-forget: the refusal arrives with the next reply
    with pytest.raises(BeekernError, match="bad argument.*bk.rand_int"):
        d.sync()
    d.int_binary(0, 0, a, b, 0, y, n + 1)
    with pytest.raises(BeekernError, match="bad handle.*bk.int_binary"):
        d.sync()
    with pytest.raises(BeekernError, match="bad argument"):
        d.int_reduce(5, a, n)
    d.sync()
    d.sock.close()
    assert _finish(p)["live"] == "0"

"""The kernel broker's SORT, ARG_REDUCE and TAKE ops against well-formed and
hostile frames, on CPU: the protocol core over the host-memory device of
``bee-broker-fuzz`` under ASan + UBSan (tests/test_broker_fuzz_cpu.py has the
harness's story).  The host device computes real answers (a stable sort under
numpy's order), so read-backs are checked against tests/sort_ref.py; every
refusal is checked against a Python model of the core's validation, and a wrong
bound in the core is a sanitizer report.  The three ops are never part of a
fused pair (tests/test_broker_fuse_cpu.py's launch log)."""

from __future__ import annotations

import random
import struct

import numpy as np
import pytest

from bee_code_interpreter_fs_amd.ops import driver as drv_mod

from . import sort_ref as R
from .test_broker_fuse_cpu import Broker, _launches, alloc_at, fill, post, reduce_axis, sync
from .test_broker_fuzz_cpu import (ALLOC_AT, BAD_ARG, BAD_HANDLE, OK, PROTOCOL, READ, WRITE, _finish, _serve,  # noqa: F401
                                   frame, fuzz_bin, run)

SORT, ARG_REDUCE, TAKE = 37, 38, 39
F32, F64, BF16, I64, BOOL = 0, 1, 2, 5, 6
ESIZE = {F32: 4, F64: 8, BF16: 2, I64: 8}
N = 8  # elements: 64 bytes of f64 / int64, what one echoed READ returns
WS_BYTES = drv_mod.sort_workspace_bytes(F64, N, True)  # (the largest of the dtypes at N)
X, S, IDX, WS, SHORT, SHORT_WS, OUT, X2 = 1, 2, 3, 4, 5, 6, 7, 8  # client handles
SIZES = {X: N * 8, S: N * 8, IDX: N * 8, WS: WS_BYTES, SHORT: N * 8 - 1, SHORT_WS: drv_mod.sort_workspace_bytes(BF16, N, False) - 1,
         OUT: N * 8, X2: N * 8}
MAX_SORT_N = 0x7FFFFFFF


def sort(dt, flags, x, n, s, i, ws):
    return frame(SORT, struct.pack("<IIQqQQQ", dt, flags, x, n, s, i, ws))


def arg_reduce(op, dt, x, n):
    return frame(ARG_REDUCE, struct.pack("<IIQq", op, dt, x, n))


def take(dt, x, n, idx, m, out, pad=0):
    return frame(TAKE, struct.pack("<IIQqQqQ", dt, pad, x, n, idx, m, out))


def write(h, host):
    return frame(WRITE, struct.pack("<QQ", h, 0) + np.ascontiguousarray(host).tobytes())


def read(h, nbytes):
    return frame(READ, struct.pack("<QQQ", h, 0, nbytes))


def setup_frames():
    return [frame(ALLOC_AT, struct.pack("<QQ", h, size)) for h, size in SIZES.items()]


def rows_of(fuzz_bin, frames):
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[:len(SIZES)]] == [OK] * len(SIZES)
    return rows[len(SIZES):]


def host_data(dt):
    f = np.array([3.5, -0.0, np.nan, 0.0, -np.inf, 3.5, np.inf, np.nan])
    if dt == I64:
        return np.array([5, -7, 0, R.I64_MAX, R.I64_MIN, 5, -1, 0], np.int64), "i64"
    if dt == BF16:
        bits = R.bf16_bits(f)
        bits[7] |= 0x8000  # a negative NaN
        return bits, "bf16"
    a = f.astype(np.float32 if dt == F32 else np.float64)
    a.view(np.uint8).reshape(N, -1)[7, -1] |= 0x80
    return a, ("f32" if dt == F32 else "f64")


# ---- results through the host device ---------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F32, F64, BF16, I64])
def test_sort_and_arg_reduce_read_back_numpys_answers(fuzz_bin, dt):
    a, name = host_data(dt)
    es = ESIZE[dt]
    frames = [write(X, a), sort(dt, 3, X, N, S, IDX, WS), read(S, N * es), read(IDX, N * 8), read(X, N * es),
              sort(dt, 1, X, N, OUT, 999, WS), read(OUT, N * es), sort(dt, 2, X, N, 999, OUT, WS), read(OUT, N * 8),
              sort(dt, 3, X, 0, S, IDX, WS), sort(dt, 3, X, 1, S, IDX, WS), read(IDX, 8),
              arg_reduce(0, dt, X, N), arg_reduce(1, dt, X, N), arg_reduce(0, dt, X, 1), arg_reduce(1, dt, X, 2)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(rows)
    order = R.argsort(a, name)
    vals = R.as_values(a, name)
    assert np.array_equal(order, np.argsort(vals, kind="stable"))
    got_sorted = np.frombuffer(rows[2][4], a.dtype)
    np.testing.assert_array_equal(R.as_values(got_sorted, name), np.sort(vals))
    assert np.array_equal(np.frombuffer(rows[3][4], np.int64), order)
    assert rows[4][4] == a.tobytes()  # x is only read
    assert rows[6][4] == rows[2][4] and rows[8][4] == rows[3][4]
    assert struct.unpack("<q", rows[11][4])[0] == 0
    got = [struct.unpack("<q", r[4])[0] for r in rows[12:16]]
    assert got == [int(np.argmax(vals)), int(np.argmin(vals)), 0, int(np.argmin(vals[:2]))]
    assert got[:2] == [R.argmax(a, name), R.argmin(a, name)]


@pytest.mark.parametrize("dt", [F32, F64, BF16, I64, BOOL])
def test_take_reads_back_the_gather_and_the_bad_count(fuzz_bin, dt):
    es = 1 if dt == BOOL else ESIZE[dt]
    x = (np.arange(N) + 1).astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[es])
    good = np.array([0, -1, N - 1, -N], np.int64)
    bad = np.array([N, -N - 1, R.I64_MIN, R.I64_MAX], np.int64)
    frames = [write(X, x), write(IDX, np.concatenate([good, bad])), take(dt, X, N, IDX, 4, OUT), read(OUT, 4 * es),
              take(dt, X, N, IDX, 8, OUT), read(OUT, 8 * es), take(dt, X, N, IDX, 0, OUT), take(dt, X, 0, IDX, 2, OUT),
              read(OUT, 2 * es)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(rows)
    want, nbad = R.take(x, good)
    assert struct.unpack("<q", rows[2][4])[0] == nbad == 0 and rows[3][4] == want.tobytes() == x[good].tobytes()
    want, nbad = R.take(x, np.concatenate([good, bad]))
    assert struct.unpack("<q", rows[4][4])[0] == nbad == 4 and rows[5][4] == want.tobytes()
    assert struct.unpack("<q", rows[6][4])[0] == 0
    assert struct.unpack("<q", rows[7][4])[0] == 2 and rows[8][4] == bytes(2 * es)  # nothing is in range of an empty x


# ---- refusals against a model of the validation ---------------------------------------------------------------

def _fits(h, nbytes):
    return h in SIZES and nbytes <= SIZES[h]


def model_status(op, payload):
    """The status the protocol core gives a frame (csrc/executor/broker_core.cpp): a short payload is a protocol
    error; codes, flags and counts are judged before handles; then handles, sizes and aliasing."""
    full = {SORT: 48, ARG_REDUCE: 24, TAKE: 48}[op]
    if len(payload) < full:
        return PROTOCOL
    if op == SORT:
        dt, flags, x, n, s, i, ws = struct.unpack_from("<IIQqQQQ", payload)
        if dt not in ESIZE or flags not in (1, 2, 3) or not 0 <= n <= MAX_SORT_N:
            return BAD_ARG
        ok = _fits(x, n * ESIZE[dt]) and _fits(ws, drv_mod.sort_workspace_bytes(dt, n, bool(flags & 2))) and ws != x
        outs = []
        if flags & 1:
            ok = ok and _fits(s, n * ESIZE[dt])
            outs.append(s)
        if flags & 2:
            ok = ok and _fits(i, n * 8)
            outs.append(i)
        ok = ok and len({x, ws, *outs}) == 2 + len(outs)
        return OK if ok else BAD_HANDLE
    if op == ARG_REDUCE:
        code, dt, x, n = struct.unpack_from("<IIQq", payload)
        if code > 1 or dt not in ESIZE or n < 1:
            return BAD_ARG
        return OK if _fits(x, n * ESIZE[dt]) else BAD_HANDLE
    dt, pad, x, n, idx, m, out = struct.unpack_from("<IIQqQqQ", payload)
    es = 1 if dt == BOOL else ESIZE.get(dt)
    if es is None or pad != 0 or n < 0 or m < 0:
        return BAD_ARG
    ok = _fits(x, n * es) and _fits(idx, m * 8) and _fits(out, m * es) and out != x and out != idx
    return OK if ok else BAD_HANDLE


def check_against_model(fuzz_bin, frames, data=()):
    rows = rows_of(fuzz_bin, list(data) + frames)[len(data):]
    assert len(rows) == len(frames)
    want = [model_status(struct.unpack_from("<I", f)[0], f[16:]) for f in frames]
    got = [r[1] for r in rows]
    assert got == want, [(i, g, w, frames[i][16:].hex()) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    for r, w in zip(rows, want):  # SORT replies nothing, the other two one i64 (a refusal: its text)
        assert w != OK or r[2] == (0 if r[0] == SORT else 8)
    return want


def test_hostile_frames_get_the_documented_status(fuzz_bin):
    big = 1 << 61
    bad_arg = [
        sort(3, 3, X, N, S, IDX, WS), sort(4, 3, X, N, S, IDX, WS), sort(BOOL, 3, X, N, S, IDX, WS), sort(7, 1, X, N, S, IDX, WS),
        sort((1 << 32) - 1, 3, X, N, S, IDX, WS), sort(F64, 0, X, N, S, IDX, WS), sort(F64, 4, X, N, S, IDX, WS),
        sort(F64, 7, X, N, S, IDX, WS), sort(F64, 3, X, -1, S, IDX, WS), sort(F64, 3, X, MAX_SORT_N + 1, S, IDX, WS),
        sort(F64, 3, X, big, S, IDX, WS), sort(F64, 3, 999, -1, 999, 999, 999),  # the count is judged before the handles
        arg_reduce(2, F64, X, N), arg_reduce((1 << 32) - 1, F64, X, N), arg_reduce(0, 3, X, N), arg_reduce(0, BOOL, X, N),
        arg_reduce(0, F64, X, 0), arg_reduce(1, F64, X, -1), arg_reduce(0, 9, 999, 0),
        take(3, X, N, IDX, 4, OUT), take(4, X, N, IDX, 4, OUT), take(7, X, N, IDX, 4, OUT), take(F64, X, -1, IDX, 4, OUT),
        take(F64, X, N, IDX, -1, OUT), take(F64, X, N, IDX, 4, OUT, pad=1), take(F64, X, -(1 << 63), IDX, 4, OUT),
    ]
    bad_handle = [
        sort(F64, 3, SHORT, N, S, IDX, WS), sort(F64, 3, X, N, SHORT, IDX, WS), sort(F64, 3, X, N, S, SHORT, WS),
        sort(F64, 3, X, N, S, IDX, SHORT_WS), sort(BF16, 1, X, N, S, IDX, SHORT_WS), sort(F64, 3, X, N, S, IDX, X2),  # short ws
        sort(F64, 3, 999, N, S, IDX, WS), sort(F64, 1, X, N, 999, IDX, WS), sort(F64, 2, X, N, S, 999, WS),
        sort(F64, 3, X, N, S, IDX, 999), sort(F64, 3, X, N + 1, S, IDX, WS), sort(F64, 3, X, MAX_SORT_N, S, IDX, WS),
        sort(F64, 3, X, N, X, IDX, WS), sort(F64, 3, X, N, S, X, WS), sort(F64, 3, X, N, S, S, WS), sort(F64, 3, X, N, S, IDX, X),
        sort(F64, 3, X, N, WS, IDX, WS), sort(F64, 3, X, N, S, WS, WS), sort(F64, 3, WS, N, S, IDX, WS), sort(F64, 2, X, N, S, X, WS),
        arg_reduce(0, F64, SHORT, N), arg_reduce(0, F64, X, N + 1), arg_reduce(0, F64, 999, 1), arg_reduce(1, I64, X, big + 1),
        arg_reduce(0, BF16, X, 4 * N + 1),
        take(F64, SHORT, N, IDX, 4, OUT), take(F64, X, N, SHORT, N, OUT), take(F64, X, N, IDX, N, SHORT), take(F64, X, N, IDX, N + 1, OUT),
        take(F64, X, N + 1, IDX, 4, OUT), take(F64, 999, N, IDX, 4, OUT), take(F64, X, N, 999, 4, OUT), take(F64, X, N, IDX, 4, 999),
        take(F64, X, N, IDX, 4, X), take(F64, X, N, IDX, 4, IDX), take(F64, X, big + 1, IDX, 4, OUT), take(F64, X, N, IDX, big + 1, OUT),
        take(BOOL, X, 8 * N + 1, IDX, 4, OUT),
    ]
    want = check_against_model(fuzz_bin, bad_arg + bad_handle)
    assert want == [BAD_ARG] * len(bad_arg) + [BAD_HANDLE] * len(bad_handle)
    # an absent output's handle is ignored (it may even name x); a larger scratch is fine; n = 0 sorts nothing
    ok = [sort(F64, 1, X, N, S, X, WS), sort(F64, 2, X, N, X, IDX, WS), sort(F32, 3, X, N, S, IDX, WS), sort(BF16, 1, X, 4 * N, S, IDX, WS),
          sort(F64, 3, X, 0, S, IDX, WS), sort(BF16, 1, SHORT, N, S, 0, WS), take(BOOL, X, 8 * N, IDX, N, OUT), take(I64, X, N, IDX, 0, OUT),
          arg_reduce(1, BF16, X, 4 * N)]
    assert check_against_model(fuzz_bin, ok) == [OK] * len(ok)


def test_short_frames_are_protocol_errors(fuzz_bin):
    whole = {SORT: sort(F64, 3, X, N, S, IDX, WS), ARG_REDUCE: arg_reduce(0, F64, X, N), TAKE: take(F64, X, N, IDX, 4, OUT)}
    frames = [frame(op, f[16:16 + cut]) for op, f in whole.items() for cut in (0, 3, 4, 8, 16, 23, len(f) - 17)]
    assert check_against_model(fuzz_bin, frames) == [PROTOCOL] * len(frames)
    longer = [frame(op, f[16:] + b"\0" * 8) for op, f in whole.items()]  # trailing bytes are ignored, as by the other ops
    assert check_against_model(fuzz_bin, longer) == [OK] * len(longer)


def _random_frames(seed: int, count: int):
    rnd = random.Random(seed)
    handles = list(SIZES) * 2 + [999, 0]
    counts = [0, 1, 2, 3, 7, 8, 15, 16, 17, 32, 64, 65, -1, -16, MAX_SORT_N, MAX_SORT_N + 1, 2**31, 2**61, 2**61 + 1, 2**62 + 4,
              2**63 - 1, -(2**63)]
    codes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 2**31, 2**32 - 1]
    out = []
    for _ in range(count):
        op = rnd.choice([SORT, ARG_REDUCE, TAKE])
        n = rnd.choice(counts[:10] * 3 + counts) if rnd.random() < 0.9 else rnd.getrandbits(63) - (1 << 62)
        h = lambda: rnd.choice(handles)  # noqa: E731
        if op == SORT:
            payload = struct.pack("<IIQqQQQ", rnd.choice([0, 1, 2, 5] * 4 + codes), rnd.choice([1, 2, 3] * 4 + codes), h(), n, h(), h(),
                                  rnd.choice([WS] * 3 + handles))
        elif op == ARG_REDUCE:
            payload = struct.pack("<IIQq", rnd.choice([0, 1] * 4 + codes), rnd.choice([0, 1, 2, 5] * 4 + codes), h(), n)
        else:
            payload = struct.pack("<IIQqQqQ", rnd.choice([0, 1, 2, 5, 6] * 4 + codes), rnd.choice([0] * 9 + [1]), h(), n, h(),
                                  rnd.choice(counts[:10] * 3 + counts), h())
        if rnd.random() < 0.05:
            payload = payload[: rnd.randrange(0, len(payload) + 1)]
        out.append(frame(op, payload))
    return out


@pytest.mark.parametrize("seed", [51, 52])
def test_a_storm_of_hostile_frames_matches_the_model_with_no_sanitizer_findings(fuzz_bin, seed):
    # the index buffer holds hostile indices too: the device model never reads through one
    idx = np.array([0, -1, N, -N - 1, R.I64_MIN, R.I64_MAX, 5, 1 << 40], np.int64)
    data = [write(h, idx) for h in (X, S, IDX, OUT, X2)]
    want = check_against_model(fuzz_bin, _random_frames(seed, 3000), data)
    assert len(want) == 3000 and {OK, BAD_ARG, BAD_HANDLE, PROTOCOL} <= set(want)
    assert want.count(OK) > 100  # the stream reaches the device model often


def test_a_refused_sort_leaves_its_outputs_to_the_lazy_scrub(fuzz_bin):
    frames = [sort(F64, 3, X, N, S, IDX, SHORT_WS), sort(9, 3, X, N, S, IDX, WS), take(F64, X, N, IDX, 4, X), read(S, N * 8),
              read(IDX, N * 8)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [BAD_HANDLE, BAD_ARG, BAD_HANDLE, OK, OK]
    assert rows[3][4] == bytes(N * 8) == rows[4][4]


# ---- the plan ---------------------------------------------------------------------------------------------------

def test_the_three_ops_are_never_fused(fuzz_bin, tmp_path):
    """A reduce_axis followed by an arg-reduction, a sort or a gather of its whole output -- the place a cast or a
    closing reduce would be fused at -- goes out as two launches each; and none of the three is a producer for the
    reduce that follows it."""
    REDUCE = 11
    C, ROWS, ORD, SORTED, SCRATCH = 1, 2, 3, 4, 5
    R_ = 64
    b = Broker(fuzz_bin, tmp_path)
    st, _ = b.call(alloc_at(C, 4 * R_ * R_), fill(C, 4 * R_ * R_), alloc_at(ROWS, 4 * R_), alloc_at(ORD, 8 * R_),
                   alloc_at(SORTED, 4 * R_), alloc_at(SCRATCH, drv_mod.sort_workspace_bytes(F32, R_, True)), sync())
    assert st == OK
    n0 = 1
    st, v = b.call(reduce_axis(C, ROWS, R_, R_, 1), frame(ARG_REDUCE, struct.pack("<IIQq", 0, F32, ROWS, R_)))
    assert st == OK and len(v) == 8
    st, _ = b.call(reduce_axis(C, ROWS, R_, R_, 1), post(SORT, struct.pack("<IIQqQQQ", F32, 3, ROWS, R_, SORTED, ORD, SCRATCH)),
                   frame(REDUCE, struct.pack("<IIQQq", 0, F32, SORTED, 0, R_)))
    assert st == OK
    st, v = b.call(reduce_axis(C, ROWS, R_, R_, 1), frame(TAKE, struct.pack("<IIQqQqQ", F32, 0, ROWS, R_, ORD, R_, SORTED)))
    assert st == OK and struct.unpack("<q", v)[0] == 0
    st, _ = b.call(post(TAKE, struct.pack("<IIQqQqQ", F32, 0, ROWS, R_, ORD, R_, SORTED)),
                   frame(REDUCE, struct.pack("<IIQQq", 0, F32, SORTED, 0, R_)))
    assert st == OK
    assert _launches(b, n0) == ["reduce_axis", "arg_reduce", "reduce_axis", "sort", "reduce", "reduce_axis", "take", "take",
                                "reduce"]


# ---- the client ---------------------------------------------------------------------------------------------------

def test_client_methods_speak_the_protocol(fuzz_bin, tmp_path, monkeypatch):
    """The real BrokerDriver's three methods against the daemon's frame reader and the protocol core."""
    from bee_code_interpreter_fs_amd.ops.driver import BeekernError, BrokerDriver

    assert (drv_mod.SORT, drv_mod.ARG_REDUCE, drv_mod.TAKE) == (SORT, ARG_REDUCE, TAKE)
    monkeypatch.chdir(tmp_path)  # (a relative socket name: sun_path holds 108 bytes)
    p = _serve(fuzz_bin, "s.sock")
    d = BrokerDriver("s.sock")
    d.init(0)
    n = 5003
    rng = np.random.Generator(np.random.PCG64(4))
    h = rng.standard_normal(n)
    h[::50], h[1::70], h[2::90] = np.nan, 0.0, -0.0
    x, s, i, o = d.malloc(n * 8), d.malloc(n * 8), d.malloc(n * 8), d.malloc(n * 8)
    ws = d.malloc(drv_mod.sort_workspace_bytes(F64, n, True))
    d.h2d(x, h)
    d.sort(F64, x, n, s, i, ws)
    got_s, got_i = np.empty(n), np.empty(n, np.int64)
    d.d2h(s, got_s), d.d2h(i, got_i)
    assert np.array_equal(got_i, np.argsort(h, kind="stable")) and np.array_equal(got_i, R.argsort(h, "f64"))
    np.testing.assert_array_equal(got_s, np.sort(h))
    d.sort(F64, x, n, 0, i, ws), d.sort(F64, x, n, s, 0, ws)
    assert d.arg_reduce(0, F64, x, n) == int(np.argmax(h)) and d.arg_reduce(1, F64, x, n) == int(np.argmin(h))
    assert isinstance(d.arg_reduce(0, F64, x, 1), int)
    assert d.take(F64, x, n, i, n, o) == 0
    d.d2h(o, got_s)
    np.testing.assert_array_equal(got_s, np.sort(h))
    d.h2d(i, np.array([0, n, -n - 1, -1], np.int64))
    assert d.take(F64, x, n, i, 4, o) == 2
    d.sort(F64, x, n, s, i, x)  # fire-and-forget: the refusal arrives with the next reply
    with pytest.raises(BeekernError, match="bad handle.*bk.sort"):
        d.sync()
    with pytest.raises(BeekernError, match="bad argument"):
        d.arg_reduce(0, F64, x, 0)
    with pytest.raises(BeekernError, match="bad handle"):
        d.take(F64, x, n, i, n, x)
    d.sync()
    d.sock.close()
    assert _finish(p)["live"] == "0"

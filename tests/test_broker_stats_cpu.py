"""The kernel broker's SELECT and HISTOGRAM ops against well-formed and hostile
frames, on CPU: the protocol core over the host-memory device of
``bee-broker-fuzz`` under ASan + UBSan (tests/test_broker_fuzz_cpu.py has the
harness's story).  The host device reads all n elements and computes real
answers (a sort, a search of the edges), so the replies are checked against
numpy and a wrong bound in the core is a sanitizer report."""

from __future__ import annotations

import struct

import numpy as np
import pytest

from .test_broker_fuzz_cpu import (ALLOC_AT, BAD_HANDLE, OK, PROTOCOL, WRITE, _finish, _serve, frame, fuzz_bin,  # noqa: F401
                                   run)

SELECT, HISTOGRAM = 27, 28
N = 64
X, SHORT = 1, 2  # client handles: N f64, and one element short
DATA = np.random.default_rng(4).standard_normal(N)


def select(dt, x, n, ranks, nranks=None):
    return frame(SELECT, struct.pack(f"<IIQq{len(ranks)}q", dt, len(ranks) if nranks is None else nranks, x, n, *ranks))


def histogram(dt, x, n, edges, bins=None):
    return frame(HISTOGRAM, struct.pack(f"<IIQq{len(edges)}d", dt, len(edges) - 1 if bins is None else bins, x, n,
                                        *edges))


def setup_frames():
    return [frame(ALLOC_AT, struct.pack("<QQ", X, N * 8)), frame(ALLOC_AT, struct.pack("<QQ", SHORT, (N - 1) * 8)),
            frame(WRITE, struct.pack("<QQ", X, 0) + DATA.tobytes())]


def rows_of(fuzz_bin, frames):
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[:3]] == [OK] * 3
    return rows[3:]


def test_well_formed_frames_reply_numpys_answers(fuzz_bin):
    s = np.sort(DATA)
    edges = [-3.0, -0.5, 0.0, 0.25, 3.0]
    frames = [
        select(1, X, N, [0, N - 1, 31, 32]),
        select(1, X, N, [5]),
        select(0, X, 2 * N, [0, 2 * N - 1]),      # the same bytes as f32: 2N elements fit
        select(2, X, 4 * N, [7]),                 # and as bf16
        select(1, X, 1, [0]),
        histogram(1, X, N, edges),
        histogram(1, X, N, [0.0, 0.0]),           # one empty bin
        histogram(0, X, 2 * N, [-1.0, 1.0]),
        histogram(1, X, 0, [0.0, 1.0]),           # n = 0
        histogram(1, X, N, [float(DATA.min()), float(DATA.max())]),
    ]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames), [r[1] for r in rows]
    assert struct.unpack("<5d", rows[0][4]) == (s[0], s[N - 1], s[31], s[32], 0.0)
    assert struct.unpack("<2d", rows[1][4]) == (s[5], 0.0)
    f32 = DATA.view(np.float32)
    s32 = np.sort(f32).astype(np.float64)  # (reinterpreted halves may hold NaNs: they sort last)
    np.testing.assert_array_equal(np.array(struct.unpack("<3d", rows[2][4])),
                                  np.array([s32[0], s32[-1], np.isnan(f32).sum()]))
    assert rows[3][2] == 16 and rows[4][4] == struct.pack("<2d", DATA[0], 0.0)
    assert struct.unpack("<4Q", rows[5][4]) == tuple(np.histogram(DATA, edges)[0])
    assert struct.unpack("<Q", rows[6][4]) == (0,)
    assert struct.unpack("<Q", rows[7][4]) == (np.histogram(f32[np.isfinite(f32)], [-1.0, 1.0])[0][0],)
    assert struct.unpack("<Q", rows[8][4]) == (0,)
    assert struct.unpack("<Q", rows[9][4]) == (N,)  # the last bin is closed on the right


def test_hostile_frames_are_refused(fuzz_bin):
    n_wrap = (1 << 61) + 2  # * 8 (f64) wraps to 16
    inf, nan = float("inf"), float("nan")
    frames = [
        # n * size overflow; negative and zero n; a buffer one element short
        select(1, X, n_wrap, [0]), histogram(1, X, n_wrap, [0.0, 1.0]),
        select(1, X, (1 << 63) - 1, [0]), histogram(1, X, (1 << 63) - 1, [0.0, 1.0]),
        select(1, X, -1, [0]), select(1, X, 0, [0]), histogram(1, X, -1, [0.0, 1.0]),
        select(1, SHORT, N, [0]), histogram(1, SHORT, N, [0.0, 1.0]), select(0, X, 2 * N + 1, [0]),
        # nranks outside 1..32, a rank outside [0, n)
        select(1, X, N, []), select(1, X, N, list(range(33))), select(1, X, N, [0], nranks=(1 << 32) - 1),
        select(1, X, N, [N]), select(1, X, N, [-1]), select(1, X, N, [0, 1 << 62]), select(1, X, 1, [1]),
        # bins outside 1..4096
        histogram(1, X, N, [0.0]), histogram(1, X, N, [float(i) for i in range(4098)]),
        histogram(1, X, N, [0.0, 1.0], bins=(1 << 32) - 1),
        # edges not finite, not non-decreasing
        histogram(1, X, N, [0.0, inf]), histogram(1, X, N, [-inf, 0.0]), histogram(1, X, N, [0.0, nan, 1.0]),
        histogram(1, X, N, [nan, nan]), histogram(1, X, N, [1.0, 0.0]), histogram(1, X, N, [0.0, 2.0, 1.0, 3.0]),
        # unknown dtypes, bool included; missing handles
        select(3, X, N, [0]), select(6, X, N, [0]), select(99, X, N, [0]),
        histogram(3, X, N, [0.0, 1.0]), histogram(6, X, N, [0.0, 1.0]), histogram((1 << 32) - 1, X, N, [0.0, 1.0]),
        select(1, 999, N, [0]), histogram(1, 999, N, [0.0, 1.0]),
    ]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [BAD_HANDLE] * len(frames), [(i, r[1]) for i, r in enumerate(rows) if r[1] != BAD_HANDLE]


def test_payload_length_must_match_the_announced_count(fuzz_bin):
    frames = [
        select(1, X, N, [0, 1], nranks=3), select(1, X, N, [0, 1, 2], nranks=2), select(1, X, N, [], nranks=1),
        histogram(1, X, N, [0.0, 1.0, 2.0], bins=3), histogram(1, X, N, [0.0, 1.0, 2.0], bins=1),
        histogram(1, X, N, [], bins=1),
        frame(SELECT, select(1, X, N, [0, 1])[16:] + b"\0"), frame(HISTOGRAM, histogram(1, X, N, [0.0, 1.0])[16:] + b"\0" * 8),
    ]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [PROTOCOL] * len(frames), [r[1] for r in rows]


def test_short_frames_are_protocol_errors(fuzz_bin):
    whole = [select(1, X, N, [0, 1, 2]), histogram(1, X, N, [0.0, 1.0, 2.0])]
    frames = []
    for f in whole:
        op, _, length = struct.unpack_from("<IIQ", f)
        frames += [frame(op, f[16:16 + cut]) for cut in (0, 3, 8, 23, 24, length - 8, length - 1)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [PROTOCOL] * len(frames), [r[1] for r in rows]


def _random_stats_frames(seed: int, count: int):
    import random

    rnd = random.Random(seed)
    handles = [X, SHORT, 999]
    sizes = [0, 1, 2, 31, 63, 64, 65, 128, 256, 257, 2**31, 2**61 + 2, 2**63 - 1, 2**64 - 1]
    out = []
    for _ in range(count):
        dt = rnd.choice([0, 1, 2, 1, 1, 3, 6, 2**32 - 1])
        n = rnd.choice(sizes) if rnd.random() < 0.8 else rnd.getrandbits(64)
        k = rnd.choice([0, 1, 2, 3, 31, 32, 33, 2**32 - 1]) if rnd.random() < 0.5 else rnd.randrange(1, 33)
        if rnd.random() < 0.5:
            carried = min(k, 40) if rnd.random() < 0.9 else rnd.randrange(0, 40)
            ranks = [rnd.choice([0, 1, 62, 63, 64, 2**63 - 1, 2**64 - 1, rnd.randrange(0, 64)]) for _ in range(carried)]
            payload = struct.pack(f"<IIQQ{carried}Q", dt, k, rnd.choice(handles), n, *ranks)
            op = SELECT
        else:
            carried = min(k + 1, 5000) if rnd.random() < 0.9 else rnd.randrange(0, 40)
            edges = sorted(rnd.uniform(-3, 3) for _ in range(carried))
            if edges and rnd.random() < 0.1:
                edges[rnd.randrange(len(edges))] = rnd.choice([float("nan"), float("inf"), -1e308, 7.0])
            payload = struct.pack(f"<IIQQ{carried}d", dt, k, rnd.choice(handles), n, *edges)
            op = HISTOGRAM
        if rnd.random() < 0.05:
            payload = payload[: rnd.randrange(0, len(payload) + 1)]
        out.append(frame(op, payload))
    return out


@pytest.mark.parametrize("seed", [21, 22])
def test_random_stats_frames_no_sanitizer_findings(fuzz_bin, seed):
    rows = rows_of(fuzz_bin, _random_stats_frames(seed, 2000))
    assert len(rows) == 2000
    ran = {op for op, st, *_ in rows if st == OK}
    assert {SELECT, HISTOGRAM} <= ran  # the stream reaches the device models


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_client_methods_speak_the_protocol(fuzz_bin, tmp_path, monkeypatch, dtype):
    """The real BrokerDriver's two methods against the daemon's frame reader
    and the protocol core: full-length replies checked against numpy."""
    from bee_code_interpreter_fs_amd.ops.driver import BeekernError, BrokerDriver

    monkeypatch.chdir(tmp_path)  # (a relative socket name: sun_path holds 108 bytes)
    p = _serve(fuzz_bin, "s.sock")
    d = BrokerDriver("s.sock")
    d.init(0)
    n = 5000
    h = np.random.default_rng(6).standard_normal(n).astype(dtype)
    h[[3, 77]] = np.nan
    dt = 1 if dtype == "float64" else 0
    x = d.malloc(h.nbytes)
    d.h2d(x, h)
    s = np.sort(h)
    ranks = [0, n - 1, n // 2, n // 2 - 1] + list(range(100, 128))
    vals, nans = d.select(dt, x, n, ranks)
    assert nans == 2 and len(vals) == 32
    np.testing.assert_array_equal(np.array(vals), s[ranks].astype(np.float64))
    for edges in (np.linspace(-4, 4, 51), np.histogram_bin_edges(h[np.isfinite(h)], 4096), np.array([-1.0, -1.0, 0.5, 9.0])):
        c = d.histogram(dt, x, n, edges)
        assert c.dtype == np.int64
        np.testing.assert_array_equal(c, np.histogram(h, edges)[0])
    with pytest.raises(BeekernError, match="bad handle"):
        d.select(dt, x, n, [n])
    with pytest.raises(BeekernError, match="bad handle"):
        d.histogram(dt, x, n, np.array([1.0, 0.0]))
    with pytest.raises(BeekernError, match="bad handle"):
        d.histogram(dt, x, n, np.arange(4098.0))
    d.sync()
    d.sock.close()
    assert _finish(p)["live"] == "0"

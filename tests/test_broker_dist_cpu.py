"""The kernel broker's RAND_DIST op against well-formed and hostile frames, on
CPU: the protocol core over the host-memory device of ``bee-broker-fuzz``
under ASan + UBSan (tests/test_broker_fuzz_cpu.py has the harness's story).
The host device writes every byte it is told to, with the exponential's real
values (kind 0), so a read-back is checked against the reference model
(tests/dist_ref.py) and a wrong bound in the core is a sanitizer report."""

from __future__ import annotations

import struct

import numpy as np
import pytest

from . import dist_ref as D
from .test_broker_fuzz_cpu import (ALLOC_AT, BAD_ARG, BAD_HANDLE, OK, PROTOCOL, READ, _finish, _serve, frame,  # noqa: F401
                                   fuzz_bin, run)

RAND, RAND_DIST = 6, 31
N = 64
X, SHORT = 1, 2  # client handles: N f64, and one element short
SEED = 0xB10C_D157
# valid parameters of every kind
VALID = {D.EXPONENTIAL: (2.0, 0.0), D.LAPLACE: (1.0, 0.5), D.LOGISTIC: (-1.0, 2.0), D.GUMBEL: (0.5, 1.5),
         D.RAYLEIGH: (1.5, 0.0), D.WEIBULL: (1.7, 0.0), D.PARETO: (3.0, 0.0), D.CAUCHY: (0.0, 1.0),
         D.LOGNORMAL: (0.25, 0.75), D.GAMMA: (0.3, 2.0), D.BETA: (2.0, 5.0), D.STUDENT_T: (5.0, 0.0)}


def rand_dist(kind, dt, h, n, p0, p1, seed=SEED, off=0):
    return frame(RAND_DIST, struct.pack("<IIQqQQdd", kind, dt, h, n, seed, off, p0, p1))


def setup_frames():
    return [frame(ALLOC_AT, struct.pack("<QQ", X, N * 8)), frame(ALLOC_AT, struct.pack("<QQ", SHORT, (N - 1) * 8))]


def rows_of(fuzz_bin, frames):
    rows = run(fuzz_bin, setup_frames() + frames)
    assert [r[1] for r in rows[:2]] == [OK] * 2
    return rows[2:]


def _close(got, want, dtype):
    # (the host device's libm log1p against numpy's: the same function up to an ulp or two)
    np.testing.assert_allclose(got, want, rtol=4 * np.finfo(dtype).eps, atol=0)


def test_well_formed_frames_of_every_kind(fuzz_bin):
    frames = []
    for kind, (p0, p1) in VALID.items():
        frames += [rand_dist(kind, 1, X, N, p0, p1), rand_dist(kind, 0, X, 2 * N, p0, p1), rand_dist(kind, 1, X, 0, p0, p1),
                   rand_dist(kind, 0, SHORT, 2 * N - 2, p0, p1)]
    frames += [rand_dist(D.EXPONENTIAL, 1, X, N, 0.0, 0.0), rand_dist(D.GAMMA, 1, X, N, 1e-3, 0.0),
               rand_dist(D.LOGNORMAL, 0, X, N, -3.0, 0.0), rand_dist(D.CAUCHY, 1, X, N, 1e300, 0.0)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * len(frames), [(i, r[1]) for i, r in enumerate(rows) if r[1] != OK]


@pytest.mark.parametrize("dt,dtype", [(1, np.float64), (0, np.float32)])
def test_the_exponential_reads_back_the_models_values(fuzz_bin, dt, dtype):
    n, off, scale = 13, 5, 2.5  # a ragged count: the last counter is used in part
    per = 64 // np.dtype(dtype).itemsize  # a READ reply of up to 64 bytes is echoed
    frames = [rand_dist(D.EXPONENTIAL, dt, X, n, scale, 0.0, off=off),
              frame(READ, struct.pack("<QQQ", X, 0, 64)), frame(READ, struct.pack("<QQQ", X, 64, 64))]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [OK] * 3
    got = np.frombuffer(rows[1][4] + rows[2][4], dtype)
    assert got.size == 2 * per
    _close(got[:n], D.draw(D.EXPONENTIAL, n, dtype, SEED, off, scale, 0.0), dtype)
    # the bytes past the draw: a partial write of a fresh buffer is preceded by its lazy scrub, so zeros
    assert not got[n:].view(np.uint8).any()


def test_hostile_frames_get_the_documented_status(fuzz_bin):
    inf, nan = float("inf"), float("nan")
    n_wrap = (1 << 61) + 2  # * 8 (f64) wraps to 16
    bad_arg = [
        # unknown kinds and dtypes (bf16, f16, bool among them)
        rand_dist(12, 1, X, N, 1.0, 1.0), rand_dist(99, 1, X, N, 1.0, 1.0), rand_dist((1 << 32) - 1, 1, X, N, 1.0, 1.0),
        rand_dist(D.EXPONENTIAL, 2, X, N, 1.0, 0.0), rand_dist(D.GAMMA, 3, X, N, 1.0, 1.0),
        rand_dist(D.GAMMA, 6, X, N, 1.0, 1.0), rand_dist(D.BETA, (1 << 32) - 1, X, N, 1.0, 1.0),
        # non-finite parameters, used or not
        rand_dist(D.EXPONENTIAL, 1, X, N, nan, 0.0), rand_dist(D.EXPONENTIAL, 1, X, N, inf, 0.0),
        rand_dist(D.EXPONENTIAL, 1, X, N, 1.0, nan), rand_dist(D.LAPLACE, 1, X, N, -inf, 1.0),
        rand_dist(D.LAPLACE, 1, X, N, 0.0, inf), rand_dist(D.LOGNORMAL, 0, X, N, nan, 1.0),
        rand_dist(D.GAMMA, 1, X, N, inf, 1.0), rand_dist(D.GAMMA, 1, X, N, 2.0, nan), rand_dist(D.BETA, 1, X, N, nan, nan),
        rand_dist(D.STUDENT_T, 1, X, N, inf, 0.0), rand_dist(D.CAUCHY, 1, X, N, 0.0, nan),
        # outside the domain: scale, sigma < 0; shape, a, b, df <= 0
        rand_dist(D.EXPONENTIAL, 1, X, N, -1.0, 0.0), rand_dist(D.LAPLACE, 1, X, N, 0.0, -1.0),
        rand_dist(D.LOGISTIC, 1, X, N, 0.0, -1e-300), rand_dist(D.GUMBEL, 0, X, N, 0.0, -2.0),
        rand_dist(D.RAYLEIGH, 1, X, N, -0.5, 0.0), rand_dist(D.WEIBULL, 1, X, N, 0.0, 0.0),
        rand_dist(D.WEIBULL, 1, X, N, -1.0, 0.0), rand_dist(D.PARETO, 1, X, N, 0.0, 0.0),
        rand_dist(D.CAUCHY, 1, X, N, 0.0, -1.0), rand_dist(D.LOGNORMAL, 1, X, N, 0.0, -1.0),
        rand_dist(D.GAMMA, 1, X, N, 0.0, 1.0), rand_dist(D.GAMMA, 1, X, N, -2.0, 1.0), rand_dist(D.GAMMA, 1, X, N, 2.0, -1.0),
        rand_dist(D.BETA, 1, X, N, 0.0, 1.0), rand_dist(D.BETA, 1, X, N, 1.0, 0.0), rand_dist(D.BETA, 1, X, N, 1.0, -1.0),
        rand_dist(D.STUDENT_T, 1, X, N, 0.0, 0.0), rand_dist(D.STUDENT_T, 1, X, N, -3.0, 0.0),
        # the parameters are judged before the handle
        rand_dist(D.GAMMA, 1, 999, N, -1.0, 1.0), rand_dist(77, 1, X, -1, 1.0, 1.0),
    ]
    bad_handle = [
        # short buffers, n < 0, sizes that overflow, missing handles
        rand_dist(D.EXPONENTIAL, 1, SHORT, N, 1.0, 0.0), rand_dist(D.GAMMA, 1, X, N + 1, 2.0, 1.0),
        rand_dist(D.GAMMA, 0, X, 2 * N + 1, 2.0, 1.0), rand_dist(D.BETA, 1, X, -1, 2.0, 5.0),
        rand_dist(D.EXPONENTIAL, 1, X, -(1 << 63), 1.0, 0.0), rand_dist(D.EXPONENTIAL, 1, X, n_wrap, 1.0, 0.0),
        rand_dist(D.STUDENT_T, 0, X, (1 << 62) + 4, 3.0, 0.0), rand_dist(D.LOGNORMAL, 1, X, (1 << 63) - 1, 0.0, 1.0),
        rand_dist(D.EXPONENTIAL, 1, 999, N, 1.0, 0.0), rand_dist(D.EXPONENTIAL, 1, 0, 0, 1.0, 0.0),
    ]
    rows = rows_of(fuzz_bin, bad_arg + bad_handle)
    want = [BAD_ARG] * len(bad_arg) + [BAD_HANDLE] * len(bad_handle)
    assert [r[1] for r in rows] == want, [(i, r[1]) for i, (r, w) in enumerate(zip(rows, want)) if r[1] != w]
    # kRand still takes kinds 0 and 1 alone
    rows = rows_of(fuzz_bin, [frame(RAND, struct.pack("<IIQqQQdd", k, 1, X, N, 1, 0, 0.0, 1.0)) for k in (0, 1, 2, 9)])
    assert [r[1] for r in rows] == [OK, OK, BAD_HANDLE, BAD_HANDLE]


def test_short_frames_are_protocol_errors(fuzz_bin):
    whole = rand_dist(D.GAMMA, 1, X, N, 2.0, 1.0)
    frames = [frame(RAND_DIST, whole[16:16 + cut]) for cut in (0, 3, 4, 8, 16, 24, 40, 48, 55)]
    rows = rows_of(fuzz_bin, frames)
    assert [r[1] for r in rows] == [PROTOCOL] * len(frames), [r[1] for r in rows]


def test_a_refused_draw_leaves_the_buffer_to_the_lazy_scrub(fuzz_bin):
    # a fresh buffer holds another tenant's bytes; a draw the core refuses writes nothing, so a read scrubs first
    frames = [rand_dist(D.GAMMA, 1, X, N, -1.0, 1.0), frame(READ, struct.pack("<QQQ", X, 0, 64))]
    rows = rows_of(fuzz_bin, frames)
    assert rows[0][1] == BAD_ARG and rows[1][1] == OK and rows[1][4] == bytes(64)


def _random_dist_frames(seed: int, count: int):
    import random

    rnd = random.Random(seed)
    handles = [X, SHORT, 999]
    sizes = [0, 1, 2, 3, 31, 63, 64, 65, 126, 127, 128, 129, 256, 2**31, 2**61 + 2, 2**62 + 4, 2**63 - 1, 2**64 - 1]
    values = [0.0, -0.0, 1.0, 2.5, 0.3, 1e-300, 1e300, -1.0, -1e-300, float("nan"), float("inf"), -float("inf")]
    out = []
    for _ in range(count):
        kind = rnd.choice(list(range(12)) * 3 + [12, 13, 2**31, 2**32 - 1])
        dt = rnd.choice([0, 1, 0, 1, 1, 2, 3, 6, 2**32 - 1])
        n = rnd.choice(sizes) if rnd.random() < 0.8 else rnd.getrandbits(64)
        p0 = rnd.choice(values) if rnd.random() < 0.7 else rnd.uniform(-1, 5)
        p1 = rnd.choice(values) if rnd.random() < 0.7 else rnd.uniform(-1, 5)
        payload = struct.pack("<IIQQQQdd", kind, dt, rnd.choice(handles), n, rnd.getrandbits(64), rnd.getrandbits(64),
                              p0, p1)
        if rnd.random() < 0.05:
            payload = payload[: rnd.randrange(0, len(payload) + 1)]
        out.append(frame(RAND_DIST, payload))
    return out


@pytest.mark.parametrize("seed", [31, 32])
def test_random_dist_frames_no_sanitizer_findings(fuzz_bin, seed):
    rows = rows_of(fuzz_bin, _random_dist_frames(seed, 3000))
    assert len(rows) == 3000
    seen = {st for _, st, *_ in rows}
    assert {OK, BAD_ARG, BAD_HANDLE, PROTOCOL} <= seen  # the stream reaches the device model and every refusal


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_client_method_speaks_the_protocol(fuzz_bin, tmp_path, monkeypatch, dtype):
    """The real BrokerDriver's rand_dist against the daemon's frame reader and
    the protocol core: a whole exponential draw read back."""
    from bee_code_interpreter_fs_amd.ops.driver import RAND_DIST as CLIENT_OP
    from bee_code_interpreter_fs_amd.ops.driver import BeekernError, BrokerDriver

    assert CLIENT_OP == RAND_DIST
    monkeypatch.chdir(tmp_path)  # (a relative socket name: sun_path holds 108 bytes)
    p = _serve(fuzz_bin, "d.sock")
    d = BrokerDriver("d.sock")
    d.init(0)
    n, dt = 5003, 1 if dtype == "float64" else 0
    x = d.malloc(n * np.dtype(dtype).itemsize)
    d.rand_dist(D.EXPONENTIAL, x, n, dt, SEED, 7, 1.5, 0.0)
    got = np.empty(n, dtype)
    d.d2h(x, got)
    _close(got, D.draw(D.EXPONENTIAL, n, dtype, SEED, 7, 1.5, 0.0), np.dtype(dtype))
    for kind, (p0, p1) in VALID.items():
        d.rand_dist(kind, x, n, dt, SEED, 0, p0, p1)
    d.sync()
    d.rand_dist(D.GAMMA, x, n, dt, SEED, 0, -1.0, 1.0)  # fire-and-forget: the refusal arrives with the next reply
    with pytest.raises(BeekernError, match="bad argument.*bk.rand_dist"):
        d.sync()
    d.rand_dist(D.GAMMA, x, n + 1, dt, SEED, 0, 2.0, 1.0)
    with pytest.raises(BeekernError, match="bad handle.*bk.rand_dist"):
        d.sync()
    d.sync()
    d.sock.close()
    assert _finish(p)["live"] == "0"

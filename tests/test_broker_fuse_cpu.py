"""The broker's fused pairs on CPU: which producer / consumer pairs of a batch
go out as one launch, and that nothing but the launch count tells.

Through ``bee-broker-fuzz`` (the daemon's reader, batch walk and session over
the host-memory device, ASan + UBSan) and its launch log, as
tests/test_broker_plan_cpu.py: a fused pair is one log line
(``reduce_axis+cast``, ``reduce_axis+reduce``, ``gemm+reduce``), an unfused
one two.  Replies, statuses, deferred errors and buffer contents are compared
with the switch off (BEE_BROKER_FUSE=0) and with a device that has no fused
launches (BEE_FUZZ_NO_FUSED=1: the session must fall back by itself).
"""

from __future__ import annotations

import random
import struct

import pytest

from .test_broker_plan_cpu import (BAD_HANDLE, NO_REPLY, OK, Broker, _stdin_run, alloc_at, fill, frame, fuzz_bin,  # noqa: F401
                                   post, sync)

FREE, READ, CAST, REDUCE, GEMM, REDUCE_AXIS = 3, 5, 9, 11, 12, 20
F32, F64, BF16 = 0, 1, 2
SUM, MAX, DOT, MAX_ABS_DIFF = 0, 3, 5, 6
ESIZE = {F32: 4, F64: 8, BF16: 2}
R = 64  # the payload's 4096, scaled down


def reduce_axis(x, y, rows, cols, axis, dt=F32, op=0, ld=None):
    return post(REDUCE_AXIS, struct.pack("<IIQQqqqII", op, dt, x, y, rows, cols, cols if ld is None else ld, axis, 0))


def cast(s, d, x, y, n):
    return post(CAST, struct.pack("<IIQQq", s, d, x, y, n))


def reduce_(op, dt, a, b, n, flags=0):
    return frame(REDUCE, struct.pack("<IIQQq", op, dt, a, b, n), flags)


def gemm(A, Bt, C, M, N, K, ldc=None, beta=0.0, odt=F32, lda=None, ldb=None):
    return post(GEMM, struct.pack("<QQQiiiiiiffii", A, Bt, C, M, N, K, K if lda is None else lda, K if ldb is None else ldb,
                                  N if ldc is None else ldc, 1.0, beta, odt, 0))


def free(h):
    return post(FREE, struct.pack("<Q", h))


def read(h, n, off=0):
    return frame(READ, struct.pack("<QQQ", h, off, n))


A, B, C, ROWS, S32, S16, REF, OTHER = 1, 2, 3, 4, 5, 6, 7, 8


def _operands(b):
    """a, b (bf16) and c (f32), R x R, written."""
    st, _ = b.call(alloc_at(A, 2 * R * R), alloc_at(B, 2 * R * R), alloc_at(C, 4 * R * R), fill(A, 2 * R * R),
                   fill(B, 2 * R * R), fill(C, 4 * R * R), alloc_at(OTHER, 4 * R), fill(OTHER, 4 * R), sync())
    assert st == OK
    return 4  # launches so far


def _launches(b, skip):
    return [k for _, k in b.finish()][skip:]


def test_the_payloads_short_batches_are_fused(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    n0 = _operands(b)
    # rows = c.sum(axis=1); rows.sum()
    st, total = b.call(alloc_at(ROWS, 4 * R), reduce_axis(C, ROWS, R, R, 1), reduce_(SUM, F32, ROWS, 0, R))
    assert st == OK and len(total) == 8
    # s = b.sum(axis=0).astype(bf16); ref = a @ s; max|rows - ref|
    st, err = b.call(alloc_at(S32, 4 * R), reduce_axis(B, S32, R, R, 0, dt=BF16), alloc_at(S16, 2 * R),
                     cast(F32, BF16, S32, S16, R), free(S32), alloc_at(REF, 4 * R), gemm(A, S16, REF, R, 1, R),
                     reduce_(MAX_ABS_DIFF, F32, ROWS, REF, R))
    assert st == OK and len(err) == 8
    assert _launches(b, n0) == ["reduce_axis+reduce", "reduce_axis+cast", "gemm+reduce"]


def test_switch_off_and_a_device_without_fused_launches(fuzz_bin, tmp_path):
    for i, env in enumerate(({"BEE_BROKER_FUSE": "0"}, {"BEE_FUZZ_NO_FUSED": "1"})):
        d = tmp_path / str(i)
        d.mkdir()
        b = Broker(fuzz_bin, d, **env)
        n0 = _operands(b)
        assert b.call(alloc_at(ROWS, 4 * R), reduce_axis(C, ROWS, R, R, 1), reduce_(SUM, F32, ROWS, 0, R))[0] == OK
        assert b.call(alloc_at(S16, 2 * R), cast(F32, BF16, ROWS, S16, R), alloc_at(REF, 4 * R), gemm(A, S16, REF, R, 1, R),
                      reduce_(MAX_ABS_DIFF, F32, ROWS, REF, R))[0] == OK
        assert _launches(b, n0) == ["reduce_axis", "reduce", "cast", "gemm", "reduce"]


def test_frames_outside_a_batch_are_not_fused(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    n0 = _operands(b)
    b.send(alloc_at(ROWS, 4 * R), reduce_axis(C, ROWS, R, R, 1))  # no closing frame: no batch
    b.launched(n0 + 1, "reduce_axis")
    assert b.call(reduce_(SUM, F32, ROWS, 0, R))[0] == OK
    assert _launches(b, n0) == ["reduce_axis", "reduce"]


LIMIT_F32 = 4 * 1024 + 3  # bk_reduce runs one block up to 1024 16-byte vectors (and the scalar rest)

NEAR_MISSES = {
    # name: (frames after `alloc_at(ROWS)`, launches)
    "a fill between": ([reduce_axis(C, ROWS, R, R, 1), fill(OTHER, 4 * R), reduce_(SUM, F32, ROWS, 0, R)],
                       ["reduce_axis", "fill", "reduce"]),
    "a free between": ([reduce_axis(C, ROWS, R, R, 1), free(OTHER), reduce_(SUM, F32, ROWS, 0, R)],
                       ["reduce_axis", "reduce"]),
    "another handle": ([reduce_axis(C, ROWS, R, R, 1), reduce_(SUM, F32, OTHER, 0, R)], ["reduce_axis", "reduce"]),
    "part of the output": ([reduce_axis(C, ROWS, R, R, 1), reduce_(SUM, F32, ROWS, 0, R - 1)], ["reduce_axis", "reduce"]),
    "another dtype": ([reduce_axis(C, ROWS, R, R, 1), reduce_(SUM, BF16, ROWS, 0, R)], ["reduce_axis", "reduce"]),
    "both operands the output": ([reduce_axis(C, ROWS, R, R, 1), reduce_(DOT, F32, ROWS, ROWS, R)],
                                 ["reduce_axis", "reduce"]),
    "the cast's output is the producer's input": ([reduce_axis(C, ROWS, R, R, 1), cast(F32, BF16, ROWS, C, R)],
                                                  ["reduce_axis", "cast"]),
    "the cast's output is its input": ([reduce_axis(C, ROWS, R, R, 1), cast(F32, F64, ROWS, ROWS, R // 2)],
                                       ["reduce_axis", "cast"]),
    "a cast to the same dtype": ([reduce_axis(C, ROWS, R, R, 1), cast(F32, F32, ROWS, OTHER, R)], ["reduce_axis", "cast"]),
    "ldc != N": ([gemm(A, B, C, R, 2, R, ldc=3), reduce_(SUM, F32, C, 0, 2 * R)], ["gemm", "reduce"]),
    "beta != 0": ([gemm(A, B, C, R, 2, R, beta=1.0), reduce_(SUM, F32, C, 0, 2 * R)], ["gemm", "reduce"]),
    "N = 17": ([gemm(A, B, C, R, 17, R), reduce_(SUM, F32, C, 0, 17 * R)], ["gemm", "reduce"]),
    "N = 16 fuses": ([gemm(A, B, C, R, 16, R), reduce_(SUM, F32, C, 0, 16 * R)], ["gemm+reduce"]),
    "B given [K][N]": ([post(GEMM, struct.pack("<QQQiiiiiiffii", A, B, C, R, 2, R, R, 2, 2, 1.0, 0.0, F32, 1)),
                        reduce_(SUM, F32, C, 0, 2 * R, flags=NO_REPLY)], ["gemm_nn", "reduce"]),
}


@pytest.mark.parametrize("name", sorted(NEAR_MISSES))
def test_near_misses_are_not_fused(fuzz_bin, tmp_path, name):
    frames, want = NEAR_MISSES[name]
    b = Broker(fuzz_bin, tmp_path)
    n0 = _operands(b)
    b.call(alloc_at(ROWS, 4 * R), *frames, sync())
    assert _launches(b, n0) == want


def test_single_block_limit_of_the_closing_reduce(fuzz_bin, tmp_path):
    """LIMIT_F32 row sums are reduced by the producer, one more by bk_reduce."""
    b = Broker(fuzz_bin, tmp_path)
    big = LIMIT_F32 + 1
    assert b.call(alloc_at(1, 4 * 8 * big), fill(1, 4 * 8 * big), alloc_at(2, 4 * big), sync())[0] == OK
    assert b.call(reduce_axis(1, 2, LIMIT_F32, 8, 1), reduce_(SUM, F32, 2, 0, LIMIT_F32))[0] == OK
    assert b.call(reduce_axis(1, 2, big, 8, 1), reduce_(SUM, F32, 2, 0, big))[0] == OK
    # f64 rows hold half as many per vector
    assert b.call(reduce_axis(1, 2, 2049, 8, 1, dt=F64), reduce_(SUM, F64, 2, 0, 2049))[0] == OK
    assert b.call(reduce_axis(1, 2, 2050, 8, 1, dt=F64), reduce_(SUM, F64, 2, 0, 2050))[0] == OK
    assert _launches(b, 1) == ["reduce_axis+reduce", "reduce_axis", "reduce", "reduce_axis+reduce", "reduce_axis", "reduce"]


def test_invalid_consumer_gets_its_status_and_the_producer_still_runs(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    n0 = _operands(b)
    st, _ = b.call(alloc_at(ROWS, 4 * R), reduce_axis(C, ROWS, R, R, 1), reduce_(SUM, F32, 99, 0, R))  # no buffer 99
    assert st == BAD_HANDLE
    # a fire-and-forget consumer: its failure is the deferred one, and names the cast
    st, msg = b.call(reduce_axis(C, ROWS, R, R, 1), cast(F32, BF16, ROWS, 99, R), sync())
    assert st == BAD_HANDLE and msg == b"deferred from bk.cast"
    assert b.call(read(ROWS, 4 * R))[1] == bytes(4 * R)  # written by the producer (the device writes zeros)
    assert _launches(b, n0) == ["reduce_axis", "reduce_axis"]


def test_invalid_producer_is_reported_as_ever(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    n0 = _operands(b)
    st, msg = b.call(alloc_at(ROWS, 4 * R), reduce_axis(99, ROWS, R, R, 1), reduce_(SUM, F32, ROWS, 0, R))
    assert st == BAD_HANDLE and msg == b"deferred from bk.reduce_axis"
    assert b.call(reduce_(SUM, F32, ROWS, 0, R)) == (OK, struct.pack("<d", 0.0))  # never written: scrubbed, then summed
    assert _launches(b, n0) == ["reduce"]


def test_producer_the_device_refuses_keeps_its_place_in_the_error_order(fuzz_bin, tmp_path):
    """A column reduction wider than the device's workspace passes the session's
    checks and fails at its launch -- late, when it is held for its partner.
    Its failure is still the one reported, ahead of the allocation that failed
    after it, and its output is not taken for written."""
    wide = 262144 + 1

    def run(d, **env):
        d.mkdir()
        b = Broker(fuzz_bin, d, **env)
        assert b.call(alloc_at(1, 4 * wide), fill(1, 4 * wide), alloc_at(2, 4 * wide), alloc_at(3, 2 * wide), sync())[0] == OK
        first = b.call(reduce_axis(1, 2, 1, wide, 0), alloc_at(2, 64), cast(F32, BF16, 2, 3, wide), sync())
        second = b.call(read(2, 64))
        return first, second, [k for _, k in b.finish()]

    on = run(tmp_path / "on")
    off = run(tmp_path / "off", BEE_BROKER_FUSE="0")
    assert on == off
    assert on[0][0] == 1 and on[0][1].startswith(b"deferred from bk.reduce_axis")  # kBadArgument, not the kBadHandle
    assert on[1] == (OK, bytes(64))


# ---- random batches: identical with the switch on, off, and on a device that declines ----------


def _random_stream(seed: int) -> bytes:
    rng = random.Random(seed)
    sizes = {}  # handle -> bytes
    out = []
    next_h = [1]

    def new(nbytes):
        h = next_h[0]
        next_h[0] += 1
        sizes[h] = nbytes
        out.append(alloc_at(h, nbytes))
        return h

    def pick(min_bytes=0):
        ok = [h for h, s in sizes.items() if s >= min_bytes]
        return rng.choice(ok) if ok and rng.random() > 0.03 else 999  # now and then a handle that does not exist

    for _ in range(rng.randrange(280, 340)):
        for _ in range(rng.randrange(0, 4)):
            kind = rng.randrange(8)
            if kind == 0 and len(sizes) > 6:
                h = rng.choice(list(sizes))
                del sizes[h]
                out.append(free(h))
                continue
            if kind == 1:
                h = pick()
                out.append(fill(h, rng.randrange(0, sizes.get(h, 64) + 1)))
                continue
            # a producer, sometimes allocations, a consumer -- mostly of the producer's output
            if rng.random() < 0.6:
                dt = rng.choice([F32, F64, BF16])
                rows, cols, axis = rng.randrange(1, 40), rng.randrange(1, 40), rng.randrange(2)
                x = new(ESIZE[dt] * rows * cols)
                out.append(fill(x, sizes[x]))
                ydt, count = (F64 if dt == F64 else F32), (cols if axis == 0 else rows)
                y = new(ESIZE[ydt] * count + rng.choice([0, 0, 8]))
                out.append(reduce_axis(x if rng.random() > 0.05 else 999, y, rows, cols, axis, dt=dt, op=rng.randrange(2)))
                ins = [x]
            else:
                M, N, K = rng.randrange(1, 24), rng.choice([1, 1, 2, 16, 17]), rng.choice([8, 16, 64, 12])
                ydt = rng.choice([F32, BF16])
                a, bt = new(2 * M * K), new(2 * N * K)
                out += [fill(a, sizes[a]), fill(bt, sizes[bt])]
                ldc = N + rng.choice([0, 0, 0, 1])
                y, count = new(ESIZE[ydt] * M * ldc), M * N
                out.append(gemm(a, bt, y, M, N, K, ldc=ldc, beta=rng.choice([0.0, 0.0, 0.5]), odt=ydt))
                ins = [a, bt]
            for _ in range(rng.choice([0, 0, 1, 2])):
                new(rng.randrange(1, 256))
            if rng.random() < 0.15:
                out.append(fill(pick(), 0))  # something between that is no allocation
            src = y if rng.random() > 0.1 else pick()
            n = count if rng.random() > 0.1 else max(0, count - 1)
            if rng.random() < 0.5:
                d = rng.choice([F32, F64, BF16])
                dst = new(ESIZE[d] * n) if rng.random() > 0.15 else rng.choice(ins + [y, 999])
                out.append(cast(ydt, d, src, dst, n))
            else:
                rop = rng.choice([0, 1, 2, 3, 4, 5, 6])
                other = pick(ESIZE[ydt] * n) if rng.random() > 0.1 else y
                a_, b_ = (src, other) if rng.random() > 0.5 else (other, src)
                if rop < 5:
                    a_ = src
                out.append(reduce_(rop, ydt, a_, b_, n, flags=rng.choice([0, NO_REPLY])))
                if out[-1][4] == 0:  # it wanted its reply: the batch ended there
                    break
        closer = rng.randrange(3)
        h = pick()
        out.append(sync() if closer == 0 else read(h, min(64, sizes.get(h, 64))) if closer == 1
                   else reduce_(SUM, F32, h, 0, min(16, sizes.get(h, 64) // 4)))
    for h in sorted(sizes):  # what every buffer holds at the end
        out.append(read(h, min(64, sizes[h])))
    return b"".join(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_batches_are_the_same_fused_and_unfused(fuzz_bin, seed):
    data = _random_stream(seed)
    on = _stdin_run(fuzz_bin, data, BEE_FUZZ_LAUNCH_LOG="1")
    off = _stdin_run(fuzz_bin, data, BEE_BROKER_FUSE="0")
    declined = _stdin_run(fuzz_bin, data, BEE_FUZZ_NO_FUSED="1")
    fused = [ln for ln in on if ln.startswith("LAUNCH") and "+" in ln]
    assert len(fused) > 30, len(fused)  # the streams do fuse
    assert {ln.split()[3] for ln in fused} == {"reduce_axis+cast", "reduce_axis+reduce", "gemm+reduce"}
    on = [ln for ln in on if not ln.startswith("LAUNCH")]
    assert len(on) > 1000
    assert on == off
    assert on == declined

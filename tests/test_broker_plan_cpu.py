"""The broker's batch plan on CPU: which batches run on the priority lane.

``bee-broker-fuzz --listen`` runs the daemon's frame reader, batch walk and
session (csrc/executor/broker_core.cpp) over the host-memory device, under
ASan + UBSan.  With ``BEE_FUZZ_LAUNCH_LOG=1`` that device prints one line per
launch -- its issue order, the lane it went to, the kernel -- so the plan is
checked on what was really issued, and the replies against a run of the same
frames with the plan switched off.
"""

from __future__ import annotations

import os
import socket
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "sanitize", "bee-broker-fuzz")

READ, RAND, UNARY, FILL, REDUCE, SYNC, MEMSTATS, RAND_REDUCE, ALLOC_AT = 5, 6, 7, 10, 11, 14, 15, 18, 19
OK, BAD_HANDLE = 0, 6
NO_REPLY = 1
SHORT_BYTES = 16 << 20  # broker_core.hpp kShortBytes


@pytest.fixture(scope="module")
def fuzz_bin():
    from bee_code_interpreter_fs_amd import _build

    _build.build(["broker-fuzz"], verbose=False)
    assert os.path.exists(BIN)
    return BIN


def frame(op: int, payload: bytes = b"", flags: int = 0) -> bytes:
    return struct.pack("<IIQ", op, flags, len(payload)) + payload


def post(op: int, payload: bytes = b"") -> bytes:
    return frame(op, payload, NO_REPLY)


def alloc_at(h, nbytes):
    return post(ALLOC_AT, struct.pack("<QQ", h, nbytes))


def fill(h, nbytes, flags=NO_REPLY):
    return frame(FILL, struct.pack("<QqQII", h, nbytes, 0x0101010101010101, 8, 0), flags)


def rand(h, n, dt=1, seed=7):
    return post(RAND, struct.pack("<IIQqQQdd", 0, dt, h, n, seed, 0, 0.0, 1.0))


def reduce_(h, n, dt=1, flags=0):
    return frame(REDUCE, struct.pack("<IIQQq", 0, dt, h, 0, n), flags)


def rand_reduce(n, seed=11, flags=0):
    return frame(RAND_REDUCE, struct.pack("<IIqQQdd", 1, 1, n, seed, 0, 0.0, 1.0), flags)


def sync():
    return frame(SYNC)


def memstats():
    """A frame that wants a reply and waits for nothing: the session stays undrained."""
    return frame(MEMSTATS)


class Broker:
    """One session with the fuzz harness's broker over its Unix socket."""

    def __init__(self, fuzz_bin, tmp_path, budget=96 << 20, **env):
        self.cwd = str(tmp_path)  # the socket by a relative name: sun_path holds 108 bytes
        self.p = subprocess.Popen([fuzz_bin, "--listen", "b.sock", str(budget), "0"], cwd=self.cwd,
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                  env={**os.environ, "ASAN_OPTIONS": "abort_on_error=1:detect_leaks=1",
                                       "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
                                       "BEE_FUZZ_LAUNCH_LOG": "1", **env})
        assert self.p.stdout.readline().strip() == b"LISTENING"
        self.seen = []  # launch lines read ahead of finish()
        self.s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        cwd = os.getcwd()
        os.chdir(self.cwd)
        try:
            self.s.connect("b.sock")
        finally:
            os.chdir(cwd)

    def send(self, *frames):
        self.s.sendall(b"".join(frames))

    def reply(self):
        buf = b""
        while len(buf) < 16:
            chunk = self.s.recv(16 - len(buf))
            assert chunk, "broker closed the connection"
            buf += chunk
        st, _, n = struct.unpack("<iIQ", buf)
        body = b""
        while len(body) < n:
            chunk = self.s.recv(n - len(body))
            assert chunk, "broker closed the connection"
            body += chunk
        return st, body

    def launched(self, total, kernel):
        """Block until the broker has issued `total` launches, the last one `kernel` (the log is flushed per line)."""
        while len(self.seen) < total:
            line = self.p.stdout.readline().decode()
            assert line.startswith("LAUNCH"), line
            self.seen.append(line)
        assert self.seen[-1].split()[3] == kernel, self.seen

    def call(self, *frames):
        """Send one batch (its last frame wants the reply) in one write."""
        self.send(*frames)
        return self.reply()

    def finish(self):
        """Close; the launches as (lane, kernel) in issue order."""
        self.s.close()
        out, err = self.p.communicate(timeout=60)
        err = err.decode(errors="replace")
        assert self.p.returncode == 0 and "AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
        lines = "".join(self.seen).splitlines() + out.decode().splitlines()
        assert lines[-1].startswith("SERVED") and lines[-1].endswith("live=0"), lines[-1]
        log = [ln.split() for ln in lines if ln.startswith("LAUNCH")]
        assert [int(x[1]) for x in log] == list(range(len(log)))  # the issue order, as printed
        return [(int(x[2]), x[3]) for x in log]


def test_all_short_batch_after_a_completed_wait_runs_on_the_priority_lane(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(sync())[0] == OK
    st, body = b.call(alloc_at(1, 4096), fill(1, 4096), reduce_(1, 512))
    assert st == OK and struct.unpack("<d", body)[0] == 4096.0
    assert b.finish() == [(1, "fill"), (1, "reduce")]


def test_one_long_op_keeps_the_batch_on_the_normal_lane(fuzz_bin, tmp_path):
    """The smallest long op: 16 MiB + 1 byte of traffic (a fill of that many
    bytes); exactly 16 MiB is still short."""
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(alloc_at(1, SHORT_BYTES + 1), alloc_at(2, 4096), sync())[0] == OK
    assert b.call(fill(2, 4096), fill(1, SHORT_BYTES + 1), reduce_(2, 512))[0] == OK   # one long op: normal
    assert b.call(fill(2, 4096), fill(1, SHORT_BYTES), reduce_(2, 512))[0] == OK       # all short: priority
    assert b.call(fill(1, SHORT_BYTES + 1), sync())[0] == OK                           # and back
    assert b.finish() == [(0, "fill"), (0, "fill"), (0, "reduce"), (1, "fill"), (1, "fill"), (1, "reduce"), (0, "fill")]


def test_short_batch_while_not_drained_does_not_change_lane(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    # the closing frame waits for nothing: the long fill is still queued when the reply leaves
    assert b.call(alloc_at(1, SHORT_BYTES + 1), alloc_at(2, 4096), fill(1, SHORT_BYTES + 1), memstats())[0] == OK
    assert b.call(fill(2, 4096), reduce_(2, 512))[0] == OK  # all short, but the lane stays; this wait drains
    assert b.call(fill(2, 4096), reduce_(2, 512))[0] == OK  # now it moves
    assert b.finish() == [(0, "fill"), (0, "fill"), (0, "reduce"), (1, "fill"), (1, "reduce")]


def test_not_drained_on_the_priority_lane_keeps_a_long_batch_there(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(alloc_at(1, SHORT_BYTES + 1), alloc_at(2, 4096), sync())[0] == OK
    assert b.call(fill(2, 4096), memstats())[0] == OK                  # short, drained: priority; fill still queued
    assert b.call(fill(1, SHORT_BYTES + 1), reduce_(2, 512))[0] == OK  # long, but not drained: stays
    assert b.call(fill(1, SHORT_BYTES + 1), sync())[0] == OK           # drained by the reduce: back to normal
    assert b.finish() == [(1, "fill"), (1, "fill"), (1, "reduce"), (0, "fill")]


def test_closing_frame_in_a_second_write_is_arrival_order_on_the_current_lane(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(alloc_at(1, 4096), fill(1, 4096), reduce_(1, 512))[0] == OK  # drained, on the priority lane
    b.send(alloc_at(2, SHORT_BYTES + 1), fill(2, SHORT_BYTES + 1))              # no closing frame: no batch
    b.launched(3, "fill")                                                       # handled before the rest arrives
    st, body = b.call(rand_reduce(1 << 23))
    assert st == OK and struct.unpack("<d", body)[0] == float(1 << 23)
    # a long fill and a long draw-reduce, in arrival order, where the session was
    assert b.finish() == [(1, "fill"), (1, "reduce"), (1, "fill"), (1, "rand_reduce")]


def test_draw_reduce_counts_by_its_draws(fuzz_bin, tmp_path):
    """2^22 draws are short, one more is long."""
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(alloc_at(1, 4096), fill(1, 4096), rand_reduce(1 << 22))[0] == OK
    assert b.call(fill(1, 4096), rand_reduce((1 << 22) + 1))[0] == OK
    assert b.finish() == [(1, "fill"), (1, "rand_reduce"), (0, "fill"), (0, "rand_reduce")]


def _bad_handle_batch(fuzz_bin, tmp_path, **env):
    b = Broker(fuzz_bin, tmp_path, **env)
    first = b.call(rand(99, 4096), rand_reduce(1000))  # no buffer 99
    second = b.call(rand_reduce(1000))                 # the failure was reported once
    b.finish()
    return first, second


def test_deferred_failure_is_reported_the_same_with_the_plan_off(fuzz_bin, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    first, second = _bad_handle_batch(fuzz_bin, tmp_path / "a")
    first0, second0 = _bad_handle_batch(fuzz_bin, tmp_path / "b", BEE_BROKER_LANES="0")
    assert first[0] == BAD_HANDLE and first[1] == b"deferred from bk.rand"
    assert first == first0
    assert second[0] == OK and second == second0


def test_lanes_off_switch(fuzz_bin, tmp_path):
    b = Broker(fuzz_bin, tmp_path, BEE_BROKER_LANES="0")
    assert b.call(alloc_at(1, 4096), fill(1, 4096), reduce_(1, 512))[0] == OK
    assert b.finish() == [(0, "fill"), (0, "reduce")]


def test_walk_refuses_a_frame_length_that_would_wrap(fuzz_bin, tmp_path):
    """A header whose length, added to its position, wraps 64 bits: the walk
    finds no batch and plans nothing (the lane does not move); next() then refuses the frame as it always has and the
    connection ends with nothing read past the buffer."""
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(alloc_at(1, 4096), sync())[0] == OK
    hostile = struct.pack("<IIQ", FILL, NO_REPLY, (1 << 64) - 8)
    b.send(fill(1, 4096), hostile, rand_reduce(1000))
    try:
        assert b.s.recv(16) == b""  # closed without a reply
    except ConnectionResetError:
        pass
    assert b.finish() == [(0, "fill")]


def test_walk_stops_at_the_bytes_it_has(fuzz_bin, tmp_path):
    """Lengths that end exactly at, and one byte past, the buffered bytes."""
    b = Broker(fuzz_bin, tmp_path)
    assert b.call(alloc_at(1, 4096), sync())[0] == OK
    whole = fill(1, 4096) + reduce_(1, 512)
    b.send(whole[:-1])      # the closing frame one byte short: no batch
    b.launched(1, "fill")   # (the frame before it was handled on its own)
    b.send(whole[-1:])
    assert b.reply()[0] == OK
    assert b.call(fill(1, 4096), reduce_(1, 512))[0] == OK  # whole: a batch
    assert b.finish() == [(0, "fill"), (0, "reduce"), (1, "fill"), (1, "reduce")]


# ---- the walk over hostile streams, in the stand-alone harness's stdin loop ----------


def _stdin_run(fuzz_bin, data: bytes, **env):
    p = subprocess.run([fuzz_bin, str(64 << 20), "0"], input=data, capture_output=True, timeout=120,
                       env={**os.environ, "ASAN_OPTIONS": "abort_on_error=1:detect_leaks=1",
                            "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", **env})
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err[-4000:]
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    lines = p.stdout.decode().splitlines()
    assert lines[-1].startswith("CLOSED live=0 account=0"), lines[-3:]
    return lines


def _walk_stream(seed: int) -> bytes:
    """Batches of queued frames with their closers, sized so that batches
    straddle the reader's 64 KB buffer at every offset, and one hostile tail:
    a length that wraps, one just past the frame limit, or a cut header."""
    import random

    rng = random.Random(seed)
    out = [alloc_at(1, 1 << 16)]
    for _ in range(rng.randrange(150, 300)):
        for _ in range(rng.randrange(0, 12)):
            pick = rng.randrange(5)
            if pick == 0:
                out.append(fill(1, rng.randrange(0, 1 << 16)))
            elif pick == 1:
                out.append(rand(1, rng.randrange(0, 1 << 13)))
            elif pick == 2:
                out.append(rand(77, 16))  # no such buffer: a deferred failure in the batch
            elif pick == 3:
                out.append(post(SYNC, bytes(rng.randrange(0, 2000))))  # padding the walk has to step over
            else:
                out.append(reduce_(1, rng.randrange(0, 1 << 13), flags=NO_REPLY))
        closer = rng.randrange(3)
        out.append(rand_reduce(rng.randrange(0, 1 << 24), seed=rng.randrange(1 << 16)) if closer == 0
                   else reduce_(1, rng.randrange(0, 1 << 13)) if closer == 1 else sync())
    tail = rng.randrange(4)
    out.append(fill(1, 64))
    if tail == 0:
        out.append(struct.pack("<IIQ", FILL, NO_REPLY, (1 << 64) - rng.randrange(1, 64)))
    elif tail == 1:
        out.append(struct.pack("<IIQ", RAND_REDUCE, 0, (16 << 20) + 1))  # the stdin reader's limit is 16 MiB
    elif tail == 2:
        out.append(rand_reduce(1000)[: rng.randrange(1, 16)])
    else:
        out.append(rand_reduce(1000)[: rng.randrange(16, 63)])
    return b"".join(out)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_walk_over_hostile_streams_changes_no_reply(fuzz_bin, seed):
    """Every frame's status and reply bytes are the same with the plan on
    and off, and the sanitizers see nothing."""
    data = _walk_stream(seed)
    on = _stdin_run(fuzz_bin, data)
    off = _stdin_run(fuzz_bin, data, BEE_BROKER_LANES="0")
    assert len(on) > 300
    assert on == off

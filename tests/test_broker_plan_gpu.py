"""The broker's batch plan on a real MI355X: every value a sandbox gets is
the same, bit for bit, with the priority lane on (the default) and off
(BEE_BROKER_LANES=0).

One service per setting, each running the same three sandbox scripts through
a real broker session; the scripts print every scalar as a hex float.
"""

import os
import tempfile

import pytest

from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

# the headline payload's sequence (examples/benchmark_numpy_gpu.py) at
# 256 x 256: [draws, GEMM, draw-reduce], then the all-short batches
# [rowsum, sum] and [colsum, cast, GEMV, max_abs_diff] of a drained session
# (priority lane), then the next round's first batch (back to the normal lane
# where its draw-reduce is long: n = 2^22 + 1 is the smallest such; with
# n = 1000 every batch is short).
PAYLOAD = """
import beekern as bk
def payload(n):
    bk.random.seed(1234)
    a = bk.random.uniform(-1, 1, (256, 256), dtype="bfloat16")
    b = bk.random.uniform(-1, 1, (256, 256), dtype="bfloat16")
    c = bk.matmul(a, b.T)
    x = bk.random.rand(n)
    result = bk.sum(bk.square(x))
    rows = bk.sum(c, axis=1)
    checksum = bk.sum(rows)
    s = bk.sum(b, axis=0).astype("bfloat16").reshape(1, 256)
    ref = bk.gemm_bf16_tn(a, s, out_dtype="float32").reshape(256)
    return result, checksum, bk.max_abs_diff(rows, ref)
for n in (1000, (1 << 22) + 1, 1000):
    print(n, *[float(v).hex() for v in payload(n)])
"""

# a long op (a unary over 16 MiB + 8 bytes of f64) and a wait; a short batch
# that reads its output (normal lane -> priority lane); a long batch that
# overwrites it (and back); a last short batch
LANES = """
import os, beekern as bk
from bee_code_interpreter_fs_amd.ops.driver import BrokerDriver
d = BrokerDriver(os.environ["BEE_BROKER_SOCK"]); d.init(0)
n = (1 << 21) + 1
x = d.malloc(8 * n); y = d.malloc(8 * n)
d.rand(0, x, n, 1, 99, 0, 0.0, 1.0)
d.unary(3, 1, x, y, n)            # y = sqrt(x)
d.sync()
print(d.reduce(0, 1, y, 0, 4096).hex())          # short: sum of y[:4096]
d.unary(0, 1, x, y, n)            # y = x * x, long
print(d.reduce(0, 1, y, 0, n).hex())             # long: sum of all of y
d.unary(1, 1, y, y, 4096)         # short again, in place
print(d.reduce(3, 1, y, 0, 4096).hex(), d.reduce(0, 1, x, 0, 4096).hex())
"""

# forty sessions one after another, each on a pooled context: an even one
# ends on the priority lane, the odd one after it starts with a long batch
SESSIONS = """
import os, beekern as bk
from bee_code_interpreter_fs_amd.ops.driver import BrokerDriver
n_long = (1 << 21) + 1
for i in range(40):
    d = BrokerDriver(os.environ["BEE_BROKER_SOCK"]); d.init(0)
    out = []
    if i % 2:
        h = d.malloc(8 * n_long)
        d.rand(0, h, n_long, 1, 1000 + i, 0, 0.0, 1.0)
        out.append(d.reduce(0, 1, h, 0, n_long))
    s = d.malloc(8 * 4096)
    d.rand(0, s, 4096, 1, 2000 + i, 0, 0.0, 1.0)
    out.append(d.reduce(0, 1, s, 0, 4096))
    out.append(d.rand_reduce(1, 1, 1000 + i, 3000 + i, 0, 0.0, 1.0))
    print(i, *[v.hex() for v in out])
    d.sock.close()
"""

SCRIPTS = {"payload": PAYLOAD, "lanes": LANES, "sessions": SESSIONS}


def _serve_all(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ensure_native_executor()
        h = ServiceHarness(tempfile.mkdtemp(prefix="bee-plan-"), gpu_ids=[0], workers_per_gpu_target=1,
                           default_timeout=120.0)
        h.start()  # (the daemon inherits the switches)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        out = {}
        for name, code in SCRIPTS.items():
            r = h.call(h.ctx.code_executor.execute(source_code=code, timeout=120), timeout=300)
            assert r.exit_code == 0, (name, r.stdout, r.stderr)
            out[name] = r.stdout
        return out
    finally:
        h.stop()


@pytest.fixture(scope="module")
def served():
    """stdout of every script, with the plan on and off."""
    on = _serve_all({"BEE_BROKER_LANES": "1"})
    off = _serve_all({"BEE_BROKER_LANES": "0"})
    return on, off


def _floats(line):
    return [float.fromhex(v) for v in line.split()[1:]]


def test_payload_sequence_is_bit_equal(served):
    on, off = served
    assert on["payload"] == off["payload"]
    lines = on["payload"].splitlines()
    assert [int(ln.split()[0]) for ln in lines] == [1000, (1 << 22) + 1, 1000]
    for ln in lines:
        n = int(ln.split()[0])
        result, checksum, row_err = _floats(ln)
        # sum of n squared uniforms: mean n / 3, standard deviation sqrt(4 n / 45); six of them
        assert abs(result - n / 3) < 6 * (4 * n / 45) ** 0.5, ln
        # rowsum(A @ B.T) against A @ bf16(colsum(B)): the column sums (|s| < ~50) round to bf16 within
        # 2^-9 |s| = 0.1, and 256 such errors times |a| < 1 with random signs stay under a tenth of this
        assert row_err < 8.0, ln


def test_lane_changes_in_both_directions_are_bit_equal(served):
    on, off = served
    assert on["lanes"] == off["lanes"]
    v = [float.fromhex(t) for t in on["lanes"].split()]
    n = (1 << 21) + 1
    assert len(v) == 4
    assert abs(v[0] - 4096 * 2 / 3) < 6 * (4096 / 18) ** 0.5   # sqrt(u): mean 2/3, variance 1/18
    assert abs(v[1] - n / 3) < 6 * (4 * n / 45) ** 0.5           # u * u over all of y
    assert 0.0 < v[2] <= 1.0                                     # max of |y[:4096]|
    assert abs(v[3] - 4096 / 2) < 6 * (4096 / 12) ** 0.5         # x itself is untouched


def test_forty_sessions_on_pooled_contexts_are_bit_equal(served):
    on, off = served
    assert on["sessions"] == off["sessions"]
    lines = on["sessions"].splitlines()
    assert [int(ln.split()[0]) for ln in lines] == list(range(40))
    for i, ln in enumerate(lines):
        v = _floats(ln)
        assert len(v) == (3 if i % 2 else 2)
        assert abs(v[-2] - 4096 / 2) < 6 * (4096 / 12) ** 0.5, ln           # sum of 4096 uniforms
        assert abs(v[-1] - (1000 + i) / 3) < 6 * (4 * (1000 + i) / 45) ** 0.5, ln

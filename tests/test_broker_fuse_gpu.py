"""The broker's fused pairs on a real MI355X: the headline payload's two short
batches -- [rowsum, sum] and [colsum, cast, GEMV, max_abs_diff] -- give a
sandbox the same bits with the pairs fused (the default) and not
(BEE_BROKER_FUSE=0), and the fused service launches three kernels fewer per
payload.

One service per setting, in the pattern of tests/test_broker_plan_gpu.py; the
script prints every scalar as a hex float and every vector as its bytes.
"""

import os
import tempfile

import pytest

from .harness import ServiceHarness, ensure_native_executor

pytestmark = pytest.mark.gpu

ROUNDS = 3
# examples/benchmark_numpy_gpu.py at 256 x 256, as tests/test_broker_plan_gpu.py
# runs it: the 256 row sums and the GEMV's 256 outputs are within the closing
# reduction's single block, as the payload's 4096 are
PAYLOAD = """
import beekern as bk
def payload(seed):
    bk.random.seed(seed)
    a = bk.random.uniform(-1, 1, (256, 256), dtype="bfloat16")
    b = bk.random.uniform(-1, 1, (256, 256), dtype="bfloat16")
    c = bk.matmul(a, b.T)
    x = bk.random.rand(1000)
    result = bk.sum(bk.square(x))
    rows = bk.sum(c, axis=1)
    checksum = bk.sum(rows)
    s = bk.sum(b, axis=0).astype("bfloat16").reshape(1, 256)
    ref = bk.gemm_bf16_tn(a, s, out_dtype="float32").reshape(256)
    err = bk.max_abs_diff(rows, ref)
    return [result, checksum, err], [rows, s, ref]
for seed in range(%d):
    scalars, vectors = payload(seed)
    print(seed, *[float(v).hex() for v in scalars], *[v.numpy().tobytes().hex() for v in vectors])
""" % ROUNDS


def _serve(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ensure_native_executor()
        h = ServiceHarness(tempfile.mkdtemp(prefix="bee-fuse-"), gpu_ids=[0], workers_per_gpu_target=1, default_timeout=120.0)
        h.start()  # (the daemon inherits the switch)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        status = lambda: h.call(h.ctx.code_executor.slots[0].executor.get_json("/v1/status"), timeout=30)  # noqa: E731
        ops0 = status()["broker"]["gpu_ops"]
        r = h.call(h.ctx.code_executor.execute(source_code=PAYLOAD, timeout=120), timeout=300)
        assert r.exit_code == 0, (r.stdout, r.stderr)
        return r.stdout, status()["broker"]["gpu_ops"] - ops0
    finally:
        h.stop()


@pytest.fixture(scope="module")
def served():
    return _serve({"BEE_BROKER_FUSE": "1"}), _serve({"BEE_BROKER_FUSE": "0"})


def test_short_batches_are_bit_equal_fused_and_unfused(served):
    (on, _), (off, _) = served
    assert on == off
    lines = on.splitlines()
    assert [int(ln.split()[0]) for ln in lines] == list(range(ROUNDS))
    for ln in lines:
        result, checksum, err = [float.fromhex(v) for v in ln.split()[1:4]]
        # the bounds of tests/test_broker_plan_gpu.py: six standard deviations of the sum of 1000 squared uniforms;
        # rowsum(A @ B.T) against A @ bf16(colsum(B))
        assert abs(result - 1000 / 3) < 6 * (4 * 1000 / 45) ** 0.5, ln
        assert err < 8.0, ln


def test_fused_service_launches_three_kernels_fewer_per_payload(served):
    """rowsum + sum, colsum + cast and GEMV + max_abs_diff go out as one launch
    each (the broker's count of the ops it timed)."""
    (_, ops_on), (_, ops_off) = served
    assert ops_off - ops_on == 3 * ROUNDS, (ops_on, ops_off)

"""Headline benchmark: Execute RPCs/sec + p50 latency of the benchmark-numpy
payload on N GPU-pinned executor pods (BASELINE.json metric / configs 3-5).

    python bench.py --gpus N --steps K --warmup W
    torchrun --nproc-per-node N bench.py --gpus N --steps K --warmup W

Topology: rank 0 starts the service as its own process tree, exactly as it
is deployed (``python -m bee_code_interpreter_fs_amd``): a supervisor owning
one native bee-executor per GPU (warm single-use sandboxes pinned to that
MI355X + the GPU's kernel broker) and ``--frontends`` gRPC/HTTP replicas on
one SO_REUSEPORT port.  Every rank runs ``--concurrency`` closed-loop gRPC
clients (one connection each), so offered load grows with N (weak
scaling).  One "step" = one Execute RPC per client of the payload
(examples/benchmark_numpy_gpu.py: 1e8 f64 Philox rand + fused square-sum +
4096^3 bf16 MFMA GEMM on the sandbox's GPU; result and GEMM checked); a
rank's K steps are its K x concurrency Executes, which its clients take from
one shared budget (closed loop, next request as soon as the previous one
returns), so the timed window ends when the work does, not when the unluckiest
client's K-th request does.
K steps are timed between a barrier + torch.cuda.synchronize() on every
rank; time = max over ranks; ``value`` = completed RPCs / that time.
A plain run does only that: set up, warm up, time the K steps, print the
headline line.  ``--dump-outputs DIR`` also writes what the last timed
step's Executes returned (the numbers the payload printed) as DIR/<name>.npy;
the payload's draws are seeded (``--seed``), so the same arguments give the
same inputs and two builds can be compared output for output.

``--full`` adds everything else to the line: the idle-CPU profile, CPU and
GPU time per Execute by role, the materialised-draw run, executor, admission
and memory figures, what bounds the node, and for N>1 BASELINE config 5
through the service: one gang Execute with gpus=N whose ranks all-reduce
over RCCL/xGMI.
"""

from __future__ import annotations

import argparse
import asyncio
import gc
import json
import math
import os
import shutil
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PAYLOAD = os.path.join(ROOT, "examples", "benchmark_numpy_gpu.py")
MATERIALIZED = os.path.join(ROOT, "examples", "benchmark_numpy_gpu_materialized.py")
EXPECTED = 10**8 / 3  # E[sum U^2]
N_DRAWS = 10**8
# sum of n U^2 (U ~ U[0,1)): variance n * (E[U^4] - E[U^2]^2) = n * (1/5 - 1/9) = n * 4/45
RESULT_SIGMA = (N_DRAWS * 4 / 45) ** 0.5  # ~2981


def result_ok(value: float, sigmas: float = 6.0) -> bool:
    """The payload's Result against its distribution: within 6 sigma of
    E = n/3 (a fair draw fails this about once in 5e8 runs; a wrong kernel,
    a truncated draw or a reduction that drops a block does not pass)."""
    return abs(value - EXPECTED) <= sigmas * RESULT_SIGMA


GEMM_ROW_TOL = 64.0


def gemm_row_ok(max_row_error: float) -> bool:
    """The payload's row check of its 4096^3 bf16 GEMM: max_i |rowsum(C)_i -
    (A @ colsum(B))_i|.  A correct GEMM stays within a few units (bf16
    rounding of C and of colsum(B): sigma ~2 per row); one corrupt 256x256
    tile shifts 256 row sums by ~300 each (tests/test_bench_cpu.py emulates
    both)."""
    return 0.0 <= max_row_error <= GEMM_ROW_TOL

# BASELINE.json configs; "numpy_gpu" is the headline (metric + config the
# driver records), the others are reported by tools/bench_suite.py.
WORKLOADS = {
    "numpy_gpu": (
        "examples/benchmark_numpy_gpu.py",
        "Execute RPCs/sec (benchmark-numpy payload via HIP kernels)",
        "benchmark-numpy.py payload: 1e8 f64 rand+square+sum + 4096^3 bf16 GEMM per Execute",
        "float64 (rand/square/sum) + bf16 (GEMM)",
    ),
    "numpy_cpu": (
        # the reference's payload verbatim; --numpy-offload runs it on the GPU
        # (ops/numpy_offload.py), without it numpy runs on the CPU
        "examples/benchmark_numpy_reference.py",
        "Execute RPCs/sec (unmodified benchmark-numpy payload, numpy on CPU)",
        "benchmark-numpy.py payload: 1e8 f64 numpy rand+square+sum per Execute",
        "float64",
    ),
    "fib": (
        "examples/benchmark_fib.py",
        "Execute RPCs/sec (benchmark-fib payload, GPU-pinned executor)",
        "benchmark-fib.py payload: 1000 x fib(10000) Python bigint per Execute",
        "python int",
    ),
    "scientific": (
        "examples/scientific_stack.py",
        "Execute RPCs/sec (numpy/pandas/scipy t-test payload, light sandboxes)",
        "using_imports-style payload: pandas DataFrame describe + scipy.stats t-test per Execute",
        "float64",
    ),
    "hello": (
        "examples/hello_world.py",
        "Execute RPCs/sec (hello_world plumbing)",
        "hello_world payload: print per Execute",
        "n/a",
    ),
}


# the sandbox kind each workload's payload is routed to
ROUTED_POOL = {"numpy_gpu": "nano", "numpy_cpu": "min", "fib": "nano_cpu", "hello": "nano_cpu", "scientific": "light"}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=600)  # per client: 4800 Executes on 1 GPU, ~2 s
    # untimed: 400 Executes on 1 GPU bring the allocator caches, sandbox
    # pools and zygote page state to steady state (30 timed steps after 10
    # warm-up steps ran at 1836 RPS vs ~2700 sustained, profiles/archive/r2_s3_bench_suite.jsonl)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--concurrency", type=int, default=8, help="closed-loop clients per GPU")
    p.add_argument("--clients-per-loadgen", type=int, default=0,
                   help="clients per load-generator process (single-process runs; 0 = all of a GPU's clients in one)")
    p.add_argument("--pool-target", type=int, default=16, help="warm minimal sandboxes per GPU")
    p.add_argument("--frontends", type=int, default=0, help="front-end replicas (0 = three per GPU, at most 16)")
    p.add_argument("--workload", choices=sorted(WORKLOADS), default="numpy_gpu")
    p.add_argument("--payload", default=None, help="override the workload's script")
    p.add_argument("--cpu-only", action="store_true", help="executors without GPUs (BASELINE config 1)")
    p.add_argument("--virtual-gpus", action="store_true",
                   help="CPU rehearsal of an N-GPU node: N executors pinned to GPU ids 0..N-1 that need not exist "
                        "(no kernel broker, no HIP warm-up); use with a CPU workload such as --workload hello")
    p.add_argument("--no-gang-check", action="store_true")
    p.add_argument("--idle-probe", type=float, default=2.0,
                   help="seconds the service sits idle after READY, before the clients (with --full its CPU is sampled "
                        "meanwhile); 0 = skip")
    p.add_argument("--fold", action="store_true",
                   help="keep one executor daemon (broker, HIP context, pools) per requested GPU even when fewer GPUs "
                        "are visible: the N-GPU node's topology rehearsed on this box")
    p.add_argument("--max-inflight", type=int, default=0,
                   help="admitted executions per GPU (each daemon's bound for all front-ends; 0 = 2 x concurrency)")
    p.add_argument("--numpy-offload", action="store_true",
                   help="Execute with numpy_offload=True: numpy.random draws of the payload live on the sandbox's GPU "
                        "and numpy calls on them run on the beekern kernels (ops/numpy_offload.py)")
    p.add_argument("--materialized-steps", type=int, default=-1,
                   help="with --full: steps of the secondary materialised-draw run (numpy's HBM traffic; "
                        "-1 = min(steps, 20), 0 = skip)")
    p.add_argument("--full", action="store_true",
                   help="everything beside the headline figure: the idle-CPU profile, CPU / GPU time per Execute by role, "
                        "the materialised-draw run, the gang all-reduce check (N > 1), admission checks, executor and "
                        "memory statistics, what bounds the node.  Without it a run sets up, warms up, times the steps "
                        "and prints the headline line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step's Executes returned (every number a "
                        "payload printed, and the exit codes) as DIR/<name>.npy, float64")
    p.add_argument("--seed", type=int, default=20240611,
                   help="seed of the payload's random draws (beekern / numpy.random): the same arguments give the same "
                        "inputs, so two builds can be compared output for output")
    return p.parse_args()


_SEED_PROLOGUE = (
    # (module the payload imports, the line that seeds its global generator)
    ("beekern", "import beekern as _bee_seed; _bee_seed.random.seed({seed}); del _bee_seed\n"),
    ("numpy", "import numpy as _bee_seed; _bee_seed.random.seed({seed}); del _bee_seed\n"),
)


def seeded(source: str, seed: int) -> str:
    """The payload with its random generators seeded: one line in front per
    generator module the payload itself imports (none is added that it does
    not import, so it is routed to the same sandbox kind).  Every Execute of a
    run sends the same text -- the service's per-source caches (routing,
    precompiled payload) work as for any re-submitted script -- and so draws
    the same inputs."""
    import re

    lines = [line.format(seed=seed) for mod, line in _SEED_PROLOGUE
             if re.search(rf"^\s*(?:import|from)\s+{mod}\b", source, re.M)]
    return "".join(lines) + source


_NUMBER_LINE = None


def printed_numbers(stdout: str) -> dict:
    """{label: value} of a payload's ``Label: number`` lines -- what a caller
    of Execute gets back -- without its own wall-clock line."""
    global _NUMBER_LINE
    if _NUMBER_LINE is None:
        import re

        _NUMBER_LINE = re.compile(r"^([A-Za-z][\w ]*?):[ \t]*(\S+)", re.M)
    out = {}
    for label, value in _NUMBER_LINE.findall(stdout):
        if label == "Execution Time" or label in out:
            continue
        try:
            out[label] = float(value)
        except ValueError:
            pass
    return out


def dump_outputs(directory: str, last_step) -> list:
    """``last_step``: (load generator, request index, exit code, stdout) of
    the last timed step's Executes.  One float64 array per printed label (in
    load-generator, then request order; NaN where an Execute did not print
    it) and ``exit_code``; returns the file names."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    rows = [(rc, printed_numbers(text)) for _, _, rc, text in sorted(last_step, key=lambda r: (r[0], r[1]))]
    arrays = {"exit_code": [float(rc) for rc, _ in rows]}
    for label in sorted({k for _, nums in rows for k in nums}):
        name = "_".join(label.lower().split())
        arrays[name] = [nums.get(label, float("nan")) for _, nums in rows]
    for name, values in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), np.asarray(values, dtype=np.float64))
    return sorted(name + ".npy" for name in arrays)


def dist_env():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return world, rank, local


def percentile(xs, q):
    if not xs:
        return None
    xs = sorted(xs)
    k = max(0, min(len(xs) - 1, int(round(q / 100.0 * (len(xs) - 1)))))
    return xs[k]


def visible_gpus() -> int:
    import torch

    return max(torch.cuda.device_count(), 1)


def cpu_usage_s():
    """(seconds of CPU used by this container so far, source) -- cgroup v2,
    cgroup v1 cpuacct, or the host's /proc/stat busy time as a fallback."""
    try:
        with open("/sys/fs/cgroup/cpu.stat") as f:
            for line in f:
                if line.startswith("usage_usec"):
                    return int(line.split()[1]) / 1e6, "cgroup2"
    except OSError:
        pass
    try:
        with open("/sys/fs/cgroup/cpuacct/cpuacct.usage") as f:
            return int(f.read()) / 1e9, "cgroup1"
    except OSError:
        pass
    with open("/proc/stat") as f:
        v = [int(x) for x in f.readline().split()[1:]]
    return (sum(v) - v[3] - v[4]) / os.sysconf("SC_CLK_TCK"), "procstat"


def cpu_throttle(paths=(("/sys/fs/cgroup/cpu.stat", 1.0), ("/sys/fs/cgroup/cpu/cpu.stat", 1e-3))) -> dict:
    """The container's CFS bandwidth counters (cgroup v2 cpu.stat or v1
    cpu/cpu.stat): enforcement periods, periods in which the quota ran out,
    and the time processes sat throttled -- {} without a quota."""
    for path, scale in paths:
        try:
            with open(path) as f:
                kv = dict(line.split() for line in f if len(line.split()) == 2)
        except OSError:
            continue
        if "nr_periods" in kv:
            t = kv.get("throttled_usec") if scale == 1.0 else kv.get("throttled_time")
            return {"periods": int(kv["nr_periods"]), "throttled": int(kv.get("nr_throttled", 0)),
                    "throttled_ms": int(t or 0) * scale / 1e3}
    return {}


def throttle_delta(a: dict, b: dict):
    if not a or not b:
        return None
    return {"periods": b["periods"] - a["periods"], "throttled_periods": b["throttled"] - a["throttled"],
            "throttled_ms": round(b["throttled_ms"] - a["throttled_ms"], 1)}


def _proc_times(pid: int):
    """(own CPU s, reaped children's CPU s) of a process, from /proc/<pid>/stat."""
    with open(f"/proc/{pid}/stat") as f:
        fields = f.read().rsplit(")", 1)[1].split()
    tck = os.sysconf("SC_CLK_TCK")
    return (int(fields[11]) + int(fields[12])) / tck, (int(fields[13]) + int(fields[14])) / tck


def _children(pid: int):
    out = []
    try:
        for tid in os.listdir(f"/proc/{pid}/task"):
            with open(f"/proc/{pid}/task/{tid}/children") as f:
                out.extend(int(x) for x in f.read().split())
    except OSError:
        pass
    return out


def cpu_by_role(service_pid):
    """CPU seconds so far of the service's processes by role: front-end
    replicas, executor daemons (+ their kernel broker threads), zygotes (the
    forks) and sandboxes (reaped children of the zygotes; live ones count
    once reaped), plus this bench process and its load generators."""
    roles = {"frontend": 0.0, "executor_daemon": 0.0, "zygote": 0.0, "sandboxes": 0.0, "bench_clients": 0.0}
    t = os.times()
    roles["bench_clients"] = t.user + t.system + t.children_user + t.children_system
    if service_pid is None:
        return roles
    stack, seen = [service_pid], set()
    while stack:
        pid = stack.pop()
        if pid in seen:
            continue
        seen.add(pid)
        try:
            with open(f"/proc/{pid}/cmdline", "rb") as f:
                cmd = f.read()
            own, reaped = _proc_times(pid)
        except OSError:
            continue
        if b"bee-executor" in cmd:
            roles["executor_daemon"] += own + reaped
            stack.extend(_children(pid))
        elif b"zygote" in cmd:
            roles["zygote"] += own
            roles["sandboxes"] += reaped  # live sandboxes: counted when reaped
        else:
            roles["frontend"] += own + reaped
            stack.extend(_children(pid))
    return roles


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def gpu_ids(n_gpus: int, args):
    """One executor per GPU; a run with more ranks than visible GPUs folds the
    extra ranks onto the existing devices (and says so in the JSON).  With
    --fold, every rank keeps an executor daemon of its own -- N daemons,
    brokers and HIP contexts -- on the visible GPUs: the N-GPU node's process
    topology rehearsed on fewer GPUs."""
    if args.virtual_gpus:
        return list(range(n_gpus))
    if args.fold:
        return [i % visible_gpus() for i in range(n_gpus)]
    return sorted({i % visible_gpus() for i in range(n_gpus)})


def cpu_quota_cores() -> tuple:
    """(CPUs of time this job may use per period, source): the cgroup CPU
    quota (scheduler/topology.py cpu_quota), else the CPUs it may run on."""
    from bee_code_interpreter_fs_amd.scheduler.topology import cpu_quota

    q = cpu_quota()
    if q > 0:
        return q, "cgroup cpu.max"
    try:
        return float(len(os.sched_getaffinity(0))), "affinity"
    except (AttributeError, OSError):
        return float(os.cpu_count() or 1), "cpu_count"


def frontends_for(n_slots: int, quota: float) -> int:
    """Front-end replicas: three per GPU slot (measured on one GPU: a
    replica saturates a core at ~2.2k Execute/s, and a third one per GPU
    took p50 down, profiles/archive/r2_s3_frontends3_ab.log), but no more
    than one per ~5 cores of the CPU quota -- at ~4.5 ms of CPU per Execute a
    5-core share carries ~1.1k Execute/s, half a replica's capacity; 24
    replicas on a 16-core quota (8 slots folded onto one GPU box) would only
    add processes that compete with the sandboxes for the same quota."""
    per_gpu = 3 * max(1, n_slots)
    return max(min(3, per_gpu), min(per_gpu, int(math.ceil(quota / 5.0))), 1)


def pss_by_role(service_pid):
    """Proportional set size (MB) of the service's processes by role: a
    shared page counts once across the node (smaps_rollup Pss)."""
    roles = {"frontend": 0.0, "executor_daemon": 0.0, "zygote": 0.0, "pooled_sandboxes": 0.0}
    if service_pid is None:
        return roles
    stack, seen = [(service_pid, None)], set()
    while stack:
        pid, parent_role = stack.pop()
        if pid in seen:
            continue
        seen.add(pid)
        try:
            with open(f"/proc/{pid}/cmdline", "rb") as f:
                cmd = f.read()
            with open(f"/proc/{pid}/smaps_rollup") as f:
                pss = next((int(l.split()[1]) for l in f if l.startswith("Pss:")), 0) / 1024.0
        except (OSError, StopIteration, ValueError):
            continue
        role = ("pooled_sandboxes" if parent_role == "zygote" else "executor_daemon" if b"bee-executor" in cmd
                else "zygote" if b"zygote" in cmd else "frontend")
        roles[role] += pss
        stack.extend((c, role) for c in _children(pid))
    return {k: round(v, 1) for k, v in roles.items()}


def daemon_threads(service_pid):
    """CPU seconds so far of the executor daemons' threads, summed by thread
    name (csrc/executor/util.cpp names them by role: http, refill, broker,
    watchdog, ...) over every daemon of the service."""
    out = {}
    if service_pid is None:
        return out
    tck = os.sysconf("SC_CLK_TCK")
    stack, seen = [service_pid], set()
    while stack:
        pid = stack.pop()
        if pid in seen:
            continue
        seen.add(pid)
        try:
            with open(f"/proc/{pid}/cmdline", "rb") as f:
                cmd = f.read()
        except OSError:
            continue
        if b"bee-executor" not in cmd:
            stack.extend(_children(pid))
            continue
        try:
            tids = os.listdir(f"/proc/{pid}/task")
        except OSError:
            continue
        for tid in tids:
            try:
                with open(f"/proc/{pid}/task/{tid}/stat") as f:
                    raw = f.read()
                name = raw[raw.index("(") + 1: raw.rindex(")")]
                fields = raw.rsplit(")", 1)[1].split()
                out[name] = out.get(name, 0.0) + (int(fields[11]) + int(fields[12])) / tck
            except (OSError, ValueError):
                continue
    return out


def idle_profile(service_pid, seconds: float):
    """The service's CPU with no requests in flight (pools full, READY):
    cores by role and the daemons' busiest threads -- fixed overhead that
    every slot of the node pays whatever its load."""
    r0, t0, c0 = cpu_by_role(service_pid), daemon_threads(service_pid), time.perf_counter()
    time.sleep(seconds)
    r1, t1, dt = cpu_by_role(service_pid), daemon_threads(service_pid), time.perf_counter() - c0
    threads = {k: round((t1.get(k, 0.0) - v) / dt, 3) for k, v in t0.items()}
    return {"seconds": round(dt, 2),
            "cores_by_role": {k: round((r1[k] - r0[k]) / dt, 3) for k in r0 if k != "bench_clients"},
            "daemon_thread_cores": dict(sorted(((k, v) for k, v in threads.items() if v > 0.001),
                                               key=lambda kv: -kv[1])[:12])}


_GPU_TIME: dict = {}  # slot_executions' last GPU-time read, by the list it returned


def slot_executions(hport):
    """Executions so far of every GPU slot's daemon (for the per-slot
    balance of the timed region); the same status read's kernel-broker GPU
    time (gpu_time_of) rides along."""
    import urllib.request

    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{hport}/v1/status", timeout=10) as f:
            st = json.load(f)
        out = [int(s["executor"].get("executions", 0)) for s in st["slots"]]
        _GPU_TIME[id(out)] = [(s["executor"].get("broker") or {}) for s in st["slots"]]
        return out
    except Exception:  # noqa: BLE001
        return None


def gpu_time_of(slots0, slots1, total, elapsed):
    """The GPU side of the timed window from the kernel brokers' event-timed
    ops (csrc/executor/broker.cpp "GPU time per op"): per Execute, the busy
    time (the union of the kernels' intervals on each GPU's clock: sessions
    overlapping on one GPU count once) and the summed kernel durations; the
    busy fraction of the window; and the rate the GPUs would allow at that
    busy time per Execute, next to cpu_bound_rps (VERDICT r5 "next" #2)."""
    b0, b1 = _GPU_TIME.get(id(slots0)), _GPU_TIME.get(id(slots1))
    if not b0 or not b1 or len(b0) != len(b1) or not total or elapsed <= 0:
        return None
    if not all(x.get("gpu_timing") for x in b1):
        return {"timing": "off"}
    busy = sum(y.get("gpu_busy_ms", 0.0) - x.get("gpu_busy_ms", 0.0) for x, y in zip(b0, b1))
    ops_ms = sum(y.get("gpu_op_ms", 0.0) - x.get("gpu_op_ms", 0.0) for x, y in zip(b0, b1))
    ops = sum(y.get("gpu_ops", 0) - x.get("gpu_ops", 0) for x, y in zip(b0, b1))
    per = busy / total
    return {
        "gpu_ms_per_exec": round(per, 4),           # busy GPU time per Execute (union of kernel intervals)
        "kernel_ms_per_exec": round(ops_ms / total, 4),  # summed kernel durations (overlap counted twice)
        "kernels_per_exec": round(ops / total, 2),
        "gpu_utilisation": round(busy / (elapsed * 1e3 * len(b1)), 3),  # of the window, mean over GPUs
        "gpu_bound_rps": round(len(b1) * 1e3 / per, 1) if per > 0 else None,
    }


def start_service(tmp: str, n_gpus: int, args):
    gport, hport = free_port(), free_port()
    # three front-end replicas per GPU: one Python gRPC process saturates a
    # core at ~2.2k Execute/s (2235 -> 2378 RPS with a second replica on one
    # GPU, profiles/archive/r2_bench_frontends_ab.log); a third took p50 down
    # in 3 of 3 interleaved pairs, 2794 vs 2734 RPS mean
    # (profiles/archive/r2_s3_frontends3_ab.log).  The same three per GPU at
    # every N keeps each replica's share of the offered load (8 clients per
    # GPU) what it is on one GPU -- weak scaling of the front-end too (24 at
    # N = 8; front-ends hold no GPU context)
    frontends = args.frontends or frontends_for(len(gpu_ids(n_gpus, args)) if not args.cpu_only else 1,
                                                cpu_quota_cores()[0])
    routed = None if args.payload else ROUTED_POOL[args.workload]

    def pool(kind: str) -> str:
        return str(args.pool_target if routed is None or routed == kind else min(args.pool_target, 4))

    env = dict(os.environ)
    env.update(
        {
            "APP_GRPC_LISTEN_ADDR": f"127.0.0.1:{gport}",
            "APP_HTTP_LISTEN_ADDR": f"127.0.0.1:{hport}",
            # one executor per physical GPU (a rehearsal with more ranks than
            # GPUs folds the extra ranks onto the existing devices)
            "APP_GPU_IDS": "[]" if args.cpu_only else json.dumps(gpu_ids(n_gpus, args)),
            "APP_FILE_STORAGE_PATH": os.path.join(tmp, "files"),
            "APP_SANDBOX_ROOT": os.path.join(tmp, "sandboxes"),
            "APP_WORKERS_PER_GPU_TARGET": "1",  # direct sandboxes: the payload does not need them
            # the pool the workload's payload routes to (local_gpu_pool.py
            # _mode_of_source) gets --pool-target warm sandboxes per GPU, the
            # others a few: fewer idle processes on an 8-GPU node
            "APP_MIN_WORKERS_PER_GPU_TARGET": pool("min"),
            "APP_NANO_WORKERS_PER_GPU_TARGET": os.environ.get("APP_NANO_WORKERS_PER_GPU_TARGET", pool("nano")),
            "APP_NANO_CPU_WORKERS_PER_GPU_TARGET": pool("nano_cpu"),
            # light sandboxes (pandas/scipy/matplotlib preloaded) serve the
            # scientific workload; the others only keep a few warm
            "APP_LIGHT_WORKERS_PER_GPU_TARGET": str(args.pool_target if args.workload == "scientific" else 4),
            "APP_LIGHT_ZYGOTES_PER_GPU": "4" if args.workload == "scientific" else "2",
            "APP_MAX_INFLIGHT_PER_GPU": str(args.max_inflight or max(args.concurrency * 2, 8)),
            "APP_DEFAULT_TIMEOUT": "300",
            "APP_FRONTEND_PROCESSES": str(frontends),
            "APP_LOGGING_CONFIG": json.dumps(
                {"version": 1, "disable_existing_loggers": False, "root": {"level": "WARNING"}}
            ),
        }
    )
    if args.fold and len(set(gpu_ids(n_gpus, args))) < n_gpus:
        # folded slots share the card: no warm direct (HIP-context) sandboxes,
        # so the processes holding the GPU stay the slots' daemons (brokers)
        env["APP_WORKERS_PER_GPU_TARGET"] = "0"
    if args.virtual_gpus:
        # a CPU rehearsal of the node's scheduling: lean pools (one zygote of
        # each kind per slot), no kernel broker, no HIP warm-up
        env.update({"APP_BROKER_ENABLED": "false", "APP_WORKER_WARM_GPU": "false", "APP_WORKERS_PER_GPU_TARGET": "0",
                    "APP_LIGHT_WORKERS_PER_GPU_TARGET": "1", "APP_LIGHT_ZYGOTES_PER_GPU": "1",
                    "APP_MIN_ZYGOTES_PER_GPU": "1", "APP_MIN_WORKERS_PER_GPU_TARGET": str(min(args.pool_target, 4)),
                    "APP_NANO_WORKERS_PER_GPU_TARGET": "0"})
    env.pop("RANK", None), env.pop("WORLD_SIZE", None), env.pop("LOCAL_RANK", None)
    log = open(os.path.join(tmp, "service.log"), "ab")
    proc = subprocess.Popen(
        [sys.executable, "-m", "bee_code_interpreter_fs_amd"], env=env, stdout=subprocess.PIPE, stderr=log, cwd=ROOT
    )
    line = proc.stdout.readline()
    if not line.startswith(b"BEE_SERVICE_READY"):
        proc.kill()
        tail = open(os.path.join(tmp, "service.log"), "rb").read()[-3000:].decode(errors="replace")
        raise RuntimeError(f"service failed to start: {line!r}\n{tail}")
    # replicas' own ports: clients are spread over them evenly (as an L4
    # balancer would) instead of by SO_REUSEPORT's connection hash
    replicas = []
    for part in line.decode().split():
        if part.startswith("replicas=") and part != "replicas=":
            replicas = part.split("=", 1)[1].split(",")
    return proc, gport, hport, frontends, replicas


async def open_clients(targets, first_client, concurrency):
    """``concurrency`` clients, one gRPC channel (connection) each, global
    client g on targets[g % len(targets)] (the front-end replicas,
    round-robin over all ranks' clients), connected before anything is
    timed: the warm-up, timed and materialised phases reuse them, as a
    long-lived client would (a step is an Execute, not a TCP + HTTP/2
    handshake)."""
    import grpc

    from bee_code_interpreter_fs_amd.models import proto as pb

    chans = [grpc.aio.insecure_channel(targets[(first_client + i) % len(targets)],
                                       options=[("grpc.use_local_subchannel_pool", 1)]) for i in range(concurrency)]
    await asyncio.gather(*(asyncio.wait_for(c.channel_ready(), 60) for c in chans))
    return chans, [pb.CodeInterpreterServiceStub(c) for c in chans]


async def close_clients(chans):
    await asyncio.gather(*(c.close() for c in chans), return_exceptions=True)


async def client_loop(stub, pb, source, budget, out, trace=None, extra=None):
    lat, errors, exec_times, phases, checks, last = out
    while budget[0] > 0:
        budget[0] -= 1  # (one event loop: taken before the await, no race)
        index = budget[1] - budget[0] - 1  # of this request among the run's
        t = time.perf_counter()
        try:
            r = await stub.Execute(pb.ExecuteRequest(source_code=source, **(extra or {})), timeout=600)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e)[:300])
            continue
        t1 = time.perf_counter()
        lat.append((t1 - t) * 1e3)
        if index >= budget[2]:  # the last step's: what --dump-outputs writes
            last.append((index, r.exit_code, r.stdout))
        if trace is not None:
            trace.append((round(t1, 6), round((t1 - t) * 1e3, 3)))
        for k, v in r.timings_ms.items():
            phases.setdefault(k, []).append(v)
        ok = r.exit_code == 0
        try:
            if ok and "Result:" in r.stdout:  # benchmark-numpy payloads: check the math
                ok = result_ok(float(r.stdout.split("Result:")[1].split()[0]))
                checks["result_ok"] += ok
            if ok and "GEMM max row error:" in r.stdout:  # and every row of the GEMM
                ok = gemm_row_ok(float(r.stdout.split("GEMM max row error:")[1].split()[0])) and \
                    abs(float(r.stdout.split("GEMM checksum:")[1].split()[0])) < 1e9
                checks["gemm_ok"] += ok
            if ok and "Execution Time:" in r.stdout:
                exec_times.append(float(r.stdout.split("Execution Time:")[1].split()[0]) * 1e3)
        except (IndexError, ValueError):
            ok = False
        if not ok:
            errors.append(f"exit={r.exit_code} stdout={r.stdout[-200:]!r} stderr={r.stderr[-500:]!r}")


async def run_clients(stubs, source, n, trace=None, extra=None):
    """``n`` steps of ``len(stubs)`` closed-loop clients: ``n * len(stubs)``
    Executes, each client taking the next one from the shared budget as soon
    as its previous one returns (``hey -n N -c C`` style).  With a fixed
    ``n`` per client instead, the run would end with the slowest client's
    last requests while the others sit idle -- on a 20-step run the
    max-of-8 spread of 20 latencies, ~5% of the timed window at less than
    the offered concurrency."""
    from bee_code_interpreter_fs_amd.models import proto as pb

    out = ([], [], [], {}, {"result_ok": 0, "gemm_ok": 0}, [])
    budget = [n * len(stubs), n * len(stubs), (n - 1) * len(stubs)]  # left, all, first of the last step
    await asyncio.gather(*(client_loop(stub, pb, source, budget, out, trace, extra) for stub in stubs))
    return out


def _loadgen_main(targets, first, source, concurrency, warmup, steps, barrier, results, go=None, extra=None):
    """One load-generator process (single-process ``--gpus N`` runs start N
    of them, so offered load grows with N like the torchrun ranks do).
    ``barrier``: every load generator of this process tree has warmed up;
    ``go``: the parent has also synchronised with the other ranks -- the
    timed window starts on every rank at once."""
    sys.path.insert(0, ROOT)
    loop = asyncio.new_event_loop()
    chans = []
    try:
        chans, stubs = loop.run_until_complete(open_clients(targets, first, concurrency))
        loop.run_until_complete(run_clients(stubs, source, warmup, extra=extra))
        if os.environ.get("BEE_GC_FREEZE", "1") != "0":
            gc.collect()
            gc.freeze()  # this load generator's heap out of the timed window's collections
        barrier.wait()
        if go is not None:
            go.wait()
        t0 = time.perf_counter()
        out = loop.run_until_complete(run_clients(stubs, source, steps, extra=extra))
        results.put((time.perf_counter() - t0,) + tuple(out))
    except BaseException as e:  # noqa: BLE001 - report instead of hanging the barrier
        barrier.abort()
        if go is not None:
            go.abort()
        results.put((0.0, [], [f"loadgen failed: {e!r}"[:300]], [], {}, {}, []))
    finally:
        if chans:
            loop.run_until_complete(close_clients(chans))
        loop.close()


def run_loadgens(n_procs, targets, source, concurrency, warmup, steps, sync, marks=None, first=0, extra=None):
    """``n_procs`` client processes of ``concurrency`` clients each; times
    the steps between one barrier all of them (and this process) pass and
    their completion.  Returns the gathered tuples (elapsed per process)."""
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    barrier, go = ctx.Barrier(n_procs + 1), ctx.Barrier(n_procs + 1)
    results = ctx.Queue()
    procs = [ctx.Process(target=_loadgen_main, args=(targets, first + i * concurrency, source, concurrency, warmup,
                                                     steps, barrier, results, go, extra), daemon=True)
             for i in range(n_procs)]
    for p in procs:
        p.start()
    try:
        barrier.wait(timeout=900)
    except Exception:  # a load generator failed during warm-up
        pass
    sync()  # every rank's load generators warmed up (torchrun: a dist barrier)
    try:
        go.wait(timeout=900)
    except Exception:
        pass
    if marks is not None:
        marks["t0"], marks["cpu0"], marks["thr0"] = time.perf_counter(), cpu_usage_s()[0], cpu_throttle()
        marks["roles0"] = cpu_by_role(marks.get("svc"))
        marks["threads0"] = daemon_threads(marks.get("svc"))
        if marks.get("hport"):
            marks["slots0"] = slot_executions(marks["hport"])
    out = [results.get(timeout=3600) for _ in procs]
    sync()
    for p in procs:
        p.join(timeout=30)
    if marks is not None:
        # (after the join: the load generators' CPU is then in our children's)
        marks["roles1"] = cpu_by_role(marks.get("svc"))
        marks["threads1"] = daemon_threads(marks.get("svc"))
        if marks.get("hport"):
            marks["slots1"] = slot_executions(marks["hport"])
    return out


# The gang check's job (BASELINE config 5): an all-reduce over the gang's
# ranks, its bus bandwidth per message size against the xGMI budget, the
# small-message latency, and the RCCL environment the ranks actually run
# with.  On GPUs: "nccl" (RCCL over xGMI); in the virtual-GPU CPU rehearsal:
# "gloo" on CPU tensors (smaller messages), every other step the same.
GANG_SCRIPT_TEMPLATE = """
import json, os, time, torch, torch.distributed as dist
t0 = time.perf_counter()
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
backend = "{backend}"
dev = "cuda" if backend == "nccl" else "cpu"
if dev == "cuda":
    torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
def sync():
    if dev == "cuda":
        torch.cuda.synchronize()
dist.init_process_group(backend)  # the gang's FileStore rendezvous (BEE_GANG_RDZV)
t_init = time.perf_counter()
x = torch.full(({big},), float(rank + 1), device=dev)  # the large message, f32
dist.all_reduce(x); sync()
want = world * (world + 1) / 2
ok = bool((x[:4096] == want).all()) and bool((x[-4096:] == want).all())
s = torch.ones((1024,), device=dev)  # 4 KiB: latency
for _ in range(5):
    dist.all_reduce(s)
sync(); t = time.perf_counter()
for _ in range(50):
    dist.all_reduce(s)
sync(); small_us = (time.perf_counter() - t) / 50 * 1e6
sizes = []
for numel in {sweep}:  # bus bandwidth per message size
    m = x[:numel]
    dist.all_reduce(m); sync()
    iters = max(3, min(20, (64 << 20) // (numel * 4)))
    t = time.perf_counter()
    for _ in range(iters):
        dist.all_reduce(m)
    sync(); dt = (time.perf_counter() - t) / iters
    sizes.append((numel * 4, 2 * (world - 1) / world * numel * 4 / dt / 1e9))
busbw = sizes[-1][1]
if rank == 0:
    env = {{k: v for k, v in sorted(os.environ.items()) if k.startswith(("NCCL_", "RCCL_"))}}
    ver = ".".join(map(str, torch.cuda.nccl.version())) if dev == "cuda" else None
    print(f"allreduce_ok={{ok}} busbw_GBps={{busbw:.1f}} small_us={{small_us:.1f}} init_ms={{(t_init - t0) * 1e3:.0f}}")
    print("gang_sizes=" + json.dumps([[b, float(format(g, ".4g"))] for b, g in sizes]))  # (4 digits: gloo on a busy CPU is < 0.01 GB/s)
    print("gang_env=" + json.dumps({{"backend": backend, "rccl_version": ver, "env": env}}))
dist.destroy_process_group()
"""


def gang_script(virtual: bool) -> str:
    if virtual:  # CPU rehearsal: gloo, up to 16 MB
        return GANG_SCRIPT_TEMPLATE.format(backend="gloo", big=4 << 20, sweep=[1 << 14, 1 << 18, 4 << 20])
    # 64 KiB .. 256 MB: latency-bound, LL128 / simple protocol range, link-bound
    return GANG_SCRIPT_TEMPLATE.format(backend="nccl", big=64 << 20, sweep=[1 << 14, 1 << 18, 1 << 22, 64 << 20])


GANG_SCRIPT = gang_script(False)


def _gang_warm_state(hport, n):
    """(warm-set state of the aligned n-GPU block led by slot 0, warm hits,
    cold starts) from the service's status."""
    import urllib.request

    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{hport}/v1/status", timeout=10) as f:
            e = json.load(f)["slots"][0]["executor"]
        key = ",".join(str(i) for i in range(n))
        return (e.get("gang_warm") or {}).get(key), e.get("gang_warm_hits"), e.get("gang_cold_starts")
    except Exception:  # noqa: BLE001
        return None, None, None


def gang_allreduce_check(target, n, repeats=2, hport=None, virtual=False):
    """BASELINE config 5: an N-GPU torch.distributed (RCCL) job inside one
    gang sandbox, dispatched through the service like any other request --
    ``repeats`` back to back, each timed end to end (the ranks are spawned
    for the request: N forks from the torch zygote + HIP and RCCL init), with
    the 256 MB bus bandwidth against the gang's xGMI budget and the 4 KiB
    all-reduce latency."""
    import grpc

    from bee_code_interpreter_fs_amd.models import proto as pb
    from bee_code_interpreter_fs_amd.parallel import busbw_budget_gbps

    out = {"gpus": n, "budget_GBps": round(busbw_budget_gbps(n), 1), "runs": []}
    # a bounded side check: the headline line must come out even if a gang
    # hangs on a node (RCCL init, a stuck rank) -- one budget for all runs,
    # and the first failing run ends the check
    end = time.monotonic() + float(os.environ.get("BEE_BENCH_GANG_BUDGET_S", "240"))
    try:
        with grpc.insecure_channel(target) as ch:
            stub = pb.CodeInterpreterServiceStub(ch)
            # the service's RCCL policy for gangs (config.gang_rccl_env), then
            # one run with more channels over the 7-link xGMI mesh set in the
            # script itself (RCCL reads the env at communicator init): the
            # node's own measurement of that knob, reported side by side
            script0 = gang_script(virtual)
            variants = [("default", script0)] * repeats + ([] if virtual else [
                ("NCCL_MIN_NCHANNELS=112", "import os\nos.environ['NCCL_MIN_NCHANNELS'] = '112'\n" + script0)])
            for policy, script in variants:
                left = end - time.monotonic()
                if left < 30:
                    out["skipped"] = f"gang check budget spent before {policy}"
                    break
                # the gang's warm rank set (config.gang_warm_sizes): wait for it
                # to be ready, so the run measures the warm path (the state
                # and the wait are reported; a cold start says so)
                state, waited = None, time.perf_counter()
                if hport:
                    deadline = time.monotonic() + min(60, left / 3)
                    while time.monotonic() < deadline:
                        state, _, _ = _gang_warm_state(hport, n)
                        if state in ("ready", None):
                            break
                        time.sleep(0.2)
                _, hits0, cold0 = _gang_warm_state(hport, n) if hport else (None, None, None)
                t = time.perf_counter()
                left = max(end - time.monotonic(), 20.0)
                r = stub.Execute(pb.ExecuteRequest(source_code=script, gpus=n, timeout=min(180.0, left - 10)),
                                 timeout=left)
                run = {"rccl": policy, "exit_code": r.exit_code, "latency_ms": round((time.perf_counter() - t) * 1e3, 1),
                       "warm_set": state, "warm_wait_s": round(t - waited, 2),
                       "acquire_ms": round(r.timings_ms.get("acquire", -1.0), 1),
                       "queue_ms": round(r.timings_ms.get("queue", -1.0), 1)}
                if hport:
                    _, hits1, cold1 = _gang_warm_state(hport, n)
                    if hits0 is not None and hits1 is not None:
                        run["rank_start"] = "warm" if hits1 > hits0 else "cold" if cold1 > cold0 else "?"
                line = [l for l in r.stdout.splitlines() if l.startswith("allreduce_ok")]
                if line:
                    kv = dict(p.split("=", 1) for p in line[0].split())
                    run.update(ok=kv.get("allreduce_ok") == "True", busbw_GBps=float(kv.get("busbw_GBps", "nan")),
                               small_allreduce_us=float(kv.get("small_us", "nan")), init_ms=float(kv.get("init_ms", "nan")))
                    for l in r.stdout.splitlines():
                        if l.startswith("gang_sizes="):
                            run["busbw_by_size"] = [
                                {"bytes": b, "busbw_GBps": g, "of_budget": round(g / out["budget_GBps"], 3)}
                                for b, g in json.loads(l.split("=", 1)[1])]
                        elif l.startswith("gang_env=") and "rccl_env" not in out:
                            out["rccl_env"] = json.loads(l.split("=", 1)[1])
                elif r.exit_code:
                    run["stderr_tail"] = r.stderr[-300:]
                out["runs"].append(run)
                if not run.get("ok"):
                    break  # (a failing gang would fail the same way again: no retries)
    except Exception as e:  # noqa: BLE001
        out["error"] = repr(e)[:300]
    ok = [r for r in out["runs"] if r.get("ok")]
    out["ok"] = bool(ok) and len(ok) == len(out["runs"])
    ok = [r for r in ok if r.get("rccl") == "default"]  # the headline figures: the service's own policy
    if ok:
        out["busbw_GBps"] = max(r["busbw_GBps"] for r in ok)
        out["busbw_of_budget"] = round(out["busbw_GBps"] / out["budget_GBps"], 3)
        out["latency_ms"] = [r["latency_ms"] for r in out["runs"]]
        best = max(ok, key=lambda r: r["busbw_GBps"])
        if best.get("busbw_by_size"):
            out["busbw_by_size"] = best["busbw_by_size"]  # the service policy's best run, per message size
    out["transport"] = "gloo over loopback (virtual-GPU CPU rehearsal)" if virtual else "RCCL over xGMI"
    out["budget_s"] = float(os.environ.get("BEE_BENCH_GANG_BUDGET_S", "240"))
    return out


def executor_stats(hport):
    import urllib.request

    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{hport}/v1/status", timeout=10) as f:
            st = json.load(f)
        keys = ("mean_warm_ms", "mean_worker_warm_ms", "mean_fork_ms", "mean_acquire_ms", "executions")
        out = []
        for s in st["slots"]:
            e = s["executor"]
            d = {"gpu": s.get("gpu")}
            d.update({k: round(e.get(k, 0), 3) for k in keys})
            adm = e.get("admission") or {}
            # the daemon's bound, held for every front-end replica: high-water
            # marks of admitted jobs and committed HBM against the caps
            d["admission"] = {k: adm.get(k) for k in ("max_inflight", "max_jobs_seen", "hbm_capacity", "max_hbm_seen",
                                                      "admitted", "timeouts")}
            n = max(e.get("executions", 0), 1)
            d["daemon_cpu_ms_per_exec"] = {k: round(v / n, 3) for k, v in (e.get("cpu_ms") or {}).items()}
            # whole daemon lifetime (start-up included) by thread role
            d["daemon_thread_cpu_ms_per_exec"] = {k: round(v / n, 3) for k, v in (e.get("thread_cpu_ms") or {}).items()}
            # an executed sandbox's whole CPU (wait4 in its zygote) vs its own
            # last report: the difference is its teardown (exit, kill)
            sb = e.get("sandbox_cpu") or {}
            d["sandbox_cpu"] = {k: round(v, 3) if isinstance(v, float) else v for k, v in sb.items()}
            out.append(d)
        return out
    except Exception as e:  # noqa: BLE001
        return repr(e)[:200]


def admission_checks(target, n_gpus):
    """Requests no GPU of the node can take must fail at once with
    INVALID_ARGUMENT, not queue forever: an hbm_bytes above one GPU's HBM and
    a gang larger than the node."""
    import grpc

    from bee_code_interpreter_fs_amd.models import proto as pb

    out = {}
    with grpc.insecure_channel(target) as ch:
        stub = pb.CodeInterpreterServiceStub(ch)
        for name, req in (("oversized_hbm", pb.ExecuteRequest(source_code="print(1)", hbm_bytes=10**15)),
                          ("too_many_gpus", pb.ExecuteRequest(source_code="print(1)", gpus=n_gpus + 1))):
            t = time.perf_counter()
            try:
                stub.Execute(req, timeout=30)
                code = "OK"
            except grpc.RpcError as e:
                code = e.code().name
            out[name] = {"code": code, "ms": round((time.perf_counter() - t) * 1e3, 1)}
    return out


def wait_pools_ready(hport, timeout_s=240.0):
    """Steady state before timing: every slot's direct (torch) and light
    (pandas) pools at target, all zygotes up.  Their start-up (interpreter
    imports, huge-page collapse, HIP warm-up of direct sandboxes) is one-time
    CPU that would otherwise land inside the timed region."""
    import urllib.request

    deadline = time.monotonic() + timeout_s
    while time.monotonic() < deadline:
        try:
            with urllib.request.urlopen(f"http://127.0.0.1:{hport}/v1/status", timeout=10) as f:
                st = json.load(f)
            ready = True
            for s in st["slots"]:
                e = s["executor"]
                if e.get("zygotes_alive", 0) < e.get("zygotes", 0) or e.get("ready_direct", 0) < e.get("target", 0) or \
                        e.get("ready_light", 0) < e.get("light_target", 0):
                    ready = False
            if ready:
                time.sleep(0.5)
                return True
        except Exception:  # noqa: BLE001
            pass
        time.sleep(0.25)
    return False


def main():
    args = parse_args()
    world, rank, local = dist_env()
    n_gpus = args.gpus if world == 1 else world
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo", init_method="env://", world_size=world, rank=rank)
    has_gpu = torch.cuda.is_available()
    if has_gpu:
        torch.cuda.set_device(local % visible_gpus())

    def barrier():
        if world > 1:
            dist.barrier()
        if has_gpu:
            torch.cuda.synchronize()

    script, metric, model, dtype = WORKLOADS[args.workload]
    source = seeded(open(args.payload or os.path.join(ROOT, script)).read(), args.seed)
    full = args.full
    extra = {"numpy_offload": True} if args.numpy_offload else None
    if args.numpy_offload:
        metric = metric.replace("numpy on CPU", "numpy offloaded to the GPU (numpy_offload)")
    loop = asyncio.new_event_loop()
    proc = None
    tmp = tempfile.mkdtemp(prefix="bee-bench-", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    info = [None, None, None, None]
    chans = []
    try:
        t_start = time.perf_counter()
        if rank == 0:
            proc, gport, hport, frontends, replicas = start_service(tmp, n_gpus, args)
            info = [gport, hport, frontends, replicas]
        ready_s = time.perf_counter() - t_start  # service start -> READY (pools warm, self-warm done)
        if world > 1:
            dist.broadcast_object_list(info, src=0)
        gport, hport, frontends, replicas = info
        target = f"127.0.0.1:{gport}"
        targets = replicas or [target]
        first = rank * args.concurrency
        # offered load: `concurrency` clients per GPU.  A torchrun rank drives
        # its GPU's clients, a single-process N-GPU run all N GPUs'; either
        # in this process, or over load-generator processes of
        # --clients-per-loadgen clients each (every rank the same way, so the
        # per-GPU client setup does not change with N)
        per_lg = args.clients_per_loadgen if 0 < args.clients_per_loadgen < args.concurrency else args.concurrency
        lg_per_gpu = -(-args.concurrency // per_lg)
        loadgens = (n_gpus if world == 1 else 1) * lg_per_gpu
        if loadgens == 1:
            per_lg = args.concurrency

        def gather_ranks(local):  # every rank's load-generator tuples, on every rank
            if world == 1:
                return local
            allg = [None] * world
            dist.all_gather_object(allg, local)
            return [g for part in allg for g in part]

        idle = None
        if rank == 0:
            wait_pools_ready(hport)
            if args.idle_probe > 0 and full:
                idle = idle_profile(proc.pid, args.idle_probe)
            elif args.idle_probe > 0:
                # the same pause without the sampling: it lets the self-warm's
                # sandbox teardown and the pool refill finish before a short
                # timed window (profiles/archive/r4_idle_probe_ab.jsonl), so
                # the headline figure needs it
                time.sleep(args.idle_probe)
        if world > 1:
            dist.barrier()
        cpu0, cpu_src = cpu_usage_s()
        svc_pid = proc.pid if proc is not None else None
        cpu_busy, thr0, thr1 = 0.0, {}, {}
        roles0 = roles1 = slots0 = slots1 = threads0 = threads1 = None
        if loadgens > 1 and not full:
            gathered = gather_ranks(run_loadgens(loadgens, targets, source, per_lg, args.warmup, args.steps, barrier,
                                                 first=first, extra=extra))
        elif loadgens > 1:
            marks = {"roles0": None, "svc": svc_pid, "hport": hport if rank == 0 else None}
            gathered = gather_ranks(run_loadgens(loadgens, targets, source, per_lg, args.warmup, args.steps, barrier,
                                                 marks, first=first, extra=extra))
            elapsed = max(g[0] for g in gathered)
            cpu_busy = (cpu_usage_s()[0] - marks["cpu0"]) / max(time.perf_counter() - marks["t0"], 1e-9)
            thr0, thr1 = marks.get("thr0") or {}, cpu_throttle()
            roles0, roles1 = marks["roles0"], marks.get("roles1")
            slots0, slots1 = marks.get("slots0"), marks.get("slots1")
            threads0, threads1 = marks.get("threads0"), marks.get("threads1")
        else:
            chans, stubs = loop.run_until_complete(open_clients(targets, first, args.concurrency))
            loop.run_until_complete(run_clients(stubs, source, args.warmup, extra=extra))  # warm every pool
            if os.environ.get("BEE_GC_FREEZE", "1") != "0":
                gc.collect()
                gc.freeze()  # the clients' heap out of the timed window's collections
            barrier()
            if full:
                thr0 = cpu_throttle()
                roles0 = cpu_by_role(svc_pid)
                threads0 = daemon_threads(svc_pid)
                slots0 = slot_executions(hport) if rank == 0 else None
            trace = [] if os.environ.get("BEE_BENCH_TRACE") else None
            # the container's CPU counter right around the timed window: the
            # samplers above and below (/proc walks, a status call through the
            # front-end) stay out of CPU per Execute
            cpu0, cpu_src = cpu_usage_s()
            t0 = time.perf_counter()
            lat, errors, exec_times, phases, checks, last = loop.run_until_complete(
                run_clients(stubs, source, args.steps, trace, extra=extra))
            barrier()
            elapsed = time.perf_counter() - t0
            cpu1 = cpu_usage_s()[0]
            if full:
                thr1 = cpu_throttle()
                roles1 = cpu_by_role(svc_pid)
                threads1 = daemon_threads(svc_pid)
                slots1 = slot_executions(hport) if rank == 0 else None
            cpu_busy = (cpu1 - cpu0) / elapsed if elapsed > 0 else 0.0
            gathered = [(elapsed, lat, errors, exec_times, phases, checks, last)]
            if trace is not None:  # completion time (s after t0) and latency of every timed Execute
                with open(os.environ["BEE_BENCH_TRACE"], "w") as fh:
                    json.dump([(round(t - t0, 6), l) for t, l in trace], fh)
            if world > 1:
                gathered = [None] * world
                dist.all_gather_object(gathered, (elapsed, lat, errors, exec_times, phases, checks, last))

        # secondary: the same payload with every draw materialised in HBM
        # (the reference's numpy data movement), same clients, untimed by
        # the headline
        mat = None
        mat_steps = args.materialized_steps if args.materialized_steps >= 0 else min(args.steps, 20)
        if full and args.workload == "numpy_gpu" and mat_steps > 0 and not args.payload:
            msrc = seeded(open(MATERIALIZED).read(), args.seed)
            if loadgens > 1:
                mg = gather_ranks(run_loadgens(loadgens, targets, msrc, per_lg, 1, mat_steps, barrier, first=first))
            else:
                loop.run_until_complete(run_clients(stubs, msrc, 1))
                barrier()
                tm = time.perf_counter()
                r = loop.run_until_complete(run_clients(stubs, msrc, mat_steps))
                barrier()
                mg = [(time.perf_counter() - tm,) + tuple(r)]
                if world > 1:
                    allmg = [None] * world
                    dist.all_gather_object(allmg, mg[0])
                    mg = allmg
            m_el = max(g[0] for g in mg)
            m_lat = [x for g in mg for x in g[1]]
            m_err = [x for g in mg for x in g[2]]
            mat = {"value": round(len(m_lat) / m_el, 3) if m_el > 0 else 0.0, "steps": mat_steps,
                   "p50_latency_ms": round(statistics.median(m_lat), 3) if m_lat else None,
                   "completed": len(m_lat), "errors": len(m_err),
                   "payload": os.path.relpath(MATERIALIZED, ROOT)}
            if m_err:
                mat["first_error"] = m_err[0][:300]

        if rank == 0:
            max_elapsed = max(g[0] for g in gathered)
            all_lat = [x for g in gathered for x in g[1]]
            all_err = [x for g in gathered for x in g[2]]
            all_exec = [x for g in gathered for x in g[3]]
            all_phases = {}
            for g in gathered:
                for k, v in g[4].items():
                    all_phases.setdefault(k, []).extend(v)
            dumped = None
            if args.dump_outputs:
                dumped = dump_outputs(args.dump_outputs, [(i,) + tuple(r) for i, g in enumerate(gathered) for r in g[6]])
            ids = gpu_ids(n_gpus, args)
            # (a gang needs n distinct GPUs: RCCL refuses two ranks on one
            # device, so a folded rehearsal skips it)
            gang = (
                gang_allreduce_check(target, n_gpus, hport=hport, virtual=args.virtual_gpus)
                if full and n_gpus > 1 and not args.no_gang_check and not args.cpu_only and len(set(ids)) >= n_gpus
                else None
            )
            total = len(all_lat)
            clients = per_lg * loadgens * world
            pods = 1 if args.cpu_only else len(ids)
            kind = "CPU-only" if args.cpu_only else "virtual-GPU (CPU rehearsal)" if args.virtual_gpus else "GPU-pinned"
            if not args.cpu_only and not args.virtual_gpus and len(set(ids)) < len(ids):
                kind += f" (folded onto {len(set(ids))} physical GPU(s): one daemon, broker and HIP context per slot)"
            out = {
                "metric": metric,
                "value": round(total / max_elapsed, 3) if max_elapsed > 0 else 0.0,
                "unit": "requests/s",
                "n_gpus": n_gpus,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(max_elapsed * 1e3 / max(args.steps, 1), 3),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": dtype,
                "data": "synthetic (device Philox RNG; random bf16 GEMM operands)"
                if args.workload == "numpy_gpu"
                else "synthetic (the payload generates its own inputs)",
                "config": {
                    "model": model,
                    "global_batch": clients,
                    "seq_len": None,
                    "parallelism": f"{pods} {kind} executor pods, {frontends} front-end replicas, "
                    f"{clients} concurrent clients ({args.concurrency} per GPU, {max(world, loadgens * world)} load-generator processes)"
                    + (f" (round-robin over the {len(replicas)} replica ports)" if replicas else ""),
                    "execution": "every Execute runs in its own single-use sandbox process on the pinned GPU; "
                    "beekern draws are lazy, so sum(square(rand(1e8))) lowers to one fused Philox->square->reduce "
                    "kernel (the unobserved draw never round-trips HBM; set BEE_LAZY_RANDOM=0 to materialise it)",
                },
                "p50_latency_ms": round(statistics.median(all_lat), 3) if all_lat else None,
                "p95_latency_ms": round(percentile(all_lat, 95), 3) if all_lat else None,
                "p50_in_sandbox_exec_ms": round(statistics.median(all_exec), 3) if all_exec else None,
                "p50_phase_ms": {k: round(statistics.median(v), 3) for k, v in sorted(all_phases.items())},
                "completed": total,
                "errors": len(all_err),
            }
            if all_err:
                out["first_error"] = all_err[0][:400]
            out["per_gpu_rps"] = round(out["value"] / max(n_gpus, 1), 3)
            if args.numpy_offload:
                out["numpy_offload"] = True  # the payload is unmodified numpy; its draws and reductions ran on the GPU
            # counted from the responses: every timed Execute's Result within
            # 6 sigma and every row of its GEMM checked (result_ok / gemm_row_ok)
            n_res = sum(g[5].get("result_ok", 0) for g in gathered)
            n_gemm = sum(g[5].get("gemm_ok", 0) for g in gathered)
            out["checked"] = {"result_ok": n_res, "gemm_rows_ok": n_gemm, "of": total}
            out["gemm_verified"] = total > 0 and n_gemm == total
            out["ready_s"] = round(ready_s, 2)
            if dumped is not None:
                out["dumped_outputs"] = {"dir": args.dump_outputs, "files": dumped, "seed": args.seed}
            if full:
                if mat is not None:
                    out["materialized"] = mat
                if gang is not None:
                    out["gang_allreduce"] = gang
                out["executors"] = executor_stats(hport)
                if not args.cpu_only:
                    out["admission_checks"] = admission_checks(target, len(gpu_ids(n_gpus, args)))
                out["cpu_cores_busy"] = {"value": round(cpu_busy, 2), "source": cpu_src}
                if roles0 is not None and roles1 is not None and total:
                    # CPU per Execute by role over the timed region (rank 0's node)
                    per = {k: round((roles1[k] - roles0[k]) * 1e3 / total, 3) for k in roles0}
                    per["all_cgroup"] = round(cpu_busy * max_elapsed * 1e3 / total, 3)
                    per["unattributed"] = round(
                        per["all_cgroup"] - sum(v for k, v in per.items() if k != "all_cgroup"), 3)
                    out["cpu_ms_per_exec"] = per
                    if threads0 and threads1:
                        th = {k: round((threads1.get(k, 0.0) - v) * 1e3 / total, 3) for k, v in threads0.items()}
                        out["daemon_threads_ms_per_exec"] = dict(sorted(((k, v) for k, v in th.items() if v > 0.0005),
                                                                        key=lambda kv: -kv[1]))
                if idle is not None:
                    out["idle_cpu"] = idle
                # what bounds this node: the CPU quota over CPU per Execute is the
                # rate the service could reach with the GPUs idle; a run near it is
                # CPU-bound (more GPUs would not help), one well below it is set by
                # latency / GPU time at the offered concurrency
                quota, quota_src = cpu_quota_cores()
                bound = {"cpu_quota_cores": round(quota, 2), "quota_source": quota_src,
                         "cpu_utilisation_of_quota": round(cpu_busy / quota, 3) if quota else None}
                # quota enforcement during the timed window: periods in which the
                # container ran out of quota stall every process of it until the
                # next period (latency the GPU never sees)
                thr = throttle_delta(thr0, thr1)
                if thr is not None:
                    bound["cpu_throttling"] = thr
                if "cpu_ms_per_exec" in out and out["cpu_ms_per_exec"]["all_cgroup"] > 0:
                    cap = quota * 1e3 / out["cpu_ms_per_exec"]["all_cgroup"]
                    bound["cpu_bound_rps"] = round(cap, 1)
                    # the same without the load generators (they share this box's
                    # quota here; production clients run elsewhere)
                    svc_ms = out["cpu_ms_per_exec"]["all_cgroup"] - out["cpu_ms_per_exec"].get("bench_clients", 0.0)
                    if svc_ms > 0:
                        bound["cpu_bound_rps_service_only"] = round(quota * 1e3 / svc_ms, 1)
                    bound["fraction_of_cpu_bound"] = round(out["value"] / cap, 3)
                    bound["bound_by"] = "cpu" if out["value"] >= 0.85 * cap or cpu_busy >= 0.9 * quota else \
                        "latency/gpu at this concurrency"
                gt = gpu_time_of(slots0, slots1, total, max_elapsed) if rank == 0 else None
                if gt is not None:
                    out["gpu_time"] = gt
                    if gt.get("gpu_bound_rps"):
                        bound["gpu_bound_rps"] = gt["gpu_bound_rps"]
                        bound["gpu_utilisation"] = gt["gpu_utilisation"]
                        if "cpu_bound_rps" in bound and gt["gpu_bound_rps"] < bound["cpu_bound_rps"]:
                            bound["bound_by"] = "gpu" if out["value"] >= 0.85 * gt["gpu_bound_rps"] else bound["bound_by"]
                out["node_bound"] = bound
                # next to the measured value: the rate this node's CPU quota allows
                # at the measured CPU per Execute -- a flat 1 -> N curve explains
                # itself when value sits at it
                out["cpu_bound_rps"] = bound.get("cpu_bound_rps")
                out["gpu_bound_rps"] = bound.get("gpu_bound_rps")
                out["pss_mb"] = pss_by_role(svc_pid)
                if slots0 and slots1 and len(slots0) == len(slots1):
                    per_slot = [b - a for a, b in zip(slots0, slots1)]
                    mean = sum(per_slot) / len(per_slot)
                    out["slot_balance"] = {"executions": per_slot,
                                           "max_dev_from_mean": round(max(abs(x - mean) for x in per_slot) / mean, 3)
                                           if mean else None}
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.barrier()
    finally:
        if chans:
            loop.run_until_complete(close_clients(chans))
        if proc is not None:
            proc.terminate()
            try:
                proc.wait(timeout=60)
            except subprocess.TimeoutExpired:
                proc.kill()
        if world > 1:
            dist.destroy_process_group()
        loop.close()
        # the service's sandbox tree lives in /dev/shm (memory): gone with the run
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

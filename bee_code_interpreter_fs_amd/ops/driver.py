"""Kernel drivers behind ``DeviceArray``.

* :class:`NativeDriver` — this process owns a HIP context; kernels are
  launched directly through ctypes on ``libbeekern.so`` (used by "direct"
  sandboxes that also run torch, by tests and by tools).
* :class:`BrokerDriver` — a "light" sandbox that never initialises HIP; every
  op is a small binary request to the executor daemon's kernel broker
  (csrc/executor/broker.cpp), which owns the GPU context, gives this
  sandbox its own HIP stream and bounds-checked handles, and enforces the
  request's HBM quota.  Saves the 0.1-0.5 s per-sandbox HIP init measured on
  MI355X.

Handles/pointers are plain ints in both cases; ``DeviceArray`` never sees
which driver is active.
"""

from __future__ import annotations

import ctypes
import os
import socket
import struct
import threading
import time
from typing import Optional

from . import _native
from ._lazy import np
from ._native import BeekernError, QuotaExceeded, check

_vp = ctypes.c_void_p


# bk_select takes 1 to MAX_RANKS ranks a call, bk_histogram 1 to MAX_BINS bins
# (BK_MAX_RANKS / BK_MAX_BINS of csrc/kernels/beekern.h and the broker's checks)
MAX_RANKS = 32
MAX_BINS = 4096
_STATS_EDGES_AT = 512
_STATS_COUNTS_AT = _STATS_EDGES_AT + (MAX_BINS + 1) * 8
_STATS_SCRATCH_BYTES = _STATS_COUNTS_AT + MAX_BINS * 8

# bk_sort: at most MAX_SORT_N elements a call (BK_MAX_SORT_N), and the bytes of its scratch
# (bk_sort_workspace_bytes of csrc/kernels/sort.hip; the broker checks its own copy against the library's)
MAX_SORT_N = 0x7FFFFFFF
_SORT_WS_HEADER = 256 + 256 * 4 + 512 * 256 * 4
_SORT_DTYPES = {0: 4, 1: 8, 2: 2, 5: 8}


def sort_workspace_bytes(dt: int, n: int, with_index: bool) -> int:
    """The size of ``sort``'s scratch buffer; 0 for a dtype or n it does not take."""
    if dt not in _SORT_DTYPES or not 0 <= n <= MAX_SORT_N:
        return 0
    r16 = lambda b: (b + 15) & ~15  # noqa: E731
    return _SORT_WS_HEADER + 2 * r16(n * _SORT_DTYPES[dt]) + (2 * r16(n * 4) if with_index else 0)


# the kernels' scratch workspaces: enum BkWorkspace of csrc/kernels/beekern.h
WS_REDUCE, WS_REDUCE_AXIS, WS_AXIS_STAT, WS_COMPRESS, WS_SELECT, WS_HISTOGRAM, WS_COUNT = range(7)

# the distributions of bk_rand_dist: enum BkRandDist of csrc/kernels/beekern.h
(DIST_EXPONENTIAL, DIST_LAPLACE, DIST_LOGISTIC, DIST_GUMBEL, DIST_RAYLEIGH, DIST_WEIBULL, DIST_PARETO, DIST_CAUCHY,
 DIST_LOGNORMAL, DIST_GAMMA, DIST_BETA, DIST_STUDENT_T, DIST_COUNT) = range(13)

# the integer-valued draws of bk_rand_int: enum BkRandInt of csrc/kernels/beekern.h
RINT_INTEGERS, RINT_POISSON, RINT_BINOMIAL, RINT_GEOMETRIC, RINT_COUNT = range(5)


class NativeDriver:
    name = "native"

    def __init__(self) -> None:
        self.lib = _native.lib()
        self.stream = _vp(0)
        self.device: Optional[int] = None
        self.workspaces = [0] * WS_COUNT  # by kind
        self.scalar = 0
        self.stats_scratch = 0

    def init(self, device: int) -> None:
        check(self.lib.bk_init(int(device)), "bk_init")
        self.device = device
        self._workspace(WS_REDUCE)  # (the reductions read workspaces[WS_REDUCE] themselves)
        self.scalar = self.malloc(256)

    def _workspace(self, kind: int) -> int:
        """The workspace of ``kind``, allocated and initialised on first use."""
        ws = self.workspaces[kind]
        if not ws:
            ws = self.malloc(self.lib.bk_workspace_bytes(kind))
            check(self.lib.bk_workspace_init(kind, _vp(ws), self.stream), "bk_workspace_init")
            self.workspaces[kind] = ws
        return ws

    def malloc(self, nbytes: int) -> int:
        out = _vp()
        check(self.lib.bk_malloc(ctypes.byref(out), max(int(nbytes), 1)), "bk_malloc")
        return int(out.value or 0)

    def free(self, h: int) -> None:
        self.lib.bk_free(_vp(h))

    def h2d(self, h: int, host: np.ndarray, offset: int = 0) -> None:
        if host.nbytes:
            check(self.lib.bk_memcpy(_vp(h + offset), host.ctypes.data, host.nbytes, 1, self.stream), "upload")

    def d2h(self, h: int, host: np.ndarray, offset: int = 0) -> None:
        if host.nbytes:
            check(self.lib.bk_memcpy(host.ctypes.data, _vp(h + offset), host.nbytes, 2, self.stream), "download")

    def rand(self, kind: int, h: int, n: int, dt: int, seed: int, off: int, a: float, b: float) -> None:
        fn = self.lib.bk_rand_uniform if kind == 0 else self.lib.bk_rand_normal
        check(fn(_vp(h), n, dt, seed, off, a, b, self.stream), "bk_rand")

    def rand_dist(self, kind: int, h: int, n: int, dt: int, seed: int, off: int, p0: float, p1: float) -> None:
        """n draws of the distribution ``kind`` (a DIST_* code) into h; f32 / f64."""
        check(self.lib.bk_rand_dist(kind, _vp(h), n, dt, seed, off, p0, p1, self.stream), "bk_rand_dist")

    def unary(self, op: int, dt: int, x: int, y: int, n: int) -> None:
        check(self.lib.bk_unary(op, dt, _vp(x), _vp(y), n, self.stream), "bk_unary")

    def binary(self, op: int, dt: int, mode: int, a: int, b: int, sc: float, y: int, n: int) -> None:
        check(self.lib.bk_binary(op, dt, mode, _vp(a), _vp(b) if b else None, sc, _vp(y), n, self.stream), "bk_binary")

    def cast(self, s: int, d: int, x: int, y: int, n: int) -> None:
        check(self.lib.bk_cast(s, d, _vp(x), _vp(y), n, self.stream), "bk_cast")

    def fill(self, y: int, nbytes: int, pattern: int, width: int) -> None:
        check(self.lib.bk_fill(_vp(y), nbytes, pattern, width, self.stream), "bk_fill")

    def reduce(self, op: int, dt: int, a: int, b: int, n: int) -> float:
        check(self.lib.bk_reduce(op, dt, _vp(a), _vp(b) if b else None, n, _vp(self.workspaces[WS_REDUCE]),
                                 _vp(self.scalar), self.stream), "bk_reduce")
        out = np.zeros(1, np.float64)
        self.d2h(self.scalar, out)
        return float(out[0])

    def rand_reduce(self, op: int, dt: int, n: int, seed: int, off: int, lo: float, hi: float) -> float:
        check(self.lib.bk_rand_reduce(op, dt, n, seed & 0xFFFFFFFFFFFFFFFF, off, lo, hi, _vp(self.workspaces[WS_REDUCE]),
                                      _vp(self.scalar), self.stream), "bk_rand_reduce")
        out = np.zeros(1, np.float64)
        self.d2h(self.scalar, out)
        return float(out[0])

    def gemm(self, A, Bt, C, M, N, K, lda, ldb, ldc, alpha, beta, odt) -> None:
        check(
            self.lib.bk_gemm_bf16_tn(_vp(A), _vp(Bt), _vp(C), M, N, K, lda, ldb, ldc, alpha, beta, odt, self.stream),
            "bk_gemm_bf16_tn",
        )

    def gemm_nn(self, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, odt) -> None:
        """C = A . B with B stored [K][N] (callers check nn_shape_ok first)."""
        check(
            self.lib.bk_gemm_bf16_nn(_vp(A), _vp(B), _vp(C), M, N, K, lda, ldb, ldc, alpha, beta, odt, self.stream),
            "bk_gemm_bf16_nn",
        )

    def gemm_fp(self, dt, ta, tb, A, B, C, M, N, K, lda, ldb, ldc) -> None:
        """C = op(A) . op(B) in f64 (dt 1) / f32 (dt 0); ta: A given as [K][M],
        tb: B given as [N][K] (csrc/kernels/gemm_fp.hip)."""
        check(self.lib.bk_gemm_fp(dt, int(ta), int(tb), _vp(A), _vp(B), _vp(C), M, N, K, lda, ldb, ldc, self.stream),
              "bk_gemm_fp")

    def gemm_f32x6(self, ta, tb, A, B, C, M, N, K, lda, ldb, ldc, W, ws_bytes) -> None:
        """The same f32 product on the bf16 MFMA through the six-piece split
        (csrc/kernels/gemm_fp.hip bk_gemm_f32x6); W: ws_bytes of workspace."""
        check(self.lib.bk_gemm_f32x6(int(ta), int(tb), _vp(A), _vp(B), _vp(C), M, N, K, lda, ldb, ldc, _vp(W), ws_bytes,
                                     self.stream), "bk_gemm_f32x6")

    def reduce_axis(self, op: int, dt: int, x: int, y: int, rows: int, cols: int, ld: int, axis: int) -> None:
        check(self.lib.bk_reduce_axis(op, dt, _vp(x), rows, cols, ld, axis, _vp(y), _vp(self._workspace(WS_REDUCE_AXIS)),
                                      self.stream), "bk_reduce_axis")

    # ---- a matrix against a vector, per-axis statistics (csrc/kernels/axis.hip) -------
    def broadcast(self, op: int, dt: int, kind: int, swapped: bool, a: int, v: int, y: int, rows: int, cols: int,
                  lda: int, ldy: int) -> None:
        """y[r, c] = a[r, c] OP v[c] (kind 0) or a[r, c] OP v[r] (kind 1); swapped: v OP a.
        op: the codes of ``binary``; f32 / f64; y may be a itself."""
        check(self.lib.bk_broadcast(op, dt, kind, int(bool(swapped)), _vp(a), rows, cols, lda, _vp(v), _vp(y), ldy,
                                    self.stream), "bk_broadcast")

    def axis_stat(self, op: int, dt: int, x: int, y: int, rows: int, cols: int, ld: int, axis: int,
                  divisor: float) -> None:
        """y = max (op 0) / min (1) / var (2) / std (3) of x[rows, cols] along ``axis``, in x's
        dtype (f32 / f64); divisor: the variance's n - ddof."""
        check(self.lib.bk_axis_stat(op, dt, _vp(x), rows, cols, ld, axis, float(divisor), _vp(y),
                                    _vp(self._workspace(WS_AXIS_STAT)), self.stream), "bk_axis_stat")

    # ---- boolean masks (csrc/kernels/mask.hip): one byte per element ----------------
    def compare(self, op: int, dt: int, mode: int, a: int, b: int, sc: float, y: int, n: int) -> None:
        """y[i] = a[i] OP (b[i] | sc) as 0 / 1 bytes; op 0 < 1 <= 2 > 3 >= 4 == 5 !=; mode 0 array, 1 scalar."""
        check(self.lib.bk_compare(op, dt, mode, _vp(a), _vp(b) if b else None, sc, _vp(y), n, self.stream), "bk_compare")

    def compare_count(self, op: int, dt: int, mode: int, a: int, b: int, sc: float, n: int) -> float:
        """The number of true comparisons, no mask written (one fused launch)."""
        check(self.lib.bk_compare_count(op, dt, mode, _vp(a), _vp(b) if b else None, sc, n, _vp(self.workspaces[WS_REDUCE]),
                                        _vp(self.scalar), self.stream), "bk_compare_count")
        out = np.zeros(1, np.float64)
        self.d2h(self.scalar, out)
        return float(out[0])

    def mask_logical(self, op: int, a: int, b: int, y: int, n: int) -> None:
        """op 0 and, 1 or, 2 xor, 3 not (b unused)."""
        check(self.lib.bk_mask_logical(op, _vp(a), _vp(b) if b else None, _vp(y), n, self.stream), "bk_mask_logical")

    def where(self, dt: int, mask: int, flags: int, a: int, b: int, sa: float, sb: float, y: int, n: int) -> None:
        """y[i] = mask[i] ? A : B; flags bit 0: A is the scalar sa, bit 1: B is the scalar sb."""
        check(self.lib.bk_where(dt, _vp(mask), flags, _vp(a) if a else None, _vp(b) if b else None, sa, sb, _vp(y), n,
                                self.stream), "bk_where")

    def compress(self, dt: int, x: int, mask: int, n: int, y: int, cap: int) -> None:
        """y[0:cap] = x[mask] in index order (writes past cap are dropped)."""
        check(self.lib.bk_compress(dt, _vp(x), _vp(mask), n, _vp(y), cap, _vp(self._workspace(WS_COMPRESS)), self.stream),
              "bk_compress")

    # ---- int64 arrays (csrc/kernels/integer.hip) ---------------------------------------
    def rand_int(self, kind: int, h: int, n: int, seed: int, off: int, a: int, b: int, p: float) -> None:
        """n int64 draws of ``kind`` (a RINT_* code) into h; a, b, p: the kind's parameters."""
        check(self.lib.bk_rand_int(kind, _vp(h), n, seed, off, int(a), int(b), float(p), self.stream), "bk_rand_int")

    def int_binary(self, op: int, mode: int, a: int, b: int, sc: int, y: int, n: int) -> None:
        """y = a OP (b | sc) on int64; op 0 + 1 - 2 * 3 // 4 % 5 max 6 min; mode as ``binary``; y may be a or b."""
        check(self.lib.bk_int_binary(op, mode, _vp(a), _vp(b) if b else None, int(sc), _vp(y), n, self.stream),
              "bk_int_binary")

    def int_compare(self, op: int, mode: int, a: int, b: int, sc: int, y: int, n: int) -> None:
        """y[i] = a[i] OP (b[i] | sc) as 0 / 1 bytes; the op codes of ``compare``; mode 0 array, 1 scalar."""
        check(self.lib.bk_int_compare(op, mode, _vp(a), _vp(b) if b else None, int(sc), _vp(y), n, self.stream),
              "bk_int_compare")

    def int_reduce(self, op: int, a: int, n: int) -> int:
        """op 0 sum (wrapping), 1 max, 2 min of n int64, as a Python int."""
        check(self.lib.bk_int_reduce(op, _vp(a), n, _vp(self.workspaces[WS_REDUCE]), _vp(self.scalar), self.stream),
              "bk_int_reduce")
        out = np.zeros(1, np.int64)
        self.d2h(self.scalar, out)
        return int(out[0])

    def int_cast(self, s: int, d: int, x: int, y: int, n: int) -> None:
        """int64 -> f64 / f32, f64 / f32 / bool -> int64 (dtype codes)."""
        check(self.lib.bk_int_cast(s, d, _vp(x), _vp(y), n, self.stream), "bk_int_cast")

    # ---- sorting, arg-reductions, gather (csrc/kernels/sort.hip) ------------------------
    def sort(self, dt: int, x: int, n: int, sorted_out: int, index_out: int, ws: int) -> None:
        """sorted_out = np.sort(x) and / or index_out (int64) = np.argsort(x, kind="stable"); 0: not wanted.
        ws: ``sort_workspace_bytes(dt, n, bool(index_out))`` bytes of scratch."""
        check(self.lib.bk_sort(dt, _vp(x), n, _vp(sorted_out) if sorted_out else None,
                               _vp(index_out) if index_out else None, _vp(ws),
                               sort_workspace_bytes(dt, n, bool(index_out)), self.stream), "bk_sort")

    def arg_reduce(self, op: int, dt: int, x: int, n: int) -> int:
        """op 0 np.argmax, 1 np.argmin of the n elements (n >= 1), as a Python int."""
        check(self.lib.bk_arg_reduce(op, dt, _vp(x), n, _vp(self.workspaces[WS_REDUCE]), _vp(self.scalar), self.stream),
              "bk_arg_reduce")
        out = np.zeros(1, np.int64)
        self.d2h(self.scalar, out)
        return int(out[0])

    def take(self, dt: int, x: int, n: int, idx: int, m: int, out: int) -> int:
        """out[i] = x[idx[i]] for m int64 indices in [-n, n); returns the number of indices outside it
        (their elements are zero, nothing is read through them)."""
        check(self.lib.bk_take(dt, _vp(x), n, _vp(idx), m, _vp(out), _vp(self.workspaces[WS_REDUCE]), _vp(self.scalar),
                               self.stream), "bk_take")
        bad = np.zeros(1, np.int64)
        self.d2h(self.scalar, bad)
        return int(bad[0])

    # ---- order statistics and histograms (csrc/kernels/stats.hip) ---------------------
    def _stats_scratch(self) -> int:
        """Device scratch of the two ops: 33 f64 select results, then the
        histogram's edges (MAX_BINS + 1 f64) and counts (MAX_BINS u64)."""
        if not self.stats_scratch:
            self.stats_scratch = self.malloc(_STATS_SCRATCH_BYTES)
        return self.stats_scratch

    def select(self, dt: int, x: int, n: int, ranks) -> tuple:
        """(np.sort(x)[k] as a float for every 0-based k of ``ranks`` (1 to
        32 of them), the number of NaNs in x); x is only read."""
        ranks = [int(k) for k in ranks]
        out = self._stats_scratch()
        karr = (ctypes.c_int64 * max(len(ranks), 1))(*ranks)
        check(self.lib.bk_select(dt, _vp(x), n, karr, len(ranks), _vp(out), _vp(self._workspace(WS_SELECT)), self.stream),
              "bk_select")
        host = np.zeros(len(ranks) + 1, np.float64)
        self.d2h(out, host)
        return [float(v) for v in host[:-1]], int(host[-1])

    def histogram(self, dt: int, x: int, n: int, edges: np.ndarray) -> np.ndarray:
        """int64 counts of np.histogram's bin rule for the ``len(edges) - 1``
        bins between the non-decreasing f64 ``edges`` (at most MAX_BINS bins)."""
        edges = np.ascontiguousarray(edges, np.float64)
        bins = edges.size - 1
        if not 1 <= bins <= MAX_BINS:
            raise BeekernError(f"bk_histogram: 1 to {MAX_BINS} bins, got {bins}")
        base = self._stats_scratch()
        d_edges, d_counts = base + _STATS_EDGES_AT, base + _STATS_COUNTS_AT
        self.h2d(d_edges, edges)
        check(self.lib.bk_histogram(dt, _vp(x), n, _vp(d_edges), bins, _vp(d_counts), _vp(self._workspace(WS_HISTOGRAM)),
                                    self.stream), "bk_histogram")
        counts = np.zeros(bins, np.uint64)
        self.d2h(d_counts, counts)
        return counts.astype(np.int64)

    def transpose(self, src: int, dst: int, rows: int, cols: int, ldi: int, ldo: int, src_dtype: int = 2,
                  dst_dtype: int = 2) -> None:
        check(self.lib.bk_transpose(src_dtype, dst_dtype, _vp(src), _vp(dst), rows, cols, ldi, ldo, self.stream),
              "transpose")

    def copy(self, dst: int, src: int, nbytes: int) -> None:
        check(self.lib.bk_memcpy_async(_vp(dst), _vp(src), nbytes, 3, self.stream), "d2d copy")

    def sync(self) -> None:
        check(self.lib.bk_sync(self.stream), "bk_sync")

    def memory_stats(self) -> dict:
        s = (ctypes.c_int64 * 4)()
        check(self.lib.bk_memory_stats(s), "bk_memory_stats")
        return {"in_use": s[0], "cached": s[1], "peak": s[2], "quota": s[3]}

    def set_quota(self, q: int) -> None:
        check(self.lib.bk_set_quota(int(q)), "bk_set_quota")

    def empty_cache(self) -> None:
        check(self.lib.bk_empty_cache(), "bk_empty_cache")

    def device_info(self) -> dict:
        info = (ctypes.c_int64 * 5)()
        name = ctypes.create_string_buffer(64)
        check(self.lib.bk_device_info(info, name, 64), "bk_device_info")
        return _info_dict(list(info), name.value.decode())

    # device-side timing
    def timer_start(self):
        s, e = _vp(), _vp()
        check(self.lib.bk_event_pair_create(ctypes.byref(s), ctypes.byref(e)), "events")
        check(self.lib.bk_event_record(s, self.stream), "event record")
        return (s, e)

    def timer_stop(self, tok) -> float:
        s, e = tok
        check(self.lib.bk_event_record(e, self.stream), "event record")
        ms = float(self.lib.bk_event_elapsed_ms(s, e))
        self.lib.bk_event_destroy(s)
        self.lib.bk_event_destroy(e)
        return ms


def _info_dict(v, arch: str) -> dict:
    return {
        "arch": arch,
        "compute_units": int(v[0]),
        "total_bytes": int(v[1]),
        "free_bytes": int(v[2]),
        "clock_khz": int(v[3]),
        "lds_bytes_per_cu": int(v[4]),
    }


# ---- broker client --------------------------------------------------------------------

(HELLO, ALLOC, FREE, WRITE, READ, RAND, UNARY, BINARY, CAST, FILL, REDUCE, GEMM, TRANSPOSE, SYNC, MEMSTATS, INFO,
 COPY, RAND_REDUCE, ALLOC_AT, REDUCE_AXIS, GEMM_FP, COMPARE, COMPARE_COUNT, MASK_LOGICAL, WHERE,
 COMPRESS, SELECT, HISTOGRAM, BROADCAST, AXIS_STAT, RAND_DIST, RAND_INT, INT_BINARY, INT_COMPARE, INT_REDUCE,
 INT_CAST, SORT, ARG_REDUCE, TAKE) = range(1, 40)
_HDR = struct.Struct("<IIQ")
_NO_REPLY = 1  # request flag: no response unless a later request collects an error
_RHDR = struct.Struct("<iIQ")
_CHUNK = 64 << 20
# allocations up to this size are fire-and-forget with a client-chosen handle
# (ALLOC_AT): no round trip, the broker's verdict arrives with the next reply
_ASYNC_ALLOC_MAX = 1 << 30


def _charged(nbytes: int) -> int:
    """What the broker charges for an allocation (broker_core.cpp charged_bytes)."""
    if nbytes < (1 << 20):
        return (nbytes + 511) & ~511
    return (nbytes + (2 << 20) - 1) & ~((2 << 20) - 1)


class BrokerDriver:
    name = "broker"

    def __init__(self, path: str) -> None:
        self.path = path
        self.sock: Optional[socket.socket] = None
        self.lock = threading.Lock()
        self.device: Optional[int] = None
        self.quota = 0
        self._arch = ""
        self._next = 1  # client handle ids (the broker's own start at 2**62)
        self._sizes: dict = {}
        self._charged = 0
        # fire-and-forget frames waiting to go out with the next request that
        # wants a reply (or a flush): one send and one broker wake-up per
        # batch instead of per launch
        self._out = bytearray()
        self._out_frames = 0
        self._rbuf = bytearray(4096)

    def init(self, device: int, lazy: bool = False) -> None:
        """Open the broker session (connect); with ``lazy`` the
        session opens on the first request instead, so a sandbox that never
        touches the GPU costs the broker nothing."""
        self.device = device
        if not lazy:
            self._connect()

    def _connect(self) -> None:
        # the C socket type: socket.socket's Python layer cost a pooled
        # sandbox ~40 copy-on-write faults; and no HELLO round trip -- the
        # quota the client pre-checks against is the run's (note_quota /
        # BEE_HBM_QUOTA_BYTES), the broker enforces its own
        import _socket

        s = _socket.socket(_socket.AF_UNIX, _socket.SOCK_STREAM)
        s.connect(self.path)
        self.sock = s
        import atexit

        atexit.register(self.flush)  # queued launches still reach the GPU at exit
        if not self.quota:
            self.quota = int(os.environ.get("BEE_HBM_QUOTA_BYTES", "0") or 0)

    def hello(self) -> dict:
        """The broker's view of this session: {quota, arch}."""
        payload = self._call(HELLO, b"")
        (quota,) = struct.unpack_from("<q", payload, 0)
        (n,) = struct.unpack_from("<I", payload, 8)
        self._arch = payload[12 : 12 + n].decode()
        return {"quota": quota, "arch": self._arch}

    @property
    def arch(self) -> str:
        if not self._arch:
            self.hello()
        return self._arch

    def _recv_into(self, view: memoryview) -> None:
        got = 0
        while got < len(view):
            k = self.sock.recv_into(view[got:])
            if k == 0:
                raise BeekernError("kernel broker closed the connection")
            got += k

    def _call(self, op: int, payload: bytes, out: Optional[memoryview] = None) -> bytes:
        if self.sock is None:
            self._connect()
        hdr = _HDR.pack(op, 0, len(payload))
        with self.lock:
            if self._out:
                # queued launches go first, in the same send
                self._out += hdr
                self._out += payload
                frame, self._out, self._out_frames = self._out, bytearray(), 0
                self.sock.sendall(frame)
            elif len(payload) < (1 << 16):
                self.sock.sendall(hdr + payload)
            else:
                self.sock.sendall(hdr)
                self.sock.sendall(payload)
            # the broker sends header and body in one message: one recv
            # usually takes both
            view = memoryview(self._rbuf)
            got = 0
            while got < _RHDR.size:
                k = self.sock.recv_into(view[got:])
                if k == 0:
                    raise BeekernError("kernel broker closed the connection")
                got += k
            status, _, n = _RHDR.unpack_from(self._rbuf, 0)
            have = got - _RHDR.size
            if have > n:
                raise BeekernError("kernel broker: protocol error (reply longer than announced)")
            if status == 0 and out is not None and n == len(out):
                out[:have] = view[_RHDR.size : got]
                if n > have:
                    self._recv_into(out[have:])
                return b""
            body = bytearray(n)
            body[:have] = view[_RHDR.size : got]
            if n > have:
                self._recv_into(memoryview(body)[have:])
        if status != 0:
            msg = {1: "bad argument", 2: "launch failed", 3: "out of device memory", 4: "HBM quota exceeded",
                   5: "not initialised", 6: "bad handle / out of bounds", 7: "protocol error"}.get(status, str(status))
            detail = bytes(body).decode(errors="replace")
            text = f"kernel broker: {msg}" + (f" ({detail})" if detail else "")
            if status == 4:
                raise QuotaExceeded(text)
            if status == 3:
                raise MemoryError(text)
            raise BeekernError(text)
        return bytes(body)

    def _post(self, op: int, payload: bytes) -> None:
        """Fire-and-forget request (kernel launches, frees): no reply; a
        failure is raised by the next request that waits for one (sync,
        reduce, read, alloc) -- the asynchronous-error model of GPU streams.
        Frames are queued and leave with that next request (or once the
        queue holds 64 frames / 64 KB, on flush(), or at exit)."""
        if self.sock is None:
            self._connect()
        with self.lock:
            self._out += _HDR.pack(op, _NO_REPLY, len(payload))
            self._out += payload
            self._out_frames += 1
            if self._out_frames >= 64 or len(self._out) >= (64 << 10):
                self._flush_locked()

    def _flush_locked(self) -> None:
        if self._out:
            frame, self._out, self._out_frames = self._out, bytearray(), 0
            self.sock.sendall(frame)

    def flush(self) -> None:
        """Send queued launches now (without waiting for them)."""
        if self.sock is None:
            return
        with self.lock:
            try:
                self._flush_locked()
            except OSError:
                pass

    def malloc(self, nbytes: int) -> int:
        nbytes = max(int(nbytes), 1)
        cost = _charged(nbytes)
        if self.quota > 0 and self._charged + cost > self.quota:
            # the broker would refuse it too (it stays the authority: other
            # connections of this sandbox count against the same quota)
            raise QuotaExceeded(f"kernel broker: HBM quota exceeded ({self._charged + cost} > {self.quota} bytes)")
        if nbytes <= _ASYNC_ALLOC_MAX:
            with self.lock:
                h = self._next
                self._next += 1
            self._post(ALLOC_AT, struct.pack("<QQ", h, nbytes))
        else:
            h = struct.unpack("<Q", self._call(ALLOC, struct.pack("<Q", nbytes)))[0]
        self._sizes[h] = cost
        self._charged += cost
        return h

    def free(self, h: int) -> None:
        self._charged -= self._sizes.pop(h, 0)
        try:
            self._post(FREE, struct.pack("<Q", h))
        except OSError:
            pass

    def h2d(self, h: int, host: np.ndarray, offset: int = 0) -> None:
        raw = memoryview(np.ascontiguousarray(host)).cast("B")
        for i in range(0, len(raw), _CHUNK):
            piece = raw[i : i + _CHUNK]
            self._call(WRITE, struct.pack("<QQ", h, offset + i) + piece.tobytes())

    def d2h(self, h: int, host: np.ndarray, offset: int = 0) -> None:
        raw = memoryview(host).cast("B")
        for i in range(0, len(raw), _CHUNK):
            piece = raw[i : i + _CHUNK]
            self._call(READ, struct.pack("<QQQ", h, offset + i, len(piece)), out=piece)

    def rand(self, kind, h, n, dt, seed, off, a, b) -> None:
        self._post(RAND, struct.pack("<IIQqQQdd", kind, dt, h, n, seed & 0xFFFFFFFFFFFFFFFF, off, a, b))

    def rand_dist(self, kind, h, n, dt, seed, off, p0, p1) -> None:
        self._post(RAND_DIST, struct.pack("<IIQqQQdd", kind, dt, h, n, seed & 0xFFFFFFFFFFFFFFFF, off, p0, p1))

    def unary(self, op, dt, x, y, n) -> None:
        self._post(UNARY, struct.pack("<IIQQq", op, dt, x, y, n))

    def binary(self, op, dt, mode, a, b, sc, y, n) -> None:
        self._post(BINARY, struct.pack("<IIIIQQdQq", op, dt, mode, 0, a, b or 0, sc, y, n))

    def cast(self, s, d, x, y, n) -> None:
        self._post(CAST, struct.pack("<IIQQq", s, d, x, y, n))

    def fill(self, y, nbytes, pattern, width) -> None:
        self._post(FILL, struct.pack("<QqQII", y, nbytes, pattern, width, 0))

    def reduce(self, op, dt, a, b, n) -> float:
        return struct.unpack("<d", self._call(REDUCE, struct.pack("<IIQQq", op, dt, a, b or 0, n)))[0]

    def rand_reduce(self, op, dt, n, seed, off, lo, hi) -> float:
        payload = struct.pack("<IIqQQdd", op, dt, n, seed & 0xFFFFFFFFFFFFFFFF, off, lo, hi)
        return struct.unpack("<d", self._call(RAND_REDUCE, payload))[0]

    def gemm(self, A, Bt, C, M, N, K, lda, ldb, ldc, alpha, beta, odt) -> None:
        self._post(GEMM, struct.pack("<QQQiiiiiiffii", A, Bt, C, M, N, K, lda, ldb, ldc, alpha, beta, odt, 0))

    def gemm_nn(self, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, odt) -> None:
        # flags bit 0: the second operand is B[K][N] (broker_core.cpp kGemmNN)
        self._post(GEMM, struct.pack("<QQQiiiiiiffii", A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, odt, 1))

    def gemm_fp(self, dt, ta, tb, A, B, C, M, N, K, lda, ldb, ldc) -> None:
        flags = (1 if ta else 0) | (2 if tb else 0)
        self._post(GEMM_FP, struct.pack("<IIQQQiiiiqqq", dt, flags, A, B, C, M, N, K, 0, lda, ldb, ldc))

    def gemm_f32x6(self, ta, tb, A, B, C, M, N, K, lda, ldb, ldc, W, ws_bytes) -> None:
        # flags bit 2: the split product; the workspace handle trails (broker_core.hpp kGemmFpSplit)
        flags = (1 if ta else 0) | (2 if tb else 0) | 4
        self._post(GEMM_FP, struct.pack("<IIQQQiiiiqqqQ", 0, flags, A, B, C, M, N, K, 0, lda, ldb, ldc, W))

    def reduce_axis(self, op, dt, x, y, rows, cols, ld, axis) -> None:
        self._post(REDUCE_AXIS, struct.pack("<IIQQqqqII", op, dt, x, y, rows, cols, ld, axis, 0))

    # a matrix against a vector, per-axis statistics: payload layouts in broker_core.hpp
    def broadcast(self, op, dt, kind, swapped, a, v, y, rows, cols, lda, ldy) -> None:
        self._post(BROADCAST, struct.pack("<IIIIQQQqqqq", op, dt, kind, 1 if swapped else 0, a, v, y, rows, cols, lda,
                                          ldy))

    def axis_stat(self, op, dt, x, y, rows, cols, ld, axis, divisor) -> None:
        self._post(AXIS_STAT, struct.pack("<IIQQqqqIId", op, dt, x, y, rows, cols, ld, axis, 0, float(divisor)))

    # boolean masks: payload layouts beside the op enum in csrc/executor/broker_core.hpp
    def compare(self, op, dt, mode, a, b, sc, y, n) -> None:
        self._post(COMPARE, struct.pack("<IIIIQQdQq", op, dt, mode, 0, a, b or 0, sc, y, n))

    def compare_count(self, op, dt, mode, a, b, sc, n) -> float:
        payload = struct.pack("<IIIIQQdq", op, dt, mode, 0, a, b or 0, sc, n)
        return struct.unpack("<d", self._call(COMPARE_COUNT, payload))[0]

    def mask_logical(self, op, a, b, y, n) -> None:
        self._post(MASK_LOGICAL, struct.pack("<IIQQQq", op, 0, a, b or 0, y, n))

    def where(self, dt, mask, flags, a, b, sa, sb, y, n) -> None:
        self._post(WHERE, struct.pack("<IIQQQddQq", dt, flags, mask, a or 0, b or 0, sa, sb, y, n))

    def compress(self, dt, x, mask, n, y, cap) -> None:
        self._post(COMPRESS, struct.pack("<IIQQqQq", dt, 0, x, mask, n, y, cap))

    # int64 arrays: payload layouts beside the op enum in csrc/executor/broker_core.hpp
    def rand_int(self, kind, h, n, seed, off, a, b, p) -> None:
        self._post(RAND_INT, struct.pack("<IIQqQQqqd", kind, 0, h, n, seed & 0xFFFFFFFFFFFFFFFF, off, int(a), int(b),
                                         float(p)))

    def int_binary(self, op, mode, a, b, sc, y, n) -> None:
        self._post(INT_BINARY, struct.pack("<IIQQqQq", op, mode, a, b or 0, int(sc), y, n))

    def int_compare(self, op, mode, a, b, sc, y, n) -> None:
        self._post(INT_COMPARE, struct.pack("<IIQQqQq", op, mode, a, b or 0, int(sc), y, n))

    def int_reduce(self, op, a, n) -> int:
        return struct.unpack("<q", self._call(INT_REDUCE, struct.pack("<IIQq", op, 0, a, n)))[0]

    def int_cast(self, s, d, x, y, n) -> None:
        self._post(INT_CAST, struct.pack("<IIQQq", s, d, x, y, n))

    # sorting, arg-reductions, gather: payload layouts beside the op enum in csrc/executor/broker_core.hpp
    def sort(self, dt, x, n, sorted_out, index_out, ws) -> None:
        flags = (1 if sorted_out else 0) | (2 if index_out else 0)
        self._post(SORT, struct.pack("<IIQqQQQ", dt, flags, x, n, sorted_out or 0, index_out or 0, ws))

    def arg_reduce(self, op, dt, x, n) -> int:
        return struct.unpack("<q", self._call(ARG_REDUCE, struct.pack("<IIQq", op, dt, x, n)))[0]

    def take(self, dt, x, n, idx, m, out) -> int:
        return struct.unpack("<q", self._call(TAKE, struct.pack("<IIQqQqQ", dt, 0, x, n, idx, m, out)))[0]

    # order statistics and histograms: both reply, like REDUCE
    def select(self, dt, x, n, ranks) -> tuple:
        ranks = [int(k) for k in ranks]
        payload = struct.pack(f"<IIQq{len(ranks)}q", dt, len(ranks), x, n, *ranks)
        v = struct.unpack(f"<{len(ranks) + 1}d", self._call(SELECT, payload))
        return list(v[:-1]), int(v[-1])

    def histogram(self, dt, x, n, edges) -> np.ndarray:
        edges = np.ascontiguousarray(edges, np.float64)
        bins = edges.size - 1
        body = self._call(HISTOGRAM, struct.pack("<IIQq", dt, max(bins, 0), x, n) + edges.tobytes())
        return np.frombuffer(body, np.uint64).astype(np.int64)

    def transpose(self, src, dst, rows, cols, ldi, ldo, src_dtype=2, dst_dtype=2) -> None:
        self._post(TRANSPOSE, struct.pack("<QQiiiiii", src, dst, rows, cols, ldi, ldo, src_dtype, dst_dtype))

    def copy(self, dst, src, nbytes) -> None:
        self._post(COPY, struct.pack("<QQQQQ", dst, 0, src, 0, nbytes))

    def sync(self) -> None:
        self._call(SYNC, b"")

    def memory_stats(self) -> dict:
        v = struct.unpack("<4q", self._call(MEMSTATS, b""))
        return {"in_use": v[0], "cached": v[1], "peak": v[2], "quota": v[3]}

    def set_quota(self, q: int) -> None:
        raise BeekernError("the HBM quota of a light sandbox is set by the executor, not by user code")

    def note_quota(self, q: int) -> None:
        """The executor's quota for the run this sandbox was handed (used for
        early client-side refusals only; the broker enforces it)."""
        self.quota = int(q)

    def empty_cache(self) -> None:
        return None

    def device_info(self) -> dict:
        body = self._call(INFO, b"")
        return _info_dict(struct.unpack_from("<5q", body, 0), body[40:].decode())

    def timer_start(self):
        self.sync()
        return time.perf_counter()

    def timer_stop(self, tok) -> float:
        self.sync()
        return (time.perf_counter() - tok) * 1e3


def nn_shape_ok(M: int, N: int, K: int, lda: int, ldb: int, ldc: int, out_bf16: bool) -> bool:
    """Shapes the [K][N]-B GEMM kernel takes (gemm256w4_impl.hpp nn_ok), and
    large enough to fill the chip with 256^2 tiles (smaller ones go to the
    128^2 kernel after a transpose).  Pointers must be 16-B aligned too."""
    span = lambda ld: 256 * ld * 2 + K * 2 < 0x7FFFFFFF  # noqa: E731
    return (M > 0 and N > 0 and K > 0 and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and lda % 8 == 0
            and ldb % 8 == 0 and ldb >= N and ldc % (8 if out_bf16 else 4) == 0 and span(lda)
            and K * ldb * 2 < 0x7FFFFFFF and (M // 256) * (N // 256) >= 128)


def make_driver():
    sock = os.environ.get("BEE_BROKER_SOCK")
    if sock and os.environ.get("BEE_BEEKERN_DIRECT") != "1":
        return BrokerDriver(sock)
    return NativeDriver()

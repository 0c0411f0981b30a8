"""The numpy model of the kernel driver (tests/host_driver_stats.py) with the
two ops of ``csrc/kernels/axis.hip``: ``broadcast`` (a matrix against a vector
along one axis, numpy's own arithmetic in the dtype) and ``axis_stat`` (max /
min / var / std along an axis: f64 arithmetic, the variance in two passes
about an f64 mean, rounded once).  Every call is recorded in ``launches``.
"""

from __future__ import annotations

import numpy as np

from .host_driver import _NP, HostDriver
from .host_driver_stats import StatsHostDriver

MAX_AXIS0_COLUMNS = 1 << 18


class AxisHostDriver(StatsHostDriver):
    def _matrix(self, p, rows, cols, ld, dt):
        """The (rows, cols) view of a row-major matrix of row stride ld."""
        span = (rows - 1) * ld + cols
        flat = self._view(p, span, dt)
        return np.lib.stride_tricks.as_strided(flat, (rows, cols), (ld * flat.itemsize, flat.itemsize))

    def broadcast(self, op, dt, kind, swapped, a, v, y, rows, cols, lda, ldy) -> None:
        self.launches.append(("broadcast", op, kind, bool(swapped), rows, cols))
        assert dt in (0, 1) and kind in (0, 1) and 0 <= op <= 6 and lda >= cols and ldy >= cols
        m = self._matrix(a, rows, cols, lda, dt)
        vec = self._view(v, cols if kind == 0 else rows, dt)
        out = self._matrix(y, rows, cols, ldy, dt)
        assert not np.shares_memory(out, vec), "y overlaps v"
        w = vec[None, :] if kind == 0 else vec[:, None]
        fn = HostDriver._BINARY[op]
        with np.errstate(all="ignore"):
            out[...] = fn(w, m) if swapped else fn(m, w)

    def axis_stat(self, op, dt, x, y, rows, cols, ld, axis, divisor) -> None:
        self.launches.append(("axis_stat", op, axis, rows, cols, float(divisor)))
        assert dt in (0, 1) and axis in (0, 1) and 0 <= op <= 3 and rows > 0 and cols > 0 and ld >= cols
        assert axis == 1 or cols <= MAX_AXIS0_COLUMNS
        m = self._matrix(x, rows, cols, ld, dt).astype(np.float64)
        with np.errstate(all="ignore"):
            if op == 0:
                r = m.max(axis=axis)
            elif op == 1:
                r = m.min(axis=axis)
            else:
                assert np.isfinite(divisor) and divisor > 0
                mean = m.sum(axis=axis, keepdims=True) / m.shape[axis]
                r = np.square(m - mean).sum(axis=axis) / divisor
                if op == 3:
                    r = np.sqrt(r)
        self._view(y, r.size, dt)[...] = r.astype(_NP[dt])


def use_axis_host_driver(monkeypatch) -> AxisHostDriver:
    """Point beekern at a fresh AxisHostDriver for one test."""
    import sys

    A = sys.modules["bee_code_interpreter_fs_amd.ops.array"]  # (the package exports a function named `array`)
    drv = AxisHostDriver()
    monkeypatch.setattr(A, "_driver", drv)
    return drv

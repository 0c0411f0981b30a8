"""The numpy model of the kernel driver (tests/host_driver_masks.py) with the
two ops of ``csrc/kernels/stats.hip``: ``select`` (np.sort, NaNs last, and the
NaN count) and ``histogram`` (the last edge <= v by searchsorted, the last bin
closed on the right).  Every call is recorded in ``launches``.
"""

from __future__ import annotations

import numpy as np

from .host_driver_masks import MaskHostDriver

MAX_RANKS = 32
MAX_BINS = 4096


class StatsHostDriver(MaskHostDriver):
    def select(self, dt, x, n, ranks):
        ranks = [int(k) for k in ranks]
        self.launches.append(("select", n, tuple(ranks)))
        assert dt in (0, 1, 2) and n >= 1 and 1 <= len(ranks) <= MAX_RANKS
        assert all(0 <= k < n for k in ranks)
        s = np.sort(self._load(x, n, dt))  # f64: the kernel widens every value it returns
        return [float(s[k]) for k in ranks], int(np.isnan(s).sum())

    def histogram(self, dt, x, n, edges):
        edges = np.asarray(edges)
        assert edges.dtype == np.float64 and edges.ndim == 1
        bins = edges.size - 1
        self.launches.append(("histogram", n, bins))
        assert dt in (0, 1, 2) and 1 <= bins <= MAX_BINS
        assert np.isfinite(edges).all() and not np.any(edges[:-1] > edges[1:])
        v = self._load(x, n, dt)
        v = v[(v >= edges[0]) & (v <= edges[-1])]  # (drops NaN)
        idx = np.minimum(np.searchsorted(edges, v, side="right") - 1, bins - 1)
        return np.bincount(idx, minlength=bins).astype(np.int64)


def use_stats_host_driver(monkeypatch) -> StatsHostDriver:
    """Point beekern at a fresh StatsHostDriver for one test."""
    import sys

    A = sys.modules["bee_code_interpreter_fs_amd.ops.array"]  # (the package exports a function named `array`)
    drv = StatsHostDriver()
    monkeypatch.setattr(A, "_driver", drv)
    return drv

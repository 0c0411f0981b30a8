"""The numpy model of the kernel driver (tests/host_driver_int.py) with the
three calls of ``csrc/kernels/sort.hip``: ``sort``, ``arg_reduce`` and ``take``
from their reference (tests/sort_ref.py), the entry points' argument checks as
assertions.  Every call is recorded in ``launches``.
"""

from __future__ import annotations

import numpy as np

from bee_code_interpreter_fs_amd.ops import driver as drvmod

from . import sort_ref
from .host_driver_int import IntHostDriver

_NAME = {code: name for name, code in sort_ref.DTYPES.items()}
_TAKE_SIZE = {0: 4, 1: 8, 2: 2, 5: 8, 6: 1}


class SortHostDriver(IntHostDriver):
    def _elements(self, p: int, n: int, dt: int) -> np.ndarray:
        name = _NAME[dt]
        return self._at(p, n * np.dtype(sort_ref.NP_DTYPES[name]).itemsize).view(sort_ref.NP_DTYPES[name])

    def sort(self, dt, x, n, sorted_out, index_out, ws) -> None:
        self.launches.append(("sort", dt, n, bool(sorted_out), bool(index_out)))
        assert dt in _NAME and 0 <= n <= drvmod.MAX_SORT_N and (sorted_out or index_out)
        if n == 0:
            return
        need = drvmod.sort_workspace_bytes(dt, n, bool(index_out))
        assert x and ws and need > 0
        self._at(ws, need)  # (the scratch is large enough)
        assert len({x, sorted_out or -1, index_out or -2, ws}) == 4, "x, the outputs and the scratch are different buffers"
        a = self._elements(x, n, dt).copy()
        order = sort_ref.argsort(a, _NAME[dt])
        if sorted_out:
            self._elements(sorted_out, n, dt)[...] = a[order]
        if index_out:
            self._at(index_out, n * 8).view(np.int64)[...] = order

    def arg_reduce(self, op, dt, x, n) -> int:
        self.launches.append(("arg_reduce", op, dt, n))
        assert op in (0, 1) and dt in _NAME and n >= 1 and x
        return (sort_ref.argmax if op == 0 else sort_ref.argmin)(self._elements(x, n, dt), _NAME[dt])

    def take(self, dt, x, n, idx, m, out) -> int:
        self.launches.append(("take", dt, n, m))
        assert dt in _TAKE_SIZE and n >= 0 and m >= 0 and x and idx and out
        size = _TAKE_SIZE[dt]
        src = self._at(x, n * size).reshape(n, size)
        got, bad = sort_ref.take(np.arange(n), self._at(idx, m * 8).view(np.int64))
        ok = np.ones(m, bool)
        if bad:
            i = self._at(idx, m * 8).view(np.int64)
            ok = (i >= -n) & (i < n)
        dst = self._at(out, m * size).reshape(m, size)
        dst[...] = 0
        dst[ok] = src[got[ok]]
        return bad


def use_sort_host_driver(monkeypatch) -> SortHostDriver:
    """Point beekern at a fresh SortHostDriver for one test."""
    import sys

    A = sys.modules["bee_code_interpreter_fs_amd.ops.array"]  # (the package exports a function named `array`)
    drv = SortHostDriver()
    monkeypatch.setattr(A, "_driver", drv)
    return drv

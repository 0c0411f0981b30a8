"""The numpy model of the kernel driver (tests/host_driver_dist.py) with the
int64 ops of ``csrc/kernels/integer.hip``: ``rand_int``, ``int_binary``,
``int_compare``, ``int_reduce`` and ``int_cast`` from their reference model
(tests/int_ref.py), the entry points' argument checks as assertions.  Every
call is recorded in ``launches``.
"""

from __future__ import annotations

import numpy as np

from . import int_ref
from .host_driver_dist import DistHostDriver

_CAST_NP = {int_ref.F32: np.float32, int_ref.F64: np.float64, int_ref.I64: np.int64, int_ref.BOOL: np.uint8}


class IntHostDriver(DistHostDriver):
    def _i64(self, p: int, n: int) -> np.ndarray:
        return self._at(p, n * 8).view(np.int64)

    def rand_int(self, kind, h, n, seed, off, a, b, p) -> None:
        self.launches.append(("rand_int", kind, n, int(a), int(b), float(p)))
        assert 0 <= kind < int_ref.COUNT and n >= 0 and 0 <= seed < 1 << 64 and off >= 0
        assert int_ref.params_ok(kind, int(a), int(b), float(p)), (kind, a, b, p)
        self._i64(h, n)[...] = int_ref.draw(kind, n, seed, off, int(a), int(b), float(p))

    def int_binary(self, op, mode, a, b, sc, y, n) -> None:
        self.launches.append(("int_binary", op, mode, n))
        assert 0 <= op < int_ref.BINARY_COUNT and mode in (0, 1, 2) and n >= 0
        assert int_ref.I64_MIN <= int(sc) <= int_ref.I64_MAX and (mode != 0 or b)
        x = self._i64(a, n).copy()
        w = self._i64(b, n).copy() if mode == 0 else np.int64(sc)
        self._i64(y, n)[...] = int_ref.binary(op, w, x) if mode == 2 else int_ref.binary(op, x, w)

    def int_compare(self, op, mode, a, b, sc, y, n) -> None:
        self.launches.append(("int_compare", op, mode, n))
        assert 0 <= op < 6 and mode in (0, 1) and n >= 0
        assert int_ref.I64_MIN <= int(sc) <= int_ref.I64_MAX and (mode != 0 or b)
        w = self._i64(b, n) if mode == 0 else np.int64(sc)
        self._at(y, n)[...] = int_ref.compare(op, self._i64(a, n), w).astype(np.uint8)

    def int_reduce(self, op, a, n) -> int:
        self.launches.append(("int_reduce", op, n))
        assert op in (0, 1, 2) and n >= 0
        return int_ref.reduce(op, self._i64(a, n))

    def int_cast(self, s, d, x, y, n) -> None:
        self.launches.append(("int_cast", s, d, n))
        assert (s, d) in int_ref.CAST_PAIRS and n >= 0
        src = self._at(x, n * np.dtype(_CAST_NP[s]).itemsize).view(_CAST_NP[s])
        self._at(y, n * np.dtype(_CAST_NP[d]).itemsize).view(_CAST_NP[d])[...] = int_ref.cast(s, d, src)


def use_int_host_driver(monkeypatch) -> IntHostDriver:
    """Point beekern at a fresh IntHostDriver for one test."""
    import sys

    A = sys.modules["bee_code_interpreter_fs_amd.ops.array"]  # (the package exports a function named `array`)
    drv = IntHostDriver()
    monkeypatch.setattr(A, "_driver", drv)
    return drv

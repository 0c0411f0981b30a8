"""The numpy model of the kernel driver (tests/host_driver.py) with the mask
ops of ``csrc/kernels/mask.hip``: compare, compare_count, mask_logical, where,
compress, ``reduce`` on a bool mask (count / any / all) and the bool -> float
casts.  Masks are one byte per element; the models write 0 / 1 and read any
non-zero byte as true, as the kernels do.
"""

from __future__ import annotations

import numpy as np

from .host_driver import _NP, _SIZE, HostDriver, _bf16_bits

_CMP = [np.less, np.less_equal, np.greater, np.greater_equal, np.equal, np.not_equal]
_BOOL = 6


class MaskHostDriver(HostDriver):
    def _mask(self, p: int, n: int) -> np.ndarray:
        return self._at(p, n)  # uint8 view

    def _cmp(self, op, dt, mode, a, b, sc, n) -> np.ndarray:
        x = self._load(a, n, dt)  # f64: the kernel widens every element
        other = self._load(b, n, dt) if mode == 0 else np.float64(sc)
        assert mode in (0, 1)
        with np.errstate(all="ignore"):
            return _CMP[op](x, other)

    def fill(self, y, nbytes, pattern, width) -> None:
        if width == 1:
            self._at(y, nbytes)[...] = pattern & 0xFF
        else:
            super().fill(y, nbytes, pattern, width)

    def compare(self, op, dt, mode, a, b, sc, y, n) -> None:
        self.launches.append(("compare", op, n))
        self._mask(y, n)[...] = self._cmp(op, dt, mode, a, b, sc, n).astype(np.uint8)

    def compare_count(self, op, dt, mode, a, b, sc, n) -> float:
        self.launches.append(("compare_count", op, n))
        return float(np.count_nonzero(self._cmp(op, dt, mode, a, b, sc, n)))

    def mask_logical(self, op, a, b, y, n) -> None:
        self.launches.append(("mask_logical", op, n))
        x = self._mask(a, n) != 0
        if op == 3:
            r = ~x
        else:
            z = self._mask(b, n) != 0
            r = [x & z, x | z, x ^ z][op]
        self._mask(y, n)[...] = r.astype(np.uint8)

    def where(self, dt, mask, flags, a, b, sa, sb, y, n) -> None:
        self.launches.append(("where", flags, n))
        m = self._mask(mask, n) != 0

        def side(is_scalar, ptr, s):
            if not is_scalar:
                return self._view(ptr, n, dt).copy()  # bits
            # the kernel's conversion: f64 as is, f32 RNE, bf16 through f32
            with np.errstate(all="ignore"):
                one = np.array([s], np.float64)
                one = _bf16_bits(one.astype(np.float32)) if dt == 2 else one.astype(_NP[dt])
            return np.repeat(one, n)

        self._view(y, n, dt)[...] = np.where(m, side(flags & 1, a, sa), side(flags & 2, b, sb))

    def compress(self, dt, x, mask, n, y, cap) -> None:
        self.launches.append(("compress", n, cap))
        es = 1 if dt == _BOOL else _SIZE[dt]
        src = self._at(x, n * es).reshape(n, es)
        picked = src[self._mask(mask, n) != 0][:cap]
        self._at(y, picked.shape[0] * es)[...] = picked.ravel()

    def reduce(self, op, dt, a, b, n) -> float:
        if dt != _BOOL:
            return super().reduce(op, dt, a, b, n)
        self.launches.append(("reduce", op, n))
        m = self._mask(a, n) != 0
        assert op in (0, 3, 4), "bk_reduce on a mask: count, any, all"
        return float(np.count_nonzero(m)) if op == 0 else float(m.any()) if op == 3 else float(m.all())

    def cast(self, s, d, x, y, n) -> None:
        if s != _BOOL:
            return super().cast(s, d, x, y, n)
        assert d in (0, 1), "bool casts to f32 / f64"
        self.launches.append(("cast", s, d, n))
        self._view(y, n, d)[...] = (self._mask(x, n) != 0).astype(_NP[d])


def use_mask_host_driver(monkeypatch) -> MaskHostDriver:
    """Point beekern at a fresh MaskHostDriver for one test."""
    import sys

    A = sys.modules["bee_code_interpreter_fs_amd.ops.array"]  # (the package exports a function named `array`)
    drv = MaskHostDriver()
    monkeypatch.setattr(A, "_driver", drv)
    return drv

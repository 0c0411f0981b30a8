"""The numpy model of the kernel driver (tests/host_driver_axis.py) with
``rand_dist``: the continuous distributions of ``csrc/kernels/random.hip``
from their reference model (tests/dist_ref.py), the driver's argument checks
as assertions.  Every call is recorded in ``launches``.
"""

from __future__ import annotations

from . import dist_ref
from .host_driver import _NP
from .host_driver_axis import AxisHostDriver


class DistHostDriver(AxisHostDriver):
    def rand_dist(self, kind, h, n, dt, seed, off, p0, p1) -> None:
        self.launches.append(("rand_dist", kind, n, float(p0), float(p1)))
        assert 0 <= kind < dist_ref.COUNT and dt in (0, 1) and n >= 0 and 0 <= seed < 1 << 64 and off >= 0
        assert dist_ref.params_ok(kind, float(p0), float(p1)), (kind, p0, p1)
        self._view(h, n, dt)[...] = dist_ref.draw(kind, n, _NP[dt], seed, off, float(p0), float(p1))


def use_dist_host_driver(monkeypatch) -> DistHostDriver:
    """Point beekern at a fresh DistHostDriver for one test."""
    import sys

    A = sys.modules["bee_code_interpreter_fs_amd.ops.array"]  # (the package exports a function named `array`)
    drv = DistHostDriver()
    monkeypatch.setattr(A, "_driver", drv)
    return drv

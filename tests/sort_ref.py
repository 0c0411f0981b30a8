"""The reference of the sort family (csrc/kernels/sort.hip) in numpy.

The order is numpy's, written out as an unsigned key so that it does not lean
on np.sort itself: floats numerically with -0.0 == +0.0 a tie and every NaN,
of either sign, tied last; int64 signed; ties keep index order.

* ``keys(a)``: the order-preserving unsigned key of every element;
* ``argsort(a)``: the stable order of the keys (equal to
  ``np.argsort(a, kind="stable")`` -- tests assert both);
* ``argmax(a)`` / ``argmin(a)``: the first extremum, the first NaN if there is one;
* ``take(x, idx)``: (x[idx] with negative indices wrapped and zero bits where an
  index is outside [-n, n), the number of such indices).

bf16 arrays are their uint16 bits (``bf16_bits`` makes them from floats).
"""

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DTYPES = {"f32": 0, "f64": 1, "bf16": 2, "i64": 5}
NP_DTYPES = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16, "i64": np.int64}
_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
_INF = {2: 0x7F80, 4: 0x7F800000, 8: 0x7FF0000000000000}


def bf16_bits(values):
    """float32 values truncated to bf16, as uint16 bits (NaN and inf keep their class)."""
    return (np.asarray(values, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_floats(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def keys(a, name):
    """The unsigned keys of ``a`` (dtype name: f32, f64, bf16, i64) whose order is the sorted order."""
    a = np.ascontiguousarray(a)
    size = a.dtype.itemsize
    U = _UINT[size]
    u = a.view(U)
    sign = U(1 << (8 * size - 1))
    if name == "i64":
        return u ^ sign
    mag = u & ~sign
    u = np.where(mag == 0, U(0), u)  # the two zeros tie
    k = np.where(u & sign != 0, ~u, u | sign)
    return np.where(mag > U(_INF[size]), ~U(0), k)  # every NaN last


def argsort(a, name):
    return np.argsort(keys(a, name), kind="stable").astype(np.int64)


def as_values(a, name):
    """What numpy compares: bf16 bits as floats (exact), everything else as it is."""
    return bf16_floats(a) if name == "bf16" else np.asarray(a)


def sort(a, name):
    """np.sort(a) as values (bf16: as floats)."""
    return as_values(a, name)[argsort(a, name)]


def argmax(a, name):
    k = keys(a, name)
    return int(np.flatnonzero(k == k.max())[0])


def argmin(a, name):
    k = keys(a, name)
    top = ~k.dtype.type(0)
    if name != "i64" and (k == top).any():
        return int(np.flatnonzero(k == top)[0])  # the first NaN
    return int(np.flatnonzero(k == k.min())[0])


def take(x, idx):
    x, idx = np.asarray(x), np.asarray(idx, np.int64)
    n = x.size
    ok = (idx >= -n) & (idx < n)
    out = np.zeros(idx.shape, x.dtype)
    wrapped = np.where(idx < 0, idx + n, idx)
    out[ok] = x[wrapped[ok]]
    return out, int((~ok).sum())

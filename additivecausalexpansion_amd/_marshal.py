"""Conversion and allocation between numpy and the C ABI: what every caller
of the library (native.py, model.py) does to its arguments before a call and
to its outputs after one.  Matrices are column-major (R / Armadillo layout).

A converter returns its argument's own memory when that already conforms
(float64 / int32, contiguous), so the arguments the library writes through
(theta in para_update / train) are never copied on the way in.
"""
from __future__ import annotations

import numpy as np

from ._lib import _I32, _I64P, _U32, AceError


def vec(x):
    """Contiguous float64 vector of anything, raveled (theta, y, a test column)."""
    return np.ascontiguousarray(np.ravel(x), dtype=np.float64)


def scalar(v):
    """float of a scalar, a 0-d or a 1-element array."""
    return float(np.ravel([v])[0])


def cols(a, n):
    """n x k column-major float64 matrix of a matrix with n rows, or of a
    vector of n entries (one column)."""
    return np.asfortranarray(np.asarray(a, dtype=np.float64).reshape(n, -1))


def rows(a, k):
    """m x k column-major float64 matrix of a matrix taken as it is, or of a
    vector read column-major (the basis rows of a grid: k = max(B - 1, 1))."""
    a = np.asarray(a, dtype=np.float64)
    return np.asfortranarray(a.reshape((-1, k), order="F") if a.ndim != 2 else a)


def labels(label, nx):
    """int32 group label of each of the nx test points."""
    lab = np.ascontiguousarray(np.ravel(label), dtype=np.int32)
    if lab.size != nx:
        raise AceError("label must have one entry per test point")
    return lab


def _typed_ptr(ptype, dtype):
    def f(a):
        if a is None:
            return None
        assert a.dtype == dtype and (a.flags.f_contiguous or a.flags.c_contiguous)
        return a.ctypes.data_as(ptype)
    return f


i32ptr = _typed_ptr(_I32, np.int32)   # int32_t* of a contiguous int32 array (or None)
u32ptr = _typed_ptr(_U32, np.uint32)  # uint32_t*
iptr = _typed_ptr(_I64P, np.int64)    # int64_t*


def map_ci_var(*lead):
    """The prediction outputs of leading shape `lead`: map (lead), ci (lead,
    2) and var (lead), column-major, and the result dict that holds them."""
    mp, var = np.empty(lead, order="F"), np.empty(lead, order="F")
    ci = np.empty(lead + (2,), order="F")
    return mp, ci, var, {"map": mp, "ci": ci, "var": var}


def ate_dicts(avg):
    """{"ate", "att", "atu"} of the 12 averages (map, ci0, ci1, var of each):
    scalars and a ci pair from a 12-vector, per-step vectors and a T x 2 ci
    from a 12 x T array (views of avg)."""
    out = {}
    for j, key in enumerate(("ate", "att", "atu")):
        a = avg[4 * j:4 * j + 4]
        out[key] = {"map": a[0], "ci": np.array([a[1], a[2]]) if avg.ndim == 1 else a[1:3].T,
                    "var": a[3]}
    return out


def pack_folds(folds):
    """(nf, off, idx) of a list of integer index arrays: the packed fold list
    of ace_model_cv / ace_cv_from_inverse (fold f = idx[off[f]:off[f + 1]])."""
    fl = [np.ascontiguousarray(np.ravel(f), dtype=np.int64) for f in folds]
    if not fl:
        raise AceError("folds must hold at least one fold")
    off = np.zeros(len(fl) + 1, dtype=np.int64)
    np.cumsum([f.size for f in fl], out=off[1:])
    idx = np.concatenate(fl) if off[-1] else np.zeros(1, dtype=np.int64)
    return len(fl), off, np.ascontiguousarray(idx, dtype=np.int64)

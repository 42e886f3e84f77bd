"""The Python layer's shared pieces, without a GPU: the marshalling unit
(_marshal.py: converters, typed pointers, the map / ci / var allocator, the
ATE dictionaries, pack_folds), the resident guard of the kernel classes, the
named tuple _prepare returns, and the signature table against a frozen copy."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import additivecausalexpansion_amd as A
from additivecausalexpansion_amd import _lib, _marshal as M, model, native


def _f64(a, shape, order):
    assert a.dtype == np.float64 and a.shape == shape
    assert a.flags.f_contiguous if order == "F" else a.flags.c_contiguous


# ---------------------------------------------------------------- converters
C_MAT = np.arange(12.0).reshape(4, 3)
F_MAT = np.asfortranarray(C_MAT)


@pytest.mark.parametrize("x, size", [([1, 2, 3], 3), (C_MAT, 12), (F_MAT, 12),
                                     (np.arange(5, dtype=np.int64), 5), (np.float32(2.0), 1),
                                     (C_MAT[:, 1], 4)])
def test_vec_is_a_contiguous_float64_vector(x, size):
    v = M.vec(x)
    _f64(v, (size,), "C")
    assert np.array_equal(v, np.ravel(np.asarray(x, dtype=np.float64)))


@pytest.mark.parametrize("v", [2.5, np.float64(2.5), np.array(2.5), np.array([2.5]),
                               np.array([[2.5]]), [2.5], np.float32(2.5)])
def test_scalar_is_a_python_float(v):
    s = M.scalar(v)
    assert type(s) is float and s == 2.5


@pytest.mark.parametrize("a", [C_MAT.tolist(), C_MAT, F_MAT])
def test_cols_of_a_matrix(a):
    m = M.cols(a, 4)
    _f64(m, (4, 3), "F")
    assert np.array_equal(m, C_MAT)


@pytest.mark.parametrize("a", [[1, 2, 3, 4], np.arange(1.0, 5.0), np.arange(1, 5)])
def test_cols_of_a_vector_is_one_column(a):
    m = M.cols(a, 4)
    _f64(m, (4, 1), "F")
    assert np.array_equal(m[:, 0], [1, 2, 3, 4])


def test_cols_refuses_a_wrong_row_count():
    with pytest.raises(ValueError):
        M.cols(np.zeros(5), 4)


@pytest.mark.parametrize("a", [C_MAT.tolist(), C_MAT, F_MAT])
def test_rows_takes_a_matrix_as_it_is(a):
    m = M.rows(a, 3)
    _f64(m, (4, 3), "F")
    assert np.array_equal(m, C_MAT)


def test_rows_reads_a_vector_column_major():
    """The basis rows of a grid: k = max(B - 1, 1) columns."""
    m = M.rows(np.arange(6.0), 2)
    _f64(m, (3, 2), "F")
    assert np.array_equal(m, [[0, 3], [1, 4], [2, 5]])
    m = M.rows([7, 8, 9], max(1 - 1, 1))
    _f64(m, (3, 1), "F")
    assert np.array_equal(m[:, 0], [7, 8, 9])


@pytest.mark.parametrize("lab", [[0, 1, -1, 1], np.array([0, 1, -1, 1]),
                                 np.array([[0, 1], [-1, 1]], dtype=np.int64),
                                 np.array([0.0, 1.0, -1.0, 1.0])])
def test_labels_are_int32_one_per_point(lab):
    out = M.labels(lab, 4)
    assert out.dtype == np.int32 and out.shape == (4,) and out.flags.c_contiguous
    assert out.tolist() == [0, 1, -1, 1]


def test_labels_of_the_wrong_length():
    with pytest.raises(A.AceError, match="^label must have one entry per test point$"):
        M.labels([0, 1, 2], 4)


def test_conforming_arrays_are_not_copied():
    """The in-place contracts: what already conforms comes back as the same
    memory, so the library writes through to the caller's array."""
    th = np.linspace(0.0, 1.0, 11)
    assert np.shares_memory(M.vec(th), th) and M.vec(th).ctypes.data == th.ctypes.data
    thF = np.asfortranarray(np.zeros((11, 3)))
    assert np.shares_memory(_lib.fmat(thF), thF)
    assert np.shares_memory(M.cols(F_MAT, 4), F_MAT)
    assert np.shares_memory(M.rows(F_MAT, 3), F_MAT)
    col = np.arange(4.0)
    assert np.shares_memory(M.cols(col, 4), col)
    lab = np.array([0, 1, 2], dtype=np.int32)
    assert np.shares_memory(M.labels(lab, 3), lab)
    # and a non-conforming one is: the caller's array is left alone
    assert not np.shares_memory(M.vec(th.astype(np.float32)), th)
    assert not np.shares_memory(M.cols(C_MAT, 4), C_MAT)


def test_typed_pointers():
    for f, dtype, ctype in ((M.i32ptr, np.int32, ctypes.c_int32), (M.iptr, np.int64, ctypes.c_int64),
                            (M.u32ptr, np.uint32, ctypes.c_uint32)):
        a = np.array([3, 1, 4], dtype=dtype)
        p = f(a)
        assert isinstance(p, ctypes.POINTER(ctype))
        assert ctypes.addressof(p.contents) == a.ctypes.data and p[2] == 4
        assert f(None) is None
        with pytest.raises(AssertionError):
            f(a.astype(np.float64))
    assert native.iptr is M.iptr and native.pack_folds is M.pack_folds
    cube = np.zeros((2, 3, 4, 5), order="F")
    assert ctypes.addressof(_lib.ptr(cube).contents) == cube.ctypes.data


# ---------------------------------------------------------------- allocation
@pytest.mark.parametrize("lead", [(5,), (5, 3)])
def test_map_ci_var(lead):
    mp, ci, var, out = M.map_ci_var(*lead)
    _f64(mp, lead, "F")
    _f64(var, lead, "F")
    _f64(ci, lead + (2,), "F")
    assert list(out) == ["map", "ci", "var"]
    assert out["map"] is mp and out["ci"] is ci and out["var"] is var
    assert not np.shares_memory(mp, var)


def test_ate_dicts_of_a_12_vector():
    avg = np.array([0.5, 0.1, 0.9, 0.04, 1.5, 1.1, 1.9, 0.16, 2.5, 2.1, 2.9, 0.36])
    d = M.ate_dicts(avg)
    assert list(d) == ["ate", "att", "atu"]
    want = {"ate": (0.5, [0.1, 0.9], 0.04), "att": (1.5, [1.1, 1.9], 0.16),
            "atu": (2.5, [2.1, 2.9], 0.36)}
    for key, (mp, ci, var) in want.items():
        assert list(d[key]) == ["map", "ci", "var"]
        assert type(d[key]["map"]) is np.float64 and d[key]["map"] == mp
        assert type(d[key]["var"]) is np.float64 and d[key]["var"] == var
        assert d[key]["ci"].shape == (2,) and d[key]["ci"].tolist() == ci
        assert not np.shares_memory(d[key]["ci"], avg)


def test_ate_dicts_of_a_12_by_T_array():
    T = 3
    avg = np.asfortranarray(np.arange(12.0)[:, None] + 0.01 * np.arange(T)[None, :])
    d = M.ate_dicts(avg)
    assert list(d) == ["ate", "att", "atu"]
    for j, key in enumerate(d):
        e = d[key]
        assert list(e) == ["map", "ci", "var"]
        assert e["map"].shape == (T,) and e["var"].shape == (T,) and e["ci"].shape == (T, 2)
        assert e["map"].tolist() == [4 * j + 0.01 * t for t in range(T)]
        assert e["ci"].tolist() == [[4 * j + 1 + 0.01 * t, 4 * j + 2 + 0.01 * t] for t in range(T)]
        assert e["var"].tolist() == [4 * j + 3 + 0.01 * t for t in range(T)]
        assert all(np.shares_memory(e[k], avg) for k in e)  # views of avg, as before
    # a column of a 12 x M array (the batched engine) is the vector form
    one = M.ate_dicts(avg[:, 1])
    assert one["att"]["map"] == 4 + 0.01 and one["att"]["ci"].tolist() == [5 + 0.01, 6 + 0.01]
    assert type(one["att"]["map"]) is np.float64


def test_pack_folds():
    nf, off, idx = M.pack_folds([[4, 2, 7], np.array([1]), np.array([[0, 3], [5, 6]])])
    assert nf == 3 and off.tolist() == [0, 3, 4, 8] and idx.tolist() == [4, 2, 7, 1, 0, 3, 5, 6]
    assert off.dtype == np.int64 and idx.dtype == np.int64 and idx.flags.c_contiguous
    nf, off, idx = M.pack_folds([[1, 2], [], [0]])  # one empty fold
    assert nf == 3 and off.tolist() == [0, 2, 2, 3] and idx.tolist() == [1, 2, 0]
    nf, off, idx = M.pack_folds([[], []])  # nothing held out: still a valid pointer
    assert nf == 2 and off.tolist() == [0, 0, 0] and idx.shape == (1,) and idx.dtype == np.int64
    with pytest.raises(A.AceError, match="^folds must hold at least one fold$"):
        M.pack_folds([])


# ---------------------------------------------------------------- kernel classes
GUARDED = {
    "robust_treatment": lambda K, d: K.robust_treatment(*d, d[1], d[2], d[2], 1.0, 1.0),
    "coef_posterior": lambda K, d: K.coef_posterior(*d, d[1]),
    "predict_surface": lambda K, d: K.predict_surface(*d, d[1], d[2], False, 0.0, 1.0, 1.0),
    "coef_groups": lambda K, d: K.coef_groups(*d, d[1], 1, np.zeros(6, dtype=np.int32)),
    "average_response": lambda K, d: K.average_response(*d, d[1], 1, np.zeros(6, dtype=np.int32),
                                                        d[2], False, 0.0, 1.0, 1.0),
    "predict_joint": lambda K, d: K.predict_joint(*d, d[1], d[2], 0.0, 1.0, marginal=True),
    "cross_validate": lambda K, d: K.cross_validate(*d, [np.arange(3)], 0.0, 1.0),
}


@pytest.mark.parametrize("name", sorted(GUARDED))
def test_resident_guard_fires_before_any_library_call(name, monkeypatch):
    def touched(*a, **k):
        raise RuntimeError("the library was reached")
    for mod in (model, native):
        monkeypatch.setattr(mod, "lib", touched)
        monkeypatch.setattr(mod, "default_context", touched)
    rng = np.random.default_rng(3)
    data = (rng.normal(size=6), np.asfortranarray(rng.normal(size=(6, 2))),
            np.asfortranarray(rng.normal(size=(6, 2))))
    K = A.KernelClass_SE_R6(2, 3, np.zeros(2 + 3 * 3))  # never ran para_update
    with pytest.raises(A.AceError) as e:
        GUARDED[name](K, data)
    assert str(e.value) == (f"{name} needs the fit's device-resident inverse "
                            "(para_update on the same data)")


# ---------------------------------------------------------------- train
def test_prepare_is_a_named_eight_tuple():
    from additivecausalexpansion_amd.train import _prepare
    rng = np.random.default_rng(5)
    n = 12
    y, X, Z = rng.normal(size=n), rng.normal(size=(n, 2)), rng.normal(size=n)
    q = _prepare(y, X, Z, None, "ns", 2, None, 20.0, False)
    yv, Xi, Zi, px, moments, isbinary, basis, theta0 = q
    assert len(q) == 8
    assert q._fields == ("y", "X", "Z", "px", "moments", "isbinary", "basis", "theta0")
    for got, want in zip((q.y, q.X, q.Z, q.px, q.moments, q.isbinary, q.basis, q.theta0),
                         (yv, Xi, Zi, px, moments, isbinary, basis, theta0)):
        assert got is want
    assert px == 2 and yv.shape == (n,) and Xi.shape == (n, 2) and Zi.shape == (n, 1)
    assert Xi.flags.f_contiguous and Zi.flags.f_contiguous and moments.shape == (4, 3)
    assert not isbinary[0] and theta0.shape == (2 + basis.dim() * 3,)
    assert q[0] is yv and q[3] == 2 and q[6].B.shape[0] == n and q[7] is theta0


# ---------------------------------------------------------------- signatures
def test_signatures_equal_the_frozen_table():
    """tests/golden/signatures.json: name -> [restype, [argtypes]] as ctypes
    type names, written once from the table as it stood before the aliases."""
    with open(os.path.join(GOLDEN, "signatures.json")) as f:
        frozen = json.load(f)

    def name(t):
        return "None" if t is None else t.__name__
    now = {k: [name(res), [name(a) for a in args]] for k, (res, args) in _lib.SIGNATURES.items()}
    assert list(now) == list(frozen)
    for k in frozen:
        assert now[k] == frozen[k], k

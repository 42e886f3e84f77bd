"""CPU-side checks of the batched engine (ace_batch_* / ace_train_batch): the
library exports the new entry points with the declared signatures, and
ace_train_batch refuses datasets it cannot batch before it touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

BATCH = ("ace_batch_create", "ace_batch_destroy", "ace_batch_set_data", "ace_batch_para_update",
         "ace_batch_train", "ace_batch_get_inverse")

CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
         "double*": ctypes.POINTER(ctypes.c_double), "int*": ctypes.POINTER(ctypes.c_int32),
         "ace_ctx*": ctypes.c_void_p, "ace_batch*": ctypes.c_void_p,
         "ace_batch**": ctypes.POINTER(ctypes.c_void_p)}


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.lib()
    return pkg


def declared():
    """name -> (return type, [argument types]) of the header's ace_batch_* prototypes"""
    txt = open(os.path.join(ROOT, "include", "ace_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(ace_batch_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            a = a.replace("const", "").strip()
            stars = a.count("*")
            types.append(a.replace("*", " ").split()[0] + "*" * stars)
        out[name] = (ret, types)
    return out


def test_batch_symbols_exported_with_declared_signatures(A):
    from additivecausalexpansion_amd._lib import SIGNATURES, lib
    decl = declared()
    assert sorted(decl) == sorted(BATCH)
    L = lib()
    for name, (ret, types) in decl.items():
        assert hasattr(L, name), name
        res, args = SIGNATURES[name]
        assert res is (None if ret == "void" else ctypes.c_int), name
        assert args == [CTYPE[t] for t in types], (name, types)
    assert L.ace_abi_version() == 1  # functions were only added
    assert hasattr(A, "BatchModel") and hasattr(A, "ace_train_batch")


def _data(n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, p))
    z = rng.normal(size=(n, 1))
    y = X[:, 0] + z[:, 0] * X[:, -1] + 0.1 * rng.normal(size=n)
    return y, X, z


@pytest.fixture()
def no_context(A, monkeypatch):
    """Any attempt to create a context (or a batch) fails the test."""
    from additivecausalexpansion_amd import _lib, model

    def boom(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib.Context, "__init__", boom)
    monkeypatch.setattr(model, "default_context", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def test_train_batch_refuses_mixed_p(A, no_context):
    d = [_data(40, 2, 1), _data(40, 3, 2)]
    with pytest.raises(A.AceError, match="p = 3"):
        A.ace_train_batch([q[0] for q in d], [q[1] for q in d], [q[2] for q in d], maxiter=2)


def test_train_batch_refuses_mixed_basis_dimension(A, no_context):
    # a binary treatment takes the binary basis (B = 2) whatever was asked for,
    # a continuous one the natural cubic spline with two knots (B = 4)
    d = [_data(40, 2, 1), _data(40, 2, 2)]
    zb = (d[1][2] > 0).astype(float)
    with pytest.raises(A.AceError, match="basis dimension"):
        A.ace_train_batch([q[0] for q in d], [q[1] for q in d], [d[0][2], zb], basis="ns",
                          n_knots=2, maxiter=2)


def test_train_batch_refuses_mixed_kernel(A, no_context):
    d = [_data(40, 2, 1), _data(40, 2, 2)]
    with pytest.raises(A.AceError, match="one kernel"):
        A.ace_train_batch([q[0] for q in d], [q[1] for q in d], [q[2] for q in d],
                          kernel=["SE", "Matern32"], maxiter=2)


def test_train_batch_refuses_n_above_512(A, no_context):
    d = [_data(40, 2, 1), _data(513, 2, 2)]
    with pytest.raises(A.AceError, match="513"):
        A.ace_train_batch([q[0] for q in d], [q[1] for q in d], [q[2] for q in d], maxiter=2)


def test_train_batch_refuses_ragged_arguments(A, no_context):
    d = [_data(40, 2, 1), _data(40, 2, 2)]
    with pytest.raises(A.AceError, match="length M"):
        A.ace_train_batch([q[0] for q in d], [q[1] for q in d], [q[2] for q in d],
                          init_length_scale=[20.0, 10.0, 5.0], maxiter=2)

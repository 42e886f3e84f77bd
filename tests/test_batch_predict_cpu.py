"""CPU-side checks of batched prediction (ace_predict_batch,
ace_predict_marginal_batch, ace_set_inverse_batch, predict_ace_batch): the
library exports the entry points with the declared signatures,
predict_ace_batch refuses fits it cannot batch before it touches a GPU, and
the oracle alone gives ATE/ATT/ATU square roots that exist for every case the
GPU tests compare (tests/batch_predict_cases.ate_cases)."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import batch_predict_cases as PC

NEW = ("ace_predict_batch", "ace_predict_marginal_batch", "ace_set_inverse_batch")

CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
         "double*": ctypes.POINTER(ctypes.c_double), "int*": ctypes.POINTER(ctypes.c_int32),
         "int64_t*": ctypes.POINTER(ctypes.c_int64),
         "ace_ctx*": ctypes.c_void_p, "ace_batch*": ctypes.c_void_p,
         "ace_batch**": ctypes.POINTER(ctypes.c_void_p)}


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.lib()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


def declared():
    """name -> (return type, [argument types]) of the header's ace_*_batch prototypes"""
    txt = open(os.path.join(ROOT, "include", "ace_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(ace_[a-z_]+_batch)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            a = a.replace("const", "").strip()
            stars = a.count("*")
            types.append(a.replace("*", " ").split()[0] + "*" * stars)
        out[name] = (ret, types)
    return out


def test_batch_predict_symbols_exported_with_declared_signatures(A):
    from additivecausalexpansion_amd._lib import SIGNATURES, lib
    decl = declared()
    assert sorted(decl) == sorted(NEW)
    L = lib()
    for name, (ret, types) in decl.items():
        assert hasattr(L, name), name
        res, args = SIGNATURES[name]
        assert res is ctypes.c_int and ret == "int", name
        assert args == [CTYPE[t] for t in types], (name, types)
    assert L.ace_abi_version() == 1  # functions were only added
    assert hasattr(A, "predict_ace_batch")
    for m in ("predict", "predict_marginal", "set_inverse"):
        assert hasattr(A.BatchModel, m), m


@pytest.fixture()
def no_context(A, monkeypatch):
    """Any attempt to create a context (or a batch) fails the test."""
    from additivecausalexpansion_amd import _lib, model

    def boom(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib.Context, "__init__", boom)
    monkeypatch.setattr(model, "default_context", boom)
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(model.BatchModel, "__init__", boom)


def _fit(A, kernel="SE", n=40, p=2, B=3, seed=1):
    """A fit as ace_train_batch returns it, put together on the host."""
    from additivecausalexpansion_amd.model import KernelClass_Matern32_R6, KernelClass_SE_R6
    from additivecausalexpansion_amd.synthetic import make_problem
    from additivecausalexpansion_amd.train import AceFit, square_spline
    y, X, Zb, th, sy = make_problem(n, p, B, seed=seed)
    K = (KernelClass_Matern32_R6 if kernel == "Matern32" else KernelClass_SE_R6)(p, B, th, sy)
    K._inv = np.eye(n)
    basis = square_spline()
    basis.B = Zb
    mom = np.zeros((2 + p, 3))
    mom[:, 1] = 1.0
    return AceFit(Kernel=K, Basis=basis, moments=mom,
                  train_data={"y": y, "X": X, "Z": np.zeros((n, 1)), "Zbinary": np.array([False])})


def test_predict_batch_refuses_none(A, no_context):
    with pytest.raises(A.AceError, match="None"):
        A.predict_ace_batch([_fit(A), None])


def test_predict_batch_refuses_mixed_kernel(A, no_context):
    with pytest.raises(A.AceError, match="one kernel"):
        A.predict_ace_batch([_fit(A), _fit(A, kernel="Matern32")])


def test_predict_batch_refuses_mixed_p(A, no_context):
    with pytest.raises(A.AceError, match="p = 3"):
        A.predict_ace_batch([_fit(A), _fit(A, p=3)])


def test_predict_batch_refuses_mixed_basis_dimension(A, no_context):
    with pytest.raises(A.AceError, match="basis dimension B = 2"):
        A.predict_ace_batch([_fit(A), _fit(A, B=2)])


def test_predict_batch_refuses_n_above_512(A, no_context):
    with pytest.raises(A.AceError, match="513"):
        A.predict_ace_batch([_fit(A), _fit(A, n=513)])


@pytest.mark.parametrize("kernel", PC.KERNELS)
def test_oracle_ate_radicands_are_positive(O, kernel):
    """The oracle alone (its kernels, its inverse, theta_T = theta_{T-1}): the
    posterior variances of ATE / ATT / ATU are finite and strictly positive
    wherever the group is not empty, for every case the GPU tests use."""
    for B, j, case in PC.ate_cases():
        ms = PC.models(PC.ATE_NS, PC.ATE_NXS, PC.ATE_P, B, PC.ATE_SEED0)
        th = PC.theta_now(ms[j][0][3], mix=False)
        zx = PC.treated(PC.ATE_NXS[j], case)
        ref, _ = PC.oracle_marginal(O, kernel, ms[j], th, zx, PC.std_y(j), PC.std_Z(j))
        keys = {"third": ("ate", "att", "atu"), "none_treated": ("ate", "atu"),
                "all_treated": ("ate", "att")}[case]
        for k in keys:
            v = ref[k]["var"]
            assert np.isfinite(v) and v > 0.0, (kernel, B, j, case, k, v)

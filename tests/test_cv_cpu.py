"""CPU-side checks of cross-validation from the resident inverse:
the referee (tests/cv_ref.py) against the identity the device uses, the fold
plan (csrc/ace_cv_plan.cpp) under AddressSanitizer + UBSan, and the loud
failure without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cv_ref as C
import joint_ref as J
from conftest import ROOT

KERNELS = ["SE", "Matern32"]
IDENTITY_TOL = 1e-10  # measured: <= 1.0e-12 (SE 300/70)


@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_identity_matches_explicit_conditioning(kernel, case):
    """B_F^-1 alpha_F, diag B_F^-1 and lpd from the oracle's invkernel_cpp
    inverse against explicit conditioning on the remaining rows, for every
    fold the GPU tests use; B_F is SPD with cond(B_F) <= cond(A), so a device
    status != 0 on these inputs can only be a defect."""
    s = J.problem(case, kernel)
    y, mu, inv = np.ravel(s["y"]), s["th"][1], s["inv"]
    A = C.system(case, kernel)
    condA = np.linalg.cond(A)
    worst = 0.0
    for name in C.sets_of(case):
        folds = C.fold_sets(s["n"])[name]
        if name == "loo":  # every tenth row here: the GPU test holds all of them
            folds = folds[::10]
            ref = C.pack([C.condition(A, y, mu, F) for F in folds])
        else:
            ref = C.reference(case, kernel, name)
        got = C.pack([C.from_inverse(inv, y, mu, F) for F in folds])
        for k in ("map", "var", "resid", "lpd", "mahal"):
            scale = np.abs(ref[k]).max()
            err = np.abs(got[k] - ref[k]).max() / scale
            worst = max(worst, err)
            assert err <= IDENTITY_TOL, (name, k, err)
        for F in C.fold_sets(s["n"])[name]:
            f = C.from_inverse(inv, y, mu, F)
            ev = np.linalg.eigvalsh(f["B"])
            assert ev[0] > 0 and f["sign"] > 0
            assert ev[-1] / ev[0] <= condA * (1 + 1e-8)
    print(f"{kernel} {case}: identity vs conditioning, max rel err {worst:.2e}")


def test_cv_plan_is_consistent_and_sanitizer_clean(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "additivecausalexpansion_amd", "csrc")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "cv_plan_check")
    subprocess.run([gxx, *flags, "-std=c++17", "-I", csrc,
                    os.path.join(ROOT, "tests", "cv_plan_check.cpp"),
                    os.path.join(csrc, "ace_cv_plan.cpp"), "-o", exe], check=True)
    # verify_asan_link_order=0: the process environment may preload other
    # libraries ahead of the ASan runtime; that is not a finding
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cv_plan_check: OK" in out.stdout


class _Basis:
    def __init__(self, B):
        self.B = B


def test_no_resident_inverse_and_no_gpu_fail_loudly():
    """No CPU fallback: a fit whose inverse is not device-resident, and a
    DeviceModel on a machine without a GPU, raise AceError."""
    import ctypes

    import additivecausalexpansion_amd as A
    from additivecausalexpansion_amd._lib import lib
    rng = np.random.default_rng(0)
    n = 20
    y, X = rng.normal(size=n), np.asfortranarray(rng.normal(size=(n, 2)))
    Bm = np.asfortranarray(rng.normal(size=(n, 1)))
    K = A.KernelClass_SE_R6(2, 2, np.zeros(2 + 2 * 3))
    fit = {"Kernel": K, "train_data": {"y": y, "X": X}, "Basis": _Basis(Bm),
           "moments": np.array([[0.0, 1.0, 0.0]])}
    for folds in (5, "loo", [np.arange(3)]):
        with pytest.raises(A.AceError, match="device-resident inverse"):
            A.cross_validate(fit, folds=folds)
    with pytest.raises(A.AceError):
        A.cross_validate(fit, folds="kfold")
    h = ctypes.c_void_p()
    if lib().ace_create(0, ctypes.byref(h)) == 0:
        lib().ace_destroy(h)
        return  # a GPU is visible: tests/test_cv_gpu.py covers the device
    with pytest.raises(A.AceError):
        A.DeviceModel("SE", n, 2, 2).cv(np.zeros(8), [np.arange(3)], 0.0, 1.0)
    with pytest.raises(A.AceError):
        A.cv_from_inverse(np.eye(4), np.ones(4), [np.arange(2)])

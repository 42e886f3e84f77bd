"""The inputs of tests/test_dmat_state_gpu.py, checked on the CPU with the
oracle alone (tests/dmat_cases.py): the library is not called here."""
import numpy as np
import pytest

import dmat_cases as C
from oracle import ace_oracle as O
from test_gpu import close


@pytest.mark.parametrize("kernel,name,dsigma", C.healthy_cases())
def test_healthy_problems_are_positive_definite(kernel, name, dsigma):
    """A = Kfull + e^sigma I is positive definite and the oracle's own inverse
    satisfies |A inv - I| <= 1e-9, the bound the GPU inverse is held to."""
    s = C.oracle_state(kernel, name, dsigma)
    n = s["full"].shape[0]
    A = s["full"] + np.exp(s["th"][0]) * np.eye(n)
    w = np.linalg.eigvalsh(A)
    print(f"{kernel} {name} dsigma {dsigma}: n {n} eig [{w[0]:.3e}, {w[-1]:.3e}] "
          f"cond {w[-1] / w[0]:.3e}")
    assert w[0] > 0
    assert np.all(s["eigenval"] > 0)
    assert np.max(np.abs(A @ s["inv"] - np.eye(n))) <= 1e-9


@pytest.mark.parametrize("n", [130, 300])
def test_nonpd_input_has_a_negative_eigenvalue(n):
    A = C.nonpd_matrix(n) + np.exp(C.NONPD_SIGMA) * np.eye(n)
    assert np.linalg.eigvalsh(A)[0] < 0


@pytest.mark.parametrize("n1,n2,B", [(130, 130, 4), (37, 130, 4), (130, 1, 130), (37, 1, 130)])
def test_region_list_covers_every_case(n1, n2, B):
    regs = C.regions(n1, n2, B)
    assert C.region_coverage(regs, n1, n2, B) >= C.REGION_CASES
    sl = n1 * n2
    for off, cnt in C.slice_cache_reads(n1, n2):
        assert 0 <= off and off + cnt <= sl * B
    slices = [sorted({off // sl, (off + cnt - 1) // sl}) for off, cnt in C.slice_cache_reads(n1, n2)]
    assert slices == [[2], [0], [0, 1], [2]]
    e = C.element_reads(n1, n2)
    if sl >= 300:
        assert len(e) == 600 and e[0] < sl <= e[-1] and np.all(np.diff(e) == 1)


@pytest.mark.parametrize("kernel", C.KERNEL_NAMES)
def test_chunk_reference_is_the_oracles(kernel):
    """The numpy shortcut of the chunked prediction (no nx x nx K_xx) against
    pred_cpp / pred_marginal_cpp on 200 of its rows, the chunk boundary's
    included, at 1e-12."""
    c = C.chunk_case(kernel)
    rows = C.chunk_subset()
    assert rows.shape == (200,) and np.unique(rows).shape == (200,)
    assert np.any(rows < 8192) and np.any(rows >= 8192)
    y, X, Z, th, inv = c["y"], c["X"], c["Z"], c["th"], c["inv"]
    X2, Z2, dZ2 = c["X2"][rows], c["Z2"][rows], c["dZ2"][rows]
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    ref = O.pred_cpp(y, th[0], th[1], inv, cross(X2, X, Z2, Z, th)["full"],
                     sym(X2, Z2, th)["full"], C.MEAN_Y, C.STD_Y)
    close(c["pred"]["map"][rows], ref["map"], 1e-12, 1e-12)
    close(c["pred"]["var"][rows], ref["var"], 1e-12, 1e-12)
    ref = O.pred_marginal_cpp(y, None, th[0], th[1], inv, cross(X2, X, dZ2, Z, th)["elements"],
                              sym(X2, dZ2, th)["elements"], C.MEAN_Y, C.STD_Y, C.STD_Z, False)
    close(c["marginal"]["map"][rows], ref["map"], 1e-12, 1e-12)
    close(c["marginal"]["var"][rows], ref["var"], 1e-12, 1e-12)
    # the variance's bound in the GPU test is VAR_TOL of these terms: they are
    # the sizes of what the variance cancels, never smaller than the variance
    assert np.all(c["pred"]["terms"] >= c["pred"]["var"] * (1 - 1e-12))
    assert np.all(c["marginal"]["terms"] >= c["marginal"]["var"] * (1 - 1e-12))

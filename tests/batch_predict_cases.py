"""Cases and oracle references shared by the batched prediction's tests
(tests/test_batch_predict_cpu.py, tests/test_batch_predict_gpu.py) -- TEST
INFRASTRUCTURE ONLY, plain numpy and the oracle.

The convention is test_predict_gpu._fit_state's: the resident inverse at
theta_{T-1} = make_problem's theta (para_update(2, theta)), the kernels at
theta_T = theta + 0.02 with theta_T[1] = 0.13 (the Q6 mix), or at theta itself
with theta_T[1] = 0.13 (mix off) where ATE/ATT/ATU's square roots must exist.
"""
import numpy as np

import batch_cases as C

KERNELS = ("SE", "Matern32")

# (n per model, nx per model, p, B)
PLAIN_CASES = [
    ((7, 16, 17, 64, 65, 130), (1, 15, 16, 17, 33, 70), 3, 5),  # the ragged batch
    ((33,), (9,), 1, 1),
    ((97,), (20,), 17, 2),    # PM = 32 at 256 threads
    ((70,), (18,), 64, 2),
    ((50,), (10,), 2, 32),
    ((512,), (40,), 2, 2),    # the largest LDS
    ((257,), (49,), 20, 3),
]
# every LDS region of the prediction kernel at its maximum: 157.9 KiB of 160
MAX_LDS_CASE = ((512,), (20,), 33, 32)
ATE_NS, ATE_NXS, ATE_P, ATE_BS = (130, 65, 17), (50, 33, 16), 3, (1, 2, 6)
EDGE_B = 6  # the empty-group and independence tests use the ATE models of this B
ATE_SEED0 = 0  # seed offset of the ATE models; the CPU pre-check holds for it


def mean_y(j):
    return 0.3 - 0.25 * j


def std_y(j):
    return 1.7 + 0.3 * j


def std_Z(j):
    return 0.8 + 0.1 * j


def models(ns, nxs, p, B, seed0=0):
    """[(problem, X2, Z2)]: make_problem's training side and test side."""
    from additivecausalexpansion_amd.synthetic import make_problem
    probs = C.problems(ns, p, B, seed0)
    out = []
    for j, (prob, nx) in enumerate(zip(probs, nxs)):
        # (the first nx of at least 40 points: make_problem's basis needs a sample)
        _, X2, Z2, _, _ = make_problem(max(nx, 40), p, B, seed=1000 + seed0 + 13 * j + nx)
        out.append((prob, np.asfortranarray(X2[:nx]), np.asfortranarray(Z2[:nx])))
    return out


def theta_now(th, mix=True):
    t = th + 0.02 if mix else th.copy()
    t[1] = 0.13
    return t


def dbasis(Z2):
    return np.asfortranarray(Z2 * 0.7 + 0.1)  # a stand-in derivative basis


def treated(nx, case="third"):
    if case == "none_treated":
        return np.zeros(nx)
    if case == "all_treated":
        return np.ones(nx)
    return (np.arange(nx) % 3 == 0).astype(float)


def oracle_inverse(O, kernel, prob):
    y, X, Z, th, _ = prob
    return O.invkernel_cpp(O.KERNELS[kernel][0](X, Z, th)["full"], th[0])["inv"]


def oracle_plain(O, kernel, model, th, my, sy, inv=None):
    """(pred_cpp's result, the terms the variance cancels) of one model."""
    (y, X, Z, _, _), X2, Z2 = model
    inv = oracle_inverse(O, kernel, model[0]) if inv is None else inv
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    K_xX = cross(X2, X, Z2, Z, th)["full"]
    K_xx = sym(X2, Z2, th)["full"]
    ref = O.pred_cpp(y, th[0], th[1], inv, K_xX, K_xx, my, sy)
    q = np.abs(np.sum((K_xX @ inv) * K_xX, axis=1))
    terms = sy ** 2 * (np.abs(np.diag(K_xx)) + q + np.exp(th[0]))
    return ref, terms


def oracle_marginal(O, kernel, model, th, zx, sy, sz, ate=True):
    """(pred_marginal_cpp's result, the terms the variance cancels)."""
    (y, X, Z, _, _), X2, Z2 = model
    B = Z.shape[1] + 1
    dZ2 = dbasis(Z2)
    inv = oracle_inverse(O, kernel, model[0])
    sym, cross = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    Km_xX = cross(X2, X, dZ2, Z, th)["elements"]
    Km_xx = sym(X2, dZ2, th)["elements"]
    ref = O.pred_marginal_cpp(y, zx, th[0], th[1], inv, Km_xX, Km_xx, 0.3, sy, sz, ate)
    sl = slice(1, B) if B > 1 else slice(0, 1)
    KmX = Km_xX[:, :, sl].sum(axis=2)
    kxx = np.diag(Km_xx[:, :, sl].sum(axis=2))
    q = np.abs(np.sum((KmX @ inv) * KmX, axis=1))
    return ref, (sy / sz) ** 2 * (np.abs(kxx) + q)


def ate_cases():
    """Every (B, model index, treatment pattern) whose ATE/ATT/ATU the GPU
    tests compare: the three models with every third point treated for each
    B, and for EDGE_B the first model with no treated and the second with no
    untreated point."""
    out = [(B, j, "third") for B in ATE_BS for j in range(len(ATE_NS))]
    return out + [(EDGE_B, 0, "none_treated"), (EDGE_B, 1, "all_treated")]

"""Inputs of the device-handle state tests (tests/test_dmat_state_gpu.py):
the problems, the oracle's results for them (computed once and shared,
read-only), the region lists of ace_dmat_read and the numpy reference of the
chunked prediction.  No GPU code; tests/test_dmat_cases_cpu.py checks these
inputs on the CPU (healthy where they should be, broken where they should
be, the regions covering every slice-boundary case, the chunk reference tied
to the oracle's pred_cpp / pred_marginal_cpp)."""
import functools

import numpy as np

from additivecausalexpansion_amd.synthetic import make_problem
from oracle import ace_oracle as O

KERNEL_NAMES = ("SE", "Matern32")

# name: (n, p, B, seed).  n = 300 is no multiple of 64 / 128 / 256 and takes
# two sweep blocks with a ragged one, n = 130 a single block.
PROBLEMS = {
    "n130": (130, 3, 4, 61),
    "n130b": (130, 3, 4, 62),
    "n300": (300, 3, 4, 63),
    "n300b": (300, 3, 4, 64),
    "n300_p2B5": (300, 2, 5, 65),   # another (p, B) at the same n
    "n299": (299, 3, 4, 66),        # a response of another length
    "B1_p1": (130, 1, 1, 67),
    "B1_p20": (130, 20, 1, 68),     # p at the edge of a feature bucket
    "chunk": (333, 2, 3, 3),        # test_device_predict_chunks_and_padding's shape
}
CHUNK_NX = 8192 + 77
NONPD_SIGMA = -5.0


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def vary_theta(th, seed):
    """make_problem's theta has equal amplitudes and length scales in every
    slice; perturbed, a swapped slice or feature index changes the values."""
    rng = np.random.default_rng(1000 + seed)
    t = th + 0.15 * rng.normal(size=th.shape)
    t[0], t[1] = th[0], th[1]
    return t


@functools.lru_cache(maxsize=None)
def problem(name):
    """(y, X, Z, theta, std_y) of PROBLEMS[name], read-only."""
    n, p, B, seed = PROBLEMS[name]
    y, X, Z, th, sy = make_problem(n, p, B, seed=seed)
    return frozen(y), frozen(X), frozen(Z), frozen(vary_theta(th, seed)), sy


@functools.lru_cache(maxsize=None)
def new_points(name, nx, scale=1.0, shift=0.0):
    """(X2, Z2) for PROBLEMS[name]'s (p, B); Z2 * scale + shift stands in for
    a derivative basis in the marginal cases."""
    _, p, B, seed = PROBLEMS[name]
    _, X2, Z2, _, _ = make_problem(nx, p, B, seed=seed + 500)
    return frozen(X2), frozen(np.asfortranarray(Z2 * scale + shift))


def oracle_kernel(kernel, X, Z, th):
    r = O.KERNELS[kernel][0](X, Z, th)
    return {k: frozen(np.asfortranarray(v)) for k, v in r.items()}


def oracle_inverse(Kfull, sigma):
    r = O.invkernel_cpp(Kfull, sigma)
    return {k: frozen(np.asfortranarray(v)) for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def oracle_state(kernel, name, dsigma=0.0):
    """The oracle's kernels and inverse for a problem at its theta (sigma
    shifted by dsigma), and mu = mu_solution_cpp: computed once, read-only."""
    y, X, Z, th, sy = problem(name)
    th = th.copy()
    th[0] += dsigma
    K = oracle_kernel(kernel, X, Z, th)
    inv = oracle_inverse(K["full"], th[0])
    mu = O.mu_solution_cpp(y, inv["inv"])
    th[1] = mu
    return {"y": y, "X": X, "Z": Z, "th": frozen(th), "sy": sy, "full": K["full"],
            "elements": K["elements"], "inv": inv["inv"], "eigenval": inv["eigenval"], "mu": mu}


def oracle_grad(kernel, y, X, Z, Kfull, K, inv, eigenval, th, sy):
    st = np.zeros(2)
    B = K.shape[2]
    g = O.KERNELS[kernel][2](y, X, Z, Kfull, K, inv, eigenval, np.array(th), st, B, sy)
    return g, st


def healthy_cases():
    """Every (kernel, problem, dsigma) whose A = Kfull + e^sigma I the GPU
    tests invert."""
    out = [(k, name, 0.0) for k in KERNEL_NAMES for name in PROBLEMS]
    out += [(k, "n300", 0.7) for k in KERNEL_NAMES]  # two inverses alive, different sigma
    return out


def nonpd_matrix(n):
    return -np.eye(n)


# ---------------------------------------------------------------- regions
def regions(n1, n2, B):
    """(name, offset, count) reads of an n1 x n2 x B column-major cube, B >= 3.
    For a matrix pass (rows, 1, cols): its "slices" are then the columns."""
    sl, total = n1 * n2, n1 * n2 * B
    assert B >= 3 and sl >= 32
    return [
        ("first element of the cube", 0, 1),
        ("first element of slice 1", sl, 1),
        ("last element of slice 1", 2 * sl - 1, 1),
        ("last element of the cube", total - 1, 1),
        ("inside slice 1", sl + 5, 17),
        ("ends on the boundary 1|2", 2 * sl - 11, 11),
        ("starts on the boundary 1|2", 2 * sl, 13),
        ("starts on the boundary 0|1 and ends on 1|2", sl, sl),
        ("spans the boundaries 0|1 and 1|2", sl - 7, sl + 14),
        ("the whole cube", 0, total),
        ("nothing at 0", 0, 0),
        ("nothing at total", total, 0),
    ]


def region_coverage(regs, n1, n2, B):
    """Which of the issue's cases a region list reaches (for the CPU check)."""
    sl, total = n1 * n2, n1 * n2 * B
    got = set()
    for _, off, cnt in regs:
        assert 0 <= off and 0 <= cnt and off + cnt <= total
        end = off + cnt
        if cnt == 0:
            got.add("empty at 0" if off == 0 else "empty at total" if off == total else "empty")
            continue
        crossed = sum(1 for b in range(1, B) if off < b * sl < end)
        if cnt == 1 and off % sl == 0:
            got.add("single first of slice")
        if cnt == 1 and off % sl == sl - 1:
            got.add("single last of slice")
        if cnt > 1 and crossed == 0 and off % sl != 0 and end % sl != 0:
            got.add("inside one slice")
        if cnt > 1 and end % sl == 0 and off % sl != 0 and crossed == 0:
            got.add("ends on a boundary")
        if cnt > 1 and off % sl == 0 and off > 0 and end % sl != 0 and crossed == 0:
            got.add("starts on a boundary")
        if crossed >= 2 and off % sl != 0 and end % sl != 0:
            got.add("spans two boundaries")
        if off == 0 and cnt == total:
            got.add("whole")
    return got


REGION_CASES = {"single first of slice", "single last of slice", "inside one slice",
                "ends on a boundary", "starts on a boundary", "spans two boundaries", "whole",
                "empty at 0", "empty at total"}


def slice_cache_reads(n1, n2):
    """Slice 2, slice 0, a region straddling 0|1, slice 2 again (a cube with
    B >= 3): each replaces or reuses the handle's one cached slice."""
    sl = n1 * n2
    return [(2 * sl, sl), (0, sl), (sl - 19, 40), (2 * sl, sl)]


def element_reads(n1, n2, count=600):
    """Offsets of `count` consecutive one-element reads across 0|1."""
    sl = n1 * n2
    return list(range(sl - count // 2, sl + count // 2))


# ---------------------------------------------------------------- chunked prediction
MEAN_Y, STD_Y, STD_Z = 0.5, 1.5, 0.8


def closed_form_diag(Z2, th, marginal):
    """diag of the test points' kernel: r = 0, so slice 0 is exp(lam_0) and
    slice b is z_b^2 exp(lam_b), for both kernels; marginal: slices 1..B-1."""
    B = Z2.shape[1] + 1
    k = np.zeros(Z2.shape[0]) if marginal else np.full(Z2.shape[0], np.exp(th[2]))
    for b in range(1, B):
        k = k + Z2[:, b - 1] ** 2 * np.exp(th[2 + b])
    return k


@functools.lru_cache(maxsize=None)
def chunk_case(kernel):
    """The chunked prediction's inputs and numpy reference: the inverse at
    theta_{T-1} = th, kernels at theta_T = th + 0.02 (Q6, as
    test_predict_gpu._fit_state), nx = 8192 + 77 test points.  The reference
    is src/pred_cpp.cpp:19-28 and :55-80 without the nx x nx K_xx: only its
    diagonal enters map and var, and that is closed_form_diag."""
    y, X, Z, th_prev, sy = problem("chunk")
    X2, Z2 = new_points("chunk", CHUNK_NX)
    dZ2 = frozen(np.asfortranarray(Z2 * 0.7 + 0.1))
    th = th_prev + 0.02
    th[1] = 0.13
    inv = oracle_inverse(oracle_kernel(kernel, X, Z, th_prev)["full"], th_prev[0])["inv"]
    out = {"y": y, "X": X, "Z": Z, "th_prev": th_prev, "th": frozen(th), "X2": X2, "Z2": Z2,
           "dZ2": dZ2, "inv": inv}
    w = y - th[1]
    K_xX = O.KERNELS[kernel][1](X2, X, Z2, Z, th)["full"]
    tmp = K_xX @ inv
    kxx = closed_form_diag(Z2, th, False)
    q = np.sum(tmp * K_xX, axis=1)
    out["pred"] = {"map": frozen(MEAN_Y + STD_Y * (tmp @ w + th[1])),
                   "var": frozen((STD_Y * np.sqrt(np.abs(kxx - q + np.exp(th[0])))) ** 2),
                   "terms": frozen(STD_Y ** 2 * (np.abs(kxx) + np.abs(q) + np.exp(th[0])))}
    E = O.KERNELS[kernel][1](X2, X, dZ2, Z, th)["elements"]
    out["KmxX"] = frozen(np.asfortranarray(E))
    Km = E[:, :, 1].copy()
    for b in range(2, E.shape[2]):
        Km = Km + E[:, :, b]
    tmp = Km @ inv
    kxx = closed_form_diag(dZ2, th, True)
    q = np.sum(tmp * Km, axis=1)
    s = STD_Y / STD_Z
    out["marginal"] = {"map": frozen(s * (tmp @ w)),
                       "var": frozen((s * np.sqrt(np.abs(kxx - q))) ** 2),
                       "terms": frozen(s ** 2 * (np.abs(kxx) + np.abs(q)))}
    return out


def chunk_boundary_rows():
    return np.arange(8192 - 64, 8192 + 77)


def chunk_subset():
    """200 rows for the CPU tie to the oracle: 100 around the chunk boundary,
    100 spread over the rest."""
    return np.concatenate([np.linspace(0, 8100, 100).astype(int), np.arange(8192 - 50, 8192 + 50)])

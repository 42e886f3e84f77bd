"""The numpy referee of cross-validation from the resident inverse
(ace_model_cv).  It never uses the inverse identity: for each fold
F it conditions explicitly on the remaining rows R of A = K(theta_{T-1}) +
e^sigma I (the oracle's kernel), mu = theta_T[1]:
    E[y_F | y_R] = mu + A_FR solve(A_RR, y_R - mu),
    C_F = A_FF - A_FR solve(A_RR, A_RF),  slogdet(C_F).
Shared by tests/test_cv_cpu.py (which ties it to the identity through the
oracle's invkernel_cpp) and tests/test_cv_gpu.py; every state is computed once
and never modified.  The problems are those of tests/joint_ref.py."""
import functools

import numpy as np

import joint_ref as J

MEAN_Y, STD_Y = J.MEAN_Y, J.STD_Y
CASES = ["130/9", "300/70", "700/257"]
SETS = ["loo", "mixed", "m64", "m100", "ragged", "overlap", "descending"]


def fold_sets(n):
    """The fold sets of a case of n rows, by name (lists of index arrays)."""
    rng = np.random.default_rng(1000 + n)
    perm = rng.permutation(n)
    cuts = np.sort(rng.choice(np.arange(1, n), 6, replace=False))
    out = {
        "loo": [np.array([i]) for i in range(n)],
        "mixed": [perm[0:1], perm[1:16], perm[16:32], perm[32:49]],  # 1, 15, 16, 17 rows
        "m64": [perm[50:114]],
        "m100": [perm[10:110]],
        "ragged": np.split(rng.permutation(n), cuts),  # a partition, seven ragged folds
        "overlap": [perm[:40], perm[20:70]],
        "descending": [np.sort(perm[:33])[::-1].copy()],
    }
    if n == 700:  # 513: the smallest fold the whole-chip sweep takes by default
        out["split513"] = [perm[:513], perm[513:]]
    return out


def sets_of(case):
    return SETS + (["split513"] if J.CASES[case][0] == 700 else [])


@functools.lru_cache(maxsize=None)
def system(case, kernel):
    """A = K(theta_{T-1}) + e^sigma I of the case, read-only."""
    from oracle import ace_oracle as O
    s = J.problem(case, kernel)
    A = O.KERNELS[kernel][0](s["X"], s["Z"], s["th_prev"])["full"] + \
        np.exp(s["th_prev"][0]) * np.eye(s["n"])
    A = 0.5 * (A + A.T)
    A.setflags(write=False)
    return A


def condition(A, y, mu, F, std_y=STD_Y, mean_y=MEAN_Y):
    """One fold by explicit conditioning on the other rows (idx's order)."""
    n = A.shape[0]
    F = np.asarray(F)
    R = np.setdiff1d(np.arange(n), F)
    m = F.size
    if R.size:
        S = np.linalg.solve(A[np.ix_(R, R)], np.column_stack([y[R] - mu, A[np.ix_(R, F)]]))
        mean = mu + A[np.ix_(F, R)] @ S[:, 0]
        C = A[np.ix_(F, F)] - A[np.ix_(F, R)] @ S[:, 1:]
    else:
        mean, C = np.full(m, mu), A[np.ix_(F, F)].copy()
    C = 0.5 * (C + C.T)
    r = y[F] - mean
    mahal = float(r @ np.linalg.solve(C, r))
    sign, ld = np.linalg.slogdet(C)
    assert sign > 0
    lpd = -0.5 * mahal - 0.5 * ld - 0.5 * m * np.log(2 * np.pi) - m * np.log(std_y)
    return dict(map=mean_y + std_y * mean, var=std_y ** 2 * np.diag(C), resid=std_y * r,
                lpd=lpd, mahal=mahal, cov=C)


def pack(per_fold):
    out = {k: np.concatenate([f[k] for f in per_fold]) for k in ("map", "var", "resid")}
    out["lpd"] = np.array([f["lpd"] for f in per_fold])
    out["mahal"] = np.array([f["mahal"] for f in per_fold])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case, kernel, name):
    """map, var, resid (packed fold after fold, idx's order), lpd, mahal of
    one fold set."""
    s = J.problem(case, kernel)
    A = system(case, kernel)
    y = np.ravel(s["y"])
    return pack([condition(A, y, s["th"][1], F) for F in fold_sets(s["n"])[name]])


def from_inverse(inv, y, mu, F, std_y=STD_Y, mean_y=MEAN_Y):
    """The identity the device uses, in numpy: B_F = inv[F, F], alpha = inv (y - mu)."""
    F = np.asarray(F)
    al = (inv @ (y - mu))[F]
    Bf = inv[np.ix_(F, F)]
    Bf = 0.5 * (Bf + Bf.T)
    r = np.linalg.solve(Bf, al)
    sign, ld = np.linalg.slogdet(Bf)
    m = F.size
    mahal = float(al @ r)
    lpd = -0.5 * mahal + 0.5 * ld - 0.5 * m * np.log(2 * np.pi) - m * np.log(std_y)
    return dict(map=mean_y + std_y * (y[F] - r), var=std_y ** 2 * np.diag(np.linalg.inv(Bf)),
                resid=std_y * r, lpd=lpd, mahal=mahal, B=Bf, sign=sign)

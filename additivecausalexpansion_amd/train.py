"""User API mirror: ace.train / predict.ace (R/main_ace.R:132-254,
R/predict.ace.R:30-99), the basis classes (R/spline_*_R6.R) and the
parameter initialisation (R/parameters.R).  Host preprocessing; the hot
path underneath is the device-resident para_update (model.py).
"""
from __future__ import annotations

import math
from collections import namedtuple
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np

from . import native
from ._lib import AceError
from .model import BatchModel, KernelClass_Matern32_R6, KernelClass_SE_R6, set_optimizer


# --------------------------------------------------------------------------
# Basis classes
# --------------------------------------------------------------------------
class linear_spline:
    """R/spline_linear_R6.R"""

    def __init__(self):
        self.B = self.dB = None

    def dim(self):
        return self.B.shape[1] + 1

    def trainbasis(self, Z, n_knots, verbose=False):
        if verbose:
            print("Using binary/linear-basis")
        n = np.asarray(Z).size
        self.B = np.asfortranarray(np.asarray(Z, dtype=np.float64).reshape(n, 1))
        self.dB = np.ones((n, 1), order="F")
        return self.B

    def testbasis(self, Znew=None):
        if Znew is not None:
            z = np.ravel(np.asarray(Znew, dtype=np.float64))
            return {"B": z.reshape(-1, 1).copy(order="F"), "dB": np.ones((z.size, 1), order="F")}
        return {"B": self.B.copy(order="F"), "dB": self.dB.copy(order="F")}


class square_spline:
    """R/spline_square_R6.R"""

    def __init__(self):
        self.B = self.dB = None

    def dim(self):
        return self.B.shape[1] + 1

    def trainbasis(self, Z, n_knots, verbose=False):
        if verbose:
            print("Using square-basis")
        z = np.ravel(np.asarray(Z, dtype=np.float64))
        self.B = np.asfortranarray(np.column_stack([z, z ** 2]))
        self.dB = np.asfortranarray(np.column_stack([np.ones_like(z), 2 * z]))
        return self.B

    def testbasis(self, Znew=None):
        if Znew is not None:
            z = np.ravel(np.asarray(Znew, dtype=np.float64))
            return {"B": np.asfortranarray(np.column_stack([z, z ** 2])),
                    "dB": np.asfortranarray(np.column_stack([np.ones_like(z), 2 * z]))}
        return {"B": self.B, "dB": self.dB}


class ns_spline:
    """R/spline_ns_R6.R: internal knots at type-7 quantiles, boundary (-1, 1)."""

    def __init__(self):
        self.B = self.dB = self.myknots = None

    def dim(self):
        return self.B.shape[1] + 1

    def trainbasis(self, Z, n_knots, verbose=False):
        if verbose:
            print("Using natural cubic-spline")
        z = np.ravel(np.asarray(Z, dtype=np.float64))
        if n_knots > 0:
            ik = np.quantile(z, np.arange(1, n_knots + 1) / (n_knots + 1), method="linear")
        else:
            ik = np.array([])
        self.myknots = np.concatenate([ik, [-1.0, 1.0]])
        self.B = native.ncs_basis(z, self.myknots)
        self.dB = native.ncs_basis_deriv(z, self.myknots)
        return self.B

    def testbasis(self, Znew=None):
        if Znew is not None:
            return {"B": native.ncs_basis(Znew, self.myknots),
                    "dB": native.ncs_basis_deriv(Znew, self.myknots)}
        return {"B": self.B, "dB": self.dB}


def set_basis(basis, isuniv):
    """R/utilities.R:23-30.  "B" (splines2::bSpline) is not available here."""
    if basis in ("binary", "linear"):
        return linear_spline()
    if isuniv and basis == "B":
        raise AceError("basis 'B' needs splines2::bSpline (not available); use 'ns'")
    if isuniv and basis == "square":
        return square_spline()
    if isuniv:
        return ns_spline()  # "cubic", "ns" and anything else
    raise AceError("multivariate Z is not supported by the reference either")


def set_initial_parameters(p, B, n, y, X, Z, init_sigma=None, init_length_scale=20.0,
                           verbose=False):
    """R/parameters.R:1-23.  ace.train always passes init.sigma, so the OLS
    residual variance of y on [X, Z, 1] is always used (see oracle notes)."""
    Xm = np.column_stack([X, Z, np.ones(n)])
    Q, R = np.linalg.qr(Xm)
    rank = int(np.sum(np.abs(np.diag(R)) > 1e-7 * np.abs(R).max()))
    Q = Q[:, :rank]
    yv = np.ravel(y)
    init_sigma = math.log(float(yv @ (yv - Q @ (Q.T @ yv))) / (n - 1))
    if verbose:
        print("Initial noise variance: ", math.exp(init_sigma))
    return np.concatenate([[init_sigma, 0.0], -np.log(np.ones(B)),
                           np.log(np.full(B * p, init_length_scale))])


class AceFit(dict):
    """The S3 "ace" list (R/main_ace.R:242-253)."""


def _make_fit(myKernel, q, settings, bias_corrected, init_length_scale, convergence, stats):
    """The fit of one prepared dataset q (_prepare) from its trained kernel
    object; settings = (optimizer, learning_rate, momentum, beta1, beta2),
    stats the 2 x iterations table of the iterations that ran."""
    return AceFit(Kernel=myKernel, Basis=q.basis,
                  OptimSettings=dict(zip(("optim", "lr", "momentum", "beta1", "beta2"), settings)),
                  moments=q.moments,
                  train_data={"y": q.y, "X": q.X, "Z": q.Z, "Zbinary": q.isbinary},
                  train_stats={"RIC_bias_corrected": bias_corrected,
                               "init.length_scale": init_length_scale,
                               "convergence": convergence, "final_evidence": stats[1, -1],
                               "stats": stats})


def _view(fit):
    """What the queries on a fit read from it, unpacked once."""
    td, mom = fit["train_data"], fit["moments"]
    px, pz = td["X"].shape[1], td["Z"].shape[1]
    return SimpleNamespace(K=fit["Kernel"], basis=fit["Basis"], Btr=fit["Basis"].B, y=td["y"],
                           X=td["X"], Z=td["Z"], mom=mom, px=px, pz=pz, mean_y=mom[0, 0],
                           std_y=mom[0, 1], std_Z=mom[1 + px:1 + px + pz, 1],
                           binary=bool(np.all(td["Zbinary"])))


_Prepared = namedtuple("_Prepared", "y X Z px moments isbinary basis theta0")


def _prepare(y, X, Z, pi, basis, n_knots, init_sigma, init_length_scale, verbose):
    """ace.train's host preprocessing (R/main_ace.R:146-211): normalisation,
    the basis and the initial parameters of one dataset."""
    yv = np.array(np.ravel(y), dtype=np.float64)
    n = yv.shape[0]
    Xi = np.array(X, dtype=np.float64, order="F", copy=True)
    if Xi.ndim == 1:
        Xi = Xi.reshape(n, 1, order="F")
    px = Xi.shape[1]
    Zi = np.array(Z, dtype=np.float64, order="F", copy=True)
    if Zi.ndim == 1:
        Zi = Zi.reshape(n, 1, order="F")
    pz = Zi.shape[1]
    if Xi.shape != (n, px):
        raise AceError("Dimension of X not correct.")
    if Zi.shape != (n, pz):
        raise AceError("Dimension of Z not correct.")
    moments = native.normalize_train(yv, Xi, Zi)
    isuniv = pz == 1
    isbinary = moments[1 + px:1 + px + pz, 2] == 1
    if np.all(isbinary):
        if verbose:
            print("Assuming binary Z")
        if pi is None:
            basis = "binary"
    elif verbose:
        print("Non-Binary Z detected")
    if pi is not None and isuniv:
        pint = np.ravel(np.asarray(pi, dtype=np.float64)).reshape(n, 1)
        if not isbinary[0]:
            pint = (pint - moments[1 + px, 0]) / moments[1 + px, 1]
        Zi = np.asfortranarray(Zi - pint)
    myBasis = set_basis(basis, isuniv)
    myBasis.trainbasis(Zi, n_knots, verbose)
    theta0 = set_initial_parameters(px, myBasis.dim(), n, yv, Xi, Zi, init_sigma,
                                    init_length_scale, verbose)
    return _Prepared(yv, Xi, Zi, px, moments, isbinary, myBasis, theta0)


def ace_train(y, X, Z, pi=None, kernel="SE", basis="linear", n_knots=1, optimizer="Nadam",
              maxiter=1000, tol=1e-4, learning_rate=0.01, beta1=0.9, beta2=0.999, momentum=0.0,
              norm_clip=None, clip_at=1.0, init_sigma=None, init_length_scale=20.0,
              plot_stats=False, verbose=True, ctx=None, native_loop=False):
    """R/main_ace.R:132-254 (ace.train).  native_loop=True runs the optimisation
    loop inside the library (ace_model_train: no per-iteration round trip
    through Python; same arithmetic, so the same trajectory)."""
    if norm_clip is None:
        norm_clip = optimizer in ("Adam", "Nadam")  # R/main_ace.R:143 (Q5)
    q = _prepare(y, X, Z, pi, basis, n_knots, init_sigma, init_length_scale, verbose)
    yv, Xi, myBasis = q.y, q.X, q.basis
    Kc = KernelClass_Matern32_R6 if kernel == "Matern32" else KernelClass_SE_R6
    myKernel = Kc(q.px, myBasis.dim(), q.theta0, q.moments[0, 1], verbose, ctx=ctx)
    myOptimizer = set_optimizer(optimizer, myKernel, learning_rate, momentum, beta1, beta2,
                                norm_clip, clip_at)
    if native_loop:
        model = myKernel._ensure_model(yv, Xi, myBasis.B)
        theta = np.ascontiguousarray(myKernel.parameters, dtype=np.float64)
        stats, it, convergence = model.train(theta, optimizer, learning_rate, momentum, beta1,
                                             beta2, norm_clip, clip_at, maxiter, tol)
        myKernel.parameters = theta
        myKernel._mark_kernel(Xi, myBasis.B)
        myKernel._inv = None
        myKernel._inv_from_model = True
    else:
        stats = np.zeros((2, maxiter + 2))
        it = 0
        for it in range(1, maxiter + 1):
            stats[:, it] = myKernel.para_update(it, yv, Xi, myBasis.B, myOptimizer,
                                                verbose=verbose)
            change = abs(stats[1, it] - stats[1, it - 1])
            if change < tol and it > 3:
                if verbose:
                    print(f"Stopped: change smaller than tolerance after {it} iterations")
                break
        convergence = it < maxiter
        stats[:, it + 1] = myKernel.get_train_stats(yv, Xi, myBasis.B)
        if verbose and not convergence:
            print("WARNING NO CONVERGENCE - Optimization stopped: maximum iterations reached")
    if verbose:
        print("Final training log Evidence: ", stats[1, it + 1])
    return _make_fit(myKernel, q, (optimizer, learning_rate, momentum, beta1, beta2),
                     pi is not None, init_length_scale, convergence, stats[:, 2:it + 2])


BATCH_NMAX = 512  # rows of the largest model the batched engine takes


def _check_nmax(noun, j, n, instead):
    if n > BATCH_NMAX:
        raise AceError(f"{noun} {j}: n = {n} > {BATCH_NMAX}, the batched engine's limit (use "
                       f"{instead})")


def _batch(noun, items, ctx, instead=None):
    """The batch of `items`, one (kernel, p, B, y, X, basis, std_y) per model.
    Checked at once, before a GPU is touched: the models agree in kernel, p
    and B and, with `instead` (the unbatched function to name), fit in the
    engine; `noun` names them in the errors.  Returns a context manager:
    entering it gives a BatchModel that holds every model's training data,
    leaving it closes that."""
    k0, p0, B0 = items[0][:3]
    for j, (k, p, B, y, *_) in enumerate(items):
        if k != k0:
            raise AceError(f"{noun} {j} uses kernel {k}, {noun} 0 {k0}: the {noun}s of a "
                           "batch must use one kernel")
        if p != p0:
            raise AceError(f"{noun} {j} has p = {p}, {noun} 0 has p = {p0}")
        if B != B0:
            raise AceError(f"{noun} {j} has basis dimension B = {B}, {noun} 0 has B = {B0}")
        if instead:
            _check_nmax(noun, j, y.size, instead)

    @contextmanager
    def opened():
        bm = BatchModel(k0, len(items), max(it[3].size for it in items), p0, B0, ctx=ctx)
        try:
            for j, (_k, _p, _B, y, X, basis, std_y) in enumerate(items):
                bm.set_data(j, y, X, basis, std_y)
            yield bm
        finally:
            bm.close()
    return opened()


def ace_train_batch(ys, Xs, Zs, pis=None, kernel="SE", basis="linear", n_knots=1,
                    optimizer="Nadam", maxiter=1000, tol=1e-4, learning_rate=0.01, beta1=0.9,
                    beta2=0.999, momentum=0.0, norm_clip=None, clip_at=1.0, init_sigma=None,
                    init_length_scale=20.0, verbose=False, ctx=None, nonfinite="raise"):
    """ace_train of M small datasets (n <= 512 each) in one ace_batch_train
    call: one workgroup per model on one GPU.  ys, Xs, Zs (and pis) are
    sequences of length M; init_length_scale and init_sigma may be sequences
    of length M (multi-start: pass the same dataset M times).  The datasets
    must agree in p and in the basis dimension B.  Returns a list of AceFit;
    each carries its model's inverse of the last para_update on the host
    (Q6), so predict_ace runs through the host-buffer path; predict_ace_batch
    predicts for all of them in one batched call.  A model whose
    gradient becomes non-finite stops alone: nonfinite="raise" then raises
    AceError naming the models (ace_train's behaviour), nonfinite="none" puts
    None in their places and returns the other fits."""
    M = len(ys)
    if M < 1 or len(Xs) != M or len(Zs) != M or (pis is not None and len(pis) != M):
        raise AceError("ys, Xs, Zs (and pis) must be sequences of one length M >= 1")
    if isinstance(kernel, (list, tuple)):  # one kernel per dataset: they must agree
        if len(kernel) != M or len(set(kernel)) != 1:
            raise AceError("the datasets of a batch must use one kernel")
        kernel = kernel[0]
    if kernel not in ("SE", "Matern32"):
        raise AceError(f"unknown kernel {kernel!r}")
    if norm_clip is None:
        norm_clip = optimizer in ("Adam", "Nadam")
    if nonfinite not in ("raise", "none"):
        raise AceError('nonfinite must be "raise" or "none"')

    def per_model(v, j):
        return v[j] if isinstance(v, (list, tuple, np.ndarray)) else v

    for j in range(M):
        _check_nmax("dataset", j, np.size(ys[j]), "ace_train")
    for v in (init_length_scale, init_sigma):
        if isinstance(v, (list, tuple, np.ndarray)) and len(v) != M:
            raise AceError("init_length_scale / init_sigma sequences must have length M")
    prep = [_prepare(ys[j], Xs[j], Zs[j], None if pis is None else pis[j], basis, n_knots,
                     per_model(init_sigma, j), per_model(init_length_scale, j), verbose)
            for j in range(M)]
    px, B = prep[0].px, prep[0].basis.dim()
    with _batch("dataset", [(kernel, q.px, q.basis.dim(), q.y, q.X, q.basis.B, q.moments[0, 1])
                            for q in prep], ctx) as bm:
        theta = np.asfortranarray(np.column_stack([q.theta0 for q in prep]))
        stats, its, conv, status = bm.train(theta, optimizer, learning_rate, momentum, beta1,
                                            beta2, norm_clip, clip_at, maxiter, tol)
        bad = [j for j in range(M) if status[j] != 0]
        if bad and nonfinite != "none":
            raise AceError(f"ACE_ERR_NONFINITE: models {bad}: Some gradients are not finite, "
                           "NaN, or NA. Often this is due to too large learning rates.")
        invs = [None if j in bad else bm.inverse(j) for j in range(M)]
    Kc = KernelClass_Matern32_R6 if kernel == "Matern32" else KernelClass_SE_R6
    fits = []
    for j, q in enumerate(prep):
        if invs[j] is None:
            fits.append(None)
            continue
        myKernel = Kc(px, B, theta[:, j].copy(), q.moments[0, 1], False, ctx=ctx)
        myKernel._mark_kernel(q.X, q.basis.B)
        myKernel._inv = invs[j]
        myKernel._inv_from_model = False
        fits.append(_make_fit(myKernel, q, (optimizer, learning_rate, momentum, beta1, beta2),
                              pis is not None and pis[j] is not None,
                              per_model(init_length_scale, j), bool(conv[j]),
                              stats[:, 2:int(its[j]) + 2, j]))
    return fits


def _new_X(v, newX, Zn=None, normalize=True, check=True):
    """Raw test rows newX as the fit (view v) takes them: a column-major
    copy, its width checked against the training X, normalised with the fit's
    moments -- together with the treatment column Zn(nx) of the same points
    (a function of their number; normalised with them), else on its own.
    Returns (Xn, Zn)."""
    Xn = np.array(newX, dtype=np.float64, order="F", copy=True)
    if check and (Xn.ndim != 2 or Xn.shape[1] != v.px):
        raise AceError("Dimension mismatch of X with newX")
    Zn = np.zeros((Xn.shape[0], v.pz), order="F") if Zn is None else Zn(Xn.shape[0])
    if normalize:
        native.normalize_test(Xn, Zn, v.mom)
    return Xn, Zn


def _test_points(v, newX, newZ, normalize):
    """predict.ace's argument handling (R/predict.ace.R:30-80): the normalised
    test points (Xn, Zn) of one fit (view v) for the four newX / newZ cases."""
    def level(n):
        return np.full((n, 1), float(np.ravel(newZ)[0]), order="F")

    if newX is None and newZ is None:
        Xn, Zn = v.X, v.Z
    elif newX is None:
        Xn = np.array(v.X, order="F", copy=True)
        if np.size(newZ) == 1:
            Zn = level(Xn.shape[0])
        else:
            Zn = np.asfortranarray(np.ravel(newZ).astype(np.float64).reshape(-1, 1))
            if normalize:
                native.normalize_test(Xn, Zn, v.mom)
            Xn = v.X
    elif newZ is None:
        Xn, _ = _new_X(v, newX, None, normalize, check=False)
        Zn = np.zeros((Xn.shape[0], 1), order="F")
    elif np.size(newZ) == 1:
        Xn, Zn = _new_X(v, newX, level, normalize)
    else:
        Xn, Zn = _new_X(v, newX, lambda n: np.array(newZ, dtype=np.float64, order="F", copy=True)
                        .reshape(-1, v.pz, order="F"), normalize)
    return Xn, Zn


def predict_ace(obj, newX=None, newZ=None, marginal=False, return_average_treatments=False,
                normalize=True):
    """R/predict.ace.R:30-99 (predict.ace)."""
    v = _view(obj)
    Xn, Zn = _test_points(v, newX, newZ, normalize)
    tb = v.basis.testbasis(Zn)
    if not marginal:
        return v.K.predict(v.y, v.X, v.Btr, Xn, tb["B"], v.mean_y, v.std_y)
    return v.K.predict_marginal(v.y, v.X, v.Btr, Xn, tb["B"], tb["dB"], v.mean_y, v.std_y,
                                v.std_Z, v.binary and return_average_treatments)


def posterior_draws(fit, newX=None, newZ=None, marginal=False, n_draws=1000, seed=0, xi=None,
                    jitter=None, return_average_treatments=False, return_cov=False):
    """Joint posterior draws at the test points of predict_ace(fit, newX, newZ,
    marginal): {"map": (nx), "draws": (nx, S)} with draws = map 1^T + L xi, L
    the Cholesky factor of the posterior covariance of the predictions (the
    noise term included) or, with marginal, of the marginal effects -- what
    simultaneous bands, P(effect > 0 on a subgroup), quantiles and ranks of
    the CATE are computed from.  xi (nx x S standard normals) defaults to
    numpy's default_rng(seed).standard_normal((nx, n_draws)); the device draws
    nothing itself.  jitter (absolute, added to the diagonal before factoring)
    defaults to 0 for the prediction and to 1e-10 mean(diag cov) for the
    marginal, whose covariance has no noise term to keep it definite.
    return_average_treatments with a binary treatment adds "ate", "att",
    "atu" (S each): every draw's mean over all, the treated and the untreated
    test points (NaN for an empty group).  return_cov adds "cov"."""
    v = _view(fit)
    Xn, Zn = _test_points(v, newX, newZ, True)
    tb = v.basis.testbasis(Zn)
    nx = Xn.shape[0]
    if xi is None:
        xi = np.random.default_rng(seed).standard_normal((nx, int(n_draws)))
    xi = np.asfortranarray(np.asarray(xi, dtype=np.float64).reshape(nx, -1))
    if jitter is None:
        jitter = 0.0
        if marginal:
            var = v.K.predict_marginal(v.y, v.X, v.Btr, Xn, tb["B"], tb["dB"], v.mean_y, v.std_y,
                                       v.std_Z, False)["var"]
            jitter = 1e-10 * float(np.mean(var))
    r = v.K.predict_joint(v.y, v.X, v.Btr, Xn, tb["dB"] if marginal else tb["B"], v.mean_y,
                          v.std_y, marginal=marginal, std_Z=v.std_Z, noise=True, jitter=jitter,
                          xi=xi, return_cov=return_cov)
    if r["info"] > 0:
        raise AceError(
            f"posterior_draws: the posterior covariance is not positive definite at pivot "
            f"{r['info']} of {nx} (jitter={jitter:g}). Pass a larger jitter=; note that the "
            "fit's inverse is the last para_update's while the kernels use the final "
            "parameters (Q6), so the matrix need not be positive semidefinite at all")
    out = {"map": r["map"], "draws": r["draws"]}
    if return_cov:
        out["cov"] = r["cov"]
    if return_average_treatments and v.binary:
        D = r["draws"]
        zx = np.ravel(tb["B"]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["ate"] = D.sum(axis=0) / nx
            out["att"] = (zx @ D) / np.sum(zx)
            out["atu"] = ((zx == 0).astype(np.float64) @ D) / np.sum(zx == 0)
    return out


def cross_validate(fit, folds=10, seed=0, groups=None):
    """Cross-validation of a fit without refitting: the held-out prediction of
    every fold from the fit's resident inverse, hyperparameters and mu held
    fixed (Rasmussen & Williams §5.4.2 and its block form; DeviceModel.cv).
    folds: an int K -- the random partition np.array_split(default_rng(seed)
    .permutation(n), K); "loo" -- leave-one-out; or a list of index arrays
    (they may overlap and need not cover the data).  groups (labels per row)
    means leave-one-group-out, one fold per distinct label.
    Returns, for disjoint folds, "map", "var", "ci" (n x 2: map -+ 1.96
    sqrt(var)), "resid" (held-out y - map), "z" = resid / sqrt(var), each of
    length n in original units and NaN where a row is in no fold, and "fold"
    (the fold id per row, -1 if in none); for overlapping folds the same
    arrays packed fold after fold ("off" the offsets, no "fold").  Per fold:
    "lpd" (the joint log predictive density of its held-out rows), "mahal",
    "size", "status"; and "elpd" = sum lpd, "rmse", "coverage" (the share of
    held-out y inside ci).  The inverse is the last para_update's, theta_{T-1}'s,
    while mu is the final one (Q6): the model predict_ace uses in-sample."""
    K, mom = fit["Kernel"], fit["moments"]  # Z is not read: no _view
    y, X = fit["train_data"]["y"], fit["train_data"]["X"]
    n = X.shape[0]
    if groups is not None:
        g = np.ravel(np.asarray(groups))
        if g.size != n:
            raise AceError("groups must have one label per training row")
        fl = [np.flatnonzero(g == u) for u in np.unique(g)]
    elif isinstance(folds, str):
        if folds != "loo":
            raise AceError('folds must be an int, "loo" or a list of index arrays')
        fl = [np.array([i]) for i in range(n)]
    elif np.ndim(folds) == 0:
        k = int(folds)
        if not 2 <= k <= n:
            raise AceError("folds must be between 2 and n")
        fl = np.array_split(np.random.default_rng(seed).permutation(n), k)
    else:
        fl = [np.ravel(np.asarray(f)).astype(np.int64) for f in folds]
    r = K.cross_validate(y, X, fit["Basis"].B, fl, mom[0, 0], mom[0, 1])
    bad = np.flatnonzero(r["status"] != 0)
    if bad.size:
        f = int(bad[0])
        raise AceError(
            f"cross_validate: fold {f} ({fl[f].size} rows) is not positive definite at pivot "
            f"{int(r['status'][f])}: its block of the inverse cannot be conditioned on. Note that "
            "the fit's inverse is the last para_update's (theta_{T-1}'s) while mu is the final "
            "one (Q6)")
    idx = np.concatenate(fl)
    yo = mom[0, 0] + mom[0, 1] * np.ravel(y)[idx]
    sd = np.sqrt(r["var"])
    ci = np.column_stack([r["map"] - 1.96 * sd, r["map"] + 1.96 * sd])
    out = {"lpd": r["lpd"], "mahal": r["mahal"], "size": np.array([f.size for f in fl]),
           "status": r["status"], "elpd": float(np.sum(r["lpd"])),
           "rmse": float(np.sqrt(np.mean(r["resid"] ** 2))),
           "coverage": float(np.mean((yo >= ci[:, 0]) & (yo <= ci[:, 1])))}
    packed = {"map": r["map"], "var": r["var"], "ci": ci, "resid": r["resid"],
              "z": r["resid"] / sd}
    if np.unique(idx).size != idx.size:  # overlapping folds: packed fold after fold
        out.update(packed, off=r["off"])
        return out
    for k, a in packed.items():
        full = np.full((n,) + a.shape[1:], np.nan)
        full[idx] = a
        out[k] = full
    fid = np.full(n, -1, dtype=np.int64)
    fid[idx] = np.repeat(np.arange(len(fl)), [f.size for f in fl])
    out["fold"] = fid
    return out


def predict_ace_batch(fits, newXs=None, newZs=None, marginal=False,
                      return_average_treatments=False, normalize=True):
    """predict_ace of M fits of small models (n <= 512 each, one kernel, p and
    B) in one batched call: what [predict_ace(f, newX_j, newZ_j, ...) for f in
    fits] returns, with one workgroup per fit on one GPU
    (BatchModel.predict / predict_marginal).  newXs / newZs: None, or
    sequences of length M whose entries are what predict_ace takes (None
    included).  The fits may come from ace_train_batch or from ace_train; each
    one's inverse of its last para_update (Q6) is installed next to its
    training data, and the kernels are evaluated at its final parameters."""
    fits = list(fits)
    M = len(fits)
    if M < 1:
        raise AceError("fits must hold at least one fit")
    if any(f is None for f in fits):
        bad = [j for j, f in enumerate(fits) if f is None]
        raise AceError(f"fits {bad} are None (models that ace_train_batch could not fit)")
    if newZs is not None and not isinstance(newZs, (list, tuple)) and np.size(newZs) == 1:
        newZs = [newZs] * M  # one treatment value for every test point of every fit
    for name, v in (("newXs", newXs), ("newZs", newZs)):
        if v is not None and (not isinstance(v, (list, tuple)) or len(v) != M):
            raise AceError(f"{name} must be None or a sequence of length M = {M}")
    vs = [_view(f) for f in fits]
    batch = _batch("fit", [(v.K.kernel, v.K.p, v.K.B, v.y, v.X, v.Btr, v.std_y) for v in vs],
                   vs[0].K.ctx, instead="predict_ace")
    pts = [_test_points(v, None if newXs is None else newXs[j],
                        None if newZs is None else newZs[j], normalize)
           for j, v in enumerate(vs)]
    tbs = [v.basis.testbasis(Zn) for v, (_, Zn) in zip(vs, pts)]
    theta = np.asfortranarray(np.column_stack([v.K.parameters for v in vs]))
    with batch as bm:
        for j, v in enumerate(vs):
            bm.set_inverse(j, v.K.invKmatn)
        Xns = [q[0] for q in pts]
        if not marginal:
            return bm.predict(theta, Xns, [t["B"] for t in tbs], [v.mean_y for v in vs],
                              [v.std_y for v in vs])
        ate = [v.binary and return_average_treatments for v in vs]
        if any(ate) != all(ate):
            raise AceError("return_average_treatments needs a binary treatment in every fit of "
                           "the batch, or in none")
        return bm.predict_marginal(theta, Xns, [t["dB"] for t in tbs], [t["B"] for t in tbs],
                                   [v.std_y for v in vs], [np.ravel(v.std_Z)[0] for v in vs],
                                   ate[0])


def robust_treatment(obj, newX=None, n_steps=5):
    """R/robust_treatment.R:67-128 without the plots: ATE (in-sample also ATT
    and ATU) while the points with the largest posterior variance of the
    marginal effect are discarded, n_steps + 1 nested subsets cut at the
    type-7 quantiles of that variance.  In-sample (newX None) the training X
    and Z are the test points (the reference's normalize=FALSE calls);
    out-of-sample newX is taken with newZ = 1.  One marginal pass and one
    grouped pass on the device replace the reference's n_steps + 2
    predictions.  Returns {"idx": n_pred x (n_steps + 1) bool (the reference's
    return value), "ate": its ate_results table (map, ci0, ci1, var, retained;
    in-sample also treated, untreated), "thresholds"} and in-sample "att" /
    "atu" (map, ci0, ci1, var; NaN rows where the group is empty)."""
    v = _view(obj)
    if not v.binary:
        raise AceError("Average treatment effect requires binary treatment indicator.")
    insample = newX is None
    if insample:
        Xn, Zn = v.X, v.Z
    else:
        Xn, Zn = _new_X(v, newX, lambda n: np.full((n, 1), 1.0, order="F"))  # newZ = 1
    tb = v.basis.testbasis(Zn)
    r = v.K.robust_treatment(v.y, v.X, v.Btr, Xn, tb["B"], tb["dB"], v.std_y, v.std_Z, n_steps)
    T = int(n_steps) + 1
    avg, counts = r["avg"], r["counts"]
    out = {"idx": r["level"][:, None] <= np.arange(T)[None, :], "thresholds": r["thresholds"]}
    ate = np.full((T, 5 + 2 * insample), np.nan)
    ate[:, :4] = avg[0:4].T
    ate[:, 4] = counts[0]
    out["ate"] = ate
    if insample:
        ate[:, 5] = counts[1]
        ate[:, 6] = counts[2]
        for j, key in ((1, "att"), (2, "atu")):
            tab = np.full((T, 4), np.nan)
            keep = counts[j] > 0
            tab[keep] = avg[4 * j:4 * j + 4].T[keep]
            out[key] = tab
    return out


def _surface_points(v, newX, newZ=None):
    """newX (nx raw rows) and newZ (nz raw treatment values) normalised with
    the fit's moments as predict_ace normalises them, each on its own."""
    Xn = v.X if newX is None else _new_X(v, newX)[0]
    if newZ is None:
        return Xn, None
    Zn = np.array(np.ravel(newZ), dtype=np.float64).reshape(-1, v.pz, order="F")
    Zn = np.asfortranarray(Zn)
    native.normalize_test(np.zeros((Zn.shape[0], v.px), order="F"), Zn, v.mom)
    return Xn, Zn


def coef_posterior(obj, newX=None):
    """Posterior of the coefficient functions g_b(x) of the fit at the rows
    of newX (raw units; None: the training points): {"mean": (nx, B), "cov":
    (nx, B, B)} in normalised-y units, without mu and the noise term."""
    v = _view(obj)
    Xn, _ = _surface_points(v, newX)
    return v.K.coef_posterior(v.y, v.X, v.Btr, Xn)


def response_surface(obj, newX, newZ, marginal=False):
    """predict_ace on the grid of every row of newX (nx raw rows) with every
    treatment value of newZ (nz raw values), what plot_ace computes for its
    curves and surfaces (R/plot_ace.R:146-154, 288, 350-351), from one
    coefficient pass: {"map": (nx, nz), "ci": (nx, nz, 2), "var": (nx, nz)};
    raveled in Fortran order the first two axes are expand.grid(X, Z)."""
    v = _view(obj)
    Xn, Zn = _surface_points(v, newX, newZ)
    tb = v.basis.testbasis(Zn)
    return v.K.predict_surface(v.y, v.X, v.Btr, Xn, tb["dB"] if marginal else tb["B"], marginal,
                               v.mean_y, v.std_y, v.std_Z)


def _group_labels(nx, groups):
    """(distinct labels in np.unique order, int32 label per row) of `groups`
    (one entry per row; None: one group of all rows)."""
    if groups is None:
        return np.array([0]), np.zeros(nx, dtype=np.int32)
    g = np.ravel(np.asarray(groups))
    if g.size != nx:
        raise AceError("groups must have one entry per row of newX (the training rows if None)")
    names, lab = np.unique(g, return_inverse=True)
    if names.size > 64:
        raise AceError(f"groups has {names.size} distinct labels; at most 64 are supported")
    return names, np.ravel(lab).astype(np.int32)


def average_coef_posterior(obj, newX=None, groups=None):
    """Posterior of the group averages (1/|g|) sum_{c in g} g(x_c) of the
    coefficient functions over the rows of newX (raw units; None: the training
    points).  groups: one label per row (None: one group of all rows).
    Returns {"groups": the distinct labels in np.unique order, "count": (G,),
    "mean": (G, B), "cov": (G, B, G, B)}, averages in normalised-y units,
    without mu and the noise term; cov[g, :, h, :] is the covariance between
    two groups' averages, so contrasts of groups need no second pass."""
    v = _view(obj)
    Xn, _ = _surface_points(v, newX)
    names, lab = _group_labels(Xn.shape[0], groups)
    r = v.K.coef_groups(v.y, v.X, v.Btr, Xn, names.size, lab)
    cnt = r["gcount"].astype(np.float64)
    return {"groups": names, "count": r["gcount"], "mean": r["gmean"] / cnt[:, None],
            "cov": r["gcov"] / (cnt[:, None, None, None] * cnt[None, None, :, None])}


def average_response(obj, newZ, newX=None, groups=None, marginal=False, return_cov=False):
    """The average dose-response curve z -> (1/|g|) sum_{c in g} E[y | x_c, z]
    of every group of rows of newX (raw units; None: the training points) at
    the nz raw treatment values newZ, with its credible band; marginal: the
    average derivative curve (for a binary fit ATE / ATT / ATU with groups
    None / the treatment).  One grouped coefficient pass, whatever nz.
    Returns {"groups", "count", "map": (G, nz), "var": (G, nz), "ci":
    (G, nz, 2)} and, with return_cov, "cov" (G, nz, nz) for simultaneous
    bands over z.  No noise term: the posterior of the averaged mean
    function, not of averaged observations."""
    v = _view(obj)
    Xn, Zn = _surface_points(v, newX, newZ)
    names, lab = _group_labels(Xn.shape[0], groups)
    tb = v.basis.testbasis(Zn)
    r = v.K.average_response(v.y, v.X, v.Btr, Xn, names.size, lab,
                             tb["dB"] if marginal else tb["B"], marginal, v.mean_y, v.std_y,
                             v.std_Z, return_cov)
    r["groups"] = names
    r["count"] = np.bincount(lab, minlength=names.size).astype(np.int64)
    return r

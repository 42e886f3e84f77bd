"""The reference's `.Call` surface (R/RcppExports.R:4-78), same names and
argument order, implemented over the C ABI (include/ace_hip.h).

Return values mirror the Rcpp lists (`dict` with the same keys); arguments
the reference takes by non-const reference (`stats` in grad_*_cpp, m/v/nu/
para in the optimizers, grads in norm_clip_cpp, y/X/Z in normalize_*) are
mutated in place, so they must be writable float64 numpy arrays.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import KIND, AceError, check, default_context, fmat, lib, ptr
from ._marshal import ate_dicts, i32ptr, iptr, map_ci_var, pack_folds, scalar, u32ptr, vec


def _ctx(ctx):
    return (ctx or default_context()).handle


# ---------------------------------------------------------------- device handles
class DMat:
    """An ace_dmat handle: a device-resident matrix / cube, or a virtual
    `elements` cube (X, Z, theta recorded; values assembled only if read).
    What the R shim wraps in an ALTREP vector: reading it (np.asarray, or
    any numpy use) materialises it, passing it back to a *_cpp routine does
    not (include/ace_hip.h "device-matrix handles")."""

    def __init__(self, handle, ctx):
        # the Context is kept alive until the handle is freed: ace_dmat_free
        # returns sweep buffers to the context's pool
        self._owner = ctx or default_context()
        self.handle, self.ctx = handle, self._owner.handle
        r, c, sl = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(lib().ace_dmat_dims(handle, ctypes.byref(r), ctypes.byref(c), ctypes.byref(sl)))
        self.shape = (r.value, c.value) if sl.value == 1 else (r.value, c.value, sl.value)

    @classmethod
    def upload(cls, a, ctx=None):
        a = np.asarray(a, dtype=np.float64)
        dims = a.shape + (1,) * (3 - a.ndim)
        af = np.asfortranarray(a)
        h = ctypes.c_void_p()
        check(lib().ace_dmat_upload(_ctx(ctx), dims[0], dims[1], dims[2], ptr(af),
                                    ctypes.byref(h)), _ctx(ctx))
        return cls(h, ctx)

    def read(self):
        out = np.empty(self.shape, order="F")
        check(lib().ace_dmat_read(self.handle, 0, out.size, ptr(out)), self.ctx)
        return out

    def read_region(self, offset, count):
        """`count` values from column-major index `offset` on (the R shim's
        ALTREP Elt / Get_region reads); count = 0 is allowed."""
        out = np.empty(max(int(count), 0))
        buf = out if out.size else np.empty(1)  # a valid pointer for count <= 0
        check(lib().ace_dmat_read(self.handle, int(offset), int(count), ptr(buf)), self.ctx)
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.read()
        return a if dtype is None else a.astype(dtype)

    @property
    def on_device(self):
        return bool(lib().ace_dmat_materialized(self.handle) & 1)

    @property
    def read_to_host(self):
        return bool(lib().ace_dmat_materialized(self.handle) & 2)

    def __del__(self):
        try:
            # a context closed first took its handles' memory with it
            if getattr(self, "handle", None) and self._owner.handle:
                lib().ace_dmat_free(self.handle)
                self.handle = None
        except Exception:
            pass


def _dmat(a, ctx, keep):
    """A handle for a matrix argument: DMat as is, a host array uploaded (the
    R shim does the same for a plain R matrix); `keep` holds temporaries."""
    if isinstance(a, DMat):
        return a.handle
    d = DMat.upload(a, ctx)
    keep.append(d)
    return d.handle


def _any_dev(*xs):
    return any(isinstance(x, DMat) for x in xs)


def _mat_args(ms, ctx):
    """The matrix arguments `ms` (None passes through) of a routine with a
    host-buffer and a handle entry point: (True, handles, keep) if any is a
    DMat -- the others are uploaded -- else (False, double*s, keep); `keep`
    holds what the arguments point into until the call has returned."""
    keep = []
    if _any_dev(*ms):
        return True, [None if m is None else _dmat(m, ctx, keep) for m in ms], keep
    keep = [None if m is None else fmat(m) for m in ms]
    return False, [ptr(f) for f in keep], keep


def _shape(a):
    return a.shape if isinstance(a, DMat) else np.shape(a)  # np.shape would read a DMat


def _zmat(Z, n):
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 1:
        Z = Z.reshape(n, 1)
    return np.asfortranarray(Z)


def _check_theta(theta, B, p, grad=False):
    """The kernel reads theta up to P - 2 (P = 2 + B (p + 1)), so the kernmat_*
    routines accept P - 1 entries like the reference's; the gradient also
    reads the last, gradient-indexed length scale (Q1) and needs all P."""
    need = 2 + B * (p + 1) - (0 if grad else 1)
    if theta.shape[0] < need:
        raise AceError(f"parameters too short for B={B} and p={p}: {theta.shape[0]} < {need}")


# ---------------------------------------------------------------- kernels
def _kernmat_cross(kind, X1, X2, Z1, Z2, parameters, ctx=None, elements=True, device=False):
    X1 = fmat(X1)
    X2 = fmat(X2)
    n1, n2, p = X1.shape[0], X2.shape[0], X2.shape[1]
    Z1 = _zmat(Z1, n1)
    Z2 = _zmat(Z2, n2)
    B = Z1.shape[1] + 1
    th = vec(parameters)
    _check_theta(th, B, p)
    if device:
        hf, he = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().ace_kernmat_cross_dev(_ctx(ctx), kind, n1, n2, p, B, ptr(X1), ptr(X2), ptr(Z1),
                                          ptr(Z2), ptr(th), ctypes.byref(hf), ctypes.byref(he)),
              _ctx(ctx))
        return {"full": DMat(hf, ctx), "elements": DMat(he, ctx)}
    full = np.empty((n1, n2), order="F")
    el = np.empty((n1, n2, B), order="F") if elements else None
    check(lib().ace_kernmat_cross(_ctx(ctx), kind, n1, n2, p, B, ptr(X1), ptr(X2), ptr(Z1),
                                  ptr(Z2), ptr(th), ptr(full), ptr(el)), _ctx(ctx))
    return {"full": full, "elements": el}


def _kernmat_sym(kind, X, Z, parameters, ctx=None, elements=True, device=False):
    X = fmat(X)
    n, p = X.shape
    Z = _zmat(Z, n)
    B = Z.shape[1] + 1
    th = vec(parameters)
    _check_theta(th, B, p)
    if device:
        hf, he = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().ace_kernmat_sym_dev(_ctx(ctx), kind, n, p, B, ptr(X), ptr(Z), ptr(th),
                                        ctypes.byref(hf), ctypes.byref(he)), _ctx(ctx))
        return {"full": DMat(hf, ctx), "elements": DMat(he, ctx)}
    full = np.empty((n, n), order="F")
    el = np.empty((n, n, B), order="F") if elements else None
    check(lib().ace_kernmat_sym(_ctx(ctx), kind, n, p, B, ptr(X), ptr(Z), ptr(th), ptr(full),
                                ptr(el)), _ctx(ctx))
    return {"full": full, "elements": el}


def kernmat_SE_cpp(X1, X2, Z1, Z2, parameters, ctx=None, device=False):
    """src/kernel_SE_cpp.cpp:9-64"""
    return _kernmat_cross(KIND["SE"], X1, X2, Z1, Z2, parameters, ctx, device=device)


def kernmat_SE_symmetric_cpp(X, Z, parameters, ctx=None, device=False):
    """src/kernel_SE_cpp.cpp:67-134"""
    return _kernmat_sym(KIND["SE"], X, Z, parameters, ctx, device=device)


def kernmat_Matern32_cpp(X1, X2, Z1, Z2, parameters, ctx=None, device=False):
    """src/kernel_Matern_cpp.cpp:52-93"""
    return _kernmat_cross(KIND["Matern32"], X1, X2, Z1, Z2, parameters, ctx, device=device)


def kernmat_Matern32_symmetric_cpp(X, Z, parameters, ctx=None, device=False):
    """src/kernel_Matern_cpp.cpp:190-240"""
    return _kernmat_sym(KIND["Matern32"], X, Z, parameters, ctx, device=device)


def invkernel_cpp(pdmat, sigma, ctx=None):
    """src/kernel_SE_cpp.cpp:137-157.  `eigenval` holds the elimination
    pivots (sum(log(.)) == log det, the only use the reference makes of it)."""
    sig = scalar(sigma)
    dev = _any_dev(pdmat)
    K = pdmat if dev else fmat(pdmat)
    n = K.shape[0]
    if not dev and K.shape != (n, n):
        raise AceError("pdmat must be square")
    ev = np.empty(n)
    if dev:  # handle in, handle out: the inverse stays in HBM
        h = ctypes.c_void_p()
        check(lib().ace_invkernel_dev(_ctx(ctx), K.handle, sig, ptr(ev), ctypes.byref(h)),
              _ctx(ctx))
        inv = DMat(h, ctx)
    else:
        inv = np.empty((n, n), order="F")
        check(lib().ace_invkernel(_ctx(ctx), n, ptr(K), sig, ptr(ev), ptr(inv)), _ctx(ctx))
    return {"eigenval": ev, "inv": inv}


def _grad(kind, y, X, Z, Kfull, K, invKmatn, eigenval, parameters, stats, B, std_y, ctx):
    X = fmat(X)
    n, p = X.shape
    Z = _zmat(Z, n)
    if Z.shape[1] + 1 != B:
        raise AceError("B != ncol(Z) + 1")
    yv = vec(y)
    th = vec(parameters)
    _check_theta(th, B, p, grad=True)
    ev = vec(eigenval)
    if not (isinstance(stats, np.ndarray) and stats.dtype == np.float64 and stats.size >= 2):
        raise AceError("stats must be a float64 numpy array of length 2 (mutated in place)")
    st = np.ascontiguousarray(stats)
    g = np.empty(th.shape[0])
    dev, mats, _keep = _mat_args((Kfull, K, invKmatn), ctx)
    fn = lib().ace_grad_dev if dev else lib().ace_grad
    check(fn(_ctx(ctx), kind, n, p, B, ptr(yv), ptr(X), ptr(Z), *mats, ptr(ev), ptr(th), ptr(st),
             float(std_y), ptr(g)), _ctx(ctx))
    stats.flat[0:2] = st.flat[0:2]
    return g


def grad_SE_cpp(y, X, Z, Kfull, K, invKmatn, eigenval, parameters, stats, B, std_y, ctx=None):
    """src/kernel_SE_cpp.cpp:192-243 (stats written in place)."""
    return _grad(KIND["SE"], y, X, Z, Kfull, K, invKmatn, eigenval, parameters, stats, B,
                 std_y, ctx)


def grad_Matern_cpp(y, X, Z, Kfull, K, invKmatn, eigenval, parameters, stats, B, std_y,
                    ctx=None):
    """src/kernel_Matern_cpp.cpp:420-467 (stats written in place)."""
    return _grad(KIND["Matern32"], y, X, Z, Kfull, K, invKmatn, eigenval, parameters, stats, B,
                 std_y, ctx)


def stats_cpp(y, Kmat, invKmatn, eigenval, mu, std_y=1.0, ctx=None):
    """src/stats_cpp.cpp:9-32"""
    yv, ev = vec(y), vec(eigenval)
    out = np.empty(2)
    dev, mats, _keep = _mat_args((Kmat, invKmatn), ctx)
    fn = lib().ace_stats_dev if dev else lib().ace_stats
    check(fn(_ctx(ctx), yv.shape[0], ptr(yv), *mats, ptr(ev), scalar(mu), float(std_y),
             ptr(out)), _ctx(ctx))
    return out


def mu_solution_cpp(y, invKmat, ctx=None):
    """src/utilities_cpp.cpp:6-10"""
    yv = vec(y)
    out = ctypes.c_double()
    dev, mats, _keep = _mat_args((invKmat,), ctx)
    fn = lib().ace_mu_solution_dev if dev else lib().ace_mu_solution
    check(fn(_ctx(ctx), yv.shape[0], ptr(yv), *mats, ctypes.byref(out)), _ctx(ctx))
    return out.value


def pred_cpp(y_X, sigma, mu, invK_XX, K_xX, K_xx, mean_y, std_y, ctx=None):
    """src/pred_cpp.cpp:8-34"""
    yv = vec(y_X)
    nx, nX = _shape(K_xX)
    mp, ci, var, out = map_ci_var(nx)
    dev, mats, _keep = _mat_args((invK_XX, K_xX, K_xx), ctx)
    fn = lib().ace_pred_dev if dev else lib().ace_pred
    check(fn(_ctx(ctx), nX, nx, ptr(yv), float(sigma), float(mu), *mats, float(mean_y),
             float(std_y), ptr(mp), ptr(ci), ptr(var)), _ctx(ctx))
    return out


def pred_marginal_cpp(y_X, Z_x, sigma, mu, invK_XX, K_xX, K_xx, mean_y, std_y, std_Z,
                      calculate_ate, ctx=None):
    """src/pred_cpp.cpp:37-126"""
    yv = vec(y_X)
    zx = vec(Z_x) if Z_x is not None else None
    avg = np.empty(12)
    shape = _shape(K_xX)
    nx, nX = shape[:2]
    mp, ci, var, out = map_ci_var(nx)
    dev, mats, _keep = _mat_args((invK_XX, K_xX, K_xx), ctx)
    if dev:  # the handles carry their slice count
        fn, dims = lib().ace_pred_marginal_dev, (nX, nx)
    else:
        fn, dims = lib().ace_pred_marginal, (nX, nx, shape[2])
    check(fn(_ctx(ctx), *dims, ptr(yv), ptr(zx), float(sigma), float(mu), *mats, float(mean_y),
             float(std_y), scalar(std_Z), 1 if calculate_ate else 0, ptr(mp), ptr(ci), ptr(var),
             ptr(avg)), _ctx(ctx))
    if calculate_ate:
        out.update(ate_dicts(avg))
    return out


# ---------------------------------------------------------------- host-only
def _inplace(a, name):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and
            (a.flags.c_contiguous or a.flags.f_contiguous) and a.flags.writeable):
        raise AceError(f"{name} must be a writable contiguous float64 numpy array")
    return a


def _optimizer(entry, hyper, state, grad, para):
    """One optimizer step: `state` ({name: array}) and para in place."""
    g = vec(grad)
    return bool(getattr(lib(), entry)(g.shape[0], *map(float, hyper),
                                      *[ptr(_inplace(a, k)) for k, a in state.items()], ptr(g),
                                      ptr(_inplace(para, "para"))))


def Nesterov_cpp(learn_rate, momentum, nu, grad, para):
    """src/optimizer_cpp.cpp:8-20 (nu, para in place)."""
    return _optimizer("ace_nesterov", (learn_rate, momentum), {"nu": nu}, grad, para)


def Nadam_cpp(iter, learn_rate, beta1, beta2, eps, m, v, grad, para):  # noqa: A002
    """src/optimizer_cpp.cpp:23-42 (m, v, para in place)."""
    return _optimizer("ace_nadam", (iter, learn_rate, beta1, beta2, eps), {"m": m, "v": v}, grad,
                      para)


def Adam_cpp(iter, learn_rate, beta1, beta2, eps, m, v, grad, para):  # noqa: A002
    """src/optimizer_cpp.cpp:45-63 (m, v, para in place)."""
    return _optimizer("ace_adam", (iter, learn_rate, beta1, beta2, eps), {"m": m, "v": v}, grad,
                      para)


def norm_clip_cpp(flag, grads, max_length):
    """src/utilities_cpp.cpp:121-129 (grads in place)."""
    g = _inplace(grads, "grads")
    lib().ace_norm_clip(1 if flag else 0, g.size, ptr(g), float(max_length))


def _ncs(fn, x, knots):
    xv, kv = vec(x), vec(knots)
    nk = np.unique(kv).shape[0]
    out = np.empty((xv.shape[0], nk), order="F")
    ncols = ctypes.c_int64()
    check(fn(xv.shape[0], ptr(xv), kv.shape[0], ptr(kv), ptr(out), ctypes.byref(ncols)))
    return out[:, :ncols.value]


def ncs_basis(x, knots):
    """src/ncs_basis_cpp.cpp:61-79"""
    return _ncs(lib().ace_ncs_basis, x, knots)


def ncs_basis_deriv(x, knots):
    """src/ncs_basis_cpp.cpp:82-99"""
    return _ncs(lib().ace_ncs_basis_deriv, x, knots)


def normalize_train(y, X, Z):
    """src/utilities_cpp.cpp:13-104: y (n), X (n x px), Z (n x pz) in place
    (Fortran-ordered float64); returns the (1+px+pz) x 3 moments."""
    y = _inplace(y, "y")
    X = _inplace(X, "X")
    Z = _inplace(Z, "Z")
    if X.ndim != 2 or Z.ndim != 2 or not X.flags.f_contiguous or not Z.flags.f_contiguous:
        raise AceError("X and Z must be 2-D Fortran-ordered arrays")
    n, px = X.shape
    pz = Z.shape[1]
    mom = np.empty((1 + px + pz, 3), order="F")
    check(lib().ace_normalize_train(n, px, pz, ptr(y), ptr(X), ptr(Z), ptr(mom)))
    return mom


def normalize_test(X, Z, moments):
    """src/utilities_cpp.cpp:108-118 (X, Z in place)."""
    X = _inplace(X, "X")
    Z = _inplace(Z, "Z")
    mom = fmat(moments)
    check(lib().ace_normalize_test(X.shape[0], X.shape[1], Z.shape[1], ptr(X), ptr(Z), ptr(mom),
                                   mom.shape[0]))


def robust_levels(var, n_steps):
    """ace_robust_levels (R/robust_treatment.R:83-84, 94): the type-7 quantile
    thresholds of var at seq(0, 1, 1 / n_steps) and, per point, the first step
    at which it is retained.  Returns (thresholds (n_steps + 1), level (int32))."""
    v = vec(var)
    thr = np.empty(max(int(n_steps), 0) + 1)
    level = np.empty(v.size, dtype=np.int32)
    check(lib().ace_robust_levels(v.size, ptr(v), int(n_steps), ptr(thr), i32ptr(level)))
    return thr, level


def zero_pattern_order(Z):
    """ace_zero_pattern_order: the stable order of the rows of Z (n x ZS) by
    their pattern of exact zeros, fewest nonzero columns first, and the slice
    masks of the 64-point blocks of that order (bit j: some point of the block
    has a nonzero z in column j; a last block that is not full has every bit
    set).  Returns (perm (int64), blockmask (uint32) or None for ZS > 32)."""
    Zf = fmat(Z)
    if Zf.ndim != 2 or Zf.shape[0] < 1:
        raise AceError("Z must be n x ZS with n >= 1")
    n, ZS = Zf.shape
    perm = np.empty(n, dtype=np.int64)
    mask = np.zeros((n + 63) // 64, dtype=np.uint32)
    has = np.zeros(1, dtype=np.int32)
    check(lib().ace_zero_pattern_order(n, ZS, ptr(Zf) if ZS else None, iptr(perm), u32ptr(mask),
                                       i32ptr(has)))
    return perm, (mask if has[0] else None)


def _weights(W, B):
    """nz x B column-major weight rows of W, read column-major whatever its shape."""
    return np.asfortranarray(np.asarray(W, dtype=np.float64).reshape((-1, B), order="F"))


def coef_contract(mean, cov, W, offset=0.0, scale=1.0, shift=0.0, noise=0.0):
    """ace_coef_contract: a coefficient posterior (mean nx x B, cov nx x B x B)
    contracted with the nz weight rows W (nz x B), the tails of pred_cpp /
    pred_marginal_cpp (src/pred_cpp.cpp:20-29, 70-78):
    map = offset + scale (W_j . mean_c + shift), var = scale^2 |W_j^T cov_c W_j
    + noise|.  Returns {"map": (nx, nz), "ci": (nx, nz, 2), "var": (nx, nz)};
    raveled in Fortran order the first two axes are expand.grid(X, Z)."""
    mf = fmat(mean)
    if mf.ndim != 2:
        raise AceError("mean must be nx x B")
    nx, B = mf.shape
    cf = np.asfortranarray(np.asarray(cov, dtype=np.float64).reshape((nx, B, B), order="F"))
    Wf = _weights(W, B)
    mp, ci, var, out = map_ci_var(nx, Wf.shape[0])
    check(lib().ace_coef_contract(nx, B, Wf.shape[0], ptr(mf), ptr(cf), ptr(Wf), float(offset),
                                  float(scale), float(shift), float(noise), ptr(mp), ptr(ci),
                                  ptr(var)))
    return out


def coef_group_contract(gmean, gcov, gcount, W, offset=0.0, scale=1.0, shift=0.0,
                        return_cov=False):
    """ace_coef_group_contract: a group-summed coefficient posterior (gmean
    G x B, gcov G x B x G x B, gcount G: DeviceModel.coef_groups) contracted
    with the nz weight rows W (nz x B) into group averages:
    map = offset + scale (W_j . gmean_g / |g| + shift), var = scale^2
    |W_j^T C_gg W_j| / |g|^2 with C_gg group g's diagonal block.  Returns
    {"map": (G, nz), "ci": (G, nz, 2), "var": (G, nz)} and, with return_cov,
    "cov" (G, nz, nz), the signed scale^2 W_j^T C_gg W_j' / |g|^2.  An empty
    group gives NaN."""
    mf = fmat(gmean)
    if mf.ndim != 2:
        raise AceError("gmean must be G x B")
    G, B = mf.shape
    cf = np.asfortranarray(np.asarray(gcov, dtype=np.float64).reshape((G, B, G, B), order="F"))
    cnt = np.ascontiguousarray(np.ravel(gcount), dtype=np.int64)
    if cnt.size != G:
        raise AceError("gcount must have one entry per group")
    Wf = _weights(W, B)
    nz = Wf.shape[0]
    mp, ci, var, out = map_ci_var(G, nz)
    if return_cov:
        out["cov"] = np.empty((G, nz, nz), order="F")
    check(lib().ace_coef_group_contract(G, B, nz, ptr(mf), ptr(cf), iptr(cnt), ptr(Wf),
                                        float(offset), float(scale), float(shift), ptr(mp),
                                        ptr(ci), ptr(var), ptr(out.get("cov"))))
    return out


def potrf_lower(A, jitter=0.0, lda=None):
    """ace_potrf_lower: (L, info) with L the lower Cholesky factor of A +
    jitter I (the lower triangle of A is read; zeros above L's diagonal),
    info = 0, or the 1-based index of the first pivot that is <= 0 or not
    finite (L is then all NaN).  A: n x n, or with lda an (lda, n)
    column-major array whose first n rows are the matrix."""
    Af = fmat(A)
    if Af.ndim != 2:
        raise AceError("A must be a matrix")
    n = Af.shape[1]
    ld = Af.shape[0] if lda is None else int(lda)
    if Af.shape[0] != ld or ld < n or n < 1:
        raise AceError("A must be lda x n with lda >= n >= 1")
    L = np.empty((n, n), order="F")
    info = ctypes.c_int64(0)
    check(lib().ace_potrf_lower(n, ptr(Af), ld, float(jitter), ptr(L), n, ctypes.byref(info)))
    return L, int(info.value)


def cv_from_inverse(P, alpha, folds, ctx=None):
    """ace_cv_from_inverse: for every fold F (a list of integer arrays) of a
    symmetric P (n x n, the lower triangle is read) and alpha (n):
    {"resid": B_F^-1 alpha_F and "var": diag(B_F^-1), packed in the folds'
    order; "logdet": log det B_F, "mahal": alpha_F^T B_F^-1 alpha_F and
    "status" per fold; "off"} with B_F = P[F, F].  status = 0, or the 1-based
    index of the first pivot (rows sorted) that is <= 0 or not finite; that
    fold's outputs are NaN and the others are unaffected."""
    Pf = fmat(P)
    if Pf.ndim != 2 or Pf.shape[0] != Pf.shape[1]:
        raise AceError("P must be a square matrix")
    n = Pf.shape[0]
    al = vec(alpha)
    if al.size != n:
        raise AceError("alpha must have n entries")
    nf, off, idx = pack_folds(folds)
    tot = int(off[-1])
    r, v = np.empty(max(tot, 1)), np.empty(max(tot, 1))
    ld, mh = np.empty(nf), np.empty(nf)
    st = np.zeros(nf, dtype=np.int32)
    h = _ctx(ctx)
    check(lib().ace_cv_from_inverse(h, n, ptr(Pf), n, ptr(al), nf, iptr(off), iptr(idx), ptr(r),
                                    ptr(v), ptr(ld), ptr(mh), i32ptr(st)), h)
    return {"resid": r[:tot], "var": v[:tot], "logdet": ld, "mahal": mh, "status": st, "off": off}

"""Host-side mirror of the reference's R6 classes on the hot path:
KernelClass_SE_R6 / KernelClass_Matern32_R6 (R/kernel_SE_R6.R,
R/kernel_Matern32_R6.R) and the optimizer classes (R/optimizer_classes.R).

The numerics all run through the C ABI.  `para_update` uses the
device-resident model (ace_model_para_update): X, Z and y stay in HBM, the
n x n x B cube is never built, and `Kmat`, `Karray` and `invKmatn` become
on-demand handles that are materialised (at the theta they refer to) only
when a caller reads them (SURVEY.md §7 hard part ii).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native
from ._lib import (KIND, OPTIMIZER, UNIQUE_ID_BYTES, AceError, Handle, check, default_context, fmat,
                   lib, ptr)
from ._marshal import (ate_dicts, cols, i32ptr, iptr, labels, map_ci_var, pack_folds, rows, scalar,
                       vec)


class _ModelHandle(Handle):
    """A handle that lives in a Context (`self.ctx`): every entry point takes
    the handle first and reports its errors through the context."""

    def _call(self, name, *args):
        check(getattr(lib(), name)(self.handle, *args), self.ctx.handle)


class DeviceModel(_ModelHandle):
    """ace_model handle: one fit's resident data and the last inverse."""

    _destroy = "ace_model_destroy"

    def __init__(self, kind, n, p, B, ctx=None, world=1, rank=0, unique_id=None,
                 sharded=False, host_comm=None):
        """sharded=False: one GPU (ace_model_create).  sharded=True: rank
        `rank` of a `world`-rank block-column-sharded model
        (ace_model_create_sharded): unique_id = the 128 bytes rank 0 got from
        comm_unique_id() (RCCL, one process per GPU), or None to simulate all
        ranks in this process (validation mode).  host_comm (a HostComm):
        the collectives go through torch.distributed on host buffers
        (ace_model_create_sharded_host; validation over gloo)."""
        self.ctx = ctx or default_context()
        self.kind, self.n, self.p, self.B = kind, n, p, B
        self.P = 2 + B * (p + 1)
        self.world, self.rank = (world, rank) if sharded else (1, 0)
        c, h = self.ctx.handle, ctypes.c_void_p()
        if sharded and host_comm is not None:
            self._host_comm = host_comm  # keeps the callbacks alive
            check(lib().ace_model_create_sharded_host(c, KIND[kind], n, p, B, int(world), int(rank),
                                                      ctypes.byref(host_comm.ops),
                                                      ctypes.byref(h)), c)
        elif sharded:
            if unique_id is not None and len(unique_id) != UNIQUE_ID_BYTES:
                raise ValueError("unique_id must be 128 bytes")
            check(lib().ace_model_create_sharded(c, KIND[kind], n, p, B, int(world), int(rank),
                                                 unique_id, ctypes.byref(h)), c)
        else:
            check(lib().ace_model_create(c, KIND[kind], n, p, B, ctypes.byref(h)), c)
        self.handle = h

    def set_data(self, y, X, Z, std_y):
        yv, Xf, Zf = vec(y), fmat(X), cols(Z, self.n)
        self._call("ace_model_set_data", ptr(yv), ptr(Xf), ptr(Zf), float(std_y))

    def para_update(self, it, theta):
        """theta (float64, P) is mutated at it == 1 (mu overwrite)."""
        g = np.empty(self.P)
        st = np.empty(2)
        mu = ctypes.c_double()
        self._call("ace_model_para_update", int(it), ptr(theta), ptr(g), ptr(st), ctypes.byref(mu))
        return g, st, mu.value

    def train(self, theta, optimizer="Nadam", learning_rate=0.01, momentum=0.0, beta1=0.9,
              beta2=0.999, norm_clip=True, clip_at=1.0, maxiter=1000, tol=1e-4):
        """ace_model_train: the whole ace.train loop natively (R/main_ace.R:213-235).
        theta (float64, P) is updated in place; returns (stats 2 x (maxiter+2),
        iterations, converged)."""
        if optimizer == "GD":
            momentum = 0.0
        stats = np.zeros((2, maxiter + 2), order="F")
        it = ctypes.c_int()
        conv = ctypes.c_int()
        self._call("ace_model_train", OPTIMIZER[optimizer], float(learning_rate), float(momentum),
                   float(beta1), float(beta2), 1 if norm_clip else 0, float(clip_at), int(maxiter),
                   float(tol), ptr(theta), ptr(stats), ctypes.byref(it), ctypes.byref(conv))
        return stats, it.value, bool(conv.value)

    def train_stats(self, theta):
        th = np.ascontiguousarray(theta, dtype=np.float64)
        st = np.empty(2)
        self._call("ace_model_train_stats", ptr(th), ptr(st))
        return st

    def inverse(self):
        out = np.empty((self.n, self.n), order="F")
        self._call("ace_model_get_inverse", ptr(out))
        return out

    def apply_inverse(self, V):
        """ace_model_apply_inverse: A^-1 V with the resident inverse (V n x k)."""
        Vf = cols(V, self.n)
        out = np.empty_like(Vf, order="F")
        self._call("ace_model_apply_inverse", Vf.shape[1], ptr(Vf), ptr(out))
        return out if np.ndim(V) == 2 else out.ravel()

    def _test_side(self, theta, X2, Z2=None, label=None):
        """What every query at test points starts from: theta, the rows X2
        and, where given, their basis rows (nx x (B-1)) and int32 group
        labels, converted for the library; and nx."""
        X2f = fmat(X2)
        nx = X2f.shape[0]
        return (vec(theta), X2f, None if Z2 is None else cols(Z2, nx),
                None if label is None else labels(label, nx), nx)

    def predict(self, theta, X2, Z2, mean_y, std_y):
        """ace_model_predict: pred_cpp with the resident inverse (Q6), kernels at theta."""
        th, X2f, Z2f, _, nx = self._test_side(theta, X2, Z2)
        mp, ci, var, out = map_ci_var(nx)
        self._call("ace_model_predict", ptr(th), nx, ptr(X2f), ptr(Z2f), float(mean_y),
                   float(std_y), ptr(mp), ptr(ci), ptr(var))
        return out

    def predict_marginal(self, theta, X2, dZ2, Z_x, std_y, std_Z, calculate_ate):
        """ace_model_predict_marginal: pred_marginal_cpp with the resident inverse."""
        th, X2f, dZf, _, nx = self._test_side(theta, X2, dZ2)
        zx = vec(Z_x) if calculate_ate else None
        mp, ci, var, out = map_ci_var(nx)
        avg = np.empty(12)
        self._call("ace_model_predict_marginal", ptr(th), nx, ptr(X2f), ptr(dZf), ptr(zx),
                   float(std_y), scalar(std_Z), 1 if calculate_ate else 0, ptr(mp), ptr(ci),
                   ptr(var), ptr(avg))
        if calculate_ate:
            out.update(ate_dicts(avg))
        return out

    def predict_marginal_groups(self, theta, X2, dZ2, std_y, std_Z, G, label):
        """ace_model_predict_marginal_groups: predict_marginal's map / ci / var
        plus, for the G groups of `label` (int, -1 = no group), gsum (the sum
        of map), gcount and gcov = E^T C E (G x G) with C the unscaled
        marginal posterior covariance; the nx x nx test kernel is never built."""
        th, X2f, dZf, lab, nx = self._test_side(theta, X2, dZ2, label)
        G = int(G)
        Gs = max(G, 1)
        mp, ci, var, out = map_ci_var(nx)
        out.update(gsum=np.empty(Gs), gcount=np.zeros(Gs, dtype=np.int64),
                   gcov=np.empty((Gs, Gs), order="F"))
        self._call("ace_model_predict_marginal_groups", ptr(th), nx, ptr(X2f), ptr(dZf),
                   float(std_y), scalar(std_Z), G, i32ptr(lab), ptr(mp), ptr(ci), ptr(var),
                   ptr(out["gsum"]), iptr(out["gcount"]), ptr(out["gcov"]))
        return out

    def robust_treatment(self, theta, X2, dZ2, Z_x, std_y, std_Z, n_steps=5):
        """ace_model_robust_treatment: the ATE / ATT / ATU of every discard step
        of R/robust_treatment.R from one marginal pass and one grouped pass.
        avg is 12 x (n_steps + 1) (column t as predict_marginal's averages on
        step t's subset), counts 3 x (n_steps + 1) (retained, treated,
        untreated); "ate" / "att" / "atu" hold the per-step map, ci, var."""
        th, X2f, dZf, _, nx = self._test_side(theta, X2, dZ2)
        zx = vec(Z_x)
        if zx.size != nx:
            raise AceError("Z_x must have one entry per test point")
        n_steps = int(n_steps)
        T = max(n_steps, 0) + 1
        mp, ci, var, out = map_ci_var(nx)
        thr = np.empty(T)
        level = np.empty(nx, dtype=np.int32)
        avg = np.empty((12, T), order="F")
        counts = np.zeros((3, T), dtype=np.int64, order="F")
        self._call("ace_model_robust_treatment", ptr(th), nx, ptr(X2f), ptr(dZf), ptr(zx),
                   float(std_y), scalar(std_Z), n_steps, ptr(mp), ptr(ci), ptr(var), ptr(thr),
                   i32ptr(level), ptr(avg), iptr(counts))
        out.update(thresholds=thr, level=level, avg=avg, counts=counts)
        out.update(ate_dicts(avg))
        return out

    def coef_posterior(self, theta, X2):
        """ace_model_coef_posterior: the posterior of the coefficient vector
        g(x) at every row of X2 -- {"mean": (nx, B), "cov": (nx, B, B)} in
        normalised-y units, without mu and without the noise term."""
        th, X2f, _, _, nx = self._test_side(theta, X2)
        mean = np.empty((nx, self.B), order="F")
        cov = np.empty((nx, self.B, self.B), order="F")
        self._call("ace_model_coef_posterior", ptr(th), nx, ptr(X2f), ptr(mean), ptr(cov))
        return {"mean": mean, "cov": cov}

    def coef_cross(self, theta, X2):
        """ace_model_coef_cross: the per-slice cross kernels (nx, n, B) the
        coefficient posterior is formed from (a test basis of ones)."""
        th, X2f, _, _, nx = self._test_side(theta, X2)
        Kc = np.empty((nx, self.n, self.B), order="F")
        self._call("ace_model_coef_cross", ptr(th), nx, ptr(X2f), ptr(Kc))
        return Kc

    def predict_surface(self, theta, X2, Zb, marginal, mean_y, std_y, std_Z):
        """ace_model_predict_surface: pred_cpp (marginal false; Zb the test
        basis, nz x (B-1)) or pred_marginal_cpp (Zb its derivative) on the
        grid of every row of X2 with every row of Zb, from one coefficient
        pass: {"map": (nx, nz), "ci": (nx, nz, 2), "var": (nx, nz)}."""
        th, X2f, _, _, nx = self._test_side(theta, X2)
        Zf = rows(Zb, max(self.B - 1, 1))
        nz = Zf.shape[0]
        mp, ci, var, out = map_ci_var(nx, nz)
        self._call("ace_model_predict_surface", ptr(th), nx, ptr(X2f), nz, ptr(Zf),
                   1 if marginal else 0, float(mean_y), float(std_y), scalar(std_Z), ptr(mp),
                   ptr(ci), ptr(var))
        return out

    def coef_groups(self, theta, X2, G, label):
        """ace_model_coef_groups: the posterior of the coefficient vectors
        summed over each of the G groups of `label` (int, -1 = no group) --
        {"gmean": (G, B), "gcov": (G, B, G, B), "gcount": (G,)}, sums (not
        averages) in normalised-y units, without mu and the noise term.
        gcov[g, b, h, b'] is the covariance of group g's slice b with group
        h's slice b'; G <= 64 and G B <= 2048."""
        th, X2f, _, lab, nx = self._test_side(theta, X2, label=label)
        G = int(G)
        Gs = max(G, 1)
        gmean = np.empty((Gs, self.B), order="F")
        gcov = np.empty((Gs, self.B, Gs, self.B), order="F")
        gcount = np.zeros(Gs, dtype=np.int64)
        self._call("ace_model_coef_groups", ptr(th), nx, ptr(X2f), G, i32ptr(lab), ptr(gmean),
                   ptr(gcov), iptr(gcount))
        return {"gmean": gmean, "gcov": gcov, "gcount": gcount}

    def average_response(self, theta, X2, G, label, Zb, marginal, mean_y, std_y, std_Z,
                         return_cov=False):
        """ace_model_average_response: the average dose-response curve of
        every group at the nz rows of Zb (the test basis, nz x (B-1), or with
        marginal its derivative), predict_surface's conventions without a
        noise term: {"map": (G, nz), "ci": (G, nz, 2), "var": (G, nz)} and,
        with return_cov, "cov" (G, nz, nz).  An empty group gives NaN."""
        th, X2f, _, lab, nx = self._test_side(theta, X2, label=label)
        G = int(G)
        Zf = rows(Zb, max(self.B - 1, 1))
        nz = Zf.shape[0]
        mp, ci, var, out = map_ci_var(max(G, 1), nz)
        if return_cov:
            out["cov"] = np.empty((max(G, 1), nz, nz), order="F")
        self._call("ace_model_average_response", ptr(th), nx, ptr(X2f), G, i32ptr(lab), nz,
                   ptr(Zf), 1 if marginal else 0, float(mean_y), float(std_y), scalar(std_Z),
                   ptr(mp), ptr(ci), ptr(var), ptr(out.get("cov")))
        return out

    def predict_joint(self, theta, X2, Z2, mean_y, std_y, *, marginal=False, std_Z=1.0,
                      noise=True, jitter=0.0, xi=None, return_cov=False, return_factor=False):
        """ace_model_predict_joint: the joint posterior at the rows of X2 --
        {"map", "info"} and, if asked, "cov" (nx x nx, exactly symmetric), "L"
        (lower Cholesky factor of cov + jitter I) and, with xi (nx x S standard
        normals, the caller's), "draws" = map 1^T + L xi.  Z2: the test basis,
        or with marginal its derivative (then std_y / std_Z scales, and
        mean_y and noise are not used).  info > 0: pivot info of the factor
        was not positive -- L and draws are NaN, map and cov valid; under Q6
        (kernels at a theta other than the resident inverse's) cov need not be
        positive semidefinite.  nx <= 8192, S <= 4096, single-GPU models."""
        th, X2f, Zf, _, nx = self._test_side(theta, X2, Z2)
        S = 0
        xif = draws = None
        if xi is not None:
            xif = cols(xi, nx)
            S = xif.shape[1]
            draws = np.empty((nx, S), order="F") if S else None
            if not S:
                xif = None
        mp = np.empty(nx)
        cov = np.empty((nx, nx), order="F") if return_cov else None
        L = np.empty((nx, nx), order="F") if return_factor else None
        info = ctypes.c_int64(0)
        self._call("ace_model_predict_joint", ptr(th), nx, ptr(X2f), ptr(Zf), 1 if marginal else 0,
                   float(mean_y), float(std_y), scalar(std_Z), 1 if noise else 0, float(jitter), S,
                   ptr(xif), ptr(mp), ptr(cov), ptr(L), ptr(draws), ctypes.byref(info))
        out = {"map": mp, "info": int(info.value)}
        if return_cov:
            out["cov"] = cov
        if return_factor:
            out["L"] = L
        if xi is not None:
            out["draws"] = draws if S else np.empty((nx, 0), order="F")
        return out

    def cv(self, theta, folds, mean_y, std_y):
        """ace_model_cv: cross-validation from the resident inverse, without
        a refit.  folds: a list of integer arrays of the caller's rows (they
        may overlap and need not cover the data).  Returns {"map", "var",
        "resid": packed in the folds' order, original units; "lpd", "mahal",
        "status": per fold; "off": the packed offsets}.  status > 0: that
        fold's block of the inverse is not positive definite at that pivot
        -- its outputs are NaN, the other folds are unaffected.  The inverse
        is the last para_update's, mu = theta[1] (Q6), as predict uses them.
        Single-GPU models."""
        th = vec(theta)
        nf, off, idx = pack_folds(folds)
        tot = int(off[-1])
        mp, var, res = (np.empty(max(tot, 1)) for _ in range(3))
        lpd, mh = np.empty(nf), np.empty(nf)
        st = np.zeros(nf, dtype=np.int32)
        self._call("ace_model_cv", ptr(th), nf, iptr(off), iptr(idx), float(mean_y), float(std_y),
                   ptr(mp), ptr(var), ptr(res), ptr(lpd), ptr(mh), i32ptr(st))
        return {"map": mp[:tot], "var": var[:tot], "resid": res[:tot], "lpd": lpd, "mahal": mh,
                "status": st, "off": off}

    def comm_calls(self):
        """ace_model_comm_calls: collectives this rank issued since creation,
        {"broadcast", "allgather", "allreduce", "groups"} (zeros when simulated)."""
        c = (ctypes.c_int64 * 4)()
        self._call("ace_model_comm_calls", c)
        return dict(zip(("broadcast", "allgather", "allreduce", "groups"), c))

    def profile(self, enable):
        self._call("ace_model_profile", 1 if enable else 0)

    def kernel_time(self, which):
        ms = ctypes.c_double()
        nl = ctypes.c_int64()
        work = ctypes.c_double()
        self._call("ace_model_kernel_time", which, ctypes.byref(ms), ctypes.byref(nl),
                   ctypes.byref(work))
        return ms.value, nl.value, work.value


class BatchModel(_ModelHandle):
    """ace_batch handle: M independent models of at most nmax <= 512 rows, one
    kernel kind, p and B; one workgroup per model (single GPU)."""

    _destroy = "ace_batch_destroy"

    def __init__(self, kind, M, nmax, p, B, ctx=None):
        self.ctx = ctx or default_context()
        self.kind, self.M, self.nmax, self.p, self.B = kind, int(M), int(nmax), p, B
        self.P = 2 + B * (p + 1)
        self.n = [0] * self.M
        h = ctypes.c_void_p()
        check(lib().ace_batch_create(self.ctx.handle, KIND[kind], self.M, self.nmax, p, B,
                                     ctypes.byref(h)), self.ctx.handle)
        self.handle = h

    def set_data(self, j, y, X, Z, std_y):
        yv = vec(y)
        n = yv.size
        Xf, Zf = cols(X, n), cols(Z, n)
        self._call("ace_batch_set_data", int(j), n, ptr(yv), ptr(Xf), ptr(Zf), float(std_y))
        self.n[int(j)] = n

    def para_update(self, it, theta):
        """theta (float64, P x M column-major) is mutated at it == 1 (mu
        overwrite); returns grad (P x M), stats (2 x M), mu_post (M)."""
        assert theta.shape == (self.P, self.M) and theta.flags.f_contiguous
        g = np.empty((self.P, self.M), order="F")
        st = np.empty((2, self.M), order="F")
        mu = np.empty(self.M)
        self._call("ace_batch_para_update", int(it), ptr(theta), ptr(g), ptr(st), ptr(mu))
        return g, st, mu

    def train(self, theta, optimizer="Nadam", learning_rate=0.01, momentum=0.0, beta1=0.9,
              beta2=0.999, norm_clip=True, clip_at=1.0, maxiter=1000, tol=1e-4):
        """ace_batch_train: every model's ace.train loop, in lock step.  theta
        (float64, P x M column-major) is updated in place; returns (stats
        2 x (maxiter + 2) x M, iterations M, converged M, status M -- 0 or
        ACE_ERR_NONFINITE = 5 per model)."""
        assert theta.shape == (self.P, self.M) and theta.flags.f_contiguous
        if optimizer == "GD":
            momentum = 0.0
        stats = np.zeros((2, maxiter + 2, self.M), order="F")
        it, conv, status = (np.zeros(self.M, dtype=np.int32) for _ in range(3))
        self._call("ace_batch_train", OPTIMIZER[optimizer], float(learning_rate), float(momentum),
                   float(beta1), float(beta2), 1 if norm_clip else 0, float(clip_at), int(maxiter),
                   float(tol), ptr(theta), ptr(stats), i32ptr(it), i32ptr(conv), i32ptr(status))
        return stats, it, conv.astype(bool), status

    def inverse(self, j):
        n = self.n[int(j)]
        out = np.empty((n, n), order="F")
        self._call("ace_batch_get_inverse", int(j), ptr(out))
        return out

    def set_inverse(self, j, inv):
        """ace_set_inverse_batch: inv (n_j x n_j, symmetric) becomes model j's
        resident inverse (after its set_data)."""
        n = self.n[int(j)] if 0 <= int(j) < self.M else 0
        a = fmat(inv)
        if n and a.shape != (n, n):
            raise AceError(f"ACE_ERR_ARG: the inverse of model {j} must be {n} x {n}")
        self._call("ace_set_inverse_batch", int(j), ptr(a))

    def _pack_test(self, theta, X2s, Zts):
        """theta (P x M), and the packed test side: off (M + 1), every model's
        X2 block (nx_j x p) and basis block (nx_j x (B - 1)), column-major."""
        th = fmat(theta)
        if th.shape != (self.P, self.M) or len(X2s) != self.M or len(Zts) != self.M:
            raise AceError(f"ACE_ERR_ARG: theta must be P x M = {self.P} x {self.M} and the test "
                           "sides sequences of length M")
        xs = [fmat(x) for x in X2s]
        xs = [x.reshape(-1, self.p, order="F") if self.p else x.reshape(-1, 0) for x in xs]
        nx = [x.shape[0] for x in xs]
        off = np.zeros(self.M + 1, dtype=np.int64)
        off[1:] = np.cumsum(nx)
        zs = []
        for j, z in enumerate(Zts):
            z = fmat(z) if self.B > 1 else np.zeros((nx[j], 0))
            if z.size != nx[j] * (self.B - 1):
                raise AceError(f"ACE_ERR_ARG: the test basis of model {j} must be nx_j x (B - 1) = "
                               f"{nx[j]} x {self.B - 1}")
            zs.append(z.reshape(nx[j], self.B - 1, order="F"))
        cat = lambda blocks: np.ascontiguousarray(  # noqa: E731
            np.concatenate([np.ravel(b, order="F") for b in blocks]) if blocks else np.empty(0))
        return th, off, cat(xs), cat(zs)

    def _per_model(self, v):
        a = np.ravel(np.asarray(v, dtype=np.float64))
        if a.size == 1:
            a = np.full(self.M, a[0])
        if a.size != self.M:
            raise AceError("ACE_ERR_ARG: a moment must be a scalar or have length M")
        return np.ascontiguousarray(a)

    def predict(self, theta, X2s, Z2s, mean_y, std_y):
        """ace_predict_batch: pred_cpp of every model in one launch, each with
        its own resident inverse (Q6) and kernels at its column of theta.
        X2s, Z2s: sequences of length M; mean_y, std_y: scalars or length M.
        Returns a list of M dicts {"map", "ci", "var"}."""
        th, off, x2, z2 = self._pack_test(theta, X2s, Z2s)
        my, sy = self._per_model(mean_y), self._per_model(std_y)
        N = int(off[-1])
        mp, var, ci = np.empty(N), np.empty(N), np.empty(2 * N)
        self._call("ace_predict_batch", ptr(th), iptr(off), ptr(x2), ptr(z2), ptr(my), ptr(sy),
                   ptr(mp), ptr(ci), ptr(var))
        return [self._split(off, j, mp, ci, var) for j in range(self.M)]

    @staticmethod
    def _split(off, j, mp, ci, var):
        o, e = int(off[j]), int(off[j + 1])
        return {"map": mp[o:e].copy(), "ci": ci[2 * o:2 * e].reshape(e - o, 2, order="F").copy(order="F"),
                "var": var[o:e].copy()}

    def predict_marginal(self, theta, X2s, dZ2s, Z_xs, std_y, std_Z, calculate_ate=False):
        """ace_predict_marginal_batch: pred_marginal_cpp of every model in one
        launch; with calculate_ate also "ate" / "att" / "atu" per model, as
        DeviceModel.predict_marginal gives them (Z_xs: the binary treatment of
        every model's test points)."""
        th, off, x2, dz = self._pack_test(theta, X2s, dZ2s)
        sy, sz = self._per_model(std_y), self._per_model(std_Z)
        N = int(off[-1])
        zx = avg = None
        if calculate_ate:
            if len(Z_xs) != self.M:
                raise AceError("ACE_ERR_ARG: Z_xs must have length M")
            zx = np.ascontiguousarray(np.concatenate([np.ravel(np.asarray(z, dtype=np.float64))
                                                      for z in Z_xs]))
            if zx.size != N:
                raise AceError("ACE_ERR_ARG: Z_xs must hold one value per test point")
            avg = np.empty((12, self.M), order="F")
        mp, var, ci = np.empty(N), np.empty(N), np.empty(2 * N)
        self._call("ace_predict_marginal_batch", ptr(th), iptr(off), ptr(x2), ptr(dz), ptr(zx),
                   ptr(sy), ptr(sz), 1 if calculate_ate else 0, ptr(mp), ptr(ci), ptr(var),
                   ptr(avg))
        outs = [self._split(off, j, mp, ci, var) for j in range(self.M)]
        if calculate_ate:
            for j, out in enumerate(outs):
                out.update(ate_dicts(avg[:, j]))
        return outs


def comm_unique_id():
    """ace_comm_unique_id: the RCCL bootstrap id (rank 0 calls it and sends
    the bytes to every rank out of band)."""
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    check(lib().ace_comm_unique_id(buf), None)
    return buf.raw


class _KernelClass:
    """Common body of KernelClass_SE_R6 / KernelClass_Matern32_R6."""

    kernel = None  # "SE" | "Matern32"

    def __init__(self, p_arg, B_arg, ext_init_parameters, std_y_arg=1.0, verbose=False,
                 ctx=None):
        if verbose:
            print("Using SE kernel" if self.kernel == "SE" else "Using Matern 3/2 kernel")
        self.B = int(B_arg)
        self.p = int(p_arg)
        self.parameters = np.array(np.ravel(ext_init_parameters), dtype=np.float64)
        self.stdy = float(std_y_arg)
        self.ctx = ctx
        self._model = None
        self._data_id = None
        self._kern_theta = None   # theta of the current Kmat / Karray handle
        self._kern_data = None    # (X, Z) they are evaluated on
        self._kcache = None
        self._inv = None          # explicit inverse (getinv_kernel path)
        self._inv_from_model = False

    # ----------------------------------------------------------- R6 fields
    @property
    def Kmat(self):
        return self._materialise()["full"] if self._kern_theta is not None else None

    @property
    def Karray(self):
        return self._materialise()["elements"] if self._kern_theta is not None else None

    @property
    def invKmatn(self):
        if self._inv_from_model and self._inv is None:
            self._inv = self._model.inverse()
        return self._inv

    def _sym(self, X, Z, theta=None):
        """This kind's symmetric kernel list at theta (None: the parameters)."""
        return native._kernmat_sym(KIND[self.kernel], X, Z,
                                   self.parameters if theta is None else theta, self.ctx)

    def _materialise(self):
        if self._kcache is None:
            self._kcache = self._sym(*self._kern_data, self._kern_theta)
        return self._kcache

    def _mark_kernel(self, X, Z):
        self._kern_theta = self.parameters.copy()
        self._kern_data = (X, Z)
        self._kcache = None

    # ----------------------------------------------------------- R6 methods
    def kernel_mat(self, X1, X2, Z1, Z2):
        return native._kernmat_cross(KIND[self.kernel], X1, X2, Z1, Z2, self.parameters, self.ctx)

    def kernel_mat_sym(self, X, Z):
        Klist = self._sym(X, Z)
        self._mark_kernel(X, Z)
        self._kcache = Klist
        return Klist

    def getinv_kernel(self, X, Z):
        self.kernel_mat_sym(X, Z)
        lst = native.invkernel_cpp(self.Kmat, self.parameters[0], ctx=self.ctx)
        self._inv = lst["inv"]
        self._inv_from_model = False
        return lst

    def _ensure_model(self, y, X, Z):
        key = (id(y), id(X), id(Z))
        n = np.asarray(X).shape[0]
        if self._model is None or self._data_id != key:
            self._model = DeviceModel(self.kernel, n, self.p, self.B, self.ctx)
            self._model.set_data(y, X, Z, self.stdy)
            self._data_id = key
        return self._model

    def use_model(self, model, y, X, Z):
        """Attach an already-created DeviceModel (e.g. a sharded one) holding
        y, X, Z; para_update then runs on it."""
        model.set_data(y, X, Z, self.stdy)
        self._model = model
        self._data_id = (id(y), id(X), id(Z))
        return model

    def para_update(self, iter, y, X, Z, Optim, printevery=100, verbose=True):  # noqa: A002
        """R/kernel_SE_R6.R:40-62 (R/kernel_Matern32_R6.R:39-60)."""
        model = self._ensure_model(y, X, Z)
        self._mark_kernel(X, Z)
        gradients, stats, mu_post = model.para_update(iter, self.parameters)
        self._inv = None
        self._inv_from_model = True
        self.parameters = Optim.update(iter, self.parameters, gradients)
        self.parameters[1] = mu_post  # mean_solution with this iteration's inverse
        if verbose and iter % printevery == 0:
            print("%5d | log Evidence %9.4f | RMSE %9.4f | Norm. noise var: %3.4f | "
                  "Gradient L2: %3.4f" % (iter, stats[1], stats[0], np.exp(self.parameters[0]),
                                          np.linalg.norm(gradients)))
        return stats

    def get_train_stats(self, y, X, Z, invKmatList=None):
        """R/kernel_SE_R6.R:63-74: fresh kernel + inverse at the current theta,
        stats_cpp with mu = theta[1]; the stored inverse is NOT replaced (Q6)."""
        if invKmatList is not None:
            self.kernel_mat_sym(X, Z)
            return native.stats_cpp(y, self.Kmat, invKmatList["inv"], invKmatList["eigenval"],
                                    self.parameters[1], self.stdy, ctx=self.ctx)
        model = self._ensure_model(y, X, Z)
        self._mark_kernel(X, Z)
        return model.train_stats(self.parameters)

    def _resident(self, y, X, Z):
        """The device model holds this fit's inverse (invKmatn never replaced
        from outside) and was built on the same training data."""
        return (self._inv_from_model and self._model is not None and
                self._data_id == (id(y), id(X), id(Z)))

    def _on_model(self, what, y, X, Z):
        """The fit's device model, for the queries that exist only on it."""
        if not self._resident(y, X, Z):
            raise AceError(f"{what} needs the fit's device-resident inverse "
                           "(para_update on the same data)")
        return self._model

    def predict(self, y, X, Z, X2, Z2, mean_y, std_y):
        """R/kernel_SE_R6.R:75-83.  With the fit's device model the inverse
        stays in HBM (ace_model_predict); otherwise the pred_cpp ABI."""
        if self._resident(y, X, Z):
            return self._model.predict(self.parameters, X2, Z2, mean_y, std_y)
        K_xX = self.kernel_mat(X2, X, Z2, Z)["full"]
        K_xx = self._sym(X2, Z2)["full"]
        return native.pred_cpp(y, self.parameters[0], self.parameters[1], self.invKmatn, K_xX,
                               K_xx, mean_y, std_y, ctx=self.ctx)

    def predict_marginal(self, y, X, Z, X2, Z2, dZ2, mean_y, std_y, std_Z, calculate_ate):
        """R/kernel_SE_R6.R:84-97 (device-resident like predict)."""
        if self._resident(y, X, Z):
            return self._model.predict_marginal(self.parameters, X2, dZ2, Z2, std_y, std_Z,
                                                calculate_ate)
        Km_xX = self.kernel_mat(X2, X, dZ2, Z)["elements"]
        Km_xx = self._sym(X2, dZ2)["elements"]
        return native.pred_marginal_cpp(y, Z2, self.parameters[0], self.parameters[1],
                                        self.invKmatn, Km_xX, Km_xx, mean_y, std_y, std_Z,
                                        calculate_ate, ctx=self.ctx)

    def robust_treatment(self, y, X, Z, X2, Z2, dZ2, std_y, std_Z, n_steps=5):
        """R/robust_treatment.R:83-128 on the fit's device model: Z2 is the
        binary treatment of the test points, dZ2 their derivative basis."""
        return self._on_model("robust_treatment", y, X, Z).robust_treatment(
            self.parameters, X2, dZ2, Z2, std_y, std_Z, n_steps)

    def coef_posterior(self, y, X, Z, X2):
        """The posterior of the coefficient functions at the rows of X2, on
        the fit's device model (DeviceModel.coef_posterior)."""
        return self._on_model("coef_posterior", y, X, Z).coef_posterior(self.parameters, X2)

    def predict_surface(self, y, X, Z, X2, Zb, marginal, mean_y, std_y, std_Z):
        """predict / predict_marginal on the grid of the rows of X2 and of Zb
        (the test basis, or its derivative when marginal), on the fit's device
        model (DeviceModel.predict_surface)."""
        return self._on_model("predict_surface", y, X, Z).predict_surface(
            self.parameters, X2, Zb, marginal, mean_y, std_y, std_Z)

    def coef_groups(self, y, X, Z, X2, G, label):
        """The group-summed posterior of the coefficient functions at the rows
        of X2, on the fit's device model (DeviceModel.coef_groups)."""
        return self._on_model("coef_groups", y, X, Z).coef_groups(self.parameters, X2, G, label)

    def average_response(self, y, X, Z, X2, G, label, Zb, marginal, mean_y, std_y, std_Z,
                         return_cov=False):
        """The groups' average dose-response curves at the rows of Zb, on the
        fit's device model (DeviceModel.average_response)."""
        return self._on_model("average_response", y, X, Z).average_response(
            self.parameters, X2, G, label, Zb, marginal, mean_y, std_y, std_Z, return_cov)

    def predict_joint(self, y, X, Z, X2, Z2, mean_y, std_y, **kw):
        """The joint posterior at the test points on the fit's device model
        (DeviceModel.predict_joint and its keywords; Z2 the test basis, or its
        derivative with marginal=True)."""
        return self._on_model("predict_joint", y, X, Z).predict_joint(
            self.parameters, X2, Z2, mean_y, std_y, **kw)

    def cross_validate(self, y, X, Z, folds, mean_y, std_y):
        """Cross-validation from the fit's resident inverse, without a refit
        (DeviceModel.cv; folds a list of index arrays)."""
        return self._on_model("cross_validate", y, X, Z).cv(self.parameters, folds, mean_y, std_y)

    def mean_solution(self, y):
        """R/kernel_SE_R6.R:99-102 (private in the SE class)."""
        self.parameters[1] = native.mu_solution_cpp(y, self.invKmatn, ctx=self.ctx)


class KernelClass_SE_R6(_KernelClass):
    kernel = "SE"


class KernelClass_Matern32_R6(_KernelClass):
    kernel = "Matern32"


# --------------------------------------------------------------------------
# R/optimizer_classes.R
# --------------------------------------------------------------------------
_NONFINITE = ("Some gradients are not finite, NaN, or NA. Often this is due to too large "
              "learning rates.")


class optAdam:
    def __init__(self, KernelObj, lr, beta1, beta2, norm_clip, clip_at):
        self.m = KernelObj.parameters * 0
        self.v = KernelObj.parameters * 0
        self.lr, self.beta1, self.beta2 = lr, beta1, beta2
        self.norm_clip, self.clip_at = norm_clip, clip_at

    def update(self, iter, parameters, gradients):  # noqa: A002
        native.norm_clip_cpp(self.norm_clip, gradients, self.clip_at)
        if not native.Adam_cpp(iter, self.lr, self.beta1, self.beta2, 1e-8, self.m, self.v,
                               gradients, parameters):
            raise AceError(_NONFINITE)
        return parameters


class optNadam(optAdam):
    def update(self, iter, parameters, gradients):  # noqa: A002
        native.norm_clip_cpp(self.norm_clip, gradients, self.clip_at)
        if not native.Nadam_cpp(iter, self.lr, self.beta1, self.beta2, 1e-8, self.m, self.v,
                                gradients, parameters):
            raise AceError(_NONFINITE)
        return parameters


class optNesterov:
    def __init__(self, KernelObj, lr, momentum, norm_clip, clip_at):
        self.nu = KernelObj.parameters * 0
        self.lr, self.momentum = lr, momentum
        self.norm_clip, self.clip_at = norm_clip, clip_at

    def update(self, iter, parameters, gradients):  # noqa: A002
        native.norm_clip_cpp(self.norm_clip, gradients, self.clip_at)
        if not native.Nesterov_cpp(self.lr, self.momentum, self.nu, gradients, parameters):
            raise AceError(_NONFINITE)
        return parameters


def set_optimizer(optimizer, myKernel, learning_rate, momentum, beta1, beta2, norm_clip,
                  clip_at):
    """R/utilities.R:8-21"""
    if optimizer == "Adam":
        return optAdam(myKernel, learning_rate, beta1, beta2, norm_clip, clip_at)
    if optimizer == "Nadam":
        return optNadam(myKernel, learning_rate, beta1, beta2, norm_clip, clip_at)
    if optimizer in ("GD", "NAG"):
        if optimizer == "GD":
            momentum = 0.0
        return optNesterov(myKernel, learning_rate, momentum, norm_clip, clip_at)
    raise AceError(f"unknown optimizer {optimizer!r}")

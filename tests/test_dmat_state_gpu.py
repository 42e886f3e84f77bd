"""The stateful side of the device-handle path (csrc/ace_dmat.cpp): region
reads of every handle kind, chunked prediction through handles, the dense
branches, the per-context caches (packed side, last response), the pool of
recycled sweep buffers, a non-PD inverse in every consumer, and B == 1.

References: oracle/ace_oracle.py and numpy, on inputs tests/dmat_cases.py
builds and tests/test_dmat_cases_cpu.py checks.  Another call of the library
is the reference only where the library promises bitwise equality, and there
the oracle comparison is made as well.  Tolerances are the project's: kernel
values 1e-12, inverse 1e-9 (both of the largest entry of the whole array, as
close() takes them on a whole read), gradient / stats / map close()'s
defaults, variances VAR_TOL of the cancelled terms, averaged effects as
test_device_predict_marginal_ate_matches_oracle.
"""
import os

import numpy as np
import pytest

import dmat_cases as C
from conftest import ROOT, record_error, run_child
from test_gpu import RTOL, close
from test_predict_gpu import CI_TOL, VAR_TOL

pytestmark = pytest.mark.gpu

KERNELS = C.KERNEL_NAMES


@pytest.fixture(scope="module")
def A():
    import additivecausalexpansion_amd as pkg
    pkg.default_context()
    return pkg


@pytest.fixture(scope="module")
def O():
    from oracle import ace_oracle
    return ace_oracle


def sym_fn(A, kernel):
    return A.kernmat_SE_symmetric_cpp if kernel == "SE" else A.kernmat_Matern32_symmetric_cpp


def cross_fn(A, kernel):
    return A.kernmat_SE_cpp if kernel == "SE" else A.kernmat_Matern32_cpp


def grad_fn(A, kernel):
    return A.grad_SE_cpp if kernel == "SE" else A.grad_Matern_cpp


def flat(a):
    return np.ravel(np.asarray(a), order="F")


def close_in(got, ref, tol, scale, check):
    """|got - ref| <= tol |ref| + tol scale, scale the largest entry of the
    whole array the range was taken from (close() on a whole read)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (check, got.shape, ref.shape)
    if not ref.size:
        return
    bound = tol * np.abs(ref) + tol * scale
    err = np.abs(got - ref)
    assert np.all(np.isfinite(got)), check
    record_error(f"{check}: bound used", float(np.max(err / bound)), 1.0)
    assert np.all(err <= bound), (check, float(np.max(err / bound)))


def var_held(got, ref, terms, check):
    err = np.abs(np.asarray(got) - ref)
    assert np.all(np.isfinite(got)), check
    record_error(f"{check}: max |err| / terms", float(np.max(err / terms)), VAR_TOL)
    assert np.all(err <= VAR_TOL * terms), (check, float(np.max(err / terms)))


def mu_held(got, ref, check):
    """As test_dmat_handles_read_and_mix: relative 1e-8."""
    record_error(f"{check}: |err| / |ref|", abs(got - ref) / abs(ref), 1e-8)
    assert got == pytest.approx(ref, rel=1e-8), check


def ate_held(got, ref):
    """As test_device_predict_marginal_ate_matches_oracle."""
    for k in ("ate", "att", "atu"):
        close(got[k]["map"], ref[k]["map"], check=f"{k} map")
        close(got[k]["var"], ref[k]["var"], 1e-6, 1e-10, check=f"{k} var")
        sd = np.sqrt(abs(ref[k]["var"]))
        size = abs(ref[k]["map"]) + 1.96 * sd
        err = np.max(np.abs(got[k]["ci"] - ref[k]["ci"]))
        record_error(f"{k} ci: max |err| / (|map| + 1.96 sd)", err / size, CI_TOL)
        assert err <= CI_TOL * size, (k, got[k]["ci"], ref[k]["ci"])


def inv_held(h, ref, check):
    close(np.asarray(h), ref, 1e-9, 1e-9, check=check)


def device_kernel(A, kernel, s):
    return sym_fn(A, kernel)(s["X"], s["Z"], s["th"], device=True)


def grad_held(A, kernel, s, Kfull, K, lst_inv, eigenval, check, y=None, X=None, ref=None):
    """grad_*_cpp over handles against the oracle's gradient and stats for
    the state s (or the reference given)."""
    y = s["y"] if y is None else y
    X = s["X"] if X is None else X
    B = s["Z"].shape[1] + 1
    st = np.zeros(2)
    g = grad_fn(A, kernel)(y, X, s["Z"], Kfull, K, lst_inv, eigenval, s["th"], st, B, s["sy"])
    if ref is None:
        ref = C.oracle_grad(kernel, y, X, s["Z"], s["full"], s["elements"], s["inv"],
                            s["eigenval"], s["th"], s["sy"])
    close(g, ref[0], check=f"{check}: gradient")
    close(st, ref[1], check=f"{check}: stats")
    return g, st


def test_handles_keep_their_context_alive(A):
    """A handle frees into its context's buffer pool, so it holds the
    Context: dropping the caller's last reference to the Context leaves the
    handles usable, and a context closed first is not freed into."""
    ctx = A.Context(0)
    lst = A.invkernel_cpp(A.DMat.upload(2.0 * np.eye(5), ctx), 0.0, ctx)
    owner = lst["inv"]._owner
    assert owner is ctx
    del ctx, owner
    assert np.allclose(np.asarray(lst["inv"]), np.eye(5) / 3.0, rtol=1e-14, atol=0)
    assert lst["inv"]._owner.handle


# ====================================================================== A
KINDS = ("virtual symmetric cube", "virtual cross cube", "dense cube", "ksym full", "cross full",
         "swept inverse")
NX_A = 37


def make_handle(A, O, kernel, kind):
    """(handle, oracle values, tolerance, stays virtual, what keeps it alive)."""
    s = C.oracle_state(kernel, "n130")
    X2, Z2 = C.new_points("n130", NX_A)
    if kind in ("virtual cross cube", "cross full"):
        Kl = cross_fn(A, kernel)(X2, s["X"], Z2, s["Z"], s["th"], device=True)
        ref = O.KERNELS[kernel][1](X2, s["X"], Z2, s["Z"], s["th"])
        if kind == "cross full":
            return Kl["full"], ref["full"], 1e-12, False, Kl
        return Kl["elements"], ref["elements"], 1e-12, True, Kl
    if kind == "dense cube":
        return A.DMat.upload(s["elements"]), s["elements"], 1e-12, False, None
    Kl = device_kernel(A, kernel, s)
    if kind == "virtual symmetric cube":
        return Kl["elements"], s["elements"], 1e-12, True, Kl
    if kind == "ksym full":
        return Kl["full"], s["full"], 1e-12, False, Kl
    lst = A.invkernel_cpp(Kl["full"], s["th"][0])
    return lst["inv"], s["inv"], 1e-9, False, (Kl, lst)


def region_dims(h):
    # a matrix's "slices" are its columns
    return h.shape if len(h.shape) == 3 else (h.shape[0], 1, h.shape[1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_region_reads_match_oracle(A, O, kernel, kind):
    """ace_dmat_read(h, offset, count) as the R shim's Elt / Get_region call
    it: every region of the CPU-checked list equals the oracle's column-major
    range, and is bitwise the same range of the handle's whole read.  The
    regions at offset > 0 are read first, so a SWEPT / KSYM handle is
    materialised by an offset read."""
    h, ref, tol, virtual, _keep = make_handle(A, O, kernel, kind)
    assert h.shape == ref.shape
    want = flat(ref)
    scale = np.abs(want).max()
    regs = C.regions(*region_dims(h))
    got = {}
    for name, off, cnt in sorted(regs, key=lambda r: r[1] == 0):
        got[name] = h.read_region(off, cnt)
        assert got[name].shape == (cnt,)
        close_in(got[name], want[off:off + cnt], tol, scale, f"{kind} '{name}'")
        assert h.read_to_host
        assert h.on_device == (not virtual), (kind, name)
    whole = flat(h.read())
    assert h.on_device == (not virtual)
    for name, off, cnt in regs:
        assert np.array_equal(got[name], whole[off:off + cnt]), (kind, name)


@pytest.mark.parametrize("form", ["symmetric", "cross"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_virtual_cube_slice_cache(A, O, kernel, form):
    """Slice 2, slice 0, a region over 0|1, slice 2 again: the one cached
    slice is replaced, reused and replaced; the cube is never built."""
    h, ref, tol, _, _keep = make_handle(A, O, kernel, f"virtual {form} cube")
    want = flat(ref)
    scale = np.abs(want).max()
    for j, (off, cnt) in enumerate(C.slice_cache_reads(*h.shape[:2])):
        close_in(h.read_region(off, cnt), want[off:off + cnt], tol, scale,
                 f"{form} cube, slice-cache read {j}")
        assert not h.on_device
    # the straddling read left slice 1 cached: a read inside it is a download
    sl = h.shape[0] * h.shape[1]
    close_in(h.read_region(sl + 3, 9), want[sl + 3:sl + 12], tol, scale, "read of the cached slice")
    assert not h.on_device


@pytest.mark.parametrize("kernel", KERNELS)
def test_virtual_cube_element_reads(A, O, kernel):
    """600 one-element reads across the slice boundary 0|1 (ALTREP Elt)."""
    h, ref, tol, _, _keep = make_handle(A, O, kernel, "virtual cross cube")
    assert h.shape[:2] == (NX_A, 130)
    want = flat(ref)
    offs = C.element_reads(*h.shape[:2])
    got = np.array([h.read_region(o, 1)[0] for o in offs])
    close_in(got, want[offs[0]:offs[-1] + 1], tol, np.abs(want).max(), "element reads")
    assert not h.on_device


@pytest.mark.parametrize("kernel", KERNELS)
def test_offset_read_materialises_without_changing_consumers(A, kernel):
    """A KSYM / SWEPT handle first read at offset > 0 is materialised; the
    inverse of the materialised KSYM and the gradient with the materialised
    inverse are bitwise what they were before."""
    s = C.oracle_state(kernel, "n130")
    n = 130
    Kl = device_kernel(A, kernel, s)
    before = A.invkernel_cpp(Kl["full"], s["th"][0])
    assert not Kl["full"].on_device
    off = 7 * n + 11
    close_in(Kl["full"].read_region(off, 3 * n), flat(s["full"])[off:off + 3 * n], 1e-12,
             np.abs(s["full"]).max(), "ksym offset read")
    assert Kl["full"].on_device
    after = A.invkernel_cpp(Kl["full"], s["th"][0])
    assert np.array_equal(after["eigenval"], before["eigenval"])
    inv_held(after["inv"], s["inv"], "inverse of the materialised ksym")
    assert np.array_equal(np.asarray(after["inv"]), np.asarray(before["inv"]))
    lst = A.invkernel_cpp(Kl["full"], s["th"][0])
    g0, st0 = grad_held(A, kernel, s, Kl["full"], Kl["elements"], lst["inv"], lst["eigenval"],
                        "before the offset read")
    assert not lst["inv"].on_device
    close_in(lst["inv"].read_region(off, 3 * n), flat(s["inv"])[off:off + 3 * n], 1e-9,
             np.abs(s["inv"]).max(), "swept offset read")
    assert lst["inv"].on_device
    g1, st1 = grad_held(A, kernel, s, Kl["full"], Kl["elements"], lst["inv"], lst["eigenval"],
                        "after the offset read")
    assert np.array_equal(g0, g1) and np.array_equal(st0, st1)


@pytest.mark.parametrize("kind", KINDS)
def test_read_refusals_leave_the_handle_usable(A, O, kind):
    h, ref, tol, _, _keep = make_handle(A, O, "SE", kind)
    total = ref.size
    for off, cnt in ((-1, 1), (total - 1, 2), (0, total + 1), (total + 1, 0), (0, -1), (5, -1)):
        with pytest.raises(A.AceError, match="ACE_ERR_ARG"):
            h.read_region(off, cnt)
    want = flat(ref)
    close_in(h.read_region(total - 9, 9), want[total - 9:], tol, np.abs(want).max(),
             f"{kind} after refusals")


# ====================================================================== B
def chunk_held(got, ref, what):
    close(got["map"], ref["map"], check=f"{what} map")
    var_held(got["var"], ref["var"], ref["terms"], f"{what} var")
    # an off-by-a-chunk row offset shows first around the chunk boundary
    mscale = np.abs(ref["map"]).max()
    for r in C.chunk_boundary_rows():
        assert abs(got["map"][r] - ref["map"][r]) <= RTOL * abs(ref["map"][r]) + 1e-9 * mscale, \
            f"{what} map, test point {r} (chunk boundary 8192)"
        assert abs(got["var"][r] - ref["var"][r]) <= VAR_TOL * ref["terms"][r], \
            f"{what} var, test point {r} (chunk boundary 8192)"


def chunk_inverse(A, kernel, c):
    Kl = sym_fn(A, kernel)(c["X"], c["Z"], c["th_prev"], device=True)
    lst = A.invkernel_cpp(Kl["full"], c["th_prev"][0])
    inv_held(lst["inv"], c["inv"], "chunk case inverse")
    return lst


@pytest.mark.parametrize("kernel", KERNELS)
def test_chunked_pred_through_handles(A, kernel):
    """pred_cpp over handles with nx = 8192 + 77: K_xX the cross `full`
    handle (read at values + c0 with ld = nx in the second chunk), K_xx the
    virtual KSYM of the test points (only its diagonal is formed), a SWEPT
    inverse.  Reference: dmat_cases.chunk_case; var held to VAR_TOL of
    std_y^2 (|kxx| + |q| + e^sigma)."""
    c = C.chunk_case(kernel)
    lst = chunk_inverse(A, kernel, c)
    th = c["th"]
    KxX = cross_fn(A, kernel)(c["X2"], c["X"], c["Z2"], c["Z"], th, device=True)["full"]
    Kxx = sym_fn(A, kernel)(c["X2"], c["Z2"], th, device=True)["full"]
    got = A.pred_cpp(c["y"], th[0], th[1], lst["inv"], KxX, Kxx, C.MEAN_Y, C.STD_Y)
    assert not Kxx.on_device
    chunk_held(got, c["pred"], "chunked pred_cpp")
    sd = np.sqrt(got["var"])
    close(got["ci"], np.stack([got["map"] - 1.96 * sd, got["map"] + 1.96 * sd], axis=1), 1e-12,
          1e-12, check="ci = map -+ 1.96 sd")


def test_chunked_pred_marginal_through_handles(A):
    """pred_marginal_cpp over virtual cubes with nx = 8192 + 77: the second
    chunk's marginal slice sums are assembled from row 8192 on
    (marginal_rows with r0 > 0); the test points' symmetric cube gives its
    diagonal and stays virtual.  No averaged effects at this size."""
    kernel = "SE"
    c = C.chunk_case(kernel)
    lst = chunk_inverse(A, kernel, c)
    th = c["th"]
    KxX = cross_fn(A, kernel)(c["X2"], c["X"], c["dZ2"], c["Z"], th, device=True)["elements"]
    Kxx = sym_fn(A, kernel)(c["X2"], c["dZ2"], th, device=True)["elements"]
    got = A.pred_marginal_cpp(c["y"], None, th[0], th[1], lst["inv"], KxX, Kxx, C.MEAN_Y, C.STD_Y,
                              C.STD_Z, False)
    assert not Kxx.on_device and not KxX.on_device
    assert "ate" not in got
    chunk_held(got, c["marginal"], "chunked pred_marginal_cpp")
    # the oracle's cross cube uploaded: the second chunk copies its rows out of
    # the slice sum cached on the handle
    Dense = A.DMat.upload(c["KmxX"])
    got = A.pred_marginal_cpp(c["y"], None, th[0], th[1], lst["inv"], Dense, Kxx, C.MEAN_Y,
                              C.STD_Y, C.STD_Z, False)
    chunk_held(got, c["marginal"], "chunked pred_marginal_cpp, dense K_xX cube")


# ====================================================================== C
NX_C = 90


def pred_inputs(O, kernel, name, nx):
    """The oracle's test kernels for PROBLEMS[name] at the theta of its
    inverse (the averaged variances exist), and the references."""
    s = C.oracle_state(kernel, name)
    X2, Z2 = C.new_points(name, nx)
    _, dZ2 = C.new_points(name, nx, 0.7, 0.1)
    zx = (np.arange(nx) % 3 == 0).astype(float)
    symo, crosso = O.KERNELS[kernel][0], O.KERNELS[kernel][1]
    th, y, inv = s["th"], s["y"], s["inv"]
    p = {"X2": X2, "Z2": Z2, "dZ2": dZ2, "zx": zx}
    p["KxX"] = np.asfortranarray(crosso(X2, s["X"], Z2, s["Z"], th)["full"])
    p["Kxx"] = np.asfortranarray(symo(X2, Z2, th)["full"])
    p["KmxX"] = np.asfortranarray(crosso(X2, s["X"], dZ2, s["Z"], th)["elements"])
    p["Kmxx"] = np.asfortranarray(symo(X2, dZ2, th)["elements"])
    p["pred"] = O.pred_cpp(y, th[0], s["mu"], inv, p["KxX"], p["Kxx"], 0.3, 1.7)
    q = np.abs(np.sum((p["KxX"] @ inv) * p["KxX"], axis=1))
    p["pred_terms"] = 1.7 ** 2 * (np.abs(np.diag(p["Kxx"])) + q + np.exp(th[0]))
    p["marg"] = O.pred_marginal_cpp(y, zx, th[0], s["mu"], inv, p["KmxX"], p["Kmxx"], 0.3, 1.7,
                                    0.8, True)
    B = p["KmxX"].shape[2]
    sl = slice(1, B) if B > 1 else slice(0, 1)
    KmX = p["KmxX"][:, :, sl].sum(axis=2)
    q = np.abs(np.sum((KmX @ inv) * KmX, axis=1))
    p["marg_terms"] = (1.7 / 0.8) ** 2 * (np.abs(np.diag(p["Kmxx"][:, :, sl].sum(axis=2))) + q)
    return s, p


def pred_held(A, s, p, inv, KxX, Kxx, check):
    got = A.pred_cpp(s["y"], s["th"][0], s["mu"], inv, KxX, Kxx, 0.3, 1.7)
    close(got["map"], p["pred"]["map"], check=f"{check}: pred map")
    var_held(got["var"], p["pred"]["var"], p["pred_terms"], f"{check}: pred var")
    close(got["ci"], p["pred"]["ci"], 1e-6, 1e-8, check=f"{check}: pred ci")
    return got


def marginal_held(A, s, p, inv, KmxX, Kmxx, check):
    got = A.pred_marginal_cpp(s["y"], p["zx"], s["th"][0], s["mu"], inv, KmxX, Kmxx, 0.3, 1.7, 0.8,
                              True)
    close(got["map"], p["marg"]["map"], check=f"{check}: marginal map")
    var_held(got["var"], p["marg"]["var"], p["marg_terms"], f"{check}: marginal var")
    ate_held(got, p["marg"])
    return got


@pytest.mark.parametrize("kernel", KERNELS)
def test_dense_inverse_and_dense_cubes(A, O, kernel):
    """Uploaded (DENSE) inverse, cubes and Kfull in every consumer: the
    branches a SWEPT inverse / virtual cube never takes."""
    s, p = pred_inputs(O, kernel, "n300", NX_C)
    y, th, sy = s["y"], s["th"], s["sy"]
    Dinv, Dfull, Dcube = (A.DMat.upload(s[k]) for k in ("inv", "full", "elements"))
    mu_held(A.mu_solution_cpp(y, Dinv), s["mu"], "dense inverse: mu_solution")
    close(A.stats_cpp(y, Dfull, Dinv, s["eigenval"], s["mu"], sy),
          O.stats_cpp(y, s["full"], s["inv"], s["eigenval"], s["mu"], sy), check="dense: stats")
    grad_held(A, kernel, s, Dfull, Dcube, Dinv, s["eigenval"], "dense inverse, dense cube")
    grad_held(A, kernel, s, Dfull, None, Dinv, s["eigenval"], "dense inverse, K = None")
    DKxX, DKxx = A.DMat.upload(p["KxX"]), A.DMat.upload(p["Kxx"])
    pred_held(A, s, p, Dinv, DKxX, DKxx, "dense")
    DmX, Dmx = A.DMat.upload(p["KmxX"]), A.DMat.upload(p["Kmxx"])
    first = marginal_held(A, s, p, Dinv, DmX, Dmx, "dense cubes")
    # the second call takes the slice sums cached on the (immutable) handles
    again = marginal_held(A, s, p, Dinv, DmX, Dmx, "dense cubes, cached slice sum")
    for k in ("map", "var", "ci"):
        assert np.array_equal(first[k], again[k]), k
    for k in ("ate", "att", "atu"):
        for f in ("map", "var", "ci"):
            assert np.array_equal(first[k][f], again[k][f]), (k, f)
    assert np.array_equal(np.asarray(DmX), p["KmxX"])
    assert np.array_equal(np.asarray(Dmx), p["Kmxx"])
    assert np.array_equal(np.asarray(Dcube), s["elements"])
    assert np.array_equal(np.asarray(Dinv), s["inv"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_handle_kinds_in_one_call(A, O, kernel):
    """SWEPT inverse + DENSE Kfull + virtual cube, and DENSE inverse + KSYM
    Kfull.  The RMSE residual may be taken as e^sigma alpha only when the
    inverse was swept from that very Kfull handle: a DENSE Kfull of other
    values, and a DENSE inverse of another sigma, must give the oracle's
    explicit ybar - Kfull alpha."""
    s, p = pred_inputs(O, kernel, "n300", NX_C)
    y, th, sy = s["y"], s["th"], s["sy"]
    Kl = device_kernel(A, kernel, s)
    lst = A.invkernel_cpp(Kl["full"], th[0])
    Dfull = A.DMat.upload(s["full"])
    grad_held(A, kernel, s, Dfull, Kl["elements"], lst["inv"], lst["eigenval"],
              "swept inverse, dense Kfull, virtual cube")
    other = C.oracle_state(kernel, "n300b")["full"]
    ref = C.oracle_grad(kernel, y, s["X"], s["Z"], other, s["elements"], s["inv"], s["eigenval"],
                        th, sy)
    grad_held(A, kernel, s, A.DMat.upload(other), Kl["elements"], lst["inv"], lst["eigenval"],
              "swept inverse, dense Kfull of other values", ref=ref)
    close(A.stats_cpp(y, A.DMat.upload(other), lst["inv"], lst["eigenval"], s["mu"], sy),
          O.stats_cpp(y, other, s["inv"], s["eigenval"], s["mu"], sy),
          check="swept inverse, dense Kfull of other values: stats")
    s7 = C.oracle_state(kernel, "n300", 0.7)
    D7 = A.DMat.upload(s7["inv"])
    close(A.stats_cpp(y, Kl["full"], D7, s7["eigenval"], s["mu"], sy),
          O.stats_cpp(y, s["full"], s7["inv"], s7["eigenval"], s["mu"], sy),
          check="dense inverse of another sigma, ksym Kfull: stats")
    ref = C.oracle_grad(kernel, y, s["X"], s["Z"], s["full"], s["elements"], s7["inv"],
                        s7["eigenval"], th, sy)
    grad_held(A, kernel, s, Kl["full"], Kl["elements"], D7, s7["eigenval"],
              "dense inverse of another sigma, ksym Kfull", ref=ref)
    # prediction: swept inverse with dense kernels, dense inverse with virtual ones
    pred_held(A, s, p, lst["inv"], A.DMat.upload(p["KxX"]), A.DMat.upload(p["Kxx"]),
              "swept inverse, dense kernels")
    Kc = cross_fn(A, kernel)(p["X2"], s["X"], p["dZ2"], s["Z"], th, device=True)
    Ks = sym_fn(A, kernel)(p["X2"], p["dZ2"], th, device=True)
    marginal_held(A, s, p, A.DMat.upload(s["inv"]), Kc["elements"], Ks["elements"],
                  "dense inverse, virtual cubes")
    assert not Kc["elements"].on_device and not Ks["elements"].on_device


# ====================================================================== D
def changed(a, row, col, by):
    b = np.array(a, order="F")
    b[row, col] += by
    return b


@pytest.mark.parametrize("kernel", KERNELS)
def test_side_cache_invalidation_and_handle_immutability(A, O, kernel):
    """The packed (X, Z) side is reused only for bitwise the same X and Z,
    kind, p and B; a handle keeps the side it was made from."""
    s = C.oracle_state(kernel, "n300")
    X, Z, th = s["X"], s["Z"], s["th"]
    n = X.shape[0]
    other = "Matern32" if kernel == "SE" else "SE"
    s5 = C.oracle_state(kernel, "n300_p2B5")
    X2 = changed(X, n - 1, 1, 0.5)
    Z3 = changed(Z, n - 1, 2, 0.25)
    made = [(kernel, X, Z, th), (kernel, X2, Z, th), (kernel, X, Z3, th), (other, X, Z, th),
            (kernel, s5["X"], s5["Z"], s5["th"]), (kernel, X, Z, th)]
    hs = [sym_fn(A, k)(x, z, t, device=True) for k, x, z, t in made]
    lst = A.invkernel_cpp(hs[0]["full"], th[0])  # h1 after the cache has moved on
    inv_held(lst["inv"], s["inv"], "inverse of h1 after h2 .. h6")
    for j, (k, x, z, t) in enumerate(made):
        ref = s if j in (0, 5) else s5 if j == 4 else O.KERNELS[k][0](x, z, t)
        close(np.asarray(hs[j]["full"]), ref["full"], 1e-12, 1e-12, check=f"h{j + 1} full")
        close(np.asarray(hs[j]["elements"]), ref["elements"], 1e-12, 1e-12,
              check=f"h{j + 1} elements")
    # the changed entry is visible in the oracle (else the comparison is blind)
    assert np.abs(O.KERNELS[kernel][0](X2, Z, th)["full"] - s["full"]).max() > 1e-6
    assert np.abs(O.KERNELS[kernel][0](X, Z3, th)["full"] - s["full"]).max() > 1e-6
    # the gradient takes X and Z of its own call: (X', Z) with Kfull and the
    # inverse of X is the oracle's result for that mixture (cube and distances
    # from X', residual and inverse from X), not the handles' own side
    mix = O.KERNELS[kernel][0](X2, Z, th)["elements"]
    ref = C.oracle_grad(kernel, s["y"], X2, Z, s["full"], mix, s["inv"], s["eigenval"], th, s["sy"])
    plain = C.oracle_grad(kernel, s["y"], X, Z, s["full"], s["elements"], s["inv"], s["eigenval"],
                          th, s["sy"])
    assert np.max(np.abs(ref[0] - plain[0]) / (RTOL * np.abs(plain[0])
                                                + 1e-9 * np.abs(plain[0]).max())) > 10
    grad_held(A, kernel, s, hs[0]["full"], None, lst["inv"], lst["eigenval"], "grad with X'",
              X=X2, ref=ref)
    grad_held(A, kernel, s, hs[0]["full"], None, lst["inv"], lst["eigenval"], "grad with X again")


_FRESH_Y = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import additivecausalexpansion_amd as A
import dmat_cases as C
out = {{}}
for kernel in C.KERNEL_NAMES:
    s = C.oracle_state(kernel, "n300")
    sym = A.kernmat_SE_symmetric_cpp if kernel == "SE" else A.kernmat_Matern32_symmetric_cpp
    grad = A.grad_SE_cpp if kernel == "SE" else A.grad_Matern_cpp
    Kl = sym(s["X"], s["Z"], s["th"], device=True)
    lst = A.invkernel_cpp(Kl["full"], s["th"][0])  # no y has been seen
    out[kernel + "_direct"] = np.array(float(not Kl["full"].on_device))
    out[kernel + "_ev"] = lst["eigenval"]
    out[kernel + "_mu"] = np.array(A.mu_solution_cpp(s["y"], lst["inv"]))
    st = np.zeros(2)
    out[kernel + "_g"] = grad(s["y"], s["X"], s["Z"], Kl["full"], Kl["elements"], lst["inv"],
                              lst["eigenval"], s["th"], st, 4, s["sy"])
    out[kernel + "_gst"] = st
    out[kernel + "_st"] = A.stats_cpp(s["y"], Kl["full"], lst["inv"], lst["eigenval"], s["mu"],
                                      s["sy"])
    out[kernel + "_inv"] = np.asarray(lst["inv"])
    del lst, Kl
np.savez({out!r}, **out)
"""


@pytest.mark.parametrize("direct", ["1", "0"])
def test_inverse_before_any_response_in_a_fresh_context(O, tmp_path, direct):
    """invkernel before any y was seen (no response rides in AUG row 0), then
    mu, grad, stats: in a child, with the direct assembly of a virtual Kfull
    and with ACE_DMAT_DIRECT=0's copy-in path, to the same bounds."""
    out = str(tmp_path / "fresh.npz")
    run_child(_FRESH_Y.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out),
              env=dict(os.environ, ACE_DMAT_DIRECT=direct))
    with np.load(out) as f:
        got = {k: f[k] for k in f.files}
    for kernel in KERNELS:
        s = C.oracle_state(kernel, "n300")
        assert bool(got[kernel + "_direct"]) == (direct == "1")
        inv_held(got[kernel + "_inv"], s["inv"], f"{kernel} inverse, no y seen")
        assert np.sum(np.log(got[kernel + "_ev"])) == pytest.approx(
            np.sum(np.log(s["eigenval"])), rel=1e-10)
        mu_held(float(got[kernel + "_mu"]), s["mu"], f"{kernel} mu, no y seen")
        ref = C.oracle_grad(kernel, s["y"], s["X"], s["Z"], s["full"], s["elements"], s["inv"],
                            s["eigenval"], s["th"], s["sy"])
        close(got[kernel + "_g"], ref[0], check=f"{kernel} gradient, no y seen")
        close(got[kernel + "_gst"], ref[1], check=f"{kernel} gradient stats, no y seen")
        close(got[kernel + "_st"], O.stats_cpp(s["y"], s["full"], s["inv"], s["eigenval"], s["mu"],
                                               s["sy"]), check=f"{kernel} stats, no y seen")


@pytest.mark.parametrize("kernel", KERNELS)
def test_response_cache_sequences(A, O, kernel):
    """invkernel sweeps the last noted response along only when its length
    is n; the gradient takes alpha from the swept AUG rows only for bitwise
    that response, else from a product with the inverse."""
    s = C.oracle_state(kernel, "n300")
    y, th, sy = s["y"], s["th"], s["sy"]
    Kl = device_kernel(A, kernel, s)

    def stats_held(yv, inv, ev, check):
        got = A.stats_cpp(yv, Kl["full"], inv, ev, s["mu"], sy)
        close(got, O.stats_cpp(yv, s["full"], s["inv"], s["eigenval"], s["mu"], sy), check=check)
        return got

    def grad_of(yv, lst, check):
        ref = C.oracle_grad(kernel, yv, s["X"], s["Z"], s["full"], s["elements"], s["inv"],
                            s["eigenval"], th, sy)
        return grad_held(A, kernel, s, Kl["full"], Kl["elements"], lst["inv"], lst["eigenval"],
                         check, y=yv, ref=ref)

    # (ii) a response of length n - 1 is noted, then an inverse at n
    s9 = C.oracle_state(kernel, "n299")
    l9 = A.invkernel_cpp(device_kernel(A, kernel, s9)["full"], s9["th"][0])
    mu_held(A.mu_solution_cpp(s9["y"], l9["inv"]), s9["mu"], "mu at n - 1")
    lst = A.invkernel_cpp(Kl["full"], th[0])
    inv_held(lst["inv"], s["inv"], "inverse after a response of another length")
    mu_held(A.mu_solution_cpp(y, lst["inv"]), s["mu"], "mu after a response of another length")
    grad_of(y, lst, "(ii) grad")
    stats_held(y, lst["inv"], lst["eigenval"], "(ii) stats")
    # (iii) ya noted, inverse (ya rides along), grad(yb), grad(ya), stats(yb)
    ya, yb = y, C.problem("n300b")[0]
    mu_held(A.mu_solution_cpp(ya, lst["inv"]), s["mu"], "mu notes ya")
    la = A.invkernel_cpp(Kl["full"], th[0])
    grad_of(yb, la, "(iii) grad(yb)")
    grad_of(ya, la, "(iii) grad(ya) from the AUG rows")
    stats_held(yb, la["inv"], la["eigenval"], "(iii) stats(yb)")
    stats_held(ya, la["inv"], la["eigenval"], "(iii) stats(ya) from the AUG rows")
    # alternating: an inverse that yb rode along
    A.stats_cpp(yb, Kl["full"], la["inv"], la["eigenval"], s["mu"], sy)
    lb = A.invkernel_cpp(Kl["full"], th[0])
    grad_of(ya, lb, "grad(ya) by the product")
    grad_of(yb, lb, "grad(yb) from the AUG rows")
    grad_of(ya, lb, "grad(ya) after yb")
    grad_of(yb, la, "grad(yb) on the inverse of ya")
    stats_held(ya, la["inv"], la["eigenval"], "stats(ya) from the AUG rows, after yb")


def used(a, b, rtol, atol_rel):
    """The largest fraction of close()'s bound that |a - b| uses."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / (rtol * np.abs(b) + atol_rel * np.abs(b).max())))


@pytest.mark.parametrize("kernel", KERNELS)
def test_aug_rows_agree_with_the_product_path(A, kernel):
    """grad(ya) and stats(ya) with alpha from the swept AUG rows (ya rode
    along) against the same with alpha = inv (ya - mu) (yb rode along), to the
    1e-10, 1e-12 of test_virtual_kfull_sweep_matches_fused_model.  The
    gradient of mu, sum(inv ybar), is the sensitive entry: summed over a
    product with the swept inverse it was 2.4e-10 off at SE (1.75 of the
    bound; the oracle and the AUG rows are within 1e-12 of a long-double
    solve), so grad_dev takes it from the inverse's AUG row 1 on both paths."""
    s = C.oracle_state(kernel, "n300")
    ya, yb, th, sy = s["y"], C.problem("n300b")[0], s["th"], s["sy"]
    Kl = device_kernel(A, kernel, s)
    grad = grad_fn(A, kernel)
    res = {}
    for path, rode in (("aug", ya), ("product", yb)):
        A.stats_cpp(rode, Kl["full"], A.DMat.upload(s["inv"]), s["eigenval"], s["mu"], sy)
        lst = A.invkernel_cpp(Kl["full"], th[0])  # `rode` is in AUG row 0
        st = np.zeros(2)
        g = grad(ya, s["X"], s["Z"], Kl["full"], Kl["elements"], lst["inv"], lst["eigenval"], th,
                 st, 4, sy)
        res[path] = (g, st, A.stats_cpp(ya, Kl["full"], lst["inv"], lst["eigenval"], s["mu"], sy))
    ref = C.oracle_grad(kernel, ya, s["X"], s["Z"], s["full"], s["elements"], s["inv"],
                        s["eigenval"], th, sy)
    worst = {}
    for j, what in enumerate(("gradient", "gradient stats", "stats")):
        worst[what] = used(res["aug"][j], res["product"][j], 1e-10, 1e-12)
        record_error(f"AUG rows against product: {what}: bound used", worst[what], 1.0)
    print(f"{kernel}: bound used {worst}; mu-gradient aug {res['aug'][0][1]!r} product "
          f"{res['product'][0][1]!r} oracle {ref[0][1]!r}")
    close(res["aug"][0], ref[0], check="AUG rows: gradient")
    close(res["product"][0], ref[0], check="product: gradient")
    assert all(v <= 1.0 for v in worst.values()), worst


# ====================================================================== E
_FRESH_INV = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import additivecausalexpansion_amd as A
import dmat_cases as C
out, keep = {{}}, []
for kernel in C.KERNEL_NAMES:
    for name in ("n300b", "n130b"):
        s = C.oracle_state(kernel, name)
        sym = A.kernmat_SE_symmetric_cpp if kernel == "SE" else A.kernmat_Matern32_symmetric_cpp
        Kl = sym(s["X"], s["Z"], s["th"], device=True)
        for path, K in (("virtual", Kl["full"]), ("dense", A.DMat.upload(s["full"]))):
            lst = A.invkernel_cpp(K, s["th"][0])
            keep.append((Kl, K, lst))  # nothing is freed: every inverse is on new buffers
            out[kernel + name + path] = np.asarray(lst["inv"])
            out[kernel + name + path + "_ev"] = lst["eigenval"]
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def fresh_inverses(tmp_path_factory):
    """Inverses made on never-used sweep buffers, in a fresh process."""
    out = str(tmp_path_factory.mktemp("fresh") / "inv.npz")
    run_child(_FRESH_INV.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out))
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


def K_of(A, kernel, s, path):
    if path == "virtual":
        return device_kernel(A, kernel, s)["full"]
    return A.DMat.upload(s["full"])


def make_inverse(A, kernel, s, path, check):
    lst = A.invkernel_cpp(K_of(A, kernel, s, path), s["th"][0])
    assert np.all(lst["eigenval"] > 0), check
    inv_held(lst["inv"], s["inv"], check)
    assert np.sum(np.log(lst["eigenval"])) == pytest.approx(np.sum(np.log(s["eigenval"])),
                                                            rel=1e-10), check
    return lst


def make_nonpd(A, n):
    r = A.invkernel_cpp(A.DMat.upload(C.nonpd_matrix(n)), C.NONPD_SIGMA)
    assert np.all(np.isnan(np.asarray(r["inv"])))
    assert np.any(r["eigenval"] <= 0)
    return r


@pytest.mark.parametrize("path", ["virtual", "dense"])
@pytest.mark.parametrize("first", ["healthy", "nonpd"])
@pytest.mark.parametrize("name_a,name_b", [("n300", "n300b"), ("n130", "n130b")])
@pytest.mark.parametrize("kernel", KERNELS)
def test_recycled_sweep_buffers(A, fresh_inverses, kernel, name_a, name_b, first, path):
    """An inverse freed (healthy, or one whose sweep was not positive
    definite) hands its buffers to the next inverse of that n: the flag and
    the counters start clean, and the result is bitwise what a fresh process
    computes (sweeps are deterministic)."""
    sa, sb = C.oracle_state(kernel, name_a), C.oracle_state(kernel, name_b)
    n = sa["X"].shape[0]
    # two inverses kept alive take whatever the pool held for this n, so inv_a
    # is on new buffers and inv_b on exactly those
    hold = [A.invkernel_cpp(K_of(A, kernel, sa, "dense"), sa["th"][0]) for _ in range(2)]
    for _ in range(2):
        a = make_inverse(A, kernel, sa, path, "inv_a") if first == "healthy" else make_nonpd(A, n)
        del a
        b = make_inverse(A, kernel, sb, path, f"inv_b on buffers of a {first} inverse")
        key = kernel + name_b + path
        assert np.array_equal(np.asarray(b["inv"]), fresh_inverses[key])
        assert np.array_equal(b["eigenval"], fresh_inverses[key + "_ev"])
        grad_held(A, kernel, sb, K_of(A, kernel, sb, "dense"), None, b["inv"], b["eigenval"],
                  "grad on recycled buffers")
        del b
    for lst in hold:
        inv_held(lst["inv"], sa["inv"], "an inverse alive throughout")


@pytest.mark.parametrize("kernel", KERNELS)
def test_two_inverses_alive_and_pool_sizes(A, kernel):
    s, s7 = C.oracle_state(kernel, "n300"), C.oracle_state(kernel, "n300", 0.7)
    sb, sm = C.oracle_state(kernel, "n300b"), C.oracle_state(kernel, "n130")
    Kl = device_kernel(A, kernel, s)
    # two alive at once, same n, different sigma; the second is read first
    l0 = A.invkernel_cpp(Kl["full"], s["th"][0])
    l7 = A.invkernel_cpp(Kl["full"], s7["th"][0])
    inv_held(l7["inv"], s7["inv"], "second of two inverses alive")
    inv_held(l0["inv"], s["inv"], "first of two inverses alive")
    grad_held(A, kernel, s, Kl["full"], Kl["elements"], l0["inv"], l0["eigenval"], "first alive")
    grad_held(A, kernel, s7, Kl["full"], Kl["elements"], l7["inv"], l7["eigenval"], "second alive")
    grad_held(A, kernel, s, Kl["full"], Kl["elements"], l0["inv"], l0["eigenval"], "first again")
    del l0, l7
    # a pool holding another n: free 130, make 300, then 130
    m = make_inverse(A, kernel, sm, "virtual", "n = 130")
    del m
    make_inverse(A, kernel, s, "virtual", "n = 300 with n = 130 pooled")
    make_inverse(A, kernel, sm, "dense", "n = 130 after n = 300")
    # three freed in a row (the pool keeps two), then three made and all alive
    three = [make_inverse(A, kernel, st, "virtual", "before the frees") for st in (s, sb, s7)]
    while three:
        three.pop()
    three = [make_inverse(A, kernel, st, path, f"after three frees: {j}")
             for j, (st, path) in enumerate(((sb, "virtual"), (s7, "dense"), (s, "virtual")))]
    for lst, st in zip(three, (sb, s7, s)):
        inv_held(lst["inv"], st["inv"], "three alive, read again")
    del three
    # the direct path and the dense path alternately on recycled buffers
    for j in range(4):
        st, path = ((s, "virtual"), (sb, "dense"))[j % 2]
        lst = make_inverse(A, kernel, st, path, f"alternating {path} {j}")
        mu_held(A.mu_solution_cpp(st["y"], lst["inv"]), st["mu"], f"alternating mu {j}")
        del lst


# ====================================================================== F
@pytest.mark.parametrize("kernel", KERNELS)
def test_nonpd_inverse_in_every_consumer(A, O, kernel):
    """The inverse handle of -I (sigma -5): every consumer returns NaN where
    the reference's outputs are non-finite, none raises, and the next healthy
    call on the context is right.  A numerical outcome, not a device fault."""
    s, p = pred_inputs(O, kernel, "n130", 40)
    n, y, th, sy = 130, s["y"], s["th"], s["sy"]
    Kl = device_kernel(A, kernel, s)
    bad = make_nonpd(A, n)
    inv, ev = bad["inv"], bad["eigenval"]
    assert np.isnan(A.mu_solution_cpp(y, inv))
    with np.errstate(invalid="ignore", divide="ignore"):
        for Kfull in (Kl["full"], A.DMat.upload(C.nonpd_matrix(n))):
            assert np.all(np.isnan(A.stats_cpp(y, Kfull, inv, ev, 0.1, sy)))
            for K in (Kl["elements"], None, A.DMat.upload(s["elements"])):
                st = np.zeros(2)
                g = grad_fn(A, kernel)(y, s["X"], s["Z"], Kfull, K, inv, ev, th, st, 4, sy)
                assert g.shape == th.shape and np.all(np.isnan(g)) and np.all(np.isnan(st))
    Kc = cross_fn(A, kernel)(p["X2"], s["X"], p["Z2"], s["Z"], th, device=True)
    Ks = sym_fn(A, kernel)(p["X2"], p["Z2"], th, device=True)
    got = A.pred_cpp(y, th[0], 0.1, inv, Kc["full"], Ks["full"], 0.3, 1.7)
    for k in ("map", "var", "ci"):
        assert np.all(np.isnan(got[k])), ("pred", k)
    for cubes in ((Kc["elements"], Ks["elements"]),
                  (A.DMat.upload(p["KmxX"]), A.DMat.upload(p["Kmxx"]))):
        got = A.pred_marginal_cpp(y, p["zx"], th[0], 0.1, inv, cubes[0], cubes[1], 0.3, 1.7, 0.8,
                                  True)
        for k in ("map", "var", "ci"):
            assert np.all(np.isnan(got[k])), ("pred_marginal", k)
        for k in ("ate", "att", "atu"):
            assert np.isnan(got[k]["map"]) and np.isnan(got[k]["var"]), k
    # the next healthy calls on the same context, the freed buffers included
    del bad, inv
    lst = make_inverse(A, kernel, s, "virtual", "healthy after non-PD")
    mu_held(A.mu_solution_cpp(y, lst["inv"]), s["mu"], "mu after non-PD")
    grad_held(A, kernel, s, Kl["full"], Kl["elements"], lst["inv"], lst["eigenval"],
              "grad after non-PD")
    pred_held(A, s, p, lst["inv"], Kc["full"], Ks["full"], "pred after non-PD")


# ====================================================================== G
@pytest.mark.parametrize("name", ["B1_p1", "B1_p20"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_single_slice_sequence_through_handles(A, O, kernel, name):
    """B == 1 (Z has no columns; the marginal kernel is slice 0) through the
    whole handle sequence, at p = 1 and p = 20."""
    s, p = pred_inputs(O, kernel, name, 40)
    y, X, Z, th, sy = s["y"], s["X"], s["Z"], s["th"], s["sy"]
    assert Z.shape == (130, 0) and s["elements"].shape == (130, 130, 1)
    Kl = device_kernel(A, kernel, s)
    lst = make_inverse(A, kernel, s, "virtual", "B = 1 inverse")
    lst = A.invkernel_cpp(Kl["full"], th[0])
    inv_held(lst["inv"], s["inv"], "B = 1 inverse of the handle")
    mu_held(A.mu_solution_cpp(y, lst["inv"]), s["mu"], "B = 1 mu")
    grad_held(A, kernel, s, Kl["full"], Kl["elements"], lst["inv"], lst["eigenval"], "B = 1 grad")
    close(A.stats_cpp(y, Kl["full"], lst["inv"], lst["eigenval"], s["mu"], sy),
          O.stats_cpp(y, s["full"], s["inv"], s["eigenval"], s["mu"], sy), check="B = 1 stats")
    Kc = cross_fn(A, kernel)(p["X2"], X, p["Z2"], Z, th, device=True)
    Ks = sym_fn(A, kernel)(p["X2"], p["Z2"], th, device=True)
    pred_held(A, s, p, lst["inv"], Kc["full"], Ks["full"], "B = 1")
    assert not Ks["full"].on_device
    marginal_held(A, s, p, lst["inv"], Kc["elements"], Ks["elements"], "B = 1 virtual cubes")
    assert not Kc["elements"].on_device and not Ks["elements"].on_device
    # a cube of one slice has a matrix's shape
    close(np.asarray(Kl["elements"]), s["elements"][:, :, 0], 1e-12, 1e-12, check="B = 1 cube read")
    close(np.asarray(Kc["elements"]), p["KmxX"][:, :, 0], 1e-12, 1e-12,
          check="B = 1 cross cube read")

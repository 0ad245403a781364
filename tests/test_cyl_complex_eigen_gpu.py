"""es_cyl_complex_eigenfunction and es_cyl_complex_polarisation (C ABI section 16) and CylinderComplex.eigenfunction /
.polarisation against the NumPy restatement tests/cyl_complex_eigen_model.py, DOP853 on complex y, sections 14 / 15, the real
path on the real axis and the roots of the Kelvin-Helmholtz unstable jet.

Bounds: 1e-10 of max|array| per row against the model (the project's figure for a march against its NumPy restatement);
real_eigen_model.bound(N) against DOP853; 1e-12 / 1e-10 of max(|outer|, |inner|) for the identities with section 14 (the
outward RK4 step is the transpose of the determinant's adjoint step: the jump of the flux is D_c to rounding)."""
import ctypes as C

import numpy as np
import pytest

from tests import cyl_complex_eigen_model as cem
from tests.cases import truth_problem
from tests.real_eigen_model import bound

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5
ARRAYS = ("value_int", "flux_int", "value_ext", "flux_ext")


def _np(d):
    return {a: (v.cpu().numpy() if hasattr(v, "cpu") else v) for a, v in d.items()}


def _row_error(got, want):
    """max over the rows of max|got - want| / max|want| (rows of finite `want`)."""
    if want.shape[1] == 0:
        return 0.0
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


# ---- 1. the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", cem.NODE_COUNTS)
@pytest.mark.parametrize("name", cem.NAMES)
def test_eigenfunction_against_model(es_ctx, name, n_nodes):
    from eigensolver_amd import CylinderComplex
    eq, mode, m, window = cem.problems(n_nodes)[name]
    E = cem.CylComplexEigenModel(eq, mode, m)
    c = CylinderComplex(eq, ctx=es_ctx)
    k, w = cem.sample(window, 65, cem.seed_of(name, n_nodes))
    want = E.eigenfunction(k, w, n_ext=37)
    ok = want["status"] == 0
    assert ok.sum() > 32, ok.sum()
    worst = 0.0
    for n, n_ext in ((1, 37), (65, 0), (65, 2), (65, 37)):
        wn = want if n_ext == 37 else E.eigenfunction(k[:n], w[:n], n_ext=n_ext)
        got = _np(c.eigenfunction(mode, k[:n], w[:n], n_ext=n_ext, m=m))
        o = ok[:n]
        assert np.array_equal(got["status"], want["status"][:n]), (name, n_nodes, n)
        assert got["value_int"].shape == (n, n_nodes) and got["x_ext"].shape == (n, n_ext)
        assert np.max(np.abs(got["x_int"] - wn["x_int"])) <= 1e-15
        if n_ext:
            assert np.max(np.abs(got["x_ext"] - wn["x_ext"][:n]) / np.abs(wn["x_ext"][:n, :1])) <= 1e-15
            assert np.all(np.abs(got["x_ext"][:, -1]) == 1.0)
        for a in ARRAYS:
            assert np.all(np.isnan(got[a][~o].real)) and np.all(np.isnan(got[a][~o].imag)), a
            if o.any():
                worst = max(worst, _row_error(got[a][o], wn[a][:n][o]))
    print(f"{name} N={n_nodes}: max |array - model| / max|array| per row = {worst:.3e} ({int(ok.sum())} OK pairs of 65)")
    assert worst < 1e-10
    c.close()


# ---- 2. DOP853 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [130, 500])
@pytest.mark.parametrize("name", cem.NAMES)
def test_interior_against_dop853(es_ctx, name, n_nodes):
    from eigensolver_amd import CylinderComplex
    eq, mode, m, _ = cem.problems(n_nodes)[name]
    E = cem.CylComplexEigenModel(eq, mode, m)
    prob = truth_problem(eq, mode, m)
    c = CylinderComplex(eq, ctx=es_ctx)
    k, w = cem.dop_pairs(name, n_nodes)
    got = _np(c.eigenfunction(mode, k, w, n_ext=0, m=m))
    assert np.all(got["status"] == 0)
    for i in range(2):
        P, xi = E.interior_dop853(prob, k[i], w[i])
        for key, want in (("value_int", P), ("flux_int", xi)):
            err = float(np.max(np.abs(got[key][i] - want)) / np.max(np.abs(want)))
            print(f"{name} N={n_nodes} pair {i} {key}: |gpu - DOP853| / max = {err:.3e} (bound {bound(n_nodes):.1e})")
            assert err < bound(n_nodes)
    c.close()


# ---- 3. consistency with sections 14 / 15 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cem.NAMES)
def test_consistent_with_the_determinant(es_ctx, name):
    from eigensolver_amd import CylinderComplex
    eq, mode, m, window = cem.problems(130)[name]
    c = CylinderComplex(eq, ctx=es_ctx)
    k, w = cem.sample(window, 65, cem.seed_of(name, 130))
    D, st, _, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k, w, m=m, parts=True))
    e = _np(c.eigenfunction(mode, k, w, n_ext=5, m=m))
    assert np.array_equal(e["status"], st)
    ok = st == 0
    assert ok.sum() > 32 and (~ok).any()
    sc = np.maximum(np.abs(outer[ok]), np.abs(inner[ok]))
    fe, fi = e["flux_ext"][ok, -1], e["flux_int"][ok, 0]
    assert np.max(np.abs(fe - outer[ok]) / sc) <= 1e-12
    jump = float(np.max(np.abs((fe - fi) - D[ok]) / sc))
    print(f"{name}: max |flux_ext[-1] - flux_int[0] - D_c| / scale = {jump:.3e}")
    assert jump <= 1e-10
    assert np.max(np.abs(e["value_ext"][ok, -1] - 1.0)) <= 1e-12 and np.max(np.abs(e["value_int"][ok, 0] - 1.0)) <= 1e-12
    for a in ARRAYS:
        assert np.all(np.isnan(e[a][~ok].real)) and np.all(np.isnan(e[a][~ok].imag))
    assert np.all(np.isfinite(e["x_ext"])) and np.all(np.abs(e["x_ext"][:, -1]) == 1.0)
    # a pair that is not OK between OK pairs leaves its neighbours' rows as a call without it gives them, bit for bit
    bad = int(np.flatnonzero(~ok)[0])
    keep = np.flatnonzero(ok)[:6]
    order = np.concatenate((keep[:3], [bad], keep[3:]))
    with_bad = _np(c.eigenfunction(mode, k[order], w[order], n_ext=5, m=m))
    without = _np(c.eigenfunction(mode, k[keep], w[keep], n_ext=5, m=m))
    assert with_bad["status"][3] != 0
    rows = [0, 1, 2, 4, 5, 6]
    for a in ARRAYS + ("x_ext",):
        assert np.array_equal(with_bad[a][rows].view(np.uint64), without[a].view(np.uint64)), a
    c.close()


def test_leaky_pair_between_ok_pairs(es_ctx):
    """Re m_e < 0 (a phase speed above the exterior sound speed): LEAKY, all NaN, the neighbours untouched."""
    from eigensolver_amd import CylinderComplex
    eq, mode, m, _ = cem.problems(130)["flow_kink"]
    c = CylinderComplex(eq, ctx=es_ctx)
    E = cem.CylComplexEigenModel(eq, mode, m)
    k = np.array([1.1, 1.1, 1.1])
    w = np.array([1.1 * 0.3 + 0.05j, 1.1 * 1.6 + 0.05j, 1.1 * 0.35 - 0.04j])
    want = E.eigenfunction(k, w, n_ext=4)
    assert list(want["status"]) == [0, 1, 0]
    got = _np(c.eigenfunction(mode, k, w, n_ext=4, m=m))
    alone = _np(c.eigenfunction(mode, k[[0, 2]], w[[0, 2]], n_ext=4, m=m))
    assert list(got["status"]) == [0, 1, 0]
    for a in ARRAYS:
        assert np.all(np.isnan(got[a][1].real))
        assert np.array_equal(got[a][[0, 2]].view(np.uint64), alone[a].view(np.uint64))
    assert np.all(np.isfinite(got["x_ext"][1]))
    c.close()


# ---- 4. the real axis -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", [("flow_m3", (2.7, 5.6)), ("density_rplus", (0.52, 1.7))])
def test_real_axis_is_the_real_path(es_ctx, name, window):
    from eigensolver_amd import CylinderComplex
    eq, mode, m, _ = cem.problems(130)[name]
    c = CylinderComplex(eq, ctx=es_ctx)
    p = c.problem(mode, m)
    k = np.repeat(cem.K3, 12)
    w = k * np.tile(np.linspace(window[0], window[1], 12), 3)
    sr = p.eval_points(k, w)[1].cpu().numpy()
    ok = sr == 0
    assert ok.sum() >= 8
    k, w = k[ok], w[ok]
    real = _np(p.eigenfunction(k, w, n_ext=9))
    e = _np(c.eigenfunction(mode, k, w + 0j, n_ext=9, m=m))
    assert np.all(e["status"] == 0)
    sign = np.sign(real["value_ext"][:, -1])[:, None]           # the real path keeps the sign of P_e(boundary)
    assert np.all(np.abs(sign) == 1.0)
    worst = 0.0
    for a in ARRAYS:
        scale = np.max(np.abs(real[a]), axis=1, keepdims=True)
        worst = max(worst, float(np.max(np.abs(e[a].real - sign * real[a]) / scale)))
        assert np.max(np.abs(e[a].imag) / scale) <= 1e-13, a
    print(f"{name}: max |Re complex - sign * real| / max|row| over P, xi_r = {worst:.3e} ({int(ok.sum())} pairs)")
    assert worst <= 1e-10
    if eq.x_boundary > 0:
        polr = _np(p.polarisation(k, w, n_ext=9))
        polc = _np(c.polarisation(mode, k, w + 0j, n_ext=9, m=m))
        assert np.array_equal(polc["radius"], polr["radius"])
        scale = np.max(np.abs(polr["amp"]), axis=2, keepdims=True)
        err = float(np.max(np.abs(polc["amp"].real - sign[:, :, None] * polr["amp"]) / scale))
        print(f"{name}: max |Re amp - sign * section 7| / max|channel| = {err:.3e}")
        assert err <= 1e-10 and np.max(np.abs(polc["amp"].imag) / scale) <= 1e-13
    c.close()


# ---- 5. the unstable jet ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jet_roots(es_ctx):
    """CylinderComplex of the jet (r_sign = +1, N = 130) and the accepted root of find_roots next to each entry of JET_ROOTS:
    (c, [(mode, k, w, resid percent)])."""
    from eigensolver_amd import CylinderComplex
    c = CylinderComplex(cem.jet(130), ctx=es_ctx)
    found = []
    for mode, k, w0 in cem.JET_ROOTS:
        w_re = w0.real + np.linspace(-0.05, 0.07, 7)          # the root inside a cell, away from its edges
        w_im = w0.imag + np.linspace(-0.025, 0.035, 5)
        D, st, _ = c.eval_grid(mode, [k], w_re, w_im)
        roots, _ = c.find_roots(mode, [k], w_re, w_im, D, st)
        flag = roots["flag"].cpu().numpy() == 1
        ws, resid = roots["w"].cpu().numpy()[flag], roots["resid"].cpu().numpy()[flag]
        assert len(ws), (mode, k)
        i = int(np.argmin(np.abs(ws - w0)))
        found.append((mode, k, complex(ws[i]), float(resid[i])))
    yield c, found
    c.close()


def test_unstable_jet_roots_and_their_eigenfunctions(jet_roots):
    c, found = jet_roots
    for (mode, k, w, resid), (_, _, w0) in zip(found, cem.JET_ROOTS):
        assert abs(w - w0) < 1e-6, (mode, k, w)
        e = _np(c.eigenfunction(mode, [k], [w], n_ext=50))
        assert e["status"][0] == 0
        xi = np.concatenate((e["flux_int"][0], e["flux_ext"][0]))
        jump = abs(e["flux_ext"][0, -1] - e["flux_int"][0, 0]) / np.max(np.abs(xi))
        print(f"jet {mode} k={k}: w = {w:.6f}, resid {resid:.2e} %, xi_r jump / max|xi_r| = {jump:.2e}")
        # resid is 100 |D_c| / max(|outer|, |inner|) of section 14 and max|xi_r| is at least that scale; the jump is that D_c
        # to the 1e-10 of the scale of test_consistent_with_the_determinant.  The allowance matters: the secant iteration
        # converges to rounding (resid 9.6e-16 % measured, jump 3.5e-16), where the two evaluations of D_c differ in their last bits
        assert jump <= resid / 100.0 + 1e-10
        if mode == "kink":                                    # P(axis node) = bc_const_raw xi_e; bc_const is 0 here
            assert abs(e["value_int"][0, -1]) <= 1e-15 * np.max(np.abs(e["value_int"][0]))
        assert np.argmax(np.abs(e["value_ext"][0])) == 49     # the exterior decays away from the boundary


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_calls(es_ctx):
    import torch
    from eigensolver_amd import CylinderComplex, ShootProblem, _lib, equilibrium as q
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    c = CylinderComplex(cem.jet(11), ctx=es_ctx)
    p = c.problem("kink")
    slab = ShootProblem(q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=11), "kink", ctx=es_ctx)
    N, n_ext, n = 11, 3, 2
    P = _lib.ptr
    k = torch.full((n,), 1.1, dtype=torch.float64, device=dev)
    wre, wim = torch.full((n,), 1.5, dtype=torch.float64, device=dev), torch.full((n,), 0.03, dtype=torch.float64, device=dev)
    full = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)   # noqa: E731
    vi, fi, xe, ve, fe = full(n, N, 2), full(n, N, 2), full(n, n_ext), full(n, n_ext, 2), full(n, n_ext, 2)
    st = torch.full((n,), 9, dtype=torch.uint8, device=dev)

    def call(prob=p.handle, n_=n, n_ext_=n_ext, k_=P(k), wim_=P(wim), vi_=P(vi), xe_=P(xe), st_=P(st)):
        return lib.es_cyl_complex_eigenfunction(h, prob, k_, P(wre), wim_, n_, vi_, P(fi), n_ext_, xe_, P(ve), P(fe), st_)
    assert call(prob=slab.handle) == UNSUPPORTED
    for bad in (dict(prob=None), dict(n_=-1), dict(n_ext_=-1), dict(n_ext_=1), dict(k_=None), dict(wim_=None), dict(vi_=None),
                dict(xe_=None)):
        assert call(**bad) == INVALID, bad
    assert call(n_=0, k_=None, vi_=None, xe_=None, st_=None) == 0
    es_ctx.synchronize()
    assert all(bool((a == -7.0).all()) for a in (vi, fi, xe, ve, fe)) and bool((st == 9).all())
    assert call(st_=None) == 0                                # the status array is optional
    es_ctx.synchronize()
    assert all(bool((a != -7.0).all()) for a in (vi, fi, xe, ve, fe)) and bool((st == 9).all())
    with_status = [a.clone() for a in (vi, fi, ve, fe)]
    assert call() == 0
    es_ctx.synchronize()
    assert bool((st == 0).all())
    assert all(torch.equal(a, b) for a, b in zip(with_status, (vi, fi, ve, fe)))
    # polarisation: the checks of section 7, and the imaginary parts
    prof = {a: torch.ones(N, dtype=torch.float64, device=dev) for a in _lib._FIELD_PROFILE_FIELDS}
    fp = _lib.FieldProfiles(*[prof[a].data_ptr() for a in _lib._FIELD_PROFILE_FIELDS])
    radius, amp = full(n, N + n_ext), full(n, 7, N + n_ext, 2)

    def pol(n_=n, N_=N, n_ext_=n_ext, k_=P(k), wim_=P(wim), vi_=P(vi), xe_=P(xe), fp_=C.byref(fp), m=1, flags=0, rad=P(radius),
            amp_=P(amp)):
        return lib.es_cyl_complex_polarisation(h, k_, P(wre), wim_, n_, N_, vi_, P(fi), n_ext_, xe_, P(ve), P(fe), fp_, m, 0.2,
                                               5.0, 0.5, 0.49, flags, rad, amp_)
    for bad in (dict(n_=-1), dict(N_=-1), dict(n_ext_=-1), dict(k_=None), dict(wim_=None), dict(vi_=None), dict(xe_=None),
                dict(fp_=None), dict(m=-1), dict(flags=8), dict(rad=None), dict(amp_=None)):
        assert pol(**bad) == INVALID, bad
    assert pol(n_=0, k_=None, rad=None, amp_=None) == 0 and pol(N_=0, n_ext_=0) == 0
    es_ctx.synchronize()
    assert bool((radius == -7.0).all()) and bool((amp == -7.0).all())
    assert pol() == 0
    es_ctx.synchronize()
    assert bool((radius != -7.0).all()) and bool((amp != -7.0).all())
    # the Python layer: positive radii only
    neg = CylinderComplex(q.CylinderFlow(**cem.KH, width=1.5, n_nodes=11), ctx=es_ctx)
    for f in (lambda: neg.polarisation("kink", [1.1], [1.5 + 0.03j], n_ext=4),
              lambda: neg.fields("kink", 1.1, 1.5 + 0.03j, [0.0, 1.0], [0.0], [0.0])):
        with pytest.raises(ValueError, match=r"r_sign=\+1"):
            f()
    assert _np(neg.eigenfunction("kink", [1.1], [1.5 + 0.03j], n_ext=4))["status"][0] == 0     # both signs of r are accepted
    neg.close()
    slab.close()
    c.close()

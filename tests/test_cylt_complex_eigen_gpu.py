"""es_cylt_complex_eigenfunction (C ABI section 19) and RotatingCylinderComplex.eigenfunction against the NumPy restatement
tests/cylt_complex_eigen_model.py, section 17, the real path on the real axis, the untwisted kernels in the zero-twist limit
and the unstable m = 3 root of case A.

Bounds: 1e-10 of max|array| per row against the model (the project's figure for a march against its NumPy restatement);
1e-12 of max(|outer|, |inner|) for the boundary values and the exterior flux; the jump of the flux against D_c of section 17
within 1e-10 of that scale where the axis target is zero (sausage, zero twist) and within 4 x the model's
boundary_flux_spread + 1e-10 otherwise (the factor 4 of real_eigen_model.boundary_flux_spread).  Every figure is printed
before it is asserted."""
import numpy as np
import pytest

from tests import cyl_complex_eigen_model as cem
from tests import cylt_complex_eigen_model as tem

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5
ARRAYS = ("value_int", "flux_int", "value_ext", "flux_ext")
COUNTS = ((1, 16), (65, 0), (65, 2), (130, 16))                   # (pairs, n_ext): one lane, a ragged wave, three workgroups


def _np(d):
    return {a: (v.cpu().numpy() if hasattr(v, "cpu") else v) for a, v in d.items()}


def _row_error(got, want):
    """max over the rows of max|got - want| / max|want| (rows of finite `want`)."""
    if want.shape[1] == 0:
        return 0.0
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


def solver(es_ctx, name, n_nodes):
    """RotatingCylinderComplex of a problem of the model's list, its cached problem carrying the problem's accept_norm."""
    from eigensolver_amd import RotatingCylinderComplex, ShootProblem
    eq, mode, m, an, _, _ = tem.problems(n_nodes)[name]
    c = RotatingCylinderComplex(eq, ctx=es_ctx)
    if an:
        key = (mode, (1 if mode == "kink" else 0) if m is None else int(m))
        c._problems[key] = ShootProblem(eq, mode, m=key[1], ctx=es_ctx, accept_norm=1)
    return c, mode, m


def leaky_pair(M):
    """A (k, omega) pair off the real axis whose status is ES_PT_LEAKY in the model: Re omega / k beyond every exterior speed."""
    k, w = 1.0, 2.4 + 0.05j
    assert M.eval(k, [w])[4][0] == 1
    return k, w


# ---- 1. the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", tem.NODE_COUNTS)
@pytest.mark.parametrize("name", tem.NAMES)
def test_eigenfunction_against_model(es_ctx, name, n_nodes):
    """Every array within 1e-10 of max|array| per row, statuses identical, x_int / x_ext to 1e-15, a leaky pair placed by hand
    between OK pairs NaN with its neighbours untouched.  Measured on the MI355X, worst over the four calls and the three node
    counts, value_int / flux_int: sausage 7e-16 / 1e-15, reference 9e-16 / 2e-15, A 4e-15 / 2e-15, C 6e-14 / 3e-14, B 9e-14 /
    9e-14; the exterior arrays at 2e-15 or below."""
    E = tem.model_of(name, n_nodes)
    c, mode, m = solver(es_ctx, name, n_nodes)
    k, w = tem.pairs(name, n_nodes, 130)
    assert (w.imag > 0).any() and (w.imag < 0).any() and len(np.unique(k)) == 130
    st0 = E.M.eval_points(k, w)[4]
    L = next(j for j in range(1, 60) if st0[j - 1] == 0 and st0[j] == 0 and st0[j + 1] == 0)
    k_ok, w_ok = k[L], w[L]
    k[L], w[L] = leaky_pair(E.M)                                 # a leaky lane placed by hand between OK lanes
    worst = {a: 0.0 for a in ARRAYS}
    for n, n_ext in COUNTS:
        want = E.eigenfunction(k[:n], w[:n], n_ext=n_ext)
        ok = want["status"] == 0
        if n > 1:
            assert ok.sum() >= n // 2 and want["status"][L] == 1 and ok[L - 1] and ok[L + 1]
        got = _np(c.eigenfunction(mode, k[:n], w[:n], n_ext=n_ext, m=m))
        assert np.array_equal(got["status"], want["status"]), (name, n_nodes, n)
        assert got["value_int"].shape == (n, n_nodes) and got["x_ext"].shape == (n, n_ext)
        assert np.max(np.abs(got["x_int"] - want["x_int"])) <= 1e-15
        if n_ext:
            assert np.max(np.abs(got["x_ext"] - want["x_ext"]) / np.abs(want["x_ext"][:, :1])) <= 1e-15
            assert np.all(np.abs(got["x_ext"][:, -1]) == 1.0)
        for a in ARRAYS:
            assert np.all(np.isnan(got[a][~ok].real)) and np.all(np.isnan(got[a][~ok].imag)), a
            if ok.any():
                worst[a] = max(worst[a], _row_error(got[a][ok], want[a][ok]))
    # the neighbours of the leaky lane: bit for bit what they are with an OK lane in its place
    k2, w2 = k[:65].copy(), w[:65].copy()
    k2[L], w2[L] = k_ok, w_ok
    a_ = _np(c.eigenfunction(mode, k[:65], w[:65], n_ext=2, m=m))
    b_ = _np(c.eigenfunction(mode, k2, w2, n_ext=2, m=m))
    assert a_["status"][L] == 1 and b_["status"][L] == 0
    for a in ARRAYS:
        assert np.all(np.isnan(a_[a][L].real)) and np.all(np.isfinite(b_[a][L]))
        for j in (L - 1, L + 1):
            assert a_[a][j].tobytes() == b_[a][j].tobytes(), (name, n_nodes, a, j)
    print(f"{name} N={n_nodes}: max |array - model| / max|array| per row: "
          + ", ".join(f"{a} {worst[a]:.3e}" for a in ARRAYS) + " (bound 1e-10)")
    c.close()
    assert max(worst.values()) < 1e-10


# ---- 2. consistency with section 17 -----------------------------------------------------------------------------------------
_CONSISTENCY = {}


def consistency(es_ctx, name):
    """The 65-pair sample of a problem at N = 130 through eval_points and eigenfunction, and the model's figures for it; computed
    once per problem and shared by the three tests below, which do not modify it."""
    if name not in _CONSISTENCY:
        E = tem.model_of(name, 130)
        c, mode, m = solver(es_ctx, name, 130)
        k, w = tem.pairs(name, 130)
        D, st, _, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k, w, m=m, parts=True))
        e = _np(c.eigenfunction(mode, k, w, n_ext=16, m=m))
        c.close()
        want = E.eigenfunction(k, w, n_ext=16)
        assert np.array_equal(e["status"], st) and np.array_equal(st, want["status"])
        ok = st == 0
        assert ok.sum() >= 33
        sc = np.maximum(np.abs(outer[ok]), np.abs(inner[ok]))
        spread = np.abs(want["inner_outward"][ok] - want["inner"][ok]) / sc           # boundary_flux_spread of these pairs
        _CONSISTENCY[name] = dict(e=e, want=want, ok=ok, sc=sc, D=D[ok], outer=outer[ok], spread=spread)
    return _CONSISTENCY[name]


@pytest.mark.parametrize("name", tem.ALL_NAMES)
def test_boundary_values(es_ctx, name):
    """flux_ext[:, -1] = outer of eval_points, value_ext[:, -1] = 1 and value_int[:, 0] = 1, each at 1e-12.  Measured (N = 130,
    65-pair sample): the exterior figures are 0 and |value_int[:, 0] - 1| is 2.3e-16 on every problem -- b = 1 / P(g_0) imposes
    it and the part marched inwards has no P at the boundary.  (Formed as section 16 forms it, by a march of the axis state
    target e + beta d, the same figure was 3e-12, 2e-9 and 2e-7 on B, A and C: DESIGN.md section 8n.)"""
    r = consistency(es_ctx, name)
    e, ok, sc = r["e"], r["ok"], r["sc"]
    outer = float(np.max(np.abs(e["flux_ext"][ok, -1] - r["outer"]) / sc))
    v_ext = float(np.max(np.abs(e["value_ext"][ok, -1] - 1.0)))
    v_int = float(np.max(np.abs(e["value_int"][ok, 0] - 1.0)))
    print(f"{name}: |flux_ext[-1] - outer| / scale = {outer:.3e}, |value_ext[-1] - 1| = {v_ext:.3e}, |value_int[0] - 1| = "
          f"{v_int:.3e} (bounds 1e-12); {int(ok.sum())} OK pairs")
    for a in ARRAYS:
        assert np.all(np.isnan(e[a][~ok].real)) and np.all(np.isnan(e[a][~ok].imag))
    assert np.all(np.isfinite(e["x_ext"])) and np.all(np.abs(e["x_ext"][:, -1]) == 1.0)
    assert outer <= 1e-12 and v_ext <= 1e-12
    assert v_int <= 1e-12


@pytest.mark.parametrize("name", tem.ALL_NAMES)
def test_jump_of_the_flux_against_the_determinant(es_ctx, name):
    """Jump - D_c within 1e-10 of the scale where the axis target is zero, within 4 x boundary_flux_spread + 1e-10 otherwise.
    Measured: sausage 1.4e-16, zero twist 2.1e-16; A 2.1e-6, B 2.7e-5, C 1.2e-7, reference 1.7e-4, each the model's spread of the
    pair to three digits (0.25 of what is allowed)."""
    r = consistency(es_ctx, name)
    e, ok, sc = r["e"], r["ok"], r["sc"]
    jump_err = np.abs((e["flux_ext"][ok, -1] - e["flux_int"][ok, 0]) - r["D"]) / sc
    allowed = 1e-10 + (0.0 if name in ("sausage", tem.ZERO_TWIST) else 4.0) * r["spread"]
    print(f"{name}: max |jump - D_c| / scale = {np.max(jump_err):.3e}, worst model spread {np.max(r['spread']):.3e}, "
          f"max (|jump - D_c| / allowed) = {np.max(jump_err / allowed):.3f}")
    assert np.all(jump_err <= allowed)


@pytest.mark.parametrize("name", tem.ALL_NAMES)
def test_jump_of_the_flux_is_the_models(es_ctx, name):
    """The GPU's jump equals the model's jump at 1e-10 of the scale.  Measured: 1.1e-15 to 1.7e-15 on the six problems."""
    r = consistency(es_ctx, name)
    e, want, ok, sc = r["e"], r["want"], r["ok"], r["sc"]
    jump = e["flux_ext"][ok, -1] - e["flux_int"][ok, 0]
    jump_model = want["flux_ext"][ok, -1] - want["flux_int"][ok, 0]
    err = float(np.max(np.abs(jump - jump_model) / sc))
    print(f"{name}: |jump - model's jump| / scale = {err:.3e} (bound 1e-10)")
    assert err <= 1e-10


# ---- 3. the real axis -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sausage", "reference"])
def test_real_axis_is_the_real_path(es_ctx, name):
    """Im omega = 0, pairs OK on both paths: the arrays of ShootProblem.eigenfunction times sign(P_e(boundary)).
    The problems: B has no pair in its window that is OK on the real path (the window lies in the continuum of the rotating
    flow: its roots exist off the axis only), and on A and C (m = 3, 4) the real path's own march of the axis state keeps only
    8 and 6 digits, so it is no yardstick at 1e-10 there.  Both paths solve the same discrete
    problem, the real path by a march of the axis state, this one in two directions.  Measured: sausage 5.5e-15 on 36 pairs,
    reference 3.1e-13 on 24; imaginary parts exactly 0."""
    c, mode, m = solver(es_ctx, name, 130)
    p = c.problem(mode, m)
    _, _, _, _, W, _ = tem.problems(130)[name]
    k = np.repeat(np.array([0.7, 1.1, 1.9]), 12)
    w = k * np.tile(np.linspace(W[0], W[1], 12), 3)
    sr = p.eval_points(k, w)[1].cpu().numpy()
    sc_ = c.eval_points(mode, k, w + 0j, m=m)[1].cpu().numpy()
    ok = (sr == 0) & (sc_ == 0)
    assert ok.sum() >= 8
    k, w = k[ok], w[ok]
    real = _np(p.eigenfunction(k, w, n_ext=9))
    e = _np(c.eigenfunction(mode, k, w + 0j, n_ext=9, m=m))
    c.close()
    assert np.all(e["status"] == 0)
    sign = np.sign(real["value_ext"][:, -1])[:, None]           # the real path keeps the sign of P_e(boundary)
    assert np.all(np.abs(sign) == 1.0)
    worst = worst_im = 0.0
    for a in ARRAYS:
        scale = np.max(np.abs(real[a]), axis=1, keepdims=True)
        worst = max(worst, float(np.max(np.abs(e[a].real - sign * real[a]) / scale)))
        worst_im = max(worst_im, float(np.max(np.abs(e[a].imag) / scale)))
    print(f"{name}: max |Re complex - sign * real| / max|row| over P, xi_r = {worst:.3e} (bound 1e-10), max |Im| / max|row| = "
          f"{worst_im:.3e} (bound 1e-13), {int(ok.sum())} pairs")
    assert worst <= 1e-10 and worst_im <= 1e-13


# ---- 4. the zero-twist limit ------------------------------------------------------------------------------------------------
def test_zero_twist_limit_is_the_untwisted_kernel(es_ctx):
    """v_phi = B_phi = 0 through the twisted coefficient set, the full-shape step and the two-direction solve:
    es_cyl_complex_eigenfunction on the same jet, to rounding (measured 2.2e-15 on 66 pairs)."""
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, equilibrium as q
    ct = RotatingCylinderComplex(tem.twisted_jet(**tem.JET, n_nodes=130), ctx=es_ctx)
    c0 = CylinderComplex(q.CylinderFlow(**tem.JET, n_nodes=130), ctx=es_ctx)
    k, w = tem.pairs(tem.ZERO_TWIST, 130)
    k, w = np.append(k, 2.0), np.append(w, tem.JET_ROOT)
    et, e0 = _np(ct.eigenfunction("kink", k, w, n_ext=16)), _np(c0.eigenfunction("kink", k, w, n_ext=16))
    ct.close()
    c0.close()
    assert np.array_equal(et["status"], e0["status"])
    ok = e0["status"] == 0
    assert ok.sum() >= 33 and ok[-1]
    worst = max(_row_error(et[a][ok], e0[a][ok]) for a in ARRAYS)
    print(f"zero twist: max |twisted - untwisted| / max|array| per row = {worst:.3e} on {int(ok.sum())} pairs (bound 1e-10)")
    assert worst <= 1e-10
    assert np.array_equal(et["x_ext"], e0["x_ext"]) and np.array_equal(et["x_int"], e0["x_int"])


# ---- 5. the unstable root of case A -------------------------------------------------------------------------------------------
def test_unstable_root_of_case_a(es_ctx):
    from tests.cylt_complex_model import root_cases
    from eigensolver_amd import RotatingCylinderComplex
    eq, m, krow, w_re, w_im, quoted = root_cases(130)["A"]
    c = RotatingCylinderComplex(eq, ctx=es_ctx)
    D, st, _ = c.eval_grid("kink", krow, w_re, w_im, m=m)
    roots, _ = c.find_roots("kink", krow, w_re, w_im, D, st, m=m)
    flag = roots["flag"].cpu().numpy() == 1
    ws, resid = roots["w"].cpu().numpy()[flag], roots["resid"].cpu().numpy()[flag]
    assert len(ws)
    i = int(np.argmin(np.abs(ws - quoted)))
    k, w, resid = float(krow[0]), complex(ws[i]), float(resid[i])
    assert abs(w - quoted) < 1e-6 and w.imag > 0
    _, _, _, outer, inner = (t.cpu().numpy() for t in c.eval_points("kink", [k], [w], m=m, parts=True))
    e = _np(c.eigenfunction("kink", [k], [w], n_ext=16, m=m))
    c.close()
    assert e["status"][0] == 0
    sc = max(abs(outer[0]), abs(inner[0]))
    jump = abs(e["flux_ext"][0, -1] - e["flux_int"][0, 0]) / sc
    spread = float(tem.boundary_flux_spread("A", np.array([k]), np.array([w]), 130)[0]) / sc
    print(f"case A: w = {w:.7f}, resid {resid:.2e} %, jump of xi_r / scale = {jump:.3e}, model spread / scale = {spread:.3e}")
    # resid is 100 |D_c| / scale of section 17; the jump is that D_c to the spread of the two marches
    assert jump <= resid / 100.0 + 4.0 * spread + 1e-10
    assert np.argmax(np.abs(e["value_ext"][0])) == 15             # the exterior decays away from the boundary
    assert np.all(np.isfinite(e["value_int"])) and np.all(np.isfinite(e["flux_int"]))


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_calls(es_ctx):
    import torch
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, ShootProblem, _lib, equilibrium as q
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    c = RotatingCylinderComplex(q.CylinderRotation(v_twist=2.0, power=1.0, r_axis=1e-2, n_nodes=11), ctx=es_ctx)
    p = c.problem("kink", 3)
    slab = ShootProblem(q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=11), "kink", ctx=es_ctx)
    untw = CylinderComplex(cem.jet(11), ctx=es_ctx)
    pu = untw.problem("kink")
    N, n_ext, n = 11, 3, 2
    P = _lib.ptr
    k = torch.full((n,), 1.0, dtype=torch.float64, device=dev)
    wre, wim = torch.full((n,), 1.5, dtype=torch.float64, device=dev), torch.full((n,), 0.7, dtype=torch.float64, device=dev)
    full = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)   # noqa: E731
    vi, fi, xe, ve, fe = full(n, N, 2), full(n, N, 2), full(n, n_ext), full(n, n_ext, 2), full(n, n_ext, 2)
    st = torch.full((n,), 9, dtype=torch.uint8, device=dev)

    def call(prob=p.handle, n_=n, n_ext_=n_ext, k_=P(k), wim_=P(wim), vi_=P(vi), xe_=P(xe), st_=P(st), f=None):
        f = f or lib.es_cylt_complex_eigenfunction
        return f(h, prob, k_, P(wre), wim_, n_, vi_, P(fi), n_ext_, xe_, P(ve), P(fe), st_)
    assert call(prob=slab.handle) == UNSUPPORTED
    assert call(prob=pu.handle) == UNSUPPORTED                                # the untwisted cylinder has section 16
    assert call(f=lib.es_cyl_complex_eigenfunction) == UNSUPPORTED            # which keeps refusing twisted problems
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
    slab.close()
    untw.close()
    c.close()

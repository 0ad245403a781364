"""Results must not depend on the unit system, GPU leg: every comparison is the HIP kernels at the reference's normalised
units against the same kernels on inputs rescaled by exact powers of two (V = 2^pv on speeds, R = 4^pr on densities),
through unit_scaling.assert_scaled -- exact equality of the float64 bit patterns after LAW's exponent shift, never a
tolerance.  (3, 0) is the control: a failure there is no matter of range.

Restrictions, each with the formula that causes it:
  * the flow slab with shear (SFG_*, and SlabComplexFlow on a sheared profile) goes under the density scale only: the
    reference's D(x), flow_multiprocessor_coronal.py:423, adds Omega^2 - k^2 cT^2 to a term without dimension of speed
    (coef_pre<FAM_SLABF>: G = S t^2 + k^4 cT^2 c^2); see test_unit_scaling_cpu.py.
"""
import numpy as np
import pytest

from tests import unit_scaling as us
from tests.cases import all_cases

pytestmark = pytest.mark.gpu

SCALES = [(3, 0), (20, 0), (-20, 0), (0, 20), (0, -20), (7, -13)]
DENSITY_ONLY = [(0, 20), (0, -20)]
CASES = all_cases()
N_BISECT = 30
PT_UNSURE = 0x80


def _scales_of(name):
    return DENSITY_ONLY if name.startswith("SFG_") else SCALES


def _pairs(names):
    out = [(n, pv, pr) for n in names for pv, pr in _scales_of(n)]
    return pytest.mark.parametrize("name,pv,pr", out, ids=[f"{n}-V{pv}-R{pr}" for n, pv, pr in out])


def _np(x):
    if isinstance(x, dict):
        return {a: _np(b) for a, b in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(_np(b) for b in x) if not hasattr(x, "_fields") else type(x)(*[_np(b) for b in x])
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def _problem(ctx, name, pv, pr):
    eq, mode, m, _ = CASES[name]
    return us.ScaledShootProblem(eq, mode, m, ctx=ctx, pv=pv, pr=pr)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- (a) fp64 grid and search ------------------------------------------------------------------------------------------
def _fp64(ctx, name, pv, pr, nk=6, nw=96):
    """Everything group (a) compares, as host arrays, at the units (pv, pr)."""
    import torch
    from eigensolver_amd import shooting as s

    def run():
        gp = _problem(ctx, name, pv, pr)
        k, W = us.grid_of(CASES[name], nk, nw)
        Ws = np.ldexp(W, pv)
        out = {"fam": us.family(gp.desc.geometry), "k": k, "Ws": Ws}
        D, st, rel = gp.eval_grid(k, Ws, want_rel=True)
        out["grid"] = _np((D, st, rel))
        out["grid_skip"] = _np(gp.eval_grid(k, Ws, want_rel=True, skip_continuum=True))
        kk = np.repeat(k, nw)
        out["points"] = _np(gp.eval_points(kk, (k[:, None] * Ws[None, :]).ravel(), want_rel=True))
        rule = ctx.refine_rule
        try:
            for label, r in (("section", s.REFINE_SECTION), ("hybrid", s.REFINE_HYBRID)):
                ctx.refine_rule = r
                out["roots_" + label] = _np(gp.find_roots(k, Ws, D, st, n_bisect=N_BISECT))
            ctx.refine_rule = s.REFINE_SECTION
            table = gp.alloc_root_table(1024)
            count = torch.zeros(1, dtype=torch.int32, device=D.device)
            t = gp.find_roots_async(k, Ws, D, st, table, count, n_bisect=N_BISECT)
            n = int(count.item())
            assert n <= 1024
            out["roots_async"] = ({a: b[:n].cpu().numpy() for a, b in t.items()}, n)
        finally:
            ctx.refine_rule = rule
        gp.close()
        return out

    return _cached(("fp64", name, pv, pr, nk, nw), run)


def _check_grid(ref, got, fam, pv, pr, what):
    (D0, st0, rel0), (D1, st1, rel1) = ref, got
    us.assert_same(st0, st1, what + ".status")
    ok = st0 == 0
    us.assert_scaled(D0, D1, *us.LAW[fam]["D"], pv, pr, ok=ok, what=what + ".D")
    us.assert_scaled(rel0, rel1, *us.LAW[fam]["rel"], pv, pr, ok=ok, what=what + ".rel")


def _check_fp64(ref, got, pv, pr):
    fam = ref["fam"]
    for what in ("grid", "grid_skip", "points"):
        _check_grid(ref[what], got[what], fam, pv, pr, what)
    for what in ("roots_section", "roots_hybrid", "roots_async"):
        assert ref[what][1] > 0 and np.count_nonzero(ref[what][0]["flag"] == 1) > 0, what
        us.assert_root_table_scaled(ref[what], got[what], pv, pr, fam, what)


FP64_CASES = ["CF_flow_kink", "CF_flow_m3", "CDC_w095_sausage", "CDP_kink", "CR_kink", "CR_sausage", "SD_w15_kink",
              "SFU_sausage", "SFG_flow_kink"]


@_pairs(FP64_CASES)
def test_fp64_grid_and_search(es_ctx, name, pv, pr):
    """eval_grid with and without skip_continuum, eval_points on the flattened grid, find_roots under REFINE_SECTION and
    REFINE_HYBRID, find_roots_async: statuses, rows, flags and counts equal, D / rel / w by LAW, exactly."""
    _check_fp64(_fp64(es_ctx, name, 0, 0), _fp64(es_ctx, name, pv, pr), pv, pr)


@pytest.mark.parametrize("pv,pr", SCALES, ids=[f"V{pv}-R{pr}" for pv, pr in SCALES])
def test_fp64_ragged_rows_nw700(es_ctx, pv, pr):
    """CF_flow_kink, 4 k-rows of 700 frequencies: ragged, and the two-rows-per-workgroup kernel where that applies."""
    _check_fp64(_fp64(es_ctx, "CF_flow_kink", 0, 0, 4, 700), _fp64(es_ctx, "CF_flow_kink", pv, pr, 4, 700), pv, pr)


# ---- (b) fp32 screening ------------------------------------------------------------------------------------------------
def _screen(ctx, name, pv, pr):
    def run():
        gp = _problem(ctx, name, pv, pr)
        k, W = us.grid_of(CASES[name])
        Ws = np.ldexp(W, pv)
        out = {"screen": _np(gp.screen_grid(k, Ws))}
        t, cnt, Dm, stm, stats = gp.find_roots_mixed(k, Ws, n_bisect=N_BISECT)
        out["mixed"] = (_np(t), cnt)
        out["stats"] = stats
        a = gp.audit_screening(k, Ws)
        out["audit"] = (a.missed, a.false, a.status, a.sign)
        gp.close()
        return out

    return _cached(("screen", name, pv, pr), run)


SCREEN_CASES = ["CF_flow_kink", "CDC_w095_kink", "CR_kink", "CR_sausage", "SD_w15_kink", "SFU_sausage"]


@_pairs(SCREEN_CASES)
def test_fp32_screening(es_ctx, name, pv, pr):
    """screen_grid alone: statuses identical INCLUDING the ES_PT_SCREEN_UNSURE bit, D at vouched-for points by LAW.
    find_roots_mixed: its table is the fp64 table of the same units bit for bit, no unconfirmed bracket, as many fp64
    re-evaluations of unsure points as at reference units.  audit_screening at the scaled units: nothing missed, nothing
    false, no wrong status, no wrong sign."""
    ref, got = _screen(es_ctx, name, 0, 0), _screen(es_ctx, name, pv, pr)
    f64 = _fp64(es_ctx, name, pv, pr)
    fam = f64["fam"]
    (D0, st0), (D1, st1) = ref["screen"], got["screen"]
    print(f"{name} V=2^{pv} R=4^{pr}: unsure {np.count_nonzero(st0 & PT_UNSURE)} -> {np.count_nonzero(st1 & PT_UNSURE)}, "
          f"stats {ref['stats']} -> {got['stats']}, audit {got['audit']}")
    us.assert_same(st0, st1, "screen.status")
    us.assert_scaled(D0, D1, *us.LAW[fam]["D"], pv, pr, ok=st0 == 0, what="screen.D")
    (tm, cm), (t64, c64) = got["mixed"], f64["roots_section"]
    assert cm == c64
    for col in ("k", "w", "w_lo", "w_hi", "resid", "row", "flag"):
        assert np.array_equal(tm[col].view(np.uint8), t64[col].view(np.uint8)), f"mixed.{col} is not the fp64 table"
    assert got["stats"][2] == 0, got["stats"]
    assert got["stats"][0] == ref["stats"][0], (ref["stats"], got["stats"])
    assert got["audit"] == (0, 0, 0, 0), got["audit"]


# ---- (c) jets and Newton, (d) eigenfunctions and labels --------------------------------------------------------------------
def _roots_of(ctx, name, pv, limit=None):
    """The accepted roots of group (a) at reference units, in the units V = 2^pv: (k, w)."""
    t, _ = _fp64(ctx, name, 0, 0)["roots_section"]
    sel = np.flatnonzero(t["flag"] == 1)[:limit]
    return t["k"][sel].copy(), np.ldexp(t["w"][sel], pv)


def _jets(ctx, name, pv, pr):
    def run():
        gp = _problem(ctx, name, pv, pr)
        k, w = _roots_of(ctx, name, pv)
        _, w0 = _roots_of(ctx, name, 0)
        sl = gp.root_slopes(k, w)
        out = {"slopes": _np((sl.outer, sl.inner, sl.d, sl.d_w, sl.d_k, sl.status)),
               "cg": _np(gp.group_velocity({"k": k, "w": w})),
               "newton": _np(gp.newton(k, np.ldexp(w0 * (1.0 + 1e-4), pv)))}
        gp.close()
        return out

    return _cached(("jets", name, pv, pr), run)


@_pairs(["CF_flow_kink", "CR_kink", "SD_w15_kink"])
def test_jets_and_newton(es_ctx, name, pv, pr):
    """root_slopes (D, D_w, D_k and the two sides), group_velocity and newton from w (1 + 1e-4) at the roots of (a)."""
    ref, got = _jets(es_ctx, name, 0, 0), _jets(es_ctx, name, pv, pr)
    fam = _fp64(es_ctx, name, 0, 0)["fam"]
    law = us.LAW[fam]
    o0, i0, d0, dw0, dk0, st0 = ref["slopes"]
    o1, i1, d1, dw1, dk1, st1 = got["slopes"]
    us.assert_same(st0, st1, "slopes.status")
    assert np.all(st0 == 0) and st0.size > 0
    for r, row in enumerate(us.SLOPE_ROWS):
        us.assert_scaled(o0[r], o1[r], *law[row], pv, pr, what=f"outer[{row}]")
        us.assert_scaled(i0[r], i1[r], *law[row], pv, pr, what=f"inner[{row}]")
    for a, b, row in ((d0, d1, "D"), (dw0, dw1, "D_w"), (dk0, dk1, "D_k")):
        us.assert_scaled(a, b, *law[row], pv, pr, what=row)
    us.assert_scaled(ref["cg"], got["cg"], *law["cg"], pv, pr, what="group_velocity")
    n0, n1 = ref["newton"], got["newton"]
    assert np.count_nonzero(n0["flag"] == 1) > 0
    for col in ("iters", "flag", "status"):
        us.assert_same(n0[col], n1[col], "newton." + col)
    us.assert_scaled(n0["w"], n1["w"], *law["w"], pv, pr, what="newton.w")
    us.assert_scaled(n0["dwdk"], n1["dwdk"], *law["dwdk"], pv, pr, what="newton.dwdk")
    us.assert_scaled(n0["resid"], n1["resid"], *law["resid"], pv, pr, what="newton.resid")


def _modes(ctx, name, pv, pr):
    def run():
        from eigensolver_amd import _lib
        gp = _problem(ctx, name, pv, pr)
        k, w = _roots_of(ctx, name, pv)
        out = {"eig": _np(gp.eigenfunction(k[:4], w[:4], n_ext=64)),
               "sig": _np(gp.mode_signature(k, w)),
               "label": _np(gp.label_roots({"k": gp._dev(k), "w": gp._dev(w)}))}
        if us.family(gp.desc.geometry) == "cyl" and gp.desc.x_boundary > 0:
            out["pol"] = _np(gp.polarisation(k[:4], w[:4], n_ext=64))
            out["amp_names"] = _lib.AMP_NAMES
        gp.close()
        return out

    return _cached(("modes", name, pv, pr), run)


@_pairs(["CF_flow_kink", "CR_kink", "SD_w15_kink", "CDP_kink"])
def test_eigenfunctions_and_labels(es_ctx, name, pv, pr):
    """eigenfunction, mode_signature / label_roots at the roots of (a): arrays by LAW, node counts equal; on the cylinders
    with positive radii (CR_kink, and CDP_kink for an untwisted one) also polarisation, each of the seven amplitudes with
    its own law.  Two restrictions, both formulas of the reference's export scripts (unit_scaling.py has them):
      * the exterior xi_z, v_z carry the omega^2 of Export_vtk.py:781 (LAW's *_ext_reference);
      * the interior xi_z, v_z of the rotating tube CR_kink are left out: Export_vtk.py:780 subtracts
        (2 Omega v_phi B_phi + f_B v_phi^2) xi_r / r from terms of another dimension, so they follow no law where v_phi != 0."""
    ref, got = _modes(es_ctx, name, 0, 0), _modes(es_ctx, name, pv, pr)
    law = us.LAW[_fp64(es_ctx, name, 0, 0)["fam"]]
    for col, row in (("x_int", "x"), ("x_ext", "x"), ("value_int", "value"), ("value_ext", "value"), ("flux_int", "flux"),
                     ("flux_ext", "flux")):
        us.assert_scaled(ref["eig"][col], got["eig"][col], *law[row], pv, pr, what="eigenfunction." + col)
    for what in ("sig", "label"):
        s0, s1 = ref[what], got[what]
        assert np.all(s0.status == 0)
        for col in ("nodes_value", "nodes_flux", "peak_node_value", "peak_node_flux", "status"):
            us.assert_same(getattr(s0, col), getattr(s1, col), f"{what}.{col}")
        us.assert_scaled(s0.peak_value, s1.peak_value, *law["peak_value"], pv, pr, what=what + ".peak_value")
        us.assert_scaled(s0.peak_flux, s1.peak_flux, *law["peak_flux"], pv, pr, what=what + ".peak_flux")
    assert ("pol" in ref) == (name in ("CR_kink", "CDP_kink"))
    if "pol" in ref:
        N = ref["eig"]["value_int"].shape[1]                 # columns [:N] interior (axis to boundary), [N:] exterior
        us.assert_scaled(ref["pol"]["radius"], got["pol"]["radius"], *law["x"], pv, pr, what="polarisation.radius")
        for c, amp in enumerate(ref["amp_names"]):
            a0, a1 = ref["pol"]["amp"][:, c], got["pol"]["amp"][:, c]
            assert np.isfinite(a0).all()
            if amp in ("xi_z", "v_z"):
                us.assert_scaled(a0[:, N:], a1[:, N:], *law[amp + "_ext_reference"], pv, pr, what=f"polarisation.{amp} (exterior)")
                if name != "CR_kink":
                    us.assert_scaled(a0[:, :N], a1[:, :N], *law[amp], pv, pr, what=f"polarisation.{amp} (interior)")
            else:
                us.assert_scaled(a0, a1, *law[amp], pv, pr, what="polarisation." + amp)


# ---- (e) closed-form uniform cylinder -------------------------------------------------------------------------------------
def _uniform(ctx, pv, pr):
    def run():
        case = CASES["CF_uniform_kink"]
        eq, mode, _, _ = case
        k, W = us.grid_of(case)
        Ws = np.ldexp(W, pv)
        out = {}
        for m in range(4):
            out["eval", m] = _np(us.scaled_uniform(eq, mode, m, ctx, pv, pr).eval_grid(k, Ws, want_rel=True))
        t, cnt, D, st = us.scaled_uniform(eq, mode, 0, ctx, pv, pr).find_roots(k, Ws, orders=range(4), n_bisect=N_BISECT,
                                                                                want_grid=True)
        out["roots"] = (_np(t), cnt)
        out["grid"] = _np((D, st))
        return out

    return _cached(("uniform", pv, pr), run)


@pytest.mark.parametrize("pv,pr", SCALES, ids=[f"V{pv}-R{pr}" for pv, pr in SCALES])
def test_closed_form_uniform_cylinder(es_ctx, pv, pr):
    """es_cyl_uniform_eval and es_cyl_uniform_find_roots, orders 0 - 3, the parameters of CF_uniform_kink."""
    ref, got = _uniform(es_ctx, 0, 0), _uniform(es_ctx, pv, pr)
    law = us.LAW["cyl"]
    for m in range(4):
        _check_grid(ref["eval", m], got["eval", m], "cyl", pv, pr, f"uniform_eval[m={m}]")
    (D0, st0), (D1, st1) = ref["grid"], got["grid"]
    us.assert_same(st0, st1, "uniform_find_roots.status")
    us.assert_scaled(D0, D1, *law["D"], pv, pr, ok=st0 == 0, what="uniform_find_roots.D")
    assert np.count_nonzero(ref["roots"][0]["flag"] == 1) > 0
    us.assert_root_table_scaled(ref["roots"], got["roots"], pv, pr, "cyl", "uniform_roots")
    us.assert_same(ref["roots"][0]["order"], got["roots"][0]["order"], "uniform_roots.order")


# ---- (f) complex frequencies ----------------------------------------------------------------------------------------------
README_GRID = (np.linspace(1.2, 1.9, 8), np.linspace(0.45, 1.15, 8))     # the 8 x 8 complex omega grid of the README
JET_GRID = (np.linspace(1.8, 3.0, 8), np.linspace(0.02, 0.5, 8))         # 8 x 8 around the unstable kink root of the jet at k = 2


def _complex_setups():
    from eigensolver_amd import equilibrium as q
    from eigensolver_amd.complex_flow import SlabComplexFlow, SlabFlowKH
    from eigensolver_amd.cyl_complex import CylinderComplex
    from eigensolver_amd.cylt_complex import RotatingCylinderComplex
    return {
        "jet": (CylinderComplex, q.CylinderFlow(c_e=1.5, vA_e=0.5, U_i0=3.0, width=1.5), None, [2.0], (README_GRID, JET_GRID), "cyl"),
        "tube": (RotatingCylinderComplex, q.CylinderRotation(v_twist=2.0, power=1.0, r_axis=1e-2), 3, [1.0], (README_GRID,), "cyl"),
        "slab": (SlabComplexFlow, SlabFlowKH(width=0.9), None, [1.0], ((np.linspace(0.1, 1.2, 8), np.linspace(-0.2, 0.3, 8)),), "slab"),
    }


def _complex(ctx, which, pv, pr):
    def run():
        cls, eq, m, k, grids, fam = _complex_setups()[which]
        sel = {} if which == "slab" else {"m": m}
        solver = us.complex_solver(cls, eq, ctx, "kink", m, pv, pr)
        out = {"fam": fam, "grids": []}
        for w_re, w_im in grids:
            w_re, w_im = np.ldexp(w_re, pv), np.ldexp(w_im, pv)
            D, st, rel = solver.eval_grid("kink", k, w_re, w_im, **sel)
            g = {"D": _np(D), "st": _np(st), "rel": _np(rel)}
            t, cnt = solver.find_roots("kink", k, w_re, w_im, D, st, **sel)
            g["roots"], g["count"] = _np(t), cnt
            g["unstable"] = solver.unstable_roots("kink", k, w_re, w_im, **sel) if which != "slab" else []
            if which != "slab":
                W = (w_re[None, :] + 1j * w_im[:, None]).ravel()
                _, st_p, _, outer, inner = solver.eval_points("kink", k[0], W, parts=True, **sel)
                g["parts"] = _np((st_p, outer, inner))
            acc = np.flatnonzero(g["roots"]["flag"] == 1)
            if which == "slab":                                 # the slopes of the slab at every grid point
                sl = solver.root_slopes("kink", k[0], (w_re[None, :] + 1j * w_im[:, None]).ravel())
                g["slopes"] = _np((sl.outer, sl.inner, sl.status))
            elif acc.size:
                sl = solver.root_slopes("kink", g["roots"]["k"][acc], g["roots"]["w"][acc], **sel)
                g["slopes"] = _np((sl.outer, sl.inner, sl.status))
            out["grids"].append(g)
        solver.close()
        return out

    return _cached(("complex", which, pv, pr), run)


COMPLEX_PAIRS = [(w, pv, pr) for w in ("jet", "tube") for pv, pr in SCALES] + [("slab", pv, pr) for pv, pr in DENSITY_ONLY]


@pytest.mark.parametrize("which,pv,pr", COMPLEX_PAIRS, ids=[f"{w}-V{pv}-R{pr}" for w, pv, pr in COMPLEX_PAIRS])
def test_complex_frequencies(es_ctx, which, pv, pr):
    """Untwisted jet (kink, k = 2), rotating tube (m = 3, k = 1) and the flow slab SlabComplexFlow(width=0.9) on 8 x 8 complex
    omega grids: D_c, outer, inner and rel by LAW; the same roots with Re omega and Im omega times V exactly, flags equal;
    root_slopes at the roots by LAW (the slab, whose 8 x 8 grid need hold no accepted root: at every grid point, and its
    find_roots table compared as it is; it has no unstable_roots).  The slab is sheared (width = 0.9) and goes under the density scale only: its D(x) is
    the non-homogeneous formula of the module docstring.  The jet runs on the README's grid as the tube does and on a
    second 8 x 8 grid that holds its unstable root."""
    ref, got = _complex(es_ctx, which, 0, 0), _complex(es_ctx, which, pv, pr)
    law = us.LAW[ref["fam"]]
    if which != "slab":
        assert any(np.count_nonzero(g["roots"]["flag"] == 1) > 0 for g in ref["grids"]), "no accepted root on any grid"
    for n, (g0, g1) in enumerate(zip(ref["grids"], got["grids"])):
        us.assert_same(g0["st"], g1["st"], f"grid{n}.status")
        ok = g0["st"] == 0
        us.assert_scaled(g0["D"], g1["D"], *law["D"], pv, pr, ok=ok, what=f"grid{n}.D_c")
        us.assert_scaled(g0["rel"], g1["rel"], *law["rel"], pv, pr, ok=ok, what=f"grid{n}.rel")
        if "parts" in g0:
            (s0, o0, i0), (s1, o1, i1) = g0["parts"], g1["parts"]
            us.assert_same(s0, s1, f"grid{n}.points.status")
            us.assert_scaled(o0, o1, *law["outer"], pv, pr, ok=s0 == 0, what=f"grid{n}.outer")
            us.assert_scaled(i0, i1, *law["inner"], pv, pr, ok=s0 == 0, what=f"grid{n}.inner")
        assert g0["count"] == g1["count"]
        r0, r1 = g0["roots"], g1["roots"]
        for col in ("row", "flag"):
            us.assert_same(r0[col], r1[col], f"grid{n}.roots.{col}")
        us.assert_scaled(r0["w"], r1["w"], *law["w"], pv, pr, what=f"grid{n}.roots.w")
        us.assert_scaled(r0["k"], r1["k"], *law["k"], pv, pr, what=f"grid{n}.roots.k")
        us.assert_scaled(r0["resid"], r1["resid"], *law["resid"], pv, pr, what=f"grid{n}.roots.resid")
        assert [len(r) for r in g0["unstable"]] == [len(r) for r in g1["unstable"]], "unstable_roots: another number of roots"
        for row, (u0, u1) in enumerate(zip(g0["unstable"], g1["unstable"])):
            us.assert_scaled(u0, u1, *law["w"], pv, pr, what=f"grid{n}.unstable_roots[{row}]")
        assert ("slopes" in g0) == ("slopes" in g1)
        if "slopes" in g0:
            (o0, i0, s0), (o1, i1, s1) = g0["slopes"], g1["slopes"]
            us.assert_same(s0, s1, f"grid{n}.slopes.status")
            for r, row in enumerate(us.SLOPE_ROWS):
                us.assert_scaled(o0[r], o1[r], *law[row], pv, pr, what=f"grid{n}.outer[{row}]")
                us.assert_scaled(i0[r], i1[r], *law[row], pv, pr, what=f"grid{n}.inner[{row}]")

"""Helper (not a test): yardsticks for es_cylt_complex_root_slopes and es_cylt_complex_newton (include/eigensolver_amd.h
section 18).

  jets          NumPy forward-mode restatement of tests/cylt_complex_model.CyltComplexModel.eval over the jet class J of
                tests/complex_slope_model.py (value, d/d omega, d/dk; complex arrays): the model's formulas (coef, row with the
                full-shape step, _axis, _finish), in its order, with omega = (w, 1, 0) and k = (k, 0, 1), one k per point.
                The exterior is the jet exterior of tests/cyl_complex_slope_model.py as it is: the medium outside is the
                same.  Returns outer[3, p], inner[3, p] and the status; row 0 is CyltComplexModel.eval.
  cauchy_parts  d/d omega and d/dk of [outer, inner] of the model itself by Cauchy's formula: that of
                tests/cyl_complex_slope_model.py, which goes through exterior, row and _finish and so bypasses eval's float k.
  newton_model  the iteration rule of es_cylt_complex_newton, step for step, on `jets` (the rule of
                cyl_complex_slope_model.newton_model, whose evaluator is fixed: restated here over this evaluator).
  model_root / curve_slope   those of tests/cyl_complex_slope_model.py: roots of the model's own secant iteration, and the
                slope d omega / dk of the root curve from roots re-solved at k +- 1e-3 and k +- 5e-4, Richardson-combined.
"""
import functools

import numpy as np

from tests.complex_slope_model import J, dwdk
from tests.cyl_complex_slope_model import _exterior, cauchy_parts, curve_slope, model_root, rel_of  # noqa: F401
from tests.cylt_complex_model import AXIS_KINK, AXIS_ROTATION_KINK, AXIS_SAUSAGE, ST_OK, model_for, root_cases

ST_NONFINITE = 2
N0 = 130
NEWTON_OFFSET = 1e-3 * (1 + 1j)
NAMES = ("A", "B", "C", "sausage", "reference")

# worst |jets - Cauchy| / max(|outer_x|, |inner_x|) over outer_w, inner_w, outer_k, inner_k of the pairs of cauchy_pairs(),
# r = 1e-2, M = 32, and the worst relative disagreement of the radii r and r / 2 there (tests/test_cylt_complex_slope_model.py
# prints the figures of a run; the test's bound is 10 x this)
CAUCHY_MEASURED = 1.5e-14
CAUCHY_RADII_MEASURED = 4.1e-14
# |d omega / dk (jets) - curve slope| / max(1, |slope|) at root A and the three rows of C, measured the same way; bound 10 x.
# The figure is the difference quotient's own error: it grows with the curvature of the root curve, and row 2 of C (k = 1,
# d omega / dk = -0.0007 - 5.2241i) lies next to the branch point near k = 1.06 where the root returns to the real axis.
SLOPE_MEASURED = {("A", 0): 1.3e-11, ("C", 0): 3.8e-13, ("C", 1): 3.2e-12, ("C", 2): 2.2e-8}
# the rotating tube whose nine real roots (the C port's search, tests/mode_signature_model.py; N = 2000) the complex path is
# checked on, and the worst |d omega / dk (this model, Im omega = 0) - c_g (tests/root_slope_model.py)| / max(1, |c_g|) over
# those roots; bound 10 x.  Im d omega / dk is exactly 0 in the model.
REAL_AXIS_CASE = "CR_kink"
REAL_AXIS_MEASURED = 9.6e-15
# steps the Newton rule takes on the model from root + / - 1e-3 (1 + i) at A, B and the three rows of C, max_iter = 8: step
# lengths 1.4e-3, 2e-6 .. 7e-6, 5e-12 .. 2e-10, < 2e-15
NEWTON_STEPS = 4

# the densify case: problem A on k in [0.85, 1.1], five coarse rows in A's own window (one distinct root each in the model's
# cell rule), 21 fine wavenumbers.  At k = 0.8 a cell corner of the window is leaky and the row is empty.
DENSIFY_K = (0.85, 1.1)
DENSIFY_W_RE, DENSIFY_W_IM = np.linspace(1.2, 1.9, 8), np.linspace(0.45, 1.15, 8)
DENSIFY_ENDS = (1.5619837 + 1.0130337j, 1.5523954 + 0.5650253j)       # the roots of the first and the last coarse row
# worst |Hermite prediction - model secant root| over the 21 fine k with the model's exact slopes at the five coarse roots
# (bound 10 x); the smallest shift bound of shooting.hermite_guess (shift_factor 4) is 2.7e-2, 250 times that
DENSIFY_PREDICTION_MEASURED = 1.2e-4


# ---- jets --------------------------------------------------------------------------------------------------------------------
def _coef(M, j, k, w):
    """CyltComplexModel.coef over jets"""
    f = lambda a: float(a[j])                                                                     # noqa: E731
    kb = k * f(M.BZ) + f(M.MB)
    wA = k * f(M.BA) + f(M.MB)
    e1 = wA * wA
    e2 = e1 * f(M.Q)
    e7 = f(M.C7) * kb * f(M.INVR)
    e8 = kb * f(M.BPHI)
    e11 = f(M.S) * (f(M.M2R2) + k * k)
    Om = w - (k * f(M.VZ) + f(M.MV))
    Om2 = Om * Om
    t1, t2 = Om2 - e1, Om2 - e2
    D = f(M.E3) * t1 * t2
    Q = Om * e7 + (Om2 * f(M.E6) + -(t1 * f(M.E5)))
    T = f(M.E9) * Om + e8
    OmP = Om2 if M.d["c1_power"] == 2 else Om
    t2T = t2 * T
    C1 = Q * OmP + -(f(M.E10) * t2T)
    C2 = Om2 * Om2 + -(e11 * t2)
    C3 = D * (f(M.RHO) * t1 + f(M.RDC3)) + (Q * Q + -((f(M.E13) * t2T) * T))
    inv = 1.0 / D
    return C1 * inv, (C3 * f(M.INVR)) * inv, (-(f(M.R) * C2)) * inv


def _row(M, k, w):
    """CyltComplexModel.row over jets"""
    N, h = M.N, M.h
    h2, h6, h3 = 0.5 * h, h / 6.0, h / 3.0
    zero, one = np.zeros_like(w.v), np.ones_like(w.v)
    d0, b0, a0 = _coef(M, 2 * (N - 1), k, w)
    if M.d["axis_bc"] == AXIS_SAUSAGE:
        p, q = -d0, b0
    else:
        p, q = J(one, zero, zero), J(zero, zero, zero)

    def rhs(d, b, a, pp, qq):
        return -d * pp + a * qq, d * qq + b * pp

    for j in range(N - 2, -1, -1):
        dm, bm, am = _coef(M, 2 * j + 1, k, w)
        d1, b1, a1 = _coef(M, 2 * j, k, w)
        k1p, k1q = rhs(d0, b0, a0, p, q)
        k2p, k2q = rhs(dm, bm, am, h2 * k1p + p, h2 * k1q + q)
        k3p, k3q = rhs(dm, bm, am, h2 * k2p + p, h2 * k2q + q)
        k4p, k4q = rhs(d1, b1, a1, h * k3p + p, h * k3q + q)
        p = h6 * (k1p + k4p) + (h3 * (k2p + k3p) + p)
        q = h6 * (k1q + k4q) + (h3 * (k2q + k3q) + q)
        d0, b0, a0 = d1, b1, a1
    return p, q


def _axis(M, xi_e, p, q):
    """CyltComplexModel._axis over jets"""
    bc = M.d["axis_bc"]
    if bc == AXIS_KINK:
        return (M.d["bc_const"] * xi_e - p * 1.0) / q
    if bc == AXIS_ROTATION_KINK:
        return (-(M.d["bc_const"] * xi_e) - p * 1.0) / q
    return -(p * 1.0) / q


def jets(M, k, w):
    """(outer[3, p], inner[3, p], status[p]) at the pairs k[p] (real, broadcast), w[p] (complex): CyltComplexModel.eval over
    jets.  Rows of a pair that is not ST_OK, or that holds a non-finite entry (the status is then ST_NONFINITE), are NaN."""
    w = np.atleast_1d(np.asarray(w, dtype=complex)).reshape(-1)
    kv = np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy()
    one, zero = np.ones_like(w), np.zeros_like(w)
    kj, wj = J(kv + 0j, zero, one), J(w, one, zero)
    with np.errstate(all="ignore"):
        st, xi_e = _exterior(M, kj, wj)
        p, q = _row(M, kj, wj)
        xi_i = _axis(M, xi_e, p, q) / M.d["x_boundary"]                                            # CyltComplexModel._finish
        outer, inner = xi_e.rows(w.shape).copy(), xi_i.rows(w.shape).copy()
    fin = np.isfinite(outer[0] - inner[0]) & np.isfinite(outer).all(axis=0) & np.isfinite(inner).all(axis=0)
    st = np.where((st == ST_OK) & ~fin, ST_NONFINITE, st).astype(np.uint8)
    bad = st != ST_OK
    outer[:, bad] = np.nan + 1j * np.nan
    inner[:, bad] = np.nan + 1j * np.nan
    return outer, inner, st


# ---- Newton's iteration, the rule of es_cylt_complex_newton ------------------------------------------------------------------
def newton_model(M, k, guess, max_iter=8, step_cap=np.inf, max_shift=np.inf, tol_percent=4.0):
    """dict(w, resid, iters, flag, dwdk, status, steps) for one guess; steps: the |s| of every step taken"""
    w, iters, ok, steps = complex(guess), 0, True, []
    for _ in range(max_iter):
        outer, inner, st = jets(M, k, w)
        D, Dw = outer[0, 0] - inner[0, 0], outer[1, 0] - inner[1, 0]
        if st[0] != ST_OK or not np.isfinite(D) or not np.isfinite(Dw) or Dw == 0:
            ok = False
            break
        s = -D / Dw
        if abs(s) > step_cap:
            s *= step_cap / abs(s)
        w += s
        iters += 1
        steps.append(abs(s))
        if abs(s) <= 1e-14 * max(1.0, abs(w)):
            break
    outer, inner, st = jets(M, k, w)
    with np.errstate(all="ignore"):
        resid = rel_of(M, outer, inner)[0]
        slope = dwdk(outer, inner)[0]
    flag = bool(ok and st[0] == ST_OK and resid < tol_percent and abs(w - guess) <= max_shift)
    return dict(w=w, resid=resid, iters=iters, flag=int(flag), dwdk=slope, status=int(st[0]), steps=steps)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def problems(n_nodes=N0):
    """name -> (equilibrium, mode, m, accept_norm): the five problems of tests/test_cylt_complex_gpu.py -- both values of
    c1_power, the rotational sausage condition and ES_AXIS_ROTATION_KINK ("reference") among them"""
    from eigensolver_amd import equilibrium as q
    rot = lambda v, p, **kw: q.CylinderRotation(v_twist=v, power=p, n_nodes=n_nodes, **kw)             # noqa: E731
    return {
        "A": (rot(2.0, 1.0, r_axis=1e-2), "kink", 3, 0),
        "B": (rot(2.0, 0.8, r_axis=1e-2, c1_power=1), "kink", 1, 1),
        "C": (rot(1.0, 1.0, r_axis=1e-2), "kink", 4, 0),
        "sausage": (rot(0.15, 1.25, r_axis=1e-2, c1_power=1), "sausage", 0, 0),
        "reference": (rot(0.25, 0.8), "kink", None, 1),
    }


# phase-speed window of Re omega / k and the window of |Im omega| / k of the samples (those of tests/test_cylt_complex_gpu.py)
WINDOW = {"A": ((1.2, 1.9), (0.45, 1.15)), "B": ((1.2, 1.7), (0.05, 0.35)), "C": ((0.9, 1.4), (0.15, 1.2)),
          "sausage": ((0.6, 1.45), (0.02, 0.3)), "reference": ((0.6, 1.45), (0.02, 0.3))}
# two non-root pairs (k, omega) of each problem, one of either sign of Im omega, inside its window
NON_ROOT = {
    "A": ((1.0, 1.35 + 0.6j), (0.8, 1.3 - 0.7j)),
    "B": ((1.0, 1.3 + 0.25j), (1.5, 2.2 - 0.3j)),
    "C": ((0.75, 0.8 + 0.4j), (1.0, 1.2 - 0.5j)),
    "sausage": ((1.0, 0.9 + 0.2j), (2.0, 2.4 - 0.3j)),
    "reference": ((1.0, 1.1 + 0.15j), (2.0, 1.6 - 0.4j)),
}
# a pair with Re m_e < 0 for every problem: Re omega / k beyond every exterior speed (that of tests/test_cylt_complex_gpu.py)
LEAKY = (1.0, 2.4 + 0.05j)


@functools.lru_cache(maxsize=None)
def model(name, n_nodes=N0):
    eq, mode, m, an = problems(n_nodes)[name]
    return model_for(eq, mode, m, accept_norm=an)


@functools.lru_cache(maxsize=None)
def case_roots(name, n_nodes=N0):
    """((k, root), ...) of a root case of tests/cylt_complex_model.root_cases (A, B: one row; C: three): the model's cell rule
    and secant iteration in the case's window, one distinct root per row"""
    eq, m, k, w_re, w_im, quoted = root_cases(n_nodes)[name]
    M = model_for(eq, "kink", m)
    cells, roots = M.find_roots(np.asarray(k), w_re, w_im)
    out = []
    for r, kk in enumerate(k):
        ws = [w for cell, w in zip(cells, roots) if cell[0] == r and w is not None]
        assert ws and all(abs(w - ws[0]) <= 1e-8 for w in ws), (name, r, ws)
        out.append((float(kk), complex(ws[0])))
    if quoted is not None:
        assert abs(out[0][1] - quoted) < 1e-5
    return tuple(out)


@functools.lru_cache(maxsize=None)
def root_model(name, n_nodes=N0):
    """the model the roots of case_roots belong to (accept_norm 0, as root_cases poses them)"""
    eq, m, _, _, _, _ = root_cases(n_nodes)[name]
    return model_for(eq, "kink", m)


def cauchy_pairs():
    """[(model, label, k, w)]: the roots of cases A and B and the three rows of C, and the two non-root pairs of each of the
    five problems"""
    out = []
    for name in ("A", "B", "C"):
        out += [(root_model(name), f"root {name}", k, w) for k, w in case_roots(name)]
    for name in NAMES:
        out += [(model(name), name, k, w) for k, w in NON_ROOT[name]]
    return out


@functools.lru_cache(maxsize=None)
def slope_cases():
    """{(name, row): (model, k, root, curve slope)} at root A and the three rows of C, computed once per session"""
    out = {}
    for name, row in SLOPE_MEASURED:
        M = root_model(name)
        k, root = case_roots(name)[row]
        outer, inner, _ = jets(M, k, root)
        out[(name, row)] = (M, k, root, curve_slope(M, k, root, dwdk(outer, inner)[0]))
    return out


@functools.lru_cache(maxsize=None)
def real_axis_case():
    """(eq, mode, m, k, w, c_g of the real model, d omega / dk of this model) at the real roots of REAL_AXIS_CASE"""
    from tests import mode_signature_model as S
    from tests import real_eigen_model as RM
    from tests import root_slope_model as R
    eq, mode, m, _ = RM.all_cases()[REAL_AXIS_CASE]
    k, w, _ = S.port_roots(REAL_AXIS_CASE)
    cg = R.group_velocity(*R.jets(REAL_AXIS_CASE, k, w))
    outer, inner, st = jets(model_for(eq, mode, m), k, w + 0j)
    assert np.all(st == ST_OK), st
    return eq, mode, m, k, w, cg, dwdk(outer, inner)


def follow(M, k_from, w_from, ks):
    """the model's branch through (k_from, w_from) at the wavenumbers ks (monotone, starting next to k_from): secant roots,
    each start predicted with the model's slope at the previous root"""
    out, k, w = [], k_from, w_from
    for kk in ks:
        outer, inner, _ = jets(M, k, w)
        w = model_root(M, kk, w + dwdk(outer, inner)[0] * (kk - k))
        k = kk
        out.append(w)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def densify_case(n_fine=21):
    """(model, coarse k[5], coarse roots[5] by the model's cell rule, fine k, the model's secant roots at the fine k)"""
    M = root_model("A")
    kf = np.linspace(DENSIFY_K[0], DENSIFY_K[1], n_fine)
    step = (n_fine - 1) // 4
    kc = kf[::step]
    cells, roots = M.find_roots(kc, DENSIFY_W_RE, DENSIFY_W_IM)
    wc = []
    for r in range(len(kc)):
        ws = [w for cell, w in zip(cells, roots) if cell[0] == r and w is not None]
        assert ws and all(abs(w - ws[0]) <= 1e-8 for w in ws), (r, ws)
        wc.append(complex(ws[0]))
    wc = np.array(wc)
    branch = np.concatenate([[wc[0]], follow(M, kc[0], wc[0], kf[1:])])
    for a in (kf, kc, wc, branch):
        a.setflags(write=False)
    return M, kc, wc, kf, branch

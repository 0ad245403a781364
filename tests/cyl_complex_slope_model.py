"""Helper (not a test): yardsticks for es_cyl_complex_root_slopes and es_cyl_complex_newton (include/eigensolver_amd.h
section 15).

  jets          NumPy forward-mode restatement of tests/cyl_complex_model.CylComplexModel.eval over the jet class J of
                tests/complex_slope_model.py (value, d/d omega, d/dk; complex arrays): the model's formulas, in its order, with
                omega = (w, 1, 0) and k = (k, 0, 1).  The exterior is rewritten in jets: scipy's kve and ive at the value, the
                argument derivative by the identities d/dz[e^z K_n] = e^z K_n - e^z K_{n+1} + (n/z) e^z K_n and its three
                companions.  Returns outer[3, p], inner[3, p] and the status; row 0 is CylComplexModel.eval.
  cauchy_parts  d/d omega and d/dk of [outer, inner] of the model itself by the trapezoid rule on Cauchy's formula
                (complex_slope_model.cauchy): a different route from the jets, no step to trust.  The model is holomorphic in
                a complex k once the float(k) of its eval is bypassed.  Two radii; the disagreement is reported.
  newton_model  the iteration rule of es_cyl_complex_newton, step for step, on `jets` (the rule of
                complex_slope_model.newton_model, whose resid has no accept_norm and whose evaluator is fixed: restated here
                over this evaluator).
  model_root / curve_slope   roots of the model's own secant iteration, and the slope d omega / dk of the root curve from
                roots re-solved at k +- 1e-3 and k +- 5e-4, Richardson-combined.
"""
import functools

import numpy as np
from scipy import special

from tests.complex_slope_model import J, cauchy, dwdk, jexp, jsqrt
from tests.cyl_complex_model import AXIS_KINK, AXIS_SAUSAGE, ST_LEAKY, ST_NONFINITE, ST_OK, model_for

K0 = 2.0
N0 = 130
KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0)           # the jet that is Kelvin-Helmholtz unstable
# the kink roots at k = 2, N = 130 by width, as the table states them
KH_ROOTS = {1e5: 2.372765 + 0.584713j, 3.0: 2.252841 + 0.190187j, 1.5: 2.673523 + 0.084843j}
NEWTON_OFFSET = 1e-3 * (1 + 1j)

# worst |jets - Cauchy| / max(|outer_x|, |inner_x|) over outer_w, inner_w, outer_k, inner_k of the pairs of cauchy_pairs(),
# r = 1e-2, M = 32, and the worst relative disagreement of the radii r and r / 2 there (tests/test_cyl_complex_slope_model.py
# prints the figures of a run; the test's bound is 10 x this).  At r = 1e-3 the two figures are 4.5e-13 and 8.2e-13: rounding
# of the sum divided by the radius, not the model.
CAUCHY_MEASURED = 4.8e-14
CAUCHY_RADII_MEASURED = 9.9e-14
# |d omega / dk (jets) - curve slope| / max(1, |slope|) per width, measured the same way; bound 10 x
SLOPE_MEASURED = {1e5: 1.1e-12, 3.0: 3.7e-12, 1.5: 1.6e-12}
# the untwisted cylinder whose real roots (the C port's search, tests/mode_signature_model.py) the complex path is checked on,
# and the worst |d omega / dk (this model, Im omega = 0) - c_g (tests/root_slope_model.py)| / max(1, |c_g|) over those roots,
# imaginary part included; bound 10 x
REAL_AXIS_CASE = "CF_flow_kink_N130"
REAL_AXIS_MEASURED = 2.7e-15


# ---- jets --------------------------------------------------------------------------------------------------------------------
def _where(cond, a, b):
    a, b = J.lift(a), J.lift(b)
    return J(np.where(cond, a.v, b.v), np.where(cond, a.dw, b.dw), np.where(cond, a.dk, b.dk))


def _lift(f, df, x):
    """f(x) for a function known by its value f and derivative df at the value of x"""
    return J(f, df * x.dw, df * x.dk)


def _coef(M, j, k, w):
    """CylComplexModel.coef over jets"""
    m2, k2 = float(M.d["m"]) ** 2, k * k
    wA = k * float(M.bA[j])
    e1 = wA * wA
    e2 = e1 * float(M.q[j])
    Bq = float(M.B1[j])
    g = m2 * float(M.E1[j]) + k2 * float(M.E2[j])
    e5 = g - Bq * (e1 + e2)
    e6 = -(Bq * (e2 * e2))
    Om = w - k * float(M.vz[j])
    t1 = Om * Om - e1
    t2 = Om * Om - e2
    a12 = float(M.A1[j]) * t1
    a21 = (e5 * t2 + e6) * (1.0 / (t1 * t2)) + (-Bq)
    return a12, a21


def _row(M, k, w):
    """CylComplexModel.row over jets"""
    N, h = M.N, M.h
    h2, h6, h3 = 0.5 * h, h / 6.0, h / 3.0
    zero, one = np.zeros_like(w.v), np.ones_like(w.v)
    b0, a0 = _coef(M, 2 * (N - 1), k, w)
    if M.d["axis_bc"] == AXIS_SAUSAGE:
        p, q = J(zero, zero, zero), b0
    else:
        p, q = J(one, zero, zero), J(zero, zero, zero)
    for j in range(N - 2, -1, -1):
        bm, am = _coef(M, 2 * j + 1, k, w)
        b1, a1 = _coef(M, 2 * j, k, w)
        k1p, k1q = a0 * q, b0 * p
        tp, tq = h2 * k1p + p, h2 * k1q + q
        k2p, k2q = am * tq, bm * tp
        tp, tq = h2 * k2p + p, h2 * k2q + q
        k3p, k3q = am * tq, bm * tp
        tp, tq = h * k3p + p, h * k3q + q
        k4p, k4q = a1 * tq, b1 * tp
        p = h6 * (k1p + k4p) + (h3 * (k2p + k3p) + p)
        q = h6 * (k1q + k4q) + (h3 * (k2q + k3q) + q)
        b0, a0 = b1, a1
    return p, q


def _exterior(M, k, w):
    """CylComplexModel.exterior over jets -> (status, xi_e)"""
    d = M.d
    k2, w2 = k * k, w * w
    vAe2, ce2, cTe2 = d["vA_e"] ** 2, d["c_e"] ** 2, d["cT_e"] ** 2
    m_e = ((k2 * vAe2 - w2) * (k2 * ce2 - w2)) / ((vAe2 + ce2) * (k2 * cTe2 - w2))
    cst = -1.0 / (d["rho_e"] * (k2 * vAe2 - w2))
    st = np.where(m_e.v.real < 0, ST_LEAKY, np.where(np.isfinite(m_e.v) & np.isfinite(cst.v), ST_OK, ST_NONFINITE))
    mu = jsqrt(_where(st == ST_OK, m_e, 1.0 + 0j))            # principal root
    sgn = -1.0 if d["x_boundary"] < 0 else 1.0
    n = float(d["m_ext"])
    xR, xb = mu * (d["L_factor"] * 2.0 * np.pi / k), mu

    def K(z):
        a, b = special.kve(n, z.v), special.kve(n + 1, z.v)
        Kn = _lift(a, a - b + (n / z.v) * a, z)
        Kn1 = _lift(b, b - a - ((n + 1.0) / z.v) * b, z)
        return Kn, (n / z) * Kn - Kn1                         # e^z K_n, e^z K_n'

    def I(z):
        ph = np.exp(-1j * z.v.imag)
        a, b = special.ive(n, z.v) * ph, special.ive(n + 1, z.v) * ph
        In = _lift(a, b - a + (n / z.v) * a, z)
        In1 = _lift(b, a - b - ((n + 1.0) / z.v) * b, z)
        return In, In1 + (n / z) * In                         # e^-z I_n, e^-z I_n'

    Kb, dKb = K(xb)
    KR, dKR = K(xR)
    Ib, dIb = I(xb)
    IR, dIR = I(xR)
    g = d["ic_slope"] / (sgn * mu)
    a_s, b_s = -(d["ic_value"] * dKR - g * KR), -(g * IR - d["ic_value"] * dIR)
    gap = xR - xb
    E2 = jexp(-2.0 * gap)
    near = gap.v.real < 40.0
    Pv = _where(near, b_s * Kb + E2 * a_s * Ib, Kb)
    dPv = (sgn * mu) * _where(near, b_s * dKb + E2 * a_s * dIb, dKb)
    outer = cst * (dPv / Pv)
    st = np.where((st == ST_OK) & ~np.isfinite(outer.v), ST_NONFINITE, st)
    return st, outer


def jets(M, k, w):
    """(outer[3, p], inner[3, p], status[p]) at the pairs k[p] (real, broadcast), w[p] (complex): CylComplexModel.eval over
    jets.  Rows of a pair that is not ST_OK, or that holds a non-finite entry (the status is then ST_NONFINITE), are NaN."""
    w = np.atleast_1d(np.asarray(w, dtype=complex)).reshape(-1)
    kv = np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy()
    one, zero = np.ones_like(w), np.zeros_like(w)
    kj, wj = J(kv + 0j, zero, one), J(w, one, zero)
    d = M.d
    with np.errstate(all="ignore"):
        st, xi_e = _exterior(M, kj, wj)
        p, q = _row(M, kj, wj)
        # CylComplexModel._finish
        if d["axis_bc"] == AXIS_KINK:
            Xb = (d["bc_const"] * xi_e - p * 1.0) / q
        else:
            Xb = -(p * 1.0) / q
        xi_i = Xb / d["x_boundary"]
        outer, inner = xi_e.rows(w.shape).copy(), xi_i.rows(w.shape).copy()
    fin = np.isfinite(outer[0] - inner[0]) & np.isfinite(outer).all(axis=0) & np.isfinite(inner).all(axis=0)
    st = np.where((st == ST_OK) & ~fin, ST_NONFINITE, st).astype(np.uint8)
    bad = st != ST_OK
    outer[:, bad] = np.nan + 1j * np.nan
    inner[:, bad] = np.nan + 1j * np.nan
    return outer, inner, st


def rel_of(M, outer, inner):
    """the rel of section 14 (percent) from rows 0 of jets"""
    with np.errstate(all="ignore"):
        sc = np.abs(outer[0]) if M.d.get("accept_norm", 0) else np.maximum(np.abs(outer[0]), np.abs(inner[0]))
        return np.abs(outer[0] - inner[0]) * 100.0 / sc


# ---- Cauchy's formula on the model -------------------------------------------------------------------------------------------
def model_parts(M, k, w):
    """np.array([outer, inner]) of CylComplexModel at one pair; k may be complex (eval's float(k) bypassed)"""
    w = np.atleast_1d(np.asarray(w, dtype=complex))
    with np.errstate(all="ignore"):
        st, xi_e = M.exterior(k, w)
        p, q = M.row(k, w)
        _, outer, inner, _, _ = M._finish(st, xi_e, p, q)
    return np.array([outer[0], inner[0]])


def cauchy_parts(M, k, w, r=1e-2, n=32):
    """(d/d omega, d/dk) of [outer, inner] of the model at the pair by Cauchy's formula, and the relative disagreement of
    the radii r and r / 2 (the condition under which the figures may be used)."""
    out, worst = [], 0.0
    for f, z0 in ((lambda z: model_parts(M, k, z), complex(w)), (lambda z: model_parts(M, z, w), complex(k))):
        a, b = cauchy(f, z0, r, n), cauchy(f, z0, 0.5 * r, n)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
        out.append(a)
    return out[0], out[1], worst


# ---- Newton's iteration, the rule of es_cyl_complex_newton -------------------------------------------------------------------
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


# ---- roots of the model and the slope of its root curve ----------------------------------------------------------------------
def model_root(M, k, guess):
    """the root of the model's D_c next to `guess`: its secant iteration run to convergence"""
    w = M.secant(float(k), complex(guess), complex(guess) + 1e-4 * (1 + 1j))
    assert w is not None, (k, guess)
    return complex(w)


def curve_slope(M, k, w, slope_guess):
    """d omega / dk of the model's root curve through (k, w): central differences of re-solved roots at k +- 1e-3 and
    k +- 5e-4, Richardson-combined.  slope_guess only places the secant starts."""
    s = []
    for dk in (1e-3, 5e-4):
        hi = model_root(M, k + dk, w + slope_guess * dk)
        lo = model_root(M, k - dk, w - slope_guess * dk)
        s.append((hi - lo) / (2.0 * dk))
    return (4.0 * s[1] - s[0]) / 3.0


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def problems(n_nodes=N0):
    """name -> (equilibrium, mode, m): the three jets of DESIGN 8i (kink), the sausage mode of the narrow one, a density
    cylinder, m = 3, and r_sign = +1"""
    from eigensolver_amd import equilibrium as q
    return {
        "kh_w1e5": (q.CylinderFlow(**KH, width=1e5, n_nodes=n_nodes), "kink", None),
        "kh_w3": (q.CylinderFlow(**KH, width=3.0, n_nodes=n_nodes), "kink", None),
        "kh_w15": (q.CylinderFlow(**KH, width=1.5, n_nodes=n_nodes), "kink", None),
        "sausage": (q.CylinderFlow(**KH, width=1.5, n_nodes=n_nodes), "sausage", None),
        "density": (q.CylinderDensity(width=0.95, n_nodes=n_nodes), "kink", None),
        "m3": (q.CylinderFlow(U_i0=0.35, width=0.9, n_nodes=n_nodes), "kink", 3),
        "rplus": (q.CylinderDensity(width=1.5, c_e=1.5, vA_e=0.5, r_sign=1.0, n_nodes=n_nodes, ic=(1e-8, 1e-8)), "kink", None),
    }


KH_NAMES = {1e5: "kh_w1e5", 3.0: "kh_w3", 1.5: "kh_w15"}
# the five problem kinds of the GPU tests: the narrow jet's kink and sausage modes, a density cylinder, m = 3, r_sign = +1
KINDS = ("kh_w15", "sausage", "density", "m3", "rplus")
# non-root pairs (k, omega) of each kind, both signs of Im omega, inside the kind's non-leaky window (the windows of
# tests/test_cyl_complex_gpu.py)
NON_ROOT = {
    "kh_w1e5": ((2.0, 2.1 + 0.3j), (2.0, 2.6 - 0.2j)),
    "kh_w3": ((2.0, 2.1 + 0.3j), (2.0, 2.6 - 0.2j)),
    "kh_w15": ((2.0, 2.1 + 0.3j), (2.0, 2.6 - 0.2j), (1.1, 1.2 + 0.15j)),
    "sausage": ((2.0, 2.2 + 0.25j), (2.0, 2.5 - 0.3j), (0.5, 0.6 + 0.1j)),
    "density": ((2.0, 6.0 + 0.4j), (2.0, 8.0 - 0.3j), (0.5, 1.8 + 0.1j)),
    "m3": ((2.0, 7.0 + 0.5j), (2.0, 9.0 - 0.4j), (1.1, 4.5 + 0.2j)),
    "rplus": ((2.0, 1.6 + 0.3j), (2.0, 2.6 - 0.25j), (1.1, 1.2 - 0.1j)),
}
# a pair with Re m_e < 0 for every kind: the phase speed above every exterior speed
LEAKY = {"kh_w15": (2.0, 8.0 + 0.1j), "sausage": (2.0, 8.0 + 0.1j), "density": (2.0, 30.0 + 0.1j), "m3": (2.0, 30.0 + 0.1j),
         "rplus": (2.0, 8.0 + 0.1j)}


@functools.lru_cache(maxsize=None)
def model(name, n_nodes=N0):
    eq, mode, m = problems(n_nodes)[name]
    return model_for(eq, mode, m)


@functools.lru_cache(maxsize=None)
def kh_root(width, n_nodes=N0):
    """the kink root of the table of DESIGN 8i polished on the model (the six digits above are where the table states it)"""
    return model_root(model(KH_NAMES[width], n_nodes), K0, KH_ROOTS[width])


def cauchy_pairs():
    """[(name, k, w, r)]: the three roots, and the first two non-root pairs (one of each sign of Im omega) of every problem
    kind, with the Cauchy radius"""
    out = [(KH_NAMES[wd], K0, kh_root(wd), 1e-2) for wd in KH_ROOTS]
    for name in KINDS:
        out += [(name, k, w, 1e-2) for k, w in NON_ROOT[name][:2]]
    return out


@functools.lru_cache(maxsize=None)
def slope_cases():
    """{width: (model, k, root, curve slope)} of the three KH roots, computed once per session"""
    out = {}
    for wd in KH_ROOTS:
        M = model(KH_NAMES[wd])
        root = kh_root(wd)
        outer, inner, _ = jets(M, K0, root)
        out[wd] = (M, K0, root, curve_slope(M, K0, root, dwdk(outer, inner)[0]))
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
    assert np.all(st == ST_OK)
    return eq, mode, m, k, w, cg, dwdk(outer, inner)

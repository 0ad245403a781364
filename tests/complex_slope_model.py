"""Helper (not a test): yardsticks for es_complex_root_slopes and es_complex_newton (include/eigensolver_amd.h section 12).

  jets          NumPy forward-mode restatement of oracle.slab_complex.ComplexFlowSlab.eval_rk4 over the small jet class J
                (value, d/d omega, d/dk; complex arrays): the oracle's formulas, in its order, with omega = (w, 1, 0) and
                k = (k, 0, 1).  Returns outer[3, p], inner[3, p] and the status; row 0 is eval_rk4.
  cauchy        f'(z0) by the trapezoid rule on Cauchy's formula, (1 / M r) sum_m f(z0 + r e^{i t_m}) e^{-i t_m}: in omega
                and in k (the oracle takes a complex scalar k unchanged).  A different route from the jets, no step to
                trust -- and valid only where two radii agree (cauchy_parts reports the disagreement).
  newton_model  the iteration rule of es_complex_newton, step for step, on `jets`.
  oracle_root / curve_slope   roots of the oracle's own eval_rk4 polished by secant steps, and the slope d omega / dk of
                the root curve from roots re-solved at k +- 1e-3 and k +- 5e-4, Richardson-combined.
"""
import functools

import numpy as np

from oracle.slab_complex import ST_LEAKY, ST_NONFINITE, ST_OK, ComplexFlowSlab
from tests import complex_eigen_model as E

K0 = E.K0
KH_ROOT, NON_ROOT, LEAKY = E.KH_ROOT, E.NON_ROOT, E.LEAKY
# the two kink / sfx roots of the sheared slab (width 0.9) on three nodes at k = 0.5
N3_ROOTS = (-0.130510 - 0.256677j, 0.337941 - 0.225817j)
# the branch the densify test follows from k = 0.5 (width 0.9, N = 3, kink, sfx)
N3_UPPER = 0.164226 + 0.151410j
NEWTON_OFFSET = 0.02 + 0.015j

# worst |model - Cauchy| / max(|outer_x|, |inner_x|) over outer_w, inner_w, outer_k, inner_k of the required pairs, r = 1e-2,
# M = 32 (tests/test_complex_slope_model.py prints the figures of a run; the test's bound is 10 x this)
CAUCHY_MEASURED = 3.8e-14
# |d omega / dk (model) - curve slope| / max(1, |slope|) per case, measured the same way; bound 10 x
SLOPE_MEASURED = {"uniform": 1.8e-11, "n3": 1.1e-13}

# the real SFG flow slab whose real roots (the C port's search, tests/mode_signature_model.py) the complex path is checked on,
# and the worst |d omega / dk (this model, Im omega = 0) - c_g (tests/root_slope_model.py)| / max(1, |c_g|) over those roots,
# imaginary part included: the two NumPy models, measured by tests/test_complex_slope_model.py; bound 10 x
REAL_AXIS_CASE = "SFG_flow_kink_N130"
REAL_AXIS_MEASURED = 2.9e-15


# ---- jets ------------------------------------------------------------------------------------------------------------------
class J:
    """value and two derivative components, complex arrays of one shape"""
    __array_ufunc__ = None           # NumPy scalars and arrays on the left defer to the reflected operators

    def __init__(self, v, dw, dk):
        self.v, self.dw, self.dk = v, dw, dk

    @staticmethod
    def lift(a):
        return a if isinstance(a, J) else J(a, 0.0, 0.0)

    def __add__(self, o):
        o = J.lift(o)
        return J(self.v + o.v, self.dw + o.dw, self.dk + o.dk)

    __radd__ = __add__

    def __neg__(self):
        return J(-self.v, -self.dw, -self.dk)

    def __sub__(self, o):
        o = J.lift(o)
        return J(self.v - o.v, self.dw - o.dw, self.dk - o.dk)

    def __rsub__(self, o):
        return J.lift(o) - self

    def __mul__(self, o):
        o = J.lift(o)
        return J(self.v * o.v, self.v * o.dw + self.dw * o.v, self.v * o.dk + self.dk * o.v)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = J.lift(o)
        q = self.v / o.v
        return J(q, (self.dw - q * o.dw) / o.v, (self.dk - q * o.dk) / o.v)

    def __rtruediv__(self, o):
        return J.lift(o) / self

    def __pow__(self, n):
        assert n == 2
        return self * self

    def rows(self, shape):
        return np.array([np.broadcast_to(np.asarray(c, dtype=complex), shape) for c in (self.v, self.dw, self.dk)])


def jsqrt(a):
    s = np.sqrt(a.v)
    return J(s, a.dw / (2.0 * s), a.dk / (2.0 * s))


def jexp(a):
    e = np.exp(a.v)
    return J(e, e * a.dw, e * a.dk)


def _interior(o, x, k, w):
    """ComplexFlowSlab.interior_coefficients over jets -> (D, coeff, P_Ti, add)"""
    Om = w - k * float(o.U(x))
    Om2 = Om * Om
    S = o.c_i ** 2 + o.vA_i ** 2
    k2 = k * k
    kc2, kvA2, kcT2 = k2 * o.c_i ** 2, k2 * o.vA_i ** 2, k2 * o.cT_i2
    m0 = (kc2 - Om2) * (kvA2 - Om2) / (S * (kcT2 - Om2))
    dU, ddU = float(o.dU(x)), float(o.ddU(x))
    if o.variant == "sfx":
        D = 2.0 * k * dU * (Om2 / (Om2 - kc2) - kcT2 / (Om2 - kcT2)) / Om
    else:
        D = 2.0 * k * dU * ((Om2 - kcT2) + k2 * k2 * o.cT_i2 * o.c_i ** 2 / (S * (Om2 - kcT2))) / (Om * (Om2 - kc2))
    coeff = k * ddU / Om + k * dU * D / Om - m0
    P_Ti = o.rho_i * S * (kcT2 - Om2) / (Om * (kc2 - Om2))
    add = -(k * dU) / Om if o.variant == "sfx" else 0.0 * Om
    return D, coeff, P_Ti, add


def jets(o, k, w):
    """(outer[3, p], inner[3, p], status[p]) at the pairs k[p] (real, broadcast), w[p] (complex): eval_rk4 over jets.  Rows of
    a pair that is not ST_OK, or that holds a non-finite entry, are NaN."""
    w = np.atleast_1d(np.asarray(w, dtype=complex)).reshape(-1)
    kv = np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy()
    one, zero = np.ones_like(w), np.zeros_like(w)
    kj, wj = J(kv + 0j, zero, one), J(w, one, zero)
    with np.errstate(all="ignore"):
        # exterior (ComplexFlowSlab.exterior_constants, .exterior)
        Oe = wj - kj * o.U_e
        S = o.vA_e ** 2 + o.c_e ** 2
        k2, Oe2 = kj * kj, Oe * Oe
        m_e = ((k2 * o.vA_e ** 2 - Oe2) * (k2 * o.c_e ** 2 - Oe2)) / (S * (k2 * o.cT_e2 - Oe2))
        p_e = o.rho_e * S * (k2 * o.cT_e2 - Oe2) / (Oe * (k2 * o.c_e ** 2 - Oe2))
        mu = jsqrt(m_e)
        R = o.L_factor * 2.0 * np.pi / kj
        E2 = jexp(-2.0 * mu * (R - 1.0))
        gp, gm = o.ic[0] + o.ic[1] / mu, o.ic[0] - o.ic[1] / mu
        outer = p_e * (mu * (gp - E2 * gm) / (gp + E2 * gm))
        st = np.where(m_e.v.real < 0.0, ST_LEAKY, ST_OK)
        st = np.where((st == ST_OK) & ~np.isfinite(outer.v), ST_NONFINITE, st)
        # interior (ComplexFlowSlab.eval_rk4): the adjoint march of the eigenfunction model, over jets
        def coef(o, x, k, w):
            D, cf, _, _ = _interior(o, x, k, w)
            return -cf, -D

        p, q = E.adjoint_rk4(o, kj, wj, coef=coef, start=(J(one, zero, zero), J(zero, zero, zero)))
        # ComplexFlowSlab._finish
        sigma = -1.0 if o.mode == "sausage" else 1.0
        Vb = (wj - kj * float(o.U(-1.0))) / (wj - kj * o.U_e)
        sv = (sigma - p) * Vb / q
        _, _, PTi, add = _interior(o, -1.0, kj, wj)
        inner = PTi * (sv - add * Vb)
        d = outer.v - inner.v
    st = np.where((st == ST_OK) & ~np.isfinite(d), ST_NONFINITE, st).astype(np.uint8)
    outer, inner = outer.rows(w.shape).copy(), inner.rows(w.shape).copy()
    bad = (st != ST_OK) | ~np.isfinite(outer).all(axis=0) | ~np.isfinite(inner).all(axis=0)
    outer[:, bad] = np.nan + 1j * np.nan
    inner[:, bad] = np.nan + 1j * np.nan
    return outer, inner, st


def dwdk(outer, inner):
    return -(outer[2] - inner[2]) / (outer[1] - inner[1])


# ---- Cauchy's formula on the oracle ----------------------------------------------------------------------------------------
def cauchy(f, z0, r, M):
    """f'(z0) of a function holomorphic on the closed disc of radius r around z0, M-point trapezoid rule"""
    ph = np.exp(2j * np.pi * np.arange(M) / M)
    return sum(f(z0 + r * e) * np.conj(e) for e in ph) / (M * r)


def oracle_parts(o, k, w):
    """np.array([outer, inner]) of the oracle at one pair; k may be complex"""
    w = np.atleast_1d(np.asarray(w, dtype=complex))
    with np.errstate(all="ignore"):
        _, outer, _ = o.exterior(k, w)
        d, _, _ = o.eval_rk4(k, w)
    return np.array([outer[0], outer[0] - d[0]])


def cauchy_parts(o, k, w, r=1e-2, M=32):
    """(d/d omega, d/dk) of [outer, inner] of the oracle at the pair by Cauchy's formula, and the relative disagreement
    of the radii r and r / 2 (the condition under which the figures may be used)."""
    out, worst = [], 0.0
    for f, z0 in ((lambda z: oracle_parts(o, k, z), complex(w)), (lambda z: oracle_parts(o, z, w), complex(k))):
        a, b = cauchy(f, z0, r, M), cauchy(f, z0, 0.5 * r, M)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
        out.append(a)
    return out[0], out[1], worst


# ---- Newton's iteration, the rule of es_complex_newton ---------------------------------------------------------------------
def newton_model(o, k, guess, max_iter=8, step_cap=np.inf, max_shift=np.inf, tol_percent=4.0):
    """dict(w, resid, iters, flag, dwdk, status, steps) for one guess; steps: the |s| of every step taken"""
    w, iters, ok, steps = complex(guess), 0, True, []
    for _ in range(max_iter):
        outer, inner, st = jets(o, k, w)
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
    outer, inner, st = jets(o, k, w)
    with np.errstate(all="ignore"):
        D = outer[0, 0] - inner[0, 0]
        resid = abs(D) * 100.0 / max(abs(outer[0, 0]), abs(inner[0, 0]))
        slope = dwdk(outer, inner)[0]
    flag = bool(ok and st[0] == ST_OK and resid < tol_percent and abs(w - guess) <= max_shift)
    return dict(w=w, resid=resid, iters=iters, flag=int(flag), dwdk=slope, status=int(st[0]), steps=steps)


# ---- roots of the oracle and the slope of its root curve -------------------------------------------------------------------
def oracle_root(o, k, guess, steps=40):
    """the root of the oracle's eval_rk4 next to `guess`, by its secant rule run to a standstill"""
    ev = lambda z: o.eval_rk4(k, [z])[0][0]
    w0, w1 = complex(guess), complex(guess) + 1e-4 * (1 + 1j)
    f0, f1 = ev(w0), ev(w1)
    for _ in range(steps):
        df = f1 - f0
        if df == 0 or not np.isfinite(df):
            break
        w2 = w1 - f1 * (w1 - w0) / df
        if abs(w2 - w1) <= 2e-16 * max(1.0, abs(w1)):
            w1 = w2
            break
        w0, f0, w1 = w1, f1, w2
        f1 = ev(w1)
    return w1


def curve_slope(o, k, w, slope_guess):
    """d omega / dk of the oracle's root curve through (k, w): central differences of re-solved roots at k +- 1e-3 and
    k +- 5e-4, Richardson-combined.  slope_guess only places the secant starts."""
    s = []
    for dk in (1e-3, 5e-4):
        hi = oracle_root(o, k + dk, w + slope_guess * dk)
        lo = oracle_root(o, k - dk, w - slope_guess * dk)
        s.append((hi - lo) / (2.0 * dk))
    return (4.0 * s[1] - s[0]) / 3.0


def oracle_of(eq, mode, variant):
    """the oracle of a flow-slab equilibrium of eigensolver_amd.equilibrium"""
    return ComplexFlowSlab(c_i=eq.c_i0, vA_i=eq.vA_i0, c_e=eq.c_e, vA_e=eq.vA_e, rho_i=eq.rho_i0, rho_e=eq.rho_e, U_i0=eq.U_i0,
                           U_e=eq.U_e, width=eq.width, x0=eq.x0, mode=mode, L_factor=eq.L_factor, ic=eq.ic,
                           n_nodes=eq.n_nodes, variant=variant)


@functools.lru_cache(maxsize=None)
def real_axis_case():
    """(eq, k, w, c_g of the real model, d omega / dk of this model) at the real roots of REAL_AXIS_CASE"""
    from tests import mode_signature_model as S
    from tests import real_eigen_model as M
    from tests import root_slope_model as R
    eq, mode, _, _ = M.all_cases()[REAL_AXIS_CASE]
    k, w, _ = S.port_roots(REAL_AXIS_CASE)
    cg = R.group_velocity(*R.jets(REAL_AXIS_CASE, k, w))
    outer, inner, st = jets(oracle_of(eq, mode, "sfg"), k, w + 0j)
    assert np.all(st == ST_OK)
    return eq, k, w, cg, dwdk(outer, inner)


def slab(width, mode, variant, N):
    return ComplexFlowSlab(width=width, mode=mode, variant=variant, n_nodes=N)


@functools.lru_cache(maxsize=None)
def n3_roots():
    """the two N = 3 roots polished on the oracle (the six digits above are where the issue states them)"""
    o = slab(0.9, "kink", "sfx", 3)
    return tuple(oracle_root(o, K0, z) for z in N3_ROOTS)


@functools.lru_cache(maxsize=None)
def slope_cases():
    """{name: (oracle, k, root, curve slope)} of the two slope cases, computed once per session"""
    out = {}
    for name, o, z in (("uniform", slab(1e5, "kink", "sfx", 500), KH_ROOT), ("n3", slab(0.9, "kink", "sfx", 3), n3_roots()[1])):
        root = oracle_root(o, K0, z)
        outer, inner, _ = jets(o, K0, root)
        out[name] = (o, K0, root, curve_slope(o, K0, root, dwdk(outer, inner)[0]))
    return out


@functools.lru_cache(maxsize=None)
def window_roots(width, mode, variant, N):
    """the roots the oracle's find_roots flags 1 on complex_eigen_model.ROOT_WINDOW at k = K0, distinct"""
    r, _, flag = slab(width, mode, variant, N).find_roots(K0, *E.ROOT_WINDOW)
    keep = []
    for z in r[flag == 1]:
        if all(abs(z - y) > 1e-8 for y in keep):
            keep.append(z)
    return tuple(keep)

"""Helper (not a test): yardsticks for es_shoot_root_slopes (include/eigensolver_amd.h section 11).

  parts       NumPy restatement of the two sides of the matching condition, D(k, omega) = outer - inner, on the node grid:
              the coefficient sets of the oracle problem at node, mid-point, node; plain RK4 of the two columns of the
              transfer matrix from the boundary to the far end of the interior (the row the far-end condition picks is
              what the kernel's adjoint march delivers); the closed-form exterior with scipy.special.kve / ive.  Written
              complex-safe: every formula is analytic in k and omega (the normalisation by |P_b| takes the sign of the real
              part), so it can be evaluated at k + i eps or omega + i eps.
  jets        outer and inner with their derivatives in omega and k by the complex step, Im f(x + i 1e-30) / 1e-30: exact
              to rounding, no step to choose, and a different route from the kernel's forward-mode jets.
  curve_slope the slope d omega / dk of the root curve through a root of the C port: roots of the port re-solved at
              k +- 1e-3 and k +- 5e-4 (a 65-point window of +-1e-4 in omega around the predicted position, 48 bisections),
              the two central differences Richardson-combined.
"""
import functools

import numpy as np
from scipy import special

from eigensolver_amd import equilibrium as q
from eigensolver_amd import shooting as sh
from tests import cases
from tests import mode_signature_model as S
from tests import real_eigen_model as M

EPS = 1e-30

# the pairs the value tests run on: every standard case, the short grids and both `gap` branches of the cylinder exterior
VALUE_CASES = M.STANDARD + tuple(f"{a}_N{N}" for N in M.SMALL_N for a in ("CF_flow_kink", "SFG_flow_kink"))
# jets against the model: four families, m = 3 and 5, N = 2, 3, 130, both axis conditions, the rotation kink condition and a
# non-zero axis target of the untwisted cylinder (the one problem whose march scale enters the determinant)
JET_CASES = ("CF_flow_kink_N2", "CF_flow_kink_N3", "CF_flow_kink_N130", "SFG_flow_kink_N2", "SFG_flow_kink_N3",
             "SFG_flow_kink_N130", "CF_flow_sausage", "CF_flow_m3", "CF_flow_m5", "CF_flow_kink_target", "CDC_w095_kink",
             "CR_kink", "CR_sausage", "SD_w15_sausage", "SD_w15_kink", "SFG_flow_sausage", "SFU_sausage")
# c_g at the port's roots against the root-curve slope
SLOPE_CASES = ("CF_flow_kink_N130", "SFG_flow_kink_N130", "CF_flow_sausage", "SD_w15_sausage", "CR_kink")
SLOPE_ROOTS = {"CF_flow_kink_N130": 7, "SFG_flow_kink_N130": 12, "CF_flow_sausage": 8, "SD_w15_sausage": 7, "CR_kink": 9}
# 10 x the worst |c_g(model) - curve slope| / max(1, |slope|) of the case, measured with this file (DESIGN.md section 8f;
# tests/test_root_slope_model.py prints the figures): the factor covers the Richardson remainder and the 4e-16 root accuracy
# divided by the k step
SLOPE_MEASURED = {"CF_flow_kink_N130": 1.4e-12, "SFG_flow_kink_N130": 2.5e-12, "CF_flow_sausage": 4.0e-12,
                  "SD_w15_sausage": 2.0e-12, "CR_kink": 1.3e-12}


def slope_bound(name):
    return 10.0 * SLOPE_MEASURED[name]


def pairs(name):
    """(k, w) of a case: its fixed pairs; the large-gap cases use their gap-targeted pairs."""
    return M.large_gap_pairs(name) if name in M.LARGE_GAP else M.pairs(name)


@functools.lru_cache(maxsize=None)
def _desc(name):
    eq, mode, m, _ = M.all_cases()[name]
    return sh.make_desc(eq, mode, m)[0]


def _matrices(name, k, w):
    """A[2, 2, 2N - 1, p] of y' = A y at the nodes and mid-points, boundary first, for the pair arrays k[p], w[p] (complex or
    real); state (P, Xi = r xi_r) for cylinders, (Vx, F Vx') for the density slab, (Vx, Vx') for the flow slabs."""
    eq = M.all_cases()[name][0]
    prob = M.problem(name)
    x = np.linspace(eq.x_boundary, eq.x_end, 2 * eq.n_nodes - 1)[:, None]
    k, w = k[None, :], w[None, :]
    zero = np.zeros((x.shape[0], k.shape[1]), dtype=np.result_type(k, w))
    if M.is_cyl(eq):
        D, C1, C2, C3, _, _ = prob.coefficients(x, k, w)
        return np.array([[-C1 / D, C3 / (x * D)], [-x * C2 / D, C1 / D]])
    rho, c2, vA2, S, cT2, Om, m0, F = prob._coef(x, k, w)
    if isinstance(eq, q.SlabDensity):
        return np.array([[zero, 1.0 / F], [F * m0, zero]])
    k2 = k * k
    dU, ddU = prob.eq.dU(x), prob.eq.ddU(x)
    t = Om ** 2 - k2 * cT2
    Dref = 2.0 * k * dU * (t + (k2 * k2 * cT2 * c2) / (S * t)) / (Om * (Om ** 2 - k2 * c2))
    coeff = k * ddU / Om + k * dU * Dref / Om - m0
    return np.array([[zero, zero + 1.0], [-coeff, -Dref]])


def _mul(A, Y):
    """A[2, 2, p] times Y[2, 2, p], per pair"""
    return np.array([[A[0, 0] * Y[0, 0] + A[0, 1] * Y[1, 0], A[0, 0] * Y[0, 1] + A[0, 1] * Y[1, 1]],
                     [A[1, 0] * Y[0, 0] + A[1, 1] * Y[1, 0], A[1, 0] * Y[0, 1] + A[1, 1] * Y[1, 1]]])


def _transfer(name, A):
    """RK4 of the two columns (1, 0), (0, 1) from the boundary over the node grid -> T[2, 2, p]"""
    eq = M.all_cases()[name][0]
    n = eq.n_nodes
    h = (eq.x_end - eq.x_boundary) / (n - 1)
    p = A.shape[-1]
    one, zero = np.ones(p, dtype=A.dtype), np.zeros(p, dtype=A.dtype)
    Y = np.array([[one, zero], [zero, one]])
    for j in range(n - 1):
        A0, Am, A1 = A[:, :, 2 * j], A[:, :, 2 * j + 1], A[:, :, 2 * j + 2]
        k1 = _mul(A0, Y)
        k2 = _mul(Am, Y + (0.5 * h) * k1)
        k3 = _mul(Am, Y + (0.5 * h) * k2)
        k4 = _mul(A1, Y + h * k3)
        Y = Y + (h / 6.0) * (k1 + k4) + (h / 3.0) * (k2 + k3)
    return Y


def _sign_re(z):
    return np.where(np.real(z) < 0.0, -1.0, 1.0)


def _exterior(name, k, w):
    """(cst, yb, dyb, Oe): the constant of the outer side, the exterior solution and its derivative at the boundary scaled to
    |yb| = 1, the Doppler-shifted exterior frequency.  The scaled Bessel functions are the analytic e^z K(z), e^-z I(z)."""
    d = _desc(name)
    eq = M.all_cases()[name][0]
    k2 = k * k
    vAe2, ce2, cTe2 = d.vA_e ** 2, d.c_e ** 2, d.cT_e ** 2
    R = d.L_factor * 2.0 * np.pi / k
    if M.is_cyl(eq):
        w2 = w * w
        m_e = ((k2 * vAe2 - w2) * (k2 * ce2 - w2)) / ((vAe2 + ce2) * (k2 * cTe2 - w2))
        cst = -1.0 / (d.rho_e * (k2 * vAe2 - w2))
        mu = np.sqrt(m_e)
        sgn = -1.0 if d.x_boundary < 0 else 1.0
        n = float(d.m_ext)
        xR, xb = mu * R, mu

        def K_pair(z):
            a, b = special.kve(n, z), special.kve(n + 1, z)
            return a, -b + (n / z) * a

        def I_pair(z):                                      # ive scales by exp(-|Re z|): the phase makes it exp(-z)
            ph = np.exp(-1j * np.imag(z)) if np.iscomplexobj(z) else 1.0
            a, b = special.ive(n, z) * ph, special.ive(n + 1, z) * ph
            return a, b + (n / z) * a
        KR, dKR = K_pair(xR)
        Kb, dKb = K_pair(xb)
        IR, dIR = I_pair(xR)
        Ib, dIb = I_pair(xb)
        g = d.ic_slope / (sgn * mu)
        a_s = -(d.ic_value * dKR - g * KR)
        b_s = -(g * IR - d.ic_value * dIR)
        E2 = np.exp(-2.0 * (xR - xb))
        P = b_s * Kb + E2 * a_s * Ib
        dP = sgn * mu * (b_s * dKb + E2 * a_s * dIb)
        nrm = _sign_re(P) * P
        return cst, P / nrm, dP / nrm, w
    Oe = w - k * d.U_e
    Oe2 = Oe * Oe
    m_e = ((k2 * vAe2 - Oe2) * (k2 * ce2 - Oe2)) / ((vAe2 + ce2) * (k2 * cTe2 - Oe2))
    cst = d.rho_e * (vAe2 + ce2) * (k2 * cTe2 - Oe2) / (Oe * (k2 * ce2 - Oe2))
    mu = np.sqrt(m_e)
    E2 = np.exp(-2.0 * mu * (R - 1.0))
    gp, gm = d.ic_value + d.ic_slope / mu, d.ic_value - d.ic_slope / mu
    V = gp + E2 * gm
    dV = mu * (gp - E2 * gm)
    nrm = _sign_re(V) * V
    return cst, V / nrm, dV / nrm, Oe


def parts(name, k, w):
    """(outer[p], inner[p]) at the pair arrays k[p], w[p], real or complex."""
    k, w = np.atleast_1d(k), np.atleast_1d(w)
    dt = np.result_type(k, w, np.float64)
    k, w = k.astype(dt), w.astype(dt)
    d = _desc(name)
    eq = M.all_cases()[name][0]
    A = _matrices(name, k, w)
    T = _transfer(name, A)
    cst, yb, dyb, Oe = _exterior(name, k, w)
    outer = cst * dyb
    if M.is_cyl(eq):
        if d.axis_bc == sh.AXIS_SAUSAGE:                    # P'(r_ax) = a11 P + a12 Xi = 0
            a11, a12 = A[0, 0, -1], A[0, 1, -1]
            r1, r2, target = a11 * T[0, 0] + a12 * T[1, 0], a11 * T[0, 1] + a12 * T[1, 1], 0.0
        else:                                               # P(r_ax) = +- c xi_e
            r1, r2 = T[0, 0], T[0, 1]
            target = (1.0 if d.axis_bc == sh.AXIS_KINK else -1.0) * d.bc_const * outer
        return outer, (target - r1 * yb) / r2 / d.x_boundary
    sigma = -1.0 if d.slab_mode == 0 else 1.0
    r1, r2 = T[0, 0], T[0, 1]
    if isinstance(eq, q.SlabDensity):
        return outer, (sigma - r1) * yb / r2 / w
    c2, vA2 = d.c_i ** 2, d.vA_i ** 2
    cT2 = c2 * vA2 / (c2 + vA2)
    Omb = w - k * float(M.problem(name).eq.U(np.array([-1.0]))[0])
    sv = (sigma - r1) * (yb * Omb / Oe) / r2
    PTi = d.rho_i * (c2 + vA2) * (k * k * cT2 - Omb ** 2) / (Omb * (k * k * c2 - Omb ** 2))
    return outer, PTi * sv


def jets(name, k, w):
    """(outer[3, p], inner[3, p]): value, d/d omega, d/dk by the complex step, all pairs in one batch."""
    k, w = np.atleast_1d(np.asarray(k, dtype=np.float64)), np.atleast_1d(np.asarray(w, dtype=np.float64))
    p = len(k)
    kk = np.concatenate([k + 0j, k + 1j * EPS])
    ww = np.concatenate([w + 1j * EPS, w + 0j])
    o, i = parts(name, kk, ww)
    return (np.array([o[:p].real, o[:p].imag / EPS, o[p:].imag / EPS]),
            np.array([i[:p].real, i[:p].imag / EPS, i[p:].imag / EPS]))


@functools.lru_cache(maxsize=None)
def case_jets(name):
    """jets at pairs(name), computed once per session; callers must not modify the arrays"""
    return jets(name, *pairs(name))


def group_velocity(outer, inner):
    return -(outer[2] - inner[2]) / (outer[1] - inner[1])


# ---- the slope of the root curve, from the C port ------------------------------------------------------------------------------
DK = (1e-3, 5e-4)
WINDOW, NWIN, NBISECT = 1e-4, 65, 48


def _port_root_near(port, k, w_pred):
    """the root of the port's determinant in the row k nearest to w_pred inside the window; None if there is none"""
    kk = np.array([k])
    wg = w_pred + np.linspace(-WINDOW, WINDOW, NWIN)
    D, _, st = port.eval_grid(kk, wg, w_mode=0, nthreads=1)
    r, cnt = port.find_roots(kk, wg, D, st, w_mode=0, n_bisect=NBISECT, tol=1e-3, nthreads=1)
    if cnt == 0:
        return None
    return float(r["w"][int(np.argmin(np.abs(r["w"] - w_pred)))])


@functools.lru_cache(maxsize=None)
def curve_slopes(name):
    """(k, w, slope) of every accepted root of the port on the 8 x 400 grid (mode_signature_model.port_roots); slope is NaN
    where one of the four neighbouring roots was not found (the tests allow none).  The prediction of the neighbours uses the
    model's own c_g, which only centres the window."""
    eq, mode, m, _ = M.all_cases()[name]
    port = cases.port_problem(eq, mode, m)
    k, w, _ = S.port_roots(name)
    cg = group_velocity(*jets(name, k, w))
    out = np.full(len(k), np.nan)
    for i in range(len(k)):
        s = []
        for dk in DK:
            hi = _port_root_near(port, k[i] + dk, w[i] + cg[i] * dk)
            lo = _port_root_near(port, k[i] - dk, w[i] - cg[i] * dk)
            s.append(np.nan if hi is None or lo is None else (hi - lo) / (2.0 * dk))
        out[i] = (4.0 * s[1] - s[0]) / 3.0
    return k, w, out

"""Helper (not a test): NumPy restatement of es_complex_eigenfunction and its DOP853 truth, on oracle.slab_complex.

The algorithm (include/eigensolver_amd.h section 6, eigensolver_amd/csrc/es_complex.hip):
  exterior   closed form, decaying branch, per unit V_e(-1):  with mu = sqrt(m_e) (principal), R = L 2 pi / k,
             gp / gm = ic0 +- ic1 / mu, E2(a) = exp(-2 mu (R - a)),
               Vx_e(x)      =        e^{-mu (|x| - 1)} (gp + E2(|x|) gm) / (gp + E2(1) gm)
               p_e Vx_e'(x) = p_e mu e^{-mu (|x| - 1)} (gp - E2(|x|) gm) / (gp + E2(1) gm)
  interior   u' = v, v' = a21 u + a22 v on linspace(-1, 1, N), one RK4 step per interval with the coefficient sets at
             node, mid-point, node:
               1. adjoint march of (1, 0) from x = +1 to x = -1 -> (zp, zq):  Vx(+1) = zp u(-1) + zq v(-1)
               2. u(-1) = Vb = Omega(-1) / Omega_e,  v(-1) = (sigma - zp) Vb / zq,  sigma = -1 sausage, +1 kink
               3. forward march from x = -1 to x = +1, value = u, flux = P_Ti (v - add u) at every node
`model` is that algorithm, `truth` replaces the two RK4 marches by DOP853 (rtol 1e-12) on both columns of the transfer
matrix, evaluated on the nodes.  Both take one wavenumber per frequency (k is broadcast against w).
"""
import functools

import numpy as np
from scipy.integrate import solve_ivp

from oracle.slab_complex import ST_NONFINITE, ST_OK, ComplexFlowSlab

KH_ROOT = 0.3128068480162605 + 0.09428139628771133j          # kink, uniform flow, k = 0.5 (tests/test_complex_gpu.py:108)
NON_ROOT = 0.21 + 0.13j
LEAKY = 1.5 + 0.1j                                           # Re(m_e) < 0 at k = 0.5
K0 = 0.5
ROOT_WINDOW = (np.linspace(-0.25, 0.5, 16), np.linspace(-0.25, 0.25, 12))      # tests/test_complex_gpu.py:82


def bound(N):
    """The project's eigenfunction bound for RK4 on the node grid against DOP853 (tests/test_eigenfunction_gpu.py:38)."""
    return 2e-6 * max(1.0, (1000.0 / N) ** 4)


def sigma(o):
    return -1.0 if o.mode == "sausage" else 1.0


def _coef(o, x, k, w):
    _, D, cf, _, _ = o.interior_coefficients(x, k, w)
    return -cf, -D                                           # a21, a22 (a11 = 0, a12 = 1)


def adjoint_rk4(o, k, w, coef=_coef, start=None):
    """(zp, zq): the row (T11, T12) of the transfer matrix from -1 to +1, by the transposed march of eval_rk4.
    coef(o, x, k, w) -> (a21, a22) and start = (p, q) at x = +1 (default: 1, 0) let another number type make the same
    march (tests/complex_slope_model.py: jets)."""
    N = o.n_nodes
    x = np.linspace(-1.0, 1.0, 2 * N - 1)
    h = 2.0 / (N - 1)
    p, q = (np.ones_like(w), np.zeros_like(w)) if start is None else start

    def rhs(a, pp, qq):
        return a[0] * qq, pp + a[1] * qq

    with np.errstate(all="ignore"):
        B0 = coef(o, x[2 * (N - 1)], k, w)
        for j in range(N - 2, -1, -1):
            Bm, B1 = coef(o, x[2 * j + 1], k, w), coef(o, x[2 * j], k, w)
            k1p, k1q = rhs(B0, p, q)
            k2p, k2q = rhs(Bm, p + 0.5 * h * k1p, q + 0.5 * h * k1q)
            k3p, k3q = rhs(Bm, p + 0.5 * h * k2p, q + 0.5 * h * k2q)
            k4p, k4q = rhs(B1, p + h * k3p, q + h * k3q)
            p = p + h / 6.0 * (k1p + k4p) + h / 3.0 * (k2p + k3p)
            q = q + h / 6.0 * (k1q + k4q) + h / 3.0 * (k2q + k3q)
            B0 = B1
    return p, q


def forward_rk4(o, k, w, u0, v0):
    """(u, v)[n, N] on the nodes, from (u0, v0) at x = -1, with the node / mid-point / node sets of the adjoint march."""
    N = o.n_nodes
    x = np.linspace(-1.0, 1.0, 2 * N - 1)
    h = 2.0 / (N - 1)
    u, v = np.array(u0, dtype=complex), np.array(v0, dtype=complex)
    U, V = np.empty((w.size, N), complex), np.empty((w.size, N), complex)
    U[:, 0], V[:, 0] = u, v

    def rhs(a, uu, vv):
        return vv, a[0] * uu + a[1] * vv

    with np.errstate(all="ignore"):
        A0 = _coef(o, x[0], k, w)
        for j in range(N - 1):
            Am, A1 = _coef(o, x[2 * j + 1], k, w), _coef(o, x[2 * j + 2], k, w)
            k1u, k1v = rhs(A0, u, v)
            k2u, k2v = rhs(Am, u + 0.5 * h * k1u, v + 0.5 * h * k1v)
            k3u, k3v = rhs(Am, u + 0.5 * h * k2u, v + 0.5 * h * k2v)
            k4u, k4v = rhs(A1, u + h * k3u, v + h * k3v)
            u = u + h / 6.0 * (k1u + k4u) + h / 3.0 * (k2u + k3u)
            v = v + h / 6.0 * (k1v + k4v) + h / 3.0 * (k2v + k3v)
            A0 = A1
            U[:, j + 1], V[:, j + 1] = u, v
    return U, V


def exterior_closed_form(o, k, w, n_ext):
    """x_ext [n, n_ext] = linspace(-R, -1, n_ext) per pair, Vx_e and p_e Vx_e' per unit V_e(-1)."""
    m_e, p_e = o.exterior_constants(k, w)
    R = o.L_factor * 2.0 * np.pi / k
    x = np.stack([np.linspace(-r, -1.0, n_ext) for r in R]) if n_ext else np.zeros((w.size, 0))
    with np.errstate(all="ignore"):
        mu = np.sqrt(m_e)[:, None]
        ax, R = np.abs(x), R[:, None]
        gp, gm = o.ic[0] + o.ic[1] / mu, o.ic[0] - o.ic[1] / mu
        den = gp + np.exp(-2.0 * mu * (R - 1.0)) * gm
        E2x, dec = np.exp(-2.0 * mu * (R - ax)), np.exp(-mu * (ax - 1.0))
        value = dec * (gp + E2x * gm) / den
        flux = p_e[:, None] * mu * dec * (gp - E2x * gm) / den
    return x, value, flux


def _assemble(o, k, w, n_ext, u, v):
    """Fluxes, status and NaN rows from the interior state (u, v)[n, N]; shared by model and truth."""
    x_int = np.linspace(-1.0, 1.0, o.n_nodes)
    st, outer, _ = o.exterior(k, w)
    with np.errstate(all="ignore"):
        _, _, _, PTi, add = o.interior_coefficients(x_int[None, :], k[:, None], w[:, None])
        flux_int = PTi * (v - add * u)
        d = outer - flux_int[:, 0]
    st = np.where((st == ST_OK) & ~np.isfinite(d), ST_NONFINITE, st).astype(np.uint8)
    x_ext, value_ext, flux_ext = exterior_closed_form(o, k, w, n_ext)
    bad = st != ST_OK
    value_int, flux_int = u.copy(), flux_int.copy()
    for a in (value_int, flux_int, value_ext, flux_ext):
        a[bad] = np.nan + 1j * np.nan
    return dict(x_int=x_int, value_int=value_int, flux_int=flux_int, x_ext=x_ext, value_ext=value_ext,
                flux_ext=flux_ext, status=st, outer=outer, D=np.where(bad, np.nan + 0j, d))


def _pairs(k, w):
    w = np.atleast_1d(np.asarray(w, dtype=complex)).reshape(-1)
    return np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy(), w


def boundary_value(o, k, w):
    return (w - k * o.U(-1.0)) / (w - k * o.U_e)             # SF-X:422


def model(o, k, w, n_ext=500):
    k, w = _pairs(k, w)
    zp, zq = adjoint_rk4(o, k, w)
    with np.errstate(all="ignore"):
        Vb = boundary_value(o, k, w)
        sv = (sigma(o) - zp) * Vb / zq
    u, v = forward_rk4(o, k, w, Vb, sv)
    return _assemble(o, k, w, n_ext, u, v)


def truth(o, k, w, n_ext=500, rtol=1e-12):
    k, w = _pairs(k, w)
    N = o.n_nodes
    x_int = np.linspace(-1.0, 1.0, N)
    st, _, _ = o.exterior(k, w)
    u, v = np.full((w.size, N), np.nan + 0j), np.full((w.size, N), np.nan + 0j)
    for i in range(w.size):
        if st[i] != ST_OK:
            continue

        def f(x, y, ki=k[i], wi=w[i]):
            _, D, cf, _, _ = o.interior_coefficients(x, ki, wi)
            return [y[1], -D * y[1] - cf * y[0], y[3], -D * y[3] - cf * y[2]]

        sol = solve_ivp(f, (-1.0, 1.0), np.array([1, 0, 0, 1], dtype=complex), method="DOP853", rtol=rtol, atol=1e-30,
                        t_eval=x_int)
        T11, T21, T12, T22 = sol.y
        Vb = boundary_value(o, k[i], w[i])
        sv = (sigma(o) - T11[-1]) * Vb / T12[-1]
        u[i], v[i] = Vb * T11 + sv * T12, Vb * T21 + sv * T22
    return _assemble(o, k, w, n_ext, u, v)


def uniform_closed_form(o, k, w, x):
    """Kink mode of the uniform slab: Vx = Vb cosh(m x) / cosh(m) with m^2 = m0 at U = U_i0."""
    m0, _, _, _, _ = o.interior_coefficients(0.0, k, w)
    m = np.sqrt(m0)
    Vb = w - k * o.U_i0
    return Vb / (w - k * o.U_e) * np.cosh(m * x) / np.cosh(m)


# ---- the points both test files use -------------------------------------------------------------------------------------
def slab(width, mode, variant, N):
    return ComplexFlowSlab(width=width, mode=mode, variant=variant, n_nodes=N)


@functools.lru_cache(maxsize=None)
def sausage_roots(N):
    """Converged roots of the sheared sausage / sfg slab on ROOT_WINDOW (near 0.000717 +- 0.087469i)."""
    o = slab(0.9, "sausage", "sfg", N)
    r, rel, flag = o.find_roots(K0, *ROOT_WINDOW)
    keep = []
    for z in r[(flag == 1) & (rel < 1e-2)]:
        if all(abs(z - y) > 1e-8 for y in keep):
            keep.append(z)
    return tuple(keep)


def cases(N):
    """[(name, width, mode, variant, w array)] at k = K0."""
    return [("kh_root", 1e5, "kink", "sfx", np.array([KH_ROOT])),
            ("sausage_roots", 0.9, "sausage", "sfg", np.array(sausage_roots(N))),
            ("off_kink_sfx", 0.9, "kink", "sfx", np.array([NON_ROOT])),
            ("off_kink_sfg", 0.9, "kink", "sfg", np.array([NON_ROOT])),
            ("off_sausage_sfg", 0.9, "sausage", "sfg", np.array([NON_ROOT]))]


@functools.lru_cache(maxsize=None)
def _truth_case(N, name):
    for nm, width, mode, variant, w in cases(N):
        if nm == name:
            return truth(slab(width, mode, variant, N), K0, w, n_ext=500)
    raise KeyError(name)


def truth_case(N, name):
    """DOP853 truth of a case, computed once per session; callers must not modify the arrays."""
    return _truth_case(N, name)

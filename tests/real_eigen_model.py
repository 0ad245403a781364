"""Helper (not a test): yardsticks for es_shoot_eigenfunction (include/eigensolver_amd.h section 5).

  truth      oracle.cylinder.eigenfunction_outward / oracle.slab.eigenfunction: DOP853 at rtol 1e-12, closed-form exterior
             with its two terms apart.
  grid_rk4   plain NumPy RK4 of the oracle problem's _rhs on the node grid, coefficient sets at node, mid-point, node, in
             the kernel's state variables: (P, Xi = r xi_r) for cylinders, (Vx, F Vx') for the density slab, (Vx, Vx') for
             the flow slabs.  Either direction; the state arithmetic runs in the dtype of y_start (np.longdouble gives the
             rounding yardstick E_round), the coefficient sets are the oracle's float64 ones in both.
  pairs      fixed (k, omega) pairs per case, drawn with a seed inside the case's phase-speed window, away from the
             exterior cut-offs and outside the continua.  They are NOT roots: the two-region solution is defined at any
             ES_PT_OK pair.

The kernel writes the cylinder interior by a march from the axis point out to the boundary (the singular solution decays
that way) and the slab interior from x = -1 to x = +1; `write_nodes` gives the nodes in that order.
"""
import dataclasses
import functools
import zlib

import numpy as np

from eigensolver_amd import equilibrium as q
from oracle import cylinder as oc
from oracle import slab as osl
from tests import cases

N_PAIRS = 4


def bound(N):
    """The project's eigenfunction bound for RK4 on the node grid against DOP853, of max|field| per array."""
    return 2e-6 * max(1.0, (1000.0 / N) ** 4)


# The rotational kink condition P(r_ax) = -c xi_e keeps the singular solution (xi_r ~ 1/r^2) in the answer itself: on the
# uniform grid h / r is 0.5 to 1 at the last nodes, where RK4 is good to ~1e-3 of the (huge) axis value only.  Interior
# arrays of such a case: 1e-3 of max|field| on the whole interval and 2e-5 of the maximum over |r| >= 0.02 on that part --
# the allowances tests/test_eigenfunction_gpu.py has had for it from the start.
SINGULAR_AXIS = ("CR_kink",)
SINGULAR_AXIS_BOUND, SINGULAR_AXIS_FAR, SINGULAR_AXIS_FAR_BOUND = 1e-3, 0.02, 2e-5


def interior_error(name, key, got, want, x):
    """(measured, bound) pairs of one interior array against the truth, under the bounds above."""
    N = len(x)
    err = np.abs(got - want)
    if name in SINGULAR_AXIS:
        far = np.abs(x) >= SINGULAR_AXIS_FAR
        return [(float(np.max(err) / np.max(np.abs(want))), SINGULAR_AXIS_BOUND),
                (float(np.max(err[far]) / np.max(np.abs(want[far]))), SINGULAR_AXIS_FAR_BOUND)]
    return [(float(np.max(err) / np.max(np.abs(want))), bound(N))]


class FlowWithAxisTarget(q.CylinderFlow):
    """An un-twisted cylinder (FAM_CYL0) whose kink condition has a non-zero target P(r_ax) = 0.37 xi_e: the one
    configuration in which the problem's two copies of the constant differ (the fp64 determinant marches of this family
    carry a scale that the constant absorbs; the eigenfunction kernel needs it as given)."""

    def bc_const(self, axis_bc):
        return 0.37

    def plain(self):
        return q.CylinderFlow(**dataclasses.asdict(self))


SMALL_N = (130, 2, 3)


@functools.lru_cache(maxsize=None)
def all_cases():
    """tests/cases.py plus one m = 5 cylinder, the four large-gap problems (far field at 10 wavelengths), a cylinder with a
    non-zero axis target and short grids (N = 130: three workgroups' worth of pairs stay cheap; N = 2, 3: one and two steps; the
    density slab at N = 2)."""
    c = dict(cases.all_cases())
    c["CF_flow_kink_target"] = (FlowWithAxisTarget(U_i0=0.6, width=1.0), "kink", None, (2.7, 4.95))
    for N in SMALL_N:
        c[f"CF_flow_kink_N{N}"] = (q.CylinderFlow(U_i0=0.6, width=1.0, n_nodes=N), "kink", None, (2.7, 4.95))
        c[f"SFG_flow_kink_N{N}"] = (q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=N), "kink", None, (1.4, 2.45))
    c["SD_w15_sausage_N2"] = (q.SlabDensity(width=1.5, n_nodes=2), "sausage", None, (0.9, 1.25))
    c["CF_flow_m5"] = (q.CylinderFlow(U_i0=0.35, width=0.9), "kink", 5, (2.7, 4.95))
    c["LG_flow_kink"] = (q.CylinderFlow(U_i0=0.6, width=1.0, L_factor=10.0), "kink", None, (2.7, 4.95))
    c["LG_flow_sausage"] = (q.CylinderFlow(U_i0=0.6, width=1.0, L_factor=10.0), "sausage", None, (2.7, 4.95))
    c["LG_dens_kink"] = (q.CylinderDensity(width=1.5, c_e=1.5, vA_e=0.5, r_sign=1.0, ic=(1e-8, 1e-8), L_factor=10.0),
                         "kink", None, (0.52, 1.48))
    c["LG_dens_sausage"] = (q.CylinderDensity(width=1.5, c_e=1.5, vA_e=0.5, r_sign=1.0, ic=(1e-8, 1e-8), L_factor=10.0),
                            "sausage", None, (0.52, 1.48))
    return c


STANDARD = tuple(cases.all_cases()) + ("CF_flow_m5",)
LARGE_GAP = ("LG_flow_kink", "LG_flow_sausage", "LG_dens_kink", "LG_dens_sausage")
LARGE_GAP_TARGETS = (30.0, 39.0, 41.0, 50.0)        # the windows reach about 50


def is_cyl(eq):
    return isinstance(eq, q._CylinderBase)


@functools.lru_cache(maxsize=None)
def problem(name):
    eq, mode, m, _ = all_cases()[name]
    return cases.truth_problem(eq.plain() if isinstance(eq, FlowWithAxisTarget) else eq, mode, m)


def exterior_m_e(prob, k, w):
    return float(prob.exterior(k, w)[0])


def away_from_cutoffs(eq, k, w):
    we2 = (w - k * eq.U_e) ** 2
    return all(abs(k * k * c * c - we2) >= 1e-3 * we2 for c in (eq.c_e, eq.vA_e, eq.cT_e))


def cpu_ok(name, k, w):
    """ES_PT_OK as the oracle sees it: a bound exterior and no continuum inside."""
    prob = problem(name)
    eq = all_cases()[name][0]
    m_e = exterior_m_e(prob, k, w)
    return bool(np.isfinite(m_e) and m_e > 0.0 and away_from_cutoffs(eq, k, w) and not prob.continuum(k, w))


@functools.lru_cache(maxsize=None)
def pairs(name, n=N_PAIRS):
    """(k[n], w[n]): a different k per pair, omega = k W with W inside the window."""
    _, _, _, (lo, hi) = all_cases()[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ks, ws = [], []
    for _ in range(400):
        k = rng.uniform(0.8, 3.6)                       # the k range of the root searches in tests/test_eigenfunction_gpu.py
        w = k * rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
        if cpu_ok(name, k, w):
            ks.append(k)
            ws.append(w)
        if len(ks) == n:
            break
    assert len(ks) == n, name
    return np.array(ks), np.array(ws)


@functools.lru_cache(maxsize=None)
def large_gap_pairs(name):
    """One pair per target gap mu (R - 1) in LARGE_GAP_TARGETS: k fixed per target, W bisected inside the window."""
    prob = problem(name)
    _, _, _, (lo, hi) = all_cases()[name]
    ks, ws = [], []
    for t, k in zip(LARGE_GAP_TARGETS, (1.1, 1.4, 1.7, 2.3)):
        def gap(W):
            m_e = exterior_m_e(prob, k, k * W)
            return np.sqrt(m_e) * (prob.L_factor * 2.0 * np.pi / k - 1.0) if m_e > 0 else -1.0
        Wg = np.linspace(lo, hi, 400)
        g = np.array([gap(W) for W in Wg])
        ok = np.array([cpu_ok(name, k, k * W) for W in Wg])
        i = int(np.argmin(np.where(ok, np.abs(g - t), np.inf)))
        assert ok[i], (name, t)
        ks.append(k)
        ws.append(k * Wg[i])
    return np.array(ks), np.array(ws)


def truth_one(name, k, w, n_ext=500):
    """The DOP853 truth in the kernel's array names: x_int, value_int, flux_int, x_ext, value_ext, flux_ext and the two
    exterior terms value_ext_terms / flux_ext_terms (each a pair of arrays)."""
    eq = all_cases()[name][0]
    prob = problem(name)
    if is_cyl(eq):
        o = oc.eigenfunction_outward(prob, k, w, eq.n_nodes, n_ext=n_ext)
        return dict(x_int=o["r_int"], value_int=o["P_int"], flux_int=o["xi_int"], x_ext=o["r_ext"], value_ext=o["P_ext"],
                    flux_ext=o["xi_ext"], value_ext_terms=(o["P_ext_K"], o["P_ext_I"]),
                    flux_ext_terms=(o["xi_ext_K"], o["xi_ext_I"]), gap=o["gap"])
    o = osl.eigenfunction(prob, k, w, eq.n_nodes, n_ext=n_ext)
    return dict(x_int=o["x_int"], value_int=o["Vx_int"], flux_int=o["PT_int"], x_ext=o["x_ext"], value_ext=o["Vx_ext"],
                flux_ext=o["PT_ext"], value_ext_terms=(o["Vx_ext_dec"], o["Vx_ext_grow"]),
                flux_ext_terms=(o["PT_ext_dec"], o["PT_ext_grow"]), gap=o["gap"])


@functools.lru_cache(maxsize=None)
def truth(name, i, large_gap=False):
    """Truth of pair i of a case, computed once per session; callers must not modify the arrays."""
    k, w = (large_gap_pairs if large_gap else pairs)(name)
    return truth_one(name, float(k[i]), float(w[i]))


# ---- the kernel's state variables -------------------------------------------------------------------------------------
def flux_factor(name, k, w, x):
    """flux = state[1] * flux_factor at the nodes x: 1/r (xi_r = Xi / r), 1/omega (density slab), F/Omega (flow slabs)."""
    eq = all_cases()[name][0]
    x = np.asarray(x, dtype=float)
    if is_cyl(eq):
        return 1.0 / x
    if isinstance(eq, q.SlabDensity):
        return np.full_like(x, 1.0 / w)
    _, _, _, _, _, Om, _, F = problem(name)._coef(x, k, w)
    return F / Om


def write_nodes(name):
    """The nodes in the order the kernel's writing march visits them, and their indices in the output rows."""
    eq = all_cases()[name][0]
    x = np.linspace(eq.x_boundary, eq.x_end, eq.n_nodes)
    idx = np.arange(eq.n_nodes)
    return (x[::-1], idx[::-1]) if is_cyl(eq) else (x, idx)


def _matrix(prob, x, k, w):
    o = prob._rhs(float(x), np.array([1.0, 0.0, 0.0, 1.0]), k, w)
    return np.array([[o[0], o[2]], [o[1], o[3]]])


@functools.lru_cache(maxsize=32)
def _matrices(prob, k, w, x0, x1, n):
    """A at the n nodes and n - 1 mid-points of linspace(x0, x1, n), [2n - 1, 2, 2]; kept for the marches that share a grid."""
    return np.array([_matrix(prob, x, k, w) for x in np.linspace(x0, x1, 2 * n - 1)])


def grid_rk4(prob, k, w, y_start, x_nodes):
    """RK4 of y' = A(x) y (A from prob._rhs) from y_start at x_nodes[0] over the uniform grid x_nodes, one step per interval
    with A at node, mid-point, node.  y_start is one state [2] or several columns [2, c]; returns y[2, len(x_nodes)(, c)] in
    the dtype of y_start."""
    y = np.array(y_start)
    dt = y.dtype
    n = len(x_nodes)
    h = dt.type(np.linspace(x_nodes[0], x_nodes[-1], 2 * n - 1)[2] - x_nodes[0])
    A = _matrices(prob, float(k), float(w), float(x_nodes[0]), float(x_nodes[-1]), n).astype(dt)
    out = np.empty((2, n) + y.shape[1:], dtype=dt)
    out[:, 0] = y
    half, six, three = dt.type(0.5) * h, h / dt.type(6.0), h / dt.type(3.0)
    for j in range(n - 1):
        A0, Am, A1 = A[2 * j], A[2 * j + 1], A[2 * j + 2]
        k1 = A0 @ y
        k2 = Am @ (y + half * k1)
        k3 = Am @ (y + half * k2)
        k4 = A1 @ (y + h * k3)
        y = y + six * (k1 + k4) + three * (k2 + k3)
        out[:, j + 1] = y
    return out


def model(name, k, w, dtype=np.float64):
    """The kernel's interior algorithm on grid_rk4, (value, flux) rows in output order.
    Cylinders: the columns e = (1, 0) and d from the axis point to the boundary, d = (0, 1) for the kink conditions
    (P(r_ax) = target) and (a12, -a11) for the sausage condition (P'(r_ax) = a11 P + a12 Xi = 0, target = 0); the axis state
    target e + beta d with beta from P(r_b) = P_b; then that state marched out again.
    Slabs: the columns (1, 0), (0, 1) from x = -1 to +1 give the row (T11, T12); v(-1) = (sigma - T11) V_b / T12; then
    (V_b, v(-1)) marched across."""
    eq, mode, _, _ = all_cases()[name]
    prob = problem(name)
    x, idx = write_nodes(name)
    one, zero = dtype(1.0), dtype(0.0)
    if is_cyl(eq):
        _, xi_c, Pb, dPb = prob.exterior(k, w)
        xi_e = xi_c * dPb
        if prob.axis_bc == "sausage":
            A = _matrix(prob, x[0], k, w)
            target, d = 0.0, (A[0, 1], -A[0, 0])
        else:
            sign = 1.0 if prob.axis_bc == "kink" else -1.0
            target, d = sign * eq.bc_const(0) * xi_e, (0.0, 1.0)
        cols = grid_rk4(prob, k, w, np.array([[one, dtype(d[0])], [zero, dtype(d[1])]], dtype=dtype), x)
        beta = (dtype(Pb) - dtype(target) * cols[0, -1, 0]) / cols[0, -1, 1]
        y0 = np.array([dtype(target) + beta * dtype(d[0]), beta * dtype(d[1])], dtype=dtype)
    else:
        _, _, Vb_e, _ = prob.exterior(k, w)
        Om_b = prob._coef(np.array([-1.0]), k, w)[5][0]
        Vb = Vb_e if isinstance(eq, q.SlabDensity) else Vb_e * Om_b / (w - k * eq.U_e)
        cols = grid_rk4(prob, k, w, np.array([[one, zero], [zero, one]], dtype=dtype), x)
        sigma = -1.0 if mode == "sausage" else 1.0
        y0 = np.array([dtype(Vb), (dtype(sigma) - cols[0, -1, 0]) * dtype(Vb) / cols[0, -1, 1]], dtype=dtype)
    y = grid_rk4(prob, k, w, y0, x)
    ff = flux_factor(name, k, w, x).astype(dtype)
    value, flux = np.empty(len(x), dtype=dtype), np.empty(len(x), dtype=dtype)
    value[idx], flux[idx] = y[0], y[1] * ff
    return value, flux


def restate(name, k, w, value_row, flux_row, dtype=np.float64):
    """grid_rk4 started from the state the output rows hold at the first node of the kernel's writing march, in the
    kernel's direction; returned as (value, flux) rows in output order."""
    x, idx = write_nodes(name)
    ff = flux_factor(name, k, w, x)
    y0 = np.array([value_row[idx[0]], flux_row[idx[0]] / ff[0]], dtype=dtype)
    y = grid_rk4(problem(name), k, w, y0, x)
    value, flux = np.empty(len(x), dtype=dtype), np.empty(len(x), dtype=dtype)
    value[idx], flux[idx] = y[0], y[1] * ff.astype(dtype)
    return value, flux


def boundary_flux_spread(name, k, w):
    """Cylinders: |flux_int at the boundary by the outward model - the same by the inward march the determinant takes|, both
    in NumPy on the node grid.  Two RK4 marches of one order over the same grid differ by a constant times the same h^4 term;
    4 times this figure bounds what es_shoot_eval_points' D may differ by from the jump of the kernel's flux arrays."""
    eq = all_cases()[name][0]
    prob = problem(name)
    x = np.linspace(eq.x_boundary, eq.x_end, eq.n_nodes)
    cols = grid_rk4(prob, k, w, np.array([[1.0, 0.0], [0.0, 1.0]]), x)
    _, xi_c, Pb, dPb = prob.exterior(k, w)
    xi_e = xi_c * dPb
    if prob.axis_bc == "sausage":
        A = _matrix(prob, x[-1], k, w)
        r1, r2 = A[0, 0] * cols[0, -1, 0] + A[0, 1] * cols[1, -1, 0], A[0, 0] * cols[0, -1, 1] + A[0, 1] * cols[1, -1, 1]
        Xb = -(r1 * Pb) / r2
    else:
        sign = 1.0 if prob.axis_bc == "kink" else -1.0
        Xb = (sign * eq.bc_const(0) * xi_e - cols[0, -1, 0] * Pb) / cols[0, -1, 1]
    _, flux = model(name, k, w)
    return abs(flux[0] - Xb / x[0])

"""NumPy restatement of include/eigensolver_amd.h section 19 (es_cylt_complex_eigenfunction;
eigensolver_amd/csrc/es_cyl_complex_eigen.hip at FAM_CYLT) and of what sections 16's amplitude and synthesis calls make of its
arrays: test infrastructure on top of tests/cylt_complex_model.py, in the manner of tests/cyl_complex_eigen_model.py.

  * interior: CyltComplexModel.coef on the 2N - 1 samples and the full-shape outward step (rk4_step_forward<true>:
    ku = a11 u + a12 v, kv = a22 v + a21 u, a11 = -a22; S_j takes node j + 1 to node j), the discrete problem
    y_j = S_j y_{j+1}, axis condition at node N - 1, P = 1 at node 0, solved in the kernel's three passes: g from d at the axis
    outwards, s from (0, 1) at the boundary inwards by the exact inverse of the same step, y = a s + b g with b = 1 / P(g_0) and
    a = target / P(s_{N-1}); xi_r = Xi / r.  Axis condition: kink target = bc_const xi_e, rotation kink target =
    -(bc_const xi_e), both with d = (0, 1); sausage y_{N-1} along d = (a12, -a11), a = 0.  In exact arithmetic this is the
    solution section 16's march of the axis state target e + beta d gives; in fp64 that march loses up to ten digits to the
    cancellation at the boundary where the target is not zero;
  * exterior: CylComplexEigenModel.exterior_points as it is (the medium outside is the same);
  * status: CyltComplexModel.eval's, plus the non-finite check on the boundary state; rows that are not OK are NaN;
  * amplitudes: tests/field_model.polarisation on complex arrays with the twisted profiles of shooting.field_profiles
    (CylComplexEigenModel.polarisation as it is); synthesis: tests/cyl_complex_eigen_model.synthesis.
Beside it the independent leg: oracle.cylinder.CylinderProblem._rhs integrated by DOP853 on complex y for the two columns from
the axis point outwards, beta solved the same way, dense output at the nodes.

The jump of the flux and D_c.  The determinant's adjoint row march is J (outward march) J^-1 for the trace-free coefficient
matrix.  With S the discrete outward transfer matrix (columns (p1, x1) and (p2, x2) from (1, 0) and (0, 1)) the two values of
Xi(boundary) differ by (det S - 1) target / p2: nothing where the target is zero (sausage, bc_const = 0), the order of the
RK4 truncation otherwise, since RK4 keeps det S at 1 to truncation only.  `boundary_flux_spread` measures it.
NumPy has no fused multiply-add and divides complex numbers by Smith's rule: agreement with the kernels is to rounding."""
import numpy as np
from scipy.integrate import solve_ivp

from tests.cyl_complex_eigen_model import CylComplexEigenModel, NAN, synthesis, synthesis_bound  # noqa: F401
from tests.cyl_complex_model import ST_OK
from tests.cylt_complex_model import AXIS_KINK, AXIS_ROTATION_KINK, AXIS_SAUSAGE, JET, JET_ROOT, model_for  # noqa: F401

ST_NONFINITE = 2


def _forward_step(u, v, A0, Am, A1, h):
    """rk4_step_forward<true>: y' = A y with A = [[-a22, a12], [a21, a22]]; A = (a22, a12, a21) as CyltComplexModel.coef."""
    h2, h6, h3 = 0.5 * h, h / 6.0, h / 3.0

    def rhs(A, uu, vv):
        d, b, a = A
        return (-d) * uu + b * vv, d * vv + a * uu

    k1u, k1v = rhs(A0, u, v)
    k2u, k2v = rhs(Am, h2 * k1u + u, h2 * k1v + v)
    k3u, k3v = rhs(Am, h2 * k2u + u, h2 * k2v + v)
    k4u, k4v = rhs(A1, h * k3u + u, h * k3v + v)
    return h6 * (k1u + k4u) + (h3 * (k2u + k3u) + u), h6 * (k1v + k4v) + (h3 * (k2v + k3v) + v)


class CyltComplexEigenModel(CylComplexEigenModel):
    def __init__(self, eq, mode, m=None, accept_norm=0):
        self.eq, self.mode = eq, mode
        self.M = model_for(eq, mode, m, accept_norm=accept_norm)
        d = self.M.d
        self.N, self.h = self.M.N, self.M.h
        self.x_int = d["x_boundary"] + np.arange(self.N) * self.h            # the kernel's node abscissae
        from eigensolver_amd import shooting
        self.r_nodes = np.asarray(shooting.make_desc(eq, mode, m)[1]["r"])[::2]      # the radii the profile arrays are formed at
        self.sgn = -1.0 if d["x_boundary"] < 0 else 1.0

    # ---- es_cylt_complex_eigenfunction ------------------------------------------------------------------------------------
    def axis_state(self, A_axis, xi_e):
        """target, d0, d1 of the axis state target e + beta d for the arrays xi_e; A_axis: coef of the axis node."""
        one, zero = np.ones_like(xi_e), np.zeros_like(xi_e)
        bc = self.M.d["axis_bc"]
        if bc == AXIS_KINK:
            return self.M.d["bc_const"] * xi_e, zero, one
        if bc == AXIS_ROTATION_KINK:
            return -(self.M.d["bc_const"] * xi_e), zero, one
        a22, a12, _ = A_axis
        return zero, a12, a22 + zero                                         # d = (a12, -a11), a11 = -a22

    def interior(self, k, w, xi_e):
        """value, flux [n, N] (node 0 = boundary) and the boundary flux of the interior solution, for arrays k, w, xi_e [n]: the
        kernel's three passes.  g from d at the axis outwards; s from (0, 1) at the boundary inwards by the exact inverse of the
        same outward step; y = a s + b g with b = 1 / P(g_0) and a = target / P(s_{N-1}) (kink conditions) or 0 (sausage)."""
        M, N, h = self.M, self.N, self.h
        A = [M.coef(j, k, w) for j in range(2 * N - 1)]
        one, zero = np.ones_like(w), np.zeros_like(w)
        target, d0, d1 = self.axis_state(A[2 * (N - 1)], xi_e)
        gp, gv = np.empty((N,) + w.shape, w.dtype), np.empty((N,) + w.shape, w.dtype)
        u, v = d0 + zero, d1 + zero
        gp[N - 1], gv[N - 1] = u, v
        for j in range(N - 2, -1, -1):
            u, v = _forward_step(u, v, A[2 * j + 2], A[2 * j + 1], A[2 * j], -h)
            gp[j], gv[j] = u, v
        b = 1.0 / gp[0]
        sp, sv = np.empty_like(gp), np.empty_like(gp)
        u, v = zero, one
        sp[0], sv[0] = u, v
        for j in range(N - 1):
            m11, m21 = _forward_step(one, zero, A[2 * j + 2], A[2 * j + 1], A[2 * j], -h)
            m12, m22 = _forward_step(zero, one, A[2 * j + 2], A[2 * j + 1], A[2 * j], -h)
            idet = 1.0 / (m11 * m22 - m12 * m21)
            u, v = (m22 * u - m12 * v) * idet, (m11 * v - m21 * u) * idet
            sp[j + 1], sv[j + 1] = u, v
        a = zero if M.d["axis_bc"] == AXIS_SAUSAGE else target / sp[N - 1]
        inner = (a + b * gv[0]) / M.d["x_boundary"]
        value = (a * sp + b * gp).T
        flux = ((a * sv + b * gv) / self.x_int.reshape((N,) + (1,) * w.ndim)).T
        return value, flux, inner

    def eigenfunction(self, k, w, n_ext=500):
        """The dict of RotatingCylinderComplex.eigenfunction as NumPy arrays, plus D, outer, inner (the model's D_c of section
        17 and its two sides, by the adjoint march) and inner_outward (the boundary flux of this solution, flux_int[:, 0])."""
        w = np.asarray(w, dtype=complex).reshape(-1)
        k = np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy()
        with np.errstate(all="ignore"):
            D, outer, inner, _, st = self.M.eval_points(k, w)
            _, xi_e = self.M.exterior(k, w)
            vi, fi, inner_out = self.interior(k, w, xi_e)
            xe, ve, fe = self.exterior_points(k, w, n_ext)
            st = np.where((st == ST_OK) & ~(np.isfinite(inner_out) & np.isfinite(xi_e - inner_out)), ST_NONFINITE, st)
        st = st.astype(np.uint8)
        bad = st != ST_OK
        for a in (vi, fi, ve, fe):
            a[bad] = NAN
        return dict(x_int=self.x_int, value_int=vi, flux_int=fi, x_ext=xe, value_ext=ve, flux_ext=fe, status=st, D=D,
                    outer=outer, inner=inner, inner_outward=np.where(bad, NAN, inner_out))

    # ---- the independent leg ------------------------------------------------------------------------------------------------
    def interior_dop853(self, prob, k, w, rtol=1e-12):
        """value, flux [N] of one OK pair with the interior by DOP853 on complex y (prob: oracle.cylinder.CylinderProblem of
        the same equilibrium), the two columns from the axis point outwards, beta from P(r_b) = 1, this model's exterior."""
        k, w = float(k), complex(w)
        st, xi_e = self.M.exterior(k, np.array([w]))
        assert st[0] == ST_OK
        rb, ra = prob.r_sign * 1.0, prob.r_sign * prob.r_axis
        r_int = np.linspace(rb, ra, self.N)
        bc = self.M.d["axis_bc"]
        if bc == AXIS_KINK:
            target, d = self.M.d["bc_const"] * xi_e[0], (0.0, 1.0)
        elif bc == AXIS_ROTATION_KINK:
            target, d = -(self.M.d["bc_const"] * xi_e[0]), (0.0, 1.0)
        else:
            Dc, C1, _, C3, _, _ = prob.coefficients(np.array([ra]), k, w)
            target, d = 0.0, (C3[0] / (ra * Dc[0]), C1[0] / Dc[0])            # (a12, -a11)
        y0 = np.array([1.0, 0.0, d[0], d[1]], dtype=complex)
        sol = solve_ivp(prob._rhs, (ra, rb), y0, method="DOP853", rtol=rtol, atol=1e-300, t_eval=r_int[::-1], args=(k, w))
        y = sol.y[:, ::-1]                                                    # boundary first
        beta = (1.0 - target * y[0, 0]) / y[2, 0]
        return target * y[0] + beta * y[2], (target * y[1] + beta * y[3]) / r_int


# ---- the problems of the section-19 tests: those of tests/test_cylt_complex_gpu.py, restated, and the zero-twist jet ----------
NAMES = ("A", "B", "C", "sausage", "reference")
ZERO_TWIST = "zero_twist"
ALL_NAMES = NAMES + (ZERO_TWIST,)
NODE_COUNTS = (129, 130, 300)                                         # one LDS chunk of 128 steps exactly, one more, three chunks
ROOT_A = (1.0, 1.5554994 + 0.7920935j)                                # k, omega of the unstable m = 3 root of case A at N = 130


def twisted_jet(**kw):
    from eigensolver_amd import equilibrium as q

    class TwistedJet(q.CylinderFlow):
        twisted = True

    return TwistedJet(**kw)


def problems(n_nodes):
    """name -> (equilibrium, mode, m, accept_norm, (W_lo, W_hi), (g_lo, g_hi)): phase-speed window of Re omega / k and the
    window of |Im omega| / k of the sample."""
    from eigensolver_amd import equilibrium as q
    rot = lambda v, p, **kw: q.CylinderRotation(v_twist=v, power=p, n_nodes=n_nodes, **kw)             # noqa: E731
    return {
        "A": (rot(2.0, 1.0, r_axis=1e-2), "kink", 3, 0, (1.2, 1.9), (0.45, 1.15)),
        "B": (rot(2.0, 0.8, r_axis=1e-2, c1_power=1), "kink", 1, 1, (1.2, 1.7), (0.05, 0.35)),
        "C": (rot(1.0, 1.0, r_axis=1e-2), "kink", 4, 0, (0.9, 1.4), (0.15, 1.2)),
        "sausage": (rot(0.15, 1.25, r_axis=1e-2, c1_power=1), "sausage", 0, 0, (0.6, 1.45), (0.02, 0.3)),
        "reference": (rot(0.25, 0.8), "kink", None, 1, (0.6, 1.45), (0.02, 0.3)),
        ZERO_TWIST: (twisted_jet(**JET, n_nodes=n_nodes), "kink", None, 0, (0.9, 1.45), (0.05, 0.4)),
    }


def sample(W, g, n, seed):
    """n points, a different k in every lane: Re omega = k W, Im omega = +- k g, both signs."""
    rng = np.random.default_rng(seed)
    k = np.linspace(0.5, 2.0, n) if n > 1 else np.array([1.0])
    k = rng.permutation(k)
    w = k * rng.uniform(W[0], W[1], n) + 1j * k * rng.uniform(g[0], g[1], n) * rng.choice([-1.0, 1.0], n)
    return k, w


def seed_of(n_nodes):
    return 100 + n_nodes


def model_of(name, n_nodes):
    eq, mode, m, an, _, _ = problems(n_nodes)[name]
    return CyltComplexEigenModel(eq, mode, m, accept_norm=an)


def pairs(name, n_nodes, n=65):
    """The sample of a problem: (k, w), n pairs."""
    _, _, _, _, W, g = problems(n_nodes)[name]
    return sample(W, g, n, seed_of(n_nodes))


def boundary_flux_spread(name, k, w, n_nodes=130):
    """|inner of the outward step's discrete solution - inner by the adjoint row march the determinant takes| for k, w on the grid
    of n_nodes nodes, both in NumPy (NaN where the pair is not OK): the model's own measure of how far the jump of the flux may
    be from D_c, in the sense of tests/real_eigen_model.boundary_flux_spread -- two RK4 marches of one order over the same grid
    differ by a constant times the same h^4 term, and 4 times this figure bounds what the kernels' two marches may differ by."""
    e = model_of(name, n_nodes).eigenfunction(k, w, n_ext=0)
    return np.abs(e["inner_outward"] - e["inner"])


def dop_pairs(name, n_nodes):
    """Two OK pairs of a problem for the DOP853 comparison: the first two of its sample the model calls OK."""
    k, w = pairs(name, n_nodes, 16)
    st = model_of(name, n_nodes).M.eval_points(k, w)[4]
    ok = np.flatnonzero(st == ST_OK)[:2]
    assert len(ok) == 2, name
    return k[ok], w[ok]

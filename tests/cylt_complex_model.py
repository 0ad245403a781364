"""NumPy restatement of the complex-frequency determinant of the twisted (rotating) cylinder (include/eigensolver_amd.h section
17, eigensolver_amd/csrc/es_cyl_complex.hip at FAM_CYLT): test infrastructure, in the manner of tests/cyl_complex_model.py.

Step for step what the kernel does, in plain complex128:
  * the 20 base fields es_problem_create forms from the 2N - 1 profile samples, the node entries and coefficients of the
    FAM_CYLT text (make_entry, coef_pre, coef_finish of es_shoot_device.hpp), one division per node;
  * the adjoint RK4 row march from the axis end back to the boundary with the full-shape step (rk4_step_adjoint<1>,
    a11 = -a22), start vector by the axis condition;
  * the exterior of tests/cyl_complex_model.CylComplexModel as it is (the medium outside is the same), and its evaluation
    drivers, secant iteration and root search;
  * boundary algebra with P_b = 1 for the three axis conditions; the statuses of section 14.
Beside it the independent leg: the interior by DOP853 on complex y through oracle.cylinder.CylinderProblem._rhs.
Unlike the untwisted model, `eval` takes an array of wavenumbers too (one per point): the GPU tests give every lane its own k.
NumPy has no fused multiply-add and divides complex numbers by Smith's rule: agreement with the kernel is to rounding.
"""
import numpy as np
from scipy.integrate import solve_ivp

from tests.cyl_complex_model import CylComplexModel, ST_OK

AXIS_KINK, AXIS_SAUSAGE, AXIS_ROTATION_KINK = 0, 1, 2
GEOM_CYLINDER_TWIST = 1


class CyltComplexModel(CylComplexModel):
    """desc: dict of the es_shoot_desc fields; prof: the 2N - 1 profile samples (shooting.make_desc)."""

    def __init__(self, desc, prof):
        assert desc["geometry"] == GEOM_CYLINDER_TWIST, "twisted cylinder only"
        assert desc["axis_bc"] in (AXIS_KINK, AXIS_SAUSAGE, AXIS_ROTATION_KINK)
        assert desc["c1_power"] in (1, 2)
        self.d = dict(desc)
        r, rho, c2, Bz = (np.asarray(prof[n], dtype=np.float64) for n in ("r", "rho", "c2", "Bz"))
        zero = np.zeros_like(r)
        Bphi, vz, vphi, rdC3 = (np.asarray(prof.get(n, zero), dtype=np.float64) for n in ("Bphi", "vz", "vphi", "rdC3"))
        # es_problem_create, ES_GEOM_CYLINDER_TWIST
        sr = np.sqrt(rho)
        bA = Bz / sr
        vA = (Bz + Bphi) / sr
        S = c2 + vA * vA
        dm = float(desc["m"])
        invr = 1.0 / r
        invr2 = invr * invr
        bphr, vphr = Bphi / r, vphi / r
        Bphi_n, vphi_n = bphr * r, vphr * r
        self.MB, self.BZ, self.BA, self.MV, self.VZ, self.Q = dm * bphr, Bz, bA, dm * vphr, vz, c2 / S
        self.E3, self.RHO = rho * S, rho
        self.E5, self.E6 = rho * vphi_n * vphi_n * invr, 2.0 * Bphi_n * Bphi_n * invr
        self.C7, self.INVR, self.BPHI, self.E9 = 2.0 * Bphi_n * vphi_n, invr, Bphi_n, rho * vphi_n
        self.E10, self.S, self.M2R2 = 2.0 * dm * S * invr2, S, dm * dm * invr2
        self.RDC3, self.E13, self.R = rdC3, 4.0 * S * invr2, r
        self.N = int(desc["n_nodes"])
        self.h = (desc["x_end"] - desc["x_boundary"]) / (self.N - 1)

    # ---- interior ---------------------------------------------------------------------------------------------------
    def coef(self, j, k, w):
        """a22 (= -a11), a12, a21 of sample j for the arrays k (real) and w (complex)."""
        kb = k * self.BZ[j] + self.MB[j]
        wA = k * self.BA[j] + self.MB[j]
        e1 = wA * wA
        e2 = e1 * self.Q[j]
        e7 = self.C7[j] * kb * self.INVR[j]
        e8 = kb * self.BPHI[j]
        e11 = self.S[j] * (self.M2R2[j] + k * k)
        Om = w - (k * self.VZ[j] + self.MV[j])
        Om2 = Om * Om
        t1, t2 = Om2 - e1, Om2 - e2
        D = self.E3[j] * t1 * t2
        Q = Om * e7 + (Om2 * self.E6[j] + -(t1 * self.E5[j]))
        T = self.E9[j] * Om + e8
        OmP = Om2 if self.d["c1_power"] == 2 else Om
        t2T = t2 * T
        C1 = Q * OmP + -(self.E10[j] * t2T)
        C2 = Om2 * Om2 + -(e11 * t2)
        C3 = D * (self.RHO[j] * t1 + self.RDC3[j]) + (Q * Q + -((self.E13[j] * t2T) * T))
        inv = 1.0 / D
        return C1 * inv, (C3 * self.INVR[j]) * inv, (-(self.R[j] * C2)) * inv

    def row(self, k, w):
        """The row (p, q) of the interior transfer matrix the axis condition picks, marched back to the boundary."""
        N, h = self.N, self.h
        h2, h6, h3 = 0.5 * h, h / 6.0, h / 3.0
        d0, b0, a0 = self.coef(2 * (N - 1), k, w)              # a22, a12, a21
        if self.d["axis_bc"] == AXIS_SAUSAGE:
            p, q = -d0, b0.copy()                             # P'(r_ax) = a11 P + a12 Xi = 0
        else:
            p, q = np.ones_like(w), np.zeros_like(w)          # P(r_ax) = target

        def rhs(d, b, a, pp, qq):                             # A^T z with a11 = -a22
            return -d * pp + a * qq, d * qq + b * pp

        for j in range(N - 2, -1, -1):
            dm, bm, am = self.coef(2 * j + 1, k, w)
            d1, b1, a1 = self.coef(2 * j, k, w)
            k1p, k1q = rhs(d0, b0, a0, p, q)
            k2p, k2q = rhs(dm, bm, am, h2 * k1p + p, h2 * k1q + q)
            k3p, k3q = rhs(dm, bm, am, h2 * k2p + p, h2 * k2q + q)
            k4p, k4q = rhs(d1, b1, a1, h * k3p + p, h * k3q + q)
            p = h6 * (k1p + k4p) + (h3 * (k2p + k3p) + p)
            q = h6 * (k1q + k4q) + (h3 * (k2q + k3q) + q)
            d0, b0, a0 = d1, b1, a1
        return p, q

    # ---- the determinant --------------------------------------------------------------------------------------------
    def _axis(self, xi_e, p, q):
        """Xi(boundary) by the axis condition, P_b = 1."""
        bc = self.d["axis_bc"]
        if bc == AXIS_KINK:
            return (self.d["bc_const"] * xi_e - p * 1.0) / q
        if bc == AXIS_ROTATION_KINK:
            return (-(self.d["bc_const"] * xi_e) - p * 1.0) / q
        return -(p * 1.0) / q

    def _finish(self, st, xi_e, p, q):
        d = self.d
        xi_i = self._axis(xi_e, p, q) / d["x_boundary"]
        D = xi_e - xi_i
        sc = np.abs(xi_e) if d.get("accept_norm", 0) else np.maximum(np.abs(xi_e), np.abs(xi_i))
        rel = np.abs(D) * 100.0 / sc
        st = np.where((st == ST_OK) & ~(np.isfinite(D) & np.isfinite(xi_i)), 2, st).astype(np.uint8)
        bad = st != ST_OK
        nan = np.nan + 1j * np.nan
        return (np.where(bad, nan, D), np.where(bad, nan, xi_e), np.where(bad, nan, xi_i), np.where(bad, np.nan, rel), st)

    def eval(self, k, w):
        """D_c, outer, inner, rel, status for the complex array w; k: one wavenumber or one per point."""
        w = np.atleast_1d(np.asarray(w, dtype=complex))
        k = np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy()
        with np.errstate(all="ignore"):
            st, xi_e = self.exterior(k, w)
            p, q = self.row(k, w)
            return self._finish(st, xi_e, p, q)

    def eval_points(self, k, w):
        return self.eval(k, np.asarray(w, dtype=complex).reshape(-1))

    # ---- the independent leg: interior by DOP853 on complex y -----------------------------------------------------------
    def eval_dop853(self, prob, k, w, rtol=1e-12):
        """D_c, outer, inner at one (k, w) with the interior transfer matrix integrated by DOP853 (complex y) from the
        boundary to the axis end on the oracle's continuous profiles (prob: oracle.cylinder.CylinderProblem of the same
        equilibrium, through its _rhs), the axis condition as oracle.cylinder.CylinderProblem.mismatch imposes it -- the
        rotation_kink sign included --, this model's exterior."""
        w = complex(w)
        st, xi_e = self.exterior(float(k), np.array([w]))
        assert st[0] == ST_OK
        xi_e = xi_e[0]
        rb, ra = prob.r_sign * 1.0, prob.r_sign * prob.r_axis
        y0 = np.array([1.0, 0.0, 0.0, 1.0], dtype=complex)
        sol = solve_ivp(prob._rhs, (rb, ra), y0, method="DOP853", rtol=rtol, atol=1e-300, args=(float(k), w))
        y = sol.y[:, -1]
        T = np.array([[y[0], y[2]], [y[1], y[3]]])
        if self.d["axis_bc"] == AXIS_SAUSAGE:
            Dc, C1, C2, C3, _, _ = prob.coefficients(np.array([ra]), float(k), w)
            al, be = C3[0] / (ra * Dc[0]), -C1[0] / Dc[0]
            Xb = -(al * T[1, 0] + be * T[0, 0]) / (al * T[1, 1] + be * T[0, 1])
        else:
            Xb = self._axis(xi_e, T[0, 0], T[0, 1])
        xi_i = Xb / rb
        return xi_e - xi_i, xi_e, xi_i


# The zero-twist limit: equilibrium.CylinderFlow with these parameters, posed as a twisted problem by a subclass with
# twisted = True (v_phi = B_phi = 0 through the twisted coefficient set, ES_AXIS_ROTATION_KINK with bc_const = 0).
JET = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0, width=1e5, r_sign=1.0, r_axis=1e-3)   # README / DESIGN 8i
JET_ROOT = 2.372765 + 0.584713j                                                                   # kink, m = 1, k = 2


def root_cases(n_nodes=130):
    """name -> (equilibrium, m, k rows, w_re, w_im, quoted root or None): the small (Re, Im) windows around the unstable kink
    roots the CPU and GPU tests search, W_ABSOLUTE.  Cell edges are kept away from the roots."""
    from eigensolver_amd import equilibrium as q
    rot = lambda v, p: q.CylinderRotation(v_twist=v, power=p, r_axis=1e-2, n_nodes=n_nodes)             # noqa: E731
    return {
        "A": (rot(2.0, 1.0), 3, [1.0], np.linspace(1.2, 1.9, 8), np.linspace(0.45, 1.15, 8), 1.5554994 + 0.7920935j),
        "B": (rot(2.0, 0.8), 1, [1.0], np.linspace(1.2, 1.7, 6), np.linspace(0.05, 0.35, 7), 1.445346 + 0.138322j),
        "C": (rot(1.0, 1.0), 4, [0.5, 0.75, 1.0], np.linspace(0.85, 1.45, 7), np.linspace(0.15, 1.25, 12), None),
    }


def model_for(eq, mode, m=None, accept_norm=0):
    """The model of the product equilibrium `eq` (eigensolver_amd.equilibrium, twisted), built from the descriptor and the
    profile samples the product itself uploads."""
    from eigensolver_amd import shooting as s
    from tests.cases import desc_dict
    d, prof = s.make_desc(eq, mode, m)
    d.accept_norm = int(accept_norm)
    return CyltComplexModel(desc_dict(d), {a: np.asarray(v) for a, v in prof.items()})

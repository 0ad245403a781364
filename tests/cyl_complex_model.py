"""NumPy restatement of the complex-frequency determinant of the untwisted cylinder (include/eigensolver_amd.h section 14,
eigensolver_amd/csrc/es_cyl_complex.hip): test infrastructure.

Step for step what the kernel does, in plain complex128 with scipy's Bessel functions:
  * node entries and coefficients of the FAM_CYL0 text (make_entry, coef_pre, coef_finish of es_shoot_device.hpp) on the same
    2N - 1 profile samples, one division per node;
  * the adjoint RK4 row march from the axis end back to the boundary (rk4_step_adjoint<0>), start vector by the axis condition;
  * exterior: m_e, xi_e_const, mu = principal sqrt, P_e = a I_m + b K_m with the reference's far-field initial values
    (scipy.special.kve / ive at complex argument; ive scales by e^-|Re z|, hence the factor e^{-i Im z}), normalised by its own
    complex boundary value;
  * boundary algebra with P_b = 1; status: LEAKY where Re m_e < 0, NONFINITE where m_e, the constant or the result is not
    finite; no continuum status.
Beside it: the same determinant with the interior integrated by DOP853 on complex y (eval_dop853: the independent leg), the
cell rule (tests/complex_winding_model.py) and a secant iteration run to convergence (find_roots).
NumPy has no fused multiply-add and divides complex numbers by Smith's rule: agreement with the kernel is to rounding.
"""
import numpy as np
from scipy import special
from scipy.integrate import solve_ivp

from tests.complex_winding_model import flagged_cells

ST_OK, ST_LEAKY, ST_NONFINITE = 0, 1, 2
AXIS_KINK, AXIS_SAUSAGE = 0, 1
W_ABSOLUTE, W_PHASE_SPEED = 0, 1


class CylComplexModel:
    """desc: dict of the es_shoot_desc fields; prof: the 2N - 1 profile samples (shooting.make_desc)."""

    def __init__(self, desc, prof):
        assert desc["geometry"] == 0, "untwisted cylinder only"
        assert desc["axis_bc"] in (AXIS_KINK, AXIS_SAUSAGE)
        self.d = dict(desc)
        r, rho, c2, Bz = (np.asarray(prof[n], dtype=np.float64) for n in ("r", "rho", "c2", "Bz"))
        vz = np.asarray(prof.get("vz", np.zeros_like(r)), dtype=np.float64)
        bA = Bz / np.sqrt(rho)
        S = c2 + bA * bA                              # es_problem_create: vA = (Bz + Bphi) / sqrt(rho) with Bphi = 0
        self.vz, self.bA, self.q = vz, bA, c2 / S
        self.A1, self.B1 = rho / r, r / (rho * S)
        self.E1, self.E2 = 1.0 / (r * rho), r / rho
        self.N = int(desc["n_nodes"])
        self.h = (desc["x_end"] - desc["x_boundary"]) / (self.N - 1)

    # ---- interior ---------------------------------------------------------------------------------------------------
    def coef(self, j, k, w):
        """a12, a21 of sample j for the complex array w."""
        m2, k2 = float(self.d["m"]) ** 2, k * k
        wA = k * self.bA[j]
        e1 = wA * wA
        e2 = e1 * self.q[j]
        Bq = self.B1[j]
        g = m2 * self.E1[j] + k2 * self.E2[j]
        e5 = g - Bq * (e1 + e2)
        e6 = -(Bq * (e2 * e2))
        Om = w - k * self.vz[j]
        t1 = Om * Om - e1
        t2 = Om * Om - e2
        a12 = self.A1[j] * t1
        a21 = (e5 * t2 + e6) * (1.0 / (t1 * t2)) + (-Bq)
        return a12, a21

    def row(self, k, w):
        """The row (p, q) of the interior transfer matrix the axis condition picks, marched back to the boundary."""
        N, h = self.N, self.h
        h2, h6, h3 = 0.5 * h, h / 6.0, h / 3.0
        b0, a0 = self.coef(2 * (N - 1), k, w)
        if self.d["axis_bc"] == AXIS_SAUSAGE:
            p, q = np.zeros_like(w), b0.copy()        # P'(r_ax) = a12 Xi = 0
        else:
            p, q = np.ones_like(w), np.zeros_like(w)  # P(r_ax) = target
        for j in range(N - 2, -1, -1):
            bm, am = self.coef(2 * j + 1, k, w)
            b1, a1 = self.coef(2 * j, k, w)
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

    # ---- exterior ---------------------------------------------------------------------------------------------------
    def exterior(self, k, w):
        """(status, xi_e) with P_e(boundary) = 1; xi_e is NaN unless the status is OK."""
        d = self.d
        k2, w2 = k * k, w * w
        vAe2, ce2, cTe2 = d["vA_e"] ** 2, d["c_e"] ** 2, d["cT_e"] ** 2
        m_e = ((k2 * vAe2 - w2) * (k2 * ce2 - w2)) / ((vAe2 + ce2) * (k2 * cTe2 - w2))
        cst = -1.0 / (d["rho_e"] * (k2 * vAe2 - w2))
        st = np.where(m_e.real < 0, ST_LEAKY, np.where(np.isfinite(m_e) & np.isfinite(cst), ST_OK, ST_NONFINITE))
        mu = np.sqrt(np.where(st == ST_OK, m_e, 1.0 + 0j))          # principal root
        sgn = -1.0 if d["x_boundary"] < 0 else 1.0
        n = float(d["m_ext"])
        xR, xb = mu * (d["L_factor"] * 2.0 * np.pi / k), mu

        def K(z):
            a, b = special.kve(n, z), special.kve(n + 1, z)
            return a, (n / z) * a - b                               # e^z K_n, e^z K_n'

        def I(z):
            ph = np.exp(-1j * z.imag)
            a, b = special.ive(n, z) * ph, special.ive(n + 1, z) * ph
            return a, b + (n / z) * a                               # e^-z I_n, e^-z I_n'

        Kb, dKb = K(xb)
        KR, dKR = K(xR)
        Ib, dIb = I(xb)
        IR, dIR = I(xR)
        g = d["ic_slope"] / (sgn * mu)
        a_s, b_s = -(d["ic_value"] * dKR - g * KR), -(g * IR - d["ic_value"] * dIR)
        gap = xR - xb
        E2 = np.exp(-2.0 * gap)
        near = gap.real < 40.0
        Pv = np.where(near, b_s * Kb + E2 * a_s * Ib, Kb)
        dPv = (sgn * mu) * np.where(near, b_s * dKb + E2 * a_s * dIb, dKb)
        outer = cst * (dPv / Pv)
        st = np.where((st == ST_OK) & ~np.isfinite(outer), ST_NONFINITE, st)
        return st.astype(np.uint8), np.where(st == ST_OK, outer, np.nan + 0j)

    # ---- the determinant --------------------------------------------------------------------------------------------
    def _finish(self, st, xi_e, p, q):
        d = self.d
        if d["axis_bc"] == AXIS_KINK:
            Xb = (d["bc_const"] * xi_e - p * 1.0) / q
        else:
            Xb = -(p * 1.0) / q
        xi_i = Xb / d["x_boundary"]
        D = xi_e - xi_i
        sc = np.abs(xi_e) if d.get("accept_norm", 0) else np.maximum(np.abs(xi_e), np.abs(xi_i))
        rel = np.abs(D) * 100.0 / sc
        st = np.where((st == ST_OK) & ~np.isfinite(D), ST_NONFINITE, st).astype(np.uint8)
        bad = st != ST_OK
        nan = np.nan + 1j * np.nan
        return (np.where(bad, nan, D), np.where(bad, nan, xi_e), np.where(bad, nan, xi_i), np.where(bad, np.nan, rel), st)

    def eval(self, k, w):
        """D_c, outer, inner, rel, status for one wavenumber and a complex array w."""
        w = np.atleast_1d(np.asarray(w, dtype=complex))
        with np.errstate(all="ignore"):
            st, xi_e = self.exterior(float(k), w)
            p, q = self.row(float(k), w)
            return self._finish(st, xi_e, p, q)

    def eval_points(self, k, w):
        w = np.asarray(w, dtype=complex).reshape(-1)
        k = np.broadcast_to(np.asarray(k, dtype=float), w.shape)
        D, o, i = (np.empty(w.shape, complex) for _ in range(3))
        rel, st = np.empty(w.shape), np.empty(w.shape, np.uint8)
        for kk in np.unique(k):
            s = k == kk
            D[s], o[s], i[s], rel[s], st[s] = self.eval(kk, w[s])
        return D, o, i, rel, st

    def eval_grid(self, k, w_re, w_im, w_mode=W_ABSOLUTE):
        """D_c[nk, n_im, n_re], rel, status."""
        k, w_re, w_im = (np.asarray(a, dtype=float).reshape(-1) for a in (k, w_re, w_im))
        shape = (len(k), len(w_im), len(w_re))
        D, rel, st = np.empty(shape, complex), np.empty(shape), np.empty(shape, np.uint8)
        for r, kk in enumerate(k):
            f = kk if w_mode == W_PHASE_SPEED else 1.0
            W = (f * w_re)[None, :] + 1j * (f * w_im)[:, None]
            d, _, _, rr, s = self.eval(kk, W.ravel())
            D[r], rel[r], st[r] = d.reshape(W.shape), rr.reshape(W.shape), s.reshape(W.shape)
        return D, rel, st

    # ---- the independent leg: interior by DOP853 on complex y -----------------------------------------------------------
    def eval_dop853(self, prob, k, w, rtol=1e-12):
        """D_c, outer, inner at one (k, w) with the interior transfer matrix integrated by DOP853 (complex y) from the
        boundary to the axis end on the oracle's continuous profiles (prob: oracle.cylinder.CylinderProblem of the same
        equilibrium), the axis condition as oracle.cylinder.CylinderProblem.mismatch imposes it, this model's exterior."""
        w = complex(w)
        st, xi_e = self.exterior(float(k), np.array([w]))
        assert st[0] == ST_OK
        xi_e = xi_e[0]
        rb, ra = prob.r_sign * 1.0, prob.r_sign * prob.r_axis
        y0 = np.array([1.0, 0.0, 0.0, 1.0], dtype=complex)
        sol = solve_ivp(prob._rhs, (rb, ra), y0, method="DOP853", rtol=rtol, atol=1e-300, args=(float(k), w))
        y = sol.y[:, -1]
        T = np.array([[y[0], y[2]], [y[1], y[3]]])
        if self.d["axis_bc"] == AXIS_KINK:
            Xb = (self.d["bc_const"] * xi_e - T[0, 0]) / T[0, 1]
        else:
            Dc, C1, C2, C3, _, _ = prob.coefficients(np.array([ra]), float(k), w)
            al, be = C3[0] / (ra * Dc[0]), -C1[0] / Dc[0]
            Xb = -(al * T[1, 0] + be * T[0, 0]) / (al * T[1, 1] + be * T[0, 1])
        xi_i = Xb / rb
        return xi_e - xi_i, xi_e, xi_i

    # ---- roots ------------------------------------------------------------------------------------------------------
    def secant(self, k, w0, w1, max_iter=60, tol=1e-15):
        """Complex secant iteration from (w0, w1) run to convergence: the root, or None."""
        f0, f1 = self.eval(k, w0)[0][0], self.eval(k, w1)[0][0]
        for _ in range(max_iter):
            if not (np.isfinite(f0) and np.isfinite(f1)) or f1 == f0:
                break
            w2 = w1 - f1 * (w1 - w0) / (f1 - f0)
            w0, f0, w1 = w1, f1, w2
            f1 = self.eval(k, w1)[0][0]
            if abs(w1 - w0) <= tol * abs(w1):
                return w1
        return w1 if np.isfinite(f1) and abs(w1 - w0) <= 1e-12 * abs(w1) else None

    def find_roots(self, k, w_re, w_im, w_mode=W_ABSOLUTE):
        """(cells, roots): the flagged cells (row, i_im, i_re) of the model's own grid, in order, and for each the converged
        root of a secant iteration started as the kernel starts it (cell centre, centre + a quarter of the diagonal), or
        None where it does not converge or leaves the neighbourhood of two cell diagonals."""
        k, w_re, w_im = (np.asarray(a, dtype=float).reshape(-1) for a in (k, w_re, w_im))
        D, _, st = self.eval_grid(k, w_re, w_im, w_mode)
        cells = flagged_cells(D, st)
        roots = []
        for (r, a, b) in cells:
            f = k[r] if w_mode == W_PHASE_SPEED else 1.0
            lo, hi = complex(f * w_re[b], f * w_im[a]), complex(f * w_re[b + 1], f * w_im[a + 1])
            centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
            w = self.secant(k[r], centre, centre + 0.5 * half)
            if w is not None and abs(w - centre) > 4.0 * abs(half):
                w = None
            roots.append(w)
        return cells, roots

    def d_omega(self, k, w, step=1e-6):
        """dD_c / d omega at (k, w) by a central difference."""
        return (self.eval(k, w + step)[0][0] - self.eval(k, w - step)[0][0]) / (2.0 * step)


def model_for(eq, mode, m=None):
    """The model of the product equilibrium `eq` (eigensolver_amd.equilibrium), built from the descriptor and the profile
    samples the product itself uploads."""
    from eigensolver_amd import shooting as s
    from tests.cases import desc_dict
    d, prof = s.make_desc(eq, mode, m)
    return CylComplexModel(desc_dict(d), {a: np.asarray(v) for a, v in prof.items()})

"""NumPy restatement of include/eigensolver_amd.h section 16 (es_cyl_complex_eigenfunction, es_cyl_complex_polarisation,
es_cyl_complex_field_synthesis; eigensolver_amd/csrc/es_cyl_complex_eigen.hip, es_cyl_complex_fields.hip): test infrastructure
on top of tests/cyl_complex_model.py.

  * interior: CylComplexModel.coef on the 2N - 1 samples, the two outward RK4 marches of the kernel (columns e = (1, 0) and d
    from the axis node to the boundary, beta from P(r_b) = 1, the axis state marched out again), xi_r = Xi / r;
  * exterior: P_e(x) = [b_s K_m(mu |x|) + E2x a_s I_m(mu |x|)] e^{-(mu |x| - mu)} / Pv with scipy.special.kve / ive as
    CylComplexModel.exterior uses them, the I part dropped at every point where Re(xR - xb) >= 40;
  * status: CylComplexModel.eval's; rows that are not OK are NaN;
  * amplitudes: tests/field_model.polarisation, which is dtype-agnostic, on complex arrays;
  * synthesis: A_re (Theta EC) - A_im (Theta ES) with EC, ES = e^{w_im t} {cos, sin}(k z - w_re t) and section 7's angular
    factors and rotations.
Beside it the independent leg: oracle.cylinder.CylinderProblem._rhs integrated by DOP853 on complex y for the two columns from
the axis point outwards, beta solved the same way, dense output at the nodes.
NumPy has no fused multiply-add and divides complex numbers by Smith's rule: agreement with the kernels is to rounding."""
import numpy as np
from scipy import special
from scipy.integrate import solve_ivp

from tests import field_model
from tests.cyl_complex_model import AXIS_KINK, ST_OK, model_for

VAR_NAMES = field_model.VAR_NAMES
AMP_NAMES = field_model.AMP_NAMES
VELOCITIES = ("v_r", "v_phi", "v_z")
NAN = complex(np.nan, np.nan)


def _forward_step(u, v, A0, Am, A1, h):
    """rk4_step_forward<false>: y' = A y with A = [[0, a12], [a21, 0]]; A = (a12, a21)."""
    h2, h6, h3 = 0.5 * h, h / 6.0, h / 3.0
    k1u, k1v = A0[0] * v, A0[1] * u
    tu, tv = h2 * k1u + u, h2 * k1v + v
    k2u, k2v = Am[0] * tv, Am[1] * tu
    tu, tv = h2 * k2u + u, h2 * k2v + v
    k3u, k3v = Am[0] * tv, Am[1] * tu
    tu, tv = h * k3u + u, h * k3v + v
    k4u, k4v = A1[0] * tv, A1[1] * tu
    return h6 * (k1u + k4u) + (h3 * (k2u + k3u) + u), h6 * (k1v + k4v) + (h3 * (k2v + k3v) + v)


class CylComplexEigenModel:
    def __init__(self, eq, mode, m=None):
        self.eq, self.mode = eq, mode
        self.M = model_for(eq, mode, m)
        d = self.M.d
        self.N, self.h = self.M.N, self.M.h
        self.x_int = d["x_boundary"] + np.arange(self.N) * self.h            # the kernel's node abscissae
        from eigensolver_amd import shooting
        self.r_nodes = np.asarray(shooting.make_desc(eq, mode, m)[1]["r"])[::2]      # the radii the profile arrays are formed at
        self.sgn = -1.0 if d["x_boundary"] < 0 else 1.0

    # ---- es_cyl_complex_eigenfunction -------------------------------------------------------------------------------------
    def interior(self, k, w, xi_e):
        """value, flux [n, N] (node 0 = boundary) and the boundary flux by the first march's columns, for arrays k, w, xi_e [n]."""
        M, N, h = self.M, self.N, self.h
        A = [M.coef(j, k, w) for j in range(2 * N - 1)]
        one, zero = np.ones_like(w), np.zeros_like(w)
        if M.d["axis_bc"] == AXIS_KINK:
            target, d0, d1 = M.d["bc_const"] * xi_e, zero, one
        else:
            target, d0, d1 = zero, A[2 * (N - 1)][0], -zero                   # d = (a12, -a11), a11 = 0
        p1, x1, p2, x2 = one, zero, d0, d1
        for j in range(N - 2, -1, -1):
            p1, x1 = _forward_step(p1, x1, A[2 * j + 2], A[2 * j + 1], A[2 * j], -h)
            p2, x2 = _forward_step(p2, x2, A[2 * j + 2], A[2 * j + 1], A[2 * j], -h)
        beta = (1.0 - target * p1) / p2
        inner = (target * x1 + beta * x2) / M.d["x_boundary"]
        u, v = target + beta * d0, beta * d1
        value, flux = np.empty((len(w), N), complex), np.empty((len(w), N), complex)
        value[:, N - 1], flux[:, N - 1] = u, v / self.x_int[N - 1]
        for j in range(N - 2, -1, -1):
            u, v = _forward_step(u, v, A[2 * j + 2], A[2 * j + 1], A[2 * j], -h)
            value[:, j], flux[:, j] = u, v / self.x_int[j]
        return value, flux, inner

    def exterior_points(self, k, w, n_ext):
        """x [n, n_ext] = linspace(sgn R, sgn 1, n_ext), P_e and xi_e_const P_e' there per unit P_e(boundary)."""
        d, sgn = self.M.d, self.sgn
        n = float(d["m_ext"])
        R = d["L_factor"] * 2.0 * np.pi / k
        x = np.stack([np.linspace(sgn * Rk, sgn * 1.0, n_ext) for Rk in R]) if n_ext else np.empty((len(k), 0))
        k2, w2 = k * k, w * w
        vAe2, ce2, cTe2 = d["vA_e"] ** 2, d["c_e"] ** 2, d["cT_e"] ** 2
        m_e = ((k2 * vAe2 - w2) * (k2 * ce2 - w2)) / ((vAe2 + ce2) * (k2 * cTe2 - w2))
        cst = -1.0 / (d["rho_e"] * (k2 * vAe2 - w2))
        mu = np.sqrt(np.where(m_e.real >= 0, m_e, 1.0 + 0j))

        def K(z):
            a, b = special.kve(n, z), special.kve(n + 1, z)
            return a, (n / z) * a - b                               # e^z K_n, e^z K_n'

        def I(z):
            ph = np.exp(-1j * z.imag)
            a, b = special.ive(n, z) * ph, special.ive(n + 1, z) * ph
            return a, b + (n / z) * a                               # e^-z I_n, e^-z I_n'

        xR, xb = mu * R, mu
        Kb, dKb = K(xb)
        KR, dKR = K(xR)
        Ib, dIb = I(xb)
        IR, dIR = I(xR)
        g = d["ic_slope"] / (sgn * mu)
        near = (xR - xb).real < 40.0
        a_s = np.where(near, -(d["ic_value"] * dKR - g * KR), 0.0)
        b_s = np.where(near, -(g * IR - d["ic_value"] * dIR), 1.0)
        Pv = np.where(near, b_s * Kb + np.exp(-2.0 * (xR - xb)) * a_s * Ib, Kb)
        xx = mu[:, None] * np.abs(x)
        Kx, dKx = K(xx)
        Ix, dIx = I(xx)
        E2x = np.exp(-2.0 * (xR[:, None] - xx))
        dec = np.exp(-(xx - xb[:, None]))
        nr, a_s, b_s = near[:, None], a_s[:, None], b_s[:, None]
        Pe = np.where(nr, b_s * Kx + E2x * a_s * Ix, b_s * Kx)
        dPe = np.where(nr, b_s * dKx + E2x * a_s * dIx, b_s * dKx)
        value = dec * Pe / Pv[:, None]
        flux = cst[:, None] * ((sgn * mu)[:, None] * (dec * dPe) / Pv[:, None])
        return x, value, flux

    def eigenfunction(self, k, w, n_ext=500):
        """The dict of CylinderComplex.eigenfunction as NumPy arrays, plus D (the model's D_c), outer and inner."""
        w = np.asarray(w, dtype=complex).reshape(-1)
        k = np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy()
        with np.errstate(all="ignore"):
            D, outer, inner, _, st = self.M.eval_points(k, w)
            _, xi_e = self.M.exterior(k, w)
            vi, fi, _ = self.interior(k, w, xi_e)
            xe, ve, fe = self.exterior_points(k, w, n_ext)
        bad = st != ST_OK
        for a in (vi, fi, ve, fe):
            a[bad] = NAN
        return dict(x_int=self.x_int, value_int=vi, flux_int=fi, x_ext=xe, value_ext=ve, flux_ext=fe, status=st, D=D,
                    outer=outer, inner=inner)

    # ---- the independent leg ------------------------------------------------------------------------------------------------
    def interior_dop853(self, prob, k, w, rtol=1e-12):
        """value, flux [N] of one OK pair with the interior by DOP853 on complex y (prob: oracle.cylinder.CylinderProblem of
        the same equilibrium), the two columns from the axis point outwards, beta from P(r_b) = 1, this model's exterior."""
        k, w = float(k), complex(w)
        st, xi_e = self.M.exterior(k, np.array([w]))
        assert st[0] == ST_OK
        rb, ra = prob.r_sign * 1.0, prob.r_sign * prob.r_axis
        r_int = np.linspace(rb, ra, self.N)
        if self.M.d["axis_bc"] == AXIS_KINK:
            target, d = self.M.d["bc_const"] * xi_e[0], (0.0, 1.0)
        else:
            Dc, C1, _, C3, _, _ = prob.coefficients(np.array([ra]), k, w)
            target, d = 0.0, (C3[0] / (ra * Dc[0]), C1[0] / Dc[0])            # (a12, -a11)
        y0 = np.array([1.0, 0.0, d[0], d[1]], dtype=complex)
        sol = solve_ivp(prob._rhs, (ra, rb), y0, method="DOP853", rtol=rtol, atol=1e-300, t_eval=r_int[::-1], args=(k, w))
        y = sol.y[:, ::-1]                                                    # boundary first
        beta = (1.0 - target * y[0, 0]) / y[2, 0]
        return target * y[0] + beta * y[2], (target * y[1] + beta * y[3]) / r_int

    # ---- es_cyl_complex_polarisation ------------------------------------------------------------------------------------------
    def profiles(self, reference_quirks=True):
        from eigensolver_amd import shooting
        return shooting.field_profiles(self.eq, self.r_nodes, reference_quirks)

    def polarisation(self, k, w, eig, reference_quirks=True):
        """radius [n, n_r], amp [n, 7, n_r] (complex) from the arrays of `eigenfunction` (or the GPU's, as NumPy)."""
        w = np.asarray(w, dtype=complex).reshape(-1)
        k = np.broadcast_to(np.asarray(k, dtype=float), w.shape)
        d, prof = self.M.d, self.profiles(reference_quirks)
        out = [field_model.polarisation(k[i], w[i], eig["value_int"][i], eig["flux_int"][i], eig["x_ext"][i],
                                        eig["value_ext"][i], eig["flux_ext"][i], prof, d["m"], d["rho_e"], d["vA_e"], d["c_e"],
                                        d["cT_e"], reference=reference_quirks) for i in range(len(w))]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- es_cyl_complex_field_synthesis ---------------------------------------------------------------------------------------------
def synthesis(radius, amp, m, k, w, theta, z, t, variables=None, v_scale=1.0, z_reference_angle=False):
    """fp64 fields [n_t, n_sel, n_z, n_theta, n_r] in ascending order of the mask bits (VAR_NAMES) and the names: the value of a
    variable with amplitude A and angular factor Theta is A_re (Theta EC) - A_im (Theta ES)."""
    names = [v for v in VAR_NAMES if variables is None or v in variables]
    m, w = float(m), complex(w)
    amp = np.asarray(amp, dtype=complex)
    A = dict(zip(AMP_NAMES, amp))
    th = np.asarray(theta, dtype=np.float64)[None, None, :, None]
    zz = np.asarray(z, dtype=np.float64)[None, :, None, None]
    tt = np.asarray(t, dtype=np.float64)[:, None, None, None]
    ph, E = k * zz - w.real * tt, np.exp(w.imag * tt)
    EC, ES = E * np.cos(ph), E * np.sin(ph)
    cm, sm = np.cos(m * th), -np.sin(m * th)
    zf = sm if z_reference_angle else cm

    def val(name, ang):
        a = A[name] * (v_scale if name in VELOCITIES else 1.0)
        return a.real[None, None, None, :] * (ang * EC) - a.imag[None, None, None, :] * (ang * ES)

    f = {"xi_r": val("xi_r", cm), "xi_phi": val("xi_phi", sm), "P_T": val("P_T", cm), "v_r": val("v_r", cm),
         "v_phi": val("v_phi", sm), "v_z": val("v_z", zf), "xi_z": val("xi_z", zf)}
    f["xi_x"] = f["xi_r"] * np.cos(th) - f["xi_phi"] * np.sin(th)
    f["xi_y"] = f["xi_r"] * np.sin(th) + f["xi_phi"] * np.cos(th)
    f["v_x"] = f["v_r"] * np.cos(th) - f["v_phi"] * np.sin(th)
    f["v_y"] = f["v_r"] * np.sin(th) + f["v_phi"] * np.cos(th)
    return np.stack([f[v] for v in names], axis=1), names


CHANNELS = {"xi_r": ("xi_r",), "xi_phi": ("xi_phi",), "P_T": ("P_T",), "v_r": ("v_r",), "v_phi": ("v_phi",), "v_z": ("v_z",),
            "xi_z": ("xi_z",), "xi_x": ("xi_r", "xi_phi"), "xi_y": ("xi_r", "xi_phi"), "v_x": ("v_r", "v_phi"),
            "v_y": ("v_r", "v_phi")}


def synthesis_bound(model, names, amp, v_scale, w, t):
    """|gpu - model| <= 2^-24 |model| + 1e-10 v_scale e^{w_im t} max|A| of the channel(s) involved (v_scale on the velocities
    only): the one rounding to fp32 plus the fp64 phase error, in the form of slab_field_model.synthesis_bound."""
    amp = np.asarray(amp, dtype=complex)
    grow = np.exp(complex(w).imag * np.asarray(t, dtype=np.float64))[:, None, None, None]
    out = np.empty_like(model)
    for i, v in enumerate(names):
        top = max(np.nanmax(np.abs(amp[AMP_NAMES.index(c)])) for c in CHANNELS[v])
        s = v_scale if v.startswith("v_") else 1.0
        out[:, i] = 2.0 ** -24 * np.abs(model[:, i]) + 1e-10 * s * top * grow
    return out


# ---- the problems of the section-16 tests: those of tests/test_cyl_complex_gpu.py, restated -------------------------------
KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0)           # the jet that is Kelvin-Helmholtz unstable
K3 = np.array([0.5, 1.1, 2.0])
NAMES = ("flow_kink", "flow_sausage", "density", "flow_m3", "density_rplus")
NODE_COUNTS = (129, 130, 300)                                         # one LDS chunk of 128 steps exactly, one more, three chunks
# the roots of the jet with r_sign = +1 at N = 130 (the model's secant iteration run to convergence)
JET_ROOTS = (("kink", 1.1, 1.496615 + 0.028018j), ("kink", 2.0, 2.673525 + 0.084845j), ("sausage", 2.0, 2.820211 + 0.096832j))


def problems(n_nodes):
    """name -> (equilibrium, mode, m, (W_lo, W_hi)): phase-speed window of the sample."""
    from eigensolver_amd import equilibrium as q
    return {
        "flow_kink": (q.CylinderFlow(**KH, width=1.5, n_nodes=n_nodes), "kink", None, (0.4, 1.7)),
        "flow_sausage": (q.CylinderFlow(**KH, width=1.5, n_nodes=n_nodes), "sausage", None, (0.4, 1.7)),
        "density": (q.CylinderDensity(width=0.95, n_nodes=n_nodes), "kink", None, (2.0, 5.5)),
        "flow_m3": (q.CylinderFlow(U_i0=0.35, width=0.9, n_nodes=n_nodes), "kink", 3, (2.7, 5.5)),
        "density_rplus": (q.CylinderDensity(width=1.5, c_e=1.5, vA_e=0.5, r_sign=1.0, n_nodes=n_nodes, ic=(1e-8, 1e-8)),
                          "kink", None, (0.5, 1.7)),
    }


def jet(n_nodes=130):
    from eigensolver_amd import equilibrium as q
    return q.CylinderFlow(**KH, width=1.5, r_sign=1.0, n_nodes=n_nodes)


def sample(window, n, seed):
    """n points: k drawn from K3, Re omega = k W with W in the window, |Im omega| in [0.05, 0.6] k / 2 with both signs; then a
    different k in every lane: each k is scaled by a factor in [0.9, 1.1] of its own (omega with it)."""
    rng = np.random.default_rng(seed)
    k = K3[rng.integers(0, 3, n)]
    w = k * rng.uniform(window[0], window[1], n) + 1j * 0.5 * k * rng.uniform(0.05, 0.6, n) * rng.choice([-1.0, 1.0], n)
    f = rng.uniform(0.9, 1.1, n)
    return k * f, w * f


def seed_of(name, n_nodes):
    return 1600 + 10 * NAMES.index(name) + n_nodes


def dop_pairs(name, n_nodes):
    """Two OK pairs of a problem for the DOP853 comparison: the first two of its sample the model calls OK."""
    eq, mode, m, window = problems(n_nodes)[name]
    k, w = sample(window, 16, seed_of(name, n_nodes))
    st = CylComplexEigenModel(eq, mode, m).M.eval_points(k, w)[4]
    ok = np.flatnonzero(st == ST_OK)[:2]
    assert len(ok) == 2, name
    return k[ok], w[ok]

"""NumPy restatement of include/eigensolver_amd.h section 20 (es_cyl_complex_vorticity_amplitudes,
es_cyl_complex_cartesian_synthesis), taking the same arrays as the C calls: complex amplitude tables [7, n_r], complex
vorticity amplitudes [3, n_r].  Everything is computed on real and imaginary parts in the floating type `dtype`, so that
`dtype=np.longdouble` gives the yardstick E_round of the tests (a table may also be handed over as a (re, im) pair of
arrays of that type).  The region, bracket, interpolation, tie and fill rules are those of tests/cartesian_model.py
(`locate`, `region_gradient`), imported, not restated.

Value rule: with c = c_re + i c_im the coefficient of a variable at a point (interpolated amplitude times the angular
factors, rotated to x, y where the variable asks for it), EC = e^{w_im t} cos(k z - w_re t), ES = e^{w_im t}
sin(k z - w_re t), the value is c_re EC - c_im ES.

Pinned on the CPU by tests/test_cyl_complex_cartesian_model.py, first of all against tests/cartesian_model.py itself through
the superposition F_c[a + i b](z, t) = e^{w_im t} (F[a](z, t) + F[b](z + pi / (2 k), t))."""
import numpy as np

from tests.cartesian_model import CVAR_NAMES, locate, region_gradient
from tests.field_model import AMP_NAMES

CVORT_NAMES = ("W_r", "W_phi", "W_z")


def parts(a, dtype=np.float64):
    """(re, im) of a complex table, or of a (re, im) pair, in `dtype`."""
    if isinstance(a, tuple):
        return np.asarray(a[0], dtype=dtype), np.asarray(a[1], dtype=dtype)
    a = np.asarray(a)
    return np.asarray(a.real, dtype=dtype), np.asarray(a.imag, dtype=dtype)


def as_complex(re_im):
    return np.asarray(re_im[0], dtype=np.float64) + 1j * np.asarray(re_im[1], dtype=np.float64)


def vorticity_amplitudes(radius, amp, n_nodes, m, k, dtype=np.float64):
    """One mode: radius [n_r], amp [7, n_r] complex (or a (re, im) pair) -> (re, im) of the three complex amplitudes of curl v,
    each [3, n_r] in `dtype`, in the order CVORT_NAMES:
        W_r = -m a_z / r + i k a_phi,   W_phi = -a_z' + i k a_r,   W_z = (m a_r - a_phi - r a_phi') / r."""
    r = np.asarray(radius, dtype=dtype)
    re, im = parts(amp, dtype)
    i_r, i_p, i_z = (AMP_NAMES.index(v) for v in ("v_r", "v_phi", "v_z"))
    m, k = dtype(m), dtype(k)
    d = lambda a: region_gradient(a, r, n_nodes, dtype)                       # noqa: E731
    with np.errstate(all="ignore"):
        w_re = np.stack([-m * re[i_z] / r - k * im[i_p], -d(re[i_z]) - k * im[i_r],
                         (m * re[i_r] - re[i_p] - r * d(re[i_p])) / r])
        w_im = np.stack([-m * im[i_z] / r + k * re[i_p], -d(im[i_z]) + k * re[i_r],
                         (m * im[i_r] - im[i_p] - r * d(im[i_p])) / r])
    return w_re, w_im


def synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, variables=None, v_scale=1.0, fill=np.nan,
              dtype=np.float64):
    """Fields [n_t, n_sel, n_z, n_y, n_x] in `dtype`, not yet rounded, in ascending order of the mask bits (CVAR_NAMES),
    `fill` where the point is outside the tabulated radii; also the names and the valid mask [n_y, n_x].  amp, vort: complex
    arrays or (re, im) pairs; vort may be None when no vorticity variable is selected; w complex."""
    names = [v for v in CVAR_NAMES if variables is None or v in variables]
    radius = np.asarray(radius, dtype=dtype)
    x, y, z, t = (np.asarray(a, dtype=dtype).reshape(-1) for a in (x, y, z, t))
    w = complex(w)
    X, Y = x[None, :], y[:, None]
    with np.errstate(all="ignore"):
        r = np.hypot(X, Y) + np.zeros_like(X * Y)
        valid, j, last = locate(radius, n_nodes, r)
        rj, rj1 = radius[j], radius[np.minimum(j + 1, radius.size - 1)]
        frac = (r - rj) / (rj1 - rj)

        def interp(a):
            a1 = a[np.minimum(j + 1, a.size - 1)]
            return np.where(last, a1, a[j] + (a1 - a[j]) * frac)

        th = np.arctan2(Y + np.zeros_like(r), X + np.zeros_like(r))
        ct, st = X / r, Y / r
        cm, sm = np.cos(dtype(m) * th), np.sin(dtype(m) * th)
        vs = dtype(v_scale)

        def coefficients(A, V):
            """Section 8's real coefficient of every variable, of one part of the tables."""
            A = {n: interp(a) for n, a in zip(AMP_NAMES, A)}
            c = {"P_T": A["P_T"] * cm,
                 "xi_x": A["xi_r"] * cm * ct - A["xi_phi"] * (-sm) * st,
                 "xi_y": A["xi_r"] * cm * st + A["xi_phi"] * (-sm) * ct,
                 "xi_z": A["xi_z"] * cm,
                 "v_x": vs * (A["v_r"] * cm * ct - A["v_phi"] * (-sm) * st),
                 "v_y": vs * (A["v_r"] * cm * st + A["v_phi"] * (-sm) * ct),
                 "v_z": vs * A["v_z"] * cm}
            if V is not None:
                V = {n: interp(a) for n, a in zip(CVORT_NAMES, V)}
                wr, wp = sm * V["W_r"], cm * V["W_phi"]
                c["vort_x"] = vs * (wr * ct - wp * st)
                c["vort_y"] = vs * (wr * st + wp * ct)
                c["vort_z"] = vs * sm * V["W_z"]
            return c

        a_re, a_im = parts(amp, dtype)
        v_re, v_im = parts(vort, dtype) if vort is not None else (None, None)
        c_re, c_im = coefficients(a_re, v_re), coefficients(a_im, v_im)
        ph = dtype(k) * z[None, :, None, None] - dtype(w.real) * t[:, None, None, None]
        growth = np.exp(dtype(w.imag) * t[:, None, None, None])
        EC, ES = growth * np.cos(ph), growth * np.sin(ph)
        out = np.empty((t.size, len(names), z.size, y.size, x.size), dtype=dtype)
        for i, v in enumerate(names):
            f = c_re[v][None, None] * EC - c_im[v][None, None] * ES
            out[:, i] = np.where(valid[None, None], f, dtype(fill))
    return out, names, valid


def synthesis_bound(model, amp, vort, v_scale, w_im, t):
    """Section 8's bound with the growth factor: |gpu - model| <= 2^-23 |model| + 1e-12 e^{w_im t} max|A|, A over the real and
    imaginary parts of the amplitudes and the vorticity amplitudes as the synthesis scales them (velocities and vorticity by
    v_scale); model [n_t, ...], t [n_t]."""
    scale = np.array([1.0, 1.0, 1.0, 1.0, v_scale, v_scale, v_scale])[:, None]
    top = max(np.nanmax(np.abs(p * scale)) for p in parts(amp))
    if vort is not None:
        top = max(top, max(np.nanmax(np.abs(p * v_scale)) for p in parts(vort)))
    growth = np.exp(float(w_im) * np.asarray(t, dtype=np.float64).reshape(-1))
    return 2.0 ** -23 * np.abs(model) + 1e-12 * top * growth.reshape((-1,) + (1,) * (np.ndim(model) - 1))


def complex_table(n_nodes, n_ext, seed=5):
    """smooth_table's radii with its amplitudes as real part and 0.8 * np.roll(amp, 3, axis=0) as imaginary part
    (n_nodes = 0: the exterior of a table with three interior nodes)."""
    from tests.cartesian_model import smooth_table
    radius, amp = smooth_table(n_nodes or 3, n_ext, seed)
    if n_nodes == 0:
        radius, amp = radius[3:], amp[:, 3:]
    return radius, amp + 1j * (0.8 * np.roll(amp, 3, axis=0))

"""NumPy restatement of include/eigensolver_amd.h section 9 (es_slab_polarisation, es_slab_field_synthesis), taking the
same arrays as the C calls: complex amplitudes from (V, Pf), the mirrored right exterior, np.gradient(..., edge_order=2)
per region for vort_y, np.searchsorted + linear interpolation per region, the tie and fill rules.  `dtype=np.longdouble`
gives the yardstick E_round of the GPU tests: the model against itself in extended precision.

Pinned on the CPU by tests/test_slab_field_model.py: the identity d(Pf)/dx = -rho (Om^2 - k^2 vA^2) V / Om on the
oracle's eigenfunctions, the kinematic relations of the synthesised fields, parities, ties and stencils."""
import numpy as np

from tests.cartesian_model import read_vtk_rectilinear, to_f32  # noqa: F401  (shared with the GPU tests)

SAMP_NAMES = ("xi_x", "xi_z", "P_T", "v_x", "v_z", "vort_y")
SVAR_NAMES = SAMP_NAMES
SCALED = ("v_x", "v_z", "vort_y")                                         # what v_scale multiplies
PROFILE_NAMES = ("rho", "c2", "vA2", "U", "dU")


def _ctype(dtype):
    return np.clongdouble if dtype is np.longdouble else np.complex128


def region_slices(n_nodes, n_ext):
    """Left exterior, interior, right exterior of a table of 2 n_ext + n_nodes points."""
    return slice(0, n_ext), slice(n_ext, n_ext + n_nodes), slice(n_ext + n_nodes, 2 * n_ext + n_nodes)


def region_gradient(a, x, n_nodes, n_ext, dtype=np.float64):
    """d a / d x by np.gradient(., x, edge_order=2) of the real and the imaginary part, on each region separately."""
    a, x = np.asarray(a, dtype=_ctype(dtype)), np.asarray(x, dtype=dtype)
    out = np.empty_like(a)
    for s in region_slices(n_nodes, n_ext):
        if a[s].size:
            if a[s].size < 3:
                raise ValueError("a region that is present needs at least 3 points")
            with np.errstate(all="ignore"):
                out[s] = np.gradient(a[s].real, x[s], edge_order=2) + 1j * np.gradient(a[s].imag, x[s], edge_order=2)
    return out


def amplitudes(k, w, x, V, Pf, rho, c2, vA2, U, dU, shear=False, dtype=np.float64):
    """The five algebraic channels at points with local (rho, c2, vA2, U, dU): dict name -> complex array, and the flux
    actually used (with the shear term when asked)."""
    ct = _ctype(dtype)
    k, w = dtype(k), ct(w)
    V, Pf = np.asarray(V, dtype=ct), np.asarray(Pf, dtype=ct)
    rho, c2, vA2, U, dU = (np.asarray(a, dtype=dtype) for a in (rho, c2, vA2, U, dU))
    with np.errstate(all="ignore"):
        S = c2 + vA2
        q, cT2 = c2 / S, c2 * vA2 / S
        Om = w - k * U
        tT = Om * Om - k * k * cT2
        if shear:
            F = rho * S * tT / (Om * Om - k * k * c2)
            Pf = Pf + (F / Om) * (k * dU / Om) * V
        xi_x = 1j * V / Om
        xi_z = k * q * Pf / (rho * tT)
        v_z = -1j * (Om * xi_z + dU * V / Om)
    return {"xi_x": xi_x, "xi_z": xi_z, "P_T": -1j * Pf, "v_x": V, "v_z": v_z}, Pf


def polarisation(k, w, V_int, Pf_int, x_ext, V_ext, Pf_ext, prof, rho_e, vA_e, c_e, U_e, sigma, shear=False,
                 dtype=np.float64):
    """One mode: the arrays of an eigenfunction call (interior node 0 = x = -1, exterior -R -> -1; x_ext etc. may be empty)
    -> (x [n_tab], amp [6, n_tab] complex) in the order SAMP_NAMES, n_tab = 2 n_ext + N."""
    ct = _ctype(dtype)
    N, n_ext = len(V_int), len(x_ext)
    x_int = np.linspace(-1.0, 1.0, N).astype(dtype)
    inner, _ = amplitudes(k, w, x_int, V_int, Pf_int, *[prof[n] for n in PROFILE_NAMES], shear=shear, dtype=dtype)
    one = np.ones(n_ext, dtype=dtype)
    ext = (rho_e * one, c_e * c_e * one, vA_e * vA_e * one, U_e * one, 0.0 * one)
    V_ext, Pf_ext = np.asarray(V_ext, dtype=ct), np.asarray(Pf_ext, dtype=ct)
    left, _ = amplitudes(k, w, x_ext, V_ext, Pf_ext, *ext, dtype=dtype)
    right, _ = amplitudes(k, w, x_ext, sigma * V_ext[::-1], -sigma * Pf_ext[::-1], *ext, dtype=dtype)
    x = np.concatenate((np.asarray(x_ext, dtype=dtype), x_int, -np.asarray(x_ext, dtype=dtype)[::-1]))
    amp = np.empty((6, x.size), dtype=ct)
    for c, name in enumerate(SAMP_NAMES[:5]):
        amp[c] = np.concatenate((left[name], inner[name], right[name]))
    with np.errstate(all="ignore"):
        amp[5] = 1j * dtype(k) * amp[3] - region_gradient(amp[4], x, N, n_ext, dtype)
    return x, amp


def locate(xtab, n_nodes, n_ext, x):
    """(valid, j, last): region and lower bracketing index of every x.  -1 <= x <= 1 interior, -R <= x < -1 left exterior,
    1 < x <= R right exterior (edges as tabulated); everything else, NaN included, is invalid."""
    xtab, x = np.asarray(xtab), np.asarray(x)
    sl, si, sr = region_slices(n_nodes, n_ext)
    xm, xp = xtab[si][0], xtab[si][-1]
    with np.errstate(invalid="ignore"):
        inside = (x >= xm) & (x <= xp)
        left = (x >= xtab[0]) & (x < xm) if n_ext else np.zeros(x.shape, bool)
        right = (x > xp) & (x <= xtab[-1]) if n_ext else np.zeros(x.shape, bool)
    j = np.zeros(x.shape, dtype=np.int64)
    last = np.zeros(x.shape, dtype=bool)
    for sel, s in ((left, sl), (inside, si), (right, sr)):
        if sel.any():
            reg = xtab[s]
            jj = np.clip(np.searchsorted(reg, x[sel], side="right") - 1, 0, reg.size - 2)
            j[sel] = s.start + jj
            last[sel] = x[sel] >= reg[jj + 1]
    return inside | left | right, j, last


def synthesis(xtab, amp, n_nodes, n_ext, k, w, x, z, t, variables=None, v_scale=1.0, fill=np.nan, dtype=np.float64):
    """Fields [n_t, n_sel, n_z, n_x] in `dtype`, not yet rounded, in ascending order of the mask bits (SVAR_NAMES), `fill`
    where x is outside the table; also the names and the valid mask [n_x]."""
    names = [v for v in SVAR_NAMES if variables is None or v in variables]
    ct = _ctype(dtype)
    xtab = np.asarray(xtab, dtype=dtype)
    x, z, t = (np.asarray(a, dtype=dtype).reshape(-1) for a in (x, z, t))
    w = complex(w)
    valid, j, last = locate(xtab, n_nodes, n_ext, x)
    with np.errstate(all="ignore"):
        x0, x1 = xtab[j], xtab[np.minimum(j + 1, xtab.size - 1)]
        frac = (x - x0) / (x1 - x0)
        ph = dtype(k) * z[None, :] - dtype(w.real) * t[:, None]                # [n_t, n_z]
        E = np.exp(dtype(w.imag) * t)[:, None]
        EC, ES = E * np.cos(ph), E * np.sin(ph)
        out = np.empty((t.size, len(names), z.size, x.size), dtype=dtype)
        for i, v in enumerate(names):
            a = np.asarray(amp[SAMP_NAMES.index(v)], dtype=ct)
            a1 = a[np.minimum(j + 1, a.size - 1)]
            re = np.where(last, a1.real, a[j].real + (a1.real - a[j].real) * frac)
            im = np.where(last, a1.imag, a[j].imag + (a1.imag - a[j].imag) * frac)
            s = dtype(v_scale) if v in SCALED else dtype(1.0)
            f = (re * s)[None, None, :] * EC[:, :, None] - (im * s)[None, None, :] * ES[:, :, None]
            out[:, i] = np.where(valid[None, None, :], f, dtype(fill))
    return out, names, valid


def synthesis_bound(model, amp, v_scale, w, t):
    """|gpu - model| <= 2^-23 |model| + 1e-12 max|A| max e^{w_im t}, A as the synthesis scales it."""
    scale = np.array([v_scale if n in SCALED else 1.0 for n in SAMP_NAMES])[:, None]
    top = np.nanmax(np.abs(np.asarray(amp, dtype=np.complex128)) * scale)
    grow = float(np.max(np.exp(complex(w).imag * np.asarray(t, dtype=np.float64))))
    return 2.0 ** -23 * np.abs(model) + 1e-12 * top * grow


def identity_residual(x, V, Pf, rho, vA2, Om, k):
    """max |d(Pf)/dx + rho (Om^2 - k^2 vA^2) V / Om| / max |rho (Om^2 - k^2 vA^2) V / Om| with np.gradient(edge_order=2)."""
    rhs = -rho * (Om * Om - k * k * vA2) * V / Om
    d = np.gradient(np.real(Pf), x, edge_order=2) + 1j * np.gradient(np.imag(Pf) + 0.0 * x, x, edge_order=2)
    return float(np.max(np.abs(d - rhs)) / np.max(np.abs(rhs)))


def smooth_mode(n_nodes, n_ext, k=1.2, R=6.0, seed=3):
    """A made-up smooth complex eigenfunction on the layout of the eigenfunction calls, with a Gaussian flow profile:
    dict(V_int, Pf_int, x_ext, V_ext, Pf_ext, prof, rho_e, vA_e, c_e, U_e).  V and Pf are unrelated smooth functions (the
    relations the synthesis must keep are kinematic); the exterior spacing is not uniform."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 1.0, n_nodes)
    g = np.exp(-x * x / 0.81)
    prof = dict(rho=1.0 + 0.3 * g, c2=0.09 + 0.02 * x * x, vA2=1.0 - 0.1 * g, U=0.35 * g, dU=0.35 * g * (-2.0 * x / 0.81))
    V_int = (np.cos(1.3 * x) + 0.4 * x) + 1j * (0.3 * np.sin(2.1 * x) + 0.2)
    Pf_int = (0.8 * np.sin(1.7 * x) - 0.5) + 1j * (0.6 * np.cos(0.9 * x) * x + 0.1)
    if n_ext:
        h = rng.uniform(0.5, 1.5, n_ext - 1)
        x_ext = -R + (R - 1.0) * np.concatenate(([0.0], np.cumsum(h))) / np.sum(h)
        x_ext[-1] = -1.0
    else:
        x_ext = np.zeros(0)
    dec = np.exp(0.9 * (x_ext + 1.0))
    V_ext = dec * ((1.0 + 0.2 * (x_ext + 1.0)) + 0.35j * np.cos(x_ext))
    Pf_ext = dec * ((0.7 - 0.1 * x_ext) + 1j * (0.25 + 0.3 * np.sin(x_ext)))
    return dict(V_int=V_int, Pf_int=Pf_int, x_ext=x_ext, V_ext=V_ext, Pf_ext=Pf_ext, prof=prof, rho_e=0.8, vA_e=2.5,
                c_e=0.2, U_e=0.05)


def smooth_table(n_nodes, n_ext, k=1.2, w=1.9 + 0.15j, sigma=1.0, shear=True, **kw):
    """(x, amp, mode dict) of smooth_mode through `polarisation`."""
    m = smooth_mode(n_nodes, n_ext, k=k, **kw)
    x, amp = polarisation(k, w, m["V_int"], m["Pf_int"], m["x_ext"], m["V_ext"], m["Pf_ext"], m["prof"], m["rho_e"],
                          m["vA_e"], m["c_e"], m["U_e"], sigma, shear=shear)
    return x, amp, m

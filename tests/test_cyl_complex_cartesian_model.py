"""CPU checks of section 20 (Cartesian sampling of an unstable cylinder mode, with its vorticity): the NumPy restatement
tests/cyl_complex_cartesian_model.py against the already pinned real model tests/cartesian_model.py (no formula restated),
against closed forms, and against a finite-difference curl of its own velocity; the exported symbols and the methods.

Bounds, none of them taken from the code under test:
  identities (superposition, phase rotation, growth)   both sides are sums of at most eight products of O(1) factors with a
                         phase of size <= 10 that is formed in two ways (k (z + d) against k z + k d), so they differ by
                         rounding alone: held to 256 * 2^-52 of the variable's largest value.
  quadratic amplitudes   the scheme and the caps of test_cartesian_model.test_quadratic_amplitudes_give_the_analytic_curl_
                         amplitudes, per part, with the form factor doubled (two terms per part).
  finite-difference curl second order: the error must fall by a factor >= 3 when the spacing halves.
Every check prints its figure with `pytest -s`.  Measured: identities <= 5.2e-16 of the variable's largest value (cap
5.7e-14); quadratic, 64 + 65 nodes: E_round <= 1.5e-13 (cap 4.1e-10); finite-difference curl at 21^3 / 41^3 points: m = 0:
6.9e-3 / 2.0e-3, m = 1: 8.7e-3 / 2.3e-3, m = 2: 4.2e-3 / 1.2e-3, m = 3: 1.6e-2 / 4.5e-3 (ratios 3.45, 3.82, 3.53, 3.54)."""
import ctypes
import re

import numpy as np
import pytest

from tests import cartesian_model as M
from tests import cyl_complex_cartesian_model as MC
from tests.field_model import AMP_NAMES

ID_TOL = 256 * 2.0 ** -52


def _close(got, want, names, what):
    worst = 0.0
    for i, v in enumerate(names):
        top = float(np.max(np.abs(want[:, i])))
        if top == 0.0:                                       # m = 0: the variables with sin(m theta) vanish on both sides
            assert np.all(got[:, i] == 0.0), (what, v)
            continue
        err = float(np.max(np.abs(got[:, i] - want[:, i]))) / top
        worst = max(worst, err)
        assert err <= ID_TOL, (what, v, err)
    print(f"{what}: max difference {worst:.2e} of the variable's largest value (cap {ID_TOL:.1e})")


def _mesh():
    return np.linspace(-1.7, 1.9, 9), np.linspace(-1.6, 1.45, 7), np.linspace(0.0, 0.7, 3), np.array([0.0, 0.45])


@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("w_im", [0.6, -0.6])
def test_superposition_of_two_real_modes_is_the_oracle(m, w_im):
    """F_c[a + i b](z, t) = e^{w_im t} (F[a](z, t) + F[b](z + pi / (2 k), t)), F the real model with its own vorticity
    amplitudes, all ten variables."""
    n_nodes, n_ext = 33, 17
    radius, amp = MC.complex_table(n_nodes, n_ext)
    k, w_re, vs = 1.3, 3.7, 2.5
    x, y, z, t = _mesh()
    vort = MC.vorticity_amplitudes(radius, amp, n_nodes, m, k)
    got, names, valid = MC.synthesis(radius, amp, vort, n_nodes, m, k, w_re + 1j * w_im, x, y, z, t, v_scale=vs, fill=0.0)
    assert names == list(M.CVAR_NAMES) and valid.any() and not valid.all()
    a, b = amp.real.copy(), amp.imag.copy()
    Fa = M.synthesis(radius, a, M.vorticity_amplitudes(radius, a, n_nodes, m, k), n_nodes, m, k, w_re, x, y, z, t,
                     v_scale=vs, fill=0.0)[0]
    Fb = M.synthesis(radius, b, M.vorticity_amplitudes(radius, b, n_nodes, m, k), n_nodes, m, k, w_re, x, y,
                     z + np.pi / (2 * k), t, v_scale=vs, fill=0.0)[0]
    want = np.exp(w_im * t)[:, None, None, None, None] * (Fa + Fb)
    _close(got, want, names, f"superposition m={m} w_im={w_im}")


@pytest.mark.parametrize("n_nodes,n_ext", [(9, 9), (3, 0), (0, 5)])
def test_real_tables_reduce_to_section_8(n_nodes, n_ext):
    radius, amp = M.smooth_table(n_nodes, n_ext) if n_nodes else (M.smooth_table(3, n_ext)[0][3:], M.smooth_table(3, n_ext)[1][:, 3:])
    for m in (0, 1, 3):
        v5 = M.vorticity_amplitudes(radius, amp, n_nodes, m, 1.3)
        re, im = MC.vorticity_amplitudes(radius, amp + 0j, n_nodes, m, 1.3)
        assert np.array_equal(re, v5[[0, 2, 4]])
        assert np.array_equal(im[:2], -v5[[1, 3]]) and np.all(im[2] == 0.0)


@pytest.mark.parametrize("m", [0, 1, 3])
def test_phase_rotation_is_a_shift_in_z(m):
    """The frames of A e^{i alpha} (all channels and the vorticity amplitudes) are the frames of A at z + alpha / k: the sign
    of every imaginary part, without a formula."""
    n_nodes, n_ext = 33, 17
    radius, amp = MC.complex_table(n_nodes, n_ext)
    k, w, alpha = 1.3, 3.7 + 0.6j, 0.83
    x, y, z, t = _mesh()
    vort = MC.as_complex(MC.vorticity_amplitudes(radius, amp, n_nodes, m, k))
    rot = np.exp(1j * alpha)
    got, names, _ = MC.synthesis(radius, amp * rot, vort * rot, n_nodes, m, k, w, x, y, z, t, v_scale=2.5, fill=0.0)
    want = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z + alpha / k, t, v_scale=2.5, fill=0.0)[0]
    _close(got, want, names, f"phase rotation m={m}")
    # and the vorticity amplitudes of the rotated table are the rotated vorticity amplitudes
    vrot = MC.as_complex(MC.vorticity_amplitudes(radius, amp * rot, n_nodes, m, k))
    assert np.max(np.abs(vrot - vort * rot)) <= ID_TOL * np.max(np.abs(vort))


@pytest.mark.parametrize("w_im", [0.6, -0.6])
def test_growth_along_the_phase(w_im):
    """The frames at (z + d, t + k d / w_re) are e^{w_im k d / w_re} times the frames at (z, t)."""
    n_nodes, n_ext = 33, 17
    radius, amp = MC.complex_table(n_nodes, n_ext)
    m, k, w_re, d = 1, 1.3, 3.7, 0.37
    x, y, z, t = _mesh()
    vort = MC.vorticity_amplitudes(radius, amp, n_nodes, m, k)
    base = MC.synthesis(radius, amp, vort, n_nodes, m, k, w_re + 1j * w_im, x, y, z, t, fill=0.0)[0]
    got, names, _ = MC.synthesis(radius, amp, vort, n_nodes, m, k, w_re + 1j * w_im, x, y, z + d, t + k * d / w_re, fill=0.0)
    _close(got, np.exp(w_im * k * d / w_re) * base, names, f"growth w_im={w_im}")


def _quadratic_table(rng, n_nodes, n_ext):
    """radius (float64), (re, im) amplitudes (longdouble) with both parts of every channel a quadratic in r, another one on
    each side of the interface; the coefficients [part][region][channel][power]."""
    radius = np.concatenate((M.nonuniform_radii(rng, 0.15, 1.0, n_nodes), M.nonuniform_radii(rng, 1.0, 3.0, n_ext) if n_ext else []))
    coef = rng.normal(size=(2, 2, 7, 3))
    amp = np.empty((2, 7, radius.size), dtype=np.longdouble)
    for h in range(2):
        for s, reg in ((slice(0, n_nodes), 0), (slice(n_nodes, None), 1)):
            r = radius[s].astype(np.longdouble)
            c = coef[h, reg].astype(np.longdouble)
            amp[h][:, s] = c[:, 0:1] + c[:, 1:2] * r + c[:, 2:3] * r * r
    return radius, amp, coef


def _analytic(radius, n_nodes, coef, m, k):
    ld = np.longdouble
    r = radius.astype(ld)
    out = np.empty((2, 3, r.size), dtype=ld)
    i_r, i_p, i_z = (AMP_NAMES.index(v) for v in ("v_r", "v_phi", "v_z"))
    for s, reg in ((slice(0, n_nodes), 0), (slice(n_nodes, None), 1)):
        rr = r[s]
        a = lambda h, ch: (lambda c: c[ch, 0] + c[ch, 1] * rr + c[ch, 2] * rr * rr)(coef[h, reg].astype(ld))   # noqa: E731
        d = lambda h, ch: (lambda c: c[ch, 1] + 2 * c[ch, 2] * rr)(coef[h, reg].astype(ld))                    # noqa: E731
        out[0][:, s] = [-ld(m) * a(0, i_z) / rr - ld(k) * a(1, i_p), -d(0, i_z) - ld(k) * a(1, i_r),
                        (ld(m) * a(0, i_r) - a(0, i_p) - rr * d(0, i_p)) / rr]
        out[1][:, s] = [-ld(m) * a(1, i_z) / rr + ld(k) * a(0, i_p), -d(1, i_z) + ld(k) * a(0, i_r),
                        (ld(m) * a(1, i_r) - a(1, i_p) - rr * d(1, i_p)) / rr]
    return out


@pytest.mark.parametrize("n_nodes,n_ext", [(9, 9), (3, 3), (3, 0), (64, 65)])
def test_quadratic_complex_amplitudes_give_the_analytic_curl_amplitudes(n_nodes, n_ext):
    rng = np.random.default_rng(100 * n_nodes + n_ext)
    radius, amp, coef = _quadratic_table(rng, n_nodes, n_ext)
    hmin = np.min(np.diff(radius)[np.diff(radius) > 0])
    for m in (0, 1, 3):
        k = 1.3
        v64 = MC.vorticity_amplitudes(radius, (amp[0].astype(np.float64), amp[1].astype(np.float64)), n_nodes, m, k)
        vld = MC.vorticity_amplitudes(radius, (amp[0], amp[1]), n_nodes, m, k, dtype=np.longdouble)
        exact = _analytic(radius, n_nodes, coef, m, k)
        # the size of the terms that are rounded, as in test_cartesian_model, twice: a part of W_r, W_phi is two terms
        form = 2 * float(np.max(np.abs(amp))) * max(1.0, 1.0 / hmin) * max(1.0, m, k) / radius[0]
        for h, part in enumerate(("Re", "Im")):
            assert v64[h].dtype == np.float64 and vld[h].dtype == np.longdouble and v64[h].shape == (3, n_nodes + n_ext)
            for c, ch in enumerate(MC.CVORT_NAMES):
                e_ld = float(np.max(np.abs(vld[h][c] - exact[h][c])))
                e_round = float(np.max(np.abs(v64[h][c] - vld[h][c])))
                err = float(np.max(np.abs(v64[h][c] - exact[h][c])))
                cap = 64 * 2.0 ** -53 * form
                print(f"quadratic N={n_nodes} n_ext={n_ext} m={m} {part} {ch:5s}: err {err:.2e}  E_round {e_round:.2e} "
                      f"(cap {cap:.1e})  longdouble - exact {e_ld:.1e}")
                assert e_ld <= 64 * float(np.finfo(np.longdouble).eps) * form
                assert e_round <= cap
                assert err <= e_round + e_ld


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_vorticity_is_the_curl_of_the_sampled_velocity(m):
    """The table and the boxes of test_cartesian_model.test_vorticity_is_the_curl_of_the_sampled_velocity, the amplitudes
    complex and the mode growing."""
    n_nodes = 4251
    radius, amp = MC.complex_table(n_nodes, 3)
    k, w = 2.1, 3.3 + 0.4j
    vort = MC.vorticity_amplitudes(radius, amp, n_nodes, m, k)
    errs = []
    for n in (21, 41):
        x = y = np.linspace(0.2, 0.65, n)
        z = np.linspace(0.0, 0.45, n)
        out, names, valid = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, [0.3], M.FD_NAMES, v_scale=2.0)
        assert names == M.FD_NAMES and valid.all()
        errs.append(M.fd_curl_error(out[0], names, x, y, z))
    print(f"fd curl m={m}: error 21^3 {errs[0]:.3e}, 41^3 {errs[1]:.3e}, ratio {errs[0] / errs[1]:.2f}")
    assert errs[0] / errs[1] >= 3.0


def test_fill_and_region_rules_are_those_of_section_8():
    """Ties, hole, far field, origin and NaN coordinates: `locate` is the real model's, and the fill reaches every variable."""
    n_nodes, n_ext = 7, 6
    radius, amp = MC.complex_table(n_nodes, n_ext)
    vort = MC.vorticity_amplitudes(radius, amp, n_nodes, 0, 1.0)
    x = np.array([-1.0, 0.0, 1.0, 0.15, 3.0, 0.05, 3.5, np.nextafter(1.0, 2.0), np.nan])
    y = np.array([0.0, 1.0, -1.0])
    out, names, valid = MC.synthesis(radius, amp, vort, n_nodes, 0, 1.0, 2.0 + 0.3j, x, y, [0.0], [0.0], fill=-7.5)
    assert np.array_equal(valid, M.locate(radius, n_nodes, np.hypot(x[None, :], y[:, None]))[0])
    assert np.all(out[0, :, 0][:, ~valid] == -7.5) and np.all(np.isfinite(out))
    P = out[0, names.index("xi_z"), 0]                       # m = 0, z = t = 0: xi_z is Re of the amplitude itself
    iP = AMP_NAMES.index("xi_z")
    for iy, ix in ((0, 0), (0, 2), (1, 1), (2, 1)):          # r == 1 exactly: the interior's boundary value
        assert P[iy, ix] == amp[iP, n_nodes - 1].real != amp[iP, n_nodes].real


def test_header_and_library_export_section_20():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "eigensolver_amd.h")) as f:
        text = f.read()
    from eigensolver_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name, count in (("es_cyl_complex_vorticity_amplitudes", 9), ("es_cyl_complex_cartesian_synthesis", 23)):
        decl = re.search(rf"^int {name}\(([^;]*)\);", text, re.M | re.S)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(args.split(",")) == count, name
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == count, name
    assert hasattr(ctypes.CDLL(build.LIB), "es_cyl_complex_cartesian_synthesis")
    assert _lib.CVORT_NAMES == MC.CVORT_NAMES
    assert "Not offered: Cartesian sampling" not in text


def test_both_classes_have_the_three_methods_once():
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex
    for name in ("vorticity_amplitudes", "cartesian_synthesis", "cartesian_fields"):
        assert callable(getattr(RotatingCylinderComplex, name, None)), name
        assert getattr(RotatingCylinderComplex, name) is getattr(CylinderComplex, name), name

"""CPU checks of section 8 (Cartesian sampling of a cylinder mode, with its vorticity): the NumPy restatement
tests/cartesian_model.py against closed forms and against a finite-difference curl of its own velocity, the tie / fill
rules, the exported symbols and the rectilinear VTK writer.

Bounds, none of them taken from the code under test:
  quadratic amplitudes   the three-point formulas are exact on quadratics, so model - analytic is rounding alone: it is
                         held to E_round = max |model(float64) - model(longdouble)| plus the longdouble model's own
                         distance from the closed form; E_round is held to 64 * 2^-53 * F and that distance to
                         64 * eps(longdouble) * F, with F = max|a| / min(h) * max(1, m, k) / radius[0] the size of the
                         terms that are rounded (see the test).
  finite-difference curl second order: the error must fall by a factor >= 3 when the spacing halves (4 in the limit).
Every check prints its figure with `pytest -s`.  Measured: quadratic, 64 + 65 nodes: E_round <= 1.5e-13 (cap 1.1e-10);
finite-difference curl at 21^3 / 41^3 points, relative to the largest vorticity component: m = 0: 6.7e-3 / 2.0e-3,
m = 1: 6.8e-3 / 1.7e-3, m = 2: 9.0e-3 / 2.2e-3, m = 3: 1.5e-2 / 4.2e-3 (ratios 3.5 - 4.1)."""
import ctypes

import numpy as np
import pytest

from tests import cartesian_model as M
from tests.field_model import AMP_NAMES


def _quadratic_table(rng, n_nodes, n_ext):
    """radius (float64), amp (longdouble) with every channel a quadratic in r, another one on each side of the interface;
    the coefficients."""
    radius = np.concatenate((M.nonuniform_radii(rng, 0.15, 1.0, n_nodes), M.nonuniform_radii(rng, 1.0, 3.0, n_ext) if n_ext else []))
    coef = rng.normal(size=(2, 7, 3))
    amp = np.empty((7, radius.size), dtype=np.longdouble)
    for s, reg in ((slice(0, n_nodes), 0), (slice(n_nodes, None), 1)):
        r = radius[s].astype(np.longdouble)
        c = coef[reg].astype(np.longdouble)
        amp[:, s] = c[:, 0:1] + c[:, 1:2] * r + c[:, 2:3] * r * r
    return radius, amp, coef


def _analytic_vorticity(radius, n_nodes, coef, m, k):
    ld = np.longdouble
    r = radius.astype(ld)
    out = np.empty((5, r.size), dtype=ld)
    for s, reg in ((slice(0, n_nodes), 0), (slice(n_nodes, None), 1)):
        rr = r[s]
        c = coef[reg].astype(ld)
        a = lambda ch: c[ch, 0] + c[ch, 1] * rr + c[ch, 2] * rr * rr          # noqa: E731
        d = lambda ch: c[ch, 1] + 2 * c[ch, 2] * rr                           # noqa: E731
        i_r, i_p, i_z = (AMP_NAMES.index(v) for v in ("v_r", "v_phi", "v_z"))
        out[:, s] = [-ld(m) * a(i_z) / rr, -ld(k) * a(i_p), -d(i_z), -ld(k) * a(i_r),
                     (ld(m) * a(i_r) - a(i_p) - rr * d(i_p)) / rr]
    return out


@pytest.mark.parametrize("n_nodes,n_ext", [(9, 9), (3, 3), (3, 0), (64, 65)])
def test_quadratic_amplitudes_give_the_analytic_curl_amplitudes(n_nodes, n_ext):
    rng = np.random.default_rng(100 * n_nodes + n_ext)
    radius, amp, coef = _quadratic_table(rng, n_nodes, n_ext)
    hmin = np.min(np.diff(radius)[np.diff(radius) > 0])
    for m in (0, 1, 3):
        k = 1.3
        v64 = M.vorticity_amplitudes(radius, amp.astype(np.float64), n_nodes, m, k)
        vld = M.vorticity_amplitudes(radius, amp, n_nodes, m, k, dtype=np.longdouble)
        exact = _analytic_vorticity(radius, n_nodes, coef, m, k)
        assert v64.dtype == np.float64 and vld.dtype == np.longdouble and v64.shape == (5, n_nodes + n_ext)
        # size of the terms whose roundings make up the error: three products of a coefficient <= 2 / min(h) with |a|, four
        # roundings each (the amplitudes' own rounding to float64 included), the factors m and k, the division by r
        form = float(np.max(np.abs(amp))) * max(1.0, 1.0 / hmin) * max(1.0, m, k) / radius[0]
        for c, ch in enumerate(M.VORT_NAMES):
            e_ld = float(np.max(np.abs(vld[c] - exact[c])))
            e_round = float(np.max(np.abs(v64[c] - vld[c])))
            err = float(np.max(np.abs(v64[c] - exact[c])))
            cap = 64 * 2.0 ** -53 * form
            print(f"quadratic N={n_nodes} n_ext={n_ext} m={m} {ch:6s}: err {err:.2e}  E_round {e_round:.2e} (cap {cap:.1e})  "
                  f"longdouble - exact {e_ld:.1e}")
            assert e_ld <= 64 * float(np.finfo(np.longdouble).eps) * form
            assert e_round <= cap
            assert err <= e_round + e_ld


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_vorticity_is_the_curl_of_the_sampled_velocity(m):
    """A radial table fine enough (h_r = 2e-4) that its linear interpolation is invisible next to the mesh's own
    truncation error; the box x, y in [0.2, 0.65] keeps 0.28 <= r <= 0.92 inside the interior."""
    n_nodes = 4251
    radius, amp = M.smooth_table(n_nodes, 3)
    k, w = 2.1, 3.3
    vort = M.vorticity_amplitudes(radius, amp, n_nodes, m, k)
    errs = []
    for n in (21, 41):
        x = y = np.linspace(0.2, 0.65, n)
        z = np.linspace(0.0, 0.45, n)
        out, names, valid = M.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, [0.3], M.FD_NAMES, v_scale=2.0)
        assert names == M.FD_NAMES and valid.all()
        errs.append(M.fd_curl_error(out[0], names, x, y, z))
    print(f"fd curl m={m}: error 21^3 {errs[0]:.3e}, 41^3 {errs[1]:.3e}, ratio {errs[0] / errs[1]:.2f}")
    assert errs[0] / errs[1] >= 3.0


def test_tie_hole_far_field_and_origin_rules():
    n_nodes, n_ext = 7, 6
    radius, amp = M.smooth_table(n_nodes, n_ext)
    assert radius[n_nodes - 1] == 1.0 == radius[n_nodes] and radius[0] == 0.15 and radius[-1] == 3.0
    vort = M.vorticity_amplitudes(radius, amp, n_nodes, 0, 1.0)
    x = np.array([-1.0, 0.0, 1.0, 0.15, 3.0, 0.05, 3.5, np.nextafter(1.0, 2.0), np.nan])
    y = np.array([0.0, 1.0, -1.0])
    for fill in (np.nan, 0.0, -7.5):
        out, names, valid = M.synthesis(radius, amp, vort, n_nodes, 0, 1.0, 2.0, x, y, [0.0], [0.0], fill=fill)
        P = out[0, names.index("xi_z"), 0]                                     # m = 0, C = 1: xi_z is the amplitude itself
        iP = AMP_NAMES.index("xi_z")                                           # (a channel that jumps at the interface)
        # r == 1 exactly, all four points: the interior's boundary value, not the exterior's
        for iy, ix in ((0, 0), (0, 2), (1, 1), (2, 1)):
            assert valid[iy, ix] and P[iy, ix] == amp[iP, n_nodes - 1] != amp[iP, n_nodes]
        assert P[0, 7] == pytest.approx(amp[iP, n_nodes], rel=1e-12) and valid[0, 7]   # one ulp outside: exterior
        assert valid[0, 3] and P[0, 3] == amp[iP, 0]                           # on the axis node
        assert valid[0, 4] and P[0, 4] == amp[iP, -1]                          # on the last far-field node
        for iy, ix in ((0, 1), (0, 5), (0, 6), (0, 8), (1, 4)):                # origin, hole, beyond, NaN, r > 3
            assert not valid[iy, ix]
            got = M.to_f32(out[0, :, 0, iy, ix])
            assert np.array_equal(got.view(np.uint32), np.full(len(names), fill, np.float32).view(np.uint32))
        if np.isfinite(fill):
            assert np.all(np.isfinite(out))                                   # the 0/0 at the origin does not leak
    # locate: brackets and the clamp on the last node
    valid, j, last = M.locate(radius, n_nodes, np.array([0.15, 1.0, 3.0, 2.0]))
    assert valid.all() and list(j[:3]) == [0, n_nodes - 2, n_nodes + n_ext - 2] and list(last) == [False, True, True, False]
    assert radius[j[3]] <= 2.0 < radius[j[3] + 1] and j[3] >= n_nodes


def test_no_exterior_and_three_point_regions():
    radius, amp = M.smooth_table(3, 0)
    vort = M.vorticity_amplitudes(radius, amp, 3, 1, 0.7)
    assert vort.shape == (5, 3) and np.all(np.isfinite(vort))
    out, names, valid = M.synthesis(radius, amp, vort, 3, 1, 0.7, 1.1, [0.5, 1.0, 1.2], [0.0], [0.1], [0.0], fill=-1.0)
    assert list(valid[0]) == [True, True, False] and np.all(out[0, :, 0, 0, 2] == -1.0)
    # three points: the first, middle and last derivative all come from the same parabola
    r = np.array([0.2, 0.5, 0.6])
    a = 1.0 - 2.0 * r + 3.0 * r * r
    assert M.region_gradient(np.concatenate((a, a)), np.concatenate((r, r)), 3) == pytest.approx(
        np.concatenate((-2 + 6 * r, -2 + 6 * r)), rel=1e-13)
    for bad in (2, 1):                                                         # a present region of fewer than 3 points
        with pytest.raises(ValueError, match="at least 3"):
            M.region_gradient(np.ones(3 + bad), np.arange(3.0 + bad), 3)
    # nothing crosses the interface: the interior derivative does not see the exterior values
    radius, amp = M.smooth_table(5, 4)
    v1 = M.vorticity_amplitudes(radius, amp, 5, 2, 0.7)
    amp2 = amp.copy()
    amp2[:, 5:] += 10.0
    v2 = M.vorticity_amplitudes(radius, amp2, 5, 2, 0.7)
    assert np.array_equal(v1[:, :5], v2[:, :5])


def test_library_exports_the_section_8_entry_points():
    from eigensolver_amd import build
    lib = ctypes.CDLL(build.build())
    for sym in ("es_cyl_vorticity_amplitudes", "es_cyl_cartesian_synthesis", "es_cyl_cartesian_split"):
        assert hasattr(lib, sym), sym
    from eigensolver_amd import _lib
    assert _lib.CVAR_NAMES == M.CVAR_NAMES and _lib.VORT_NAMES == M.VORT_NAMES
    from eigensolver_amd import shooting
    assert shooting.cartesian_var_mask(["vort_z", "P_T"]) == (0x201, ["P_T", "vort_z"])
    assert shooting.cartesian_var_mask(None)[0] == 0x3ff
    with pytest.raises(ValueError, match="unknown Cartesian field variable"):
        shooting.cartesian_var_mask(["xi_r"])


def test_launch_split_covers_every_plane_once():
    """es_cyl_cartesian_split, which the synthesis launches with: the kernel's item and plane loops, restated, visit every
    (frame, z plane) exactly once for every shape, the reference slice and shapes with short last pieces / groups included."""
    from eigensolver_amd import build
    lib = ctypes.CDLL(build.build())
    I, P = ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    lib.es_cyl_cartesian_split.argtypes = [I, I, I, I, P, P, P, P, P]

    def split(*shape):
        v = [I(0) for _ in range(5)]
        assert lib.es_cyl_cartesian_split(*shape, *[ctypes.byref(a) for a in v]) == 0
        return [a.value for a in v]

    assert split(267, 267, 31, 8) == [279, 16, 2, 2, 8]
    assert split(73, 70, 137, 3) == [20, 2, 69, 2, 104]
    seen_chunk = seen_short_piece = seen_group = seen_short_group = False
    for shape in [(1, 1, 1, 1), (267, 267, 31, 8), (73, 70, 137, 3), (512, 512, 7, 5), (1000, 1000, 3, 100), (16, 16, 1000, 70),
                  (300, 300, 100000, 1), (40, 40, 5, 30000), (3000, 3000, 1, 1), (100, 100, 33, 3)]:
        pieces, z_chunk, z_parts, ipg, groups = split(*shape)
        n_x, n_y, n_z, n_t = shape
        assert pieces == -(-n_x * n_y // 256) and 1 <= groups <= 65535 and z_parts == -(-n_z // z_chunk)
        n_items = n_t * z_parts
        assert (groups - 1) * ipg < n_items <= groups * ipg
        count = np.zeros((n_t, n_z), dtype=np.int64)
        for g in range(groups):                                               # blockIdx.y
            for item in range(g * ipg, min(g * ipg + ipg, n_items)):
                tau, piece = divmod(item, z_parts)
                count[tau, piece * z_chunk:min(piece * z_chunk + z_chunk, n_z)] += 1
        assert np.all(count == 1), shape
        seen_chunk |= z_chunk > 1
        seen_short_piece |= n_z % z_chunk != 0
        seen_group |= ipg > 1
        seen_short_group |= n_items % ipg != 0
    assert seen_chunk and seen_short_piece and seen_group and seen_short_group
    bad = [I(0) for _ in range(5)]
    for shape in ((0, 1, 1, 1), (1, 1, 1, -1)):
        assert lib.es_cyl_cartesian_split(*shape, *[ctypes.byref(a) for a in bad]) == 1


def test_rectilinear_writer_header_and_payload(tmp_path):
    from eigensolver_amd import postprocess
    rng = np.random.default_rng(3)
    x, y, z = np.linspace(-1.7, 1.9, 5), np.linspace(-1.6, 1.45, 3), np.array([0.0, 0.4])
    names = ["v_x", "vort_z"]
    data = {v: rng.normal(size=(2, 3, 5)).astype(np.float32) for v in names}
    data["v_x"][0, 1, 2] = np.nan
    path = postprocess.write_vtk_rectilinear(tmp_path / "frame", x, y, z, [data[v].astype(">f4") for v in names], names)
    assert path == str(tmp_path / "frame") + ".vtk"
    gx, gy, gz, got = M.read_vtk_rectilinear(path, names)
    assert np.array_equal(gx, x.astype(np.float32)) and np.array_equal(gy, y.astype(np.float32))
    assert np.array_equal(gz, z.astype(np.float32))
    for v in names:
        assert np.array_equal(got[v].view(np.uint32), data[v].view(np.uint32))
    # bytes and CPU torch tensors are payloads too; a payload of the wrong size and a missing name are refused
    import torch
    as_bytes = [data[v].astype(">f4").tobytes() for v in names]
    as_torch = [torch.from_numpy(data[v].astype(">f4").view(np.int32).copy()) for v in names]
    ref = open(path, "rb").read()
    for payloads in (as_bytes, as_torch):
        assert open(postprocess.write_vtk_rectilinear(tmp_path / "again", x, y, z, payloads, names), "rb").read() == ref
    with pytest.raises(ValueError, match="bytes"):
        postprocess.write_vtk_rectilinear(tmp_path / "bad", x, y, z[:1], as_bytes, names)
    with pytest.raises(ValueError, match="one name per variable"):
        postprocess.write_vtk_rectilinear(tmp_path / "bad", x, y, z, as_bytes, names[:1])

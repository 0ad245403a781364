"""Cartesian sampling of an unstable cylinder mode, with its vorticity, on the GPU (include/eigensolver_amd.h section 20)
against the NumPy restatement tests/cyl_complex_cartesian_model.py, which tests/test_cyl_complex_cartesian_model.py pins on
the real model of section 8, on identities and on closed forms.

Bounds, none of them measured on the kernels:
  amplitudes   1e-10 of each channel's max |.| (the project's bound for a kernel against a NumPy restatement of the same
               expressions), after the model's own E_round = max |model(float64) - model(longdouble)| <= 1e-11 of that max.
  synthesis    |gpu - model| <= 2^-23 |model| + 1e-12 e^{w_im t} max|A|, A over the real and imaginary parts of the amplitudes
               and the vorticity amplitudes as scaled by v_scale: section 8's bound with the growth factor.  Every mesh point
               is compared; the meshes keep every point 1e-9 away from the region edges (asserted).
  real axis    a real table handed over as complex with w_im = 0 gives the values of shooting.cartesian_synthesis,
               torch.equal: the expression has section 8's grouping.
  identities   phase rotation and growth, each side within the synthesis bound of the exact value: twice the bound.
  curl         finite-difference curl of the float32 GPU frames against their own vort_x, vort_y, vort_z: at most twice the
               error the float64 model shows on the same mesh with the same tables (the rule of tests/test_cartesian_gpu.py).
               The model's own figure is printed; it is the linear interpolation of the 130-node table, not a second-order
               mesh error, and is not capped.  Boxes, chosen on the CPU with the model:
                 jet, kink root at k = 2    x = y = linspace(0.05, 0.3, 41), z = linspace(0, 0.25, 41): r < 0.43, away from
                                            the critical layer near r = 0.81 (a box x, y in [0.2, 0.65] gives 0.25 and does
                                            not converge); the model gives 8.1e-3 there.
                 rotating tube, m = 3 root  x = y = linspace(0.2, 0.55, 41), z = linspace(0, 0.35, 41): 0.28 <= r <= 0.78, away
                                            from the axis node r = 0.01, where the amplitudes vary on the scale of the table
                                            (max |a'| ~ 1e4 there; the jet's box gives 6.4e-2 on this root and does not
                                            converge); the model gives 1.9e-3 there.
               Both figures are the table's linear interpolation (they grow when the mesh is refined past the table's
               spacing), and both boxes leave out the exterior: 20 points over [1, 9.4] are too coarse for a curl check.
Every check prints its measured figure with `pytest -s`.  On an MI355X (one run): the amplitudes of every case equal the
model's (err 0), the frames sit at 0.000 of their bound (the model is rounded to float32 as well), growth at 0.46 of twice the
bound; the curl at 41^3: jet 8.081e-3 for the float32 GPU frames, 8.075e-3 for the float64 model; tube 1.862e-3 for both; the
real root's frames equal the real path's times the sign in every value."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cartesian_model as M  # noqa: E402
from tests import cases  # noqa: E402
from tests import cyl_complex_cartesian_model as MC  # noqa: E402
from tests import cyl_complex_eigen_model as cem  # noqa: E402
from tests import cylt_complex_eigen_model as tem  # noqa: E402

ALL = list(M.CVAR_NAMES)
SHAPES = [(3, 3), (3, 0), (0, 3), (64, 65), (130, 257)]
MESHES = [(1, 1, 1, 1), (5, 3, 2, 1), (64, 2, 1, 2), (257, 3, 2, 2), (66, 6, 3, 1)]
JET_K, JET_W = 2.0, 2.673525 + 0.084845j


def _T(es_ctx, a):
    import torch
    a = np.asarray(a)
    dt = np.complex128 if np.iscomplexobj(a) else np.float64
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=f"cuda:{es_ctx.device}")


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _gpu_amplitudes(es_ctx, radius, amp, n_nodes, n_ext, m, k):
    """cyl_complex.vorticity_amplitudes on host tables radius [n, n_r], amp [n, 7, n_r] complex, k [n] -> [n, 3, n_r]."""
    from eigensolver_amd import cyl_complex
    return cyl_complex.vorticity_amplitudes(es_ctx, _T(es_ctx, radius), _T(es_ctx, np.asarray(amp, dtype=complex)), n_nodes,
                                            n_ext, m, _T(es_ctx, k))


def _synth(es_ctx, *args, **kw):
    from eigensolver_amd import cyl_complex
    return cyl_complex.cartesian_synthesis(es_ctx, *args, **kw)


def _tables(n_nodes, n_ext, n):
    rad, amp = zip(*[MC.complex_table(n_nodes, n_ext, seed=7 + i) for i in range(n)])
    scale = (1.0 + 0.5 * np.arange(n))[:, None, None]
    return np.stack(rad), np.stack(amp) * scale, 0.9 + 0.6 * np.arange(n)


def _check_amplitudes(tag, got, radius, amp, n_nodes, m, k):
    v64 = MC.vorticity_amplitudes(radius, amp, n_nodes, m, k)
    vld = MC.vorticity_amplitudes(radius, amp, n_nodes, m, k, dtype=np.longdouble)
    for c, ch in enumerate(MC.CVORT_NAMES):
        scale = float(np.max(np.hypot(v64[0][c], v64[1][c])))
        assert np.isfinite(scale) and scale > 0.0, "the model itself"
        for h, part in enumerate(("Re", "Im")):
            e_round = float(np.max(np.abs(v64[h][c] - vld[h][c])))
            g = got[c].real if h == 0 else got[c].imag
            err = float(np.max(np.abs(g - v64[h][c])))
            print(f"cvort {tag} {part} {ch:5s}: err {err:.3e} bound {1e-10 * scale:.3e}   E_round {e_round:.3e} bound {1e-11 * scale:.3e}")
            assert e_round <= 1e-11 * scale, (tag, ch, part, e_round, scale)
            assert err <= 1e-10 * scale, (tag, ch, part, err, scale)


# ---- amplitudes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes,n_ext", SHAPES)
def test_vorticity_amplitudes_match_the_model(es_ctx, n_nodes, n_ext):
    for n in (1, 3):
        radius, amp, k = _tables(n_nodes, n_ext, n)
        for m in (0, 1, 3):
            got = _gpu_amplitudes(es_ctx, radius, amp, n_nodes, n_ext, m, k).cpu().numpy()
            assert got.shape == (n, 3, n_nodes + n_ext) and got.dtype == np.complex128
            for i in range(n):
                _check_amplitudes(f"N={n_nodes} n_ext={n_ext} n={n} m={m} mode {i}", got[i], radius[i], amp[i], n_nodes, m, k[i])


def test_real_table_gives_the_section_8_amplitudes(es_ctx):
    from eigensolver_amd import shooting
    n_nodes, n_ext = 64, 65
    for m in (0, 1, 3):
        radius, amp, k = _tables(n_nodes, n_ext, 3)
        amp = amp.real.copy()
        v5 = shooting.vorticity_amplitudes(es_ctx, _T(es_ctx, radius), _T(es_ctx, amp), n_nodes, n_ext, m, _T(es_ctx, k)).cpu().numpy()
        got = _gpu_amplitudes(es_ctx, radius, amp + 0j, n_nodes, n_ext, m, k).cpu().numpy()
        assert np.array_equal(got.real, v5[:, [0, 2, 4]])                     # values, so that +0 and -0 are equal
        assert np.array_equal(got.imag[:, :2], -v5[:, [1, 3]]) and np.all(got.imag[:, 2] == 0.0)


def test_a_nan_node_reaches_its_stencil_neighbours_only(es_ctx):
    n_nodes, n_ext, m = 64, 65, 1
    stencil = {2: [0, 1, 2, 3], n_nodes + 30: [n_nodes + 29, n_nodes + 30, n_nodes + 31]}
    for part in (0, 1):
        radius, amp, k = _tables(n_nodes, n_ext, 1)
        for j in stencil:
            (amp.real if part == 0 else amp.imag)[0, :, j] = np.nan
        got = _gpu_amplitudes(es_ctx, radius, amp, n_nodes, n_ext, m, k).cpu().numpy()[0]
        model = MC.vorticity_amplitudes(radius[0], amp[0], n_nodes, m, k[0])
        for h, g in enumerate((got.real, got.imag)):
            assert np.array_equal(np.isnan(g), np.isnan(model[h])) and not np.any(np.isinf(g)), (part, h)
        nan = np.isnan(got.real) | np.isnan(got.imag)
        near = sorted(sum(stencil.values(), []))
        # W_r takes the node itself; W_phi and W_z its radial derivative: the nodes whose stencil holds it
        assert list(np.flatnonzero(nan[0])) == sorted(stencil), part
        assert list(np.flatnonzero(nan[1])) == near and list(np.flatnonzero(nan[2])) == near, part


# ---- synthesis ----------------------------------------------------------------------------------------------------
def _one_mode(es_ctx, n_nodes=64, n_ext=65, m=1, k=1.3, real=False):
    """Host and device tables of one synthetic mode, the vorticity amplitudes from the GPU."""
    radius, amp = MC.complex_table(n_nodes, n_ext)
    if real:
        amp = amp.real + 0j
    d_vort = _gpu_amplitudes(es_ctx, radius[None], amp[None], n_nodes, n_ext, m, [k])[0].contiguous()
    return radius, amp, d_vort.cpu().numpy(), _T(es_ctx, radius), _T(es_ctx, amp), d_vort


def _check(tag, got, model, amp, vort, v_scale, w_im, t, factor=1.0):
    ref = M.to_f32(model).astype(np.float64)
    bound = factor * MC.synthesis_bound(ref, amp, vort, v_scale, w_im, t)
    err = np.abs(got.astype(np.float64) - ref)
    assert got.shape == model.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    worst = np.max(err / bound)
    print(f"ccart {tag}: max |gpu - model| / bound = {worst:.3f} over {err.size} values")
    assert np.all(err <= bound), (tag, worst)


def _mesh(shape):
    n_x, n_y, n_z, n_t = shape
    return (np.linspace(-1.7, 1.9, n_x), np.linspace(-1.6, 1.45, n_y), np.linspace(0.1, 2.3, n_z), np.linspace(0.01, 1.7, n_t))


@pytest.mark.parametrize("shape", MESHES)
def test_synthesis_matches_the_model(es_ctx, shape):
    import torch
    n_nodes, n_ext, k, v_scale, fill = 64, 65, 1.3, 2.5, -7.5
    x, y, z, t = _mesh(shape)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (x, y, z, t))
    for m in (0, 1, 3):
        radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
        assert M.min_distance_to_region_edges(radius, n_nodes, x, y) > 1e-9
        for w in (3.7 + 0.6j, 3.7 - 0.6j, 3.7 + 0j):
            for mask in (ALL, ["v_x", "vort_y"]):
                model, names, valid = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, mask, v_scale, fill)
                out, got_names = _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t, mask,
                                        v_scale, fill)
                assert got_names == names
                got = out.cpu().numpy()
                # every point is compared: the model carries `fill` where the point is outside the table, and so must the GPU
                assert np.array_equal(got == np.float32(fill), np.broadcast_to(~valid, got.shape))
                _check(f"{shape} m={m} w={w} {'all' if mask is ALL else '+'.join(mask)} ({int((~valid).sum())} fill points)",
                       got, model, amp, vort, v_scale, w.imag, t)
    # an output that starts 4 bytes past a 16-byte boundary, sentinels on both sides: the same bits
    w = 3.7 + 0.6j
    ref, _ = _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, 3, k, w, d_x, d_y, d_z, d_t, ALL, v_scale, fill)
    total = ref.numel()
    buf = torch.full((total + 12,), -777.0, dtype=torch.float32, device=ref.device)
    off = (((4 - buf.data_ptr() % 16) % 16) // 4) % 4 + 4                    # data_ptr of buf[off] = 4 mod 16
    out = buf[off:off + total].view(ref.shape)
    assert out.data_ptr() % 16 == 4
    _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, 3, k, w, d_x, d_y, d_z, d_t, ALL, v_scale, fill, out=out)
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32))
    assert bool((buf[:off] == -777.0).all()) and bool((buf[off + total:] == -777.0).all())


def test_synthesis_with_several_planes_per_piece_and_items_per_workgroup(es_ctx):
    """The split is section 8's (es_cyl_cartesian_split), so the mesh of its test serves: z pieces of more than one plane with
    a shorter last piece, more than one item per workgroup with a shorter last group, groups straddling two frames."""
    from eigensolver_amd import shooting
    n_x, n_y, n_z, n_t = 73, 70, 137, 3
    s = shooting.cartesian_split(es_ctx, n_x, n_y, n_z, n_t)
    assert s["z_chunk"] > 1 and n_z % s["z_chunk"] != 0 and s["z_parts"] == -(-n_z // s["z_chunk"])
    items = n_t * s["z_parts"]
    assert s["items_per_group"] > 1 and items % s["items_per_group"] != 0 and s["groups"] == -(-items // s["items_per_group"])
    assert s["z_parts"] % 2 == 1                                             # a group straddles two frames
    n_nodes, n_ext, m, k, w, v_scale, fill = 64, 65, 2, 1.3, 3.7 + 0.6j, 2.5, -7.5
    x, y = np.linspace(-1.7, 1.9, n_x), np.linspace(-1.6, 1.45, n_y)
    z, t = np.linspace(0.0, 4.0, n_z), np.array([0.01, 0.8, 1.7])
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
    assert M.min_distance_to_region_edges(radius, n_nodes, x, y) > 1e-9
    mask = ["xi_z", "v_x", "vort_y"]
    model, names, valid = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, mask, v_scale, fill)
    out, got_names = _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, *(_T(es_ctx, a) for a in (x, y, z, t)),
                            mask, v_scale, fill)
    got = out.cpu().numpy()
    assert got_names == names and (~valid).any()
    assert np.array_equal(got == np.float32(fill), np.broadcast_to(~valid, got.shape))
    _check(f"{(n_x, n_y, n_z, n_t)} split {s}", got, model, amp, vort, v_scale, w.imag, t)


@pytest.mark.parametrize("shape", [(64, 6, 3, 2), (67, 5, 3, 2)])
def test_real_axis_gives_the_frames_of_section_8(es_ctx, shape):
    """A real table as complex, w_im = 0: the values of shooting.cartesian_synthesis on the same table, wide and narrow path."""
    import torch
    from eigensolver_amd import shooting
    n_nodes, n_ext, m, k, w, v_scale, fill = 64, 65, 3, 1.3, 3.7, 2.5, -7.5
    x, y, z, t = _mesh(shape)
    assert (shape[0] * shape[1] % 4 == 0) == (shape[0] == 64)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (x, y, z, t))
    radius, amp, _, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k, real=True)
    d_amp_real = _T(es_ctx, amp.real)
    d_vort_real = shooting.vorticity_amplitudes(es_ctx, d_radius[None], d_amp_real[None], n_nodes, n_ext, m, _T(es_ctx, [k]))[0]
    want, names = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp_real, d_vort_real.contiguous(), n_nodes, n_ext, m, k, w,
                                               d_x, d_y, d_z, d_t, ALL, v_scale, fill)
    got, got_names = _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w + 0j, d_x, d_y, d_z, d_t, ALL, v_scale, fill)
    assert got_names == names == ALL and bool((want != fill).any())
    assert torch.equal(got, want)


def test_phase_rotation_and_growth_on_the_gpu(es_ctx):
    n_nodes, n_ext, m, k, w, v_scale, fill = 64, 65, 3, 1.3, 3.7 + 0.6j, 2.5, 0.0
    x, y, z, t = _mesh((66, 6, 3, 2))
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)

    def frames(d_amp_, d_vort_, z_, t_):
        return _synth(es_ctx, d_radius, d_amp_, d_vort_, n_nodes, n_ext, m, k, w, _T(es_ctx, x), _T(es_ctx, y), _T(es_ctx, z_),
                      _T(es_ctx, t_), ALL, v_scale, fill)[0].cpu().numpy()

    base = frames(d_amp, d_vort, z, t)
    model = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, ALL, v_scale, fill)[0]
    # A e^{i alpha} against A at z + alpha / k
    alpha = 0.83
    rot = np.exp(1j * alpha)
    got = frames(_T(es_ctx, amp * rot), _T(es_ctx, vort * rot), z, t)
    shifted = frames(d_amp, d_vort, z + alpha / k, t)
    exact = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z + alpha / k, t, ALL, v_scale, fill)[0]
    bound = 2.0 * MC.synthesis_bound(M.to_f32(exact).astype(np.float64), amp, vort, v_scale, w.imag, t)
    err = np.abs(got.astype(np.float64) - shifted.astype(np.float64))
    print(f"phase rotation on the GPU: max |difference| / (2 bound) = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # (z + d, t + k d / w_re) against e^{w_im k d / w_re} (z, t)
    d = 0.37
    g = np.exp(w.imag * k * d / w.real)
    got = frames(d_amp, d_vort, z + d, t + k * d / w.real)
    bound = 2.0 * g * MC.synthesis_bound(M.to_f32(model).astype(np.float64), amp, vort, v_scale, w.imag, t)
    err = np.abs(got.astype(np.float64) - g * base.astype(np.float64))
    print(f"growth on the GPU: max |difference| / (2 bound) = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


def test_exact_ties_and_fill(es_ctx):
    from eigensolver_amd import _lib
    from tests.field_model import AMP_NAMES
    n_nodes, n_ext, m, k, w = 7, 6, 0, 1.0, 2.0 + 0.3j
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
    assert radius[n_nodes - 1] == 1.0 == radius[n_nodes] and radius[0] == 0.15 and radius[-1] == 3.0
    x, y = np.array([-1.0, 0.0, 1.0, 0.05, 3.5, np.nan]), np.array([-1.0, 0.0, 1.0])
    ties = [(1, 0), (1, 2), (0, 1), (2, 1)]                                  # (iy, ix) of (-1, 0), (1, 0), (0, -1), (0, 1)
    outside = [(1, 1), (1, 3), (1, 4), (0, 4), (2, 4), (0, 5), (1, 5), (2, 5)]   # origin, hole, far field (three), NaN (three)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (x, y, [0.0], [0.0]))
    iz = AMP_NAMES.index("xi_z")
    assert amp[iz, n_nodes - 1].real != amp[iz, n_nodes].real
    for fill in (np.nan, 0.0, -7.5):
        model, names, valid = MC.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, [0.0], [0.0], None, 1.5, fill)
        assert all(valid[p] for p in ties) and not any(valid[p] for p in outside) and int((~valid).sum()) == len(outside)
        le, _ = _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t, None, 1.5, fill)
        be, _ = _synth(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t, None, 1.5, fill,
                       flags=_lib.FIELD_BIG_ENDIAN)
        le, be = le.cpu().numpy()[0, :, 0], be.cpu().numpy()[0, :, 0]        # [n_sel, n_y, n_x]
        assert np.array_equal(be.view(np.uint32).byteswap(), le.view(np.uint32))
        fill_bits = np.float32(fill).view(np.uint32)
        for p in outside:
            assert np.all(le[(slice(None),) + p].view(np.uint32) == fill_bits), (fill, p)
        # m = 0, z = t = 0: xi_z is the real part of the amplitude, rounded once; r == 1 takes the interior's last node
        for p in ties:
            assert le[(names.index("xi_z"),) + p] == np.float32(amp[iz, n_nodes - 1].real), p
        ok = np.broadcast_to(valid, le.shape)
        ref = M.to_f32(model[0, :, 0]).astype(np.float64)
        assert np.all(np.isfinite(le[ok]))
        assert np.all(np.abs(le[ok] - ref[ok]) <= MC.synthesis_bound(ref[None], amp, vort, 1.5, w.imag, [0.0])[0][ok])
        if np.isfinite(fill):
            assert np.all(np.isfinite(le)), "the 0/0 at the origin or a NaN coordinate leaked into a finite fill"


def test_masks_are_slices_and_big_endian_is_the_swapped_result(es_ctx):
    from eigensolver_amd import _lib
    n_nodes, n_ext, m, k, w = 64, 65, 2, 0.8, 2.9 - 0.4j
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (np.linspace(-1.7, 1.9, 37), np.linspace(-1.6, 1.45, 5),
                                                   [0.0, 0.7, 1.1], [0.2, 0.9]))
    args = (d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t)
    full, names = _synth(es_ctx, *args, None, 2.0)
    full = full.cpu().numpy()
    assert names == ALL
    for sub in (["P_T"], ["vort_x"], ["xi_y", "vort_z"], ["v_z", "xi_x", "vort_y", "v_x"]):
        got, got_names = _synth(es_ctx, *args, sub, 2.0)
        assert got_names == [v for v in ALL if v in sub]
        want = full[:, [ALL.index(v) for v in got_names]]
        assert np.array_equal(_bits(got), want.view(np.uint32)), sub
    no_vort, _ = _synth(es_ctx, d_radius, d_amp, None, *args[3:], ["P_T", "v_y"], 2.0)
    assert np.array_equal(_bits(no_vort), full[:, [0, 5]].view(np.uint32))
    be, _ = _synth(es_ctx, *args, None, 2.0, flags=_lib.FIELD_BIG_ENDIAN)
    assert np.array_equal(_bits(be).byteswap(), full.view(np.uint32))


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jet(es_ctx):
    """CylinderComplex of the jet with r_sign = +1 at N = 130 and its kink root at k = 2, polished by Newton's iteration."""
    from eigensolver_amd import CylinderComplex
    c = CylinderComplex(cem.jet(130), ctx=es_ctx)
    r = c.newton("kink", [JET_K], [JET_W])
    w = complex(r["w"].cpu().numpy()[0])
    assert int(r["flag"].cpu().numpy()[0]) == 1 and abs(w - JET_W) < 1e-6
    yield c, "kink", None, JET_K, w
    c.close()


@pytest.fixture(scope="module")
def tube(es_ctx):
    """RotatingCylinderComplex of case A (v_twist = 2, power = 1) at N = 130 and its unstable m = 3 root at k = 1."""
    from eigensolver_amd import RotatingCylinderComplex
    eq, mode, m, _, _, _ = tem.problems(130)["A"]
    c = RotatingCylinderComplex(eq, ctx=es_ctx)
    k, w0 = tem.ROOT_A
    r = c.newton(mode, [k], [w0], m=m)
    w = complex(r["w"].cpu().numpy()[0])
    assert int(r["flag"].cpu().numpy()[0]) == 1 and abs(w - w0) < 1e-6
    yield c, mode, m, k, w
    c.close()


BOXES = {"jet": (np.linspace(0.05, 0.3, 41), np.linspace(0.0, 0.25, 41)),
         "tube": (np.linspace(0.2, 0.55, 41), np.linspace(0.0, 0.35, 41))}


@pytest.mark.parametrize("which", ["jet", "tube"])
def test_end_to_end_amplitudes_and_curl(which, request):
    c, mode, m, k, w = request.getfixturevalue(which)
    tab = {a: b.cpu().numpy()[0] for a, b in c.vorticity_amplitudes(mode, [k], [w], n_ext=20, m=m).items()}
    assert tab["status"] == 0 and tab["radius"].shape == (150,) and tab["vort"].shape == (3, 150)
    assert np.all(np.isfinite(tab["amp"].view(np.float64)))
    order = int(c.problem(mode, m).desc.m)
    _check_amplitudes(f"{which} root", tab["vort"], tab["radius"], tab["amp"], 130, order, k)
    xy, z = BOXES[which]
    t = [0.3]
    f = c.cartesian_fields(mode, k, w, xy, xy, z, t, variables=M.FD_NAMES, n_ext=20, m=m)
    assert f["names"] == M.FD_NAMES and f["frames"].shape == (1, 6, 41, 41, 41)
    e_gpu = M.fd_curl_error(f["frames"][0].cpu().numpy(), M.FD_NAMES, xy, xy, z)
    vort = MC.vorticity_amplitudes(tab["radius"], tab["amp"], 130, order, k)
    model, names, valid = MC.synthesis(tab["radius"], tab["amp"], vort, 130, order, k, w, xy, xy, z, t, M.FD_NAMES)
    assert valid.all() and np.hypot(xy[-1], xy[-1]) < 1.0                     # inside the interior
    e_model = M.fd_curl_error(model[0], names, xy, xy, z)
    print(f"fd curl of the {which} root, 41^3: float32 GPU frames {e_gpu:.3e}, float64 model {e_model:.3e}")
    assert e_gpu <= 2.0 * e_model


def test_real_root_agrees_with_the_real_path(es_ctx):
    """A real root of CF_flow_kink on positive radii: CylinderComplex.cartesian_fields against ShootProblem.cartesian_fields
    times sign(P_e(boundary)) (section 14's normalisation), to one fp32 rounding plus the 1e-12 term.  Not bit-equal: the two
    eigenfunction kernels agree to rounding only."""
    from eigensolver_amd import CylinderComplex
    eq, mode, m, _ = cases.all_cases()["CF_flow_kink"]
    c = CylinderComplex(dataclasses.replace(eq, r_sign=1.0, n_nodes=130), ctx=es_ctx)
    p = c.problem(mode, m)
    kk = np.array([1.1])
    Wv = 2.7 + (np.arange(96) + 0.5) * (4.95 - 2.7) / 96
    D, st = p.eval_grid(kk, Wv)
    roots, _ = p.find_roots(kk, Wv, D, st, n_bisect=40, tol_percent=1e-3)
    ok = roots["flag"].cpu().numpy() == 1
    assert ok.any(), "no accepted root in the window"
    k, w = float(roots["k"].cpu().numpy()[ok][0]), float(roots["w"].cpu().numpy()[ok][0])
    sign = float(np.sign(p.eigenfunction([k], [w], n_ext=20)["value_ext"].cpu().numpy()[0, -1]))
    x, y, z, t = _mesh((66, 6, 3, 2))
    real = p.cartesian_fields(k, w, x, y, z, t, v_scale=2.0, fill=0.0, n_ext=20)
    cplx = c.cartesian_fields(mode, k, w + 0j, x, y, z, t, v_scale=2.0, fill=0.0, n_ext=20, m=m)
    assert real["names"] == cplx["names"] == ALL
    a, b = sign * real["frames"].cpu().numpy().astype(np.float64), cplx["frames"].cpu().numpy().astype(np.float64)
    tab = {n: v.cpu().numpy()[0] for n, v in p.vorticity_amplitudes([k], [w], n_ext=20).items()}
    bound = M.synthesis_bound(a, tab["amp"], tab["vort"], 2.0)
    print(f"real root k={k} w={w:.6f}: max |complex - sign * real| / bound = {np.max(np.abs(a - b) / bound):.3f}; "
          f"values that differ: {int(np.sum(a != b))} of {a.size}")
    assert np.any(a != 0.0) and np.all(np.abs(a - b) <= bound)
    c.close()


# ---- the Python layer ---------------------------------------------------------------------------------------------
def test_chunked_frames_equal_the_one_call_result(jet):
    import torch
    c, mode, m, k, w = jet
    x, y, z, t = np.linspace(-1.7, 1.9, 9), np.linspace(-1.6, 1.45, 6), np.array([0.01, 1.2]), np.linspace(0.01, 2.0, 3)
    one = c.cartesian_fields(mode, k, w, x, y, z, t, n_ext=20, fill=0.0)
    chunks = list(c.cartesian_fields(mode, k, w, x, y, z, t, n_ext=20, fill=0.0, frames_per_call=1))
    assert [ch["frames"].shape[0] for ch in chunks] == [1, 1, 1]
    assert torch.equal(torch.cat([ch["frames"] for ch in chunks]).view(torch.int32), one["frames"].view(torch.int32))
    assert torch.equal(torch.cat([ch["t"] for ch in chunks]), one["t"])
    assert one["names"] == ALL and torch.equal(one["vort_z"], one["frames"][:, ALL.index("vort_z")])
    assert one["frames"].shape == (3, 10, 2, 6, 9) and bool(torch.isfinite(one["frames"]).all())
    few = c.cartesian_fields(mode, k, w, x, y, z, t, variables=["v_x", "P_T"], n_ext=20, fill=0.0)
    assert few["names"] == ["P_T", "v_x"]
    assert torch.equal(few["v_x"].contiguous().view(torch.int32), one["v_x"].contiguous().view(torch.int32))


@pytest.mark.parametrize("which", ["jet", "tube"])
def test_rectilinear_frames_parse_back(which, request, tmp_path):
    from eigensolver_amd import postprocess
    c, mode, m, k, w = request.getfixturevalue(which)
    x, y, z, t = np.linspace(-1.7, 1.9, 9), np.linspace(-1.6, 1.45, 6), np.array([0.01, 1.2]), np.array([0.01, 0.9, 1.4])
    names = ["v_x", "vort_x", "vort_z"]
    plain = c.cartesian_fields(mode, k, w, x, y, z, t, variables=names, n_ext=20, m=m)["frames"].cpu().numpy()
    chunks = c.cartesian_fields(mode, k, w, x, y, z, t, variables=names, n_ext=20, big_endian=True, frames_per_call=2, m=m)
    files = postprocess.write_vtk_rectilinear_frames(str(tmp_path / "cc_cart_"), x, y, z, chunks)
    assert files == [str(tmp_path / "cc_cart_") + f"{i}.vtk" for i in range(3)]
    assert np.isfinite(plain).any()
    for i, path in enumerate(files):
        gx, gy, gz, got = M.read_vtk_rectilinear(path, names)
        assert np.array_equal(gx, x.astype(np.float32)) and np.array_equal(gy, y.astype(np.float32))
        assert np.array_equal(gz, z.astype(np.float32))
        for j, v in enumerate(names):
            assert np.array_equal(got[v].view(np.uint32), plain[i, j].view(np.uint32)), (i, v)


def test_refusals_of_the_python_layer(es_ctx, jet):
    from eigensolver_amd import CylinderComplex
    c, mode, m, k, w = jet
    neg = CylinderComplex(dataclasses.replace(cem.jet(11), r_sign=-1.0), ctx=es_ctx)
    try:
        with pytest.raises(ValueError, match=r"r_sign=\+1"):
            neg.vorticity_amplitudes(mode, [k], [w], n_ext=4)
        with pytest.raises(ValueError, match=r"r_sign=\+1"):
            neg.cartesian_fields(mode, k, w, [0.5], [0.0], [0.0], [0.0])
    finally:
        neg.close()
    for n_ext in (1, 2):                                                     # refused before anything is marched
        with pytest.raises(ValueError, match="at least 3 points"):
            c.vorticity_amplitudes(mode, [k], [w], n_ext=n_ext)
        with pytest.raises(ValueError, match="at least 3 points"):
            c.cartesian_fields(mode, k, w, [0.5], [0.0], [0.0], [0.0], n_ext=n_ext)
    for bad_k, bad_w in (([k, k], [w, w]), (k, [w]), ([k], w)):
        with pytest.raises(ValueError, match="one root"):
            c.cartesian_fields(mode, bad_k, bad_w, [0.5], [0.0], [0.0], [0.0])
    with pytest.raises(ValueError, match="unknown Cartesian field variable"):
        c.cartesian_fields(mode, k, w, [0.5], [0.0], [0.0], [0.0], variables=["xi_r"])
    with pytest.raises(ValueError, match="frames_per_call"):
        c.cartesian_fields(mode, k, w, [0.5], [0.0], [0.0], [0.0], frames_per_call=0)


# ---- the C interface: argument errors and empty calls -----------------------------------------------------------------
def test_argument_errors_and_empty_calls(es_ctx):
    import torch
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    N, n_ext, n_x, n_y, n_z, n_t = 4, 3, 5, 3, 2, 2
    n_r = N + n_ext
    d = lambda *s: torch.ones(s, dtype=torch.float64, device=dev)            # noqa: E731
    radius = torch.tensor([0.2, 0.5, 0.8, 1.0, 1.0, 2.0, 3.0], dtype=torch.float64, device=dev)
    amp = torch.ones((7, n_r), dtype=torch.complex128, device=dev) * (1.0 + 0.5j)
    vort = torch.ones((3, n_r), dtype=torch.complex128, device=dev) * (1.0 + 0.5j)
    kk = d(1)
    x, y, z, t = torch.linspace(-1.5, 1.5, n_x, dtype=torch.float64, device=dev), d(n_y) * 0.3, d(n_z), d(n_t)
    out = torch.full((n_t * 10 * n_z * n_y * n_x,), -5.0, dtype=torch.float32, device=dev)
    vout = torch.full((3, n_r, 2), -77.0, dtype=torch.float64, device=dev)
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None        # noqa: E731

    def syn(rad=radius, amp_=amp, vort_=vort, N_=N, n_ext_=n_ext, m=1, x_=x, n_x_=n_x, y_=y, n_y_=n_y, z_=z, n_z_=n_z, t_=t,
            n_t_=n_t, mask=0x3ff, flags=0, out_=out, out_off=0):
        po = C.c_void_p(out_.data_ptr() + out_off) if out_ is not None else None
        return lib.es_cyl_complex_cartesian_synthesis(h, P(rad), P(amp_), P(vort_), N_, n_ext_, m, 1.0, 2.0, 0.25, P(x_), n_x_,
                                                      P(y_), n_y_, P(z_), n_z_, P(t_), n_t_, mask, 1.0, float("nan"), flags, po)

    def amps(rad=radius, amp_=amp, n=1, N_=N, n_ext_=n_ext, m=1, k_=kk, v=vout):
        return lib.es_cyl_complex_vorticity_amplitudes(h, P(rad), P(amp_), n, N_, n_ext_, m, P(k_), P(v))

    for bad in (dict(mask=0), dict(mask=1 << 10), dict(vort_=None), dict(vort_=None, mask=1 << 9), dict(flags=2),
                dict(flags=2 | 4), dict(flags=1), dict(flags=8), dict(N_=2, n_ext_=5), dict(N_=5, n_ext_=2),
                dict(N_=0, n_ext_=0), dict(N_=-1), dict(n_ext_=-1), dict(n_x_=-1), dict(n_y_=-1), dict(n_z_=-1),
                dict(n_t_=-1), dict(m=-1), dict(out_off=2), dict(rad=None), dict(amp_=None), dict(x_=None), dict(y_=None),
                dict(z_=None), dict(t_=None), dict(out_=None)):
        assert syn(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)
    for bad in (dict(n=-1), dict(N_=-1), dict(n_ext_=-1), dict(m=-1), dict(N_=2, n_ext_=5), dict(N_=5, n_ext_=2),
                dict(N_=1, n_ext_=0), dict(rad=None), dict(amp_=None), dict(k_=None), dict(v=None)):
        assert amps(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)
    # empty calls succeed and write nothing
    for empty in (dict(n_x_=0), dict(n_y_=0), dict(n_z_=0), dict(n_t_=0), dict(n_t_=0, t_=None, out_=None),
                  dict(n_x_=0, x_=None)):
        assert syn(**empty) == 0, empty
    assert amps(n=0) == 0 and amps(n=0, rad=None, amp_=None, k_=None, v=None) == 0 and amps(N_=0, n_ext_=0) == 0
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((vout == -77.0).all())
    assert syn(vort_=None, mask=0x7f) == 0 and amps() == 0 and amps(N_=0, n_ext_=n_r) == 0 and amps(N_=n_r, n_ext_=0) == 0
    assert syn() == 0
    es_ctx.synchronize()
    assert bool((out != -5.0).all()) and bool((vout != -77.0).all())

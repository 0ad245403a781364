"""es_cyl_complex_polarisation / es_cyl_complex_field_synthesis (C ABI section 16) and CylinderComplex.polarisation / .fields:
the growing movie of an unstable cylinder mode.

Frames against the model's synthesis (tests/cyl_complex_eigen_model.py) on the GPU's own amplitude table:
    |got - v| <= 2^-24 |v| + 1e-10 v_scale e^{w_im t} max|A| of the channel(s) involved
(one rounding to fp32 plus the fp64 phase error; the form of slab_field_model.synthesis_bound).  n_r = 160 (16-byte stores) and
167 (ragged last lane, 4-byte stores); misaligned output, big-endian, masks and chunked calls compare bits.  On the real axis
the frames are those of ShootProblem.fields to one fp32 rounding."""
import ctypes as C

import numpy as np
import pytest

from tests import cyl_complex_eigen_model as cem

pytestmark = pytest.mark.gpu

INVALID = 1
THETA = np.linspace(0.0, 2.0 * np.pi, 5)
Z = np.array([0.0, 0.45, 1.3])
T = np.array([0.2, 1.9])
MODE, K, W = "kink", 2.0, 2.673525 + 0.084845j               # a root of the jet (cem.JET_ROOTS)


def _np(d):
    return {a: (v.cpu().numpy() if hasattr(v, "cpu") else v) for a, v in d.items()}


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def jet(es_ctx):
    """CylinderComplex of the jet with r_sign = +1 at N = 130 and its kink root at k = 2, polished by Newton's iteration."""
    from eigensolver_amd import CylinderComplex
    c = CylinderComplex(cem.jet(130), ctx=es_ctx)
    r = c.newton(MODE, [K], [W])
    w = complex(r["w"].cpu().numpy()[0])
    assert int(r["flag"].cpu().numpy()[0]) == 1 and abs(w - W) < 1e-6
    yield c, w
    c.close()


@pytest.mark.parametrize("n_ext", [30, 37])
def test_polarisation_and_fields_against_model(jet, n_ext):
    c, w = jet
    E = cem.CylComplexEigenModel(cem.jet(130), MODE)
    eig = _np(c.eigenfunction(MODE, [K], [w], n_ext=n_ext))
    pol = _np(c.polarisation(MODE, [K], [w], n_ext=n_ext))
    assert pol["status"][0] == 0 and pol["amp"].shape == (1, 7, 130 + n_ext) and pol["amp"].dtype == np.complex128
    radius_m, amp_m = E.polarisation([K], [w], eig)
    assert np.array_equal(pol["radius"], radius_m)
    assert pol["radius"][0, 129] == 1.0 and pol["radius"][0, 130] == 1.0          # the boundary radius twice
    scale = np.max(np.abs(amp_m), axis=2, keepdims=True)
    err = float(np.max(np.abs(pol["amp"] - amp_m) / scale))
    print(f"n_r={130 + n_ext}: max |amp - model| / max|channel| = {err:.3e}")
    assert err < 1e-12                                                            # formulas on the same inputs: rounding
    radius, amp = pol["radius"][0], pol["amp"][0]
    for v_scale in (1.0, 25.0):
        f = c.fields(MODE, K, w, THETA, Z, T, v_scale=v_scale, n_ext=n_ext)
        got = f["frames"].cpu().numpy().astype(np.float64)
        model, names = cem.synthesis(radius, amp, 1, K, w, THETA, Z, T, v_scale=v_scale, z_reference_angle=True)
        assert names == f["names"] and got.shape == model.shape == (2, 11, 3, 5, 130 + n_ext)
        bnd = cem.synthesis_bound(model, names, amp, v_scale, w, T)
        worst = float(np.max(np.abs(got - model) / bnd))
        print(f"n_r={130 + n_ext} v_scale={v_scale}: max |frames - model| / bound = {worst:.3f}")
        assert np.all(np.abs(got - model) <= bnd)
        pts = f["points"].cpu().numpy().astype(np.float64)
        want = np.stack(np.broadcast_arrays(radius[None, None, :] * np.cos(THETA)[None, :, None],
                                            radius[None, None, :] * np.sin(THETA)[None, :, None], Z[:, None, None]), axis=-1)
        assert np.all(np.abs(pts - want) <= 2.0 ** -23 * np.abs(want) + 1e-15)      # the bound of tests/test_fields_gpu.py


@pytest.mark.parametrize("n_ext", [30, 37])
def test_layout_variants_compare_bits(jet, n_ext):
    import torch
    c, w = jet
    full = c.fields(MODE, K, w, THETA, Z, T, v_scale=3.0, n_ext=n_ext)
    ref = _bits(full["frames"])
    # misaligned output: a view offset by one float
    pol = c.polarisation(MODE, [K], [w], n_ext=n_ext)
    radius, amp = pol["radius"][0], pol["amp"][0].contiguous()
    p = c.problem(MODE)
    dth, dz, dt = (p._dev(a) for a in (THETA, Z, T))
    buf = torch.empty(ref.size + 1, dtype=torch.float32, device=radius.device)
    out = buf[1:].view(full["frames"].shape)
    assert out.data_ptr() % 16 == 4
    c.field_synthesis(radius, amp, 1, K, w, dth, dz, dt, None, 3.0, 2, want_points=False, out=out)
    assert np.array_equal(_bits(out), ref)
    # big-endian: the byte swap of the little-endian call, points included
    be = c.fields(MODE, K, w, THETA, Z, T, v_scale=3.0, n_ext=n_ext, big_endian=True)
    for a in ("frames", "points"):
        assert np.array_equal(be[a].cpu().numpy().view(">f4").astype("<f4").view(np.uint32), _bits(full[a])), a
    # a two-variable mask: those slices of the full call
    two = c.fields(MODE, K, w, THETA, Z, T, variables=["v_y", "xi_phi"], v_scale=3.0, n_ext=n_ext)
    assert two["names"] == ["xi_phi", "v_y"]
    for v in two["names"]:
        assert np.array_equal(_bits(two[v]), _bits(full[v])), v
    # one frame per call
    chunks = list(c.fields(MODE, K, w, THETA, Z, T, v_scale=3.0, n_ext=n_ext, frames_per_call=1))
    assert len(chunks) == 2 and all(ch["points"] is chunks[0]["points"] for ch in chunks)
    assert np.array_equal(np.concatenate([_bits(ch["frames"]) for ch in chunks]), ref)
    assert np.array_equal(_bits(chunks[0]["points"]), _bits(full["points"]))


def test_growth_between_two_frames(jet):
    """The frame at t2 on a mesh shifted along z by Re w (t2 - t1) / k is e^{Im w (t2 - t1)} times the frame at t1."""
    c, w = jet
    t1, t2 = 0.3, 2.1
    a = c.fields(MODE, K, w, THETA, Z, [t1], n_ext=30)["frames"].cpu().numpy().astype(np.float64)
    b = c.fields(MODE, K, w, THETA, Z + w.real * (t2 - t1) / K, [t2], n_ext=30)["frames"].cpu().numpy().astype(np.float64)
    g = np.exp(w.imag * (t2 - t1))
    pol = _np(c.polarisation(MODE, [K], [w], n_ext=30))
    top = np.nanmax(np.abs(pol["amp"][0]))
    # one fp32 rounding on each side, and the fp64 phase of a shifted z
    assert np.all(np.abs(b - g * a) <= 2.0 ** -23 * np.abs(g * a) + 1e-10 * top * np.exp(w.imag * t2))
    assert g > 1.1


def test_fields_to_vtk_files(jet, tmp_path):
    from eigensolver_amd import postprocess
    c, w = jet
    names = ["xi_r", "P_T", "xi_x", "v_y", "v_z"]
    f = c.fields(MODE, K, w, THETA, Z, T, variables=names, v_scale=25.0, big_endian=True, n_ext=30)
    files = postprocess.write_vtk_frames(str(tmp_path / "jet_kink_"), f)
    assert files == [str(tmp_path / "jet_kink_") + f"{i}.vtk" for i in range(2)]
    le = c.fields(MODE, K, w, THETA, Z, T, variables=names, v_scale=25.0, n_ext=30)
    n = 160 * 5 * 3
    for i, path in enumerate(files):
        raw = open(path, "rb").read()
        assert b"DIMENSIONS  160 5 3" in raw
        pos = raw.index(b"\n", raw.index(b"POINTS ")) + 1
        pts = np.frombuffer(raw, dtype=">f4", count=3 * n, offset=pos).astype("<f4")
        assert np.array_equal(pts.view(np.uint32), _bits(le["points"]).ravel())
        pos += 12 * n
        for v in f["names"]:
            tag = ("\nSCALARS %s float \nLOOKUP_TABLE default \n" % v).encode()
            pos = raw.index(tag, pos) + len(tag)
            got = np.frombuffer(raw, dtype=">f4", count=n, offset=pos).astype("<f4")
            assert np.array_equal(got.view(np.uint32), _bits(le[v][i]).ravel()), (i, v)
            pos += 4 * n
        assert pos == len(raw)


def test_real_axis_frames_are_section_7(es_ctx):
    """w_im = 0 on density_rplus: the frames of ShootProblem.fields times sign(P_e(boundary)), to one fp32 rounding."""
    from eigensolver_amd import CylinderComplex
    eq, mode, m, window = cem.problems(130)["density_rplus"]
    c = CylinderComplex(eq, ctx=es_ctx)
    p = c.problem(mode, m)
    k = 1.1
    cand = k * np.linspace(window[0] + 0.02, window[1], 24)
    st = p.eval_points(np.full(24, k), cand)[1].cpu().numpy()
    w = float(cand[np.flatnonzero(st == 0)[0]])
    sign = float(np.sign(p.eigenfunction([k], [w], n_ext=30)["value_ext"].cpu().numpy()[0, -1]))
    real = p.fields(k, w, THETA, Z, T, v_scale=2.0, n_ext=30)
    cplx = c.fields(mode, k, w + 0j, THETA, Z, T, v_scale=2.0, n_ext=30, m=m)
    assert real["names"] == cplx["names"]
    a, b = sign * real["frames"].cpu().numpy().astype(np.float64), cplx["frames"].cpu().numpy().astype(np.float64)
    same = np.array_equal((sign * real["frames"]).cpu().numpy().view(np.uint32), _bits(cplx["frames"]))
    top = float(np.max(np.abs(a)))
    print(f"real axis: frames bit-identical to section 7: {same}; values that differ: {int(np.sum(a != b))} of {a.size} (equal values "
          f"with other bits are zeros of the other sign); max |difference| / max|frame| = {np.max(np.abs(a - b)) / top:.3e}")
    # one fp32 rounding, and amplitudes that agree to 1e-10 of their maximum (test_real_axis_is_the_real_path)
    amp = p.polarisation([k], [w], n_ext=30)["amp"].cpu().numpy()[0]
    assert np.all(np.abs(a - b) <= 2.0 ** -23 * np.abs(a) + 1e-10 * 2.0 * np.max(np.abs(amp)))
    assert np.array_equal(_bits(real["points"]), _bits(cplx["points"]))
    c.close()


def test_synthesis_argument_errors_and_empty_meshes(es_ctx):
    import torch
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    n_r, n_th, n_z, n_t = 5, 3, 2, 2
    d = lambda n: torch.ones(max(n, 1), dtype=torch.float64, device=dev)     # noqa: E731
    radius, amp, theta, z, t = d(n_r), d(7 * n_r * 2), d(n_th), d(n_z), d(n_t)
    out = torch.full((n_t * 11 * n_z * n_th * n_r,), -5.0, dtype=torch.float32, device=dev)
    pts = torch.full((n_z * n_th * n_r * 3,), -5.0, dtype=torch.float32, device=dev)
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None        # noqa: E731

    def call(rad=radius, amp_=amp, n_r_=n_r, m=1, th=theta, n_th_=n_th, z_=z, n_z_=n_z, t_=t, n_t_=n_t, mask=0x7ff, flags=0,
             pts_=pts, out_=out, out_off=0):
        po = C.c_void_p(out_.data_ptr() + out_off) if out_ is not None else None
        return lib.es_cyl_complex_field_synthesis(h, P(rad), P(amp_), n_r_, m, 1.0, 2.0, 0.1, P(th), n_th_, P(z_), n_z_, P(t_),
                                                  n_t_, mask, 1.0, flags, P(pts_), po)
    for bad in (dict(mask=0), dict(mask=1 << 11), dict(n_r_=-1), dict(n_th_=-1), dict(n_z_=-1), dict(n_t_=-1), dict(m=-1),
                dict(flags=1), dict(flags=8), dict(rad=None), dict(amp_=None), dict(th=None), dict(z_=None), dict(t_=None),
                dict(out_=None), dict(out_off=2)):
        assert call(**bad) == INVALID, bad
    assert b"invalid argument" in lib.es_last_error(h)
    for empty in (dict(n_t_=0, pts_=None), dict(n_r_=0), dict(n_th_=0), dict(n_z_=0),
                  dict(n_t_=0, pts_=None, t_=None, out_=None), dict(n_r_=0, rad=None, amp_=None, out_=None, pts_=None)):
        assert call(**empty) == 0, empty
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((pts == -5.0).all())
    assert call(n_t_=0) == 0                                                 # no frames, the points alone
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((pts != -5.0).all())
    assert call() == 0
    es_ctx.synchronize()
    assert bool((out != -5.0).all())

"""Perturbation fields of a cylinder mode on the GPU (include/eigensolver_amd.h section 7) against the NumPy restatement
tests/field_model.py, which tests/test_field_model.py pins on the export scripts' own arrays.

Bounds, none of them measured on the kernels:
  polarisation   1e-10 of each channel's max: a GPU kernel against a NumPy restatement of the same expressions, the
                 project's bound for that (tests/test_eigenfunction_gpu.py, b).  Every pair used is asserted to keep every
                 node 1e-3 (relative) away from Om^2 = omega_A^2 and Om^2 = omega_c^2, where a few ulp would be amplified.
  synthesis      |gpu - model| <= 2^-23 |model| + 1e-12 max|A|: one fp32 rounding on each side plus the fp64 phase error.
Every check prints its measured figure with `pytest -s`.  On an MI355X: the amplitudes of all 672 (case, channel) checks
are bit-identical to the model (-ffp-contract=off, the same operations in the same order); the frames sit at 0.48 - 0.50
of their bound (the model is not rounded to fp32); the files of the end-to-end test equal the model's files."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cases  # noqa: E402
from tests import field_model as M  # noqa: E402

K = np.array([0.9, 1.4, 2.1])
# phase speeds of the three modes; the middle one is leaky (W above every exterior speed)
W = {"CDC_w095_kink": (3.3, 5.5, 4.1), "CF_flow_kink": (3.3, 5.5, 4.1), "CF_flow_sausage": (3.3, 5.5, 4.1),
     "CR_kink": (1.3, 1.7, 1.38)}
ALL = list(M.VAR_NAMES)


def _problem(ctx, name, N):
    from eigensolver_amd import ShootProblem
    eq, mode, m, _ = cases.all_cases()[name]
    return ShootProblem(dataclasses.replace(eq, r_sign=1.0, n_nodes=N), mode, m, ctx=ctx)


def _np(d):
    return {a: b.cpu().numpy() for a, b in d.items()}


# ---- polarisation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 130])
@pytest.mark.parametrize("name", list(W))
def test_polarisation_matches_the_model(es_ctx, name, N):
    gp = _problem(es_ctx, name, N)
    try:
        k, w = K, K * np.array(W[name])
        d = gp.desc
        for quirks in (True, False):
            prof = gp.field_profiles(quirks)
            for n_ext in (2, 65):
                e = _np(gp.eigenfunction(k, w, n_ext=n_ext))
                p = _np(gp.polarisation(k, w, n_ext=n_ext, reference_quirks=quirks))
                assert p["radius"].shape == (3, N + n_ext) and p["amp"].shape == (3, 7, N + n_ext)
                for i in (0, 2):
                    dist = M.resonance_distance(k[i], w[i], d.m, prof)
                    assert dist > 1e-3, (name, i, dist)
                    radius, amp = M.polarisation(k[i], w[i], e["value_int"][i], e["flux_int"][i], e["x_ext"][i],
                                                 e["value_ext"][i], e["flux_ext"][i], prof, d.m, d.rho_e, d.vA_e, d.c_e,
                                                 d.cT_e, reference=quirks)
                    assert np.array_equal(p["radius"][i], radius)
                    assert np.all(np.isfinite(amp)), "the model itself is not finite at this pair"
                    for c, ch in enumerate(M.AMP_NAMES):
                        scale = np.max(np.abs(amp[c]))
                        err = np.max(np.abs(p["amp"][i, c] - amp[c]))
                        print(f"pol {name} N={N} n_ext={n_ext} quirks={quirks} mode {i} {ch:6s} err {err:.3e} "
                              f"bound {1e-10 * scale:.3e}")
                        assert err <= 1e-10 * scale, (name, N, n_ext, quirks, i, ch, err, scale)
                # the leaky mode: NaN amplitudes, its radius row written, the neighbours bit-identical to a call without it
                assert np.all(np.isnan(e["value_int"][1]))
                assert np.all(np.isnan(p["amp"][1]))
                assert np.array_equal(p["radius"][1][:N], prof["r"][::-1]) and np.all(np.isfinite(p["radius"][1]))
                assert np.array_equal(p["radius"][1][N:], e["x_ext"][1][::-1])
                p2 = _np(gp.polarisation(k[[0, 2]], w[[0, 2]], n_ext=n_ext, reference_quirks=quirks))
                assert np.array_equal(p2["amp"].view(np.uint64), p["amp"][[0, 2]].view(np.uint64))
                assert np.array_equal(p2["radius"], p["radius"][[0, 2]])
    finally:
        gp.close()


def test_polarisation_argument_errors_and_empty_calls(es_ctx):
    import torch
    from eigensolver_amd import _lib
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    N, n_ext, n = 3, 2, 2
    z = lambda *s: torch.ones(s, dtype=torch.float64, device=dev)            # noqa: E731
    k, w, iv, ifl, ex, ev, ef = z(n), z(n), z(n, N), z(n, N), z(n, n_ext), z(n, n_ext), z(n, n_ext)
    prof = {a: z(N) for a in _lib._FIELD_PROFILE_FIELDS}
    fp = _lib.FieldProfiles(*[prof[a].data_ptr() for a in _lib._FIELD_PROFILE_FIELDS])
    radius = torch.full((n, N + n_ext), -7.0, dtype=torch.float64, device=dev)
    amp = torch.full((n, 7, N + n_ext), -7.0, dtype=torch.float64, device=dev)
    P = _lib.ptr

    def call(n_=n, N_=N, n_ext_=n_ext, k_=P(k), iv_=P(iv), ex_=P(ex), fp_=C.byref(fp), m=1, flags=0, rad=P(radius), amp_=P(amp)):
        return lib.es_cyl_polarisation(h, k_, P(w), n_, N_, iv_, P(ifl), n_ext_, ex_, P(ev), P(ef), fp_, m, 0.2, 5.0, 0.5,
                                       0.49, flags, rad, amp_)
    for bad in (dict(n_=-1), dict(N_=-1), dict(n_ext_=-1), dict(k_=None), dict(iv_=None), dict(ex_=None), dict(fp_=None),
                dict(m=-1), dict(flags=8), dict(rad=None), dict(amp_=None)):
        assert call(**bad) == 1, bad
    fp_bad = _lib.FieldProfiles(*[prof[a].data_ptr() for a in _lib._FIELD_PROFILE_FIELDS])
    fp_bad.qc = None
    assert call(fp_=C.byref(fp_bad)) == 1
    assert b"invalid argument" in lib.es_last_error(h)
    assert call(n_=0, k_=None, rad=None, amp_=None) == 0                     # n == 0: a successful no-op
    assert call(N_=0, n_ext_=0) == 0
    es_ctx.synchronize()
    assert bool((radius == -7.0).all()) and bool((amp == -7.0).all())
    assert call() == 0
    es_ctx.synchronize()
    assert bool((radius != -7.0).all()) and bool((amp != -7.0).all())


# ---- synthesis ----------------------------------------------------------------------------------------------------
def _table(n_r, seed):
    rng = np.random.default_rng(seed)
    radius = np.sort(rng.uniform(0.01, 4.0, n_r))
    amp = rng.normal(size=(7, n_r)) * np.array([1.0, 3.0, 0.2, 10.0, 2.0, 5.0, 0.5])[:, None]
    return radius, amp


def _mesh(seed):
    rng = np.random.default_rng(seed)
    theta = np.linspace(0.0, 2.0 * np.pi, 7)
    z = np.sort(rng.uniform(0.0, 5.0, 3))
    t = np.array([0.01, 1.7])
    return theta, z, t


def _check(tag, got, model, amp):
    bound = M.synthesis_bound(model, amp)
    err = np.abs(got.astype(np.float64) - model)
    worst = np.max(err / bound)
    print(f"syn {tag}: max |gpu - model| / bound = {worst:.3f}")
    assert np.all(err <= bound), (tag, worst)


@pytest.mark.parametrize("n_r", [1, 5, 64, 257])
def test_synthesis_matches_the_model(es_ctx, n_r):
    import torch
    from eigensolver_amd import _lib, shooting
    dev = f"cuda:{es_ctx.device}"
    radius, amp = _table(n_r, n_r)
    theta, z, t = _mesh(11)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)        # noqa: E731
    d_radius, d_amp, d_theta, d_z, d_t = T(radius), T(amp), T(theta), T(z), T(t)
    k, w = 1.3, 3.7
    masks = [["v_phi"], ["xi_z"], ["xi_x", "v_y", "v_z"], ALL]
    for m in (0, 1, 2):
        for mask in masks:
            for zref in (False, True):
                v_scale = 25.0 if zref else 0.5
                flags = _lib.FIELD_Z_REFERENCE_ANGLE if zref else 0
                model, pts_model, names = M.synthesis(radius, amp, m, k, w, theta, z, t, mask, v_scale, zref)
                want_points = (m == 1)
                out, pts, got_names = shooting.field_synthesis(es_ctx, d_radius, d_amp, m, k, w, d_theta, d_z, d_t, mask,
                                                               v_scale, flags, want_points=want_points)
                assert got_names == names and out.shape == model.shape
                _check(f"n_r={n_r} m={m} {'+'.join(mask) if len(mask) < 4 else 'all'} zref={zref}", out.cpu().numpy(), model,
                       amp)
                if want_points:
                    p = pts.cpu().numpy().astype(np.float64)
                    assert np.all(np.abs(p - pts_model) <= 2.0 ** -23 * np.abs(pts_model) + 1e-15)
                else:
                    assert pts is None
    # an output that starts 4 bytes past a 16-byte boundary, sentinels on both sides
    model, _, names = M.synthesis(radius, amp, 1, k, w, theta, z, t, ALL, 3.0, False)
    total = model.size
    buf = torch.full((total + 12,), -777.0, dtype=torch.float32, device=dev)
    off = (((4 - buf.data_ptr() % 16) % 16) // 4) % 4 + 4                    # data_ptr of buf[off] = 4 mod 16
    out = buf[off:off + total].view(model.shape)
    assert out.data_ptr() % 16 == 4
    shooting.field_synthesis(es_ctx, d_radius, d_amp, 1, k, w, d_theta, d_z, d_t, ALL, 3.0, 0, want_points=False, out=out)
    _check(f"n_r={n_r} offset output", out.cpu().numpy(), model, amp)
    assert bool((buf[:off] == -777.0).all()) and bool((buf[off + total:] == -777.0).all())
    ref, _, _ = shooting.field_synthesis(es_ctx, d_radius, d_amp, 1, k, w, d_theta, d_z, d_t, ALL, 3.0, 0, want_points=False)
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32))          # 16-byte and 4-byte stores: the same bits


def test_big_endian_is_the_byte_swapped_result(es_ctx):
    import torch
    from eigensolver_amd import _lib, shooting
    dev = f"cuda:{es_ctx.device}"
    radius, amp = _table(37, 2)
    theta, z, t = _mesh(3)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)        # noqa: E731
    args = (es_ctx, T(radius), T(amp), 2, 0.8, 2.9, T(theta), T(z), T(t), ALL, 2.0)
    le, ple, _ = shooting.field_synthesis(*args, flags=0)
    be, pbe, _ = shooting.field_synthesis(*args, flags=_lib.FIELD_BIG_ENDIAN)
    for a, b in ((le, be), (ple, pbe)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(b.view(">f4").astype("<f4").view(np.uint32), a.view(np.uint32))


def test_synthesis_argument_errors_and_empty_meshes(es_ctx):
    import torch
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    n_r, n_th, n_z, n_t = 5, 3, 2, 2
    d = lambda n: torch.ones(max(n, 1), dtype=torch.float64, device=dev)     # noqa: E731
    radius, amp, theta, z, t = d(n_r), d(7 * n_r), d(n_th), d(n_z), d(n_t)
    out = torch.full((n_t * 11 * n_z * n_th * n_r,), -5.0, dtype=torch.float32, device=dev)
    pts = torch.full((n_z * n_th * n_r * 3,), -5.0, dtype=torch.float32, device=dev)
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None        # noqa: E731

    def call(rad=radius, amp_=amp, n_r_=n_r, m=1, th=theta, n_th_=n_th, z_=z, n_z_=n_z, t_=t, n_t_=n_t, mask=0x7ff, flags=0,
             pts_=pts, out_=out, out_off=0):
        po = C.c_void_p(out_.data_ptr() + out_off) if out_ is not None else None
        return lib.es_cyl_field_synthesis(h, P(rad), P(amp_), n_r_, m, 1.0, 2.0, P(th), n_th_, P(z_), n_z_, P(t_), n_t_,
                                          mask, 1.0, flags, P(pts_), po)
    for bad in (dict(mask=0), dict(mask=1 << 11), dict(n_r_=-1), dict(n_th_=-1), dict(n_z_=-1), dict(n_t_=-1), dict(m=-1),
                dict(flags=1), dict(flags=8), dict(rad=None), dict(amp_=None), dict(th=None), dict(z_=None), dict(t_=None),
                dict(out_=None), dict(out_off=2)):
        assert call(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)
    for empty in (dict(n_t_=0, pts_=None), dict(n_r_=0), dict(n_t_=0, pts_=None, t_=None, out_=None),
                  dict(n_r_=0, rad=None, amp_=None, out_=None, pts_=None)):
        assert call(**empty) == 0, empty
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((pts == -5.0).all())
    assert call(n_t_=0) == 0                                                 # no frames, the points alone
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((pts != -5.0).all())
    assert call() == 0
    es_ctx.synchronize()
    assert bool((out != -5.0).all())


# ---- the Python layer, end to end ------------------------------------------------------------------------------------
def test_fields_reject_slabs_and_negative_radii(es_ctx):
    from eigensolver_amd import ShootProblem
    eq, mode, m, _ = cases.all_cases()["SD_w15_kink"]
    slab = ShootProblem(dataclasses.replace(eq, n_nodes=11), mode, m, ctx=es_ctx)
    eq, mode, m, _ = cases.all_cases()["CF_flow_kink"]
    neg = ShootProblem(dataclasses.replace(eq, n_nodes=11), mode, m, ctx=es_ctx)
    try:
        for gp, word in ((slab, "cylinders only"), (neg, "r_sign=+1")):
            with pytest.raises(ValueError, match=word.replace("+", r"\+")):
                gp.polarisation([1.0], [3.3], n_ext=4)
            with pytest.raises(ValueError, match=word.replace("+", r"\+")):
                gp.fields(1.0, 3.3, [0.0, 1.0], [0.0], [0.0])
        pos = _problem(es_ctx, "CF_flow_kink", 11)
        with pytest.raises(ValueError, match="unknown field variable"):
            pos.fields(1.0, 3.3, [0.0, 1.0], [0.0], [0.0], variables=["density"])
        with pytest.raises(ValueError, match="one root"):
            pos.fields([1.0, 1.1], [3.3, 3.4], [0.0, 1.0], [0.0], [0.0])
        pos.close()
    finally:
        slab.close()
        neg.close()


@pytest.fixture(scope="module")
def cf_root(es_ctx):
    """CF_flow_kink on positive radii, 130 nodes, and one accepted root of its grid search."""
    gp = _problem(es_ctx, "CF_flow_kink", 130)
    k = np.array([1.1])
    Wv = 2.7 + (np.arange(96) + 0.5) * (4.95 - 2.7) / 96
    D, st = gp.eval_grid(k, Wv)
    roots, _ = gp.find_roots(k, Wv, D, st, n_bisect=40, tol_percent=1e-3)
    ok = roots["flag"].cpu().numpy() == 1
    assert ok.any(), "no accepted root in the window"
    yield gp, float(roots["k"].cpu().numpy()[ok][0]), float(roots["w"].cpu().numpy()[ok][0])
    gp.close()


def _read_vtk(path, names):
    """dims, points [n, 3] and {name: [n]} of a file written by write_vtk / write_vtk_packed, as float32."""
    raw = open(path, "rb").read()
    head = raw.index(b"POINTS ")
    dims = [int(v) for v in raw[raw.index(b"DIMENSIONS"):head].split()[1:4]]
    n = dims[0] * dims[1] * dims[2]
    pos = raw.index(b"\n", head) + 1
    pts = np.frombuffer(raw, dtype=">f4", count=3 * n, offset=pos).astype(np.float32).reshape(n, 3)
    pos += 12 * n
    out = {}
    for name in names:
        tag = ("\nSCALARS %s float \nLOOKUP_TABLE default \n" % name).encode()
        assert raw[pos:].startswith(tag) or raw[pos:].startswith(b"\nPOINT_DATA"), raw[pos:pos + 40]
        pos = raw.index(tag, pos) + len(tag)
        out[name] = np.frombuffer(raw, dtype=">f4", count=n, offset=pos).astype(np.float32)
        pos += 4 * n
    assert pos == len(raw)
    return dims, pts, out


def test_root_to_vtk_files(es_ctx, cf_root, tmp_path):
    from eigensolver_amd import postprocess
    gp, k, w = cf_root
    theta, z, t = np.linspace(0.0, 2.0 * np.pi, 7), np.array([0.01, 1.2, 5.0]), np.array([0.01, 0.9])
    names = ["xi_r", "P_T", "xi_x", "v_y", "v_z"]
    n_ext = 20
    f = gp.fields(k, w, theta, z, t, variables=names, v_scale=25.0, big_endian=True, n_ext=n_ext)
    files = postprocess.write_vtk_frames(str(tmp_path / "cf_kink_0"), f)
    assert files == [str(tmp_path / "cf_kink_0") + f"{i}.vtk" for i in range(2)]
    # the model's arrays from the same amplitude table, written by write_vtk
    pol = _np(gp.polarisation([k], [w], n_ext=n_ext))
    radius, amp = pol["radius"][0], pol["amp"][0]
    assert np.all(np.isfinite(amp))
    model, pts_model, order = M.synthesis(radius, amp, gp.desc.m, k, w, theta, z, t, names, 25.0, True)
    assert order == f["names"]
    n_r = radius.size
    assert n_r == 130 + n_ext
    to_xyz = lambda a: np.transpose(a, (2, 1, 0))                            # [z, theta, r] -> (n_r, n_theta, n_z)  # noqa: E731
    for i, path in enumerate(files):
        ref = postprocess.write_vtk(tmp_path / f"model_{i}", to_xyz(pts_model[..., 0]), to_xyz(pts_model[..., 1]),
                                    to_xyz(pts_model[..., 2]), [to_xyz(model[i, j]) for j in range(len(order))], order)
        dims, pts, got = _read_vtk(path, order)
        dims_m, pts_m, want = _read_vtk(ref, order)
        assert dims == dims_m == [n_r, 7, 3]
        assert np.all(np.abs(pts.astype(np.float64) - pts_m) <= 2.0 ** -23 * np.abs(pts_m) + 1e-15)
        for j, v in enumerate(order):
            exact = to_xyz(model[i, j]).ravel(order="F")
            bound = M.synthesis_bound(exact, amp)
            err = np.abs(got[v].astype(np.float64) - want[v].astype(np.float64))
            print(f"vtk frame {i} {v:5s}: max |file - model file| / bound = {np.max(err / bound):.3f}")
            assert np.all(err <= bound), (i, v)


def test_chunked_frames_equal_the_one_call_result(es_ctx, cf_root):
    import torch
    gp, k, w = cf_root
    theta, z, t = np.linspace(0.0, 2.0 * np.pi, 7), np.array([0.01, 1.2, 5.0]), np.linspace(0.01, 2.0, 5)
    one = gp.fields(k, w, theta, z, t, n_ext=20)
    chunks = list(gp.fields(k, w, theta, z, t, n_ext=20, frames_per_call=2))
    assert [c["frames"].shape[0] for c in chunks] == [2, 2, 1]
    frames = torch.cat([c["frames"] for c in chunks])
    assert torch.equal(frames.view(torch.int32), one["frames"].view(torch.int32))
    assert all(torch.equal(c["points"].view(torch.int32), one["points"].view(torch.int32)) for c in chunks)
    assert torch.equal(torch.cat([c["t"] for c in chunks]), one["t"])
    assert one["names"] == ALL and torch.equal(one["v_z"], one["frames"][:, ALL.index("v_z")])

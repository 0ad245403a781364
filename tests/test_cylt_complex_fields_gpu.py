"""es_cyl_complex_polarisation / es_cyl_complex_field_synthesis on the arrays of es_cylt_complex_eigenfunction (C ABI section
19) and RotatingCylinderComplex.polarisation / .fields: the growing movie of an unstable rotating-tube mode.  The twisted
family is the first caller with v_phi (and s_phi) in the profiles, so the T, Q, g and s_phi terms of section 7's formulas take
part with complex Om.  (B_phi stays zero: equilibrium.CylinderRotation has no azimuthal field.)

Amplitudes against tests/field_model.polarisation on the GPU's own eigenfunction arrays, every channel within 1e-10 of its
maximum; on the real axis ShootProblem.polarisation at 1e-10.  Frames against the model's synthesis
(tests/cyl_complex_eigen_model.synthesis) on the GPU's own amplitude table under cyl_complex_eigen_model.synthesis_bound; chunked
and big-endian calls compare bits.  CylinderComplex.fields, whose methods moved to the shared base, against field_synthesis
called directly: the same bits."""
import numpy as np
import pytest

from tests import cyl_complex_eigen_model as cem
from tests import cylt_complex_eigen_model as tem

pytestmark = pytest.mark.gpu

THETA = np.linspace(0.0, 2.0 * np.pi, 5)
Z = np.array([0.0, 0.45, 1.3, 2.2])
T = np.array([0.2, 0.9, 1.9])
AMP = cem.AMP_NAMES


def _np(d):
    return {a: (v.cpu().numpy() if hasattr(v, "cpu") else v) for a, v in d.items()}


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def solver(es_ctx, name, n_nodes=130):
    from eigensolver_amd import RotatingCylinderComplex
    eq, mode, m, _, _, _ = tem.problems(n_nodes)[name]
    return RotatingCylinderComplex(eq, ctx=es_ctx), mode, m


@pytest.mark.parametrize("name", ["A", "sausage", "reference"])
def test_polarisation_against_model(es_ctx, name):
    E = tem.model_of(name, 130)
    c, mode, m = solver(es_ctx, name)
    k, w = tem.pairs(name, 130, 16)
    ok = E.M.eval_points(k, w)[4] == 0
    k, w = k[ok][:6], w[ok][:6]
    assert len(k) == 6 and (w.imag > 0).any() and (w.imag < 0).any()
    prof = E.profiles()
    # the terms the untwisted family never exercised.  CylinderRotation, the project's one twisted equilibrium, has B_phi = 0
    # by construction (CR-KF:176-189): it is v_phi, and s_phi where power != 1, that make T, Q, g and s_phi non-zero
    assert np.all(prof["vphi"] != 0.0) and np.all(prof["Bphi"] == 0.0)
    assert np.any(prof["s_phi"] != 0.0) == (name != "A")
    eig = _np(c.eigenfunction(mode, k, w, n_ext=16, m=m))
    pol = _np(c.polarisation(mode, k, w, n_ext=16, m=m))
    c.close()
    assert np.all(pol["status"] == 0) and pol["amp"].shape == (6, 7, 146) and pol["amp"].dtype == np.complex128
    radius_m, amp_m = E.polarisation(k, w, eig)
    assert np.array_equal(pol["radius"], radius_m)
    assert np.all(pol["radius"][:, 129] == 1.0) and np.all(pol["radius"][:, 130] == 1.0)      # the boundary radius twice
    scale = np.max(np.abs(amp_m), axis=2, keepdims=True)
    err = np.max(np.abs(pol["amp"] - amp_m) / scale, axis=(0, 2))
    print(f"{name}: max |amp - model| / max|channel| per channel: " + ", ".join(f"{a} {e:.2e}" for a, e in zip(AMP, err)))
    for ch in ("xi_phi", "xi_z", "v_phi", "v_z"):                              # non-trivially complex: both parts take part
        a = pol["amp"][:, AMP.index(ch), :130]
        top = np.max(np.abs(a), axis=1)
        assert np.all(top > 0.0), ch
        assert np.all(np.max(np.abs(a.real), axis=1) > 1e-3 * top) and np.all(np.max(np.abs(a.imag), axis=1) > 1e-3 * top), ch
    assert np.max(err) < 1e-10


@pytest.mark.parametrize("name", ["sausage", "reference"])
def test_real_axis_is_section_7(es_ctx, name):
    """Im omega = 0: the amplitudes of ShootProblem.polarisation times sign(P_e(boundary)), no imaginary part."""
    c, mode, m = solver(es_ctx, name)
    p = c.problem(mode, m)
    _, _, _, _, W, _ = tem.problems(130)[name]
    k = np.repeat(np.array([0.7, 1.1, 1.9]), 12)
    w = k * np.tile(np.linspace(W[0], W[1], 12), 3)
    ok = (p.eval_points(k, w)[1].cpu().numpy() == 0) & (c.eval_points(mode, k, w + 0j, m=m)[1].cpu().numpy() == 0)
    assert ok.sum() >= 8
    k, w = k[ok], w[ok]
    sign = np.sign(_np(p.eigenfunction(k, w, n_ext=9))["value_ext"][:, -1])[:, None, None]
    polr = _np(p.polarisation(k, w, n_ext=9))
    polc = _np(c.polarisation(mode, k, w + 0j, n_ext=9, m=m))
    c.close()
    assert np.array_equal(polc["radius"], polr["radius"])
    scale = np.max(np.abs(polr["amp"]), axis=2, keepdims=True)
    err = float(np.max(np.abs(polc["amp"].real - sign * polr["amp"]) / scale))
    im = float(np.max(np.abs(polc["amp"].imag) / scale))
    print(f"{name}: max |Re amp - sign * section 7| / max|channel| = {err:.3e} (bound 1e-10), max |Im amp| = {im:.3e} "
          "(bound 1e-13)")
    assert err <= 1e-10 and im <= 1e-13


@pytest.fixture(scope="module")
def root_a(es_ctx):
    """RotatingCylinderComplex of case A at N = 130 and its unstable m = 3 root at k = 1, polished by Newton's iteration."""
    c, mode, m = solver(es_ctx, "A")
    k, w0 = tem.ROOT_A
    r = c.newton(mode, [k], [w0], m=m)
    w = complex(r["w"].cpu().numpy()[0])
    assert int(r["flag"].cpu().numpy()[0]) == 1 and abs(w - w0) < 1e-6
    yield c, mode, m, k, w
    c.close()


def test_fields_of_the_unstable_root(root_a):
    c, mode, m, k, w = root_a
    pol = _np(c.polarisation(mode, [k], [w], n_ext=16, m=m))
    assert pol["status"][0] == 0
    radius, amp = pol["radius"][0], pol["amp"][0]
    full = c.fields(mode, k, w, THETA, Z, T, v_scale=3.0, n_ext=16, m=m)
    got = full["frames"].cpu().numpy().astype(np.float64)
    model, names = cem.synthesis(radius, amp, m, k, w, THETA, Z, T, v_scale=3.0, z_reference_angle=True)
    assert names == full["names"] and got.shape == model.shape == (3, 11, 4, 5, 146)
    bnd = cem.synthesis_bound(model, names, amp, 3.0, w, T)
    print(f"case A root w = {w:.7f}: max |frames - model| / bound = {float(np.max(np.abs(got - model) / bnd)):.3f}")
    assert np.all(np.abs(got - model) <= bnd)
    assert np.exp(w.imag * (T[-1] - T[0])) > 2.0                             # the movie grows
    # chunked: the same bits, the points produced once
    chunks = list(c.fields(mode, k, w, THETA, Z, T, v_scale=3.0, n_ext=16, m=m, frames_per_call=2))
    assert [ch["frames"].shape[0] for ch in chunks] == [2, 1] and all(ch["points"] is chunks[0]["points"] for ch in chunks)
    assert np.array_equal(np.concatenate([_bits(ch["frames"]) for ch in chunks]), _bits(full["frames"]))
    assert np.array_equal(_bits(chunks[0]["points"]), _bits(full["points"]))
    # big-endian: the byte swap of the little-endian run, points included
    be = list(c.fields(mode, k, w, THETA, Z, T, v_scale=3.0, n_ext=16, m=m, frames_per_call=2, big_endian=True))
    be_frames = np.concatenate([ch["frames"].cpu().numpy() for ch in be])
    assert np.array_equal(be_frames.view(">f4").astype("<f4").view(np.uint32), _bits(full["frames"]))
    assert np.array_equal(be[0]["points"].cpu().numpy().view(">f4").astype("<f4").view(np.uint32), _bits(full["points"]))


def test_fields_to_vtk_files(root_a, tmp_path):
    """The README's usage line: fields(..., big_endian=True) into write_vtk_frames."""
    from eigensolver_amd import postprocess
    c, mode, m, k, w = root_a
    f = c.fields(mode, k, w, THETA, Z, T[:2], variables=["xi_r", "v_phi"], m=m, n_ext=16, big_endian=True)
    files = postprocess.write_vtk_frames(str(tmp_path / "tube_m3_"), f)
    assert len(files) == 2
    raw = open(files[0], "rb").read()
    assert b"DIMENSIONS  146 5 4" in raw and b"SCALARS v_phi float" in raw


def test_untwisted_fields_are_what_they_were(es_ctx):
    """CylinderComplex.fields after its methods moved to the shared base: the bits of field_synthesis called directly on the
    amplitudes of polarisation, as fields() composed them before."""
    from eigensolver_amd import CylinderComplex, _lib
    from eigensolver_amd.cyl_complex import CylinderEigenfunctions
    mode, k, w = cem.JET_ROOTS[1]
    c = CylinderComplex(cem.jet(130), ctx=es_ctx)
    assert CylinderComplex.fields is CylinderEigenfunctions.fields
    f = c.fields(mode, k, w, THETA, Z, T, v_scale=3.0, n_ext=30)
    pol = c.polarisation(mode, [k], [w], n_ext=30)
    p = c.problem(mode)
    dth, dz, dt = (p._dev(a) for a in (THETA, Z, T))
    out, pts, names = c.field_synthesis(pol["radius"][0], pol["amp"][0], 1, k, w, dth, dz, dt, None, 3.0,
                                        _lib.FIELD_Z_REFERENCE_ANGLE)
    c.close()
    assert names == f["names"]
    assert np.array_equal(_bits(out), _bits(f["frames"])) and np.array_equal(_bits(pts), _bits(f["points"]))

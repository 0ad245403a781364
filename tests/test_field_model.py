"""CPU checks of the perturbation-field feature (include/eigensolver_amd.h section 7): the NumPy model of
tests/field_model.py against the export scripts' own arrays, the quirk-free limit, and the packed VTK writers.

Fixtures tests/golden/fields_{CDC,CF,CR}.npz are written by tools/gen_golden_fields.py from the text of the three export
scripts (all three slices run under the harness).  Bound of the fixture test: both sides are the same fp64 expressions
in the same order, 1e-13 of the channel's max; the one departure -- omega_A^2, omega_c^2 from bA and qc instead of
:622-630 -- costs a few ulp of omega_A^2 divided by the relative distance to the resonance, which is asserted >= 1e-3."""
import os

import numpy as np
import pytest

from eigensolver_amd import equilibrium as q, postprocess, shooting
from tests import field_model as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["CDC", "CF", "CR"])
def test_model_reproduces_the_export_scripts(name):
    g = np.load(os.path.join(G, f"fields_{name}.npz"))
    eq = M.fixture_equilibrium(name, len(g["ix"]))
    for c in ("rho_e", "vA_e", "c_e", "cT_e", "c_i0", "vA_i0"):
        assert float(g[c]) == pytest.approx(getattr(eq, c), rel=1e-15), c
    assert g["ix"][0] == 1.0 and g["ix"][-1] == eq.r_axis and g["lx"][-1] == 1.0
    k, w, m = float(g["k"]), float(g["w"]), int(g["m"])
    prof = shooting.field_profiles(eq, g["ix"], reference_quirks=True)
    dist = M.resonance_distance(k, w, m, prof)
    print(f"{name}: k = {k} w = {w} resonance distance {dist:.3e}")
    assert dist > 1e-3
    radius, amp = M.polarisation(k, w, g["inside_P_solution"], g["inside_xi_solution"], g["lx"], g["left_P_solution"],
                                 g["left_xi_solution"], prof, m, eq.rho_e, eq.vA_e, eq.c_e, eq.cT_e, reference=True)
    assert np.array_equal(radius, g["spatial"])
    for c, ch in enumerate(M.AMP_NAMES):
        ref = g["radial_" + ch]
        err = np.max(np.abs(amp[c] - ref))
        scale = np.max(np.abs(ref))
        print(f"  {ch:7s} max|model - script| = {err:.3e}  max|script| = {scale:.3e}  ratio {err / scale if scale else 0.0:.2e}")
        assert err <= 1e-13 * scale, (name, ch, err, scale)


def test_uniform_cylinder_without_quirks_reduces_to_the_exterior_forms():
    """width = 1e5, no twist, no flow, quirks off: the interior xi_phi and xi_z are the exterior's closed forms with the
    interior constants, xi_phi = (m P/r)/(rho_i (w^2 - k^2 vA_i^2)), xi_z = k c_i^2 P/(rho_i (w^2 - k^2 cT_i^2)(c_i^2 + vA_i^2))."""
    eq = q.CylinderFlow(width=1e5, U_i0=0.0, r_sign=1.0, n_nodes=40)
    r = np.linspace(eq.x_boundary, eq.x_end, eq.n_nodes)
    prof = shooting.field_profiles(eq, r, reference_quirks=False)
    rng = np.random.default_rng(7)
    P, xi = rng.normal(size=r.size), rng.normal(size=r.size)
    ext_x = np.linspace(4.0, 1.0, 9)
    eP, exi = rng.normal(size=9), rng.normal(size=9)
    k, w, m = 1.3, 3.3, 2
    radius, amp = M.polarisation(k, w, P, xi, ext_x, eP, exi, prof, m, eq.rho_e, eq.vA_e, eq.c_e, eq.cT_e, reference=False)
    N = r.size
    A = dict(zip(M.AMP_NAMES, amp))
    Pr, rr = P[::-1], r[::-1]
    c2, vA2, rho = eq.c_i0 ** 2, eq.vA_i0 ** 2, eq.rho_i0
    xi_phi = (m * Pr / rr) / (rho * (w ** 2 - k ** 2 * vA2))
    xi_z = k * c2 * Pr / (rho * (w ** 2 - k ** 2 * eq.cT_i0 ** 2) * (c2 + vA2))
    assert np.max(np.abs(A["xi_phi"][:N] - xi_phi)) <= 1e-13 * np.max(np.abs(xi_phi))
    assert np.max(np.abs(A["xi_z"][:N] - xi_z)) <= 1e-13 * np.max(np.abs(xi_z))
    assert np.array_equal(A["v_r"][:N], -w * xi[::-1]) and np.array_equal(A["v_phi"][:N], -(w * A["xi_phi"][:N]))
    # the exterior with the same formulas and its own constants; with the flag the factor w^2 of Export_vtk.py:781
    ex = (m * eP[::-1] / ext_x[::-1]) / (eq.rho_e * (w ** 2 - k ** 2 * eq.vA_e ** 2))
    assert np.allclose(A["xi_phi"][N:], ex, rtol=1e-14, atol=0)
    _, amp_ref = M.polarisation(k, w, P, xi, ext_x, eP, exi, prof, m, eq.rho_e, eq.vA_e, eq.c_e, eq.cT_e, reference=True)
    assert np.allclose(amp_ref[2][N:], w ** 2 * A["xi_z"][N:], rtol=1e-14, atol=0)
    assert np.array_equal(radius, np.concatenate((rr, ext_x[::-1])))


def test_equilibrium_shear_derivatives_match_finite_differences():
    r = np.linspace(1.0, 0.05, 7)
    h = 1e-6
    for eq in (q.CylinderFlow(U_i0=0.6, width=1.0, r_sign=1.0), q.CylinderRotation(v_twist=0.25, power=0.8),
               q.CylinderDensity(r_sign=1.0)):
        fd = lambda f: (f(r + h) - f(r - h)) / (2 * h)                       # noqa: E731
        assert np.allclose(eq.dv_z_dr(r), fd(eq.v_z), rtol=1e-6, atol=1e-9)
        assert np.allclose(eq.dv_z_over_r_dr(r), fd(lambda x: eq.v_z(x) / x), rtol=1e-6, atol=1e-9)
        assert np.allclose(eq.dv_phi_over_r_dr(r), fd(lambda x: eq.v_phi(x) / x), rtol=1e-6, atol=1e-9)


def test_write_vtk_packed_is_byte_identical_to_write_vtk(tmp_path):
    rng = np.random.default_rng(3)
    shape = (3, 4, 2)
    x, y, z, a, b = (rng.normal(size=shape) for _ in range(5))
    f1 = postprocess.write_vtk(tmp_path / "plain", x, y, z, [a, b], ["xi_r", "P_T"])
    pack = lambda v: v.astype(">f4").ravel(order="F")                        # noqa: E731
    pts = np.empty((x.size, 3), dtype=">f4")                                 # np.stack would return native byte order
    pts[:, 0], pts[:, 1], pts[:, 2] = pack(x), pack(y), pack(z)
    f2 = postprocess.write_vtk_packed(tmp_path / "packed", shape, pts.tobytes(), [pack(a).tobytes(), pack(b)],
                                      ["xi_r", "P_T"])
    assert open(f1, "rb").read() == open(f2, "rb").read()
    import torch
    as_u8 = lambda v: torch.from_numpy(np.frombuffer(v.tobytes(), dtype=np.uint8).copy())   # noqa: E731
    f3 = postprocess.write_vtk_packed(tmp_path / "packed_t", shape, as_u8(pts), [as_u8(pack(a)), as_u8(pack(b))],
                                      ["xi_r", "P_T"])
    assert open(f1, "rb").read() == open(f3, "rb").read()
    with pytest.raises(ValueError):
        postprocess.write_vtk_packed(tmp_path / "bad", shape, pts.tobytes()[:-4], [], [])


def test_write_vtk_frames_names_the_files_by_frame_number(tmp_path):
    import torch
    n_r, n_th, n_z = 3, 4, 2
    rng = np.random.default_rng(5)

    def chunk(n_t):
        fr = torch.from_numpy(rng.normal(size=(n_t, 2, n_z, n_th, n_r)).astype(np.float32))
        return dict(points=torch.zeros((n_z, n_th, n_r, 3)), names=["xi_r", "v_z"], frames=fr, xi_r=fr[:, 0], v_z=fr[:, 1])
    chunks = [chunk(2), chunk(2), chunk(1)]
    prefix = str(tmp_path / "mode_0")
    files = postprocess.write_vtk_frames(prefix, iter(chunks))
    assert files == [f"{prefix}{t}.vtk" for t in range(5)]                   # Export_vtk.py:989: name + str(t)
    assert sorted(os.listdir(tmp_path)) == [f"mode_0{t}.vtk" for t in range(5)]
    body = open(files[3], "rb").read()
    assert b"DIMENSIONS  3 4 2  \n" in body and b"SCALARS xi_r float" in body and b"SCALARS v_z float" in body
    assert body.endswith(chunks[1]["v_z"][1].numpy().tobytes())
    only = postprocess.write_vtk_frames(str(tmp_path / "one_"), chunks[2], names=["v_z"])
    assert only == [str(tmp_path / "one_") + "0.vtk"] and b"xi_r" not in open(only[0], "rb").read()


def test_field_profiles_struct_and_variable_mask():
    """The ctypes mirror of es_field_profiles has the size the C compiler gave it (es_abi_sizeof index 7; 99 stays unknown),
    and the mask of the synthesis follows the header's ES_VAR_* order."""
    import ctypes
    from eigensolver_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    lib.es_abi_sizeof.restype = ctypes.c_int
    lib.es_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.es_abi_sizeof(7) == ctypes.sizeof(_lib.FieldProfiles) == 8 * len(_lib._FIELD_PROFILE_FIELDS)
    assert lib.es_abi_sizeof(8) == -1 and lib.es_abi_sizeof(99) == -1
    assert hasattr(lib, "es_cyl_polarisation") and hasattr(lib, "es_cyl_field_synthesis")
    assert _lib.VAR_NAMES == M.VAR_NAMES and _lib.AMP_NAMES == M.AMP_NAMES
    assert shooting.var_mask(None) == (0x7ff, list(M.VAR_NAMES))
    assert shooting.var_mask(["v_z", "xi_x", "v_y"]) == ((1 << 9) | (1 << 5) | (1 << 8), ["xi_x", "v_y", "v_z"])
    with pytest.raises(ValueError):
        shooting.var_mask(["density"])

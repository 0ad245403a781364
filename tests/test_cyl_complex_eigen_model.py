"""CPU pin of tests/cyl_complex_eigen_model.py, the NumPy restatement of C ABI section 16 (no GPU):
  * the model's interior against DOP853 on complex y within real_eigen_model.bound(N) of max|field| per array, at N = 130 and
    500, two pairs per problem;
  * the jump of the flux at the boundary equals D_c of tests/cyl_complex_model.py (the outward RK4 step and the determinant's
    adjoint step are transposes of each other: to rounding), the boundary values are 1, the exterior flux there is `outer`;
  * P(axis node) = target for the kink condition;
  * the sample seeds the GPU tests use leave more than half of the points OK;
  * the synthesis at w_im = 0 and real amplitudes is tests/field_model.synthesis.
The ABI-level part: the library exports the three calls of section 16 with the signatures eigensolver_amd/_lib.py declares."""
import numpy as np
import pytest

from tests import cyl_complex_eigen_model as cem
from tests import field_model
from tests.cases import truth_problem
from tests.real_eigen_model import bound


@pytest.mark.parametrize("n_nodes", [130, 500])
@pytest.mark.parametrize("name", cem.NAMES)
def test_interior_against_dop853(name, n_nodes):
    eq, mode, m, _ = cem.problems(n_nodes)[name]
    E = cem.CylComplexEigenModel(eq, mode, m)
    prob = truth_problem(eq, mode, m)
    k, w = cem.dop_pairs(name, n_nodes)
    e = E.eigenfunction(k, w, n_ext=0)
    for i in range(2):
        P, xi = E.interior_dop853(prob, k[i], w[i])
        for key, want in (("value_int", P), ("flux_int", xi)):
            err = float(np.max(np.abs(e[key][i] - want)) / np.max(np.abs(want)))
            print(f"{name} N={n_nodes} pair {i} {key}: |model - DOP853| / max = {err:.3e} (bound {bound(n_nodes):.1e})")
            assert err < bound(n_nodes)


@pytest.mark.parametrize("n_nodes", cem.NODE_COUNTS)
@pytest.mark.parametrize("name", cem.NAMES)
def test_boundary_identities_and_seeds(name, n_nodes):
    eq, mode, m, window = cem.problems(n_nodes)[name]
    E = cem.CylComplexEigenModel(eq, mode, m)
    k, w = cem.sample(window, 65, cem.seed_of(name, n_nodes))
    e = E.eigenfunction(k, w, n_ext=37)
    ok = e["status"] == 0
    assert ok.sum() > 32, ok.sum()
    assert (w.imag > 0).any() and (w.imag < 0).any() and len(np.unique(k)) == 65
    sc = np.maximum(np.abs(e["outer"][ok]), np.abs(e["inner"][ok]))
    jump = e["flux_ext"][ok, -1] - e["flux_int"][ok, 0]
    err = float(np.max(np.abs(jump - e["D"][ok]) / sc))
    print(f"{name} N={n_nodes}: max |jump of the flux - D_c| / scale = {err:.3e}")
    assert err < 1e-12
    assert np.max(np.abs(e["flux_ext"][ok, -1] - e["outer"][ok]) / sc) < 1e-13
    assert np.max(np.abs(e["value_ext"][ok, -1] - 1.0)) < 1e-13 and np.max(np.abs(e["value_int"][ok, 0] - 1.0)) < 1e-12
    assert np.all(np.abs(e["x_ext"][:, -1]) == 1.0)
    for a in ("value_int", "flux_int", "value_ext", "flux_ext"):
        assert np.all(np.isnan(e[a][~ok].real)) and np.all(np.isfinite(e[a][ok]))
    if mode == "kink":                                       # P(r_ax) = bc_const xi_e
        target = E.M.d["bc_const"] * e["outer"][ok]
        assert np.max(np.abs(e["value_int"][ok, -1] - target)) <= 1e-15 * np.max(np.abs(e["value_int"][ok]))


def test_kink_target_is_imposed_when_it_is_not_zero():
    eq, mode, m, window = cem.problems(130)["flow_kink"]
    E = cem.CylComplexEigenModel(eq, mode, m)
    E.M.d["bc_const"] = 0.37
    k, w = cem.sample(window, 8, 5)
    e = E.eigenfunction(k, w, n_ext=0)
    ok = e["status"] == 0
    assert ok.sum() >= 4
    assert np.max(np.abs(e["value_int"][ok, -1] - 0.37 * E.M.exterior(k, w)[1][ok])) < 1e-15
    jump_free = e["value_int"][ok, 0]
    assert np.max(np.abs(jump_free - 1.0)) < 1e-12


def test_synthesis_on_the_real_axis_is_section_7():
    rng = np.random.default_rng(3)
    n_r = 9
    radius, amp = np.linspace(0.1, 2.0, n_r), rng.normal(size=(7, n_r))
    th, z, t = np.linspace(0, 2 * np.pi, 5), np.array([0.0, 0.4, 1.1]), np.array([0.0, 0.7])
    for zref in (False, True):
        want, _, names = field_model.synthesis(radius, amp, 1, 1.3, 2.1, th, z, t, v_scale=2.5, z_reference_angle=zref)
        got, names_c = cem.synthesis(radius, amp + 0j, 1, 1.3, 2.1 + 0j, th, z, t, v_scale=2.5, z_reference_angle=zref)
        assert names == names_c
        assert np.max(np.abs(got - want)) < 1e-14 * np.max(np.abs(want))
    # growth: the frame at t shifted along z by Re w t / k is e^{Im w t} times the frame at 0
    w = 2.1 + 0.3j
    a, _ = cem.synthesis(radius, amp * (1 + 0.5j), 1, 1.3, w, th, z, [0.0])
    b, _ = cem.synthesis(radius, amp * (1 + 0.5j), 1, 1.3, w, th, z + w.real * 0.7 / 1.3, [0.7])
    assert np.max(np.abs(b - np.exp(0.3 * 0.7) * a)) < 1e-13 * np.max(np.abs(a))


@pytest.mark.parametrize("mode,k,w0", cem.JET_ROOTS)
def test_quoted_jet_roots_are_the_models(mode, k, w0):
    """The six digits the GPU tests hold find_roots to: the model's secant iteration from beside them, run to convergence."""
    M = cem.CylComplexEigenModel(cem.jet(130), mode).M
    w = M.secant(k, w0 + 1e-3, w0 - 1e-3j)
    assert w is not None and abs(w - w0) < 1e-6 and w.imag > 0
    assert M.eval(k, w)[3][0] < 1e-10                          # resid, percent


def test_library_exports_section_16():
    """The ABI-level part: fails without the feature."""
    from eigensolver_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name, nargs in (("es_cyl_complex_eigenfunction", 13), ("es_cyl_complex_polarisation", 21),
                        ("es_cyl_complex_field_synthesis", 19)):
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name

"""The yardstick of tests/test_complex_eigenfunction_gpu.py, pinned on the CPU: tests/complex_eigen_model.py (the NumPy
restatement of es_complex_eigenfunction) against DOP853, the uniform closed form, the far-end condition and D_c of
oracle.slab_complex.eval_rk4."""
import numpy as np
import pytest

from tests import complex_eigen_model as M

NS = [130, 500]


def _max(a):
    return np.max(np.abs(a))


@pytest.mark.parametrize("N", NS)
def test_sausage_roots_are_the_expected_pair(N):
    r = np.array(M.sausage_roots(N))
    assert len(r) >= 2
    for want in (0.000717 + 0.087469j, 0.000717 - 0.087469j):
        assert np.min(np.abs(r - want)) < 5e-5, r


@pytest.mark.parametrize("N", NS)
def test_model_vs_dop853(N):
    for name, width, mode, variant, w in M.cases(N):
        m = M.model(M.slab(width, mode, variant, N), M.K0, w)
        t = M.truth_case(N, name)
        assert np.all(m["status"] == 0) and np.all(t["status"] == 0)
        for key in ("value_int", "flux_int"):               # the exterior is the same closed form in both
            for i in range(len(w)):
                err, scale = _max(m[key][i] - t[key][i]), _max(t[key][i])
                print(N, name, key, i, err / scale)
                assert err <= M.bound(N) * scale, (name, key, i, err / scale)


@pytest.mark.parametrize("N", NS)
def test_uniform_flow_is_cosh(N):
    o = M.slab(1e5, "kink", "sfx", N)
    m = M.model(o, M.K0, [M.KH_ROOT, M.NON_ROOT], n_ext=0)
    for i, w in enumerate((M.KH_ROOT, M.NON_ROOT)):
        want = M.uniform_closed_form(o, M.K0, w, m["x_int"])
        err = _max(m["value_int"][i] - want) / _max(want)
        print(N, w, err)
        assert err <= 1e-8


@pytest.mark.parametrize("N", NS)
def test_far_end_condition_and_dc_identity(N):
    for name, width, mode, variant, w in M.cases(N):
        o = M.slab(width, mode, variant, N)
        m = M.model(o, M.K0, w, n_ext=2)
        d, rel, st = o.eval_rk4(M.K0, w)
        assert np.array_equal(st, m["status"])
        for i in range(len(w)):
            vx = m["value_int"][i]
            far = abs(vx[-1] - M.sigma(o) * vx[0]) / _max(vx)
            outer, inner = m["flux_ext"][i, -1], m["flux_int"][i, 0]
            ident = abs((outer - inner) - d[i]) / max(abs(outer), abs(inner))
            print(N, name, i, far, ident)
            assert far <= 1e-10
            assert ident <= 1e-10
            assert abs(m["value_ext"][i, -1] - 1.0) <= 1e-12
            assert abs(outer - m["outer"][i]) <= 1e-12 * abs(outer)


def test_leaky_pair_is_nan_with_status():
    o = M.slab(0.9, "kink", "sfx", 130)
    m = M.model(o, M.K0, [M.NON_ROOT, M.LEAKY, M.NON_ROOT], n_ext=3)
    assert list(m["status"]) == [0, 1, 0]
    for key in ("value_int", "flux_int", "value_ext", "flux_ext"):
        assert np.all(np.isnan(m[key][1])) and np.all(np.isfinite(m[key][[0, 2]]))
    assert np.all(np.isfinite(m["x_ext"]))

"""The NumPy yardstick of C ABI section 15 (tests/cyl_complex_slope_model.py) pinned on the CPU, before the GPU is held to it:
  * row 0 of `jets` is CylComplexModel.eval to rounding, statuses included;
  * the derivative rows against Cauchy's formula on the model itself, in omega and in a complex k, two radii;
  * d omega / dk against the slope of the model's own root curve at the three Kelvin-Helmholtz roots of DESIGN 8i;
  * on the real axis, d omega / dk against c_g of the real path's model (tests/root_slope_model.py);
  * the Newton rule on the model reaches the three roots.
Every bound is 10 x the figure recorded in the helper; `pytest -s` prints the figures of the run."""
import numpy as np
import pytest

from tests import cyl_complex_slope_model as C

ALL = C.KINDS + ("kh_w1e5", "kh_w3")


@pytest.mark.parametrize("name", ALL)
def test_row_zero_is_the_value_model(name):
    """The same scipy calls and the same operations in the same order: a few ulp (the jet division multiplies by a
    reciprocal where the model divides), bound 64 ulp = 1.4e-14 of max(|outer|, |inner|)."""
    M = C.model(name)
    pairs = list(C.NON_ROOT[name]) + ([C.LEAKY[name]] if name in C.LEAKY else [])
    k, w = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    outer, inner, st = C.jets(M, k, w)
    D, mo, mi, rel, mst = M.eval_points(k, w)
    assert st.tolist() == mst.tolist()
    assert st.tolist() == [0] * len(C.NON_ROOT[name]) + ([1] if name in C.LEAKY else [])
    assert {np.sign(z.imag) for z in w[st == 0]} == {1.0, -1.0}
    ok = st == 0
    sc = np.maximum(np.abs(mo[ok]), np.abs(mi[ok]))
    eo, ei = np.abs(outer[0][ok] - mo[ok]) / sc, np.abs(inner[0][ok] - mi[ok]) / sc
    print(f"{name}: row 0 against the value model, outer {eo.max():.2e}, inner {ei.max():.2e} (bound 1.4e-14)")
    assert eo.max() <= 1.4e-14 and ei.max() <= 1.4e-14
    assert np.isnan(outer[:, ~ok].real).all() and np.isnan(inner[:, ~ok].imag).all()
    assert np.allclose(C.rel_of(M, outer, inner)[ok], rel[ok], rtol=1e-12, atol=0.0)
    assert np.isfinite(outer[:, ok]).all() and np.isfinite(inner[:, ok]).all()


def test_derivative_rows_against_cauchy():
    worst, worst_radii = 0.0, 0.0
    for name, k, w, r in C.cauchy_pairs():
        M = C.model(name)
        outer, inner, st = C.jets(M, k, [w])
        assert st[0] == 0
        cw, ck, radii = C.cauchy_parts(M, k, w, r=r)
        ew = np.abs(np.array([outer[1, 0], inner[1, 0]]) - cw) / max(abs(outer[1, 0]), abs(inner[1, 0]))
        ek = np.abs(np.array([outer[2, 0], inner[2, 0]]) - ck) / max(abs(outer[2, 0]), abs(inner[2, 0]))
        print(f"{name} k = {k}, omega = {w:.6f}: |jets - Cauchy| d/dw {ew.max():.2e}, d/dk {ek.max():.2e}; radii {r:g} and "
              f"{0.5 * r:g} disagree by {radii:.2e}")
        worst, worst_radii = max(worst, ew.max(), ek.max()), max(worst_radii, radii)
    print(f"worst {worst:.2e} (recorded {C.CAUCHY_MEASURED:.1e}, bound 10 x); radii {worst_radii:.2e} (recorded "
          f"{C.CAUCHY_RADII_MEASURED:.1e}, bound 10 x)")
    assert worst <= 10.0 * C.CAUCHY_MEASURED
    assert worst_radii <= 10.0 * C.CAUCHY_RADII_MEASURED


def test_slope_is_the_slope_of_the_root_curve():
    for width, (M, k, root, slope) in C.slope_cases().items():
        assert abs(root - C.KH_ROOTS[width]) < 1e-6                                     # the root of the table
        outer, inner, st = C.jets(M, k, root)
        got = C.dwdk(outer, inner)[0]
        err = abs(got - slope) / max(1.0, abs(slope))
        print(f"width {width:g}: root {root:.12f}, d omega / dk = {got:.12f}, curve slope {slope:.12f}, |difference| = {err:.2e} "
              f"(recorded {C.SLOPE_MEASURED[width]:.1e}, bound 10 x)")
        assert st[0] == 0 and err <= 10.0 * C.SLOPE_MEASURED[width]


def test_real_axis_slope_is_the_real_group_speed():
    eq, mode, m, k, w, cg, s = C.real_axis_case()
    err = np.abs(s - cg) / np.maximum(1.0, np.abs(cg))
    print(f"{C.REAL_AXIS_CASE}: {len(k)} real roots, worst |d omega / dk - c_g| / max(1, |c_g|) = {err.max():.2e}, worst |Im| = "
          f"{np.abs(s.imag).max():.2e} (recorded {C.REAL_AXIS_MEASURED:.1e}, bound 10 x)")
    assert len(k) >= 5 and err.max() <= 10.0 * C.REAL_AXIS_MEASURED


def test_conjugate_symmetry_of_the_model():
    for name in C.KINDS:
        M = C.model(name)
        k, w = C.NON_ROOT[name][0]
        a = C.dwdk(*C.jets(M, k, [w])[:2])[0]
        b = C.dwdk(*C.jets(M, k, [np.conj(w)])[:2])[0]
        print(f"{name}: |d omega / dk (conj omega) - conj d omega / dk (omega)| = {abs(b - np.conj(a)):.2e}")
        assert abs(b - np.conj(a)) <= 1e-13 * max(1.0, abs(a))


def test_newton_model_reaches_the_roots():
    for width in C.KH_ROOTS:
        M, root = C.model(C.KH_NAMES[width]), C.kh_root(width)
        for sgn in (1, -1):
            r = C.newton_model(M, C.K0, root + sgn * C.NEWTON_OFFSET)
            print(f"width {width:g}, start root {'+' if sgn > 0 else '-'} 1e-3 (1 + i): {r['iters']} steps {r['steps']}, "
                  f"|w - root| = {abs(r['w'] - root):.2e}, resid {r['resid']:.1e} %")
            assert r["flag"] == 1 and r["iters"] <= 5 and abs(r["w"] - root) <= 1e-13
    M, root = C.model("kh_w15"), C.kh_root(1.5)
    r = C.newton_model(M, C.K0, root + C.NEWTON_OFFSET, max_iter=1, step_cap=1e-4)
    assert r["iters"] == 1 and abs(abs(r["w"] - root - C.NEWTON_OFFSET) - 1e-4) <= 1e-15
    r = C.newton_model(M, C.K0, root + C.NEWTON_OFFSET, max_shift=1e-4)
    assert r["flag"] == 0 and abs(r["w"] - root) <= 1e-13
    r = C.newton_model(M, *C.LEAKY["kh_w15"])
    assert r["flag"] == 0 and r["iters"] == 0 and r["status"] == 1 and np.isnan(r["resid"])

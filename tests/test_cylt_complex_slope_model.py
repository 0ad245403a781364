"""The NumPy yardstick of C ABI section 18 (tests/cylt_complex_slope_model.py) pinned on the CPU, before the GPU is held to it,
all at N = 130 (the real-axis case at its own N = 2000):
  * row 0 of `jets` is CyltComplexModel.eval to rounding, statuses included;
  * the derivative rows against Cauchy's formula on the model itself, in omega and in a complex k, two radii;
  * d omega / dk against the slope of the model's own root curve at root A and the three rows of C;
  * on the real axis, d omega / dk against c_g of the real path's model (tests/root_slope_model.py) at the nine roots of CR_kink;
  * conjugate symmetry of the jets;
  * the Newton rule on the model reaches the roots of A, B and C;
  * the densify case: Hermite prediction from five coarse rows, Newton with the exact jets, a growth rate that falls throughout.
Every recorded bound is 10 x the figure recorded in the helper; `pytest -s` prints the figures of the run."""
import numpy as np
import pytest

from tests import cylt_complex_slope_model as C
from tests.complex_slope_model import dwdk


@pytest.mark.parametrize("name", C.NAMES)
def test_row_zero_is_the_value_model(name):
    """The same scipy calls and the same operations in the same order: bound 64 ulp = 1.4e-14 of max(|outer|, |inner|)."""
    M = C.model(name)
    pairs = list(C.NON_ROOT[name]) + [C.LEAKY]
    k, w = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    outer, inner, st = C.jets(M, k, w)
    D, mo, mi, rel, mst = M.eval_points(k, w)
    assert st.tolist() == mst.tolist() == [0, 0, 1]
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
    pairs = C.cauchy_pairs()
    assert len(pairs) == 5 + 2 * 5
    for M, label, k, w in pairs:
        outer, inner, st = C.jets(M, k, [w])
        assert st[0] == 0
        cw, ck, radii = C.cauchy_parts(M, k, w, r=1e-2, n=32)
        ew = np.abs(np.array([outer[1, 0], inner[1, 0]]) - cw) / max(abs(outer[1, 0]), abs(inner[1, 0]))
        ek = np.abs(np.array([outer[2, 0], inner[2, 0]]) - ck) / max(abs(outer[2, 0]), abs(inner[2, 0]))
        print(f"{label} k = {k}, omega = {w:.6f}: |jets - Cauchy| d/dw {ew.max():.2e}, d/dk {ek.max():.2e}; radii 0.01 and "
              f"0.005 disagree by {radii:.2e}")
        worst, worst_radii = max(worst, ew.max(), ek.max()), max(worst_radii, radii)
    print(f"worst {worst:.2e} (recorded {C.CAUCHY_MEASURED:.1e}, bound 10 x); radii {worst_radii:.2e} (recorded "
          f"{C.CAUCHY_RADII_MEASURED:.1e}, bound 10 x)")
    assert worst <= 10.0 * C.CAUCHY_MEASURED
    assert worst_radii <= 10.0 * C.CAUCHY_RADII_MEASURED


def test_slope_is_the_slope_of_the_root_curve():
    """For orientation: a secant trace of the model gives -0.0377 - 1.8345i at A (k = 1) and -0.0180 - 0.6849i at C (k = 0.5)."""
    cases = C.slope_cases()
    for key, (M, k, root, slope) in cases.items():
        outer, inner, st = C.jets(M, k, root)
        got = dwdk(outer, inner)[0]
        err = abs(got - slope) / max(1.0, abs(slope))
        print(f"{key} k = {k}: root {root:.12f}, d omega / dk = {got:.12f}, curve slope {slope:.12f}, |difference| = {err:.2e} "
              f"(recorded {C.SLOPE_MEASURED[key]:.1e}, bound 10 x)")
        assert st[0] == 0 and err <= 10.0 * C.SLOPE_MEASURED[key]
    assert abs(cases[("A", 0)][3] - (-0.0377 - 1.8345j)) < 1e-4 and abs(cases[("C", 0)][3] - (-0.0180 - 0.6849j)) < 1e-4


def test_real_axis_slope_is_the_real_group_speed():
    eq, mode, m, k, w, cg, s = C.real_axis_case()
    err = np.abs(s - cg) / np.maximum(1.0, np.abs(cg))
    print(f"{C.REAL_AXIS_CASE}: {len(k)} real roots, worst |d omega / dk - c_g| / max(1, |c_g|) = {err.max():.2e}, worst |Im| = "
          f"{np.abs(s.imag).max():.2e} (recorded {C.REAL_AXIS_MEASURED:.1e}, bound 10 x)")
    assert len(k) == 9 and err.max() <= 10.0 * C.REAL_AXIS_MEASURED
    assert np.all(s.imag == 0.0)


def test_conjugate_symmetry_of_the_model():
    for name in C.NAMES:
        M = C.model(name)
        for k, w in C.NON_ROOT[name]:
            oa, ia, _ = C.jets(M, k, [w])
            ob, ib, _ = C.jets(M, k, [np.conj(w)])
            sc = np.maximum(np.abs(oa), np.abs(ia))
            err = max(np.max(np.abs(ob - np.conj(oa)) / sc), np.max(np.abs(ib - np.conj(ia)) / sc))
            a, b = dwdk(oa, ia)[0], dwdk(ob, ib)[0]
            print(f"{name} k = {k}, omega = {w}: |jets (conj omega) - conj jets (omega)| / row scale = {err:.2e}, the same of "
                  f"d omega / dk {abs(b - np.conj(a)):.2e}")
            assert err <= 1e-13 and abs(b - np.conj(a)) <= 1e-13 * max(1.0, abs(a))


def test_newton_model_reaches_the_roots():
    for name in ("A", "B", "C"):
        M = C.root_model(name)
        for k, root in C.case_roots(name):
            for sgn in (1, -1):
                r = C.newton_model(M, k, root + sgn * C.NEWTON_OFFSET)
                print(f"{name} k = {k}, start root {'+' if sgn > 0 else '-'} 1e-3 (1 + i): {r['iters']} steps {r['steps']}, "
                      f"|w - root| = {abs(r['w'] - root):.2e}, resid {r['resid']:.1e} %")
                assert r["flag"] == 1 and r["iters"] == C.NEWTON_STEPS <= 8
                assert abs(r["w"] - root) <= 1e-12 * max(1.0, abs(root))
    M = C.root_model("A")
    k, root = C.case_roots("A")[0]
    r = C.newton_model(M, k, root + C.NEWTON_OFFSET, max_iter=0)
    assert r["iters"] == 0 and r["w"] == root + C.NEWTON_OFFSET and r["flag"] == 1
    r = C.newton_model(M, k, root + C.NEWTON_OFFSET, max_iter=1, step_cap=1e-4)
    assert r["iters"] == 1 and abs(abs(r["w"] - root - C.NEWTON_OFFSET) - 1e-4) <= 1e-15
    r = C.newton_model(M, k, root + C.NEWTON_OFFSET, max_shift=1e-4)
    assert r["flag"] == 0 and abs(r["w"] - root) <= 1e-12
    r = C.newton_model(M, *C.LEAKY)
    assert r["flag"] == 0 and r["iters"] == 0 and r["status"] == 1 and np.isnan(r["resid"])


def test_densify_case_on_the_model():
    """Problem A on k in [0.85, 1.1]: one distinct root per coarse row, the Hermite prediction of shooting.hermite_guess from the
    exact slopes far inside its shift bound, Newton with the exact jets in 1 - 3 steps on the model's secant roots, and a growth
    rate that falls over the whole interval, so postprocess.most_unstable reports no interior maximum."""
    import torch
    from eigensolver_amd import postprocess as pp
    from eigensolver_amd.shooting import hermite_guess
    M, kc, wc, kf, branch = C.densify_case()
    assert len(kc) == 5 and len(kf) == 21 and np.array_equal(kc, kf[::5])
    assert abs(wc[0] - C.DENSIFY_ENDS[0]) < 1e-6 and abs(wc[-1] - C.DENSIFY_ENDS[1]) < 1e-6
    assert np.max(np.abs(branch[::5] - wc)) <= 1e-12
    outer, inner, st = C.jets(M, kc, wc)
    assert np.all(st == 0)
    pred, bound = (t.numpy() for t in hermite_guess(*(torch.as_tensor(np.array(a)) for a in (kc, wc, dwdk(outer, inner), kf))))
    miss = np.abs(pred - branch)
    res = [C.newton_model(M, k, p, max_shift=b) for k, p, b in zip(kf, pred, bound)]
    iters = [r["iters"] for r in res]
    err = max(abs(r["w"] - b) for r, b in zip(res, branch))
    print(f"densify on the model: worst |predicted - secant root| = {miss.max():.2e} (recorded {C.DENSIFY_PREDICTION_MEASURED:.1e}, "
          f"bound 10 x), smallest shift bound {bound.min():.2e}; Newton steps {iters}, worst |w - secant root| = {err:.2e} "
          f"(bound 1.0e-12)")
    assert miss.max() <= 10.0 * C.DENSIFY_PREDICTION_MEASURED < bound.min()
    assert all(r["flag"] == 1 for r in res) and 1 <= min(iters) and max(iters) <= 3
    assert err <= 1e-12
    of, inn, _ = C.jets(M, kf, branch)
    slope = dwdk(of, inn)
    print(f"Im d omega / dk over the interval in [{slope.imag.min():.4f}, {slope.imag.max():.4f}]")
    assert np.all(slope.imag < 0.0)
    kstar, _ = pp.most_unstable(kf, branch, slope)
    assert len(kstar) == 0

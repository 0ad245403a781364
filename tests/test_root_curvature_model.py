"""The yardsticks of tests/root_curvature_model.py, pinned on the CPU (no GPU needed).

  * every pair's self-discrepancy (Cauchy's formula at the pair's radius against half of it) is what the model file stores,
    none above 1e-8, at least three pairs per case (the four large-gap cases: the gap-targeted pairs of the slope tests, two
    on each side of mu (R - 1) = 40, with the gap stored beside them); value and first derivatives are the complex-step jets of
    tests/root_slope_model.py
  * the golden file the GPU tests read is what the model gives, in every field those tests use: the pairs and all six
    rows of their jets, the roots of the curvature check with c_g and q, the extremum's bracket, answer and trace
  * d2 omega / dk2 at the model's roots against the Richardson-combined central difference of its c_g, per case under 10 x the
    stored figure
  * the restatement of the rule of es_shoot_cg_extrema finds the group-speed minimum of the fast sausage branch of the density
    slab: a minimum of c_g on a scan of the model's own curve
  * postprocess.hermite_branch_quintic
All but the last are tests of the yardstick: they run the NumPy model alone and say nothing about the library, which
tests/test_root_curvature_gpu.py, the code-object test and the hermite_branch_quintic tests here cover.
`pytest -s` prints the figures.
"""
import numpy as np
import pytest

from tests import root_curvature_model as C
from tests import root_slope_model as R


@pytest.mark.parametrize("name", C.CASES)
def test_self_discrepancy_and_golden(name):
    k, w = C.pairs(name)
    o, i, d = C.case_jets(name)
    stored = np.array(C.SELF_MEASURED[name])
    print(f"{name}: radii {C.RADIUS[name]}, self-discrepancy {d} (stored {stored})")
    assert len(k) >= 3 and np.all(stored <= 1e-8)
    assert np.all(d <= 2.0 * stored + 1e-13)                  # the stored figure, up to the run-to-run rounding of the FFT
    # value and first derivatives: the complex step
    so, si = R.jets(name, k, w)
    first = np.maximum(np.abs(o[:3] - so), np.abs(i[:3] - si)) / np.maximum(np.abs(so), np.abs(si))
    print(f"{name}: rows 0-2 against the complex step {first.max():.1e}")
    assert first.max() <= 1e-11
    g = C.read_golden()["cases"][name]
    assert np.array_equal(g["k"], k) and np.array_equal(g["w"], w)
    if name in C.M.LARGE_GAP:
        # the pairs are the slope tests' gap-targeted ones, two on each side of the branch of exterior_cylinder at 40
        gaps = C.gaps(name)
        far = C.M.problem(name).L_factor * 2.0 * np.pi / k      # R, in units of the tube radius
        print(f"{name}: gaps {gaps}, exterior arguments mu R {gaps * far / (far - 1.0)}")
        assert np.array_equal(R.pairs(name)[0], k) and np.array_equal(R.pairs(name)[1], w)
        assert np.allclose(g["gap"], gaps, rtol=1e-14, atol=0.0) and (gaps < 40.0).sum() == 2 and (gaps >= 40.0).sum() == 2
    else:
        assert "gap" not in g
    go, gi = np.array(g["outer"]), np.array(g["inner"])
    assert np.max(np.maximum(np.abs(go[:3] - o[:3]), np.abs(gi[:3] - i[:3])) / np.maximum(np.abs(o[:3]), np.abs(i[:3]))) <= 1e-12
    scale = np.maximum(np.abs(o[3:]), np.abs(i[3:]))
    assert np.all(np.maximum(np.abs(go[3:] - o[3:]), np.abs(gi[3:] - i[3:])) / scale <= 2.0 * stored + 1e-13)


@pytest.mark.parametrize("name", C.CURVE_CASES)
def test_curvature_against_the_difference_of_cg(name):
    k, w, r = C.curve_roots(name)
    wp, cg, q, dq = C.curve_check(name, k, w, r)
    err = np.abs(q - dq) / np.maximum(1.0, np.abs(q))
    print(f"{name}: {len(k)} roots, d2w/dk2 {q}, against the difference of c_g {err} (bound {10.0 * C.CURVE_MEASURED[name]:.1e})")
    assert len(k) >= 1 and err.max() <= 10.0 * C.CURVE_MEASURED[name]
    # the golden file holds these roots: k and omega to the last polish step, c_g and q to the noise of the FFT
    g = {f: np.array(v) for f, v in C.read_golden()["curve"][name].items()}
    assert np.array_equal(g["k"], k) and np.max(np.abs(g["w"] - wp) / np.abs(wp)) <= 1e-14
    assert np.max(np.abs(g["cg"] - cg) / np.maximum(1.0, np.abs(cg))) <= 1e-12
    assert np.max(np.abs(g["q"] - q) / np.maximum(1.0, np.abs(q))) <= 1e-12
    if name == C.EXTREMUM_CASE:
        # the figure the feature was specified with: 8.99374e-3 at the root (3.4305002, 3.982627), the case's first pair
        assert abs(k[0] - C.EXTREMUM_START[0]) <= 1e-7 and abs(wp[0] - C.EXTREMUM_START[1]) <= 1e-6 and abs(q[0] - 8.99374e-3) <= 1e-8


def test_extremum_rule_finds_the_group_speed_minimum():
    br = C.extremum_bracket()
    assert (br[0], br[2]) == C.EXTREMUM_BRACKET
    x = C.cg_extrema(C.EXTREMUM_CASE, *br)
    g = C.read_golden()["extremum"]
    print(f"k* = {x['k']!r}, omega* = {x['w']!r}, c_g* = {x['cg']!r}, q* = {x['q']:.1e}, {x['iters']} iterates: {x['trace']}")
    assert x["changed"] and 0 < x["iters"] < 40 and abs(x["q"]) <= 1e-10
    assert abs(x["cg"] - 1.1226) <= 1e-4 and 1.15 <= x["w"] / x["k"] <= 1.29
    # every field of the golden file the GPU test asserts on
    assert g["iters"] == x["iters"] and g["changed"] == x["changed"] and g["bracket"] == list(br)
    assert abs(g["k"] - x["k"]) <= 1e-12 * x["k"] and abs(g["w"] - x["w"]) <= 1e-12 * x["w"]
    assert abs(g["cg"] - x["cg"]) <= 1e-12 * x["cg"] and abs(g["q"] - x["q"]) <= 1e-12
    assert len(g["trace"]) == x["iters"] and np.max(np.abs(np.array(g["trace"]) / np.array(x["trace"]) - 1.0)) <= 1e-12
    # a minimum of c_g on a scan of the model's own root curve, step 1e-4, around k*: the curve by Newton from the Taylor
    # prediction of the extremum
    ks = np.round(x["k"], 4) + 1e-4 * np.arange(-300, 301)
    dk = ks - x["k"]
    ws, ok = C.newton(C.EXTREMUM_CASE, ks, x["w"] + x["cg"] * dk)
    cg = R.group_velocity(*R.jets(C.EXTREMUM_CASE, ks, ws))
    j = int(np.argmin(cg))
    print(f"scan: least c_g {cg[j]!r} at k = {ks[j]!r}")
    assert ok.all() and 0 < j < len(ks) - 1 and abs(ks[j] - x["k"]) <= 1e-4 and cg[j] >= x["cg"] - 1e-12


# ---- postprocess.hermite_branch_quintic ---------------------------------------------------------------------------------------
def test_quintic_hermite_reproduces_a_quintic_and_is_smooth():
    from eigensolver_amd import postprocess as pp
    p = np.polynomial.Polynomial([0.3, -1.2, 0.7, 0.45, -0.31, 0.08])
    ks = np.array([0.5, 0.9, 1.7, 2.0, 3.1])
    f = pp.hermite_branch_quintic(ks, p(ks), p.deriv(1)(ks), p.deriv(2)(ks))
    x = np.linspace(0.2, 3.4, 321)                            # beyond the ends: the end quintics continued
    for nu in (0, 1, 2):
        err = np.max(np.abs(f(x, nu) - p.deriv(nu)(x)) if nu else np.abs(f(x) - p(x)))
        print(f"nu = {nu}: {err:.1e}")
        assert err <= 1e-12
    # any data: value, slope and curvature are met at the knots from both sides
    rng = np.random.default_rng(5)
    y, d, c = rng.normal(size=(3, len(ks)))
    f = pp.hermite_branch_quintic(ks, y, d, c)
    for nu, want in ((0, y), (1, d), (2, c)):
        left, right = f(ks[1:] - 1e-13, nu), f(ks[:-1], nu)
        assert np.max(np.abs(right - want[:-1])) <= 1e-12 and np.max(np.abs(left - want[1:])) <= 1e-9
    assert float(f(1.0)) == f(np.array([1.0]))[0]
    with pytest.raises(ValueError):
        f(1.0, nu=3)


@pytest.mark.parametrize("args", (([1.0], [1.0], [1.0], [1.0]), ([1.0, 2.0], [1.0, 2.0], [1.0, 2.0], [1.0]),
                                  ([1.0, 1.0], [1.0, 2.0], [0.0, 0.0], [0.0, 0.0]),
                                  ([2.0, 1.0], [1.0, 2.0], [0.0, 0.0], [0.0, 0.0]),
                                  ([[1.0, 2.0]], [[1.0, 2.0]], [[0.0, 0.0]], [[0.0, 0.0]])))
def test_quintic_hermite_argument_errors(args):
    from eigensolver_amd import postprocess as pp
    with pytest.raises(ValueError):
        pp.hermite_branch_quintic(*args)
    if np.shape(args[3]) == np.shape(args[0]):
        with pytest.raises(ValueError):                        # hermite_branch raises on the same
            pp.hermite_branch(*args[:3])

"""CPU pin of tests/cylt_complex_eigen_model.py, the NumPy restatement of C ABI section 19 (no GPU):
  * the sample the GPU tests use leaves at least half of its 65 pairs OK on every problem and node count (the smallest share is
    39 of 65, problem B at N = 129), with both signs of Im omega and a different k in every lane;
  * the boundary values are 1, the exterior flux there is `outer`, P(axis node) is the target of the axis condition;
  * `boundary_flux_spread` -- |inner of the outward step's discrete solution - inner by the determinant's adjoint march| --
    is at most 1e-12 of the scale for the sausage problem and the zero-twist jet (target 0), and for A, B and reference
    (target != 0) it is not zero and smaller at N = 300 than at N = 130 on the same pairs;
  * the model's interior against DOP853 on complex y at N = 130 and 300, two pairs per problem.

Measured spread, worst over the OK pairs of the N = 130 sample as a fraction of max(|outer|, |inner|), N = 130 / 300: A 2.2e-6 /
3.4e-8, B 2.7e-5 / 7.9e-7, C 1.2e-7 / 1.1e-9, reference 1.7e-4 / 2.1e-5, sausage 5e-17 / 8e-17, zero twist 2e-16 / 2e-16.

The DOP853 comparison.  The sausage problem is held to real_eigen_model.bound(N) (measured 5e-8 at N = 130, 2e-9 at 300).  The
four ES_AXIS_ROTATION_KINK problems keep the singular solution (P, Xi ~ r^-m) in the answer, and the project's singular-axis
allowances -- SINGULAR_AXIS_BOUND = 1e-3 of max|field| on the whole interval, SINGULAR_AXIS_FAR_BOUND = 2e-5 over |r| >= 0.02 --
were set on the default grid of 1000 nodes with m = 1.  At N = 130 and 300 every one of the four needs more than those.  Measured,
worst of P and xi_r over the two pairs, whole interval / far part:
    N = 130: A 8.4e-2 / 5.1e-1, B 1.5e-2 / 2.6e-2, C 3.2e-1 / 3.0, reference 2.3e-2 / 1.9e-3
    N = 300: A 3.2e-3 / 1.0e-2, B 8.1e-4 / 2.0e-3, C 9.9e-3 / 5.6e-2, reference 1.1e-2 / 4.6e-4
The reason is the grid, not the restatement: h / r_axis is 0.77 at N = 130 for r_axis = 1e-2 (7.7 for the reference problem's
1e-3), and RK4 with coefficient sets at node, mid-point, node does not reproduce the decay of r^-m over the first steps.  For
the scalar problem y' = -m y / r the factor by which the marched solution misses (r_b / r_axis)^-m is `power_law_miss`: 0.52
(m = 3) and 4.2 (m = 4) at N = 130, 1.05e-2 and 5.7e-2 at N = 300 -- the measured far-part errors of A and C to within 30 %.
That factor stays on the singular part at every node beyond the first steps, so it is what the far part sees.  The bound
used here for these four is therefore, written down before it was compared with the model:
    allowance * (1000 / N)^4  +  4 * power_law_miss(m, N)
the first term the project's own h^4 scaling of a bound set at N = 1000 (real_eigen_model.bound), the second the scalar model
with the factor 4 real_eigen_model.boundary_flux_spread documents for two RK4 marches of one order.  At N = 130 it is vacuous
for A and C (> 1): on that grid their eigenfunctions are not converged near the axis, and the test says so in its output."""
import numpy as np
import pytest

from tests import cylt_complex_eigen_model as tem
from tests.cases import truth_problem
from tests.real_eigen_model import SINGULAR_AXIS_BOUND, SINGULAR_AXIS_FAR, SINGULAR_AXIS_FAR_BOUND, bound

ARRAYS = ("value_int", "flux_int", "value_ext", "flux_ext")


@pytest.fixture(scope="module")
def models():
    """(name, N) -> (model, k, w, eigenfunction dict of the 65-pair sample), computed once; callers do not modify it."""
    out = {}
    for n in tem.NODE_COUNTS:
        for name in tem.ALL_NAMES:
            E = tem.model_of(name, n)
            k, w = tem.pairs(name, n)
            out[name, n] = (E, k, w, E.eigenfunction(k, w, n_ext=5))
    return out


@pytest.mark.parametrize("n_nodes", tem.NODE_COUNTS)
@pytest.mark.parametrize("name", tem.ALL_NAMES)
def test_boundary_values_axis_target_and_seeds(models, name, n_nodes):
    E, k, w, e = models[name, n_nodes]
    ok = e["status"] == 0
    print(f"{name} N={n_nodes}: {int(ok.sum())} of 65 pairs OK")
    assert ok.sum() >= 33, ok.sum()
    assert (w.imag > 0).any() and (w.imag < 0).any() and len(np.unique(k)) == 65
    sc = np.maximum(np.abs(e["outer"][ok]), np.abs(e["inner"][ok]))
    assert np.max(np.abs(e["flux_ext"][ok, -1] - e["outer"][ok]) / sc) < 1e-13
    assert np.max(np.abs(e["value_ext"][ok, -1] - 1.0)) < 1e-13
    assert np.all(np.abs(e["x_ext"][:, -1]) == 1.0)
    for a in ARRAYS:
        assert np.all(np.isnan(e[a][~ok].real)) and np.all(np.isfinite(e[a][ok]))
    bc, c = E.M.d["axis_bc"], E.M.d["bc_const"]
    if bc != 1:                                              # P(r_ax) = +- bc_const xi_e
        target = (c if bc == 0 else -c) * e["outer"][ok]
        assert np.max(np.abs(e["value_int"][ok, -1] - target)) <= 1e-15 * np.max(np.abs(e["value_int"][ok]))
        assert (c != 0.0) == (name != tem.ZERO_TWIST)
    assert np.max(np.abs(e["value_int"][ok, 0] - 1.0)) < 1e-13                # b = 1 / P(g_0) imposes it; s_0 has no P


@pytest.mark.parametrize("name", tem.ALL_NAMES)
def test_boundary_flux_spread(models, name):
    """The jump of the flux equals D_c to rounding where the axis target is zero and to the RK4 truncation otherwise."""
    _, k, w, e = models[name, 130]
    ok = e["status"] == 0
    sc = np.maximum(np.abs(e["outer"][ok]), np.abs(e["inner"][ok]))
    s130 = tem.boundary_flux_spread(name, k, w, 130)[ok]
    s300 = tem.boundary_flux_spread(name, k, w, 300)[ok]          # the same pairs on the finer grid
    assert np.all(np.isfinite(s130)) and np.array_equal(s130, np.abs(e["inner_outward"][ok] - e["inner"][ok]))
    fin = np.isfinite(s300)
    assert fin.sum() >= 0.9 * ok.sum()
    w130, w300 = float(np.max(s130 / sc)), float(np.max(s300[fin] / sc[fin]))
    print(f"{name}: worst spread / scale = {w130:.2e} at N = 130, {w300:.2e} at N = 300 ({int(ok.sum())} pairs)")
    if name in ("sausage", tem.ZERO_TWIST):
        assert w130 <= 1e-12 and w300 <= 1e-12
    else:
        assert w130 > 1e-12
        if name in ("A", "B", "reference"):
            assert 0.0 < w300 < w130


def power_law_miss(q, r_axis, n_nodes):
    """|marched / exact - 1| at the boundary for y' = -q y / r marched by RK4 (coefficients at node, mid-point, node) from
    r_axis out to 1 on the grid of n_nodes nodes: how far the discrete decay of a singular solution r^-q is from the true one."""
    h = (1.0 - r_axis) / (n_nodes - 1)
    y = 1.0
    for j in range(n_nodes - 1):
        r = r_axis + j * h
        a0, am, a1 = -q / r, -q / (r + 0.5 * h), -q / (r + h)
        k1 = a0 * y
        k2 = am * (y + 0.5 * h * k1)
        k3 = am * (y + 0.5 * h * k2)
        k4 = a1 * (y + h * k3)
        y = y + h / 6.0 * (k1 + k4) + h / 3.0 * (k2 + k3)
    return abs(y * r_axis ** -q - 1.0)


def test_power_law_miss_is_what_the_docstring_quotes():
    assert abs(power_law_miss(3, 1e-2, 130) - 0.518) < 1e-3 and abs(power_law_miss(4, 1e-2, 300) - 5.69e-2) < 1e-4


@pytest.mark.parametrize("n_nodes", [130, 300])
@pytest.mark.parametrize("name", tem.NAMES)
def test_interior_against_dop853(name, n_nodes):
    eq, mode, m, _, _, _ = tem.problems(n_nodes)[name]
    E = tem.model_of(name, n_nodes)
    prob = truth_problem(eq, mode, m)
    k, w = tem.dop_pairs(name, n_nodes)
    e = E.eigenfunction(k, w, n_ext=0)
    assert np.all(e["status"] == 0)
    if E.M.d["axis_bc"] == tem.AXIS_ROTATION_KINK:
        scale = max(1.0, (1000.0 / n_nodes) ** 4)
        miss = 4.0 * power_law_miss(int(E.M.d["m"]), abs(E.M.d["x_end"]), n_nodes)
        b_whole, b_far = SINGULAR_AXIS_BOUND * scale + miss, SINGULAR_AXIS_FAR_BOUND * scale + miss
    else:
        b_whole = b_far = bound(n_nodes)
    far = np.abs(E.x_int) >= SINGULAR_AXIS_FAR
    for i in range(2):
        P, xi = E.interior_dop853(prob, k[i], w[i])
        for key, want in (("value_int", P), ("flux_int", xi)):
            err = np.abs(e[key][i] - want)
            whole, fr = float(np.max(err) / np.max(np.abs(want))), float(np.max(err[far]) / np.max(np.abs(want[far])))
            needs_more = whole > SINGULAR_AXIS_BOUND or fr > SINGULAR_AXIS_FAR_BOUND
            print(f"{name} N={n_nodes} pair {i} {key}: |model - DOP853| / max = {whole:.3e} whole (bound {b_whole:.1e}), "
                  f"{fr:.3e} over |r| >= {SINGULAR_AXIS_FAR} (bound {b_far:.1e})"
                  + ("; needs more than the singular-axis allowances 1e-3 / 2e-5: the grid, see the docstring"
                     if needs_more and b_whole != bound(n_nodes) else "")
                  + ("; the bound is vacuous on this grid" if b_far > 1.0 else ""))
            assert whole < b_whole and fr < b_far

"""CPU: the yardsticks tests/test_eigenfunction_gpu.py measures es_shoot_eigenfunction against (tests/real_eigen_model.py).

The two new oracles are pinned against what the suite already trusts -- oracle.cylinder.eigenfunction away from the axis,
the boundary flux of mismatch(), the slab symmetry condition -- and the NumPy RK4 restatement is measured against them per
case and march direction:
  E_trunc   grid_rk4 in float64 against the DOP853 truth     (what the node grid costs)
  E_round   grid_rk4 in float64 against np.longdouble        (what fp64 state arithmetic costs on that grid)
both as max over the nodes of |difference| / max|field|, worse of the two fields; printed with -s, table in DESIGN.md 8.
"""
import numpy as np
import pytest

from oracle import cylinder as oc
from tests import cases
from tests import real_eigen_model as M

CYL = [n for n in M.STANDARD if M.is_cyl(M.all_cases()[n][0])]
SLAB = [n for n in M.STANDARD if not M.is_cyl(M.all_cases()[n][0])]


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", [n for n in CYL if n != "CF_flow_m5"])
def test_outward_truth_agrees_with_inward_oracle_away_from_the_axis(name):
    """Both integrate the same ODE at rtol 1e-12; away from the axis (|r| >= 0.05) the inward one has not yet amplified its
    error.  Bound 1e-8 of max|field| there: the issue's CPU figure is 4e-10 for m = 3; the exterior is the same closed form."""
    eq = M.all_cases()[name][0]
    k, w = M.pairs(name)
    t = M.truth(name, 0)
    o = oc.eigenfunction(M.problem(name), float(k[0]), float(w[0]), eq.n_nodes, n_ext=500)
    far = np.abs(o["r_int"]) >= 0.05
    assert np.array_equal(t["x_int"], o["r_int"]) and np.array_equal(t["x_ext"], o["r_ext"])
    for kt, ko in (("value_int", "P_int"), ("flux_int", "xi_int")):
        r = _rel(t[kt][far], o[ko][far])
        print(f"{name} {kt}: outward vs inward DOP853 on |r| >= 0.05: {r:.2e} (bound 1e-8)")
        assert r <= 1e-8, (name, kt, r)
    for kt, ko in (("value_ext", "P_ext"), ("flux_ext", "xi_ext")):
        # the same closed form, summed term by term: equal to rounding of the two terms (they cancel at the far end)
        size = np.abs(t[kt + "_terms"][0]) + np.abs(t[kt + "_terms"][1])
        assert np.all(np.abs(t[kt] - o[ko]) <= 1e-14 * size), (name, kt)


@pytest.mark.parametrize("name", M.STANDARD)
def test_boundary_state_agrees_with_mismatch(name):
    """flux_int at the boundary node is mismatch()'s inner value (xi_i, P_in), flux_ext at the boundary its outer one and
    the boundary value is +-1 (flow slabs: Omega(-1) / Omega_e of it)."""
    k, w = M.pairs(name)
    prob = M.problem(name)
    for i in range(2):
        t = M.truth(name, i)
        d, outer, inner, st = prob.mismatch(float(k[i]), float(w[i]))
        assert st == 0
        # mismatch marches from the boundary inwards; the boundary slope is well conditioned in both directions
        assert abs(t["flux_int"][0] - inner) <= 1e-8 * max(abs(inner), abs(outer)), (name, i, t["flux_int"][0], inner)
        assert abs(t["flux_ext"][-1] - outer) <= 1e-13 * abs(outer), (name, i)
        assert abs(abs(t["value_ext"][-1]) - 1.0) <= 1e-13


@pytest.mark.parametrize("name", SLAB)
def test_slab_truth_is_symmetric(name):
    _, mode, _, _ = M.all_cases()[name]
    sgn = -1.0 if mode == "sausage" else 1.0
    for i in range(M.N_PAIRS):
        v = M.truth(name, i)["value_int"]
        assert abs(v[-1] - sgn * v[0]) <= 1e-10 * np.max(np.abs(v)), (name, i, v[0], v[-1])


def _figures(name, i):
    """(E_trunc, E_round) of pair i for the kernel's algorithm (real_eigen_model.model)."""
    k, w = (float(a[i]) for a in M.pairs(name))
    t = M.truth(name, i)
    v64, f64 = M.model(name, k, w)
    vld, fld = M.model(name, k, w, dtype=np.longdouble)
    checks = M.interior_error(name, "value_int", v64, t["value_int"], t["x_int"]) + \
        M.interior_error(name, "flux_int", f64, t["flux_int"], t["x_int"])
    e_r = max(_rel(v64, vld), _rel(f64, fld))
    return checks, float(e_r)


@pytest.mark.parametrize("name", M.STANDARD)
def test_model_against_truth(name):
    """The kernel's algorithm in NumPy meets the project's bound against DOP853 on the WHOLE interval, axis node included
    (so the kernel can), and its fp64 rounding stays below 1e-11 of max|field| (so that the 1e-10 kernel-against-restatement
    check of the GPU file is a statement about the kernel, not about the pair chosen)."""
    for i in range(M.N_PAIRS):
        checks, e_r = _figures(name, i)
        e_t, b = max(checks, key=lambda c: c[0] / c[1])
        print(f"{name} pair {i}: E_trunc {e_t:.2e} (bound {b:.1e})  E_round {e_r:.2e} (bound 1e-11)")
        assert all(e <= b for e, b in checks), (name, i, checks)
        assert e_r <= 1e-11, (name, i, e_r)


@pytest.mark.parametrize("name", ["CF_flow_kink", "CF_flow_m3", "CF_flow_m5", "CR_kink"])
def test_inward_march_figures(name):
    """The march the kernel used before, from the truth's boundary state to the axis, where the singular solution grows
    like r^-(m+1): printed for DESIGN.md.  For m >= 3 it must MISS the bound -- the reason the kernel marches outwards; if
    it ever met it, the conditioning argument in DESIGN.md would be wrong."""
    N = M.all_cases()[name][0].n_nodes
    k, w = (float(a[0]) for a in M.pairs(name))
    t = M.truth(name, 0)
    x = t["x_int"]
    y0 = [t["value_int"][0], t["flux_int"][0] * x[0]]
    y64 = M.grid_rk4(M.problem(name), k, w, np.array(y0), x)
    yld = M.grid_rk4(M.problem(name), k, w, np.array(y0, dtype=np.longdouble), x)
    e_t = max(_rel(y64[0], t["value_int"]), _rel(y64[1] / x, t["flux_int"]))
    e_r = float(max(_rel(y64[0], yld[0]), _rel(y64[1] / x, yld[1] / x)))
    print(f"{name} pair 0 inward march: E_trunc {e_t:.2e} (bound {M.bound(N):.1e})  E_round {e_r:.2e}")
    if name in ("CF_flow_m3", "CF_flow_m5"):
        assert e_t > 100 * M.bound(N), (name, e_t)


def test_grid_rk4_order_and_dtype():
    """Fourth order on a problem with varying coefficients, and longdouble in, longdouble out."""
    name = "SFG_flow_kink"
    k, w = (float(a[0]) for a in M.pairs(name))
    prob = M.problem(name)
    errs = []
    for n in (41, 81):
        x = np.linspace(-1.0, 1.0, n)
        y = M.grid_rk4(prob, k, w, np.array([1.0, 0.3]), x)
        ref = M.grid_rk4(prob, k, w, np.array([1.0, 0.3]), np.linspace(-1.0, 1.0, 16 * (n - 1) + 1))
        errs.append(np.max(np.abs(y[:, -1] - ref[:, -1])))
    assert 12.0 < errs[0] / errs[1] < 20.0, errs
    assert M.grid_rk4(prob, k, w, np.array([1.0, 0.3], dtype=np.longdouble), np.linspace(-1, 1, 5)).dtype == np.longdouble


def test_large_gap_pairs_straddle_the_branch():
    for name in M.LARGE_GAP:
        k, w = M.large_gap_pairs(name)
        gaps = [M.truth(name, i, True)["gap"] for i in range(len(k))]
        print(name, "gaps", ["%.2f" % g for g in gaps])
        assert min(gaps) < 40.0 < max(gaps), (name, gaps)
        assert sum(g < 40.0 for g in gaps) >= 2 and sum(g >= 40.0 for g in gaps) >= 2, (name, gaps)

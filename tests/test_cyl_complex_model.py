"""tests/cyl_complex_model.py (the NumPy restatement the GPU tests of C ABI section 14 compare with) against what is known
without it: the real oracle on the real axis, a complex DOP853 integration off it, and the unstable kink root of the uniform
jet.  CPU only."""
import numpy as np
import pytest

from eigensolver_amd import equilibrium as q
from tests.cases import truth_problem
from tests.cyl_complex_model import model_for

KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0)


@pytest.mark.parametrize("name", ["flow_kink", "density_sausage", "density_rplus_m2"])
def test_real_axis_equals_the_real_oracle(name):
    """w_im = 0, N = 200: the model equals oracle.cylinder.CylinderProblem.mismatch (DOP853) times the sign of the real
    path's P_b wherever that status is OK, within the RK4 contract of DESIGN section 2 at N = 200 -- 3e-8 (1000 / 200)^4 =
    1.9e-5 of the scale; measured 2.7e-10 ... 3.8e-9 on these points -- and carries no imaginary part; leaky points are leaky
    in both."""
    eq, mode, m, pts = {
        "flow_kink": (q.CylinderFlow(U_i0=0.6, width=1.0, n_nodes=200), "kink", None,
                      [(0.5, 1.6), (1.1, 3.4), (2.0, 6.3), (2.0, 9.1), (1.1, 5.2), (0.5, 2.6)]),
        "density_sausage": (q.CylinderDensity(width=0.95, n_nodes=200), "sausage", None,
                            [(0.5, 1.7), (1.1, 4.1), (2.0, 7.2), (2.0, 9.6), (1.1, 5.7)]),
        "density_rplus_m2": (q.CylinderDensity(width=1.5, c_e=1.5, vA_e=0.5, r_sign=1.0, n_nodes=200, ic=(1e-8, 1e-8)), "kink", 2,
                             [(0.5, 0.31), (1.1, 0.9), (2.0, 2.1), (2.0, 2.9), (1.1, 1.8)]),
    }[name]
    M, T = model_for(eq, mode, m), truth_problem(eq, mode, m)
    n_ok = n_leaky = 0
    worst = 0.0
    for k, w in pts:
        d, xi_e, xi_i, st = T.mismatch(k, w)
        D, outer, inner, rel, stm = M.eval(k, [w])
        if st == 3:
            continue                                   # continuum: the oracle does not integrate there
        assert stm[0] == st, (k, w, st, stm[0])
        if st != 0:
            n_leaky += 1
            assert np.isnan(D[0].real)
            continue
        Pb = T.exterior(k, w)[2]
        sc = max(abs(xi_e), abs(xi_i))
        assert D[0].imag == 0.0
        worst = max(worst, abs(D[0].real - Pb * d) / sc)
        n_ok += 1
    print(f"{name}: max |model - sign(P_b) oracle| / scale = {worst:.3e} on {n_ok} OK points, {n_leaky} leaky")
    assert n_ok >= 3 and n_leaky >= 1
    assert worst < 3e-8 * (1000.0 / 200.0) ** 4


POINTS = [(q.CylinderFlow(**KH, width=1.5, n_nodes=400), "kink", None, [(2.0, 2.6 + 0.1j), (1.0, 1.2 + 0.05j), (2.0, 2.2 + 0.3j)]),
          (q.CylinderFlow(**KH, width=0.9, n_nodes=400), "sausage", None, [(2.0, 2.4 + 0.2j), (1.1, 1.0 - 0.15j)]),
          (q.CylinderDensity(width=0.95, n_nodes=400), "kink", 3, [(1.1, 3.3 + 0.2j), (2.0, 8.1 - 0.4j)])]


def test_complex_dop853():
    """Off the real axis (|Im omega| >= 0.05): the model's RK4 march equals the interior integrated by DOP853 on complex y
    (solve_ivp, rtol 1e-12) within the project's RK4 contract, 3e-8 (1000 / N)^4 of the scale, here at N = 400."""
    bound = 3e-8 * (1000.0 / 400.0) ** 4
    worst = 0.0
    for eq, mode, m, pts in POINTS:
        M, T = model_for(eq, mode, m), truth_problem(eq, mode, m)
        for k, w in pts:
            D, outer, inner, rel, st = M.eval(k, [w])
            assert st[0] == 0
            d, o, i = M.eval_dop853(T, k, w)
            sc = max(abs(o), abs(i))
            assert abs(outer[0] - o) == 0.0
            worst = max(worst, abs(D[0] - d) / sc)
    print(f"max |RK4 - DOP853| / scale at N = 400: {worst:.3e} (bound {bound:.3e})")
    assert worst < bound


def test_unstable_kink_root_of_the_uniform_jet():
    """CylinderFlow(c_i0=1, vA_i0=2, c_e=1.5, vA_e=0.5, U_i0=3), width 1e5, kink, k = 2: one flagged cell in the window
    Re omega in [1.8, 3.0] x Im omega in [0.3, 0.9] and the root 2.372765 + 0.584713i, trapped (Re m_e > 0), not leaky; its
    conjugate is the damped partner; the sausage mode has no root there."""
    eq = q.CylinderFlow(**KH, width=1e5, n_nodes=130)
    M = model_for(eq, "kink")
    w_re, w_im = np.linspace(1.8, 3.0, 13), np.linspace(0.3, 0.9, 7)
    cells, roots = M.find_roots([2.0], w_re, w_im)
    assert cells == [(0, 2, 5)]
    w = roots[0]
    assert abs(w - (2.372765 + 0.584713j)) < 1e-6
    D, outer, inner, rel, st = M.eval(2.0, [w, np.conj(w)])
    assert np.all(st == 0) and np.all(rel < 1e-9)
    assert abs(D[1] - np.conj(D[0])) <= 1e-13 * max(abs(outer[0]), abs(inner[0]))
    assert M.find_roots([2.0], w_re, w_im)[1][0] == w                                # deterministic
    assert model_for(eq, "sausage").find_roots([2.0], w_re, w_im)[0] == []
    # N = 1000: the root has converged in N to the digits quoted
    w1000 = model_for(q.CylinderFlow(**KH, width=1e5, n_nodes=1000), "kink").secant(2.0, w, w + 0.01)
    assert abs(w1000 - w) < 1e-6

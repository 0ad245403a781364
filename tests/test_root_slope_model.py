"""CPU side of es_shoot_root_slopes (include/eigensolver_amd.h section 11): the entry point exists, the ABI pins hold, the NumPy
model of tests/root_slope_model.py gives the C port's outer and inner, its complex-step group speed is the slope of the port's
root curves, and the two new postprocess functions do what they say.  No GPU.

Figures of the model (python -m pytest tests/test_root_slope_model.py -s prints them):
  value against the port     worst |model - port| / max(|outer|, |inner|) over the 100 pairs: 1.1e-14 (SFG_flow_sausage)
  c_g against the curve      worst |c_g - slope| / max(1, |slope|): CF_flow_kink_N130 1.4e-12 (7 roots), SFG_flow_kink_N130
                             2.5e-12 (12), CF_flow_sausage 4.0e-12 (8), SD_w15_sausage 2.0e-12 (7), CR_kink 1.3e-12 (9); none
                             left out.  The bounds asserted are 10 x these (root_slope_model.SLOPE_MEASURED).
  CR_kink artefact roots     a central difference of the port's D at relative step 1e-7 is off by 5.7e-4 (k = 2.4,
                             W = 1.3255), 5.0e-5 (k = 2.8, W = 1.37212), 1.1e-5, 2.1e-6; the tangent by 1.0e-12 at the worst of
                             them: eight to nine orders closer.
"""
import ctypes
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from tests import cases
from tests import real_eigen_model as M
from tests import root_slope_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from eigensolver_amd import build
    return ctypes.CDLL(build.build())


def test_header_declares_and_library_exports_the_entry():
    txt = open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+es_shoot_root_slopes\s*\(", txt)
    assert hasattr(_lib(), "es_shoot_root_slopes")


def test_abi_pins_are_unchanged():
    lib = _lib()
    lib.es_abi_version.restype = ctypes.c_int
    lib.es_abi_sizeof.restype = ctypes.c_int
    lib.es_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.es_abi_version() == 1
    assert lib.es_abi_sizeof(8) == -1                     # plain arrays: no new ABI struct


@pytest.mark.parametrize("name", R.VALUE_CASES + M.LARGE_GAP)
def test_model_value_against_the_port(name):
    """outer and inner of the model within 1e-10 of max(|outer|, |inner|) of port.eval_one: the project's bound for a NumPy
    restatement of the same algorithm."""
    eq, mode, m, _ = M.all_cases()[name]
    port = cases.port_problem(eq, mode, m)
    k, w = R.pairs(name)
    o, i = R.case_jets(name)
    assert np.isfinite(o).all() and np.isfinite(i).all(), name
    worst = 0.0
    for j in range(len(k)):
        st, _, _, po, pi = port.eval_one(float(k[j]), float(w[j]))
        assert st == 0, (name, j, st)
        sc = max(abs(po), abs(pi))
        worst = max(worst, abs(o[0][j] - po) / sc, abs(i[0][j] - pi) / sc)
        assert abs(o[0][j] - po) <= 1e-10 * sc and abs(i[0][j] - pi) <= 1e-10 * sc, (name, j, o[0][j], po, i[0][j], pi)
    print(f"{name}: {len(k)} pairs, worst |model - port| / max(|outer|, |inner|) = {worst:.1e} (bound 1.0e-10)")


@pytest.mark.parametrize("name", R.SLOPE_CASES)
def test_model_group_speed_is_the_slope_of_the_root_curve(name):
    """The cap on roots left out is zero: every accepted root of the port forms its curve slope."""
    k, w, slope = R.curve_slopes(name)
    assert len(k) == R.SLOPE_ROOTS[name], (name, len(k))
    assert np.isfinite(slope).all(), (name, slope)
    cg = R.group_velocity(*R.jets(name, k, w))
    err = np.abs(cg - slope) / np.maximum(1.0, np.abs(slope))
    print(f"{name}: {len(k)} roots, worst |c_g - slope| / max(1, |slope|) = {err.max():.2e} (bound {R.slope_bound(name):.1e})")
    assert err.max() <= R.slope_bound(name), (name, err)


def test_tangent_against_difference_quotient_at_the_artefact_roots():
    """CR_kink: where a root sits beside the zero of the far-field K-coefficient, the central difference of D at relative step
    1e-7 misses the curve slope by up to 6e-4; the tangent is held to the bound of the case there too, and is asked to be at
    least 1e6 times closer than the difference quotient at the root where that one is worst (measured: 6e8)."""
    name = "CR_kink"
    eq, mode, m, _ = M.all_cases()[name]
    port = cases.port_problem(eq, mode, m)
    k, w, slope = R.curve_slopes(name)
    cg = R.group_velocity(*R.jets(name, k, w))
    fd = np.empty(len(k))
    for j in range(len(k)):
        hk, hw = 1e-7 * k[j], 1e-7 * w[j]
        Dk = (port.eval_one(k[j] + hk, w[j])[1] - port.eval_one(k[j] - hk, w[j])[1]) / (2 * hk)
        Dw = (port.eval_one(k[j], w[j] + hw)[1] - port.eval_one(k[j], w[j] - hw)[1]) / (2 * hw)
        fd[j] = -Dk / Dw
    e_fd = np.abs(fd - slope) / np.maximum(1.0, np.abs(slope))
    e_tl = np.abs(cg - slope) / np.maximum(1.0, np.abs(slope))
    for j in range(len(k)):
        print(f"k {k[j]:.2f} W {w[j] / k[j]:.5f}: slope {slope[j]:.9f}, difference quotient off by {e_fd[j]:.1e}, tangent by "
              f"{e_tl[j]:.1e}")
    j = int(np.argmax(e_fd))
    assert e_fd[j] > 1e-4                                   # the artefact is there (5.7e-4)
    assert e_tl[j] <= 1e-6 * e_fd[j]


def test_hermite_branch_reproduces_a_cubic():
    from eigensolver_amd import postprocess as pp
    c = np.array([0.3, -1.1, 2.0, 0.7])                     # omega = 0.3 k^3 - 1.1 k^2 + 2 k + 0.7
    pol, dpol = np.poly1d(c), np.poly1d(c).deriv()
    ks = np.array([0.8, 1.1, 1.9, 2.0, 3.6])                # uneven nodes
    f = pp.hermite_branch(ks, pol(ks), dpol(ks))
    x = np.array([0.8, 0.95, 1.5, 1.97, 2.0, 2.71, 3.6, 0.5, 4.0])      # nodes, off-node points, both continuations
    assert np.max(np.abs(f(x) - pol(x))) <= 1e-14 * np.max(np.abs(pol(x)))
    assert np.max(np.abs(f(x, nu=1) - dpol(x))) <= 1e-13 * np.max(np.abs(dpol(x)))
    assert float(f(1.5)) == pytest.approx(float(pol(1.5)), rel=1e-14)  # scalar in, scalar-shaped out
    assert np.ndim(f(1.5)) == 0
    with pytest.raises(ValueError):
        pp.hermite_branch([1.0, 1.0, 2.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        pp.hermite_branch([1.0], [1.0], [0.0])


Sig = namedtuple("Sig", "nodes_value nodes_flux status")
Slo = namedtuple("Slo", "group_velocity status")


def test_curves_with_slopes_on_hand_made_arrays():
    from eigensolver_amd import postprocess as pp
    nan = float("nan")
    roots = dict(k=np.array([2.0, 1.0, 1.0, 3.0, 2.0, 1.5, 0.5, 2.5]), w=np.array([5.0, 2.5, 4.0, 7.0, 8.0, 3.0, 1.0, 6.0]),
                 flag=np.array([1, 1, 1, 1, 1, 0, 1, 1], dtype=np.uint8))
    sig = Sig(np.array([0, 0, 1, 0, 1, 0, -1, 0], dtype=np.int32), np.array([0, 0, 1, 0, 1, 0, -1, 0], dtype=np.int32),
              np.array([0, 0, 0, 0, 0, 0, 1, 0], dtype=np.uint8))
    slo = Slo(np.array([0.2, 0.1, 1.1, 0.3, 1.2, 0.15, nan, nan]), np.array([0, 0, 0, 0, 0, 0, 1, 2], dtype=np.uint8))
    out = pp.curves_with_slopes(roots, sig, slo)
    assert sorted(out) == [(0, 0), (1, 1)]                  # flag 0, the leaky pair and the pair the slopes call refused are gone
    w, k, cg = out[(0, 0)]
    assert w.tolist() == [2.5, 5.0, 7.0] and k.tolist() == [1.0, 2.0, 3.0] and cg.tolist() == [0.1, 0.2, 0.3]   # aligned, k-sorted
    w, k, cg = out[(1, 1)]
    assert w.tolist() == [4.0, 8.0] and k.tolist() == [1.0, 2.0] and cg.tolist() == [1.1, 1.2]
    everything = pp.curves_with_slopes(roots, sig, slo, accepted_only=False)
    assert sorted(everything) == [(-1, -1), (0, 0), (1, 1)]
    assert everything[(0, 0)][1].tolist() == [1.0, 1.5, 2.0, 2.5, 3.0]
    assert everything[(0, 0)][2][:3].tolist() == [0.1, 0.15, 0.2] and np.isnan(everything[(0, 0)][2][3])
    f = pp.hermite_branch(out[(0, 0)][1], out[(0, 0)][0], out[(0, 0)][2])                # ready for hermite_branch
    assert float(f(2.0)) == 5.0
    empty = dict(k=np.array([]), w=np.array([]), flag=np.array([], dtype=np.uint8))
    none = Sig(np.array([], dtype=np.int32), np.array([], dtype=np.int32), np.array([], dtype=np.uint8))
    assert pp.curves_with_slopes(empty, none, Slo(np.array([]), np.array([], dtype=np.uint8))) == {}

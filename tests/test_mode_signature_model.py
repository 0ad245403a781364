"""CPU side of es_shoot_mode_signature (include/eigensolver_amd.h section 10): the entry point exists, the ABI pins hold, the
count rule labels the dispersion branches of the C port's roots, every pair tests/test_mode_signature_gpu.py uses has a count
that rounding cannot change, and postprocess.split_by_signature cuts a table by label.  No GPU.

Figures of the NumPy model (python -m pytest tests/test_mode_signature_model.py -s prints them): the smallest non-zero entry of
every row over max|row|, and per branch case the labels with their phase-speed and peak ranges.
"""
import ctypes
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from tests import mode_signature_model as S
from tests import real_eigen_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from eigensolver_amd import build
    return ctypes.CDLL(build.build())


def test_header_declares_and_library_exports_the_entry():
    txt = open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+es_shoot_mode_signature\s*\(", txt)
    assert hasattr(_lib(), "es_shoot_mode_signature")


def test_abi_pins_are_unchanged():
    lib = _lib()
    lib.es_abi_version.restype = ctypes.c_int
    lib.es_abi_sizeof.restype = ctypes.c_int
    lib.es_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.es_abi_version() == 1
    assert lib.es_abi_sizeof(8) == -1                     # plain arrays: no new ABI struct


def test_count_rule_and_decided_on_hand_made_rows():
    nan = float("nan")
    assert S.count([0.0, 1.0, 2.0, -1.0, 0.0, -3.0, nan, 4.0]) == 2       # zeros and NaNs are skipped, not counted
    assert S.count([0.0, 0.0, nan]) == 0 and S.count([]) == 0 and S.count([-2.0]) == 0
    assert S.count([1.0, 0.0, -1.0]) == 1 and S.count([1.0, nan, 1.0]) == 0
    assert S.peak([1.0, -3.0, 3.0, 2.0]) == (3.0, 1)                      # the smallest index that attains the maximum
    assert S.decided([1.0, 1e-12, -1.0]) and S.decided([1.0, -1e-12, -1.0])
    assert S.decided([0.0, 1.0, 0.0, -1.0])                               # exact zeros need no flank
    assert not S.decided([1.0, 1e-12, 1.0])                               # same sign on both sides: 0 or 2 changes
    assert not S.decided([1e-12, 1.0, -1.0]) and not S.decided([1.0, -1.0, 1e-12])     # no flank at an end
    assert not S.decided([1.0, 1e-12, 1e-13, -1.0])                       # two tiny entries may take different signs
    assert S.decided([1.0, 1e-12, 0.0, nan, -1.0])
    # whichever sign the tiny entry of a decided row takes, the count is the same
    assert S.count([1.0, 1e-12, -1.0]) == S.count([1.0, -1e-12, -1.0]) == S.count([1.0, 0.0, -1.0]) == 1


@pytest.mark.parametrize("name", S.MODEL_CASES)
def test_every_pair_of_the_gpu_test_is_decided(name):
    """The cap on left-out pairs is zero: all N_PAIRS pairs of the case, and all port roots where roots are labelled."""
    pairs = S.all_pairs(name)
    assert len(pairs) >= M.N_PAIRS
    tiniest = np.inf
    for k, w in pairs:
        s = S.signature(name, k, w)
        assert np.isfinite(s.value).all() and np.isfinite(s.flux).all(), (name, k, w)
        for row in (s.value, s.flux):
            nz = np.abs(row[row != 0.0])
            tiniest = min(tiniest, float(nz.min() / nz.max()))
        assert S.pair_decided(name, k, w), (name, k, w)
    print(f"{name}: {len(pairs)} pairs, smallest non-zero |entry| / max|row| = {tiniest:.1e}")


@pytest.mark.parametrize("name", sorted(S.BRANCHES))
def test_labels_follow_the_branches_of_the_port_roots(name):
    """Accepted, cpu_ok roots of the C port on the 8 x 400 grid: the label set is the case's, omega increases with the label
    inside a row, and the pressure peaks on the interface (peak_value 1.0 at node 0) for the (0, 0) kink branch and no other."""
    k, w, row = S.port_roots(name)
    sigs = [S.signature(name, float(a), float(b)) for a, b in zip(k, w)]
    labels = [s.label for s in sigs]
    assert set(labels) == S.BRANCHES[name], (name, sorted(set(labels)))
    for lab in sorted(set(labels)):
        sel = [i for i, l in enumerate(labels) if l == lab]
        W = [w[i] / k[i] for i in sel]
        pk = [sigs[i].peak_value for i in sel]
        print(f"{name} {lab}: {len(sel)} roots, rows {sorted(set(int(row[i]) for i in sel))}, W {min(W):.3f}-{max(W):.3f}, "
              f"peak_value {min(pk):.3g}-{max(pk):.3g}")
    for r in sorted(set(row.tolist())):
        sel = sorted((i for i in range(len(k)) if row[i] == r), key=lambda i: w[i])
        labs = [labels[i] for i in sel]
        assert labs == sorted(labs) and len(set(labs)) == len(labs), (name, r, labs)     # one root per label, omega rising
    if name == "CF_flow_kink_N130":
        # the boundary value is the state marched out from the axis, +-1 up to the rounding of the two marches (1.0000000000000002
        # in the model): 1e-10, bound b of tests/test_eigenfunction_gpu.py
        for s in sigs:
            surface = s.peak_node_value == 0 and abs(s.peak_value - 1.0) <= 1e-10
            assert surface == (s.label == (0, 0)), (s.label, s.peak_value, s.peak_node_value)


Sig = namedtuple("Sig", "nodes_value nodes_flux status")


def test_split_by_signature_on_hand_made_arrays():
    from eigensolver_amd import postprocess as pp
    roots = dict(k=np.array([2.0, 1.0, 1.0, 3.0, 2.0, 1.5, 0.5]), w=np.array([5.0, 2.5, 4.0, 7.0, 8.0, 3.0, 1.0]),
                 flag=np.array([1, 1, 1, 1, 1, 0, 1], dtype=np.uint8))
    sig = Sig(np.array([0, 0, 1, 0, 1, 0, -1], dtype=np.int32), np.array([0, 0, 1, 0, 1, 0, -1], dtype=np.int32),
              np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.uint8))
    out = pp.split_by_signature(roots, sig)
    assert sorted(out) == [(0, 0), (1, 1)]                                 # flag 0 and the leaky pair are gone
    assert out[(0, 0)][0].tolist() == [2.5, 5.0, 7.0] and out[(0, 0)][1].tolist() == [1.0, 2.0, 3.0]      # sorted by k
    assert out[(1, 1)][0].tolist() == [4.0, 8.0] and out[(1, 1)][1].tolist() == [1.0, 2.0]
    everything = pp.split_by_signature(roots, sig, accepted_only=False)
    assert sorted(everything) == [(-1, -1), (0, 0), (1, 1)]
    assert everything[(0, 0)][1].tolist() == [1.0, 1.5, 2.0, 3.0] and everything[(-1, -1)][0].tolist() == [1.0]
    # ready for fit_branch and pickle_layout
    assert pp.fit_branch(out[(1, 1)][1], out[(1, 1)][0], deg=1)(1.5) == pytest.approx(6.0)
    assert len(pp.pickle_layout({"kink": out[(1, 1)]})) == 2
    empty = dict(k=np.array([]), w=np.array([]), flag=np.array([], dtype=np.uint8))
    none = Sig(np.array([], dtype=np.int32), np.array([], dtype=np.int32), np.array([], dtype=np.uint8))
    assert pp.split_by_signature(empty, none) == {} and pp.split_by_signature(empty, none, accepted_only=False) == {}

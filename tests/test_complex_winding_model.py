"""tests/complex_winding_model.py (the plain cell rule the GPU root search is compared with) against the candidate set of
oracle/slab_complex.py::ComplexFlowSlab.find_roots on a grid of tests/test_complex_roots_gpu.py, and on hand-made cells."""
import numpy as np
import pytest

from oracle.slab_complex import ComplexFlowSlab
from tests.complex_winding_model import cell_total, corner_quadrants, flagged_cells

K = (0.3, 0.5, 0.8)
W_RE, W_IM = np.linspace(-0.5, 1.0, 16), np.linspace(-0.25, 0.25, 12)


def oracle_candidates(o, k, w_re, w_im):
    """The `cand` mask of ComplexFlowSlab.find_roots, recomputed from eval_rk4 with the oracle's own vectorised steps."""
    W = w_re[None, :] + 1j * w_im[:, None]
    d, rel, st = o.eval_rk4(k, W.ravel())
    d, st = d.reshape(W.shape), st.reshape(W.shape)
    q = o._quadrant(d)

    def turns(a, b):
        t = (b - a) & 3
        return np.where(t == 0, 0, np.where(t == 1, 1, np.where(t == 3, -1, 8)))

    q00, q10, q11, q01 = q[:-1, :-1], q[:-1, 1:], q[1:, 1:], q[1:, :-1]
    total = turns(q00, q10) + turns(q10, q11) + turns(q11, q01) + turns(q01, q00)
    okc = (st[:-1, :-1] == 0) & (st[:-1, 1:] == 0) & (st[1:, 1:] == 0) & (st[1:, :-1] == 0)
    cand = okc & ((total == 4) | (total == -4) | (total >= 6))
    return d, st, [(int(a), int(b)) for a, b in zip(*np.nonzero(cand))]


@pytest.mark.parametrize("width,mode,variant", [(0.9, "sausage", "sfg"), (1e5, "kink", "sfx")])
def test_model_is_the_oracles_candidate_rule(width, mode, variant):
    o = ComplexFlowSlab(width=width, mode=mode, variant=variant, n_nodes=130)
    D, S, want = [], [], []
    for row, k in enumerate(K):
        d, st, cells = oracle_candidates(o, k, k * W_RE, k * W_IM)
        D.append(d)
        S.append(st)
        want += [(row, a, b) for a, b in cells]
    got = flagged_cells(np.array(D), np.array(S))
    assert got == want
    assert len(got) >= 5 and len({c[0] for c in got}) == len(K)        # every row contributes: the row index is exercised
    # and the oracle's find_roots returns one record per such cell, in this order
    ro, relo, flo = o.find_roots(K[0], K[0] * W_RE, K[0] * W_IM, n_iter=0)
    assert len(ro) == sum(1 for c in got if c[0] == 0)


def cell(z00, z10, z11, z01, st=(0, 0, 0, 0)):
    D = np.array([[[z00, z10], [z01, z11]]], dtype=complex)
    S = np.array([[[st[0], st[1]], [st[3], st[2]]]], dtype=np.uint8)
    return D, S


def test_hand_made_cells():
    # one turn either way
    assert flagged_cells(*cell(1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j)) == [(0, 0, 0)]
    assert cell_total(*[a.tolist() for a in cell(1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j)], 0, 0, 0) == 4
    assert cell_total(*[a.tolist() for a in cell(1 + 1j, 1 - 1j, -1 - 1j, -1 + 1j)], 0, 0, 0) == -4
    assert flagged_cells(*cell(1 + 1j, 1 - 1j, -1 - 1j, -1 + 1j)) == [(0, 0, 0)]
    # no turn, and there-and-back
    assert flagged_cells(*cell(1 + 1j, 1 + 1j, 1 + 1j, 1 + 1j)) == []
    assert flagged_cells(*cell(1 + 1j, -1 + 1j, 1 + 1j, -1 + 1j)) == []
    # a half-turn edge counts 8: 8 + 8 = 16 and 8 - 1 - 1 + 0 = 6 are flagged
    assert flagged_cells(*cell(1 + 1j, -1 - 1j, 1 + 1j, 1 + 1j)) == [(0, 0, 0)]
    assert cell_total(*[a.tolist() for a in cell(1 + 1j, -1 - 1j, -1 + 1j, 1 + 1j)], 0, 0, 0) == 6
    assert flagged_cells(*cell(1 + 1j, -1 - 1j, -1 + 1j, 1 + 1j)) == [(0, 0, 0)]
    # -0.0 is non-negative: the same cell as its +0.0 twin, and not the one with a negative part
    nz = complex(-0.0, -0.0)
    assert flagged_cells(*cell(nz, -1 + 1j, -1 - 1j, 1 - 1j)) == [(0, 0, 0)]
    assert flagged_cells(*cell(nz, nz, nz, nz)) == []
    # a corner that is not ES_PT_OK removes the cell, whichever corner it is
    for j in range(4):
        st = [0, 0, 0, 0]
        st[j] = 1 + j % 3
        assert flagged_cells(*cell(1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j, st)) == []
    # a NaN part compares false with >= 0, like a negative one
    assert flagged_cells(*cell(1 + 1j, complex(np.nan, 1), -1 - 1j, 1 - 1j)) == [(0, 0, 0)]
    # one row or one column: no cells
    assert flagged_cells(np.ones((2, 1, 5), complex), np.zeros((2, 1, 5), np.uint8)) == []
    assert flagged_cells(np.ones((2, 5, 1), complex), np.zeros((2, 5, 1), np.uint8)) == []
    assert corner_quadrants(*cell(1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j)) == {(0, 1, 2, 3)}

"""tests/bracket_model.py against the C port of the root search (oracle/c/shoot_port.c: port_find_roots) on arrays that no
determinant produced, and the conditions the model's array makers have to meet.  No GPU."""
import dataclasses

import numpy as np
import pytest

from tests import bracket_model as bm
from tests import cases

FAMILIES = ("CF_flow_kink", "SD_w15_kink", "CR_kink")
SHAPES = ((5, 65), (3, 257))
N_NODES = 33            # the marches cost nothing; the status of the windows does not depend on it
_PORT = {}


def port(name):
    if name not in _PORT:
        eq, mode, m, _ = cases.all_cases()[name]
        _PORT[name] = cases.port_problem(dataclasses.replace(eq, n_nodes=N_NODES), mode, m)
    return _PORT[name]


@pytest.mark.parametrize("name", FAMILIES)
def test_dead_window_is_dead(name):
    """The premise of expected_table: every point with phase speed in DEAD_WINDOW is ES_PT_LEAKY with D = rel = NaN."""
    k = np.linspace(*bm.K_RANGE, 19)
    W = np.linspace(*bm.DEAD_WINDOW, 81)
    D, rel, st = port(name).eval_grid(k, W, w_mode=bm.W_PHASE_SPEED)
    assert np.all(st == bm.PT_LEAKY) and np.isnan(D).all() and np.isnan(rel).all()
    for w_mode in (bm.W_ABSOLUTE, bm.W_PER_ROW):                        # the grids make_grid hands out
        kk, WW = bm.make_grid(7, 33, w_mode, 3)
        D, rel, st = port(name).eval_grid(kk, WW, w_mode=w_mode)
        assert np.all(st == bm.PT_LEAKY) and np.isnan(D).all()


def test_live_window_is_live():
    k = np.linspace(*bm.K_RANGE, 19)
    W = np.linspace(*bm.LIVE_WINDOW, 81)
    D, rel, st = port("CF_flow_kink").eval_grid(k, W, w_mode=bm.W_PHASE_SPEED)
    assert np.all(st == bm.PT_OK) and np.isfinite(D).all()


@pytest.mark.parametrize("shape", bm.WILD_CHECKED, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wild_arrays_hold_the_pairs_worth_having(shape):
    D, st = bm.make("wild", *shape)
    got = bm.wild_conditions(D, st)
    assert all(got.values()), got
    assert np.count_nonzero(bm.brackets(D, st)) >= 20
    assert set(np.unique(st).tolist()) == set(bm.WILD_STATUS.tolist())


@pytest.mark.parametrize("nk,nw", [(1, 1), (1, 2), (3, 63), (3, 64), (64, 65), (5, 255), (5, 256), (5, 257), (2, 1024),
                                   (3, 87500)])
def test_makers(nk, nw):
    cells = nk * nw
    D, st = bm.dense(nk, nw)
    assert np.count_nonzero(bm.brackets(D, st)) == nk * (nw - 1)
    assert np.all(D.reshape(-1)[:-1] * D.reshape(-1)[1:] < 0)          # the sign changes across every row end as well
    D, st = bm.none(nk, nw)
    assert np.count_nonzero(bm.brackets(D, st)) == 0
    D, st = bm.edges(nk, nw)
    got = np.flatnonzero(bm.brackets(D, st).reshape(-1))
    want = bm.edge_cells(nk, nw)
    assert np.array_equal(got, want)
    lane63 = np.arange(63, cells, 64)
    lane63 = lane63[lane63 % nw != nw - 1]
    assert np.all(np.isin(lane63, got)) and np.all((got % 64 == 63) | (got == 0) | (got == cells - 2))
    if nw > 1:
        assert 0 in got and cells - 2 in got
        seam = np.arange(nw - 1, cells - 1, nw)
        assert np.all(D.reshape(-1)[seam] * D.reshape(-1)[seam + 1] < 0)
    seam256 = np.arange(255, cells, 256)
    assert np.all(np.isin(seam256[seam256 % nw != nw - 1], got))
    for w_mode in (bm.W_ABSOLUTE, bm.W_PHASE_SPEED, bm.W_PER_ROW):
        k, W = bm.make_grid(nk, nw, w_mode, 1)
        row, j = np.divmod(np.arange(cells), nw)
        w = bm.pick_w(W, w_mode, k, row, j).reshape(nk, nw)
        assert np.all(np.diff(w, axis=1) > 0)
        speed = w / k[:, None]
        assert speed.min() >= bm.DEAD_WINDOW[0] and speed.max() <= bm.DEAD_WINDOW[1]
        assert k.min() >= bm.K_RANGE[0] and k.max() <= bm.K_RANGE[1]
        if nk >= 3:
            assert not (np.all(np.diff(k) > 0) or np.all(np.diff(k) < 0))
        if w_mode == bm.W_PER_ROW and nk > 1:
            assert len({w[r, 0] for r in range(nk)}) == nk


def test_ulp_distance():
    a = np.array([1.0, -1.0, 0.0, 5e-324, np.nan, np.nan, np.inf, 1e308, 3.0])
    b = np.array([np.nextafter(1.0, 2.0), -1.0, -0.0, -5e-324, np.nan, 1.0, np.inf, -1e308, np.nextafter(3.0, 0.0)])
    assert bm.ulp_distance(a, b).tolist() == [1, 0, 0, 2, 0, 2 ** 62, 0, 2 ** 62, 1]


def test_screened_model_by_hand():
    """One row of eight points, worked by hand.  Screened values: + - | + + - u u +, the two unsure points hold garbage;
    fp64 at the unsure points: - and LEAKY; fp64 at the ends confirms only the bracket of cells 3 | 4."""
    U = bm.UNSURE
    D_in = np.array([[1.0, -1.0, 2.0, 3.0, -2.0, 7e77, -7e77, 1.0]])
    st_in = np.array([[0, 0, 0, 0, 0, U | 0, U | 2, 0]], dtype=np.uint8)
    D_eval = np.array([[9.0, 9.0, 9.0, 9.0, 9.0, -4.0, np.nan, 9.0]])
    st_eval = np.array([[3, 3, 3, 3, 3, 0, 1, 3]], dtype=np.uint8)
    D_ends = np.array([[1.0, 1.0, 1.0, 1.0, -1.0, -1.0, np.nan, 1.0]])
    st_ends = np.array([[0, 0, 0, 0, 0, 0, 1, 0]], dtype=np.uint8)
    Dm, stm, counts, b = bm.screened_model(D_in, st_in, D_eval, st_eval, D_ends, st_ends, capacity=8)
    assert np.array_equal(Dm[0, :6], [1.0, -1.0, 2.0, 3.0, -2.0, -4.0]) and np.isnan(Dm[0, 6]) and Dm[0, 7] == 1.0
    assert stm.tolist() == [[0, 0, 0, 0, 0, 0, 1, 0]]
    assert np.flatnonzero(b).tolist() == [0, 1, 3]                      # 4 | 5 is - -, 5 | 6 and 6 | 7 touch the leaky point
    assert counts == (3, 2, 6, 2)
    assert bm.screened_model(D_in, st_in, D_eval, st_eval, D_ends, st_ends, capacity=2)[2] == (3, 2, 4, 2)
    assert bm.screened_model(D_in, st_in, D_eval, st_eval, D_ends, st_ends, capacity=0)[2] == (3, 2, 0, 0)


@pytest.mark.parametrize("pattern", ["wild", "dense", "edges"])
@pytest.mark.parametrize("nk,nw", SHAPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_port_table_is_the_model(name, nk, nw, pattern):
    """port_find_roots in the dead window with n_bisect = 0, all three w_modes: row, k, w_lo, w_hi and flag exact, resid NaN,
    w within 2 ulp of the secant rule (three roundings, |q| <= |hi - lo|: a contraction can move the last bit at most)."""
    D, st = bm.make(pattern, nk, nw)
    worst = 0
    for w_mode in (bm.W_ABSOLUTE, bm.W_PHASE_SPEED, bm.W_PER_ROW):
        k, W = bm.make_grid(nk, nw, w_mode, seed=nk + nw)
        want = bm.expected_table(D, st, k, W, w_mode)
        got, n = port(name).find_roots(k, W, D, st, w_mode=w_mode, n_bisect=0, capacity=nk * nw)
        assert n == want["cell"].size and n >= (20 if pattern == "wild" else 7)
        for col in ("row", "k", "w_lo", "w_hi", "flag"):
            assert got[col].tobytes() == want[col].tobytes(), (w_mode, col)
        assert np.isnan(got["resid"]).all()
        ulp = bm.ulp_distance(got["w"], want["w"])
        worst = max(worst, int(ulp.max()))
        assert ulp.max() <= 2, (w_mode, int(ulp.max()))
        assert np.all((got["w"] >= got["w_lo"]) & (got["w"] <= got["w_hi"]))
    if pattern == "wild":
        assert set(np.unique(want["branch"]).tolist()) == {0, 1, 2}     # all three branches of es_secant_point
    print(f"{name} {nk}x{nw} {pattern}: brackets {n}, max ulp distance of w {worst}")

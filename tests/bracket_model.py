"""NumPy model of the bracket stage of the real root search (es_shoot_find_roots, es_shoot_find_roots_screened and their
_async forms) on arrays that no determinant produced, and the makers of such arrays.

Where every evaluation of the refinement returns NaN (the "dead window" below) and n_bisect = 0, the ES_REFINE_POLISH
secant steps leave the bracket untouched (es_secant_update ignores a NaN), so the whole root table is a closed function
of the input arrays: for the i-th flagged cell (row r, column j) in row-major order
    row = r, k = k[r], w_lo = pick_w(j), w_hi = pick_w(j + 1), w = es_secant_point(w_lo, w_hi, D[r, j], D[r, j + 1]),
    flag = 0, resid = NaN.
Written from include/eigensolver_amd.h and es_refine_rule.hpp, array-wise; the bracket predicate is the one of
screen_audit_model.brackets."""
import numpy as np

from tests.screen_audit_model import PT_OK, UNSURE, brackets

PT_LEAKY = 1
W_ABSOLUTE, W_PHASE_SPEED, W_PER_ROW = 0, 1, 2
COLUMNS = ("k", "w", "w_lo", "w_hi", "resid", "row", "flag")

# Phase speeds at which CF_flow_kink, SD_w15_kink and CR_kink (tests/cases.py) are ES_PT_LEAKY with D = NaN for every k in
# K_RANGE, and the window of CF_flow_kink that is ES_PT_OK throughout for the same k.
DEAD_WINDOW = (5.2, 6.0)
LIVE_WINDOW = (2.7, 4.95)
K_RANGE = (0.3, 3.9)
# W_ABSOLUTE has one frequency vector for all rows: k in K_ABSOLUTE and omega in W_ABSOLUTE_RANGE keep omega / k in DEAD_WINDOW
K_ABSOLUTE = (1.0, 1.1)
W_ABSOLUTE_RANGE = (5.2 * 1.1, 6.0 * 1.0)

WILD_VALUES = np.array([1.0, -1.0, 0.0, -0.0, 5e-324, -5e-324, 1e-200, -1e-200, 1e200, -1e200, np.inf, -np.inf, np.nan,
                        2.5, -0.75])
WILD_STATUS = np.array([0, 0, 0, 0, 0, 0, 1, 2, 3, 0x80, 0x81], dtype=np.uint8)


# ---- the model ----------------------------------------------------------------------------------------------------
def pick_w(W, w_mode, k, row, j):
    """omega of column j of row `row` (arrays of equal length), as the header defines the three modes."""
    W = np.asarray(W, dtype=np.float64)
    if w_mode == W_PHASE_SPEED:
        return np.asarray(k, dtype=np.float64)[row] * W.reshape(-1)[j]
    if w_mode == W_PER_ROW:
        return W[row, j]
    assert w_mode == W_ABSOLUTE
    return W.reshape(-1)[j]


def secant_point(lo, hi, flo, fhi):
    """es_secant_point, and the branch taken: 0 the secant point, 1 stay at the end with the smaller |f|, 2 the mid-point."""
    with np.errstate(all="ignore"):
        x = lo - flo * (hi - lo) / (fhi - flo)
        inside = (x > lo) & (x < hi)
        end = np.where(np.abs(flo) <= np.abs(fhi), lo, hi)
        mid = lo + (hi - lo) * 0.5
    nan = np.isnan(x)
    return np.where(inside, x, np.where(nan, mid, end)), np.where(inside, 0, np.where(nan, 2, 1))


def expected_table(D, st, k, W, w_mode, D_ends=None):
    """The root table of a dead-window search with n_bisect = 0: a dict of the seven columns plus `cell` (flat index of the
    lower end) and `branch` (see secant_point), one entry per bracket of (D, st) in row-major order.  D_ends: the values
    the refinement starts from, where they are not D itself (the screened search replaces them by its fp64 evaluation of
    the bracket ends)."""
    D = np.asarray(D, dtype=np.float64)
    nk, nw = D.shape
    cell = np.flatnonzero(brackets(D, st).reshape(-1))
    row, j = cell // nw, cell % nw
    k = np.asarray(k, dtype=np.float64).reshape(-1)
    w_lo, w_hi = pick_w(W, w_mode, k, row, j), pick_w(W, w_mode, k, row, j + 1)
    F = D if D_ends is None else np.asarray(D_ends, dtype=np.float64)
    w, branch = secant_point(w_lo, w_hi, F.reshape(-1)[cell], F.reshape(-1)[cell + 1])
    n = cell.size
    return dict(k=k[row], w=w, w_lo=w_lo, w_hi=w_hi, resid=np.full(n, np.nan), row=row.astype(np.int32),
                flag=np.zeros(n, dtype=np.uint8), cell=cell, branch=branch)


def screened_model(D_in, st_in, D_eval, st_eval, D_ends, st_ends, capacity):
    """es_shoot_find_roots_screened on the screened arrays (D_in, st_in).  D_eval, st_eval: what the fp64 point evaluation
    gives at every grid point (read at the unsure points); D_ends, st_ends: what it gives at the bracket ends, as grid
    arrays as well (the ends of a bracket are grid points).  Returns (merged D, merged status, the four count words,
    bracket mask of the merged arrays)."""
    D_in, st_in = np.asarray(D_in, dtype=np.float64), np.asarray(st_in, dtype=np.uint8)
    unsure = (st_in & UNSURE) != 0
    Dm = np.where(unsure, D_eval, D_in)
    stm = np.where(unsure, st_eval, st_in).astype(np.uint8)
    b = brackets(Dm, stm)
    cell = np.flatnonzero(b.reshape(-1))
    written = cell[:min(cell.size, capacity)]
    confirmed = brackets(D_ends, st_ends).reshape(-1)
    counts = (int(cell.size), int(np.count_nonzero(unsure)), 2 * int(written.size),
              int(np.count_nonzero(~confirmed[written])))
    return Dm, stm, counts, b


def ulp_distance(a, b):
    """Distance of two float64 arrays in units of the last place (0 where both are NaN, 2^62 where one is)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)

    def ordered(x):
        i = x.view(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 63)) - i, i)           # -0.0 -> 0, monotone in x

    na, nb = np.isnan(a), np.isnan(b)
    ia, ib = ordered(np.where(na, 0.0, a)), ordered(np.where(nb, 0.0, b))
    opposite = (ia < 0) != (ib < 0)
    # same sign: the difference fits; opposite signs: the sum of the magnitudes, formed without overflow
    apart = np.abs(ia).astype(np.uint64) + np.abs(ib).astype(np.uint64)
    d = np.where(opposite, np.minimum(apart, np.uint64(2 ** 62)).astype(np.int64), np.abs(ia - np.where(opposite, ia, ib)))
    return np.where(na | nb, np.where(na & nb, 0, 2 ** 62), np.minimum(d, 2 ** 62))


# ---- array makers, seeded -------------------------------------------------------------------------------------------
def make_k(nk, seed, k_range=K_RANGE):
    """nk distinct wavenumbers inside k_range, not monotonic from nk = 3 on."""
    rng = np.random.default_rng([seed, 101])
    k = rng.permutation(np.linspace(k_range[0], k_range[1], nk + 2)[1:-1])
    if nk >= 3 and (np.all(np.diff(k) > 0) or np.all(np.diff(k) < 0)):
        k[[0, 1]] = k[[1, 0]]
    return k


def make_grid(nk, nw, w_mode, seed):
    """(k, W) of a dead-window grid: omega / k inside DEAD_WINDOW at every point, omega increasing along every row.
    W_PER_ROW: every row has a window of its own, so the row index shows in w_lo."""
    lo, hi = DEAD_WINDOW
    frac = (np.arange(nw) + 0.5) / nw
    if w_mode == W_PHASE_SPEED:
        return make_k(nk, seed), lo + frac * (hi - lo)
    if w_mode == W_ABSOLUTE:
        return make_k(nk, seed, K_ABSOLUTE), W_ABSOLUTE_RANGE[0] + frac * (W_ABSOLUTE_RANGE[1] - W_ABSOLUTE_RANGE[0])
    rng = np.random.default_rng([seed, 202])
    k = make_k(nk, seed)
    a = rng.uniform(lo, lo + 0.3 * (hi - lo), nk)
    b = rng.uniform(hi - 0.3 * (hi - lo), hi, nk)
    return k, k[:, None] * (a[:, None] + frac[None, :] * (b - a)[:, None])


def _magnitudes(nk, nw, seed):
    return np.random.default_rng([seed, 303]).uniform(0.5, 2.0, (nk, nw))


def dense(nk, nw, seed=0):
    """Signs alternate along the flat index (so also across every row end), every status 0: nk * (nw - 1) brackets."""
    sign = 1.0 - 2.0 * (np.arange(nk * nw) & 1)
    return sign.reshape(nk, nw) * _magnitudes(nk, nw, seed), np.zeros((nk, nw), dtype=np.uint8)


def none(nk, nw, seed=0):
    """One sign, every status 0: no bracket."""
    return _magnitudes(nk, nw, seed), np.zeros((nk, nw), dtype=np.uint8)


def edge_cells(nk, nw):
    """The bracket cells of `edges`: every cell c = 63 mod 64 that is not in the last column (c = 255 mod 256 among them),
    the first cell, and cell (nk - 1, nw - 2) -- where nk * nw is a multiple of 64, the cell before the last."""
    if nw < 2:
        return np.zeros(0, dtype=np.int64)
    c = np.arange(63, nk * nw, 64, dtype=np.int64)
    c = c[c % nw != nw - 1]
    return np.unique(np.concatenate([c, [0, nk * nw - 2]]))


def edges(nk, nw, seed=0):
    """Brackets exactly at edge_cells; the sign also changes across every row end, where no bracket may be flagged."""
    cells = nk * nw
    flip = np.zeros(cells, dtype=bool)
    flip[edge_cells(nk, nw)] = True
    flip[nw - 1::nw] = True                                            # last column: sign change into the next row
    sign = np.ones(cells)
    sign[1:] = np.cumprod(1.0 - 2.0 * flip[:-1])
    return sign.reshape(nk, nw) * _magnitudes(nk, nw, seed), np.zeros((nk, nw), dtype=np.uint8)


def wild(nk, nw, seed=0):
    """Values from WILD_VALUES, statuses from WILD_STATUS (ES_PT_OK with weight 6 of 11)."""
    rng = np.random.default_rng([seed, 404])
    D = WILD_VALUES[rng.integers(0, WILD_VALUES.size, (nk, nw))]
    st = WILD_STATUS[rng.integers(0, WILD_STATUS.size, (nk, nw))]
    return D, st


PATTERNS = {"dense": dense, "none": none, "edges": edges, "wild": wild}

# seeds at which the wild array of a shape meets every condition of wild_conditions and has at least 20 brackets
# (found by search, asserted by test_bracket_model.py)
WILD_SEEDS = {(5, 65): 28, (3, 257): 2, (3, 63): 540, (3, 64): 60, (5, 256): 1, (2, 1024): 1}    # every other shape: 0
WILD_CHECKED = ((5, 65), (3, 257), (3, 63), (3, 64), (64, 65), (5, 255), (5, 256), (5, 257), (2, 1024), (24, 192),
                (3, 87500))


def make(pattern, nk, nw):
    """The array of a pattern at its seed.  A wild array is handed out only for a shape whose array test_bracket_model.py
    checks (WILD_CHECKED), or one of at most two cells, which cannot hold the pairs."""
    if pattern != "wild":
        return PATTERNS[pattern](nk, nw, 0)
    assert (nk, nw) in WILD_CHECKED or nk * nw <= 2, f"wild {nk} x {nw}: add the shape to WILD_CHECKED (and a seed that passes)"
    return wild(nk, nw, WILD_SEEDS.get((nk, nw), 0))


def wild_conditions(D, st):
    """Which of the adjacent pairs worth having occur (in either order) among the omega-neighbours with both statuses 0,
    each with the verdict the predicate must give on it."""
    D = np.asarray(D, dtype=np.float64)
    a, b = D[:, :-1], D[:, 1:]
    ok = (st[:, :-1] == PT_OK) & (st[:, 1:] == PT_OK)
    br = brackets(D, st)[:, :-1]

    def pair(x, y, is_bracket):
        hit = ok & (((a == x) & (b == y)) | ((a == y) & (b == x)))
        return bool(hit.any() and np.all(br[hit] == is_bracket))

    nan = ok & (np.isnan(a) | np.isnan(b))
    return {"(5e-324, -1) bracket": pair(5e-324, -1.0, True),
            "(1e-200, -1e-200) non-bracket": pair(1e-200, -1e-200, False),
            "(inf, -1) bracket": pair(np.inf, -1.0, True),
            "(1e200, -1e200) bracket": pair(1e200, -1e200, True),
            "(0, -1) non-bracket": pair(0.0, -1.0, False),
            "NaN neighbour": bool(nan.any() and not br[nan].any())}

"""The bracket stage of the real root search on arrays that no determinant produced: bracket_flag_kernel, the block scan,
bracket_emit_kernel, the unsure / bracket-end kernels of the screened search and the helpers of es_common.hpp, against
tests/bracket_model.py.  In the dead window (every evaluation NaN) with n_bisect = 0 the whole root table is a closed
function of D, status, k and omega, so every column is compared exactly (w within 2 ulp: three roundings, see the model)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from tests import bracket_model as bm

pytestmark = pytest.mark.gpu

N_NODES = 33                      # the marches cost nothing; the status of the two windows does not depend on it
SENT, SENT_ROW, SENT_FLAG = -12345.678, -77, 0xA5
EXACT = ("row", "k", "w_lo", "w_hi", "flag")
BIG = (3, 87500)                  # 262500 cells: 1026 scan blocks, the scan's second pass of 1024
ERR_CAPACITY, ERR_SCREENING = 3, 7
PAD = 8


# ---- plumbing ---------------------------------------------------------------------------------------------------------
def _problem(ctx, name):
    from eigensolver_amd import ShootProblem
    from tests import cases
    eq, mode, m, _ = cases.all_cases()[name]
    return ShootProblem(dataclasses.replace(eq, n_nodes=N_NODES), mode, m, ctx=ctx)


@pytest.fixture(scope="module")
def problems(es_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _problem(es_ctx, name)
        return made[name]

    yield get
    for gp in made.values():
        gp.close()


def _dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


def _table(gp, cap):
    """A root table that declares `cap` rows and owns PAD more, every row filled with sentinels: a row written at or
    behind the capacity shows, and stays inside the allocation."""
    from eigensolver_amd import _lib
    t, _ = gp.alloc_root_table(cap + PAD)
    for col in bm.COLUMNS:
        t[col].fill_({"row": SENT_ROW, "flag": SENT_FLAG}.get(col, SENT))
    return t, _lib.RootTable(*[t[col].data_ptr() for col in ("k", "w", "w_lo", "w_hi", "resid", "row", "flag")], cap)


def _host(t):
    return {col: v.cpu().numpy() for col, v in t.items()}


def _find_roots(gp, k, W, w_mode, D, st, cap, n_bisect=0):
    """es_shoot_find_roots called directly: (status, count, the whole table on the host)."""
    from eigensolver_amd import _lib
    dk, dw, nk, nw = gp._grid_args(k, W, w_mode)
    t, rt = _table(gp, cap)
    n = C.c_int(-1)
    rc = gp.ctx.lib.es_shoot_find_roots(gp.ctx.handle, gp.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw, w_mode, _lib.ptr(D),
                                        _lib.ptr(st), n_bisect, 1e-3, C.byref(rt), C.byref(n))
    return rc, n.value, _host(t)


def _find_roots_async(gp, k, W, w_mode, D, st, cap, n_bisect=0):
    import torch
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    table = _table(gp, cap)
    gp.find_roots_async(k, W, D, st, table, count, w_mode=w_mode, n_bisect=n_bisect)
    torch.cuda.synchronize()
    return int(count.item()), _host(table[0])


def _screened(gp, k, W, w_mode, D, st, cap, n_bisect):
    """es_shoot_find_roots_screened called directly, D and st merged in place: (status, the four counts, table)."""
    from eigensolver_amd import _lib
    dk, dw, nk, nw = gp._grid_args(k, W, w_mode)
    t, rt = _table(gp, cap)
    n, stats = C.c_int(-1), (C.c_int * 3)(-1, -1, -1)
    rc = gp.ctx.lib.es_shoot_find_roots_screened(gp.ctx.handle, gp.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw, w_mode,
                                                 n_bisect, 1e-3, _lib.ptr(D), _lib.ptr(st), C.byref(rt), C.byref(n), stats)
    return rc, (n.value, *stats), _host(t)


def _screened_async(gp, k, W, w_mode, D, st, cap, n_bisect):
    import torch
    counts = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    table = _table(gp, cap)
    gp.find_roots_screened_async(k, W, D, st, table, counts, w_mode=w_mode, n_bisect=n_bisect)
    torch.cuda.synchronize()
    return tuple(counts.cpu().tolist()), _host(table[0])


def _check_table(got, want, n, what):
    """The first n rows of the table `got` are the first n of the model's, every row behind them still holds the sentinels.
    Returns the largest ulp distance of w."""
    for col in EXACT:
        assert got[col][:n].tobytes() == want[col][:n].tobytes(), (what, col)
    assert np.isnan(got["resid"][:n]).all(), what
    ulp = bm.ulp_distance(got["w"][:n], want["w"][:n])
    worst = int(ulp.max()) if n else 0
    assert worst <= 2, (what, worst)
    _check_untouched(got, n, what)
    return worst


def _check_untouched(got, n, what):
    for col in bm.COLUMNS:
        sent = {"row": SENT_ROW, "flag": SENT_FLAG}.get(col, SENT)
        assert np.all(got[col][n:] == sent), (what, col, "written past the count")


def _same_rows(a, b, n, what):
    for col in bm.COLUMNS:
        assert a[col][:n].tobytes() == b[col][:n].tobytes(), (what, col)


def _same_array(got, want, what):
    """NaN masks first, then every other value bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        assert got[~nan].tobytes() == want[~nan].tobytes(), what
    else:
        assert got.tobytes() == want.tobytes(), what


@functools.lru_cache(maxsize=None)
def _dead_case(nk, nw, pattern, w_mode):
    """Inputs and the model's table, computed once: (k, W, D, st, table)."""
    k, W = bm.make_grid(nk, nw, w_mode, seed=nk + nw)
    D, st = bm.make(pattern, nk, nw)
    want = bm.expected_table(D, st, k, W, w_mode)
    for a in (D, st, *want.values()):
        a.setflags(write=False)
    return k, W, D, st, want


# ---- the premise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CF_flow_kink", "SD_w15_kink", "CR_kink"])
def test_dead_window_is_dead(problems, name):
    gp = problems(name)
    for w_mode, (k, W) in ((bm.W_PHASE_SPEED, (np.linspace(*bm.K_RANGE, 19), np.linspace(*bm.DEAD_WINDOW, 81))),
                           (bm.W_ABSOLUTE, bm.make_grid(7, 33, bm.W_ABSOLUTE, 3)),
                           (bm.W_PER_ROW, bm.make_grid(7, 33, bm.W_PER_ROW, 3))):
        D, st = gp.eval_grid(k, W, w_mode=w_mode)
        assert bool((st == bm.PT_LEAKY).all()) and bool(D.isnan().all()), w_mode


# ---- (a) es_shoot_find_roots against expected_table -------------------------------------------------------------------
SHAPES = [(1, 1), (1, 2), (3, 63), (3, 64), (64, 65), (5, 255), (5, 256), (5, 257), (2, 1024), BIG]
CASES_A = [("CF_flow_kink", s, p, bm.W_PHASE_SPEED) for s in SHAPES for p in ("dense", "edges", "wild")
           if not (s == BIG and p == "edges")]
CASES_A += [("CF_flow_kink", s, "none", bm.W_PHASE_SPEED) for s in ((3, 63), (5, 257))]
CASES_A += [("SD_w15_kink", (64, 65), p, bm.W_PHASE_SPEED) for p in ("dense", "edges", "wild")]
CASES_A += [("CF_flow_kink", s, p, m) for m in (bm.W_ABSOLUTE, bm.W_PER_ROW) for s in ((64, 65), (5, 257))
            for p in ("dense", "edges", "wild")]


def _id_a(c):
    return f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-w{c[3]}"


@pytest.mark.parametrize("case", CASES_A, ids=_id_a)
def test_table_is_the_model(problems, case):
    name, (nk, nw), pattern, w_mode = case
    k, W, D, st, want = _dead_case(nk, nw, pattern, w_mode)
    n = want["cell"].size
    assert n == {"dense": nk * (nw - 1), "none": 0}.get(pattern, n)
    rc, count, got = _find_roots(problems(name), k, W, w_mode, _dev(D), _dev(st), n + 19)
    assert (rc, count) == (0, n)
    worst = _check_table(got, want, n, case)
    print(f"{_id_a(case)}: brackets {n}, max ulp distance of w {worst}")


# ---- (b) capacity -------------------------------------------------------------------------------------------------------
def _capacities(n):
    return [n, n - 1, 1, 1000, n + 37, 0]


@pytest.mark.parametrize("which", range(6), ids=["count", "count-1", "1", "1000", "count+37", "0"])
@pytest.mark.parametrize("shape", [(5, 257), BIG], ids=["5x257", "3x87500"])
def test_capacity(problems, shape, which):
    """The count is the full one whatever the capacity, ES_ERR_CAPACITY exactly when it exceeds the capacity, the first
    min(count, capacity) rows are the model's, nothing behind them is written; capacity 1000 cuts a block of 256 flagged
    cells in its middle.  es_shoot_find_roots_async: the same rows bit for bit, the full count in its device word."""
    gp = problems("CF_flow_kink")
    k, W, D, st, want = _dead_case(*shape, "dense", bm.W_PHASE_SPEED)
    n = want["cell"].size
    cap = _capacities(n)[which]
    assert 1000 < n - 1 and 1000 % 256 not in (0, 255)
    dD, dst = _dev(D), _dev(st)
    rc, count, got = _find_roots(gp, k, W, bm.W_PHASE_SPEED, dD, dst, cap)
    assert count == n and rc == (ERR_CAPACITY if n > cap else 0), (rc, count, n, cap)
    count_a, got_a = _find_roots_async(gp, k, W, bm.W_PHASE_SPEED, dD, dst, cap)
    assert count_a == n
    m = min(n, cap)
    _check_table(got, want, m, ("sync", shape, cap))
    _check_untouched(got_a, m, ("async", shape, cap))
    _same_rows(got, got_a, m, ("sync / async", shape, cap))


# ---- (c) one context, calls of very different sizes ----------------------------------------------------------------------
def test_one_context_reused():
    """A large dense call, then small ones, then a large wild one on ONE fresh context: masks and block counts of an earlier,
    larger call must not reach a later table."""
    from eigensolver_amd import _lib
    ctx = _lib.Context(0)              # not es_ctx: the scratch of this context has seen nothing but the calls below
    gp = None
    try:
        gp = _problem(ctx, "CF_flow_kink")
        for (nk, nw), pattern in ((BIG, "dense"), ((3, 63), "wild"), ((1, 2), "dense"), ((5, 257), "edges"), (BIG, "wild"),
                                  ((5, 257), "none"), ((2, 1024), "dense")):
            k, W, D, st, want = _dead_case(nk, nw, pattern, bm.W_PHASE_SPEED)
            n = want["cell"].size
            rc, count, got = _find_roots(gp, k, W, bm.W_PHASE_SPEED, _dev(D), _dev(st), n + 5)
            assert (rc, count) == (0, n), (nk, nw, pattern)
            _check_table(got, want, n, (nk, nw, pattern))
    finally:
        if gp is not None:
            gp.close()
        ctx.close()


# ---- (d) the screened search in the dead window ---------------------------------------------------------------------------
def _unsure_mask(kind, nk, nw):
    cells = nk * nw
    if kind == "none":
        return np.zeros((nk, nw), dtype=bool)
    if kind == "all":
        return np.ones((nk, nw), dtype=bool)
    if kind == "random":
        return np.random.default_rng([nk, nw, 505]).random((nk, nw)) < 0.3
    assert kind == "lane63"
    m = np.zeros(cells, dtype=bool)
    m[63::64] = True
    m[-1] = True
    return m.reshape(nk, nw)


@pytest.mark.parametrize("w_mode", [bm.W_PHASE_SPEED, bm.W_PER_ROW], ids=["w1", "w2"])
@pytest.mark.parametrize("kind", ["none", "all", "random", "lane63"])
@pytest.mark.parametrize("shape", [(64, 65), (5, 257)], ids=["64x65", "5x257"])
def test_screened_dead_window(problems, shape, kind, w_mode):
    """Wild arrays with the unsure bit where `kind` says.  Every unsure point comes back NaN / ES_PT_LEAKY, the brackets are
    those of the merged arrays, both ends of every one evaluate to NaN: every bracket written is unconfirmed, the call
    returns ES_ERR_SCREENING with its counts filled in, and the refinement, started from NaN at both ends, reports the
    mid-point.  The async call gives the same arrays, counts and rows bit for bit."""
    nk, nw = shape
    gp = problems("CF_flow_kink")
    k, W, D0, st0, _ = _dead_case(nk, nw, "wild", w_mode)
    unsure = _unsure_mask(kind, nk, nw)
    st_in = np.where(unsure, st0 | bm.UNSURE, st0 & 0x7F).astype(np.uint8)
    dead_D, dead_st = np.full((nk, nw), np.nan), np.full((nk, nw), bm.PT_LEAKY, dtype=np.uint8)
    full = bm.screened_model(D0, st_in, dead_D, dead_st, dead_D, dead_st, nk * nw)[2][0]
    assert (full >= 20) == (kind != "all") and (full == 0) == (kind == "all")
    # kind "all": every point becomes ES_PT_LEAKY, so full = 0, the capacities are 1 and 5 and every table check below
    # compares zero rows -- the empty path: counts (0, cells, 0, 0), ES_SUCCESS, nothing written
    for cap in sorted({max(full, 1), 1, full + 5}):
        Dm, stm, counts, _ = bm.screened_model(D0, st_in, dead_D, dead_st, dead_D, dead_st, cap)
        m = min(full, cap)
        assert counts == (full, int(unsure.sum()), 2 * m, m)
        want = bm.expected_table(Dm, stm, k, W, w_mode, D_ends=dead_D)
        assert np.all(want["branch"] == 2)
        what = (shape, kind, w_mode, cap)
        Ds, sts = _dev(D0), _dev(st_in)
        rc, got_counts, got = _screened(gp, k, W, w_mode, Ds, sts, cap, 0)
        assert got_counts == counts, what
        assert rc == (ERR_SCREENING if m else 0), what
        _same_array(Ds.cpu().numpy(), Dm, what)
        _same_array(sts.cpu().numpy(), stm, what)
        _check_table(got, want, m, what)
        Da, sta = _dev(D0), _dev(st_in)
        counts_a, got_a = _screened_async(gp, k, W, w_mode, Da, sta, cap, 0)
        assert counts_a == counts, what
        _same_array(Da.cpu().numpy(), Dm, what)
        _same_array(sta.cpu().numpy(), stm, what)
        _check_untouched(got_a, m, what)
        _same_rows(got, got_a, m, what)


# ---- (e) the screened search in the live window ---------------------------------------------------------------------------
N_BISECT = 24


@functools.lru_cache(maxsize=None)
def _live_grid(nk, nw):
    lo, hi = bm.LIVE_WINDOW
    return bm.make_k(nk, nk + nw), lo + (np.arange(nw) + 0.5) * (hi - lo) / nw


def _flip_points(unsure, nw, rng):
    """Seven sure points: two of the form p = 0 mod 64 inside a row, five drawn."""
    flat = unsure.reshape(-1)
    halo = [p for p in range(64, flat.size, 64) if p % nw >= 1 and not flat[p]][:2]
    assert len(halo) == 2
    return np.unique(np.concatenate([halo, rng.choice(np.flatnonzero(~flat), size=5, replace=False)]))


@pytest.mark.parametrize("kind", ["random", "lane63"])
@pytest.mark.parametrize("shape", [(24, 192), (5, 257)], ids=["24x192", "5x257"])
def test_screened_live_window(problems, shape, kind):
    """The true fp64 grid with garbage at the unsure points: the screened search puts the true values back, confirms every
    bracket and returns the table of es_shoot_find_roots bit for bit.  Then sure points with their sign flipped, two of them
    the halo element of a lane-63 cell: counts and return code are the model's."""
    nk, nw = shape
    cells = nk * nw
    gp = problems("CF_flow_kink")
    k, W = _live_grid(nk, nw)
    Dt, stt = gp.eval_grid(k, W)
    D_true, st_true = Dt.cpu().numpy(), stt.cpu().numpy()
    assert np.all(st_true == bm.PT_OK) and np.isfinite(D_true).all() and np.all(D_true != 0)
    # what the fp64 point evaluation gives at every grid point: the model's unsure points and bracket ends
    row, j = np.divmod(np.arange(cells), nw)
    De, ste = gp.eval_points(k[row], bm.pick_w(W, bm.W_PHASE_SPEED, k, row, j))
    D_pts, st_pts = De.cpu().numpy().reshape(nk, nw), ste.cpu().numpy().reshape(nk, nw)
    _same_array(D_pts, D_true, "eval_points / eval_grid")
    n = int(np.count_nonzero(bm.brackets(D_true, st_true)))
    assert n >= 5
    rc, count, ref = _find_roots(gp, k, W, bm.W_PHASE_SPEED, Dt, stt, n + 3, n_bisect=N_BISECT)
    assert (rc, count) == (0, n)

    unsure = _unsure_mask(kind, nk, nw)
    rng = np.random.default_rng([nk, nw, 606])
    D_in = np.where(unsure, bm.WILD_VALUES[rng.integers(0, bm.WILD_VALUES.size, (nk, nw))], D_true)
    st_in = np.where(unsure, bm.UNSURE | rng.integers(0, 4, (nk, nw)), 0).astype(np.uint8)
    for cap in (n + 3, n, 5):
        what = (shape, kind, cap)
        Dm, stm, counts, _ = bm.screened_model(D_in, st_in, D_pts, st_pts, D_pts, st_pts, cap)
        m = min(n, cap)
        assert counts == (n, int(unsure.sum()), 2 * m, 0)
        Ds, sts = _dev(D_in), _dev(st_in)
        rc, got_counts, got = _screened(gp, k, W, bm.W_PHASE_SPEED, Ds, sts, cap, N_BISECT)
        assert got_counts == counts and rc == (ERR_CAPACITY if n > cap else 0), what
        _same_array(Ds.cpu().numpy(), D_true, what)
        _same_array(sts.cpu().numpy(), st_true, what)
        _same_rows(got, ref, m, what)
        _check_untouched(got, m, what)
        Da, sta = _dev(D_in), _dev(st_in)
        counts_a, got_a = _screened_async(gp, k, W, bm.W_PHASE_SPEED, Da, sta, cap, N_BISECT)
        assert counts_a == counts, what
        _same_array(Da.cpu().numpy(), D_true, what)
        _same_array(sta.cpu().numpy(), st_true, what)
        _same_rows(got_a, ref, m, what)
        _check_untouched(got_a, m, what)

    # sign flips at sure points: p = 0 mod 64 inside a row is the halo element that lane 63 of cell p - 1 reads
    flips = _flip_points(unsure, nw, rng)
    D_flip = D_in.copy()
    D_flip.reshape(-1)[flips] *= -1.0
    cap = n + 32
    Dm, stm, counts, b = bm.screened_model(D_flip, st_in, D_pts, st_pts, D_pts, st_pts, cap)
    changed = np.flatnonzero((b != bm.brackets(D_true, st_true)).reshape(-1))
    assert counts[3] > 0 and changed.size >= 4 and np.any(changed % 64 == 63)
    Ds, sts = _dev(D_flip), _dev(st_in)
    rc, got_counts, got = _screened(gp, k, W, bm.W_PHASE_SPEED, Ds, sts, cap, N_BISECT)
    assert got_counts == counts and rc == ERR_SCREENING, (shape, kind, got_counts, counts)
    _same_array(Ds.cpu().numpy(), Dm, "flipped")
    # row and k only: at n_bisect = 24 in the live window the refinement moves w_lo and w_hi, they are not pick_w(j), pick_w(j + 1)
    want_rows = bm.expected_table(Dm, stm, k, W, bm.W_PHASE_SPEED)
    assert got["row"][:counts[0]].tobytes() == want_rows["row"].tobytes()
    assert got["k"][:counts[0]].tobytes() == want_rows["k"].tobytes()
    _check_untouched(got, counts[0], "flipped")
    Da, sta = _dev(D_flip), _dev(st_in)
    counts_a, got_a = _screened_async(gp, k, W, bm.W_PHASE_SPEED, Da, sta, cap, N_BISECT)
    assert counts_a == counts
    _same_array(Da.cpu().numpy(), Dm, "flipped, async")
    _same_rows(got, got_a, counts[0], "flipped, sync / async")

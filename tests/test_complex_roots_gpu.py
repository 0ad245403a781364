"""es_complex_find_roots / es_complex_eval_* (C ABI section 6) where tests/test_complex_gpu.py does not reach: several
k-rows per call, ES_W_PHASE_SPEED, sausage and ES_CX_SFG, a root table that is too small, degenerate grids, node counts at the
edges of the LDS chunks, argument errors.  The candidate cells are compared as an ordered set with the plain cell rule of
tests/complex_winding_model.py, the refined roots with oracle/slab_complex.py."""
import ctypes as C

import numpy as np
import pytest

from tests.complex_winding_model import corner_quadrants, flagged_cells
from tests.test_complex_gpu import oracle_for

pytestmark = pytest.mark.gpu

W_ABSOLUTE, W_PHASE_SPEED, W_PER_ROW = 0, 1, 2
N_NODES = 130
K3 = np.array([0.3, 0.5, 0.8])
W_RE, W_IM = np.linspace(-0.5, 1.0, 16), np.linspace(-0.25, 0.25, 12)
N_ITER, TOL = 12, 4.0
SENT, SENT_I = -7.25, -77                  # pre-fill of the root table: what the search must leave beyond its records
COLS = ("k", "w_re", "w_im", "resid", "row", "flag")


def bits(a):
    """Bit pattern of an array (NaN compares equal to the same NaN)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def split(D):
    """(Re, Im) of a complex array as separate arrays, without arithmetic (keeps -0.0 and NaN parts as they are)."""
    D = np.asarray(D)
    return np.ascontiguousarray(D.real), np.ascontiguousarray(D.imag)


def raw_find_roots(s, mode, k, w_re, w_im, w_mode, Dre, Dim, st, n_iter, capacity, alloc=None, tol=TOL,
                   null_arrays=False, shape=None):
    """es_complex_find_roots through ctypes (the wrapper re-allocates and retries): (rc, count, table as NumPy columns of
    `alloc` entries, pre-filled with SENT / SENT_I).  k, w_re, w_im: NumPy; Dre, Dim, st: device tensors or None.
    shape = (nk, n_re, n_im) overrides the sizes taken from the arrays."""
    import torch
    from eigensolver_amd import _lib
    p = s.problem(mode)
    dk, dre, dim = (dev(a, np.float64).reshape(-1) if a is not None else None for a in (k, w_re, w_im))
    nk, n_re, n_im = shape if shape is not None else (dk.numel(), dre.numel(), dim.numel())
    alloc = capacity if alloc is None else alloc
    t = {c: torch.full((alloc,), SENT, dtype=torch.float64, device="cuda") for c in COLS[:4]}
    t.update({c: torch.full((alloc,), SENT_I, dtype=torch.int32, device="cuda") for c in COLS[4:]})
    ptr = (lambda x: None) if null_arrays else (lambda x: _lib.ptr(x) if x is not None else None)
    rt = _lib.ComplexRootTable(*[ptr(t[c]) for c in COLS], capacity)
    n = C.c_int(99)
    q = lambda x: _lib.ptr(x) if x is not None else None                                             # noqa: E731
    rc = s.ctx.lib.es_complex_find_roots(s.ctx.handle, p.handle, s.variant, q(dk), nk, q(dre), n_re, q(dim), n_im, int(w_mode),
                                         q(Dre), q(Dim), q(st), int(n_iter), float(tol), C.byref(rt), C.byref(n))
    s.ctx.synchronize()
    return rc, n.value, {c: t[c].cpu().numpy() for c in COLS}


def decode_cells(tab, n, k, w_re, w_im, w_mode):
    """The cell (row, i_im, i_re) that holds each of the first n reported omega (n_iter = 0: the report is the cell centre
    plus a quarter of the cell's diagonal, strictly inside its cell)."""
    out = []
    for j in range(n):
        r = int(tab["row"][j])
        f = k[r] if w_mode == W_PHASE_SPEED else 1.0
        gre, gim = f * w_re, f * w_im
        ire = int(np.searchsorted(gre, tab["w_re"][j])) - 1
        iim = int(np.searchsorted(gim, tab["w_im"][j])) - 1
        assert 0 <= ire < len(gre) - 1 and gre[ire] < tab["w_re"][j] < gre[ire + 1], (j, tab["w_re"][j])
        assert 0 <= iim < len(gim) - 1 and gim[iim] < tab["w_im"][j] < gim[iim + 1], (j, tab["w_im"][j])
        out.append((r, iim, ire))
    return out


# ---- (2) flag, scan and emit kernels alone, on arrays made on the host ------------------------------------------------
def synthetic(nk, n_re, n_im, seed):
    """D and status that no determinant would give: every sign / zero / tiny-value combination at the corners, statuses of
    all four kinds, NaN parts on points that claim ES_PT_OK."""
    rng = np.random.default_rng(seed)
    vals = np.array([-1.0, -0.0, 0.0, 1.0, 5e-324, -5e-324])
    shape = (nk, n_im, n_re)
    re, im = vals[rng.integers(0, 6, shape)], vals[rng.integers(0, 6, shape)]
    st = np.array([0, 0, 0, 0, 0, 1, 2, 3], dtype=np.uint8)[rng.integers(0, 8, shape)]
    ok = np.flatnonzero(st.ravel() == 0)
    pick = rng.choice(ok, size=max(9, ok.size // 150), replace=False)
    re.reshape(-1)[pick[0::3]] = np.nan
    im.reshape(-1)[pick[1::3]] = np.nan
    re.reshape(-1)[pick[2::3]] = np.nan
    im.reshape(-1)[pick[2::3]] = np.nan
    D = np.empty(shape, dtype=complex)
    D.real, D.imag = re, im
    k = np.linspace(0.3, 0.3 + 0.25 * (nk - 1), nk)
    w_re = -1.0 + np.cumsum(rng.uniform(0.01, 0.1, n_re))
    w_im = -0.5 + np.cumsum(rng.uniform(0.01, 0.1, n_im))
    return D, st, k, w_re, w_im


@pytest.fixture(scope="module")
def synthetic_grids():
    """(small, large): inputs and the model's flagged cells, computed once."""
    out = []
    for nk, n_re, n_im, seed in ((3, 37, 23, 11), (5, 231, 229, 12)):
        D, st, k, w_re, w_im = synthetic(nk, n_re, n_im, seed)
        out.append(dict(D=D, st=st, k=k, w_re=w_re, w_im=w_im, cells=flagged_cells(D, st), quadrants=corner_quadrants(D, st)))
    return out


@pytest.mark.parametrize("which", [0, 1], ids=["3x23x37", "5x229x231"])
def test_flagged_cells_synthetic(es_ctx, synthetic_grids, which):
    """cx_flag_kernel, the block scan and cx_emit_kernel against the plain cell rule: same count, same rows, same cells in
    the same order, k of the row.  3 x 23 x 37: 2553 points in 10 scan blocks, a row of 851 points (no multiple of 64 or
    256).  5 x 229 x 231: 1034 scan blocks, so the scan of the block counts takes its second pass of 1024.
    The 3 x 23 x 37 grid has about 360 cells with four ES_PT_OK corners and cannot hold all 4^4 corner-quadrant
    combinations (the rarest one has probability 1 / 6561 under this draw); the larger grid does, which is asserted."""
    from eigensolver_amd import SlabComplexFlow
    g = synthetic_grids[which]
    D, st, k, w_re, w_im, want = g["D"], g["st"], g["k"], g["w_re"], g["w_im"], g["cells"]
    assert np.all(np.diff(w_re) > 0) and np.all(np.diff(w_im) > 0)
    assert np.isnan(D.real[st == 0]).any() and np.isnan(D.imag[st == 0]).any()
    assert len(synthetic_grids[1]["quadrants"]) == 256
    assert len(g["quadrants"]) == 256 or which == 0
    assert len(want) > 50 and {c[0] for c in want} == set(range(len(k)))
    s = SlabComplexFlow(width=1e5, n_nodes=3, ctx=es_ctx)
    re, im = split(D)
    rc, n, tab = raw_find_roots(s, "kink", k, w_re, w_im, W_ABSOLUTE, dev(re), dev(im), dev(st), 0, len(want) + 16)
    assert rc == 0
    assert n == len(want)
    assert np.array_equal(tab["row"][:n], np.array([c[0] for c in want], dtype=np.int32))
    assert decode_cells(tab, n, k, w_re, w_im, W_ABSOLUTE) == want
    if which == 0:
        assert np.array_equal(tab["k"][:n], k[tab["row"][:n]])
        # centre + half / 2 of the cell (a, b): three quarters of the way from a to b
        a_re, b_re = w_re[[c[2] for c in want]], w_re[[c[2] + 1 for c in want]]
        a_im, b_im = w_im[[c[1] for c in want]], w_im[[c[1] + 1 for c in want]]
        assert np.allclose(tab["w_re"][:n], 0.5 * (a_re + b_re) + 0.25 * (b_re - a_re), rtol=1e-14, atol=0)
        assert np.allclose(tab["w_im"][:n], 0.5 * (a_im + b_im) + 0.25 * (b_im - a_im), rtol=1e-14, atol=0)
        assert set(np.unique(tab["flag"][:n])) <= {0, 1}
    for c in COLS[:4]:
        assert np.all(tab[c][n:] == SENT), c                       # nothing written past the count
    assert np.all(tab["row"][n:] == SENT_I) and np.all(tab["flag"][n:] == SENT_I)
    s.close()


# ---- (3) the whole search: rows, phase speeds, modes, variants --------------------------------------------------------
CASES = [(width, mode, variant) for width in (1e5, 0.9) for mode in ("kink", "sausage") for variant in ("sfx", "sfg")]
_CASE = {}


def case(es_ctx, width, mode, variant):
    """GPU grid and tables and the oracle's per-row results of one case, computed once per session (the oracle's secant
    iterations are the expensive part: a few seconds per case)."""
    key = (width, mode, variant)
    if key in _CASE:
        return _CASE[key]
    from eigensolver_amd import SlabComplexFlow
    s = SlabComplexFlow(width=width, variant=variant, n_nodes=N_NODES, ctx=es_ctx)
    o = oracle_for(s, mode)
    D, st, rel = s.eval_grid(mode, K3, W_RE, W_IM, W_PHASE_SPEED)
    Dre, Dim = D.real.contiguous(), D.imag.contiguous()
    c = dict(s=s, o=o, mode=mode, Dre=Dre, Dim=Dim, st=st, D=D.cpu().numpy(), stn=st.cpu().numpy(), rel=rel.cpu().numpy())
    c["cells"] = flagged_cells(c["D"], c["stn"])                          # the rule on the GPU's own D and status
    cap = len(c["cells"]) + 8
    c["t0"] = raw_find_roots(s, mode, K3, W_RE, W_IM, W_PHASE_SPEED, Dre, Dim, st, 0, cap)
    c["t12"] = raw_find_roots(s, mode, K3, W_RE, W_IM, W_PHASE_SPEED, Dre, Dim, st, N_ITER, cap)
    c["oracle"] = []
    for r, k in enumerate(K3):
        W = (k * W_RE)[None, :] + 1j * (k * W_IM)[:, None]
        d, rr, so = o.eval_rk4(k, W.ravel())
        ocells = flagged_cells(d.reshape((1,) + W.shape), so.reshape((1,) + W.shape))
        ro, relo, flo = o.find_roots(k, k * W_RE, k * W_IM, n_iter=N_ITER, tol=TOL)
        assert len(ro) == len(ocells)                                     # one record per cell, in the order of the rule
        c["oracle"].append(dict(d=d.reshape(W.shape), rel=rr.reshape(W.shape), st=so.reshape(W.shape),
                                cells=[(r, a, b) for _, a, b in ocells], w=ro, relw=relo, flag=flo))
    _CASE[key] = c
    return c


def compare_refined(c):
    """Every candidate the oracle converged (flag 1 and rel < 1e-2; next to the flow continuum the secant wanders) is a
    candidate of the GPU, accepted, at the same omega to 1e-8.  Returns how many were compared."""
    rc, n, tab = c["t12"]
    where = {cell: j for j, cell in enumerate(c["cells"])}
    compared = 0
    for orow in c["oracle"]:
        for cell, w, relw, flag in zip(orow["cells"], orow["w"], orow["relw"], orow["flag"]):
            if not (flag == 1 and relw < 1e-2):
                continue
            assert cell in where, cell
            j = where[cell]
            assert tab["flag"][j] == 1, (cell, tab["resid"][j])
            assert abs(complex(tab["w_re"][j], tab["w_im"][j]) - w) < 1e-8, (cell, w)
            compared += 1
    return compared


@pytest.mark.parametrize("width,mode,variant", CASES)
def test_find_roots_rows_modes_variants(es_ctx, width, mode, variant):
    """k = (0.3, 0.5, 0.8) in one call with ES_W_PHASE_SPEED: D and status against eval_rk4, the candidates against the cell
    rule on those very arrays (exact, ordered), the refined roots against the oracle's, and the table against three
    one-row calls and against ES_W_ABSOLUTE at k = 1 (bit for bit)."""
    c = case(es_ctx, width, mode, variant)
    s = c["s"]
    # the arrays the search was given are the determinant
    n_ok = 0
    for r, orow in enumerate(c["oracle"]):
        assert np.array_equal(c["stn"][r], orow["st"])
        ok = orow["st"] == 0
        n_ok += int(ok.sum())
        scale = np.abs(orow["d"][ok]) * 100.0 / orow["rel"][ok]
        assert np.max(np.abs(c["D"][r][ok] - orow["d"][ok]) / scale) < 1e-10
        assert np.max(np.abs(c["rel"][r][ok] - orow["rel"][ok]) / orow["rel"][ok]) < 1e-7
    assert n_ok > 100
    # candidates: exact and in order
    want = c["cells"]
    rows = np.array([cell[0] for cell in want], dtype=np.int32)
    for rc, n, tab in (c["t0"], c["t12"]):
        assert rc == 0 and n == len(want)
        assert np.array_equal(tab["row"][:n], rows)
        assert np.array_equal(tab["k"][:n], K3[rows])
        assert np.all(tab["k"][n:] == SENT) and np.all(tab["flag"][n:] == SENT_I)
    assert decode_cells(c["t0"][2], len(want), K3, W_RE, W_IM, W_PHASE_SPEED) == want
    # refinement
    assert compare_refined(c) >= 1
    # three one-row calls are the three-row call
    n = len(want)
    parts = []
    for r in range(3):
        rc1, n1, t1 = raw_find_roots(s, mode, K3[r:r + 1], W_RE, W_IM, W_PHASE_SPEED, c["Dre"][r:r + 1].contiguous(),
                                     c["Dim"][r:r + 1].contiguous(), c["st"][r:r + 1].contiguous(), N_ITER, n + 8)
        assert rc1 == 0 and n1 == int((rows == r).sum())
        t1 = {col: t1[col][:n1] for col in COLS}
        t1["row"] = t1["row"] + np.int32(r)
        parts.append(t1)
    for col in COLS:
        assert same_bits(np.concatenate([p[col] for p in parts]), c["t12"][2][col][:n]), col
    # ES_W_ABSOLUTE and ES_W_PHASE_SPEED coincide at k = 1
    one = np.array([1.0])
    tabs = []
    for w_mode in (W_ABSOLUTE, W_PHASE_SPEED):
        D1, st1, _ = s.eval_grid(mode, one, W_RE, W_IM, w_mode)
        rc1, n1, t1 = raw_find_roots(s, mode, one, W_RE, W_IM, w_mode, D1.real.contiguous(), D1.imag.contiguous(), st1,
                                     N_ITER, 192)
        assert rc1 == 0 and n1 == len(flagged_cells(D1.cpu().numpy(), st1.cpu().numpy()))
        tabs.append((n1, t1))
    assert tabs[0][0] == tabs[1][0]
    for col in COLS:
        assert same_bits(tabs[0][1][col], tabs[1][1][col]), col


def test_find_roots_compares_enough_roots(es_ctx):
    """The eight cases above together compare at least 36 converged roots (the oracle alone converges 8, 8, 3, 3, 1, 1, 3,
    17 = 44 on these inputs), and every case at least one."""
    counts = [compare_refined(case(es_ctx, *key)) for key in CASES]
    assert min(counts) >= 1, counts
    assert sum(counts) >= 36, counts


# ---- (4) capacity, degenerate grids, the first iterates ---------------------------------------------------------------
def test_capacity_and_degenerate_grids(es_ctx):
    c = case(es_ctx, 0.9, "sausage", "sfg")
    s, mode = c["s"], c["mode"]
    args = (s, mode, K3, W_RE, W_IM, W_PHASE_SPEED, c["Dre"], c["Dim"], c["st"], N_ITER)
    Cn = len(c["cells"])
    assert Cn >= 5
    rc, n, full = raw_find_roots(*args, Cn, alloc=Cn + 8)
    assert rc == 0 and n == Cn
    for col in COLS:
        assert same_bits(full[col][:Cn], c["t12"][2][col][:Cn]), col
        assert np.all(full[col][Cn:] == (SENT if col in COLS[:4] else SENT_I)), col
    for cap in (Cn - 1, 2):
        rc, n, t = raw_find_roots(*args, cap, alloc=Cn + 8)
        assert rc == 3 and n == Cn, cap                                   # ES_ERR_CAPACITY, the count still returned
        for col in COLS:
            assert same_bits(t[col][:cap], full[col][:cap]), (cap, col)
            assert np.all(t[col][cap:] == (SENT if col in COLS[:4] else SENT_I)), (cap, col)
    rc, n, t = raw_find_roots(*args, 0, null_arrays=True)
    assert rc == 3 and n == Cn
    rc, n, t = raw_find_roots(*args, 0, alloc=8)
    assert rc == 3 and n == Cn
    for col in COLS:
        assert np.all(t[col] == (SENT if col in COLS[:4] else SENT_I)), col
    # one column, one Im-line: no cells
    for sl_re, sl_im in ((slice(0, 1), slice(None)), (slice(None), slice(0, 1))):
        Dre, Dim, st = (x[:2, sl_im, sl_re].contiguous() for x in (c["Dre"], c["Dim"], c["st"]))
        rc, n, t = raw_find_roots(s, mode, K3[:2], W_RE[sl_re], W_IM[sl_im], W_PHASE_SPEED, Dre, Dim, st, N_ITER, 4)
        assert rc == 0 and n == 0
        assert np.all(t["k"] == SENT) and np.all(t["flag"] == SENT_I)
    # an empty grid: nothing is read
    for shape in ((0, 16, 12), (3, 0, 12), (3, 16, 0), (0, 0, 0)):
        rc, n, t = raw_find_roots(s, mode, None, None, None, W_PHASE_SPEED, None, None, None, N_ITER, 4, shape=shape)
        assert rc == 0 and n == 0, shape
        assert np.all(t["k"] == SENT) and np.all(t["flag"] == SENT_I)
    # n_iter = 0 and 1: the iterates themselves
    for n_iter in (0, 1):
        rc, n, t = raw_find_roots(s, mode, K3, W_RE, W_IM, W_PHASE_SPEED, c["Dre"], c["Dim"], c["st"], n_iter, Cn)
        assert rc == 0 and n == Cn
        where = {cell: j for j, cell in enumerate(c["cells"])}
        common = 0
        for r, k in enumerate(K3):
            ro, relo, flo = c["o"].find_roots(k, k * W_RE, k * W_IM, n_iter=n_iter, tol=TOL)
            ocells = c["oracle"][r]["cells"]
            assert len(ro) == len(ocells)
            for cell, w, relw, flag in zip(ocells, ro, relo, flo):
                if cell not in where:
                    continue
                j = where[cell]
                common += 1
                assert abs(complex(t["w_re"][j], t["w_im"][j]) - w) <= 1e-12 * abs(w), (n_iter, cell)
                assert np.isnan(t["resid"][j]) == np.isnan(relw), (n_iter, cell)
                if not np.isnan(relw):
                    assert abs(t["resid"][j] - relw) <= 1e-7 * relw, (n_iter, cell)
                if not abs(relw - TOL) <= 1e-6 * TOL:
                    assert t["flag"][j] == flag, (n_iter, cell, relw)
        assert common >= 5


# ---- (5) node counts at the edges of the LDS chunks -------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["sfx", "sfg"])
@pytest.mark.parametrize("mode", ["kink", "sausage"])
@pytest.mark.parametrize("N", [2, 3, 129, 130, 257, 258])
def test_eval_at_chunk_edges(es_ctx, N, mode, variant):
    """N - 1 = 1, 2, CH, CH + 1, 2 CH, 2 CH + 1 steps (CH = 128 steps per staged chunk); 257 points = one full workgroup
    and one lane, k different from lane to lane.  The project's bounds (1e-10 of the scale for D, 1e-7 for rel) hold at the
    two-node and three-node grids on their own: on these very points the fp64 eval_rk4 is within 1.3e-14 of the scale of the
    same restatement run in np.clongdouble at N = 2 and 3 (8.7e-13 at N = 130), so a step as long as the slab is not
    ill-conditioned here and no wider bound is used."""
    from eigensolver_amd import SlabComplexFlow
    s = SlabComplexFlow(width=0.9, variant=variant, n_nodes=N, ctx=es_ctx)
    o = oracle_for(s, mode)
    assert o.n_nodes == N
    rng = np.random.default_rng(1000 + N)
    n = 257
    k = np.array([0.3, 1.1, 2.7])[rng.integers(0, 3, n)]
    w = rng.uniform(-0.5, 3.0, n) * k / 1.5 + 1j * rng.uniform(-0.4, 0.4, n)
    D, st, rel = (t.cpu().numpy() for t in s.eval_points(mode, k, w))
    d, r, so = np.empty(n, complex), np.empty(n), np.empty(n, np.uint8)
    for kk in (0.3, 1.1, 2.7):
        sel = k == kk
        assert sel.sum() > 40
        d[sel], r[sel], so[sel] = o.eval_rk4(kk, w[sel])
    assert np.array_equal(st, so)
    ok = so == 0
    assert ok.sum() > 100
    assert np.all(np.isnan(D[~ok].real)) and np.all(np.isnan(rel[~ok]))
    scale = np.abs(d[ok]) * 100.0 / r[ok]
    err = np.abs(D[ok] - d[ok]) / scale
    relerr = np.abs(rel[ok] - r[ok]) / r[ok]
    print(f"N={N} {mode} {variant}: max |D - d| / scale = {err.max():.3e}, max rel error = {relerr.max():.3e}")
    assert err.max() < 1e-10
    assert relerr.max() < 1e-7
    s.close()


def test_eval_grid_without_rel_ragged_workgroup(es_ctx):
    """3 x 5 x 7 = 105 points (one ragged workgroup) with d_rel = NULL: D and status are those of the call with rel."""
    import torch
    from eigensolver_amd import SlabComplexFlow, _lib
    s = SlabComplexFlow(width=0.9, n_nodes=N_NODES, ctx=es_ctx)
    k = np.array([0.4, 1.0, 1.9])
    w_re, w_im = np.linspace(0.1, 1.2, 7), np.linspace(-0.2, 0.3, 5)
    D, st, rel = s.eval_grid("kink", k, w_re, w_im, W_PHASE_SPEED)
    p = s.problem("kink")
    dk, dre, dim = dev(k), dev(w_re), dev(w_im)
    Dre = torch.full((3, 5, 7), SENT, dtype=torch.float64, device="cuda")
    Dim = torch.full_like(Dre, SENT)
    st2 = torch.full((3, 5, 7), 99, dtype=torch.uint8, device="cuda")
    rc = es_ctx.lib.es_complex_eval_grid(es_ctx.handle, p.handle, s.variant, _lib.ptr(dk), 3, _lib.ptr(dre), 7, _lib.ptr(dim), 5,
                                         W_PHASE_SPEED, _lib.ptr(Dre), _lib.ptr(Dim), None, _lib.ptr(st2))
    assert rc == 0
    es_ctx.synchronize()
    assert torch.equal(st2, st) and int((st == 0).sum()) > 50
    assert same_bits(Dre.cpu().numpy(), D.real.cpu().numpy()) and same_bits(Dim.cpu().numpy(), D.imag.cpu().numpy())
    s.close()


# ---- (6) argument errors ------------------------------------------------------------------------------------------------
def test_complex_entry_points_reject_bad_arguments(es_ctx):
    """es_complex_eval_grid, es_complex_eval_points, es_complex_find_roots: every rejected call returns its status before
    anything is launched (the outputs keep their pre-fill), and the context computes correctly afterwards."""
    import torch
    from eigensolver_amd import SlabComplexFlow, ShootProblem, _lib, equilibrium as q
    lib = es_ctx.lib
    s = SlabComplexFlow(width=0.9, n_nodes=N_NODES, ctx=es_ctx)
    p = s.problem("kink")
    other = ShootProblem(q.SlabDensity(width=1.5, n_nodes=N_NODES), "kink", ctx=es_ctx)
    k, w_re, w_im = dev(K3), dev(W_RE), dev(W_IM)
    nk, n_re, n_im = 3, 16, 12
    npt = nk * n_re * n_im
    Dre, Dim, rel = (torch.full((npt,), SENT, dtype=torch.float64, device="cuda") for _ in range(3))
    st = torch.full((npt,), 99, dtype=torch.uint8, device="cuda")
    P = _lib.ptr
    INVALID, UNSUPPORTED = 1, 5

    def run(fn, good, cases):
        for change, status, text in cases:
            a = list(good)
            for pos, val in change.items():
                a[pos] = val
            assert fn(*a) == status, (fn.__name__, change)
            if a[0] is not None:
                assert text in lib.es_last_error(es_ctx.handle), (fn.__name__, change, lib.es_last_error(es_ctx.handle))

    flow_only = b"ES_GEOM_SLAB_FLOW"
    good = [es_ctx.handle, p.handle, 0, P(k), nk, P(w_re), n_re, P(w_im), n_im, W_PHASE_SPEED, P(Dre), P(Dim), P(rel), P(st)]
    run(lib.es_complex_eval_grid, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({2: 2}, INVALID, b"variant"),
         ({2: -1}, INVALID, b"variant"), ({9: W_PER_ROW}, INVALID, b"w_mode"), ({9: -1}, INVALID, b"w_mode"),
         ({4: -1}, INVALID, b"negative size"), ({6: -1}, INVALID, b"negative size"), ({8: -1}, INVALID, b"negative size")]
        + [({i: None}, INVALID, b"null pointer") for i in (3, 5, 7, 10, 11, 13)]
        + [({1: other.handle}, UNSUPPORTED, flow_only)])
    good = [es_ctx.handle, p.handle, 0, P(k), P(w_re), P(w_im), 3, P(Dre), P(Dim), P(rel), P(st)]
    run(lib.es_complex_eval_points, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({2: 2}, INVALID, b"variant"),
         ({6: -1}, INVALID, b"negative size")]
        + [({i: None}, INVALID, b"null pointer") for i in (3, 4, 5, 7, 8, 10)]
        + [({1: other.handle}, UNSUPPORTED, flow_only)])
    es_ctx.synchronize()
    for t in (Dre, Dim, rel):
        assert bool((t == SENT).all())
    assert bool((st == 99).all())

    # the search: a valid grid first, so that a call that slipped through would have cells to write
    D, stg, _ = s.eval_grid("kink", K3, W_RE, W_IM, W_PHASE_SPEED)
    gre, gim = D.real.contiguous(), D.imag.contiguous()
    want = flagged_cells(D.cpu().numpy(), stg.cpu().numpy())
    assert len(want) >= 2
    cap = 512                                                          # more than the 3 x 11 x 15 cells of the grid
    cols ={c: torch.full((cap,), SENT, dtype=torch.float64, device="cuda") for c in COLS[:4]}
    cols.update({c: torch.full((cap,), SENT_I, dtype=torch.int32, device="cuda") for c in COLS[4:]})

    def table(capacity=cap, drop=None):
        return _lib.ComplexRootTable(*[None if c == drop else P(cols[c]) for c in COLS], capacity)

    cnt = C.c_int(99)
    rt = table()
    good = [es_ctx.handle, p.handle, 0, P(k), nk, P(w_re), n_re, P(w_im), n_im, W_PHASE_SPEED, P(gre), P(gim), P(stg), N_ITER,
            TOL, C.byref(rt), C.byref(cnt)]
    neg = table(-1)
    run(lib.es_complex_find_roots, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({2: 2}, INVALID, b"variant"),
         ({9: W_PER_ROW}, INVALID, b"w_mode"), ({4: -1}, INVALID, b"size"), ({6: -1}, INVALID, b"size"),
         ({8: -1}, INVALID, b"size"), ({13: -1}, INVALID, b"size"), ({13: 1001}, INVALID, b"size"),
         ({15: C.byref(neg)}, INVALID, b"size"), ({15: None}, INVALID, b"null pointer"), ({16: None}, INVALID, b"null pointer")]
        + [({i: None}, INVALID, b"null pointer") for i in (3, 5, 7, 10, 11, 12)]
        + [({15: C.byref(table(drop=c))}, INVALID, b"null root table arrays") for c in COLS]
        + [({1: other.handle}, UNSUPPORTED, flow_only)])
    es_ctx.synchronize()
    for c in COLS:
        assert bool((cols[c] == (SENT if c in COLS[:4] else SENT_I)).all()), c

    # the context still computes: the same arguments, unchanged, are a valid search; a few points against the oracle
    assert lib.es_complex_find_roots(*good) == 0
    es_ctx.synchronize()
    assert cnt.value == len(want)
    assert np.array_equal(cols["row"].cpu().numpy()[:cnt.value], np.array([c[0] for c in want], dtype=np.int32))
    w = np.array([0.2 + 0.1j, 0.35 - 0.05j, 0.1 + 0.2j, 0.5 + 0.02j])
    Dp, sp, relp = (t.cpu().numpy() for t in s.eval_points("kink", 0.5, w))
    d, r, so = oracle_for(s, "kink").eval_rk4(0.5, w)
    assert np.array_equal(sp, so) and (so == 0).sum() >= 2
    ok = so == 0
    assert np.max(np.abs(Dp[ok] - d[ok]) / (np.abs(d[ok]) * 100.0 / r[ok])) < 1e-10
    other.close()
    s.close()

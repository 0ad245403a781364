"""es_cyl_complex_eval_grid / es_cyl_complex_eval_points / es_cyl_complex_find_roots (C ABI section 14) and
eigensolver_amd.CylinderComplex against the NumPy restatement tests/cyl_complex_model.py.

Values: D_c, outer, inner within 1e-10 of max(|outer|, |inner|) of the model (the bound of the project's other comparisons of a
march with its NumPy restatement, tests/test_eigenfunction_gpu.py), statuses identical; node counts 129, 130, 300 (one chunk of
CH = 128 steps exactly, one step more, three chunks), point counts 1, 63, 64, 65, 257.  Real axis: the real path's |D| and
status.  Conjugate symmetry.  Independent leg: DOP853 on complex y at N = 1000 within the RK4 contract of DESIGN section 2.
Roots: the candidate cells equal the model's cell rule on the model's own grid, every model root is reported with flag 1 within
10 x (1e-10 scale) / |dD/d omega| -- the value tolerance carried through the slope."""
import ctypes as C

import numpy as np
import pytest

from tests.cases import truth_problem
from tests.cyl_complex_model import model_for

pytestmark = pytest.mark.gpu

W_ABSOLUTE, W_PHASE_SPEED, W_PER_ROW = 0, 1, 2
SENT, SENT_I = -7.25, -77
COLS = ("k", "w_re", "w_im", "resid", "row", "flag")
INVALID, CAPACITY, UNSUPPORTED = 1, 3, 5
KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0)           # the jet that is Kelvin-Helmholtz unstable
K3 = np.array([0.5, 1.1, 2.0])
COUNTS = (1, 63, 64, 65, 257)


def problems(n_nodes):
    """name -> (equilibrium, mode, m, (W_lo, W_hi)): phase-speed window of the sample."""
    from eigensolver_amd import equilibrium as q
    return {
        "flow_kink": (q.CylinderFlow(**KH, width=1.5, n_nodes=n_nodes), "kink", None, (0.4, 1.7)),
        "flow_sausage": (q.CylinderFlow(**KH, width=1.5, n_nodes=n_nodes), "sausage", None, (0.4, 1.7)),
        "density": (q.CylinderDensity(width=0.95, n_nodes=n_nodes), "kink", None, (2.0, 5.5)),
        "flow_m3": (q.CylinderFlow(U_i0=0.35, width=0.9, n_nodes=n_nodes), "kink", 3, (2.7, 5.5)),
        "density_rplus": (q.CylinderDensity(width=1.5, c_e=1.5, vA_e=0.5, r_sign=1.0, n_nodes=n_nodes, ic=(1e-8, 1e-8)),
                          "kink", None, (0.5, 1.7)),
    }


NAMES = ("flow_kink", "flow_sausage", "density", "flow_m3", "density_rplus")


def sample(window, n, seed):
    """n points: k drawn from K3, Re omega = k W with W in the window, |Im omega| in [0.05, 0.6] k / 2 with both signs."""
    rng = np.random.default_rng(seed)
    k = K3[rng.integers(0, 3, n)]
    w = k * rng.uniform(window[0], window[1], n) + 1j * 0.5 * k * rng.uniform(0.05, 0.6, n) * rng.choice([-1.0, 1.0], n)
    return k, w


def scale_of(outer, inner):
    return np.maximum(np.abs(outer), np.abs(inner))


# ---- values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [129, 130, 300])
@pytest.mark.parametrize("name", NAMES)
def test_eval_points_against_model(es_ctx, name, n_nodes):
    from eigensolver_amd import CylinderComplex
    eq, mode, m, window = problems(n_nodes)[name]
    M = model_for(eq, mode, m)
    c = CylinderComplex(eq, ctx=es_ctx)
    k, w = sample(window, 257, 100 + n_nodes)
    Dm, om, im_, relm, stm = M.eval_points(k, w)
    ok = stm == 0
    assert ok.sum() > 120, ok.sum()
    sc = scale_of(om[ok], im_[ok])
    worst = 0.0
    for n in COUNTS:
        D, st, rel, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k[:n], w[:n], m=m, parts=True))
        assert D.shape == (n,)
        assert np.array_equal(st, stm[:n]), (name, n_nodes, n)
        o = ok[:n]
        for got, want in ((D, Dm), (outer, om), (inner, im_)):
            assert np.all(np.isnan(got[~o].real)) and np.all(np.isnan(got[~o].imag))
            if o.any():
                worst = max(worst, float(np.max(np.abs(got[o] - want[:n][o]) / sc[:int(o.sum())])))
        assert np.all(np.isnan(rel[~o]))
        if o.any():
            assert np.max(np.abs(rel[o] - relm[:n][o]) / relm[:n][o]) < 1e-7
            assert np.max(np.abs(D[o] - (outer[o] - inner[o])) / sc[:int(o.sum())]) < 1e-15
    print(f"{name} N={n_nodes}: max |value - model| / scale = {worst:.3e} over D_c, outer, inner ({int(ok.sum())} OK points)")
    assert worst < 1e-10
    c.close()


@pytest.mark.parametrize("w_mode", [W_ABSOLUTE, W_PHASE_SPEED])
@pytest.mark.parametrize("name", ["flow_kink", "density_rplus"])
def test_eval_grid_against_model(es_ctx, name, w_mode):
    """Three k-rows, 7 x 5 frequencies: 105 points, one ragged workgroup."""
    from eigensolver_amd import CylinderComplex
    eq, mode, m, window = problems(130)[name]
    M = model_for(eq, mode, m)
    c = CylinderComplex(eq, ctx=es_ctx)
    f = 1.0 if w_mode == W_PHASE_SPEED else 1.2
    w_re, w_im = f * np.linspace(window[0], window[1], 7), f * np.linspace(-0.2, 0.3, 5)
    D, st, rel = (t.cpu().numpy() for t in c.eval_grid(mode, K3, w_re, w_im, w_mode, m=m))
    Dm, relm, stm = M.eval_grid(K3, w_re, w_im, w_mode)
    assert D.shape == (3, 5, 7)
    assert np.array_equal(st, stm)
    ok = stm == 0
    assert ok.sum() > 50
    sc = np.abs(Dm[ok]) * 100.0 / relm[ok]
    err = np.max(np.abs(D[ok] - Dm[ok]) / sc)
    print(f"{name} w_mode={w_mode}: max |D_c - model| / scale = {err:.3e}")
    assert err < 1e-10
    assert np.max(np.abs(rel[ok] - relm[ok]) / relm[ok]) < 1e-7
    assert np.all(np.isnan(D[~ok].real)) and np.all(np.isnan(rel[~ok]))
    c.close()


# ---- real axis --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", [("flow_m3", (2.7, 5.6)), ("density_rplus", (0.52, 1.7))])
def test_real_axis_is_the_real_path(es_ctx, name, window):
    """w_im = 0: where the real es_shoot_eval_points reports OK, LEAKY or NONFINITE the complex path has the same status,
    Im D_c = 0 to 1e-13 of the scale and |D_c| = |D| to 1e-10 of it (the two differ by the sign of P_e(boundary)).  Points
    the real path flags as continuum are left out: their share is printed and stays under a quarter."""
    from eigensolver_amd import CylinderComplex
    eq, mode, m, _ = problems(130)[name]
    c = CylinderComplex(eq, ctx=es_ctx)
    p = c.problem(mode, m)
    k = np.repeat(K3, 40)
    w = k * np.tile(np.linspace(window[0], window[1], 40), 3)
    Dr, sr, relr = (t.cpu().numpy() for t in p.eval_points(k, w, want_rel=True))
    D, st, rel, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k, w + 0j, m=m, parts=True))
    cont = sr == 3
    print(f"{name}: continuum share of the sample {cont.mean():.3f}; OK {np.mean(sr == 0):.3f}, leaky {np.mean(sr == 1):.3f}")
    assert cont.mean() < 0.25
    keep = ~cont
    assert np.array_equal(st[keep], sr[keep])
    ok = keep & (sr == 0)
    assert ok.sum() > 40 and (sr == 1).sum() > 5
    sc = scale_of(outer[ok], inner[ok])
    assert np.max(np.abs(D[ok].imag) / sc) <= 1e-13
    err = np.max(np.abs(np.abs(D[ok]) - np.abs(Dr[ok])) / sc)
    print(f"{name}: max ||D_c| - |D|| / scale = {err:.3e}")
    assert err < 1e-10
    c.close()


def test_conjugate_symmetry(es_ctx):
    from eigensolver_amd import CylinderComplex
    for name in ("flow_kink", "flow_sausage", "density_rplus"):
        eq, mode, m, window = problems(130)[name]
        c = CylinderComplex(eq, ctx=es_ctx)
        k, w = sample(window, 65, 7)
        D, st, rel, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k, w, m=m, parts=True))
        D2, st2, _ = (t.cpu().numpy() for t in c.eval_points(mode, k, np.conj(w), m=m))
        assert np.array_equal(st, st2)
        ok = st == 0
        assert ok.sum() > 30
        err = np.max(np.abs(D2[ok] - np.conj(D[ok])) / scale_of(outer[ok], inner[ok]))
        print(f"{name}: max |D_c(conj w) - conj D_c(w)| / scale = {err:.3e}")
        assert err <= 1e-13
        c.close()


def test_independent_leg_dop853(es_ctx):
    """Eight points at N = 1000 against the interior integrated by DOP853 on complex y (rtol 1e-12): within the RK4
    contract of DESIGN section 2, 3e-8 (1000 / N)^4 of the scale."""
    from eigensolver_amd import CylinderComplex, equilibrium as q
    cases = [(q.CylinderFlow(**KH, width=1.5, n_nodes=1000), "kink", [(2.0, 2.6 + 0.1j), (1.0, 1.2 + 0.05j), (2.0, 2.2 + 0.3j)]),
             (q.CylinderFlow(**KH, width=0.9, n_nodes=1000), "sausage", [(2.0, 2.4 + 0.2j), (1.1, 1.0 - 0.15j)]),
             (q.CylinderDensity(width=0.95, n_nodes=1000), "kink", [(1.1, 3.3 + 0.2j), (2.0, 8.1 - 0.4j), (0.5, 1.9 + 0.05j)])]
    worst, count = 0.0, 0
    for eq, mode, pts in cases:
        M, T = model_for(eq, mode), truth_problem(eq, mode)
        c = CylinderComplex(eq, ctx=es_ctx)
        k, w = np.array([a for a, _ in pts]), np.array([b for _, b in pts])
        D, st, _ = (t.cpu().numpy() for t in c.eval_points(mode, k, w))
        assert np.all(st == 0)
        for j in range(len(pts)):
            d, o, i = M.eval_dop853(T, k[j], w[j])
            worst = max(worst, abs(D[j] - d) / max(abs(o), abs(i)))
            count += 1
        c.close()
    print(f"max |D_c - DOP853| / scale over {count} points at N = 1000: {worst:.3e}")
    assert count == 8 and worst < 3e-8


# ---- roots ------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def raw_find_roots(c, p, k, w_re, w_im, w_mode, Dre, Dim, st, n_iter, capacity, alloc=None, tol=4.0, shape=None):
    """es_cyl_complex_find_roots through ctypes: (rc, count, table as NumPy columns of `alloc` entries pre-filled with SENT /
    SENT_I)."""
    import torch
    from eigensolver_amd import _lib
    q = lambda x: _lib.ptr(x) if x is not None else None                                             # noqa: E731
    dk, dre, dim = (dev(a, np.float64).reshape(-1) if a is not None else None for a in (k, w_re, w_im))
    nk, n_re, n_im = shape if shape is not None else (dk.numel(), dre.numel(), dim.numel())
    alloc = capacity if alloc is None else alloc
    t = {col: torch.full((alloc,), SENT, dtype=torch.float64, device="cuda") for col in COLS[:4]}
    t.update({col: torch.full((alloc,), SENT_I, dtype=torch.int32, device="cuda") for col in COLS[4:]})
    rt = _lib.ComplexRootTable(*[_lib.ptr(t[col]) for col in COLS], capacity)
    n = C.c_int(99)
    rc = c.ctx.lib.es_cyl_complex_find_roots(c.ctx.handle, p.handle, q(dk), nk, q(dre), n_re, q(dim), n_im, int(w_mode), q(Dre),
                                             q(Dim), q(st), int(n_iter), float(tol), C.byref(rt), C.byref(n))
    c.ctx.synchronize()
    return rc, n.value, {col: t[col].cpu().numpy() for col in COLS}


def decode_cells(tab, n, k, w_re, w_im, w_mode):
    """The cell (row, i_im, i_re) of each of the first n records of an n_iter = 0 search: the report is the cell centre plus
    a quarter of the diagonal, strictly inside its cell."""
    out = []
    for j in range(n):
        r = int(tab["row"][j])
        f = k[r] if w_mode == W_PHASE_SPEED else 1.0
        gre, gim = f * w_re, f * w_im
        ire, iim = int(np.searchsorted(gre, tab["w_re"][j])) - 1, int(np.searchsorted(gim, tab["w_im"][j])) - 1
        assert gre[ire] < tab["w_re"][j] < gre[ire + 1] and gim[iim] < tab["w_im"][j] < gim[iim + 1], j
        out.append((r, iim, ire))
    return out


ROOT_CASES = {
    # name: (width, U_i0, k rows, w_re, w_im, w_mode)
    "uniform": (1e5, 3.0, [2.0], np.linspace(1.8, 3.0, 13), np.linspace(0.3, 0.9, 7), W_ABSOLUTE),
    "gaussian": (3.0, 3.0, [2.0], np.linspace(1.8, 3.0, 13), np.linspace(0.02, 0.5, 7), W_ABSOLUTE),
    "three_rows": (1e5, 3.0, [1.5, 2.0, 2.5], np.linspace(0.9, 1.5, 13), np.linspace(0.15, 0.45, 7), W_PHASE_SPEED),
}
_ROOTS = {}


def root_case(es_ctx, name):
    """The model's cells and converged roots and the GPU's grid and tables of one case, computed once per session."""
    if name in _ROOTS:
        return _ROOTS[name]
    from eigensolver_amd import CylinderComplex, equilibrium as q
    width, U, k, w_re, w_im, w_mode = ROOT_CASES[name]
    eq = q.CylinderFlow(**{**KH, "U_i0": U}, width=width, n_nodes=130)
    M = model_for(eq, "kink")
    c = CylinderComplex(eq, ctx=es_ctx)
    k = np.asarray(k)
    cells, roots = M.find_roots(k, w_re, w_im, w_mode)
    D, st, _ = c.eval_grid("kink", k, w_re, w_im, w_mode)
    Dre, Dim = D.real.contiguous(), D.imag.contiguous()
    p = c.problem("kink")
    cap = len(cells) + 8
    r = dict(c=c, p=p, M=M, k=k, w_re=w_re, w_im=w_im, w_mode=w_mode, cells=cells, roots=roots, Dre=Dre, Dim=Dim, st=st,
             t0=raw_find_roots(c, p, k, w_re, w_im, w_mode, Dre, Dim, st, 0, cap),
             t12=raw_find_roots(c, p, k, w_re, w_im, w_mode, Dre, Dim, st, 12, cap))
    _ROOTS[name] = r
    return r


@pytest.mark.parametrize("name", list(ROOT_CASES))
def test_find_roots_against_model(es_ctx, name):
    r = root_case(es_ctx, name)
    cells, roots, M, k = r["cells"], r["roots"], r["M"], r["k"]
    assert sum(w is not None for w in roots) >= 1, "the model alone must find a root in this window"
    if name == "uniform":
        assert any(w is not None and abs(w - (2.372765 + 0.584713j)) < 1e-6 for w in roots)
    if name == "three_rows":
        assert {cell[0] for cell, w in zip(cells, roots) if w is not None} == {0, 1, 2}
    for rc, n, tab in (r["t0"], r["t12"]):
        assert rc == 0 and n == len(cells)
        assert np.array_equal(tab["row"][:n], np.array([cell[0] for cell in cells], dtype=np.int32))
        assert np.array_equal(tab["k"][:n], k[tab["row"][:n]])
        assert np.all(tab["k"][n:] == SENT) and np.all(tab["flag"][n:] == SENT_I)
    assert decode_cells(r["t0"][2], len(cells), k, r["w_re"], r["w_im"], r["w_mode"]) == cells
    tab = r["t12"][2]
    for j, (cell, w) in enumerate(zip(cells, roots)):
        if w is None:
            continue
        kk = k[cell[0]]
        _, o, i, _, _ = M.eval(kk, w)
        bound = 10.0 * 1e-10 * max(abs(o[0]), abs(i[0])) / abs(M.d_omega(kk, w))
        got = complex(tab["w_re"][j], tab["w_im"][j])
        print(f"{name} cell {cell}: root {got:.12f}, |root - model| = {abs(got - w):.3e}, bound {bound:.3e}, resid {tab['resid'][j]:.3e} %")
        assert tab["flag"][j] == 1, (cell, tab["resid"][j])
        assert abs(got - w) <= bound, (cell, got, w, bound)


def test_unstable_roots_wrapper(es_ctx):
    """CylinderComplex.unstable_roots: grid, search, accepted and de-duplicated roots per k-row."""
    r = root_case(es_ctx, "three_rows")
    out = r["c"].unstable_roots("kink", r["k"], r["w_re"], r["w_im"], w_mode=r["w_mode"])
    assert len(out) == 3
    for row in range(3):
        want = [w for cell, w in zip(r["cells"], r["roots"]) if cell[0] == row and w is not None]
        assert len(out[row]) == 1 and abs(out[row][0] - want[0]) < 1e-8


def test_capacity_and_empty_grid(es_ctx):
    r = root_case(es_ctx, "gaussian")
    c, p = r["c"], r["p"]
    args = (c, p, r["k"], r["w_re"], r["w_im"], r["w_mode"], r["Dre"], r["Dim"], r["st"], 12)
    Cn = len(r["cells"])
    assert Cn >= 2
    full = r["t12"][2]
    for cap in (Cn - 1, 0):
        rc, n, t = raw_find_roots(*args, cap, alloc=Cn + 8)
        assert rc == CAPACITY and n == Cn, cap                            # the count is still returned
        for col in COLS:
            a, b = t[col][:cap], full[col][:cap]
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
            assert np.all(t[col][cap:] == (SENT if col in COLS[:4] else SENT_I)), (cap, col)
    for shape in ((0, 13, 7), (1, 0, 7), (1, 13, 0), (0, 0, 0)):
        rc, n, t = raw_find_roots(c, p, None, None, None, r["w_mode"], None, None, None, 12, 4, shape=shape)
        assert rc == 0 and n == 0, shape
        assert np.all(t["k"] == SENT) and np.all(t["flag"] == SENT_I)
    for nk, n_re, n_im in ((0, 13, 7), (1, 0, 7)):                          # eval calls with no points touch nothing
        assert c.ctx.lib.es_cyl_complex_eval_grid(c.ctx.handle, p.handle, None, nk, None, n_re, None, n_im, 0, None, None, None,
                                                  None) == 0
    assert c.ctx.lib.es_cyl_complex_eval_points(c.ctx.handle, p.handle, None, None, None, 0, None, None, None, None, None,
                                                None) == 0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments(es_ctx):
    """Every rejected call returns its status before anything is launched: the outputs keep their pre-fill."""
    import torch
    from eigensolver_amd import CylinderComplex, ShootProblem, _lib, equilibrium as q
    lib = es_ctx.lib
    r = root_case(es_ctx, "gaussian")
    p = r["p"]
    slab = ShootProblem(q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=130), "kink", ctx=es_ctx)
    twisted = ShootProblem(q.CylinderRotation(v_twist=0.25, power=0.8, n_nodes=130), "kink", ctx=es_ctx)
    k, w_re, w_im = dev(r["k"]), dev(r["w_re"]), dev(r["w_im"])
    nk, n_re, n_im = 1, 13, 7
    npt = nk * n_re * n_im
    Dre, Dim, rel = (torch.full((npt,), SENT, dtype=torch.float64, device="cuda") for _ in range(3))
    outer, inner = (torch.full((2 * npt,), SENT, dtype=torch.float64, device="cuda") for _ in range(2))
    st = torch.full((npt,), 99, dtype=torch.uint8, device="cuda")
    P = _lib.ptr

    def run(fn, good, cases):
        for change, status, text in cases:
            a = list(good)
            for pos, val in change.items():
                a[pos] = val
            assert fn(*a) == status, (fn.__name__, change)
            if a[0] is not None:
                assert text in lib.es_last_error(es_ctx.handle), (fn.__name__, change, lib.es_last_error(es_ctx.handle))

    only = b"ES_GEOM_CYLINDER"
    others = [({1: slab.handle}, UNSUPPORTED, only), ({1: twisted.handle}, UNSUPPORTED, only)]
    good = [es_ctx.handle, p.handle, P(k), nk, P(w_re), n_re, P(w_im), n_im, W_ABSOLUTE, P(Dre), P(Dim), P(rel), P(st)]
    run(lib.es_cyl_complex_eval_grid, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({8: W_PER_ROW}, INVALID, b"w_mode"),
         ({8: -1}, INVALID, b"w_mode"), ({3: -1}, INVALID, b"negative size"), ({5: -1}, INVALID, b"negative size"),
         ({7: -1}, INVALID, b"negative size")]
        + [({i: None}, INVALID, b"null pointer") for i in (2, 4, 6, 9, 10, 12)] + others)
    kp, wr, wi = dev(np.full(npt, 2.0)), dev(np.linspace(1.8, 3.0, npt)), dev(np.full(npt, 0.2))
    good = [es_ctx.handle, p.handle, P(kp), P(wr), P(wi), npt, P(Dre), P(Dim), P(rel), P(st), P(outer), P(inner)]
    run(lib.es_cyl_complex_eval_points, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({5: -1}, INVALID, b"negative size")]
        + [({i: None}, INVALID, b"null pointer") for i in (2, 3, 4, 6, 7, 9)] + others)
    es_ctx.synchronize()
    for t in (Dre, Dim, rel, outer, inner):
        assert bool((t == SENT).all())
    assert bool((st == 99).all())

    cap = 64
    cols = {c: torch.full((cap,), SENT, dtype=torch.float64, device="cuda") for c in COLS[:4]}
    cols.update({c: torch.full((cap,), SENT_I, dtype=torch.int32, device="cuda") for c in COLS[4:]})

    def table(capacity=cap, drop=None):
        return _lib.ComplexRootTable(*[None if c == drop else P(cols[c]) for c in COLS], capacity)

    cnt = C.c_int(99)
    rt, neg = table(), table(-1)
    good = [es_ctx.handle, p.handle, P(k), nk, P(w_re), n_re, P(w_im), n_im, W_ABSOLUTE, P(r["Dre"]), P(r["Dim"]), P(r["st"]), 12,
            4.0, C.byref(rt), C.byref(cnt)]
    run(lib.es_cyl_complex_find_roots, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({8: W_PER_ROW}, INVALID, b"w_mode"),
         ({3: -1}, INVALID, b"size"), ({5: -1}, INVALID, b"size"), ({7: -1}, INVALID, b"size"), ({12: -1}, INVALID, b"size"),
         ({12: 1001}, INVALID, b"size"), ({14: C.byref(neg)}, INVALID, b"size"), ({14: None}, INVALID, b"null pointer"),
         ({15: None}, INVALID, b"null pointer")]
        + [({i: None}, INVALID, b"null pointer") for i in (2, 4, 6, 9, 10, 11)]
        + [({14: C.byref(table(drop=c))}, INVALID, b"null root table arrays") for c in COLS] + others)
    es_ctx.synchronize()
    for c in COLS:
        assert bool((cols[c] == (SENT if c in COLS[:4] else SENT_I)).all()), c
    # the same arguments, unchanged, are a valid search, and the section-6 calls keep refusing the cylinder
    assert lib.es_cyl_complex_find_roots(*good) == 0
    es_ctx.synchronize()
    assert cnt.value == len(r["cells"])
    assert lib.es_complex_eval_points(es_ctx.handle, p.handle, 0, P(kp), P(wr), P(wi), npt, P(Dre), P(Dim), P(rel), P(st)) == UNSUPPORTED
    with pytest.raises(TypeError):
        CylinderComplex(q.CylinderRotation())
    slab.close()
    twisted.close()

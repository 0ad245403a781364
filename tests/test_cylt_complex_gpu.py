"""es_cylt_complex_eval_grid / es_cylt_complex_eval_points / es_cylt_complex_find_roots (C ABI section 17) and
eigensolver_amd.RotatingCylinderComplex against the NumPy restatement tests/cylt_complex_model.py.

Values: D_c, outer, inner and rel within 1e-10 of max(|outer|, |inner|) of the model (the bound of the project's other comparisons of a
march with its NumPy restatement), statuses identical; node counts 129, 130, 300 (one chunk of CH = 128 steps exactly, one step
more, three chunks), point counts 1, 65, 257, a different k in every lane, both signs of Im omega, both values of c1_power,
accept_norm 0 and 1.  Grid against points bit for bit.  Real axis: sign(P_e) D of the real path.  Zero-twist limit: the
untwisted kernels on the same jet.  Roots: every converged model root with flag 1 within 1e-12 relative, table order that of the
model's cells; capacity; argument errors."""
import ctypes as C

import numpy as np
import pytest

from tests.cylt_complex_model import JET, JET_ROOT, model_for, root_cases

pytestmark = pytest.mark.gpu

W_ABSOLUTE, W_PHASE_SPEED, W_PER_ROW = 0, 1, 2
SENT, SENT_I = -7.25, -77
COLS = ("k", "w_re", "w_im", "resid", "row", "flag")
INVALID, CAPACITY, UNSUPPORTED = 1, 3, 5
COUNTS = (1, 65, 257)


def twisted_jet(**kw):
    from eigensolver_amd import equilibrium as q

    class TwistedJet(q.CylinderFlow):
        twisted = True

    return TwistedJet(**kw)


def problems(n_nodes):
    """name -> (equilibrium, mode, m, accept_norm, (W_lo, W_hi), (g_lo, g_hi)): phase-speed window of Re omega / k and the
    window of |Im omega| / k of the sample."""
    from eigensolver_amd import equilibrium as q
    rot = lambda v, p, **kw: q.CylinderRotation(v_twist=v, power=p, n_nodes=n_nodes, **kw)             # noqa: E731
    return {
        "A": (rot(2.0, 1.0, r_axis=1e-2), "kink", 3, 0, (1.2, 1.9), (0.45, 1.15)),
        "B": (rot(2.0, 0.8, r_axis=1e-2, c1_power=1), "kink", 1, 1, (1.2, 1.7), (0.05, 0.35)),
        "C": (rot(1.0, 1.0, r_axis=1e-2), "kink", 4, 0, (0.9, 1.4), (0.15, 1.2)),
        "sausage": (rot(0.15, 1.25, r_axis=1e-2, c1_power=1), "sausage", 0, 0, (0.6, 1.45), (0.02, 0.3)),
        "reference": (rot(0.25, 0.8), "kink", None, 1, (0.6, 1.45), (0.02, 0.3)),
    }


NAMES = ("A", "B", "C", "sausage", "reference")


def sample(W, g, n, seed):
    """n points, a different k in every lane: Re omega = k W, Im omega = +- k g, both signs."""
    rng = np.random.default_rng(seed)
    k = np.linspace(0.5, 2.0, n) if n > 1 else np.array([1.0])
    k = rng.permutation(k)
    w = k * rng.uniform(W[0], W[1], n) + 1j * k * rng.uniform(g[0], g[1], n) * rng.choice([-1.0, 1.0], n)
    return k, w


def scale_of(outer, inner):
    return np.maximum(np.abs(outer), np.abs(inner))


def solver(es_ctx, eq, mode, m, accept_norm=0):
    """RotatingCylinderComplex whose cached problem of (mode, m) carries accept_norm."""
    from eigensolver_amd import RotatingCylinderComplex, ShootProblem
    c = RotatingCylinderComplex(eq, ctx=es_ctx)
    if accept_norm:
        key = (mode, (1 if mode == "kink" else 0) if m is None else int(m))
        c._problems[key] = ShootProblem(eq, mode, m=key[1], ctx=es_ctx, accept_norm=1)
    return c


def leaky_pair(M):
    """A (k, omega) pair off the real axis whose status is ES_PT_LEAKY in the model: Re omega / k beyond every exterior speed."""
    k, w = 1.0, 2.4 + 0.05j
    assert M.eval(k, [w])[4][0] == 1
    return k, w


# ---- values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [129, 130, 300])
@pytest.mark.parametrize("name", NAMES)
def test_eval_points_against_model(es_ctx, name, n_nodes):
    eq, mode, m, an, W, g = problems(n_nodes)[name]
    M = model_for(eq, mode, m, accept_norm=an)
    c = solver(es_ctx, eq, mode, m, an)
    k, w = sample(W, g, 257, 100 + n_nodes)
    st0 = M.eval_points(k, w)[4]
    L = next(j for j in range(1, 60) if st0[j - 1] == 0 and st0[j] == 0 and st0[j + 1] == 0)
    k_ok, w_ok = k[L], w[L]
    k[L], w[L] = leaky_pair(M)                                   # a leaky lane placed by hand between OK lanes
    Dm, om, im_, relm, stm = M.eval_points(k, w)
    ok = stm == 0
    assert ok.sum() > 120, ok.sum()
    assert stm[L] == 1 and stm[L - 1] == 0 and stm[L + 1] == 0
    worst = worst_rel = 0.0
    for n in COUNTS:
        D, st, rel, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k[:n], w[:n], m=m, parts=True))
        assert D.shape == (n,)
        assert np.array_equal(st, stm[:n]), (name, n_nodes, n)
        o = ok[:n]
        sc = scale_of(om[:n][o], im_[:n][o])
        for got, want in ((D, Dm), (outer, om), (inner, im_)):
            assert np.all(np.isnan(got[~o].real)) and np.all(np.isnan(got[~o].imag))
            if o.any():
                worst = max(worst, float(np.max(np.abs(got[o] - want[:n][o]) / sc)))
        assert np.all(np.isnan(rel[~o]))
        if o.any():
            # rel is a percentage of its denominator (|outer| with accept_norm, else the scale): its difference in units of the scale
            den = np.abs(om[:n][o]) if an else sc
            worst_rel = max(worst_rel, float(np.max(np.abs(rel[o] - relm[:n][o]) / 100.0 * den / sc)))
            assert np.max(np.abs(D[o] - (outer[o] - inner[o])) / sc) < 1e-15
    # the neighbours of the leaky lane: bit for bit what they are with an OK lane in its place
    k2, w2 = k[:65].copy(), w[:65].copy()
    k2[L], w2[L] = k_ok, w_ok
    a = [t.cpu().numpy() for t in c.eval_points(mode, k[:65], w[:65], m=m, parts=True)]
    b = [t.cpu().numpy() for t in c.eval_points(mode, k2, w2, m=m, parts=True)]
    assert a[1][L] == 1 and b[1][L] == 0
    for x, y in zip(a, b):
        for j in (L - 1, L + 1):
            assert x[j].tobytes() == y[j].tobytes(), (name, n_nodes, j)
    print(f"{name} N={n_nodes}: max |value - model| / scale = {worst:.3e} over D_c, outer, inner, {worst_rel:.3e} for rel "
          f"({int(ok.sum())} OK points; bound 1e-10)")
    assert worst < 1e-10 and worst_rel < 1e-10
    c.close()


@pytest.mark.parametrize("w_mode", [W_ABSOLUTE, W_PHASE_SPEED])
def test_eval_grid_equals_eval_points(es_ctx, w_mode):
    """nk = 2, 24 x 12 frequencies: 576 points, three workgroups, the last one ragged."""
    eq, mode, m, an, W, g = problems(130)["A"]
    c = solver(es_ctx, eq, mode, m)
    k = np.array([0.8, 1.0])
    w_re, w_im = np.linspace(W[0], W[1], 24), np.linspace(-0.4, 1.1, 12)
    D, st, rel = (t.cpu().numpy() for t in c.eval_grid(mode, k, w_re, w_im, w_mode, m=m))
    assert D.shape == (2, 12, 24)
    f = k[:, None, None] if w_mode == W_PHASE_SPEED else np.ones((2, 1, 1))
    wp = f * w_re[None, None, :] + 1j * (f * w_im[None, :, None])
    kp = np.broadcast_to(k[:, None, None], wp.shape)
    Dp, stp, relp = (t.cpu().numpy() for t in c.eval_points(mode, kp.ravel(), wp.ravel(), m=m))
    assert (st == 0).sum() > 100
    assert np.array_equal(st.ravel(), stp)
    assert D.ravel().tobytes() == Dp.tobytes() and rel.ravel().tobytes() == relp.tobytes()
    c.close()


# ---- real axis --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reference", "sausage"])
def test_real_axis_is_the_real_path(es_ctx, name):
    """w_im = 0: at the points where both paths report ES_PT_OK, D_c = sign(P_e(boundary)) D of es_shoot_eval_points within
    1e-10 of the scale and |Im D_c| is within 1e-13 of it.  sign(P_e) from the real oracle's exterior."""
    from tests.cases import truth_problem
    eq, mode, m, an, _, _ = problems(130)[name]
    c = solver(es_ctx, eq, mode, m)
    p = c.problem(mode, m)
    T = truth_problem(eq, mode, m)
    K = np.array([1.0, 2.0, 3.0])
    k = np.repeat(K, 40)
    w = k * np.tile(np.linspace(0.55, 1.48, 40), 3)
    Dr, sr, _ = (t.cpu().numpy() for t in p.eval_points(k, w, want_rel=True))
    D, st, rel, outer, inner = (t.cpu().numpy() for t in c.eval_points(mode, k, w + 0j, m=m, parts=True))
    ok = (sr == 0) & (st == 0)
    print(f"{name}: real path OK {np.mean(sr == 0):.3f}, continuum {np.mean(sr == 3):.3f}; complex path OK {np.mean(st == 0):.3f}")
    assert ok.sum() > 40
    assert np.array_equal(st[sr != 3], sr[sr != 3])
    sgn = np.array([np.sign(T.exterior(a, b)[2]) for a, b in zip(k[ok], w[ok])])
    sc = scale_of(outer[ok], inner[ok])
    im_err = np.max(np.abs(D[ok].imag) / sc)
    err = np.max(np.abs(D[ok].real - sgn * Dr[ok]) / sc)
    print(f"{name}: max |D_c - sign(P_e) D| / scale = {err:.3e} (bound 1e-10), max |Im D_c| / scale = {im_err:.3e} (bound 1e-13)")
    assert im_err <= 1e-13
    assert err < 1e-10
    c.close()


# ---- zero-twist limit -------------------------------------------------------------------------------------------------------
def test_zero_twist_limit(es_ctx):
    """The uniform jet through the twisted coefficient set (v_phi = B_phi = 0) against CylinderComplex on the plain CylinderFlow,
    same points, r_sign = +1: 1e-10 of the scale away from poles; unstable_roots returns the root of DESIGN 8i to 1e-6."""
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, equilibrium as q
    ct = RotatingCylinderComplex(twisted_jet(**JET, n_nodes=130), ctx=es_ctx)
    c0 = CylinderComplex(q.CylinderFlow(**JET, n_nodes=130), ctx=es_ctx)
    rng = np.random.default_rng(5)
    k = rng.uniform(1.0, 2.5, 65)
    w = k * rng.uniform(0.9, 1.45, 65) + 1j * k * rng.uniform(0.05, 0.4, 65) * rng.choice([-1.0, 1.0], 65)
    Dt, stt, _, ot, it = (t.cpu().numpy() for t in ct.eval_points("kink", k, w, parts=True))
    D0, st0, rel0, o0, i0 = (t.cpu().numpy() for t in c0.eval_points("kink", k, w, parts=True))
    assert np.array_equal(stt, st0)
    ok = (st0 == 0) & (scale_of(o0, i0) < 1e3 * np.abs(o0))                  # away from the poles of inner
    assert ok.sum() > 40
    sc = scale_of(o0[ok], i0[ok])
    err = max(np.max(np.abs(Dt[ok] - D0[ok]) / sc), np.max(np.abs(it[ok] - i0[ok]) / sc))
    print(f"zero twist: max |twisted - untwisted| / scale = {err:.3e} on {int(ok.sum())} points (bound 1e-10)")
    err = max(err, np.max(np.abs(ot[ok] - o0[ok]) / sc))
    assert err < 1e-10
    roots = ct.unstable_roots("kink", [2.0], np.linspace(1.8, 3.0, 13), np.linspace(0.3, 0.9, 7))
    assert len(roots) == 1 and len(roots[0]) == 1
    print(f"zero twist: root {roots[0][0]:.9f}")
    assert abs(roots[0][0] - JET_ROOT) < 1e-6
    ct.close()
    c0.close()


# ---- roots ------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def raw_find_roots(c, p, k, w_re, w_im, w_mode, Dre, Dim, st, n_iter, capacity, alloc=None, tol=4.0, shape=None):
    """es_cylt_complex_find_roots through ctypes: (rc, count, table as NumPy columns of `alloc` entries pre-filled with SENT /
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
    rc = c.ctx.lib.es_cylt_complex_find_roots(c.ctx.handle, p.handle, q(dk), nk, q(dre), n_re, q(dim), n_im, int(w_mode), q(Dre),
                                              q(Dim), q(st), int(n_iter), float(tol), C.byref(rt), C.byref(n))
    c.ctx.synchronize()
    return rc, n.value, {col: t[col].cpu().numpy() for col in COLS}


_ROOTS = {}


def root_case(es_ctx, name):
    """The model's cells and converged roots and the GPU's grid and table of one case, computed once per session."""
    if name in _ROOTS:
        return _ROOTS[name]
    eq, m, k, w_re, w_im, quoted = root_cases()[name]
    M = model_for(eq, "kink", m)
    c = solver(es_ctx, eq, "kink", m)
    k = np.asarray(k)
    cells, roots = M.find_roots(k, w_re, w_im)
    D, st, _ = c.eval_grid("kink", k, w_re, w_im, W_ABSOLUTE, m=m)
    Dre, Dim = D.real.contiguous(), D.imag.contiguous()
    p = c.problem("kink", m)
    cap = len(cells) + 8
    r = dict(c=c, p=p, M=M, m=m, k=k, w_re=w_re, w_im=w_im, cells=cells, roots=roots, quoted=quoted, Dre=Dre, Dim=Dim, st=st,
             t12=raw_find_roots(c, p, k, w_re, w_im, W_ABSOLUTE, Dre, Dim, st, 12, cap))
    _ROOTS[name] = r
    return r


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_find_roots_against_model(es_ctx, name):
    r = root_case(es_ctx, name)
    cells, roots, k = r["cells"], r["roots"], r["k"]
    assert {cell[0] for cell, w in zip(cells, roots) if w is not None} == set(range(len(k))), "the model alone must find a root"
    rc, n, tab = r["t12"]
    assert rc == 0 and n == len(cells)
    assert np.array_equal(tab["row"][:n], np.array([cell[0] for cell in cells], dtype=np.int32))
    assert np.array_equal(tab["k"][:n], k[tab["row"][:n]])
    assert np.all(tab["k"][n:] == SENT) and np.all(tab["flag"][n:] == SENT_I)
    for j, (cell, w) in enumerate(zip(cells, roots)):
        if w is None:
            continue
        got = complex(tab["w_re"][j], tab["w_im"][j])
        print(f"{name} cell {cell}: root {got:.12f}, |root - model| / |root| = {abs(got - w) / abs(w):.3e} (bound 1e-12), "
              f"resid {tab['resid'][j]:.3e} %")
        assert tab["flag"][j] == 1, (cell, tab["resid"][j])
        assert abs(got - w) <= 1e-12 * abs(w), (cell, got, w)
        if r["quoted"] is not None:
            assert abs(got - r["quoted"]) < 1e-5
    out = r["c"].unstable_roots("kink", k, r["w_re"], r["w_im"], m=r["m"])
    assert len(out) == len(k) and all(len(a) >= 1 for a in out)


def test_capacity(es_ctx):
    """A table one record short, and of capacity 0: ES_ERR_CAPACITY with the full count, nothing written past the capacity."""
    r = root_case(es_ctx, "C")
    c, p = r["c"], r["p"]
    args = (c, p, r["k"], r["w_re"], r["w_im"], W_ABSOLUTE, r["Dre"], r["Dim"], r["st"], 12)
    Cn = len(r["cells"])
    assert Cn >= 2
    full = r["t12"][2]
    for cap in (Cn - 1, 0):
        rc, n, t = raw_find_roots(*args, cap, alloc=Cn + 8)
        assert rc == CAPACITY and n == Cn, cap
        for col in COLS:
            assert t[col][:cap].tobytes() == full[col][:cap].tobytes(), (cap, col)
            assert np.all(t[col][cap:] == (SENT if col in COLS[:4] else SENT_I)), (cap, col)


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments(es_ctx):
    """Every rejected call returns its status before anything is launched: the outputs keep their pre-fill."""
    import torch
    from eigensolver_amd import RotatingCylinderComplex, ShootProblem, _lib, equilibrium as q
    lib = es_ctx.lib
    r = root_case(es_ctx, "C")
    p = r["p"]
    slab = ShootProblem(q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=130), "kink", ctx=es_ctx)
    untwisted = ShootProblem(q.CylinderFlow(U_i0=0.35, width=1.5, n_nodes=130), "kink", ctx=es_ctx)
    k, w_re, w_im = dev(r["k"]), dev(r["w_re"]), dev(r["w_im"])
    nk, n_re, n_im = len(r["k"]), len(r["w_re"]), len(r["w_im"])
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

    only = b"ES_GEOM_CYLINDER_TWIST"
    others = [({1: slab.handle}, UNSUPPORTED, only), ({1: untwisted.handle}, UNSUPPORTED, only)]
    good = [es_ctx.handle, p.handle, P(k), nk, P(w_re), n_re, P(w_im), n_im, W_ABSOLUTE, P(Dre), P(Dim), P(rel), P(st)]
    run(lib.es_cylt_complex_eval_grid, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({8: W_PER_ROW}, INVALID, b"w_mode"),
         ({8: -1}, INVALID, b"w_mode"), ({3: -1}, INVALID, b"negative size"), ({5: -1}, INVALID, b"negative size"),
         ({7: -1}, INVALID, b"negative size")]
        + [({i: None}, INVALID, b"null pointer") for i in (2, 4, 6, 9, 10, 12)] + others)
    kp, wr, wi = dev(np.full(npt, 1.0)), dev(np.linspace(0.9, 1.4, npt)), dev(np.full(npt, 0.2))
    good = [es_ctx.handle, p.handle, P(kp), P(wr), P(wi), npt, P(Dre), P(Dim), P(rel), P(st), P(outer), P(inner)]
    run(lib.es_cylt_complex_eval_points, good,
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
    run(lib.es_cylt_complex_find_roots, good,
        [({0: None}, INVALID, b""), ({1: None}, INVALID, b"null problem"), ({8: W_PER_ROW}, INVALID, b"w_mode"),
         ({3: -1}, INVALID, b"size"), ({5: -1}, INVALID, b"size"), ({7: -1}, INVALID, b"size"), ({12: -1}, INVALID, b"size"),
         ({12: 1001}, INVALID, b"size"), ({14: C.byref(neg)}, INVALID, b"size"), ({14: None}, INVALID, b"null pointer"),
         ({15: None}, INVALID, b"null pointer")]
        + [({i: None}, INVALID, b"null pointer") for i in (2, 4, 6, 9, 10, 11)]
        + [({14: C.byref(table(drop=c))}, INVALID, b"null root table arrays") for c in COLS] + others)
    es_ctx.synchronize()
    for c in COLS:
        assert bool((cols[c] == (SENT if c in COLS[:4] else SENT_I)).all()), c
    # empty sizes succeed and touch nothing
    c = r["c"]
    for shape in ((0, 7, 12), (1, 0, 12), (1, 7, 0), (0, 0, 0)):
        rc, n, t = raw_find_roots(c, p, None, None, None, W_ABSOLUTE, None, None, None, 12, 4, shape=shape)
        assert rc == 0 and n == 0, shape
        assert np.all(t["k"] == SENT) and np.all(t["flag"] == SENT_I)
    for a, b, d in ((0, 7, 12), (1, 0, 12)):
        assert lib.es_cylt_complex_eval_grid(es_ctx.handle, p.handle, None, a, None, b, None, d, 0, None, None, None, None) == 0
    assert lib.es_cylt_complex_eval_points(es_ctx.handle, p.handle, None, None, None, 0, None, None, None, None, None, None) == 0
    # the same arguments, unchanged, are a valid search; section 14 keeps refusing the twisted problem
    assert lib.es_cylt_complex_find_roots(*good) == 0
    es_ctx.synchronize()
    assert cnt.value == len(r["cells"])
    assert lib.es_cyl_complex_eval_points(es_ctx.handle, p.handle, P(kp), P(wr), P(wi), npt, P(Dre), P(Dim), P(rel), P(st), None,
                                          None) == UNSUPPORTED
    with pytest.raises(TypeError):
        RotatingCylinderComplex(q.CylinderFlow())
    with pytest.raises(TypeError):
        RotatingCylinderComplex(q.CylinderDensity())
    slab.close()
    untwisted.close()

"""es_complex_eigenfunction (C ABI section 6) against its NumPy restatement and DOP853 (tests/complex_eigen_model.py,
pinned on the CPU by tests/test_complex_eigen_model.py), against the existing complex entry points and, on the real
axis, against es_shoot_eigenfunction.

Shapes: n = 1 and n = 65 (two workgroups, 63 idle lanes in the barriers of the second); N = 130 (one full LDS chunk of
128 steps plus a chunk of one step) and N = 500 (three chunks plus 115 steps); n_ext in {0, 2, 500}; a different k in
every lane."""
import numpy as np
import pytest

from oracle.slab_complex import ComplexFlowSlab
from tests import complex_eigen_model as M

pytestmark = pytest.mark.gpu

FIELDS = ("value_int", "flux_int", "value_ext", "flux_ext")


def oracle_for(solver, mode):
    e = solver.eq
    return ComplexFlowSlab(c_i=e.c_i0, vA_i=e.vA_i0, c_e=e.c_e, vA_e=e.vA_e, rho_i=e.rho_i0, rho_e=e.rho_e, U_i0=e.U_i0,
                           U_e=e.U_e, width=e.width, mode=mode, L_factor=e.L_factor, ic=e.ic, n_nodes=e.n_nodes,
                           variant="sfx" if solver.variant == 0 else "sfg")


def host(ef):
    return {key: t.cpu().numpy() for key, t in ef.items()}


def random_pairs(n, seed):
    """A different k in every lane; frequencies drawn as in tests/test_complex_gpu.py:26."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.3, 2.7, n)
    w = rng.uniform(-0.5, 3.0, n) * k / 1.5 + 1j * rng.uniform(-0.4, 0.4, n)
    return k, w


def rows_close(a, b, tol):
    """max |a - b| <= tol max |b| row by row; NaN rows must be NaN in both.  Returns the largest ratio."""
    worst = 0.0
    for ra, rb in zip(a, b):
        if rb.size == 0:
            continue
        if np.all(np.isnan(rb)):
            assert np.all(np.isnan(ra))
            continue
        r = np.max(np.abs(ra - rb)) / np.max(np.abs(rb))
        worst = max(worst, r)
        assert r <= tol, r
    return worst


# ---- 1. GPU vs the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["sfx", "sfg"])
@pytest.mark.parametrize("width", [0.9, 1e5])
@pytest.mark.parametrize("mode", ["kink", "sausage"])
def test_matches_the_numpy_model(es_ctx, mode, width, variant):
    """Every array within 1e-10 of max|field| (the project's figure for the GPU against a NumPy restatement of the same
    algorithm, tests/test_complex_gpu.py:33); grids to 1e-15."""
    from eigensolver_amd import SlabComplexFlow
    n_ok = 0
    for N, n, n_ext in ((130, 65, 500), (500, 65, 2), (130, 1, 0), (500, 1, 500)):
        s = SlabComplexFlow(width=width, variant=variant, ctx=es_ctx, n_nodes=N)
        k, w = random_pairs(n, seed=7 + N + n)
        g = host(s.eigenfunction(mode, k, w, n_ext=n_ext))
        m = M.model(oracle_for(s, mode), k, w, n_ext=n_ext)
        assert g["value_int"].shape == (n, N) and g["x_ext"].shape == (n, n_ext) and g["flux_ext"].shape == (n, n_ext)
        assert g["value_int"].dtype == np.complex128 and g["status"].dtype == np.uint8
        assert np.array_equal(g["status"], m["status"])
        n_ok += int((m["status"] == 0).sum())
        assert np.max(np.abs(g["x_int"] - m["x_int"])) <= 1e-15
        if n_ext:
            assert np.max(np.abs(g["x_ext"] - m["x_ext"])) <= 1e-15
        for key in FIELDS:
            print(mode, width, variant, N, n, n_ext, key, rows_close(g[key], m[key], 1e-10))
        s.close()
    assert n_ok > 60


# ---- 2. GPU vs DOP853 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 500])
def test_matches_dop853(es_ctx, N):
    from eigensolver_amd import SlabComplexFlow
    for name, width, mode, variant, w in M.cases(N):
        s = SlabComplexFlow(width=width, variant=variant, ctx=es_ctx, n_nodes=N)
        g = host(s.eigenfunction(mode, M.K0, w, n_ext=500))
        t = M.truth_case(N, name)
        assert np.all(g["status"] == 0)
        for key in FIELDS:
            print(N, name, key, rows_close(g[key], t[key], M.bound(N)))
        s.close()


# ---- 3. consistency with the existing entry points ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["sfx", "sfg"])
@pytest.mark.parametrize("mode", ["kink", "sausage"])
def test_consistent_with_eval_points(es_ctx, mode, variant):
    from eigensolver_amd import SlabComplexFlow
    s = SlabComplexFlow(width=0.9, variant=variant, ctx=es_ctx, n_nodes=130)
    o = oracle_for(s, mode)
    k, w = random_pairs(65, seed=11)
    g = host(s.eigenfunction(mode, k, w, n_ext=2))
    D, st, rel = (t.cpu().numpy() for t in s.eval_points(mode, k, w))
    assert np.array_equal(g["status"], st)
    ok = st == 0
    assert ok.sum() > 30
    outer, inner = g["flux_ext"][ok, -1], g["flux_int"][ok, 0]
    scale = np.maximum(np.abs(outer), np.abs(inner))
    print(mode, variant, "D_c identity:", np.max(np.abs((outer - inner) - D[ok]) / scale), "bit-identical rows:",
          int(np.sum((outer - inner) == D[ok])), "of", int(ok.sum()))
    assert np.max(np.abs((outer - inner) - D[ok]) / scale) <= 1e-10
    assert np.max(np.abs(g["value_ext"][ok, -1] - 1.0)) <= 1e-12
    Vb = M.boundary_value(o, k, w)[ok]
    assert np.max(np.abs(g["value_int"][ok, 0] - Vb) / np.abs(Vb)) <= 1e-12
    vx = g["value_int"][ok]
    assert np.max(np.abs(vx[:, -1] - M.sigma(o) * vx[:, 0]) / np.max(np.abs(vx), axis=1)) <= 1e-10
    for key in FIELDS:
        assert np.all(np.isnan(g[key][~ok]))
    s.close()


# ---- 4. the known Kelvin-Helmholtz root -------------------------------------------------------------------------------------
def test_kelvin_helmholtz_mode(es_ctx):
    """find_roots -> eigenfunction on its tensors.  The interior Vx is the closed form Vb cosh(m x) / cosh(m); the total
    pressure is continuous: |flux_int[0] - flux_ext[-1]| = |D_c| = resid / 100 of their maximum, and the rows used have
    resid < 1e-2 percent."""
    import torch
    from eigensolver_amd import SlabComplexFlow
    s = SlabComplexFlow(width=1e5, variant="sfx", ctx=es_ctx)
    w_re, w_im = M.ROOT_WINDOW
    D, st, rel = s.eval_grid("kink", np.array([M.K0]), w_re, w_im)
    roots, cnt = s.find_roots("kink", np.array([M.K0]), w_re, w_im, D, st)
    acc = (roots["flag"] == 1) & (roots["resid"] < 1e-2)
    assert int(acc.sum()) >= 2
    ef = s.eigenfunction("kink", roots["k"][acc], roots["w"][acc])
    assert isinstance(ef["value_int"], torch.Tensor) and ef["value_int"].is_cuda
    g, w, resid = host(ef), roots["w"][acc].cpu().numpy(), roots["resid"][acc].cpu().numpy()
    assert np.min(np.abs(w - M.KH_ROOT)) < 1e-7 and np.all(g["status"] == 0)
    o = oracle_for(s, "kink")
    for i in range(len(w)):
        want = M.uniform_closed_form(o, M.K0, w[i], g["x_int"])
        assert np.max(np.abs(g["value_int"][i] - want)) <= 1e-8 * np.max(np.abs(want))
        fi, fe = g["flux_int"][i, 0], g["flux_ext"][i, -1]
        assert abs(fi - fe) <= (resid[i] / 100.0) * max(abs(fi), abs(fe)) * (1.0 + 1e-12)
        assert abs(fi - fe) <= 1e-4 * max(abs(fi), abs(fe))
    s.close()


# ---- 5. the real axis -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["kink", "sausage"])
def test_real_axis_is_the_real_eigenfunction(es_ctx, mode):
    """variant sfg at Im(omega) = 0: the fields of ShootProblem.eigenfunction times its boundary sign value_ext[i, -1] = +-1
    (the real path divides by |V_e(-1)|, the complex path by V_e(-1)).  Bound: the project's figure for the same comparison
    of D, 1e-10 of max|field| (tests/test_complex_gpu.py:76); imaginary parts below 1e-12 of max|field|."""
    from eigensolver_amd import ShootProblem, SlabComplexFlow, equilibrium as q
    eq = q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=130)
    s = SlabComplexFlow(equilibrium=eq, variant="sfg", ctx=es_ctx)
    gp = ShootProblem(eq, mode, ctx=es_ctx)
    k = np.repeat([0.6, 1.2, 2.4], 22)[:65]
    w = k * np.tile(np.linspace(0.05, 2.4, 22), 3)[:65]
    _, sr = gp.eval_points(k, w)
    c = host(s.eigenfunction(mode, k, w + 0j, n_ext=500))
    r = host(gp.eigenfunction(k, w, n_ext=500))
    ok = (sr.cpu().numpy() == 0) & (c["status"] == 0)
    assert ok.sum() > 15
    assert np.max(np.abs(np.abs(r["value_ext"][ok, -1]) - 1.0)) < 1e-12
    sign = np.sign(r["value_ext"][:, -1])
    assert np.max(np.abs(c["x_ext"] - r["x_ext"])) <= 1e-15
    worst = 0.0
    for key in FIELDS:
        for i in np.nonzero(ok)[0]:
            a, b = c[key][i], r[key][i] * sign[i]
            scale = np.max(np.abs(b))
            worst = max(worst, np.max(np.abs(a.real - b)) / scale)
            print(mode, key, i, np.max(np.abs(a.real - b)) / scale, np.max(np.abs(a.imag)) / scale)
            assert np.max(np.abs(a.real - b)) <= 1e-10 * scale, (key, i)
            assert np.max(np.abs(a.imag)) <= 1e-12 * scale, (key, i)
    print("real axis, worst difference / max|field|:", worst)
    gp.close()
    s.close()


# ---- 6. a leaky pair among good ones ------------------------------------------------------------------------------------------
def test_leaky_pair_does_not_disturb_its_neighbours(es_ctx):
    from eigensolver_amd import SlabComplexFlow
    s = SlabComplexFlow(width=0.9, variant="sfx", ctx=es_ctx, n_nodes=130)
    w = np.array([M.NON_ROOT, 0.1 - 0.2j, M.LEAKY, M.KH_ROOT, M.NON_ROOT])
    g = host(s.eigenfunction("kink", M.K0, w, n_ext=500))
    assert list(g["status"]) == [0, 0, 1, 0, 0]
    for key in FIELDS:
        assert np.all(np.isnan(g[key][2].real)) and np.all(np.isnan(g[key][2].imag))
    assert np.all(np.isfinite(g["x_ext"][2])) and g["x_ext"][2, -1] == -1.0
    for i in (0, 1, 3, 4):
        alone = host(s.eigenfunction("kink", M.K0, w[i:i + 1], n_ext=500))
        for key in FIELDS + ("x_ext",):
            assert np.array_equal(alone[key][0], g[key][i]), (key, i)
    s.close()


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------
def test_arguments(es_ctx):
    import torch
    from eigensolver_amd import ShootProblem, SlabComplexFlow, _lib, equilibrium as q
    lib = es_ctx.lib
    s = SlabComplexFlow(width=0.9, ctx=es_ctx, n_nodes=130)
    p = s.problem("kink")
    n, N, n_ext = 3, 130, 4
    dev = "cuda"
    k = torch.full((n,), M.K0, dtype=torch.float64, device=dev)
    wre = torch.tensor([0.21, 0.1, 0.3], dtype=torch.float64, device=dev)
    wim = torch.tensor([0.13, -0.2, 0.05], dtype=torch.float64, device=dev)
    vi, fi = (torch.empty((n, N), dtype=torch.complex128, device=dev) for _ in range(2))
    ve, fe = (torch.empty((n, n_ext), dtype=torch.complex128, device=dev) for _ in range(2))
    xe = torch.empty((n, n_ext), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    ptr = _lib.ptr

    def call(prob, variant, n_, n_ext_, status, k_=k):
        return lib.es_complex_eigenfunction(es_ctx.handle, prob, variant, ptr(k_) if k_ is not None else None, ptr(wre),
                                            ptr(wim), n_, ptr(vi), ptr(fi), n_ext_, ptr(xe), ptr(ve), ptr(fe), status)

    cyl = ShootProblem(q.CylinderFlow(U_i0=0.6, width=1.0), "kink", ctx=es_ctx)
    assert call(cyl.handle, 0, n, n_ext, ptr(st)) == 5                          # ES_ERR_UNSUPPORTED
    assert b"SLAB_FLOW" in lib.es_last_error(es_ctx.handle)
    cyl.close()
    assert call(p.handle, 2, n, n_ext, ptr(st)) == 1                            # variant
    assert call(None, 0, n, n_ext, ptr(st)) == 1
    assert call(p.handle, 0, -1, n_ext, ptr(st)) == 1
    assert call(p.handle, 0, n, 1, ptr(st)) == 1                                # n_ext = 1
    assert b"n_ext" in lib.es_last_error(es_ctx.handle)
    assert call(p.handle, 0, n, n_ext, ptr(st), k_=None) == 1                   # null input
    assert lib.es_complex_eigenfunction(es_ctx.handle, p.handle, 0, ptr(k), ptr(wre), ptr(wim), n, ptr(vi), ptr(fi), n_ext,
                                        None, ptr(ve), ptr(fe), ptr(st)) == 1   # null exterior array with n_ext > 0
    # n = 0: success, nothing touched (null pointers are fine)
    vi.fill_(7.0)
    assert lib.es_complex_eigenfunction(es_ctx.handle, p.handle, 0, None, None, None, 0, None, None, n_ext, None, None,
                                        None, None) == 0
    torch.cuda.synchronize()
    assert bool((vi == 7.0).all())
    # n_ext = 0 needs no exterior arrays; d_status = NULL is accepted and changes nothing
    assert lib.es_complex_eigenfunction(es_ctx.handle, p.handle, 0, ptr(k), ptr(wre), ptr(wim), n, ptr(vi), ptr(fi), 0, None,
                                        None, None, ptr(st)) == 0
    assert call(p.handle, 0, n, n_ext, ptr(st)) == 0
    torch.cuda.synchronize()
    ref = [t.clone() for t in (vi, fi, xe, ve, fe)]
    assert st.cpu().tolist() == [0, 0, 0]
    for t in (vi, fi, xe, ve, fe):
        t.zero_()
    assert call(p.handle, 0, n, n_ext, None) == 0
    torch.cuda.synchronize()
    for a, b in zip(ref, (vi, fi, xe, ve, fe)):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)
    s.close()

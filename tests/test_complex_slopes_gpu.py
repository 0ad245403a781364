"""es_complex_root_slopes and es_complex_newton (include/eigensolver_amd.h section 12) on the GPU, with the Python layer on top
(SlabComplexFlow.root_slopes / group_velocity / newton / densify, postprocess.most_unstable).

Yardsticks (tests/complex_slope_model.py, pinned on the CPU by tests/test_complex_slope_model.py):
  value    outer - inner of row 0 against the D_c of es_complex_eval_points at the same pairs: 1e-12 of max(|outer|, |inner|),
           the bound tests/test_root_slopes_gpu.py uses for the same comparison -- and bit for bit, since both paths run the
           one text of es_complex_shared.hpp (so is the resid of a Newton call that takes no step against rel).
  jets     the NumPy forward-mode restatement of the oracle: every row of outer and inner within 1e-10 of
           max(|outer_x|, |inner_x|), the project's bound for the GPU against a NumPy restatement.
  slope    d omega / dk against the slope of the oracle's root curve, with the bounds the CPU test fixed.
  Newton   the iteration rule restated on the model: the same number of steps, |w - w_model| <= 1e-12 max(1, |w|).
Node counts: N = 2 and 3 (one and two RK4 steps), 129 and 130 (128 steps: one full LDS chunk; 129: a chunk of one step on
top), 60 (roots close to the real axis, beside critical layers).  `pytest -s` prints every measured figure next to its bound.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import complex_slope_model as C  # noqa: E402

SENT_D, SENT_S, SENT_I = -7.25e77, 0xEE, -77
NODES = (2, 3, 60, 129, 130)
REAL_PAIRS = (0.4 + 0.0j, -0.2 + 0.0j)


class _Pool:
    """one SlabComplexFlow per (width, variant, N) on the session's context"""
    def __init__(self, ctx):
        self.ctx, self.s = ctx, {}

    def solver(self, width, variant, N):
        key = (width, variant, N)
        if key not in self.s:
            from eigensolver_amd import SlabComplexFlow
            self.s[key] = SlabComplexFlow(width=width, variant=variant, ctx=self.ctx, n_nodes=N)
        return self.s[key]

    def close(self):
        for s in self.s.values():
            s.close()


@pytest.fixture(scope="module")
def pool(es_ctx):
    p = _Pool(es_ctx)
    yield p
    p.close()


def _np(s):
    return dict(outer=s.outer.cpu().numpy(), inner=s.inner.cpu().numpy(), status=s.status.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _pairs(width, mode, variant, N):
    """KH_ROOT, NON_ROOT, the roots the oracle's find_roots flags on ROOT_WINDOW, two pairs with Im omega = 0; k = K0"""
    return np.array([C.KH_ROOT, C.NON_ROOT, *C.window_roots(width, mode, variant, N), *REAL_PAIRS])


_GPU = {}


def _gpu_case(pool, width, mode, variant, N):
    """root_slopes and eval_points of a case at _pairs, one launch each per session"""
    key = (width, mode, variant, N)
    if key not in _GPU:
        s = pool.solver(width, variant, N)
        w = _pairs(*key)
        D, st, _ = s.eval_points(mode, C.K0, w)
        _GPU[key] = (_np(s.root_slopes(mode, C.K0, w)), D.cpu().numpy(), st.cpu().numpy())
    return _GPU[key]


CASES = [(width, mode, variant) for width in (1e5, 0.9) for mode in ("kink", "sausage") for variant in ("sfx", "sfg")]


# ---- value and jets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,mode,variant", CASES)
def test_value_is_the_determinant_of_eval_points(pool, width, mode, variant):
    for N in NODES:
        g, D, st = _gpu_case(pool, width, mode, variant, N)
        assert g["status"].tolist() == st.tolist() == [0] * len(D)
        assert g["outer"].dtype == np.complex128 and g["outer"].shape == (3, len(D))
        sc = np.maximum(np.abs(g["outer"][0]), np.abs(g["inner"][0]))
        err = np.abs((g["outer"][0] - g["inner"][0]) - D) / sc
        print(f"{mode} {variant} width {width} N {N}: worst |(outer - inner) - D_c| / max(|outer|, |inner|) = {err.max():.2e} "
              f"over {len(D)} pairs (bound 1.0e-12)")
        assert err.max() <= 1e-12, (N, err)
        # one text at the scalars cz and CJet<2>, no contraction: row 0 is the value path's arithmetic, operation for operation
        assert np.array_equal(g["outer"][0] - g["inner"][0], D), N


@pytest.mark.parametrize("width,mode,variant", CASES)
def test_jets_against_the_model(pool, width, mode, variant):
    for N in NODES:
        g, _, _ = _gpu_case(pool, width, mode, variant, N)
        w = _pairs(width, mode, variant, N)
        mo, mi, mst = C.jets(C.slab(width, mode, variant, N), C.K0, w)
        assert g["status"].tolist() == mst.tolist() == [0] * len(w)
        for c, what in ((0, "value"), (1, "d/dw"), (2, "d/dk")):
            sc = np.maximum(np.abs(mo[c]), np.abs(mi[c]))
            eo, ei = np.abs(g["outer"][c] - mo[c]) / sc, np.abs(g["inner"][c] - mi[c]) / sc
            print(f"{mode} {variant} width {width} N {N} {what}: outer {eo.max():.2e}, inner {ei.max():.2e} of "
                  f"max(|outer_x|, |inner_x|) over {len(w)} pairs (bound 1.0e-10)")
            assert eo.max() <= 1e-10 and ei.max() <= 1e-10, (N, what, w, eo, ei)


def test_slope_is_the_slope_of_the_root_curve(pool):
    for name, (o, k, root, slope) in C.slope_cases().items():
        s = pool.solver(o.width, o.variant, o.n_nodes)
        r = s.root_slopes(o.mode, k, [root])
        assert r.status.cpu().numpy().tolist() == [0]
        got = complex(r.group_velocity.cpu().numpy()[0])
        err = abs(got - slope) / max(1.0, abs(slope))
        print(f"{name}: d omega / dk = {got:.12f}, curve slope {slope:.12f}, |difference| = {err:.2e} "
              f"(bound {10 * C.SLOPE_MEASURED[name]:.1e}), |Newton correction| = {abs(r.newton_dw.cpu().numpy()[0]):.1e}")
        assert err <= 10.0 * C.SLOPE_MEASURED[name]
        table = dict(k=np.array([k]), w=np.array([root]))
        assert np.array_equal(s.group_velocity(o.mode, table).cpu().numpy(), r.group_velocity.cpu().numpy())


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------
def _dev(pool, a, dtype):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype), device=f"cuda:{pool.ctx.device}")


def _raw_slopes(pool, s, mode, k, w, n, count=None, skip=(), prob=True, variant=None, null_in=False, handle=None):
    """es_complex_root_slopes into buffers pre-filled with sentinels ([3, n] complex and [n], at least one entry); outputs
    named in `skip` are passed as NULL.  Returns (return code, dict of the three arrays)."""
    import torch
    from eigensolver_amd import _lib
    na = max(n, 1)
    w = np.asarray(w, dtype=complex)
    dk, dre, dim = _dev(pool, np.broadcast_to(k, w.shape), np.float64), _dev(pool, w.real, np.float64), _dev(pool, w.imag, np.float64)
    dev = dk.device
    bufs = dict(outer=torch.full((3, na), SENT_D, dtype=torch.complex128, device=dev),
                inner=torch.full((3, na), SENT_D, dtype=torch.complex128, device=dev),
                status=torch.full((na,), SENT_S, dtype=torch.uint8, device=dev))
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    ph = handle if handle is not None else (s.problem(mode).handle if prob else None)
    rc = pool.ctx.lib.es_complex_root_slopes(pool.ctx.handle, ph, s.variant if variant is None else variant,
                                             *[None if null_in else _lib.ptr(t) for t in (dk, dre, dim)], n,
                                             _lib.ptr(dc) if dc is not None else None,
                                             *[None if f in skip else _lib.ptr(bufs[f]) for f in ("outer", "inner", "status")])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


NEWTON_OUT = ("w_re", "w_im", "resid", "dwdk", "iters", "flag")


def _raw_newton(pool, s, mode, k, guess, n, count=None, max_iter=8, step_cap=1e300, max_shift=1e300, tol=4.0, skip=(),
                prob=True, variant=None, null_in=False):
    import torch
    from eigensolver_amd import _lib
    na = max(n, 1)
    g = np.asarray(guess, dtype=complex)
    dk, dre, dim = _dev(pool, np.broadcast_to(k, g.shape), np.float64), _dev(pool, g.real, np.float64), _dev(pool, g.imag, np.float64)
    dev = dk.device
    bufs = {f: torch.full((na,), SENT_D, dtype=torch.float64, device=dev) for f in ("w_re", "w_im", "resid")}
    bufs["dwdk"] = torch.full((na,), SENT_D, dtype=torch.complex128, device=dev)
    bufs["iters"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    bufs["flag"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_complex_newton(pool.ctx.handle, s.problem(mode).handle if prob else None,
                                        s.variant if variant is None else variant,
                                        *[None if null_in else _lib.ptr(t) for t in (dk, dre, dim)], n,
                                        _lib.ptr(dc) if dc is not None else None, max_iter, step_cap, max_shift, tol,
                                        *[None if f in skip else _lib.ptr(bufs[f]) for f in NEWTON_OUT])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _same(a, b, fields):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


SLOPE_OUT = ("outer", "inner", "status")


def test_leaky_pair_in_the_middle(pool):
    """LEAKY among good pairs: its status is set, its six outputs are NaN, the others are bit for bit what they are in a
    call without it."""
    s = pool.solver(0.9, "sfx", 130)
    w = np.array([C.KH_ROOT, C.NON_ROOT, C.NON_ROOT + 0.05, C.KH_ROOT - 0.1j, 0.4 + 0.0j])
    rc, good = _raw_slopes(pool, s, "kink", C.K0, w, 5)
    assert rc == 0 and good["status"].tolist() == [0] * 5 and np.isfinite(good["outer"]).all()
    w[2] = C.LEAKY
    rc, got = _raw_slopes(pool, s, "kink", C.K0, w, 5)
    assert rc == 0 and got["status"].tolist() == [0, 0, 1, 0, 0]
    assert np.isnan(got["outer"][:, 2].real).all() and np.isnan(got["outer"][:, 2].imag).all()
    assert np.isnan(got["inner"][:, 2].real).all() and np.isnan(got["inner"][:, 2].imag).all()
    for i in (0, 1, 3, 4):
        assert np.array_equal(got["outer"][:, i], good["outer"][:, i]) and np.array_equal(got["inner"][:, i], good["inner"][:, i])


def test_ragged_workgroups(pool):
    """n = 65 (a second workgroup with one live lane) and n = 1: every copy of a pair equals its first, bit for bit."""
    s = pool.solver(0.9, "sfg", 129)
    w = _pairs(0.9, "sausage", "sfg", 129)
    k = C.K0 + 0.1 * np.arange(len(w))
    rc, first = _raw_slopes(pool, s, "sausage", k, w, len(w))
    assert rc == 0 and np.all(first["status"] == 0) and np.isfinite(first["outer"]).all()
    assert len({complex(x) for x in first["outer"][1]}) == len(w)                        # the pairs differ
    rc, out = _raw_slopes(pool, s, "sausage", np.resize(k, 65), np.resize(w, 65), 65)
    assert rc == 0 and np.all(out["status"] == 0)
    for i in range(65):
        j = i % len(w)
        assert np.array_equal(out["outer"][:, i], first["outer"][:, j]) and np.array_equal(out["inner"][:, i], first["inner"][:, j]), i
    rc, one = _raw_slopes(pool, s, "sausage", k[3:4], w[3:4], 1)
    assert rc == 0 and _same(one, {f: first[f][..., 3:4] for f in SLOPE_OUT}, SLOPE_OUT)
    rc, nw = _raw_newton(pool, s, "sausage", np.resize(k, 65), np.resize(w, 65), 65, max_iter=2)
    rc1, n1 = _raw_newton(pool, s, "sausage", k, w, len(w), max_iter=2)
    assert rc == 0 and rc1 == 0
    for i in range(65):
        assert all(np.array_equal(nw[f][i], n1[f][i % len(w)], equal_nan=True) for f in NEWTON_OUT), i


def test_device_count(pool):
    s = pool.solver(0.9, "sfx", 3)
    w = np.resize(np.array(C.n3_roots()) + 1e-3, 8)
    k = C.K0 + 1e-3 * np.arange(8)
    rc, full = _raw_slopes(pool, s, "kink", k, w, 8)
    rcn, nfull = _raw_newton(pool, s, "kink", k, w, 8)
    assert rc == 0 and rcn == 0 and np.all(full["status"] == 0) and np.all(nfull["flag"] == 1)
    assert np.all(nfull["iters"] >= 2) and np.isfinite(nfull["resid"]).all()
    for count, written in ((3, 3), (0, 0), (100, 8), (-2, 0)):
        rc, out = _raw_slopes(pool, s, "kink", k, w, 8, count=count)
        assert rc == 0
        for f in SLOPE_OUT:
            assert np.array_equal(out[f][..., :written], full[f][..., :written]), (count, f)     # rows stay 8 apart
            assert np.all(out[f][..., written:] == (SENT_S if f == "status" else SENT_D)), (count, f)
        rc, out = _raw_newton(pool, s, "kink", k, w, 8, count=count)
        assert rc == 0
        for f in NEWTON_OUT:
            assert np.array_equal(out[f][:written], nfull[f][:written]), (count, f)
            assert np.all(out[f][written:] == (SENT_I if f in ("iters", "flag") else SENT_D)), (count, f)


def test_each_output_may_be_null_and_n_zero(pool):
    s = pool.solver(0.9, "sfx", 3)
    w = np.array(C.n3_roots()) + 1e-3
    rc, full = _raw_slopes(pool, s, "kink", C.K0, w, 2)
    assert rc == 0 and np.all(full["status"] == 0)
    for f in SLOPE_OUT:
        rc, out = _raw_slopes(pool, s, "kink", C.K0, w, 2, skip=(f,))
        assert rc == 0
        assert _same(out, full, [g for g in SLOPE_OUT if g != f]), f
        assert np.all(out[f] == (SENT_S if f == "status" else SENT_D)), f
    rc, _ = _raw_slopes(pool, s, "kink", C.K0, w, 2, skip=SLOPE_OUT)
    assert rc == 0
    rc, out = _raw_slopes(pool, s, "kink", C.K0, w, 0, null_in=True)            # n = 0 with NULL arrays: nothing touched
    assert rc == 0 and np.all(out["outer"] == SENT_D) and np.all(out["status"] == SENT_S)
    rcn, nfull = _raw_newton(pool, s, "kink", C.K0, w, 2)
    rc, out = _raw_newton(pool, s, "kink", C.K0, w, 2, skip=("dwdk",))          # the one optional output of the Newton call
    assert rcn == 0 and rc == 0 and _same(out, nfull, [f for f in NEWTON_OUT if f != "dwdk"]) and np.all(out["dwdk"] == SENT_D)
    rc, out = _raw_newton(pool, s, "kink", C.K0, w, 0, null_in=True, skip=NEWTON_OUT)
    assert rc == 0


def test_argument_errors(pool):
    from eigensolver_amd import ShootProblem, _lib
    from eigensolver_amd import equilibrium as q
    s = pool.solver(0.9, "sfx", 3)
    w = np.array(C.n3_roots()) + 1e-3
    untouched_s = lambda o: np.all(o["outer"] == SENT_D) and np.all(o["inner"] == SENT_D) and np.all(o["status"] == SENT_S)
    untouched_n = lambda o: all(np.all(o[f] == (SENT_I if f in ("iters", "flag") else SENT_D)) for f in NEWTON_OUT)
    for kwargs in (dict(n=-1), dict(n=2, null_in=True), dict(n=2, prob=False), dict(n=2, variant=2), dict(n=2, variant=-1)):
        n = kwargs.pop("n")
        rc, out = _raw_slopes(pool, s, "kink", C.K0, w, n, **kwargs)
        assert rc == 1 and untouched_s(out), kwargs                                    # ES_ERR_INVALID_ARG
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
        rc, out = _raw_newton(pool, s, "kink", C.K0, w, n, **kwargs)
        assert rc == 1 and untouched_n(out), kwargs
    for kwargs in (dict(max_iter=-1), dict(step_cap=0.0), dict(step_cap=-1.0), dict(max_shift=0.0), dict(max_shift=-2.0),
                   dict(tol=0.0), dict(tol=-4.0), dict(step_cap=float("nan")), dict(skip=("w_re",)), dict(skip=("resid",)),
                   dict(skip=("iters",)), dict(skip=("flag",))):
        rc, out = _raw_newton(pool, s, "kink", C.K0, w, 2, **kwargs)
        assert rc == 1 and untouched_n(out), kwargs
    dens = ShootProblem(q.SlabDensity(n_nodes=130), "kink", ctx=pool.ctx)               # not a flow slab
    try:
        rc, out = _raw_slopes(pool, s, "kink", C.K0, w, 2, handle=dens.handle)
        assert rc == 5 and untouched_s(out)                                            # ES_ERR_UNSUPPORTED, as check_cx reports
        with pytest.raises(_lib.EsError):
            _lib.check(pool.ctx.handle, rc)
    finally:
        dens.close()
    g = _np(s.root_slopes("kink", C.K0, w))                                            # the context is still usable
    assert g["status"].tolist() == [0, 0] and np.isfinite(g["outer"]).all()


# ---- Newton -----------------------------------------------------------------------------------------------------------------
def _host(d):
    return {f: t.cpu().numpy() for f, t in d.items()}


def _check_newton(g, models, what):
    for i, m in enumerate(models):
        dw = abs(g["w"][i] - m["w"]) / max(1.0, abs(m["w"]))
        print(f"{what} lane {i}: iters {g['iters'][i]} (model {m['iters']}), |w - w_model| / max(1, |w|) = {dw:.2e} "
              f"(bound 1.0e-12), flag {g['flag'][i]} (model {m['flag']}), resid {g['resid'][i]:.1e} %")
        assert g["iters"][i] == m["iters"] and dw <= 1e-12 and g["flag"][i] == m["flag"], (what, i, g["w"][i], m)
        if m["status"] == 0:
            assert abs(g["dwdk"][i] - m["dwdk"]) <= 1e-9 * max(1.0, abs(m["dwdk"])), (what, i)


def test_newton_against_the_model(pool):
    o = C.slab(1e5, "kink", "sfx", 130)
    root = C.oracle_root(o, C.K0, C.KH_ROOT)
    g = _host(pool.solver(1e5, "sfx", 130).newton("kink", C.K0, [root + C.NEWTON_OFFSET]))
    m = C.newton_model(o, C.K0, root + C.NEWTON_OFFSET)
    _check_newton(g, [m], "uniform root + 0.02+0.015j")
    assert m["flag"] == 1 and m["iters"] <= 5 and abs(g["w"][0] - root) <= 1e-13
    o3 = C.slab(0.9, "kink", "sfx", 3)
    starts = [z + sgn * 1e-3 * (1 + 1j) for z in C.n3_roots() for sgn in (1, -1)]
    g = _host(pool.solver(0.9, "sfx", 3).newton("kink", C.K0, starts))
    _check_newton(g, [C.newton_model(o3, C.K0, z) for z in starts], "N = 3 roots +- 1e-3 (1 + i)")
    assert g["flag"].tolist() == [1] * 4 and g["w"].dtype == np.complex128 and g["iters"].dtype == np.int32


# offsets from the two N = 3 roots whose Newton runs take 1 to 8 steps (tests/complex_slope_model.py newton_model)
HAZARD_OFFSETS = ((0, 1e-9, 1e-6 * (1 - 1j), 1e-4j, 5e-3, 1e-2 * (1 - 1j)), (0, 1e-9, 1e-4j, 5e-3, 1e-2 * (1 - 1j), 2e-2 * (1 + 1j)))


def test_newton_lanes_stop_at_different_steps(pool):
    """Lanes of one workgroup that converge after 1, 2, ... 8 steps, a leaky guess among them: a lane that has stopped keeps
    marching on frozen inputs for the barriers of the others, and every lane must still match its own model run."""
    o3 = C.slab(0.9, "kink", "sfx", 3)
    s = pool.solver(0.9, "sfx", 3)
    starts = [z + off for z, offs in zip(C.n3_roots(), HAZARD_OFFSETS) for off in offs]
    models = [C.newton_model(o3, C.K0, z) for z in starts]
    assert len({m["iters"] for m in models}) >= 6 and all(m["flag"] == 1 for m in models)
    g = _host(s.newton("kink", C.K0, starts))
    _check_newton(g, models, "mixed step counts")
    with_leaky = starts[:5] + [C.LEAKY] + starts[5:]
    h = _host(s.newton("kink", C.K0, with_leaky))
    assert h["flag"][5] == 0 and h["iters"][5] == 0 and h["w"][5] == C.LEAKY and np.isnan(h["resid"][5])
    assert np.isnan(h["dwdk"][5].real) and np.isnan(h["dwdk"][5].imag)
    for f in ("w", "resid", "iters", "flag", "dwdk"):
        assert np.array_equal(np.delete(h[f], 5), g[f]), f                              # the neighbours are undisturbed


def test_newton_guards(pool):
    o3 = C.slab(0.9, "kink", "sfx", 3)
    s = pool.solver(0.9, "sfx", 3)
    root = C.n3_roots()[1]
    guess = root + 0.01 * (1 - 1j)
    # max_iter = 0: the guess with its residual and slope
    g = _host(s.newton("kink", C.K0, [guess], max_iter=0))
    outer, inner, _ = C.jets(o3, C.K0, guess)
    resid = abs(outer[0, 0] - inner[0, 0]) * 100.0 / max(abs(outer[0, 0]), abs(inner[0, 0]))
    assert g["w"][0] == guess and g["iters"][0] == 0 and abs(g["resid"][0] - resid) <= 1e-9 * resid
    assert g["flag"][0] == (1 if resid < 4.0 else 0)
    assert abs(g["dwdk"][0] - C.dwdk(outer, inner)[0]) <= 1e-9 * abs(C.dwdk(outer, inner)[0])
    # step_cap: the first step is exactly that long
    g = _host(s.newton("kink", C.K0, [guess], max_iter=1, step_cap=1e-3))
    m = C.newton_model(o3, C.K0, guess, max_iter=1, step_cap=1e-3)
    print(f"capped step: |w - guess| = {abs(g['w'][0] - guess):.17e}")
    assert g["iters"][0] == 1 and abs(abs(g["w"][0] - guess) - 1e-3) <= 1e-15 and abs(g["w"][0] - m["w"]) <= 1e-12
    # max_shift smaller than the distance travelled: flag 0, w still reported
    g = _host(s.newton("kink", C.K0, [guess, guess], max_shift=5e-3))
    assert g["flag"].tolist() == [0, 0] and abs(g["w"][0] - root) <= 1e-12 and g["resid"][0] < 1e-6
    g = _host(s.newton("kink", C.K0, [guess], max_shift=2e-2, tol_percent=1e-6))
    assert g["flag"].tolist() == [1] and abs(g["w"][0] - root) <= 1e-12


@pytest.mark.parametrize("N", (3, 130))
def test_newton_without_steps_is_eval_points(pool, N):
    """max_iter = 0 on 65 guesses (one full workgroup and a ragged one), a different k in every lane, the leaky pair among
    them: w is the guess and resid the rel of es_complex_eval_points at the guesses, bit for bit (one text at the scalars
    cz and CJet<2>); flag = 1 where the point is ES_PT_OK with rel < tol_percent."""
    s = pool.solver(0.9, "sfx", N)
    guess = C.NON_ROOT + 0.004 * np.arange(65) * (1 - 0.5j)
    k = C.K0 + 1e-3 * np.arange(65)
    guess[40], k[40] = C.LEAKY, C.K0
    _, st, rel = s.eval_points("kink", k, guess)
    st, rel = st.cpu().numpy(), rel.cpu().numpy()
    assert st[40] == 1 and np.all(np.delete(st, 40) == 0) and np.isfinite(np.delete(rel, 40)).all()
    tol = float(np.median(np.delete(rel, 40)))                                          # none of the guesses is a root
    g = _host(s.newton("kink", k, guess, max_iter=0, tol_percent=tol))
    assert np.array_equal(g["w"].real, guess.real) and np.array_equal(g["w"].imag, guess.imag)
    assert g["iters"].tolist() == [0] * 65
    assert np.array_equal(g["resid"], rel, equal_nan=True)
    assert np.isnan(g["resid"][40]) and np.isnan(rel[40]) and g["flag"][40] == 0
    assert g["flag"].tolist() == [1 if (a == 0 and r < tol) else 0 for a, r in zip(st, rel)]
    assert 0 < g["flag"].sum() < 64


# ---- densify and most_unstable ----------------------------------------------------------------------------------------------
def _follow(o, k_from, w_from, ks):
    """the oracle's branch through (k_from, w_from) at the wavenumbers ks (monotone, starting next to k_from): secant-polished
    roots, each start predicted with the model's slope at the previous root"""
    out, k, w = [], k_from, w_from
    for kk in ks:
        outer, inner, _ = C.jets(o, k, w)
        w = C.oracle_root(o, kk, w + C.dwdk(outer, inner)[0] * (kk - k))
        k = kk
        out.append(w)
    return np.array(out)


def test_densify_follows_the_branch(pool):
    """width 0.9, N = 3, kink "sfx": coarse rows k = 0.5, 1.0, ... 3.0 on the branch from 0.164226+0.151410j, k_fine spaced
    0.125.  Hermite prediction measured at 2.8e-4 of the root on the CPU; 1e-3 covers the end intervals."""
    o3 = C.slab(0.9, "kink", "sfx", 3)
    kf = 0.5 + 0.125 * np.arange(21)
    branch = _follow(o3, 0.5, C.oracle_root(o3, 0.5, C.N3_UPPER), kf)
    assert abs(branch[0] - C.N3_UPPER) < 1e-6
    s = pool.solver(0.9, "sfx", 3)
    d = _host(s.densify("kink", kf[::4], branch[::4], kf))
    err, pred = np.abs(d["w"] - branch), np.abs(d["predicted"] - d["w"])
    print(f"densify: worst |w - oracle root| = {err.max():.2e} (bound 1.0e-10), worst |predicted - w| = {pred.max():.2e} "
          f"(bound 1.0e-3), iters {d['iters'].tolist()}, smallest max_shift {d['max_shift'].min():.2e}")
    assert d["flag"].tolist() == [1] * 21 and np.array_equal(d["k"], kf)
    assert err.max() <= 1e-10 and pred.max() <= 1e-3
    outer, inner, _ = C.jets(o3, kf, branch)
    assert np.max(np.abs(d["dwdk"] - C.dwdk(outer, inner))) <= 1e-9
    # a max_shift of the caller's goes to the Newton call as it is
    d2 = _host(s.densify("kink", kf[::4], branch[::4], kf, max_shift=1e-5))
    assert d2["flag"].tolist() == [1 if p <= 1e-5 else 0 for p in np.abs(d2["w"] - d2["predicted"])] and 0 < d2["flag"].sum() < 21


def test_most_unstable_wavenumber(pool):
    """Uniform-flow kink branch on k in [0.1, 0.6] from 6 coarse rows (the oracle follows the branch down to k = 0.1): one
    growth-rate maximum, inside (0.1, 0.5), and the densified curve peaks there."""
    from eigensolver_amd import postprocess as pp
    o = C.slab(1e5, "kink", "sfx", 130)
    root = C.oracle_root(o, C.K0, C.KH_ROOT)
    down = _follow(o, C.K0, root, np.linspace(0.5, 0.1, 9)[1:])
    ks = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    ws = np.array([down[7], down[5], down[3], down[1], root, _follow(o, C.K0, root, [0.6])[0]])
    assert np.all(ws.imag > 0.02)
    s = pool.solver(1e5, "sfx", 130)
    slopes = s.group_velocity("kink", dict(k=ks, w=ws)).cpu().numpy()
    kstar, wstar = pp.most_unstable(ks, ws, slopes)
    print(f"most unstable: k* = {kstar}, omega* = {wstar}, Im d omega / dk at the rows = {slopes.imag}")
    assert kstar.shape == (1,) and 0.1 < kstar[0] < 0.5
    kk = np.array([kstar[0] - 0.02, kstar[0], kstar[0] + 0.02])
    d = _host(s.densify("kink", ks, ws, kk))
    print(f"Im omega at k* - 0.02, k*, k* + 0.02: {d['w'].imag}, |predicted - w| = {np.abs(d['predicted'] - d['w'])}")
    assert d["flag"].tolist() == [1, 1, 1]
    assert d["w"][1].imag >= d["w"][0].imag and d["w"][1].imag >= d["w"][2].imag
    assert abs(d["w"][1] - wstar[0]) <= 1e-3 and abs(d["dwdk"][1].imag) <= 1e-2


# ---- the real axis ----------------------------------------------------------------------------------------------------------
def test_real_axis_slope_is_the_real_group_speed(pool):
    """At the real roots of the SFG flow slab: Re d omega / dk of the complex path ("sfg", Im omega = 0) is
    ShootProblem.group_velocity and the imaginary part vanishes, both within 10 x the difference of the two NumPy models."""
    from eigensolver_amd import ShootProblem, SlabComplexFlow
    eq, k, w, _, _ = C.real_axis_case()
    bound = 10.0 * C.REAL_AXIS_MEASURED
    s = SlabComplexFlow(equilibrium=eq, variant="sfg", ctx=pool.ctx)
    gp = ShootProblem(eq, "kink", ctx=pool.ctx)
    try:
        cx = s.group_velocity("kink", dict(k=k, w=w + 0j)).cpu().numpy()
        cg = gp.group_velocity(dict(k=k, w=w)).cpu().numpy()
    finally:
        s.close()
        gp.close()
    sc = np.maximum(1.0, np.abs(cg))
    ere, eim = np.abs(cx.real - cg) / sc, np.abs(cx.imag) / sc
    print(f"{C.REAL_AXIS_CASE}: {len(k)} real roots, worst |Re d omega / dk - c_g| = {ere.max():.2e}, worst |Im| = {eim.max():.2e} "
          f"of max(1, |c_g|) (bound {bound:.1e})")
    assert ere.max() <= bound and eim.max() <= bound

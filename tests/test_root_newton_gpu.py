"""es_shoot_newton (include/eigensolver_amd.h section 13) on the GPU, with ShootProblem.newton / densify / trace_branches and
postprocess.traced_curves on top.

Yardsticks (tests/real_newton_model.py, pinned on the CPU by tests/test_real_newton_model.py):
  model     the rule of section 13 in NumPy over the complex-step jets of tests/root_slope_model.py, from offset guesses.
            iters is compared on the lanes the CPU test calls clear (no step within a factor 10 of the stopping threshold),
            omega, dwdk and resid on all lanes:
              omega  10 x the worst |w - w_model| / max(1, |w|) measured on the GPU (OMEGA_MEASURED), and at most 1e-10;
              dwdk   1e-10 of max(1, |slope|), the bound of the jet tests of section 11;
              resid  the two sides agree with the model within 1e-10 of their scale each (the same jet bound), so 100 |D| / scale
                     within 2e-8 (percent), plus what the difference in omega moves it by, 100 |D_w| |dw| / scale.
  bits      with max_iter = 0: w is the guess, resid is formed from the outer and inner of root_slopes at the same pairs, and
            status is that of eval_points, continuum and leaky pairs included.
  port      the C port's root next to every traced root (a window shifted off the candidate by a third of a cell): 1e-10 of
            max(1, |w|), the project's asserted root bound.
`pytest -s` prints every measured figure next to its bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mode_signature_model as S  # noqa: E402
from tests import real_eigen_model as M  # noqa: E402
from tests import real_newton_model as N  # noqa: E402

SENT_D, SENT_I, SENT_S = -7.25e77, -77, 0xEE
OUT = ("w", "resid", "dwdk", "iters", "flag", "status")
# worst |w - w_model| / max(1, |w|) over the 104 lanes of the MODEL_CASES, measured on an MI355X: 7.42e-16 (CR_kink lane 8;
# DESIGN.md section 8h), rounded up
OMEGA_MEASURED = 7.5e-16
OMEGA_BOUND = min(10.0 * OMEGA_MEASURED, 1e-10)
DWDK_BOUND = 1e-10
ROOT_BOUND = 1e-10


class _Pool:
    def __init__(self, ctx):
        self.ctx, self.gp = ctx, {}

    def problem(self, name):
        if name not in self.gp:
            from eigensolver_amd import ShootProblem
            eq, mode, m, _ = M.all_cases()[name]
            self.gp[name] = ShootProblem(eq, mode, m, ctx=self.ctx)
        return self.gp[name]

    def close(self):
        for gp in self.gp.values():
            gp.close()


@pytest.fixture(scope="module")
def pool(es_ctx):
    p = _Pool(es_ctx)
    yield p
    p.close()


def _host(d):
    return {f: (t.cpu().numpy() if hasattr(t, "cpu") else t) for f, t in d.items()}


def _raw(pool, name, k, guess, n, count=None, max_iter=8, step_cap=1e300, max_shift=1e300, tol=1e-3, skip=(), prob=True,
         null_in=False):
    """es_shoot_newton through the raw ABI into buffers pre-filled with sentinels (at least one entry each); outputs named in
    `skip` are passed as NULL.  Returns (return code, dict of the six arrays)."""
    import torch
    from eigensolver_amd import _lib
    gp = pool.problem(name)
    na = max(n, 1)
    g = np.atleast_1d(np.asarray(guess, dtype=np.float64))
    dk, dg = gp._dev(np.broadcast_to(k, g.shape).copy()), gp._dev(g)
    dev = dk.device
    bufs = {f: torch.full((na,), SENT_D, dtype=torch.float64, device=dev) for f in ("w", "resid", "dwdk")}
    bufs["iters"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    bufs["flag"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    bufs["status"] = torch.full((na,), SENT_S, dtype=torch.uint8, device=dev)
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_shoot_newton(pool.ctx.handle, gp.handle if prob else None,
                                      *[None if null_in else _lib.ptr(t) for t in (dk, dg)], n,
                                      _lib.ptr(dc) if dc is not None else None, max_iter, step_cap, max_shift, tol,
                                      *[None if f in skip else _lib.ptr(bufs[f]) for f in OUT])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _untouched(out, a=0, fields=OUT):
    sent = dict(w=SENT_D, resid=SENT_D, dwdk=SENT_D, iters=SENT_I, flag=SENT_I, status=SENT_S)
    return all(np.all(out[f][a:] == sent[f]) for f in fields)


def _same(a, b, fields=OUT):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


# ---- against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.MODEL_CASES)
def test_newton_against_the_model(pool, name):
    """Offset guesses around the port's roots (four families, m = 3, N = 2, 3, 130 and each family's own N)."""
    from tests import root_slope_model as R
    gp = pool.problem(name)
    k, guess, root = N.offset_guesses(name)
    m = N.offset_model(name)
    g = _host(gp.newton(k, guess))
    assert g["w"].dtype == np.float64 and g["iters"].dtype == np.int32 and g["flag"].dtype == np.int32 and g["status"].dtype == np.uint8
    clear = [N.clear(s, w) for s, w in zip(m["steps"], m["w"])]
    mo, mi = R.jets(name, k, m["w"])
    slope_scale = 100.0 * np.abs(mo[1] - mi[1]) / np.maximum(np.abs(mo[0]), np.abs(mi[0]))
    dw = np.abs(g["w"] - m["w"]) / np.maximum(1.0, np.abs(m["w"]))
    ds = np.abs(g["dwdk"] - m["dwdk"]) / np.maximum(1.0, np.abs(m["dwdk"]))
    dr = np.abs(g["resid"] - m["resid"])
    rb = 2e-8 + slope_scale * np.abs(g["w"] - m["w"])
    for i in range(len(k)):
        print(f"{name} lane {i}: iters {g['iters'][i]} (model {m['iters'][i]}, {'clear' if clear[i] else 'not compared'}), "
              f"|w - w_model| / max(1, |w|) = {dw[i]:.2e} (bound {OMEGA_BOUND:.1e}), dwdk {ds[i]:.2e} (bound {DWDK_BOUND:.0e}), "
              f"resid {g['resid'][i]:.2e} % (model {m['resid'][i]:.2e}, bound on the difference {rb[i]:.1e})")
    assert [int(a) for a, c in zip(g["iters"], clear) if c] == [int(a) for a, c in zip(m["iters"], clear) if c]
    assert g["flag"].tolist() == m["flag"].tolist() == [1] * len(k) and g["status"].tolist() == [0] * len(k)
    assert dw.max() <= OMEGA_BOUND and ds.max() <= DWDK_BOUND and np.all(dr <= rb), (name, dw, ds, dr)
    # every lane ends on a root of the port in its row: its own, or (CR_kink, two roots beside a pole) the neighbour
    near = np.array([np.min(np.abs(root[k == k[i]] - g["w"][i])) for i in range(len(k))])
    assert np.max(near / np.maximum(1.0, np.abs(g["w"]))) <= ROOT_BOUND, (name, near)
    # the final evaluation alone, where the residual is not rounding noise
    g0, m0 = _host(gp.newton(k, guess, max_iter=0)), N.newton_model(name, k, guess, max_iter=0)
    assert np.array_equal(g0["w"], guess) and g0["iters"].tolist() == [0] * len(k)
    err0 = np.abs(g0["resid"] - m0["resid"])
    print(f"{name} max_iter = 0: resid {g0['resid'].min():.2e} .. {g0['resid'].max():.2e} %, worst difference to the model "
          f"{err0.max():.1e} (bound 2.0e-08)")
    assert err0.max() <= 2e-8 and g0["flag"].tolist() == m0["flag"].tolist()
    assert np.max(np.abs(g0["dwdk"] - m0["dwdk"]) / np.maximum(1.0, np.abs(m0["dwdk"]))) <= DWDK_BOUND


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_lane_counts(pool, n):
    """The guesses of a case tiled to n lanes (a lone lane, a wave short of one lane, a full wave, a second workgroup with
    one live lane): every copy equals the lane of the untiled call, bit for bit, whatever stops beside it."""
    name = "CF_flow_kink_N130"
    k, guess, _ = N.offset_guesses(name)
    rc, first = _raw(pool, name, k, guess, len(k))
    assert rc == 0 and first["flag"].tolist() == [1] * len(k) and len(set(first["iters"].tolist())) >= 2
    rc, out = _raw(pool, name, np.resize(k, n), np.resize(guess, n), n)
    assert rc == 0
    for i in range(n):
        assert all(np.array_equal(out[f][i], first[f][i % len(k)]) for f in OUT), i


# ---- max_iter = 0: bits -----------------------------------------------------------------------------------------------------
def _continuum_pair(name):
    """a pair the C port calls ES_PT_CONTINUUM on the case's 8 x 400 grid (the middle one)"""
    k, W = S.root_grid(name)
    D, _, st = N._port(name).eval_grid(k, W, w_mode=1, nthreads=4)
    idx = np.argwhere(np.asarray(st).reshape(len(k), len(W)) == N.ST_CONTINUUM)
    assert len(idx) > 0, name
    r, c = idx[len(idx) // 2]
    return float(k[r]), float(k[r] * W[c])


@pytest.mark.parametrize("name", ("SD_w15_sausage", "CR_kink", "CF_flow_kink_N130", "SFG_flow_kink_N3"))
def test_without_steps_is_root_slopes_and_eval_points(pool, name):
    """max_iter = 0 on the case's pairs, a leaky pair and (density slab: phase-speed bands; twisted cylinder: tracked signs) a
    continuum pair among them: w == guess, resid == 100 |outer - inner| / scale of root_slopes bit for bit, status that of
    eval_points, flag = 1 where the point is ES_PT_OK with resid < tol_percent."""
    gp = pool.problem(name)
    eq = M.all_cases()[name][0]
    k, w = (np.resize(a, 8).copy() for a in M.pairs(name))
    w[2] = (k[2] * eq.U_e if not M.is_cyl(eq) else 0.0) + k[2] * 1.05 * max(eq.c_e, eq.vA_e)    # m_e < 0
    want_continuum = name in ("SD_w15_sausage", "CR_kink")
    if want_continuum:
        k[5], w[5] = _continuum_pair(name)
    s = gp.root_slopes(k, w)
    o, i = s.outer[0].cpu().numpy(), s.inner[0].cpu().numpy()
    with np.errstate(all="ignore"):
        resid = 100.0 * np.abs(o - i) / np.maximum(np.abs(o), np.abs(i))
        cg = s.group_velocity.cpu().numpy()
    st = gp.eval_points(k, w)[1].cpu().numpy()
    assert st[2] == 1 and (not want_continuum or st[5] == 3) and np.all(np.delete(st, [2, 5]) == 0), st
    tol = float(np.median(resid[st == 0]))
    g = _host(gp.newton(k, w, max_iter=0, tol_percent=tol))
    print(f"{name}: status {g['status'].tolist()}, resid {g['resid']}")
    assert np.array_equal(g["w"], w) and g["iters"].tolist() == [0] * 8
    assert g["status"].tolist() == st.tolist()
    assert np.array_equal(g["resid"], resid, equal_nan=True) and np.isnan(g["resid"][2]) and np.isnan(g["dwdk"][2])
    assert np.isfinite(np.delete(g["resid"], 2)).all()
    assert np.array_equal(g["dwdk"], cg, equal_nan=True)
    assert g["flag"].tolist() == [1 if (a == 0 and r < tol) else 0 for a, r in zip(st, resid)] and 0 < g["flag"].sum() < 7


# ---- independence, count word, limits ---------------------------------------------------------------------------------------
def test_bad_guesses_change_nothing_beside_them(pool):
    name = "SFG_flow_kink_N130"
    eq = M.all_cases()[name][0]
    k, guess, _ = N.offset_guesses(name)
    k, guess = np.resize(k, 70), np.resize(guess, 70)
    rc, good = _raw(pool, name, k, guess, 70)
    assert rc == 0 and good["flag"].tolist() == [1] * 70
    bad = guess.copy()
    bad[3] = k[3] * eq.U_e + k[3] * 1.05 * max(eq.c_e, eq.vA_e)                   # leaky
    bad[40] = np.nan
    bad[66] = np.inf
    rc, got = _raw(pool, name, k, bad, 70)
    assert rc == 0 and got["status"][3] == 1 and got["status"][40] == 2 and got["status"][66] == 2
    for i in (3, 40, 66):
        assert got["flag"][i] == 0 and got["iters"][i] == 0 and np.isnan(got["resid"][i]) and np.isnan(got["dwdk"][i])
        assert np.array_equal(got["w"][i], bad[i], equal_nan=True)                 # w is reported whatever the flag
    keep = np.delete(np.arange(70), [3, 40, 66])
    assert all(np.array_equal(got[f][keep], good[f][keep]) for f in OUT)


def test_device_count(pool):
    name = "SFG_flow_kink_N130"
    k, guess, _ = N.offset_guesses(name)
    k, guess = np.resize(k, 130), np.resize(guess, 130)
    rc, full = _raw(pool, name, k, guess, 130)
    assert rc == 0 and np.all(full["flag"] == 1)
    for count, written in ((70, 70), (0, 0), (500, 130), (-3, 0)):
        rc, out = _raw(pool, name, k, guess, 130, count=count)
        assert rc == 0
        for f in OUT:
            assert np.array_equal(out[f][:written], full[f][:written]), (count, f)
        assert _untouched(out, written), count


def test_step_cap_and_max_shift(pool):
    name = "CF_flow_kink_N130"
    gp = pool.problem(name)
    k, guess, _ = N.offset_guesses(name)
    full = N.offset_model(name)
    lane = int(np.argmax([s[0] for s in full["steps"]]))
    cap = 0.25 * full["steps"][lane][0]                       # the first step of that lane exceeds it
    m = N.newton_model(name, k, guess, step_cap=cap)
    g = _host(gp.newton(k, guess, step_cap=cap))
    one = _host(gp.newton(k, guess, step_cap=cap, max_iter=1))
    print(f"step_cap {cap:.3e}: lane {lane} iters {g['iters'][lane]} (model {m['iters'][lane]}), first step "
          f"{abs(one['w'][lane] - guess[lane]):.17e}")
    assert abs(abs(one["w"][lane] - guess[lane]) - cap) <= 2e-16 * abs(guess[lane]) and one["iters"][lane] == 1
    assert m["iters"][lane] > full["iters"][lane] and N.clear(m["steps"][lane], m["w"][lane])
    assert g["iters"][lane] == m["iters"][lane]
    assert np.max(np.abs(g["w"] - m["w"]) / np.maximum(1.0, np.abs(m["w"]))) <= OMEGA_BOUND and g["flag"].tolist() == [1] * len(k)
    # max_shift clears the flag only
    free = _host(gp.newton(k, guess))
    shift = 0.5 * float(np.abs(free["w"] - guess).max())
    g = _host(gp.newton(k, guess, max_shift=shift))
    assert all(np.array_equal(g[f], free[f]) for f in ("w", "resid", "dwdk", "iters", "status"))
    assert g["flag"].tolist() == [1 if abs(a - b) <= shift else 0 for a, b in zip(free["w"], guess)] and 0 < g["flag"].sum() < len(k)


def test_dwdk_and_status_may_be_null_and_n_zero(pool):
    name = "SD_w15_sausage_N2"
    k, w = M.pairs(name)
    rc, full = _raw(pool, name, k, w, len(k), max_iter=2)
    assert rc == 0 and np.all(full["status"] == 0) and np.isfinite(full["dwdk"]).all()
    for f in ("dwdk", "status"):
        rc, out = _raw(pool, name, k, w, len(k), max_iter=2, skip=(f,))
        assert rc == 0 and _same(out, full, [h for h in OUT if h != f]) and _untouched(out, 0, (f,)), f
    rc, out = _raw(pool, name, k, w, 0, null_in=True, skip=OUT)                # n = 0 with NULL arrays: nothing touched
    assert rc == 0
    rc, out = _raw(pool, name, k, w, 0)
    assert rc == 0 and _untouched(out)


def test_argument_errors(pool):
    from eigensolver_amd import _lib
    name = "CF_flow_kink_N130"
    k, guess, _ = N.offset_guesses(name)
    n = len(k)
    for kwargs in (dict(n=-1), dict(null_in=True), dict(prob=False), dict(max_iter=-1), dict(step_cap=0.0),
                   dict(step_cap=-1.0), dict(step_cap=float("nan")), dict(max_shift=0.0), dict(max_shift=-2.0), dict(tol=0.0),
                   dict(tol=-1e-3), dict(skip=("w",)), dict(skip=("resid",)), dict(skip=("iters",)), dict(skip=("flag",))):
        rc, out = _raw(pool, name, k, guess, kwargs.pop("n", n), **kwargs)
        assert rc == 1 and _untouched(out), kwargs                                # ES_ERR_INVALID_ARG
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
    g = _host(pool.problem(name).newton(k, guess))                                # the context is still usable
    assert g["flag"].tolist() == [1] * n


# ---- densify and trace_branches ---------------------------------------------------------------------------------------------
def _check_branch(name, label, b, coarse):
    """one traced branch against the NumPy Hermite and the port's roots"""
    w, k, cg = coarse
    n = len(b["k"])
    pred, bound = N.hermite(k, w, cg, b["k"])
    roots = [N.port_root_near(name, float(a), float(c)) for a, c in zip(b["k"], b["w"])]
    assert all(r is not None for r in roots), (name, label)
    err = np.abs(b["w"] - np.array(roots)) / np.maximum(1.0, np.abs(b["w"]))
    dp = np.abs(b["predicted"] - pred) / np.maximum(1.0, np.abs(pred))
    print(f"{name} {label}: {n} points, iters <= {b['iters'].max()}, worst |w - port root| / max(1, |w|) = {err.max():.1e} "
          f"(bound {ROOT_BOUND:.0e}), |predicted - NumPy Hermite| = {dp.max():.1e} (bound 1e-12), worst |w - predicted| = "
          f"{np.abs(b['w'] - b['predicted']).max():.1e}")
    assert b["flag"].tolist() == [1] * n and b["status"].tolist() == [0] * n
    assert err.max() <= ROOT_BOUND and dp.max() <= 1e-12
    assert np.max(np.abs(b["max_shift"] - bound) / bound) <= 1e-9


@pytest.mark.parametrize("name", tuple(N.TRACE_CASES))
def test_trace_branches(pool, name):
    from eigensolver_amd import postprocess as pp
    gp = pool.problem(name)
    curves = N.coarse_curves(name)
    k_fine = N.cut_in(S.ROOT_K)
    t = gp.trace_branches(curves, k_fine)
    single = sorted(lab for lab, c in curves.items() if len(c[1]) < 2)
    assert sorted(t.skipped) == single and sorted(t.branches) == sorted(set(curves) - set(single))
    assert set(N.TRACE_CASES[name]) <= set(t.branches)
    for label in N.TRACE_CASES[name]:
        b = _host(t.branches[label])
        ks = curves[label][1]
        assert np.array_equal(b["k"], k_fine[(k_fine >= ks[0]) & (k_fine <= ks[-1])]) and len(b["k"]) == N.CUT * (len(ks) - 1) + 1
        _check_branch(name, label, b, curves[label])
    tc = pp.traced_curves(t)
    for label in N.TRACE_CASES[name]:
        w, k, cg = tc[label]
        b = _host(t.branches[label])
        assert np.array_equal(k, b["k"]) and np.array_equal(w, b["w"]) and np.array_equal(cg, b["dwdk"])
        f = pp.hermite_branch(k, w, cg)                       # the layout hermite_branch, fit_branch and pickle_layout take
        assert np.array_equal(f(k), w)
        assert len(pp.pickle_layout({"kink": tc[label][:2]})) == 2
    if len(tc[N.TRACE_CASES[name][0]][1]) > 6:
        pp.fit_branch(tc[N.TRACE_CASES[name][0]][1], tc[N.TRACE_CASES[name][0]][0])


def test_densify_is_one_branch_of_trace_branches(pool):
    """densify forms the slopes itself (root_slopes) where trace_branches takes them from the curves; with cg given the two
    are the same launch on the same guesses."""
    name, label = "SFG_flow_kink_N130", (0, 1)
    gp = pool.problem(name)
    w, k, cg = N.coarse_curves(name)[label]
    kf = N.cut_in(k)
    d = _host(gp.densify(k, w, kf))
    _check_branch(name, label, d, (w, k, gp.root_slopes(k, w).group_velocity.cpu().numpy()))
    d2 = _host(gp.densify(k, w, kf, cg=cg))
    t = _host(gp.trace_branches({label: (w, k, cg)}, kf, check_signature=False).branches[label])
    assert all(np.array_equal(d2[f], t[f]) for f in ("k", "w", "resid", "dwdk", "iters", "flag", "status", "predicted", "max_shift"))
    # a max_shift of the caller's goes to the Newton call as it is
    d3 = _host(gp.densify(k, w, kf, cg=cg, max_shift=1e-5))
    assert d3["flag"].tolist() == [1 if p <= 1e-5 else 0 for p in np.abs(d3["w"] - d3["predicted"])] and 0 < d3["flag"].sum() < len(kf)
    assert np.all(d3["max_shift"] == 1e-5)
    with pytest.raises(ValueError):
        gp.densify(k[:1], w[:1], kf)


def test_two_roots_per_row_are_skipped_and_the_hand_split_traces(pool):
    """CR_kink: every root carries (1, 0) and the rows k >= 2.4 hold two of them (roots beside a pole of the exterior term):
    trace_branches does not guess; the two curves split by hand, lower and upper omega, trace with densify."""
    name = N.SPLIT_CASE
    gp = pool.problem(name)
    t = gp.trace_branches(N.coarse_curves(name), N.cut_in(S.ROOT_K))
    assert t.skipped == [(1, 0)] and t.branches == {}
    for which, (w, k, cg) in N.split_curves().items():
        d = _host(gp.densify(k, w, N.cut_in(k), cg=cg))
        _check_branch(name, which, d, (w, k, cg))
        sig = gp.mode_signature(d["k"], d["w"])
        assert set(zip(sig.nodes_value.cpu().tolist(), sig.nodes_flux.cpu().tolist())) == {N.SPLIT_LABEL}


def test_a_mislabelled_branch_is_flagged(pool):
    name = "CF_flow_kink_N130"
    gp = pool.problem(name)
    curves = dict(N.coarse_curves(name))
    curves[(5, 5)] = curves.pop((0, 0))
    t = gp.trace_branches(curves, N.cut_in(S.ROOT_K))
    wrong, right = _host(t.branches[(5, 5)]), _host(t.branches[(1, 1)])
    assert wrong["flag"].tolist() == [0] * len(wrong["k"]) and len(wrong["k"]) == 9
    assert right["flag"].tolist() == [1] * len(right["k"])
    free = _host(gp.trace_branches(curves, N.cut_in(S.ROOT_K), check_signature=False).branches[(5, 5)])
    assert free["flag"].tolist() == [1] * 9 and np.array_equal(free["w"], wrong["w"])
    from eigensolver_amd import postprocess as pp
    assert len(pp.traced_curves(t)[(5, 5)][0]) == 0 and len(pp.traced_curves(t)[(1, 1)][0]) == len(right["k"])


def test_tracing_has_no_host_synchronisation(pool):
    """A context on its own stream, that stream held busy for about 0.2 s: densify (device tensors) and trace_branches (host
    curves) return while it is still busy, and the results are those of the idle stream."""
    import torch
    from eigensolver_amd import ShootProblem, _lib
    name, label = "SFG_flow_kink_N130", (0, 1)
    eq, mode, m, _ = M.all_cases()[name]
    curves = N.coarse_curves(name)
    w, k, cg = curves[label]
    kf = N.cut_in(S.ROOT_K)
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream)
    gp = ShootProblem(eq, mode, m, ctx=ctx)
    with torch.cuda.stream(stream):
        dk, dw, dkf = gp._dev(k), gp._dev(w), gp._dev(N.cut_in(k))
    ref_d = gp.densify(dk, dw, dkf)                           # warm-up, and the reference
    ref_t = gp.trace_branches(curves, kf)
    stream.synchronize()                                      # .cpu() below waits for the current stream, not this one
    ref_d, ref_t = _host(ref_d), {lab: _host(b) for lab, b in ref_t.branches.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 1 << 22
    with torch.cuda.stream(stream):
        e0.record(stream)
        torch.cuda._sleep(cycles)
        e1.record(stream)
    stream.synchronize()
    cycles = int(cycles * 200.0 / max(e0.elapsed_time(e1), 1e-3))
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
    d = gp.densify(dk, dw, dkf)
    t = gp.trace_branches(curves, kf)
    busy = not stream.query()
    stream.synchronize()
    assert busy, "the stream finished before the calls returned: a host synchronisation inside them"
    d = _host(d)
    assert all(np.array_equal(d[f], ref_d[f]) for f in ref_d)
    for lab, b in t.branches.items():
        b = _host(b)
        assert all(np.array_equal(b[f], ref_t[lab][f]) for f in b), lab
    gp.close()
    ctx.close()


# ---- the complex densify through the shared helper --------------------------------------------------------------------------
def test_complex_densify_still_follows_its_branch(pool):
    """SlabComplexFlow.densify now takes its prediction and bound from shooting.hermite_guess: the case of
    tests/test_complex_slopes_gpu.py (width 0.9, N = 3, kink "sfx", coarse rows 0.5 apart) gives what it gave, and predicted
    and max_shift are the NumPy Hermite of the complex branch."""
    from eigensolver_amd import SlabComplexFlow
    from eigensolver_amd import postprocess as pp
    from tests import complex_slope_model as C
    o3 = C.slab(0.9, "kink", "sfx", 3)
    kf = 0.5 + 0.125 * np.arange(21)
    branch, kk, ww = [], 0.5, C.oracle_root(o3, 0.5, C.N3_UPPER)
    for x in kf:
        outer, inner, _ = C.jets(o3, kk, ww)
        ww = C.oracle_root(o3, x, ww + C.dwdk(outer, inner)[0] * (x - kk))
        kk = x
        branch.append(ww)
    branch = np.array(branch)
    s = SlabComplexFlow(width=0.9, variant="sfx", ctx=pool.ctx, n_nodes=3)
    try:
        d = _host(s.densify("kink", kf[::4], branch[::4], kf))
        slopes = s.group_velocity("kink", dict(k=kf[::4], w=branch[::4])).cpu().numpy()
    finally:
        s.close()
    err, pred = np.abs(d["w"] - branch), np.abs(d["predicted"] - d["w"])
    print(f"complex densify: worst |w - oracle root| = {err.max():.2e} (bound 1.0e-10), worst |predicted - w| = {pred.max():.2e} "
          f"(bound 1.0e-3)")
    assert d["flag"].tolist() == [1] * 21 and np.array_equal(d["k"], kf) and err.max() <= 1e-10 and pred.max() <= 1e-3
    want = pp.hermite_branch_complex(kf[::4], branch[::4], slopes)(kf)
    assert np.max(np.abs(d["predicted"] - want)) <= 1e-12
    h = 0.5
    dw = np.diff(branch[::4])
    defect = np.maximum(np.abs(dw - h * slopes[:-1]), np.abs(dw - h * slopes[1:]))
    bound = np.maximum(4.0 * defect, 1e-8 * np.maximum(1.0, np.abs(branch[::4][:-1])))
    j = np.clip(np.searchsorted(kf[::4], kf, side="right") - 1, 0, 4)
    assert np.max(np.abs(d["max_shift"] - bound[j]) / bound[j]) <= 1e-9

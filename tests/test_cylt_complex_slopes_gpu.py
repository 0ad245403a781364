"""es_cylt_complex_root_slopes and es_cylt_complex_newton (include/eigensolver_amd.h section 18) on the GPU, with the Python
layer on top (RotatingCylinderComplex.root_slopes / group_velocity / newton / densify, postprocess.most_unstable).

Yardsticks (tests/cylt_complex_slope_model.py, pinned on the CPU by tests/test_cylt_complex_slope_model.py), with the bounds
tests/test_cyl_complex_slopes_gpu.py uses for the same comparisons:
  value    rows 0 of outer and inner against es_cylt_complex_eval_points(parts): 1e-12 of max(|outer|, |inner|), statuses equal.
  jets     the NumPy forward-mode restatement of the value model: every row of outer and inner within 1e-10 of
           max(|outer_x|, |inner_x|) of its row.
  Newton   the iteration rule restated on the model: the same number of steps, |w - w_model| <= 1e-12 max(1, |w|).
The five problems of tests/test_cylt_complex_gpu.py (both values of c1_power, accept_norm 0 and 1, the rotational sausage
condition, ES_AXIS_ROTATION_KINK).  Node counts: N = 3 (two steps), 129 (128 steps: exactly one LDS chunk), 130 (a chunk of one
step on top), 300 (three chunks).  Pair counts 1, 63, 64, 65, 257: one lane, a ragged and a full workgroup, one lane in a second,
five workgroups; a different k in every lane.  `pytest -s` prints every measured figure next to its bound.
"""
import functools
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cylt_complex_slope_model as C  # noqa: E402
from tests.complex_slope_model import dwdk  # noqa: E402
from tests.cylt_complex_model import JET  # noqa: E402

SENT_D, SENT_S, SENT_I = -7.25e77, 0xEE, -77
NODES = (3, 129, 130, 300)
COUNTS = (1, 63, 64, 65, 257)
INVALID, UNSUPPORTED = 1, 5


class _Pool:
    """one RotatingCylinderComplex per (problem, N) on the session's context; names "root A" ... are the equilibria of
    cylt_complex_model.root_cases (accept_norm 0), the others those of C.problems"""
    def __init__(self, ctx):
        self.ctx, self.s = ctx, {}

    def solver(self, name, N=C.N0):
        if (name, N) not in self.s:
            from eigensolver_amd import RotatingCylinderComplex, ShootProblem
            if name.startswith("root "):
                eq, m, _, _, _, _ = C.root_cases(N)[name[5:]]
                mode, an = "kink", 0
            else:
                eq, mode, m, an = C.problems(N)[name]
            c = RotatingCylinderComplex(eq, ctx=self.ctx)
            if an:                                    # the cached problem of (mode, m) carries accept_norm
                key = (mode, (1 if mode == "kink" else 0) if m is None else int(m))
                c._problems[key] = ShootProblem(eq, mode, m=key[1], ctx=self.ctx, accept_norm=1)
            self.s[(name, N)] = (c, mode, m)
        return self.s[(name, N)]

    def close(self):
        for s, _, _ in self.s.values():
            s.close()


@pytest.fixture(scope="module")
def pool(es_ctx):
    p = _Pool(es_ctx)
    yield p
    p.close()


def _np(s):
    return dict(outer=s.outer.cpu().numpy(), inner=s.inner.cpu().numpy(), status=s.status.cpu().numpy())


def _host(d):
    return {f: t.cpu().numpy() for f, t in d.items()}


@functools.lru_cache(maxsize=None)
def _sample(name, N):
    """257 pairs, a different k in every lane: Re omega = k W, Im omega = +- k g with W and g in the problem's windows, both
    signs (some of them leaky), a good pair first, and the leaky pair put in the middle of the first three consecutive good
    ones, at index `at`.  With the model's jets at them, computed once per session: (k, w, outer, inner, status, at)."""
    rng = np.random.default_rng(700 + N)
    W, g = C.WINDOW[name]
    k = rng.permutation(np.linspace(0.5, 2.0, 257))
    w = k * rng.uniform(W[0], W[1], 257) + 1j * k * rng.uniform(g[0], g[1], 257) * rng.choice([-1.0, 1.0], 257)
    M = C.model(name, N)
    mo, mi, mst = C.jets(M, k, w)
    first = int(np.argmax(mst == 0))                  # the launch of one pair holds a good one
    for a in (k, w, mst):
        a[0], a[first] = a[first], a[0]
    for a in (mo, mi):
        a[:, [0, first]] = a[:, [first, 0]]
    at = next(i for i in range(1, 60) if mst[i - 1] == 0 and mst[i] == 0 and mst[i + 1] == 0)
    k[at], w[at] = C.LEAKY
    mo[:, at:at + 1], mi[:, at:at + 1], mst[at:at + 1] = C.jets(M, k[at], w[at:at + 1])
    for a in (k, w, mo, mi, mst):
        a.setflags(write=False)
    return k, w, mo, mi, mst, at


# ---- value and jets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NODES)
@pytest.mark.parametrize("name", C.NAMES)
def test_value_and_jets(pool, name, N):
    s, mode, m = pool.solver(name, N)
    k, w, mo, mi, mst, at = _sample(name, N)
    ok = mst == 0
    assert mst[at] == 1 and ok[at - 1] and ok[at + 1] and ok[0] and ok.sum() > 120, ok.sum()
    worst_v, worst_j, full, bitwise = 0.0, [0.0, 0.0, 0.0], None, True
    for n in COUNTS[::-1]:
        kn, wn = k[:n].copy(), w[:n].copy()
        g = _np(s.root_slopes(mode, kn, wn, m=m))
        D, st, rel, outer, inner = (t.cpu().numpy() for t in s.eval_points(mode, kn, wn, m=m, parts=True))
        assert g["outer"].dtype == np.complex128 and g["outer"].shape == (3, n) and g["status"].shape == (n,)
        assert g["status"].tolist() == st.tolist() == mst[:n].tolist(), (name, N, n)
        o = ok[:n]
        assert np.isnan(g["outer"][:, ~o].real).all() and np.isnan(g["outer"][:, ~o].imag).all()
        assert np.isnan(g["inner"][:, ~o].real).all() and np.isnan(g["inner"][:, ~o].imag).all()
        sc = np.maximum(np.abs(outer[o]), np.abs(inner[o]))
        worst_v = max(worst_v, float(np.max(np.abs(g["outer"][0][o] - outer[o]) / sc)),
                      float(np.max(np.abs(g["inner"][0][o] - inner[o]) / sc)))
        bitwise = bitwise and g["outer"][0][o].tobytes() == outer[o].tobytes() and g["inner"][0][o].tobytes() == inner[o].tobytes()
        for c in range(3):
            scm = np.maximum(np.abs(mo[c][:n][o]), np.abs(mi[c][:n][o]))
            worst_j[c] = max(worst_j[c], float(np.max(np.abs(g["outer"][c][o] - mo[c][:n][o]) / scm)),
                             float(np.max(np.abs(g["inner"][c][o] - mi[c][:n][o]) / scm)))
        if full is None:
            full = g
        else:                                        # a pair does not depend on how many others the launch holds
            assert np.array_equal(g["outer"], full["outer"][:, :n], equal_nan=True), n
            assert np.array_equal(g["inner"], full["inner"][:, :n], equal_nan=True), n
    print(f"{name} N {N}: rows 0 against eval_points {worst_v:.2e} of max(|outer|, |inner|) (bound 1.0e-12; bit for bit: "
          f"{bitwise}); against the model value {worst_j[0]:.2e}, d/dw {worst_j[1]:.2e}, d/dk {worst_j[2]:.2e} of "
          f"max(|outer_x|, |inner_x|) (bound 1.0e-10); {int(ok.sum())} OK pairs of 257")
    assert worst_v <= 1e-12
    assert max(worst_j) <= 1e-10, worst_j
    # the leaky pair's neighbours are bit for bit what they are without it
    k2, w2 = k[:64].copy(), w[:64].copy()
    k2[at], w2[at] = k[at + 1], w[at + 1]
    h = _np(s.root_slopes(mode, k2, w2, m=m))
    keep = np.arange(64) != at
    assert h["status"][at] == 0 and np.array_equal(h["outer"][:, at], full["outer"][:, at + 1])
    assert np.array_equal(h["outer"][:, keep], full["outer"][:, :64][:, keep], equal_nan=True)
    assert np.array_equal(h["inner"][:, keep], full["inner"][:, :64][:, keep], equal_nan=True)


# ---- the real axis and the conjugate ----------------------------------------------------------------------------------------
def test_real_axis_slope_is_the_real_group_speed(pool):
    """At the nine real roots of CR_kink: Im d omega / dk of the complex path vanishes (1e-13), the real part is
    ShootProblem.group_velocity within 10 x the difference of the two NumPy models, and d omega / dk at conj omega (the same
    point, written with -0.0) is the conjugate of that at omega within 1e-13."""
    from eigensolver_amd import RotatingCylinderComplex, ShootProblem
    eq, mode, m, k, w, _, _ = C.real_axis_case()
    assert len(k) == 9
    bound = 10.0 * C.REAL_AXIS_MEASURED
    s = RotatingCylinderComplex(eq, ctx=pool.ctx)
    gp = ShootProblem(eq, mode, m=m, ctx=pool.ctx)
    try:
        cx = s.group_velocity(mode, dict(k=k, w=w + 0j), m=m).cpu().numpy()
        cc = s.group_velocity(mode, dict(k=k, w=np.conj(w + 0j)), m=m).cpu().numpy()
        cg = gp.group_velocity(dict(k=k, w=w)).cpu().numpy()
    finally:
        s.close()
        gp.close()
    sc = np.maximum(1.0, np.abs(cg))
    ere, eim, ecj = np.abs(cx.real - cg) / sc, np.abs(cx.imag), np.abs(cc - np.conj(cx))
    print(f"{C.REAL_AXIS_CASE}: {len(k)} real roots, worst |Re d omega / dk - c_g| / max(1, |c_g|) = {ere.max():.2e} (bound "
          f"{bound:.1e}), worst |Im d omega / dk| = {eim.max():.2e} (bound 1.0e-13), worst |d omega / dk (conj omega) - conj| = "
          f"{ecj.max():.2e} (bound 1.0e-13)")
    assert eim.max() <= 1e-13
    assert ecj.max() <= 1e-13
    assert ere.max() <= bound


@pytest.mark.parametrize("name", C.NAMES)
def test_conjugate_symmetry(pool, name):
    s, mode, m = pool.solver(name)
    k, w, _, _, mst, _ = _sample(name, C.N0)
    ok = mst == 0
    a = s.root_slopes(mode, k[ok], w[ok], m=m).group_velocity.cpu().numpy()
    b = s.root_slopes(mode, k[ok], np.conj(w[ok]), m=m).group_velocity.cpu().numpy()
    err = np.abs(b - np.conj(a)) / np.maximum(1.0, np.abs(a))
    print(f"{name}: worst |d omega / dk (conj omega) - conj d omega / dk (omega)| / max(1, |.|) = {err.max():.2e} over "
          f"{int(ok.sum())} pairs (bound 1.0e-13)")
    assert np.isfinite(a).all() and err.max() <= 1e-13


# ---- zero-twist limit -------------------------------------------------------------------------------------------------------
def test_zero_twist_limit(pool):
    """The uniform jet through the twisted coefficient set (v_phi = B_phi = 0; the TwistedJet of tests/test_cylt_complex_gpu.py)
    against CylinderComplex.root_slopes on the plain CylinderFlow: the same 65 pairs, all three rows of outer and inner within
    1e-10 of max(|outer_x|, |inner_x|) of the row."""
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, equilibrium as q

    class TwistedJet(q.CylinderFlow):
        twisted = True

    ct = RotatingCylinderComplex(TwistedJet(**JET, n_nodes=130), ctx=pool.ctx)
    c0 = CylinderComplex(q.CylinderFlow(**JET, n_nodes=130), ctx=pool.ctx)
    try:
        rng = np.random.default_rng(5)
        k = rng.uniform(1.0, 2.5, 65)
        w = k * rng.uniform(0.9, 1.45, 65) + 1j * k * rng.uniform(0.05, 0.4, 65) * rng.choice([-1.0, 1.0], 65)
        t, u = _np(ct.root_slopes("kink", k, w)), _np(c0.root_slopes("kink", k, w))
    finally:
        ct.close()
        c0.close()
    assert np.array_equal(t["status"], u["status"])
    ok = u["status"] == 0
    assert ok.sum() > 40
    worst = [0.0, 0.0, 0.0]
    for c in range(3):
        sc = np.maximum(np.abs(u["outer"][c][ok]), np.abs(u["inner"][c][ok]))
        worst[c] = max(float(np.max(np.abs(t["outer"][c][ok] - u["outer"][c][ok]) / sc)),
                       float(np.max(np.abs(t["inner"][c][ok] - u["inner"][c][ok]) / sc)))
    print(f"zero twist: max |twisted - untwisted| / row scale = value {worst[0]:.2e}, d/dw {worst[1]:.2e}, d/dk {worst[2]:.2e} on "
          f"{int(ok.sum())} of 65 pairs (bound 1.0e-10)")
    assert max(worst) <= 1e-10, worst


# ---- Newton -----------------------------------------------------------------------------------------------------------------
def _check_newton(g, models, what):
    for i, mm in enumerate(models):
        dw = abs(g["w"][i] - mm["w"]) / max(1.0, abs(mm["w"]))
        print(f"{what} lane {i}: iters {g['iters'][i]} (model {mm['iters']}), |w - w_model| / max(1, |w|) = {dw:.2e} "
              f"(bound 1.0e-12), flag {g['flag'][i]} (model {mm['flag']}), resid {g['resid'][i]:.1e} %")
        assert g["iters"][i] == mm["iters"] and dw <= 1e-12 and g["flag"][i] == mm["flag"], (what, i, g["w"][i], mm)
        if mm["status"] == 0:
            assert abs(g["dwdk"][i] - mm["dwdk"]) <= 1e-9 * max(1.0, abs(mm["dwdk"])), (what, i)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_newton_steps_and_roots(pool, name):
    s, mode, m = pool.solver("root " + name)
    M = C.root_model(name)
    rows = C.case_roots(name)
    k = np.repeat([r[0] for r in rows], 2)
    roots = np.repeat([r[1] for r in rows], 2)
    starts = roots + np.tile([1.0, -1.0], len(rows)) * C.NEWTON_OFFSET
    g = _host(s.newton(mode, k, starts, m=m))
    _check_newton(g, [C.newton_model(M, kk, z) for kk, z in zip(k, starts)], f"{name} roots +- 1e-3 (1 + i)")
    assert g["flag"].tolist() == [1] * len(k) and np.all(g["iters"] == C.NEWTON_STEPS)
    assert np.all(np.abs(g["w"] - roots) <= 1e-12 * np.maximum(1.0, np.abs(roots)))
    assert g["w"].dtype == np.complex128 and g["iters"].dtype == np.int32


def test_newton_guards(pool):
    s, mode, m = pool.solver("root A")
    M = C.root_model("A")
    k0, root = C.case_roots("A")[0]
    guess = root + C.NEWTON_OFFSET
    # max_iter = 0 reproduces root_slopes: the guess with its residual and slope
    k = k0 + 1e-3 * np.arange(65)
    guesses = guess + 0.002 * np.arange(65) * (1 - 0.5j)
    k[40], guesses[40] = C.LEAKY
    g = _host(s.newton(mode, k, guesses, max_iter=0, tol_percent=1.0, m=m))
    r = s.root_slopes(mode, k, guesses, m=m)
    rs, gv = _np(r), r.group_velocity.cpu().numpy()
    rel = C.rel_of(M, rs["outer"], rs["inner"])
    assert np.array_equal(g["w"], guesses) and g["iters"].tolist() == [0] * 65
    good = np.arange(65) != 40
    # the kernel's -D_k / D_w against the same quotient formed by the caller: two roundings of one complex division
    assert np.max(np.abs(g["dwdk"][good] - gv[good]) / np.abs(gv[good])) <= 1e-14
    assert rs["status"][40] == 1 and np.isnan(g["resid"][40]) and g["flag"][40] == 0 and np.isnan(g["dwdk"][40].real)
    assert np.max(np.abs(g["resid"][good] - rel[good]) / rel[good]) <= 1e-12
    assert g["flag"][good].tolist() == [1 if x < 1.0 else 0 for x in g["resid"][good]] and 0 < g["flag"].sum() < 64
    # step_cap: the first step is exactly that long
    g = _host(s.newton(mode, k0, [guess], max_iter=1, step_cap=1e-4, m=m))
    mm = C.newton_model(M, k0, guess, max_iter=1, step_cap=1e-4)
    print(f"capped step: |w - guess| = {abs(g['w'][0] - guess):.17e}")
    assert g["iters"][0] == 1 and abs(abs(g["w"][0] - guess) - 1e-4) <= 1e-15 and abs(g["w"][0] - mm["w"]) <= 1e-12
    assert g["flag"][0] == mm["flag"]
    # max_shift smaller than the distance travelled: flag 0 as the model says, w still reported
    g = _host(s.newton(mode, k0, [guess, guess], max_shift=1e-4, m=m))
    mm = C.newton_model(M, k0, guess, max_shift=1e-4)
    assert g["flag"].tolist() == [mm["flag"]] * 2 == [0, 0] and abs(g["w"][0] - root) <= 1e-12 and g["resid"][0] < 1e-6
    g = _host(s.newton(mode, k0, [guess], max_shift=1e-2, tol_percent=1e-6, m=m))
    mm = C.newton_model(M, k0, guess, max_shift=1e-2, tol_percent=1e-6)
    assert g["flag"].tolist() == [mm["flag"]] == [1] and abs(g["w"][0] - root) <= 1e-12


def test_newton_leaky_guess_among_good_ones(pool):
    """Lanes of one workgroup that stop after different numbers of steps, a leaky guess among them: flag 0, no step, NaN
    resid and slope for it, and the others bit for bit what they are without it."""
    s, mode, m = pool.solver("root A")
    M = C.root_model("A")
    k0, root = C.case_roots("A")[0]
    starts = [root + off for off in (0, 1e-9, 1e-6 * (1 - 1j), 1e-4j, 1e-3, 5e-3 * (1 - 1j))]
    models = [C.newton_model(M, k0, z) for z in starts]
    assert len({mm["iters"] for mm in models}) >= 3 and all(mm["flag"] == 1 for mm in models)
    g = _host(s.newton(mode, k0, starts, m=m))
    _check_newton(g, models, "mixed step counts")
    kl, leaky = C.LEAKY
    kk = np.full(7, k0)
    kk[3] = kl
    h = _host(s.newton(mode, kk, starts[:3] + [leaky] + starts[3:], m=m))
    assert h["flag"][3] == 0 and h["iters"][3] == 0 and h["w"][3] == leaky and np.isnan(h["resid"][3])
    assert np.isnan(h["dwdk"][3].real) and np.isnan(h["dwdk"][3].imag)
    for f in ("w", "resid", "iters", "flag", "dwdk"):
        assert np.array_equal(np.delete(h[f], 3), g[f]), f


# ---- the raw ABI: count, NULL outputs, argument errors ----------------------------------------------------------------------
SLOPE_OUT = ("outer", "inner", "status")
NEWTON_OUT = ("w_re", "w_im", "resid", "dwdk", "iters", "flag")


def _dev(pool, a, dtype):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype), device=f"cuda:{pool.ctx.device}")


def _inputs(pool, k, w):
    w = np.asarray(w, dtype=complex)
    return _dev(pool, np.broadcast_to(k, w.shape), np.float64), _dev(pool, w.real, np.float64), _dev(pool, w.imag, np.float64)


def _raw_slopes(pool, handle, k, w, n, count=None, skip=(), null_in=()):
    """es_cylt_complex_root_slopes into buffers pre-filled with sentinels ([3, n] complex and [n], at least one entry); outputs
    named in `skip` and the inputs whose index is in `null_in` are passed as NULL.  Returns (return code, the three arrays)."""
    import torch
    from eigensolver_amd import _lib
    na = max(n, 1)
    ins = _inputs(pool, k, w)
    dev = ins[0].device
    bufs = dict(outer=torch.full((3, na), SENT_D, dtype=torch.complex128, device=dev),
                inner=torch.full((3, na), SENT_D, dtype=torch.complex128, device=dev),
                status=torch.full((na,), SENT_S, dtype=torch.uint8, device=dev))
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_cylt_complex_root_slopes(pool.ctx.handle, handle,
                                                  *[None if j in null_in else _lib.ptr(t) for j, t in enumerate(ins)], n,
                                                  _lib.ptr(dc) if dc is not None else None,
                                                  *[None if f in skip else _lib.ptr(bufs[f]) for f in SLOPE_OUT])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _raw_newton(pool, handle, k, guess, n, count=None, max_iter=8, step_cap=1e300, max_shift=1e300, tol=4.0, skip=(),
                null_in=()):
    import torch
    from eigensolver_amd import _lib
    na = max(n, 1)
    ins = _inputs(pool, k, guess)
    dev = ins[0].device
    bufs = {f: torch.full((na,), SENT_D, dtype=torch.float64, device=dev) for f in ("w_re", "w_im", "resid")}
    bufs["dwdk"] = torch.full((na,), SENT_D, dtype=torch.complex128, device=dev)
    bufs["iters"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    bufs["flag"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_cylt_complex_newton(pool.ctx.handle, handle,
                                             *[None if j in null_in else _lib.ptr(t) for j, t in enumerate(ins)], n,
                                             _lib.ptr(dc) if dc is not None else None, max_iter, step_cap, max_shift, tol,
                                             *[None if f in skip else _lib.ptr(bufs[f]) for f in NEWTON_OUT])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _untouched_s(o):
    return np.all(o["outer"] == SENT_D) and np.all(o["inner"] == SENT_D) and np.all(o["status"] == SENT_S)


def _untouched_n(o):
    return all(np.all(o[f] == (SENT_I if f in ("iters", "flag") else SENT_D)) for f in NEWTON_OUT)


def _same(a, b, fields):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


def test_device_count(pool):
    """count as a device word: 0, 1, 64, 65, n + 5 and -2 of n = 70 pairs (two workgroups); entries past min(count, n) keep
    the sentinel, the others are what a call without count writes."""
    s, mode, m = pool.solver("root A", 129)
    h = s.problem(mode, m).handle
    n = 70
    k0, root = C.case_roots("A", 129)[0]
    w = root + 1e-3 + 2e-4 * np.arange(n) * (1 + 1j)
    k = k0 + 1e-4 * np.arange(n)
    rc, full = _raw_slopes(pool, h, k, w, n)
    rcn, nfull = _raw_newton(pool, h, k, w, n)
    assert rc == 0 and rcn == 0 and np.all(full["status"] == 0) and np.all(nfull["flag"] == 1)
    assert np.all(nfull["iters"] >= 2) and np.isfinite(nfull["resid"]).all() and np.isfinite(full["outer"]).all()
    for count, written in ((0, 0), (1, 1), (64, 64), (65, 65), (n + 5, n), (-2, 0)):
        rc, out = _raw_slopes(pool, h, k, w, n, count=count)
        assert rc == 0
        for f in SLOPE_OUT:
            assert np.array_equal(out[f][..., :written], full[f][..., :written]), (count, f)     # rows stay n apart
            assert np.all(out[f][..., written:] == (SENT_S if f == "status" else SENT_D)), (count, f)
        rc, out = _raw_newton(pool, h, k, w, n, count=count)
        assert rc == 0
        for f in NEWTON_OUT:
            assert np.array_equal(out[f][:written], nfull[f][:written]), (count, f)
            assert np.all(out[f][written:] == (SENT_I if f in ("iters", "flag") else SENT_D)), (count, f)


def test_each_output_may_be_null_and_n_zero(pool):
    s, mode, m = pool.solver("A", 3)
    h = s.problem(mode, m).handle
    k, w = np.array([p[0] for p in C.NON_ROOT["A"]]), np.array([p[1] for p in C.NON_ROOT["A"]])
    n = len(w)
    rc, full = _raw_slopes(pool, h, k, w, n)
    assert rc == 0 and np.all(full["status"] == 0)
    for f in SLOPE_OUT:
        rc, out = _raw_slopes(pool, h, k, w, n, skip=(f,))
        assert rc == 0 and _same(out, full, [x for x in SLOPE_OUT if x != f]), f
        assert np.all(out[f] == (SENT_S if f == "status" else SENT_D)), f
    rc, _ = _raw_slopes(pool, h, k, w, n, skip=SLOPE_OUT)
    assert rc == 0
    rc, out = _raw_slopes(pool, h, k, w, 0, null_in=(0, 1, 2))                         # n = 0 with NULL arrays: nothing touched
    assert rc == 0 and _untouched_s(out)
    rcn, nfull = _raw_newton(pool, h, k, w, n)
    rc, out = _raw_newton(pool, h, k, w, n, skip=("dwdk",))                            # the one optional output of the Newton call
    assert rcn == 0 and rc == 0 and _same(out, nfull, [f for f in NEWTON_OUT if f != "dwdk"]) and np.all(out["dwdk"] == SENT_D)
    rc, out = _raw_newton(pool, h, k, w, 0, null_in=(0, 1, 2), skip=NEWTON_OUT)
    assert rc == 0


def test_argument_errors(pool):
    from eigensolver_amd import ShootProblem, _lib
    from eigensolver_amd import equilibrium as q
    s, mode, m = pool.solver("A", 3)
    h = s.problem(mode, m).handle
    k, w = np.array([p[0] for p in C.NON_ROOT["A"]]), np.array([p[1] for p in C.NON_ROOT["A"]])
    for kwargs in (dict(n=-1), dict(n=2, null_in=(0,)), dict(n=2, null_in=(1,)), dict(n=2, null_in=(2,)), dict(n=2, handle=None)):
        n, hh = kwargs.pop("n"), kwargs.pop("handle", h)
        rc, out = _raw_slopes(pool, hh, k, w, n, **kwargs)
        assert rc == INVALID and _untouched_s(out), kwargs
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
        rc, out = _raw_newton(pool, hh, k, w, n, **kwargs)
        assert rc == INVALID and _untouched_n(out), kwargs
    nan = float("nan")
    for kwargs in (dict(max_iter=-1), dict(step_cap=0.0), dict(step_cap=-1.0), dict(step_cap=nan), dict(max_shift=0.0),
                   dict(max_shift=-2.0), dict(max_shift=nan), dict(tol=0.0), dict(tol=-4.0), dict(tol=nan), dict(skip=("w_re",)),
                   dict(skip=("w_im",)), dict(skip=("resid",)), dict(skip=("iters",)), dict(skip=("flag",))):
        rc, out = _raw_newton(pool, h, k, w, 2, **kwargs)
        assert rc == INVALID and _untouched_n(out), kwargs
    slab = ShootProblem(q.SlabFlow(U_i0=0.35, width=1.5, n_nodes=130), "kink", ctx=pool.ctx)
    untwisted = ShootProblem(q.CylinderFlow(U_i0=0.35, width=1.5, n_nodes=130), "kink", ctx=pool.ctx)
    try:
        for other in (slab, untwisted):
            rc, out = _raw_slopes(pool, other.handle, k, w, 2)
            assert rc == UNSUPPORTED and _untouched_s(out)
            assert b"ES_GEOM_CYLINDER_TWIST" in pool.ctx.lib.es_last_error(pool.ctx.handle)
            with pytest.raises(_lib.EsError):
                _lib.check(pool.ctx.handle, rc)
            rc, out = _raw_newton(pool, other.handle, k, w, 2)
            assert rc == UNSUPPORTED and _untouched_n(out)
        # section 15 keeps refusing the twisted problem
        assert pool.ctx.lib.es_cyl_complex_root_slopes(pool.ctx.handle, h, None, None, None, 0, None, None, None, None) == UNSUPPORTED
    finally:
        slab.close()
        untwisted.close()
    g = _np(s.root_slopes(mode, k, w, m=m))                                             # the context is still usable
    assert g["status"].tolist() == [0, 0] and np.isfinite(g["outer"]).all()


# ---- densify and most_unstable ----------------------------------------------------------------------------------------------
def test_densify_follows_the_branch(pool):
    """Problem A (v_twist = 2, power = 1, r_axis = 1e-2, m = 3, kink), N = 130: five coarse rows on k in [0.85, 1.1] with the
    roots unstable_roots finds in A's window (one per row), densified to 21 wavenumbers with nothing read back between the
    calls: every fine point accepted and on the model's secant root; the growth rate falls over the whole interval, and
    most_unstable reports no maximum inside it."""
    import torch
    from eigensolver_amd import postprocess as pp
    s, mode, m = pool.solver("root A")
    M, kc, wc_model, kf, branch = C.densify_case()
    rows = s.unstable_roots(mode, kc, C.DENSIFY_W_RE, C.DENSIFY_W_IM, m=m)
    assert [len(r) for r in rows] == [1] * 5, rows
    wc = np.array([r[0] for r in rows])
    assert np.max(np.abs(wc - wc_model)) <= 1e-10
    dev = f"cuda:{pool.ctx.device}"
    dkc, dwc, dkf = (torch.as_tensor(np.array(a), device=dev) for a in (kc, wc, kf))
    s.problem(mode, m)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # torch calls the mode a prototype that does not see every such call
        torch.cuda.set_sync_debug_mode("error")      # a synchronising torch call between the launches would raise
        try:
            dd = s.densify(mode, dkc, dwc, dkf, m=m)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    assert set(dd) >= {"k", "w", "dwdk", "resid", "iters", "flag", "predicted", "max_shift"}
    d = _host(dd)
    err, pred = np.abs(d["w"] - branch), np.abs(d["predicted"] - d["w"])
    print(f"densify on k in [{C.DENSIFY_K[0]}, {C.DENSIFY_K[1]}]: worst |w - model secant root| = {err.max():.2e} (bound 1.0e-10), worst "
          f"|predicted - w| = {pred.max():.2e}, iters {d['iters'].tolist()}, smallest max_shift {d['max_shift'].min():.2e}")
    assert d["flag"].tolist() == [1] * 21 and np.array_equal(d["k"], kf)
    assert err.max() <= 1e-10
    assert pred.max() <= 10.0 * C.DENSIFY_PREDICTION_MEASURED < d["max_shift"].min()
    assert 1 <= d["iters"].min() and d["iters"].max() <= 3
    outer, inner, _ = C.jets(M, kf, branch)
    slope = dwdk(outer, inner)
    assert np.max(np.abs(d["dwdk"] - slope)) <= 1e-9 * np.max(np.abs(slope))
    assert np.all(d["dwdk"].imag < 0.0)
    kstar, _ = pp.most_unstable(d["k"], d["w"], d["dwdk"])
    print(f"most unstable: k* = {kstar}; Im d omega / dk over the interval in [{slope.imag.min():.4f}, {slope.imag.max():.4f}]")
    assert len(kstar) == 0

"""es_cyl_complex_root_slopes and es_cyl_complex_newton (include/eigensolver_amd.h section 15) on the GPU, with the Python layer
on top (CylinderComplex.root_slopes / group_velocity / newton / densify, postprocess.most_unstable).

Yardsticks (tests/cyl_complex_slope_model.py, pinned on the CPU by tests/test_cyl_complex_slope_model.py), with the bounds
tests/test_complex_slopes_gpu.py uses for the same comparisons:
  value    rows 0 of outer and inner against es_cyl_complex_eval_points(parts): 1e-12 of max(|outer|, |inner|), statuses equal.
  jets     the NumPy forward-mode restatement of the value model: every row of outer and inner within 1e-10 of
           max(|outer_x|, |inner_x|) of its row.
  Newton   the iteration rule restated on the model: the same number of steps, |w - w_model| <= 1e-12 max(1, |w|).
Node counts: N = 3 (two steps), 129 (128 steps: exactly one LDS chunk), 130 (a chunk of one step on top), 300 (three chunks).
Pair counts 1, 63, 64, 65, 257: one lane, a ragged and a full workgroup, one lane in a second, five workgroups.
`pytest -s` prints every measured figure next to its bound.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cyl_complex_slope_model as C  # noqa: E402

SENT_D, SENT_S, SENT_I = -7.25e77, 0xEE, -77
NODES = (3, 129, 130, 300)
COUNTS = (1, 63, 64, 65, 257)
K3 = np.array([0.5, 1.1, 2.0])
# phase-speed windows of the samples (those of tests/test_cyl_complex_gpu.py)
WINDOW = {"kh_w15": (0.4, 1.7), "sausage": (0.4, 1.7), "density": (2.0, 5.5), "m3": (2.7, 5.5), "rplus": (0.5, 1.7)}
INVALID, UNSUPPORTED = 1, 5
# the window of the densify test: phase speeds around the narrow jet's kink branch on k in [1.5, 2.5].  At N = 130 the model's
# cell rule finds exactly one distinct root in it for each of the five coarse rows (checked with CylComplexModel.find_roots).
DENSIFY_K = (1.5, 2.5)
DENSIFY_W_RE, DENSIFY_W_IM = np.linspace(1.0, 1.6, 13), np.linspace(0.005, 0.105, 11)


class _Pool:
    """one CylinderComplex per (kind, N) on the session's context"""
    def __init__(self, ctx):
        self.ctx, self.s = ctx, {}

    def solver(self, name, N=C.N0):
        if (name, N) not in self.s:
            from eigensolver_amd import CylinderComplex
            eq, mode, m = C.problems(N)[name]
            self.s[(name, N)] = (CylinderComplex(eq, ctx=self.ctx), mode, m)
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
    """257 pairs: k drawn from K3, Re omega = k W with W in the kind's window, |Im omega| in [0.05, 0.6] k / 2 with both signs
    (some of them leaky), and the kind's leaky pair put in the middle of the first three consecutive good ones, at index
    `at`.  With the model's jets at them, computed once per session: (k, w, outer, inner, status, at)."""
    rng = np.random.default_rng(500 + N)
    lo, hi = WINDOW[name]
    k = K3[rng.integers(0, 3, 257)]
    w = k * rng.uniform(lo, hi, 257) + 1j * 0.5 * k * rng.uniform(0.05, 0.6, 257) * rng.choice([-1.0, 1.0], 257)
    M = C.model(name, N)
    mo, mi, mst = C.jets(M, k, w)
    at = next(i for i in range(1, 60) if mst[i - 1] == 0 and mst[i] == 0 and mst[i + 1] == 0)
    k[at], w[at] = C.LEAKY[name]
    mo[:, at:at + 1], mi[:, at:at + 1], mst[at:at + 1] = C.jets(M, k[at], w[at:at + 1])
    for a in (k, w, mo, mi, mst):
        a.setflags(write=False)
    return k, w, mo, mi, mst, at


# ---- value and jets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NODES)
@pytest.mark.parametrize("name", C.KINDS)
def test_value_and_jets(pool, name, N):
    s, mode, m = pool.solver(name, N)
    k, w, mo, mi, mst, at = _sample(name, N)
    ok = mst == 0
    assert mst[at] == 1 and ok[at - 1] and ok[at + 1] and ok[0] and ok.sum() > 120, ok.sum()
    worst_v, worst_j, full = 0.0, [0.0, 0.0, 0.0], None
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
        for c in range(3):
            scm = np.maximum(np.abs(mo[c][:n][o]), np.abs(mi[c][:n][o]))
            worst_j[c] = max(worst_j[c], float(np.max(np.abs(g["outer"][c][o] - mo[c][:n][o]) / scm)),
                             float(np.max(np.abs(g["inner"][c][o] - mi[c][:n][o]) / scm)))
        if full is None:
            full = g
        else:                                        # a pair does not depend on how many others the launch holds
            assert np.array_equal(g["outer"], full["outer"][:, :n], equal_nan=True), n
            assert np.array_equal(g["inner"], full["inner"][:, :n], equal_nan=True), n
    print(f"{name} N {N}: rows 0 against eval_points {worst_v:.2e} of max(|outer|, |inner|) (bound 1.0e-12); against the model "
          f"value {worst_j[0]:.2e}, d/dw {worst_j[1]:.2e}, d/dk {worst_j[2]:.2e} of max(|outer_x|, |inner_x|) (bound 1.0e-10); "
          f"{int(ok.sum())} OK pairs of 257")
    assert worst_v <= 1e-12
    assert max(worst_j) <= 1e-10, worst_j
    # the leaky pair's neighbours are what they are without it
    k2, w2 = k[:64].copy(), w[:64].copy()
    k2[at], w2[at] = k[at + 1], w[at + 1]
    h = _np(s.root_slopes(mode, k2, w2, m=m))
    keep = np.arange(64) != at
    assert h["status"][at] == 0 and np.array_equal(h["outer"][:, at], full["outer"][:, at + 1])
    assert np.array_equal(h["outer"][:, keep], full["outer"][:, :64][:, keep], equal_nan=True)
    assert np.array_equal(h["inner"][:, keep], full["inner"][:, :64][:, keep], equal_nan=True)


# ---- the real axis and the conjugate ----------------------------------------------------------------------------------------
def test_real_axis_slope_is_the_real_group_speed(pool):
    """At the real roots of the real-axis case: Im d omega / dk of the complex path vanishes (1e-13) and the real part is
    ShootProblem.group_velocity within 10 x the difference of the two NumPy models."""
    from eigensolver_amd import CylinderComplex, ShootProblem
    eq, mode, m, k, w, _, _ = C.real_axis_case()
    bound = 10.0 * C.REAL_AXIS_MEASURED
    s = CylinderComplex(eq, ctx=pool.ctx)
    gp = ShootProblem(eq, mode, m=m, ctx=pool.ctx)
    try:
        cx = s.group_velocity(mode, dict(k=k, w=w + 0j), m=m).cpu().numpy()
        cg = gp.group_velocity(dict(k=k, w=w)).cpu().numpy()
    finally:
        s.close()
        gp.close()
    sc = np.maximum(1.0, np.abs(cg))
    ere, eim = np.abs(cx.real - cg) / sc, np.abs(cx.imag)
    print(f"{C.REAL_AXIS_CASE}: {len(k)} real roots, worst |Re d omega / dk - c_g| / max(1, |c_g|) = {ere.max():.2e} (bound "
          f"{bound:.1e}), worst |Im d omega / dk| = {eim.max():.2e} (bound 1.0e-13)")
    assert eim.max() <= 1e-13
    assert ere.max() <= bound


@pytest.mark.parametrize("name", C.KINDS)
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


# ---- Newton -----------------------------------------------------------------------------------------------------------------
def _check_newton(g, models, what):
    for i, mm in enumerate(models):
        dw = abs(g["w"][i] - mm["w"]) / max(1.0, abs(mm["w"]))
        print(f"{what} lane {i}: iters {g['iters'][i]} (model {mm['iters']}), |w - w_model| / max(1, |w|) = {dw:.2e} "
              f"(bound 1.0e-12), flag {g['flag'][i]} (model {mm['flag']}), resid {g['resid'][i]:.1e} %")
        assert g["iters"][i] == mm["iters"] and dw <= 1e-12 and g["flag"][i] == mm["flag"], (what, i, g["w"][i], mm)
        if mm["status"] == 0:
            assert abs(g["dwdk"][i] - mm["dwdk"]) <= 1e-9 * max(1.0, abs(mm["dwdk"])), (what, i)


@pytest.mark.parametrize("width", list(C.KH_ROOTS))
def test_newton_steps_and_roots(pool, width):
    name = C.KH_NAMES[width]
    s, mode, m = pool.solver(name)
    M, root = C.model(name), C.kh_root(width)
    starts = [root + C.NEWTON_OFFSET, root - C.NEWTON_OFFSET]
    g = _host(s.newton(mode, C.K0, starts))
    _check_newton(g, [C.newton_model(M, C.K0, z) for z in starts], f"width {width:g} root +- 1e-3 (1 + i)")
    assert g["flag"].tolist() == [1, 1] and np.all(g["iters"] <= 5) and np.all(np.abs(g["w"] - root) <= 1e-12)
    assert g["w"].dtype == np.complex128 and g["iters"].dtype == np.int32
    g = _host(s.newton(mode, C.K0, [C.KH_ROOTS[width]]))                                # from the six digits of the table
    print(f"width {width:g} from the table's digits: iters {g['iters'][0]}, flag {g['flag'][0]}, |w - root| = {abs(g['w'][0] - root):.2e}")
    assert g["flag"][0] == 1 and g["iters"][0] <= 5 and abs(g["w"][0] - root) <= 1e-12


def test_newton_guards(pool):
    s, mode, m = pool.solver("kh_w15")
    M, root = C.model("kh_w15"), C.kh_root(1.5)
    guess = root + C.NEWTON_OFFSET
    # max_iter = 0 reproduces root_slopes: the guess with its residual and slope
    k = C.K0 + 1e-3 * np.arange(65)
    guesses = guess + 0.002 * np.arange(65) * (1 - 0.5j)
    guesses[40], k[40] = C.LEAKY["kh_w15"][1], C.LEAKY["kh_w15"][0]
    g = _host(s.newton(mode, k, guesses, max_iter=0, tol_percent=1.0))
    r = s.root_slopes(mode, k, guesses)
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
    g = _host(s.newton(mode, C.K0, [guess], max_iter=1, step_cap=1e-4))
    mm = C.newton_model(M, C.K0, guess, max_iter=1, step_cap=1e-4)
    print(f"capped step: |w - guess| = {abs(g['w'][0] - guess):.17e}")
    assert g["iters"][0] == 1 and abs(abs(g["w"][0] - guess) - 1e-4) <= 1e-15 and abs(g["w"][0] - mm["w"]) <= 1e-12
    assert g["flag"][0] == mm["flag"]
    # max_shift smaller than the distance travelled: flag 0 as the model says, w still reported
    g = _host(s.newton(mode, C.K0, [guess, guess], max_shift=1e-4))
    mm = C.newton_model(M, C.K0, guess, max_shift=1e-4)
    assert g["flag"].tolist() == [mm["flag"]] * 2 == [0, 0] and abs(g["w"][0] - root) <= 1e-12 and g["resid"][0] < 1e-6
    g = _host(s.newton(mode, C.K0, [guess], max_shift=1e-2, tol_percent=1e-6))
    mm = C.newton_model(M, C.K0, guess, max_shift=1e-2, tol_percent=1e-6)
    assert g["flag"].tolist() == [mm["flag"]] == [1] and abs(g["w"][0] - root) <= 1e-12


def test_newton_leaky_guess_among_good_ones(pool):
    """Lanes of one workgroup that stop after different numbers of steps, a leaky guess among them: flag 0, no step, NaN
    resid and slope for it, and the others bit for bit what they are without it."""
    s, mode, m = pool.solver("kh_w15")
    M, root = C.model("kh_w15"), C.kh_root(1.5)
    starts = [root + off for off in (0, 1e-9, 1e-6 * (1 - 1j), 1e-4j, 1e-3, 5e-3 * (1 - 1j))]
    models = [C.newton_model(M, C.K0, z) for z in starts]
    assert len({mm["iters"] for mm in models}) >= 3 and all(mm["flag"] == 1 for mm in models)
    g = _host(s.newton(mode, C.K0, starts))
    _check_newton(g, models, "mixed step counts")
    leaky = C.LEAKY["kh_w15"][1]
    h = _host(s.newton(mode, C.K0, starts[:3] + [leaky] + starts[3:]))
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
    """es_cyl_complex_root_slopes into buffers pre-filled with sentinels ([3, n] complex and [n], at least one entry); outputs
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
    rc = pool.ctx.lib.es_cyl_complex_root_slopes(pool.ctx.handle, handle,
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
    rc = pool.ctx.lib.es_cyl_complex_newton(pool.ctx.handle, handle,
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
    """count as a device word: 0, 1, 64, 65 and n + 5 of n = 70 pairs (two workgroups); entries past min(count, n) keep the
    sentinel, the others are what a call without count writes."""
    s, mode, m = pool.solver("kh_w15", 129)
    h = s.problem(mode, m).handle
    n = 70
    w = C.kh_root(1.5) + 1e-3 + 2e-4 * np.arange(n) * (1 + 1j)
    k = C.K0 + 1e-3 * np.arange(n)
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
    s, mode, m = pool.solver("kh_w15", 3)
    h = s.problem(mode, m).handle
    k, w = np.array([p[0] for p in C.NON_ROOT["kh_w15"]]), np.array([p[1] for p in C.NON_ROOT["kh_w15"]])
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
    s, mode, m = pool.solver("kh_w15", 3)
    h = s.problem(mode, m).handle
    k, w = C.K0, np.array([2.1 + 0.3j, 2.6 - 0.2j])
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
    twisted = ShootProblem(q.CylinderRotation(v_twist=0.25, power=0.8, n_nodes=130), "kink", ctx=pool.ctx)
    try:
        for other in (slab, twisted):
            rc, out = _raw_slopes(pool, other.handle, k, w, 2)
            assert rc == UNSUPPORTED and _untouched_s(out)
            assert b"ES_GEOM_CYLINDER" in pool.ctx.lib.es_last_error(pool.ctx.handle)
            with pytest.raises(_lib.EsError):
                _lib.check(pool.ctx.handle, rc)
            rc, out = _raw_newton(pool, other.handle, k, w, 2)
            assert rc == UNSUPPORTED and _untouched_n(out)
    finally:
        slab.close()
        twisted.close()
    g = _np(s.root_slopes(mode, k, w))                                                  # the context is still usable
    assert g["status"].tolist() == [0, 0] and np.isfinite(g["outer"]).all()


# ---- densify and most_unstable ----------------------------------------------------------------------------------------------
def _follow(M, k_from, w_from, ks):
    """the model's branch through (k_from, w_from) at the wavenumbers ks (monotone, starting next to k_from): secant roots,
    each start predicted with the model's slope at the previous root"""
    out, k, w = [], k_from, w_from
    for kk in ks:
        outer, inner, _ = C.jets(M, k, w)
        w = C.model_root(M, kk, w + C.dwdk(outer, inner)[0] * (kk - k))
        k = kk
        out.append(w)
    return np.array(out)


def test_densify_follows_the_branch(pool):
    """Width 1.5, kink, N = 130: five coarse rows on k in [1.5, 2.5] with the roots unstable_roots finds in the window above
    (one per row), densified to 21 wavenumbers: every fine point accepted and on the model's secant root; the growth rate
    rises over the whole interval in the model, and most_unstable reports no maximum inside it."""
    from eigensolver_amd import postprocess as pp
    from eigensolver_amd.shooting import W_PHASE_SPEED
    s, mode, m = pool.solver("kh_w15")
    M, root = C.model("kh_w15"), C.kh_root(1.5)
    kf = np.linspace(DENSIFY_K[0], DENSIFY_K[1], 21)
    kc = kf[::5]
    rows = s.unstable_roots(mode, kc, DENSIFY_W_RE, DENSIFY_W_IM, W_PHASE_SPEED)
    assert [len(r) for r in rows] == [1] * 5, rows
    wc = np.array([r[0] for r in rows])
    branch = np.concatenate([_follow(M, C.K0, root, kf[9::-1])[::-1], [root], _follow(M, C.K0, root, kf[11:])])
    assert abs(kf[10] - C.K0) < 1e-15 and np.max(np.abs(wc - branch[::5])) <= 1e-6
    d = _host(s.densify(mode, kc, wc, kf))
    err, pred = np.abs(d["w"] - branch), np.abs(d["predicted"] - d["w"])
    print(f"densify on k in [{DENSIFY_K[0]}, {DENSIFY_K[1]}]: worst |w - model secant root| = {err.max():.2e} (bound 1.0e-10), worst "
          f"|predicted - w| = {pred.max():.2e}, iters {d['iters'].tolist()}, smallest max_shift {d['max_shift'].min():.2e}")
    assert d["flag"].tolist() == [1] * 21 and np.array_equal(d["k"], kf)
    assert err.max() <= 1e-10
    outer, inner, _ = C.jets(M, kf, branch)
    slope = C.dwdk(outer, inner)
    assert np.max(np.abs(d["dwdk"] - slope)) <= 1e-9
    kstar, wstar = pp.most_unstable(d["k"], d["w"], d["dwdk"])
    model_kstar, _ = pp.most_unstable(kf, branch, slope)
    print(f"most unstable: k* = {kstar} (model {model_kstar}); Im d omega / dk over the interval in "
          f"[{slope.imag.min():.4f}, {slope.imag.max():.4f}]")
    assert len(kstar) == len(model_kstar)
    if len(model_kstar):
        assert np.all((kstar > DENSIFY_K[0]) & (kstar < DENSIFY_K[1])) and np.max(np.abs(kstar - model_kstar)) <= 1e-6
    else:
        assert np.all(slope.imag > 0.0)

"""es_shoot_root_curvature and es_shoot_cg_extrema (include/eigensolver_amd.h section 21) on the GPU, with
ShootProblem.root_curvature / cg_extrema / group_speed_extrema on top.

Yardsticks (tests/root_curvature_model.py, pinned on the CPU by tests/test_root_curvature_model.py; read here from
tests/golden/root_curvature_model.json, so that no model runs beside the GPU):
  rows 0-2  es_shoot_root_slopes at the same pairs: 1e-13 of max(|outer_x|, |inner_x|) per row, and, the first-order part
            of the second-order jets being formed by the first-order operators themselves, bit for bit.
  rows 3-5  the model's second derivatives by Cauchy's formula: 1e-10 of max(|outer_xx|, |inner_xx|) per row, the project's
            bound for the GPU against a NumPy restatement, where the stored self-discrepancy of the pair is <= 1e-11, and
            10 x that self-discrepancy otherwise.  No pair is left out.  The four large-gap cases (far field at ten
            wavelengths, mu (R - 1) = 30, 39, 41, 50) take Jet2 through both texts of exterior_cylinder, the one without an
            I pair from 40 on and exp(-2 gap) just below; all sixteen pairs have a self-discrepancy under 1e-11.
  curvature d2 omega / dk2 at the model's roots against the model's, per case under 10 x the figure the CPU test measured
            between the model and the difference of its own c_g (CURVE_MEASURED): 3.2e-11 to 9.0e-11 of max(1, |q|).
  extrema   the NumPy restatement of the rule, iterate for iterate.
`pytest -s` prints every measured figure next to its bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import real_eigen_model as M  # noqa: E402
from tests import root_curvature_model as C  # noqa: E402
from tests import unit_scaling as us  # noqa: E402

SENT_D, SENT_I, SENT_S = -7.25e77, -77, 0xEE
EDGE = "CF_flow_kink_N130"
X_OUT = ("k", "w", "cg", "q", "resid", "iters", "flag", "status")
X_SENT = dict(k=SENT_D, w=SENT_D, cg=SENT_D, q=SENT_D, resid=SENT_D, iters=SENT_I, flag=SENT_I, status=SENT_S)


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


def _np(t):
    return t.cpu().numpy()


def _leaky(name, k):
    eq = M.all_cases()[name][0]
    return (k * eq.U_e if not M.is_cyl(eq) else 0.0) + k * 1.05 * max(eq.c_e, eq.vA_e)      # m_e < 0


# ---- the twelve rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASES)
def test_rows_against_root_slopes_and_the_model(pool, name):
    gp = pool.problem(name)
    g = C.read_golden()["cases"][name]
    k, w = np.array(g["k"]), np.array(g["w"])
    if name in M.LARGE_GAP:
        gaps = g["gap"]                                         # mu (R - 1): both texts of exterior_cylinder in one call
        assert len(gaps) == len(k) and min(gaps) < 40.0 <= max(gaps), gaps
    c, s = gp.root_curvature(k, w), gp.root_slopes(k, w)
    assert tuple(c.outer.shape) == (6, len(k)) and c.status.cpu().tolist() == [0] * len(k) == s.status.cpu().tolist()
    co, ci, so, si = _np(c.outer), _np(c.inner), _np(s.outer), _np(s.inner)
    first = np.maximum(np.abs(co[:3] - so), np.abs(ci[:3] - si)) / np.maximum(np.abs(so), np.abs(si))
    print(f"{name}: rows 0-2 against root_slopes {first.max():.1e} (bound 1e-13), bit-identical: "
          f"{np.array_equal(co[:3], so) and np.array_equal(ci[:3], si)}")
    assert first.max() <= 1e-13
    assert np.array_equal(co[:3], so) and np.array_equal(ci[:3], si)      # Jet2's first-order part IS Jet's arithmetic
    mo, mi = np.array(g["outer"]), np.array(g["inner"])
    err = np.maximum(np.abs(co[3:] - mo[3:]), np.abs(ci[3:] - mi[3:])) / np.maximum(np.abs(mo[3:]), np.abs(mi[3:]))
    disc = np.array(C.SELF_MEASURED[name])
    bound = np.where(disc <= 1e-11, 1e-10, 10.0 * disc)
    for p in range(len(k)):
        print(f"{name} pair {p}: rows 3-5 against the model {err[:, p].max():.1e} (bound {bound[p]:.1e}, model "
              f"self-discrepancy {disc[p]:.1e})")
    assert np.all(err <= bound[None, :]), (name, err)
    # the named fields and the properties are the rows' differences and the formulas of the header
    D = co - ci
    for r, f in enumerate(("D", "D_w", "D_k", "D_ww", "D_wk", "D_kk")):
        assert np.array_equal(_np(getattr(c, f)), D[r]), f
    cg = -D[2] / D[1]
    for got, want in ((c.group_velocity, cg), (c.curvature, -(D[5] + 2.0 * D[4] * cg + D[3] * cg * cg) / D[1]),
                      (c.newton_dw, -D[0] / D[1]), (c.halley_dw, -2.0 * D[0] * D[1] / (2.0 * D[1] * D[1] - D[0] * D[3]))):
        assert np.max(np.abs(_np(got) - want) / np.abs(want)) <= 1e-14


@pytest.mark.parametrize("name", C.CURVE_CASES)
def test_curvature_at_the_models_roots(pool, name):
    gp = pool.problem(name)
    g = C.read_golden()["curve"][name]
    k, w, q = (np.array(g[f]) for f in ("k", "w", "q"))
    assert len(k) >= 1
    c = gp.root_curvature(k, w)
    err = np.abs(_np(c.curvature) - q) / np.maximum(1.0, np.abs(q))
    bound = 10.0 * C.CURVE_MEASURED[name]
    print(f"{name}: d2w/dk2 {q} at {len(k)} roots, worst difference to the model {err.max():.1e} (bound {bound:.1e})")
    assert err.max() <= bound
    assert np.max(np.abs(_np(c.group_velocity) - np.array(g["cg"])) / np.maximum(1.0, np.abs(g["cg"]))) <= 1e-10


# ---- launch edges of es_shoot_root_curvature --------------------------------------------------------------------------------
def _raw(pool, name, k, w, n, count=None, skip=(), prob=True, null_in=False):
    """es_shoot_root_curvature through the raw ABI into sentinel-filled buffers; outputs named in `skip` are NULL."""
    import torch
    from eigensolver_amd import _lib
    gp = pool.problem(name)
    na = max(n, 1)
    dk, dw = gp._dev(np.atleast_1d(k)), gp._dev(np.atleast_1d(w))
    dev = dk.device
    bufs = {f: torch.full((6, na), SENT_D, dtype=torch.float64, device=dev) for f in ("outer", "inner")}
    bufs["status"] = torch.full((na,), SENT_S, dtype=torch.uint8, device=dev)
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_shoot_root_curvature(pool.ctx.handle, gp.handle if prob else None,
                                              *[None if null_in else _lib.ptr(t) for t in (dk, dw)], n,
                                              _lib.ptr(dc) if dc is not None else None,
                                              *[None if f in skip else _lib.ptr(bufs[f]) for f in ("outer", "inner", "status")])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _untouched(out, a=0, fields=("outer", "inner", "status")):
    return all(np.all(out[f][..., a:] == (SENT_S if f == "status" else SENT_D)) for f in fields)


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_lane_counts(pool, n):
    k, w = M.pairs(EDGE)
    rc, first = _raw(pool, EDGE, k, w, len(k))
    assert rc == 0 and np.all(first["status"] == 0) and np.isfinite(first["outer"]).all()
    rc, out = _raw(pool, EDGE, np.resize(k, n), np.resize(w, n), n)
    assert rc == 0
    for i in range(n):
        assert all(np.array_equal(out[f][..., i], first[f][..., i % len(k)]) for f in out), i


def test_device_count_and_null_outputs(pool):
    k, w = (np.resize(a, 130) for a in M.pairs(EDGE))
    rc, full = _raw(pool, EDGE, k, w, 130)
    assert rc == 0 and np.all(full["status"] == 0)
    for count, written in ((70, 70), (0, 0), (500, 130), (-3, 0)):
        rc, out = _raw(pool, EDGE, k, w, 130, count=count)
        assert rc == 0
        for f in out:
            assert np.array_equal(out[f][..., :written], full[f][..., :written]), (count, f)
        assert _untouched(out, written), count
    for f in ("outer", "inner", "status"):
        rc, out = _raw(pool, EDGE, k, w, 130, skip=(f,))
        assert rc == 0 and _untouched(out, 0, (f,)) and all(np.array_equal(out[h], full[h]) for h in out if h != f), f
    rc, out = _raw(pool, EDGE, k, w, 0, null_in=True, skip=("outer", "inner", "status"))
    assert rc == 0
    rc, out = _raw(pool, EDGE, k, w, 0)
    assert rc == 0 and _untouched(out)


def test_bad_pairs_change_nothing_beside_them(pool):
    k, w = (np.resize(a, 70).copy() for a in M.pairs(EDGE))
    rc, good = _raw(pool, EDGE, k, w, 70)
    assert rc == 0
    w[3], w[40], w[66] = _leaky(EDGE, k[3]), np.nan, np.inf
    rc, got = _raw(pool, EDGE, k, w, 70)
    st = pool.problem(EDGE).root_slopes(k, w).status.cpu().numpy()
    assert rc == 0 and np.array_equal(got["status"], st) and st[3] == 1 and st[40] == 2 and st[66] == 2
    for i in (3, 40, 66):
        assert np.isnan(got["outer"][:, i]).all() and np.isnan(got["inner"][:, i]).all()
    keep = np.delete(np.arange(70), [3, 40, 66])
    assert all(np.array_equal(got[f][..., keep], good[f][..., keep]) for f in got) and np.isfinite(got["outer"][:, keep]).all()


def test_argument_errors(pool):
    from eigensolver_amd import _lib
    k, w = M.pairs(EDGE)
    for kwargs in (dict(n=-1), dict(null_in=True), dict(prob=False)):
        rc, out = _raw(pool, EDGE, k, w, kwargs.pop("n", len(k)), **kwargs)
        assert rc == 1 and _untouched(out), kwargs                                # ES_ERR_INVALID_ARG
        assert pool.ctx.lib.es_last_error(pool.ctx.handle).decode() != ""
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
    assert pool.problem(EDGE).root_curvature(k, w).status.cpu().tolist() == [0] * len(k)      # the context is still usable


# ---- es_shoot_cg_extrema --------------------------------------------------------------------------------------------------------
def _raw_x(pool, name, br, n, count=None, max_iter=40, tol=1e-3, skip=(), prob=True, null_in=False):
    """es_shoot_cg_extrema through the raw ABI on the bracket arrays br = (k_lo, w_lo, k_hi, w_hi), sentinel-filled outputs"""
    import torch
    from eigensolver_amd import _lib
    gp = pool.problem(name)
    na = max(n, 1)
    din = [gp._dev(np.atleast_1d(a)) for a in br]
    dev = din[0].device
    bufs = {f: torch.full((na,), X_SENT[f], dtype=torch.float64, device=dev) for f in X_OUT[:5]}
    bufs["iters"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    bufs["flag"] = torch.full((na,), SENT_I, dtype=torch.int32, device=dev)
    bufs["status"] = torch.full((na,), SENT_S, dtype=torch.uint8, device=dev)
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_shoot_cg_extrema(pool.ctx.handle, gp.handle if prob else None,
                                          *[None if null_in else _lib.ptr(t) for t in din], n,
                                          _lib.ptr(dc) if dc is not None else None, max_iter, tol,
                                          *[None if f in skip else _lib.ptr(bufs[f]) for f in X_OUT])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _x_untouched(out, a=0, fields=X_OUT):
    return all(np.all(out[f][a:] == X_SENT[f]) for f in fields)


def _bracket():
    return tuple(C.read_golden()["extremum"]["bracket"])


def test_extremum_against_the_restatement(pool):
    """The group-speed minimum of the fast sausage branch of the density slab, k in [1.8, 2.4]."""
    gp = pool.problem(C.EXTREMUM_CASE)
    m = C.read_golden()["extremum"]
    br = _bracket()
    g = _host(gp.cg_extrema(*[np.array([a]) for a in br]))
    assert g["k"].dtype == np.float64 and g["iters"].dtype == np.int32 and g["flag"].dtype == np.int32 and g["status"].dtype == np.uint8
    ends = gp.root_curvature(np.array([br[0], br[2]]), np.array([br[1], br[3]])).curvature.cpu().numpy()
    dk, dw = abs(g["k"][0] - m["k"]) / m["k"], abs(g["w"][0] - m["w"]) / m["w"]
    print(f"k* = {g['k'][0]!r} (restatement {m['k']!r}, relative difference {dk:.1e}, bound 1e-12), omega* {dw:.1e}, c_g* = "
          f"{g['cg'][0]!r} (restatement {m['cg']!r}), q* = {g['q'][0]:.2e} (restatement {m['q']:.2e}; at the ends {ends}), "
          f"iters {g['iters'][0]} (restatement {m['iters']}), resid {g['resid'][0]:.1e} %")
    assert m["changed"] and g["flag"].tolist() == [1] and g["status"].tolist() == [0]
    assert g["iters"][0] == m["iters"] and dk <= 1e-12 and dw <= 1e-12
    assert abs(g["cg"][0] - m["cg"]) <= 1e-10 * abs(m["cg"])
    assert abs(g["q"][0] - m["q"]) <= 1e-10 * np.abs(ends).max() and ends[0] * ends[1] < 0
    assert 1.15 <= g["w"][0] / g["k"][0] <= 1.29
    # step for step: the iterate the rule reports after j steps is the restatement's
    for j in range(1, m["iters"] + 1):
        gj = _host(gp.cg_extrema(*[np.array([a]) for a in br], max_iter=j))
        assert gj["iters"][0] == j and abs(gj["k"][0] - m["trace"][j - 1]) <= 1e-12 * m["trace"][j - 1], j
    g0 = _host(gp.cg_extrema(*[np.array([a]) for a in br], max_iter=0))            # no step allowed: the better end, no flag lost
    assert g0["iters"][0] == 0 and g0["k"][0] == (br[0] if abs(ends[0]) <= abs(ends[1]) else br[2])


def test_bracket_without_a_sign_change(pool):
    gp = pool.problem(C.EXTREMUM_CASE)
    br = _bracket()
    k0, w0 = C.EXTREMUM_START
    w0 = float(gp.newton(np.array([k0]), np.array([w0]))["w"].cpu()[0])
    ends = gp.root_curvature(np.array([br[2], k0]), np.array([br[3], w0])).curvature.cpu().numpy()
    g = _host(gp.cg_extrema(np.array([br[2]]), np.array([br[3]]), np.array([k0]), np.array([w0])))
    print(f"q at the ends {ends}, reported k {g['k'][0]!r}, q {g['q'][0]!r}")
    assert ends[0] * ends[1] > 0 and g["flag"].tolist() == [0] and g["iters"].tolist() == [0] and g["status"].tolist() == [0]
    assert g["k"][0] == (br[2] if abs(ends[0]) <= abs(ends[1]) else k0)
    assert abs(g["q"][0] - ends[np.argmin(np.abs(ends))]) <= 1e-10 * np.abs(ends).max()


def test_leaky_end_and_device_count(pool):
    br = _bracket()
    rc, one = _raw_x(pool, C.EXTREMUM_CASE, br, 1)
    assert rc == 0 and one["flag"].tolist() == [1]
    tiled = [np.full(3, a) for a in br]
    tiled[3][1] = _leaky(C.EXTREMUM_CASE, br[2])
    rc, got = _raw_x(pool, C.EXTREMUM_CASE, tiled, 3)
    assert rc == 0 and got["flag"].tolist() == [1, 0, 1]
    for i in (0, 2):
        assert all(np.array_equal(got[f][i], one[f][0]) for f in X_OUT) and all(np.isfinite(got[f][i]) for f in X_OUT)
    # 65 copies, 64 counted: a full wave and a second workgroup that leaves at once
    rc, got = _raw_x(pool, C.EXTREMUM_CASE, [np.full(65, a) for a in br], 65, count=64)
    assert rc == 0 and _x_untouched(got, 64)
    assert all(np.array_equal(got[f][:64], np.full(64, one[f][0])) for f in X_OUT)
    rc, got = _raw_x(pool, C.EXTREMUM_CASE, br, 1, skip=("status",))
    assert rc == 0 and _x_untouched(got, 0, ("status",)) and all(np.array_equal(got[f], one[f]) for f in X_OUT[:-1])


def test_extrema_argument_errors(pool):
    from eigensolver_amd import _lib
    br = _bracket()
    for kwargs in (dict(n=-1), dict(null_in=True), dict(prob=False), dict(max_iter=-1), dict(tol=0.0), dict(tol=-1e-3),
                   dict(tol=float("nan"))) + tuple(dict(skip=(f,)) for f in X_OUT[:-1]):
        rc, out = _raw_x(pool, C.EXTREMUM_CASE, br, kwargs.pop("n", 1), **kwargs)
        assert rc == 1 and _x_untouched(out), kwargs                               # ES_ERR_INVALID_ARG
        assert pool.ctx.lib.es_last_error(pool.ctx.handle).decode() != ""
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
    rc, out = _raw_x(pool, C.EXTREMUM_CASE, br, 0, null_in=True, skip=X_OUT)
    assert rc == 0


def test_group_speed_extrema_of_a_traced_branch(pool):
    """trace_branches from 9 coarse rows, k in [1.2, 4.0]; the one extremum of the traced branch is the direct answer."""
    gp = pool.problem(C.EXTREMUM_CASE)
    ks = np.linspace(1.2, 4.0, 9)
    k0, w0 = C.EXTREMUM_START
    # the coarse roots of the branch, row by row from the start root (second-order Taylor prediction, Newton)
    ws = np.empty(9)
    for idx in sorted(range(9), key=lambda i: abs(ks[i] - k0)):
        near = (k0, w0) if idx == int(np.argmin(np.abs(ks - k0))) else (ks[idx - 1], ws[idx - 1]) if ks[idx] > k0 \
            else (ks[idx + 1], ws[idx + 1])
        c = gp.root_curvature(np.array([near[0]]), np.array([near[1]]))
        dk = ks[idx] - near[0]
        guess = near[1] + float(c.group_velocity.cpu()[0]) * dk + 0.5 * float(c.curvature.cpu()[0]) * dk * dk
        n = _host(gp.newton(np.array([ks[idx]]), np.array([guess])))
        assert n["flag"].tolist() == [1], (idx, n)
        ws[idx] = n["w"][0]
    cg = gp.root_slopes(ks, ws).group_velocity.cpu().numpy()
    sig = gp.mode_signature(ks, ws)
    label = (int(sig.nodes_value.cpu()[0]), int(sig.nodes_flux.cpu()[0]))
    assert sig.nodes_value.cpu().tolist() == [label[0]] * 9 and sig.nodes_flux.cpu().tolist() == [label[1]] * 9
    t = gp.trace_branches({label: (ws, ks, cg)}, np.linspace(1.2, 4.0, 113))
    b = t.branches[label]
    assert b["flag"].cpu().tolist() == [1] * 113
    x = gp.group_speed_extrema(b)
    n = int(x["count"].cpu()[0])
    x = _host(x)
    direct = _host(gp.cg_extrema(*[np.array([a]) for a in _bracket()]))
    print(f"{n} extremum: k* = {x['k'][:n]}, direct {direct['k']}, flag {x['flag'][:n]}, iters {x['iters'][:n]}")
    assert n == 1 and x["flag"][0] == 1 and len(x["k"]) == 112
    assert abs(x["k"][0] - direct["k"][0]) <= 1e-12 * direct["k"][0] and abs(x["w"][0] - direct["w"][0]) <= 1e-12 * direct["w"][0]
    assert abs(x["cg"][0] - direct["cg"][0]) <= 1e-12 * direct["cg"][0]
    # a point without a flag between two flagged ones is stepped over
    flag = b["flag"].clone()
    flag[5] = 0
    y = gp.group_speed_extrema(dict(b, flag=flag))
    assert int(y["count"].cpu()[0]) == 1 and abs(float(y["k"].cpu()[0]) - direct["k"][0]) <= 1e-12 * direct["k"][0]
    # host arrays are taken as well, flag included
    z = gp.group_speed_extrema({f: b[f].cpu().numpy() for f in ("k", "w", "flag")})
    assert int(z["count"].cpu()[0]) == 1 and float(z["k"].cpu()[0]) == x["k"][0]
    with pytest.raises(ValueError):
        gp.group_speed_extrema(dict(k=b["k"], w=b["w"], flag=b["flag"][:5]))


# ---- units -------------------------------------------------------------------------------------------------------------------
SECOND_ROWS = (("D", 0), ("D_w", -1), ("D_k", 0), ("D_ww", -2), ("D_wk", -1), ("D_kk", 0))     # powers of V beyond D's


def _scaled_run(ctx, name, pv, pr):
    eq, mode, m, _ = M.all_cases()[name]
    gp = us.ScaledShootProblem(eq, mode, m, ctx=ctx, pv=pv, pr=pr)
    k, w = M.pairs(name)
    c = gp.root_curvature(k, np.ldexp(w, pv))
    out = dict(fam=us.family(gp.desc.geometry), outer=_np(c.outer), inner=_np(c.inner), status=_np(c.status),
               D=np.array([_np(getattr(c, f)) for f, _ in SECOND_ROWS]), cg=_np(c.group_velocity), q=_np(c.curvature))
    if name == C.EXTREMUM_CASE:
        br = _bracket()
        out["x"] = _host(gp.cg_extrema(np.array([br[0]]), np.ldexp(np.array([br[1]]), pv), np.array([br[2]]),
                                       np.ldexp(np.array([br[3]]), pv)))
    gp.close()
    return out


@pytest.mark.parametrize("name", ("CF_flow_kink_N130", "SD_w15_sausage"))
def test_unit_scaling(es_ctx, name):
    """V = 2^+-20, R = 4^+-20: every second omega-derivative comes out with two more factors 1 / V than D and D_wk with one
    more; d2 omega / dk2 and c_g scale by V; k* does not move.  Exact after the exponent shift."""
    ref = _scaled_run(es_ctx, name, 0, 0)
    a, b = us.LAW[ref["fam"]]["D"]
    assert np.all(ref["status"] == 0)
    for pv, pr in ((20, 20), (-20, -20)):
        got = _scaled_run(es_ctx, name, pv, pr)
        us.assert_same(ref["status"], got["status"], "status")
        for r, (row, da) in enumerate(SECOND_ROWS):
            for side in ("outer", "inner", "D"):
                us.assert_scaled(ref[side][r], got[side][r], a + da, b, pv, pr, what=f"{side}[{row}]")
        us.assert_scaled(ref["cg"], got["cg"], 1, 0, pv, pr, what="group_velocity")
        us.assert_scaled(ref["q"], got["q"], 1, 0, pv, pr, what="curvature")
        if "x" in ref:
            assert ref["x"]["flag"].tolist() == [1]
            for f in ("iters", "flag", "status"):
                us.assert_same(ref["x"][f], got["x"][f], "cg_extrema." + f)
            for f, law in (("k", (0, 0)), ("w", (1, 0)), ("cg", (1, 0)), ("q", (1, 0)), ("resid", (0, 0))):
                us.assert_scaled(ref["x"][f], got["x"][f], *law, pv, pr, what="cg_extrema." + f)

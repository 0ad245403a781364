"""es_shoot_root_slopes (include/eigensolver_amd.h section 11) on the GPU.

Yardsticks (tests/root_slope_model.py, pinned on the CPU by tests/test_root_slope_model.py):
  value   outer - inner against the D of es_shoot_eval_points at the same pairs: the same adjoint march, only the grouping of
          the reciprocals differs (one per RK4 step here, one per two steps there): 1e-12 of max(|outer|, |inner|).
  jets    the model's complex-step derivatives, a different route from the kernel's forward-mode jets: each of outer_w,
          inner_w, outer_k, inner_k within 1e-10 of max(|outer_x|, |inner_x|) of the model, the project's bound for the GPU
          against a NumPy restatement.
  c_g     the slope of the C port's root curve through each of its accepted roots, with the per-case bounds the CPU test fixed
          (root_slope_model.slope_bound); none left out.
`pytest -s` prints every measured figure next to its bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mode_signature_model as S  # noqa: E402
from tests import real_eigen_model as M  # noqa: E402
from tests import root_slope_model as R  # noqa: E402

SENT_D, SENT_S = -7.25e77, 0xEE


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


def _np(s):
    return dict(outer=s.outer.cpu().numpy(), inner=s.inner.cpu().numpy(), status=s.status.cpu().numpy())


def _raw(pool, name, k, w, n, count=None, skip=(), prob=True, null_kw=False):
    """es_shoot_root_slopes through the raw ABI into buffers pre-filled with sentinels ([3, n] and [n], at least one entry);
    outputs named in `skip` are passed as NULL.  Returns (return code, dict of the three arrays)."""
    import torch
    from eigensolver_amd import _lib
    gp = pool.problem(name)
    na = max(n, 1)
    dk, dw = gp._dev(k), gp._dev(w)
    dev = dk.device
    bufs = dict(outer=torch.full((3, na), SENT_D, dtype=torch.float64, device=dev),
                inner=torch.full((3, na), SENT_D, dtype=torch.float64, device=dev),
                status=torch.full((na,), SENT_S, dtype=torch.uint8, device=dev))
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_shoot_root_slopes(pool.ctx.handle, gp.handle if prob else None,
                                           None if null_kw else _lib.ptr(dk), None if null_kw else _lib.ptr(dw), n,
                                           _lib.ptr(dc) if dc is not None else None,
                                           *[None if f in skip else _lib.ptr(bufs[f]) for f in ("outer", "inner", "status")])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _same(a, b, fields=("outer", "inner", "status")):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


# ---- value parts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.VALUE_CASES + M.LARGE_GAP + ("CF_flow_kink_target",))
def test_value_is_the_determinant_of_eval_points(pool, name):
    gp = pool.problem(name)
    k, w = R.pairs(name)
    g = _np(gp.root_slopes(k, w))
    D, st = (a.cpu().numpy() for a in gp.eval_points(k, w))
    assert g["status"].tolist() == [0] * len(k)
    assert all(s in (0, 3) for s in st.tolist())            # eval_points may add the continuum flag; its D is the same march
    for i in range(len(k)):
        sc = max(abs(g["outer"][0, i]), abs(g["inner"][0, i]))
        err = abs((g["outer"][0, i] - g["inner"][0, i]) - D[i]) / sc
        print(f"{name} pair {i}: |(outer - inner) - D| / max(|outer|, |inner|) = {err:.2e} (bound 1.0e-12)")
        assert err <= 1e-12, (name, i, g["outer"][0, i], g["inner"][0, i], D[i])


# Where the slopes march and the point march group their reciprocals alike, the two run the same operations on the same values
# (one formula text, es_shoot_device.hpp, over jets and over doubles): the twisted cylinder at any node count (its point march
# takes one reciprocal per step) and every family at N = 2 (a single, even top step is taken alone).
BITWISE_CASES = tuple(n for n in R.VALUE_CASES if n.startswith("CR_")) + ("CF_flow_kink_N2", "SFG_flow_kink_N2", "SD_w15_sausage_N2")


@pytest.mark.parametrize("name", BITWISE_CASES)
def test_value_is_the_determinant_bit_for_bit_where_the_reciprocals_group_alike(pool, name):
    gp = pool.problem(name)
    k, w = R.pairs(name)
    g = _np(gp.root_slopes(k, w))
    D = gp.eval_points(k, w)[0].cpu().numpy()
    assert g["status"].tolist() == [0] * len(k)
    d = g["outer"][0] - g["inner"][0]                       # fp64 on the host: the subtraction the point kernel ends with
    for i in range(len(k)):
        print(f"{name} pair {i}: outer - inner = {d[i]!r}, D = {D[i]!r}, difference {d[i] - D[i]:.1e} (required: equal bits)")
    assert np.isfinite(D).all() and np.array_equal(d, D), (name, d, D)


def test_status_and_nan_rows(pool):
    """A leaky pair and two non-finite ones among good ones: the status is the exterior status es_shoot_mode_signature reports
    (that of es_shoot_eigenfunction, whose rows are NaN exactly there), all six entries are NaN there and the other pairs are
    what they are without them."""
    name = "CF_flow_kink_N130"
    eq = M.all_cases()[name][0]
    gp = pool.problem(name)
    k, w = (np.resize(a, 8).copy() for a in M.pairs(name))
    good = _np(gp.root_slopes(k, w))
    assert good["status"].tolist() == [0] * 8
    w[1] = k[1] * 1.05 * max(eq.c_e, eq.vA_e)               # above both exterior speeds: m_e < 0
    w[4] = float("nan")
    w[6] = float("inf")
    got = _np(gp.root_slopes(k, w))
    sig = gp.mode_signature(k, w).status.cpu().numpy()
    rows = gp.eigenfunction(k, w, n_ext=0)["value_int"].cpu().numpy()
    assert got["status"].tolist() == sig.tolist()
    assert got["status"][1] == 1 and got["status"][4] == 2 and got["status"][6] == 2
    for i in range(8):
        bad = i in (1, 4, 6)
        assert np.isnan(rows[i]).all() == bad
        assert np.isnan(got["outer"][:, i]).all() == bad and np.isnan(got["inner"][:, i]).all() == bad
        if not bad:
            assert np.array_equal(got["outer"][:, i], good["outer"][:, i]) and np.array_equal(got["inner"][:, i], good["inner"][:, i])


# ---- jets against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.JET_CASES + M.LARGE_GAP)
def test_jets_against_the_model(pool, name):
    k, w = R.pairs(name)
    g = _np(pool.problem(name).root_slopes(k, w))
    mo, mi = R.case_jets(name)
    assert g["status"].tolist() == [0] * len(k)
    for i in range(len(k)):
        for c, what in ((0, "value"), (1, "d/dw"), (2, "d/dk")):
            sc = max(abs(mo[c, i]), abs(mi[c, i]))
            eo, ei = abs(g["outer"][c, i] - mo[c, i]) / sc, abs(g["inner"][c, i] - mi[c, i]) / sc
            print(f"{name} pair {i} {what}: outer {eo:.2e}, inner {ei:.2e} of max(|outer|, |inner|) (bound 1.0e-10)")
            assert eo <= 1e-10 and ei <= 1e-10, (name, i, what, g["outer"][c, i], mo[c, i], g["inner"][c, i], mi[c, i])


# ---- c_g at the port's roots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SLOPE_CASES)
def test_group_speed_is_the_slope_of_the_root_curve(pool, name):
    k, w, slope = R.curve_slopes(name)
    assert len(k) == R.SLOPE_ROOTS[name] and np.isfinite(slope).all()
    s = pool.problem(name).root_slopes(k, w)
    assert s.status.cpu().numpy().tolist() == [0] * len(k)
    cg = s.group_velocity.cpu().numpy()
    nd = s.newton_dw.cpu().numpy()
    err = np.abs(cg - slope) / np.maximum(1.0, np.abs(slope))
    print(f"{name}: {len(k)} roots, worst |c_g - slope| / max(1, |slope|) = {err.max():.2e} (bound {R.slope_bound(name):.1e}), "
          f"worst |Newton correction| = {np.abs(nd).max():.1e}")
    assert err.max() <= R.slope_bound(name), (name, err)
    assert np.array_equal(cg, pool.problem(name).group_velocity(dict(k=k, w=w)).cpu().numpy())


# ---- launch shape -----------------------------------------------------------------------------------------------------------
def test_partial_last_wave(pool):
    """n = 3 * 64 + 1 pairs, the case's pairs tiled: every copy equals the first, bit for bit."""
    name = "CF_flow_kink_N130"
    k, w = M.pairs(name)
    n = 3 * 64 + 1
    rc, out = _raw(pool, name, np.resize(k, n), np.resize(w, n), n)
    assert rc == 0 and np.all(out["status"] == 0)
    rc, first = _raw(pool, name, k, w, len(k))
    assert rc == 0 and np.isfinite(first["outer"]).all() and np.isfinite(first["inner"]).all()
    assert len({float(x) for x in first["outer"][1]}) == len(k)                          # the pairs differ
    for i in range(n):
        j = i % len(k)
        assert np.array_equal(out["outer"][:, i], first["outer"][:, j]) and np.array_equal(out["inner"][:, i], first["inner"][:, j]), i


# ---- d_count ----------------------------------------------------------------------------------------------------------------
def test_device_count(pool):
    name = "SFG_flow_kink_N130"
    k, w = M.pairs(name)
    kk, ww = np.resize(k, 130), np.resize(w, 130)
    rc, full = _raw(pool, name, kk, ww, 130)
    assert rc == 0 and np.all(full["status"] == 0)
    for count, written in ((70, 70), (0, 0), (500, 130), (-3, 0)):
        rc, out = _raw(pool, name, kk, ww, 130, count=count)
        assert rc == 0
        for f in ("outer", "inner", "status"):
            assert np.array_equal(out[f][..., :written], full[f][..., :written]), (count, f)     # rows stay 130 apart
            assert np.all(out[f][..., written:] == (SENT_S if f == "status" else SENT_D)), (count, f)


def test_table_path_without_read_back(pool):
    """find_roots_async into a table of capacity 256, then group_velocity(table, count) on the device count: the first `count`
    entries are those of the synchronous path."""
    import torch
    name = "CF_flow_kink_N130"
    gp = pool.problem(name)
    k, W = S.root_grid(name)
    D, st = gp.eval_grid(k, W)
    roots, cnt = gp.find_roots(k, W, D, st)
    want = gp.group_velocity(roots).cpu().numpy()
    table = gp.alloc_root_table(256)
    count = torch.zeros(1, dtype=torch.int32, device=D.device)
    gp.find_roots_async(k, W, D, st, table, count)
    got = gp.group_velocity(table, count)                   # enqueued behind the search: nothing has been read back yet
    assert int(count.item()) == cnt and 0 < cnt <= 256
    got = got.cpu().numpy()
    assert len(got) == 256 and np.isfinite(want).sum() >= 7
    assert np.array_equal(got[:cnt], want, equal_nan=True)


# ---- arguments --------------------------------------------------------------------------------------------------------------
def test_each_output_may_be_null(pool):
    name = "SD_w15_sausage"
    k, w = M.pairs(name)
    rc, full = _raw(pool, name, k, w, len(k))
    assert rc == 0 and np.all(full["status"] == 0)
    for f in ("outer", "inner", "status"):
        rc, out = _raw(pool, name, k, w, len(k), skip=(f,))
        assert rc == 0
        assert _same(out, full, [g for g in ("outer", "inner", "status") if g != f]), f
        assert np.all(out[f] == (SENT_S if f == "status" else SENT_D)), f
    rc, out = _raw(pool, name, k, w, len(k), skip=("outer", "inner", "status"))
    assert rc == 0


def test_argument_errors(pool):
    from eigensolver_amd import _lib
    name = "CF_flow_kink_N130"
    k, w = M.pairs(name)
    rc, out = _raw(pool, name, k, w, 0, null_kw=True)       # n = 0 with NULL arrays: success, nothing touched
    assert rc == 0 and np.all(out["outer"] == SENT_D) and np.all(out["status"] == SENT_S)
    for kwargs in (dict(n=-1), dict(n=len(k), null_kw=True), dict(n=len(k), prob=False)):
        n = kwargs.pop("n")
        rc, out = _raw(pool, name, k, w, n, **kwargs)
        assert rc == 1                                      # ES_ERR_INVALID_ARG
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
        assert np.all(out["outer"] == SENT_D) and np.all(out["inner"] == SENT_D) and np.all(out["status"] == SENT_S)
    g = _np(pool.problem(name).root_slopes(k, w))           # the context is still usable
    assert g["status"].tolist() == [0] * len(k) and np.isfinite(g["outer"]).all()

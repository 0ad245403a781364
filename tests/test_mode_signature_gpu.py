"""es_shoot_mode_signature (include/eigensolver_amd.h section 10) on the GPU.

Yardsticks (tests/mode_signature_model.py, pinned on the CPU by tests/test_mode_signature_model.py):
  model   the count rule and the peaks applied to the NumPy restatement of the interior algorithm
          (tests/real_eigen_model.model).  Every pair used here is `decided`: no entry of its rows is small enough for rounding
          to change the count, so the four integers are compared for equality.
  arrays  the same rule applied to what es_shoot_eigenfunction writes for the same pairs.  Both kernels call one function for
          the marches (csrc/es_interior_march.hpp), so the comparison is exact: each peak is max |row| bit for bit and each peak
          node is np.argmax(|row|), the smallest index that attains it in either march direction.
Bounds against the model: integers equal; peaks 1e-10 of the model's (bound b of tests/test_eigenfunction_gpu.py: the same algorithm in fp64, the
model's own rounding is <= 1e-11); a peak node equal to the model's, or one where the model's row is within 1e-10 of its peak.
GPU figures (one MI355X, `pytest -s` prints every pair): all labels equal, worst |gpu - model| / model of the 104 peaks 9.6e-14
(SFU_sausage).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mode_signature_model as S  # noqa: E402
from tests import real_eigen_model as M  # noqa: E402

INTS = ("nodes_value", "nodes_flux", "peak_node_value", "peak_node_flux")
PEAKS = ("peak_value", "peak_flux")
FIELDS = INTS + PEAKS + ("status",)
SENT_I, SENT_D, SENT_S = -7777, -7.25e77, 0xEE


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


def _np(sig):
    return {f: getattr(sig, f).cpu().numpy() for f in FIELDS}


def _raw(pool, name, k, w, n, count=None, skip=(), n_alloc=None, prob=True, null_kw=False):
    """es_shoot_mode_signature through the raw ABI into buffers pre-filled with sentinels; outputs named in `skip` are passed
    as NULL.  Returns (return code, dict of the seven arrays)."""
    import torch
    from eigensolver_amd import _lib
    gp = pool.problem(name)
    n_alloc = max(n, 1) if n_alloc is None else n_alloc
    dk, dw = gp._dev(k), gp._dev(w)
    dev = dk.device
    bufs = {f: torch.full((n_alloc,), SENT_I, dtype=torch.int32, device=dev) for f in INTS}
    bufs.update({f: torch.full((n_alloc,), SENT_D, dtype=torch.float64, device=dev) for f in PEAKS})
    bufs["status"] = torch.full((n_alloc,), SENT_S, dtype=torch.uint8, device=dev)
    dc = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    rc = pool.ctx.lib.es_shoot_mode_signature(pool.ctx.handle, gp.handle if prob else None,
                                              None if null_kw else _lib.ptr(dk), None if null_kw else _lib.ptr(dw), n,
                                              _lib.ptr(dc) if dc is not None else None,
                                              *[None if f in skip else _lib.ptr(bufs[f]) for f in FIELDS])
    pool.ctx.synchronize()
    return rc, {f: b.cpu().numpy() for f, b in bufs.items()}


def _same(a, b, fields=FIELDS):
    """bitwise equality of two result dicts (NaN peaks included)"""
    return all(np.array_equal(a[f], b[f], equal_nan=f in PEAKS) for f in fields)


# ---- against the model and against the GPU's own arrays ---------------------------------------------------------------------
@pytest.mark.parametrize("name", S.MODEL_CASES)
def test_against_model(pool, name):
    k, w = M.pairs(name)
    g = _np(pool.problem(name).mode_signature(k, w))
    assert g["status"].tolist() == [0] * len(k)
    for i in range(len(k)):
        m = S.signature(name, float(k[i]), float(w[i]))
        got = tuple(int(g[f][i]) for f in INTS[:2])
        print(f"{name} pair {i}: label {got} (model {m.label}), peaks {g['peak_value'][i]:.6g} @ {g['peak_node_value'][i]}, "
              f"{g['peak_flux'][i]:.6g} @ {g['peak_node_flux'][i]}")
        assert got == m.label, (name, i, got, m.label)
        for f, row, pk, node in (("value", m.value, m.peak_value, m.peak_node_value),
                                 ("flux", m.flux, m.peak_flux, m.peak_node_flux)):
            gp_, gn = g["peak_" + f][i], int(g["peak_node_" + f][i])
            print(f"  {f}: |gpu - model| / model = {abs(gp_ - pk) / pk:.2e} (bound 1.0e-10)")
            assert abs(gp_ - pk) <= 1e-10 * pk, (name, i, f, gp_, pk)
            assert 0 <= gn < len(row)
            assert gn == node or abs(abs(row[gn]) - pk) <= 1e-10 * pk, (name, i, f, gn, node)


@pytest.mark.parametrize("name", S.MODEL_CASES)
def test_against_own_eigenfunction_arrays(pool, name):
    gp = pool.problem(name)
    k, w = M.pairs(name)
    g = _np(gp.mode_signature(k, w))
    e = gp.eigenfunction(k, w, n_ext=0)
    value, flux = e["value_int"].cpu().numpy(), e["flux_int"].cpu().numpy()
    assert g["status"].tolist() == [0] * len(k)
    for i in range(len(k)):
        a = S.of_rows(value[i], flux[i])
        assert (int(g["nodes_value"][i]), int(g["nodes_flux"][i])) == a.label, (name, i)
        for f, row in (("value", value[i]), ("flux", flux[i])):
            peak, node = float(np.max(np.abs(row))), int(np.argmax(np.abs(row)))       # argmax: the smallest such index
            gp_, gn = float(g["peak_" + f][i]), int(g["peak_node_" + f][i])
            print(f"{name} pair {i} {f}: peak {gp_!r} @ {gn}, row {peak!r} @ {node}")
            assert gp_ == peak, (name, i, f, gp_, peak)
            assert gn == node, (name, i, f, gn, node)


# ---- on roots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CF_flow_kink_N130", "SFG_flow_kink_N130"])
def test_labels_of_roots(pool, name):
    from eigensolver_amd import postprocess as pp
    gp = pool.problem(name)
    k, W = S.root_grid(name)
    D, st = gp.eval_grid(k, W)
    roots, cnt = gp.find_roots(k, W, D, st)
    assert cnt == len(roots["k"])
    sig = gp.label_roots(roots)
    g = _np(sig)
    rk, rw, flag = (roots[a].cpu().numpy() for a in ("k", "w", "flag"))
    acc = [i for i in range(cnt) if flag[i] == 1 and g["status"][i] == 0]
    assert len(acc) >= 7
    for i in acc:
        m = S.signature(name, float(rk[i]), float(rw[i]))
        assert S.pair_decided(name, float(rk[i]), float(rw[i])), (name, i)
        assert (int(g["nodes_value"][i]), int(g["nodes_flux"][i])) == m.label, (name, i, rk[i], rw[i])
    labels = {(int(g["nodes_value"][i]), int(g["nodes_flux"][i])) for i in acc}
    assert labels == S.BRANCHES[name], (name, sorted(labels))
    curves = pp.split_by_signature(roots, sig)
    assert set(curves) == S.BRANCHES[name]
    assert sum(len(c[0]) for c in curves.values()) == len(acc)
    for lab, (ws, ks) in curves.items():
        assert len(ks) >= 1 and np.all(np.diff(ks) > 0), (name, lab, ks)        # one k-sorted curve: one root per row
        print(f"{name} {lab}: {len(ks)} roots, W {np.min(ws / ks):.3f}-{np.max(ws / ks):.3f}")


# ---- launch edges -----------------------------------------------------------------------------------------------------------
def test_launch_edges(pool):
    """n = 1, 63, 64, 65, 130 (one lane; a wave less one; a full wave; one lane into the second; a partial third): every copy
    of a pair gives what the pair gives alone, and nothing is written past entry n."""
    name = "CF_flow_kink_N130"
    k, w = M.pairs(name)
    alone = []
    for j in range(len(k)):
        rc, a = _raw(pool, name, k[j:j + 1], w[j:j + 1], 1)
        assert rc == 0 and a["status"][0] == 0 and a["nodes_value"][0] >= 0
        alone.append(a)
    assert len({(float(a["peak_value"][0]), float(a["peak_flux"][0])) for a in alone}) == len(k)     # the pairs differ
    kk, ww = np.resize(k, 130), np.resize(w, 130)
    for n in (1, 63, 64, 65, 130):
        rc, out = _raw(pool, name, kk[:n], ww[:n], n, n_alloc=n + 1)
        assert rc == 0
        for f in FIELDS:
            assert out[f][n] == (SENT_D if f in PEAKS else SENT_S if f == "status" else SENT_I), (n, f)
            for i in range(n):
                assert out[f][i] == alone[i % len(k)][f][0], (n, f, i)


# ---- d_count ----------------------------------------------------------------------------------------------------------------
def test_device_count(pool):
    name = "CF_flow_kink_N130"
    k, w = M.pairs(name)
    kk, ww = np.resize(k, 130), np.resize(w, 130)
    rc, full = _raw(pool, name, kk, ww, 130)
    assert rc == 0 and np.all(full["status"] == 0)
    for count, written in ((70, 70), (0, 0), (500, 130), (-3, 0)):
        rc, out = _raw(pool, name, kk, ww, 130, count=count)
        assert rc == 0
        for f in FIELDS:
            sent = SENT_D if f in PEAKS else SENT_S if f == "status" else SENT_I
            assert np.array_equal(out[f][:written], full[f][:written]), (count, f)
            assert np.all(out[f][written:] == sent), (count, f)


def test_table_path_without_read_back(pool):
    """find_roots_async into a table of capacity 256, then label_roots(table, count) on the device count: the first `count`
    entries are those of the synchronous search and its labels."""
    import torch
    name = "CF_flow_kink_N130"
    gp = pool.problem(name)
    k, W = S.root_grid(name)
    D, st = gp.eval_grid(k, W)
    roots, cnt = gp.find_roots(k, W, D, st)
    want = _np(gp.label_roots(roots))
    table = gp.alloc_root_table(256)
    count = torch.zeros(1, dtype=torch.int32, device=D.device)
    gp.find_roots_async(k, W, D, st, table, count)
    sig = gp.label_roots(table, count)                   # enqueued behind the search: nothing has been read back yet
    got = _np(sig)
    assert int(count.item()) == cnt and 0 < cnt <= 256
    assert all(len(got[f]) == 256 for f in FIELDS)
    assert _same({f: got[f][:cnt] for f in FIELDS}, want)
    assert np.array_equal(table[0]["w"][:cnt].cpu().numpy(), roots["w"].cpu().numpy())


# ---- a pair that is not ES_PT_OK ---------------------------------------------------------------------------------------------
def test_leaky_pair(pool):
    name = "CF_flow_kink_N130"
    eq = M.all_cases()[name][0]
    k, w = (a.copy() for a in M.pairs(name))
    rc, good = _raw(pool, name, k, w, len(k))
    assert rc == 0
    w[1] = k[1] * 1.05 * max(eq.c_e, eq.vA_e)            # above both exterior speeds: m_e < 0
    rc, out = _raw(pool, name, k, w, len(k))
    assert rc == 0
    assert out["status"][1] != 0
    assert all(out[f][1] == -1 for f in INTS) and all(np.isnan(out[f][1]) for f in PEAKS)
    others = [0, 2, 3]
    assert _same({f: out[f][others] for f in FIELDS}, {f: good[f][others] for f in FIELDS})
    assert np.all(good["status"] == 0)


# ---- NULL outputs -----------------------------------------------------------------------------------------------------------
def test_each_output_may_be_null(pool):
    name = "SFG_flow_kink_N130"
    k, w = M.pairs(name)
    rc, full = _raw(pool, name, k, w, len(k))
    assert rc == 0 and np.all(full["status"] == 0)
    for f in FIELDS:
        rc, out = _raw(pool, name, k, w, len(k), skip=(f,))
        assert rc == 0
        rest = [g for g in FIELDS if g != f]
        assert _same(out, full, rest), f
        assert np.all(out[f] == (SENT_D if f in PEAKS else SENT_S if f == "status" else SENT_I)), f
    rc, out = _raw(pool, name, k, w, len(k), skip=FIELDS)
    assert rc == 0


# ---- argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors(pool):
    from eigensolver_amd import _lib
    name = "CF_flow_kink_N130"
    k, w = M.pairs(name)
    rc, out = _raw(pool, name, k, w, 0, null_kw=True)                      # n = 0 with NULL arrays: success, nothing touched
    assert rc == 0 and np.all(out["nodes_value"] == SENT_I) and np.all(out["status"] == SENT_S)
    for kwargs in (dict(n=-1), dict(n=len(k), null_kw=True), dict(n=len(k), prob=False)):
        n = kwargs.pop("n")
        rc, out = _raw(pool, name, k, w, n, **kwargs)
        assert rc == 1                                                     # ES_ERR_INVALID_ARG
        with pytest.raises(_lib.EsError, match="invalid argument"):
            _lib.check(pool.ctx.handle, rc)
        assert np.all(out["nodes_value"] == SENT_I) and np.all(out["peak_value"] == SENT_D)
    g = _np(pool.problem(name).mode_signature(k, w))                       # the context is still usable
    assert g["status"].tolist() == [0] * len(k) and np.all(g["nodes_value"] >= 0)

"""Root search of the closed-form uniform cylinder over (order, k, omega): es_cyl_uniform_find_roots / _async.

The bracket list is checked against a NumPy composition on es_cyl_uniform_eval, the roots against a NumPy restatement of
the refinement rule that evaluates D with the scipy oracle (oracle.cylinder.uniform_closed_form)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cylinder as oc  # noqa: E402

K3 = np.array([0.6, 1.7, 3.1])
ES_ERR_INVALID_ARG, ES_ERR_CAPACITY = 1, 3
COLUMNS = ("k", "w", "w_lo", "w_hi", "resid", "row", "order", "flag")


def equilibrium(photo):
    from eigensolver_amd import equilibrium as q
    if photo:
        return q.CylinderFlow(c_e=1.5, vA_e=0.5, r_sign=1.0), oc.CylinderEquilibrium("flow", c_e=1.5, vA_e=0.5), 0.52, 1.48
    return q.CylinderFlow(), oc.CylinderEquilibrium("flow"), 0.9, 4.95


def speeds(lo, hi, nw):
    return lo + (np.arange(nw) + 0.5) * (hi - lo) / nw


def searcher(es_ctx, photo, mode):
    from eigensolver_amd import CylinderUniform
    return CylinderUniform(equilibrium(photo)[0], mode, ctx=es_ctx)


def host_brackets(es_ctx, photo, mode, orders, k, W, w_mode=1):
    """(order, row, j) of every sign change D[j] D[j+1] < 0 with both statuses 0, from eval_grid order by order; also the
    stacked D and status."""
    from eigensolver_amd import CylinderUniform
    eq = equilibrium(photo)[0]
    recs, Ds, sts = [], [], []
    for m in orders:
        D, st = CylinderUniform(eq, mode, m=m, ctx=es_ctx).eval_grid(k, W, w_mode=w_mode)
        D, st = D.cpu().numpy(), st.cpu().numpy()
        Ds.append(D); sts.append(st)
        with np.errstate(invalid="ignore"):
            hit = (D[:, :-1] * D[:, 1:] < 0.0) & (st[:, :-1] == 0) & (st[:, 1:] == 0)
        recs += [(m, int(r), int(j)) for r, j in zip(*np.nonzero(hit))]
    return recs, np.stack(Ds), np.stack(sts)


def as_numpy(t):
    return {c: t[c].cpu().numpy().copy() for c in COLUMNS}


def assert_tables_identical(a, b, n=None):
    for c in COLUMNS:
        x, y = a[c][:n], b[c][:n]
        assert x.shape == y.shape, c
        assert x.tobytes() == y.tobytes(), c


# ---- Test 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [3, 1])
@pytest.mark.parametrize("nw", [1, 2, 63, 64, 65, 257])
def test_bracket_list_is_the_composition_on_eval_grid(es_ctx, nw, nk):
    k, W = K3[:nk], speeds(0.9, 4.95, nw)
    orders = range(1, 4)
    recs, D_ref, st_ref = host_brackets(es_ctx, False, "kink", orders, k, W)
    cu = searcher(es_ctx, False, "kink")
    tg, ng, D, st = cu.find_roots(k, W, orders=orders, want_grid=True)
    t, n = cu.find_roots(k, W, orders=orders)
    tg, t = as_numpy(tg), as_numpy(t)
    print(f"nw={nw} nk={nk}: {n} brackets, {int(t['flag'].sum())} accepted")
    assert n == ng == len(recs)
    if nw == 65 and nk == 3:
        assert n >= 10
    assert [(int(m), int(r)) for m, r in zip(t["order"], t["row"])] == [(m, r) for m, r, _ in recs]
    for i, (m, r, j) in enumerate(recs):
        assert t["k"][i] == k[r]
        assert k[r] * W[j] <= t["w_lo"][i] <= t["w"][i] <= t["w_hi"][i] <= k[r] * W[j + 1], (m, r, j)
    D, st = D.cpu().numpy(), st.cpu().numpy()
    assert D.shape == (3, nk, nw)
    assert np.array_equal(np.isnan(D), np.isnan(D_ref))
    assert np.nan_to_num(D).tobytes() == np.nan_to_num(D_ref).tobytes()
    assert st.tobytes() == st_ref.tobytes()
    assert_tables_identical(t, tg)


# ---- NumPy model of the refinement rule, D from the scipy oracle ----------------------------------------------------------
def oracle_point(photo, mode, m, k, w):
    eq, oeq = equilibrium(photo)[:2]
    d, a, b, s = oc.uniform_closed_form(oeq, k, w, m, r_sign=eq.r_sign, ic=eq.ic, axis_bc=mode)
    if s != 0:
        return float("nan"), float("nan"), s
    return d, abs(d) * 100.0 / max(abs(a), abs(b)), s


def model_refine(f, lo, hi, n_bisect, tol_percent, trace=None):
    """R = ceil(n_bisect ln 2 / ln 17) rounds of 17-section, two regula-falsi steps, classification at the last secant point.
    f(w) -> (D, rel, status).  Returns (w, w_lo, w_hi, flag)."""
    rounds = int(math.ceil(n_bisect * math.log(2.0) / math.log(17.0)))
    flo, fhi = f(lo)[0], f(hi)[0]
    for _ in range(rounds):
        xs = [lo + (hi - lo) * (float(j + 1) / 17.0) for j in range(16)]
        ds = [f(x)[0] for x in xs]
        if trace is not None:
            trace.append((lo, hi, flo, list(ds)))
        first = next((j for j in range(16) if ds[j] * flo < 0.0), 16)          # NaN products compare false
        new_hi = (xs[first], ds[first]) if first < 16 else None
        if first > 0:
            lo = xs[first - 1]
            if ds[first - 1] == ds[first - 1]:                                  # a NaN D(lo) is refused
                flo = ds[first - 1]
        if new_hi is not None:
            hi, fhi = new_hi
    w, rel, st = lo, float("nan"), 0
    for _ in range(2):
        with np.errstate(all="ignore"):
            x = float(lo - np.float64(flo) * (hi - lo) / (np.float64(fhi) - np.float64(flo)))
        if not (lo < x < hi):
            x = (lo if abs(flo) <= abs(fhi) else hi) if x == x else lo + (hi - lo) * 0.5
        d, rel, st = f(x)
        w = x
        if d * flo < 0.0:
            hi, fhi = x, d
        elif d == d:
            lo, flo = x, d
    return w, lo, hi, int(st == 0 and rel < tol_percent)


_cache = {}


def searched(es_ctx, photo):
    """Sausage m = 0 and kink m = 1 .. 3 on the nw = 65 grid: [(mode, device table, model rows)], computed once."""
    if photo not in _cache:
        lo, hi = equilibrium(photo)[2:]
        W = speeds(lo, hi, 65)
        out = []
        for mode, orders in (("sausage", [0]), ("kink", [1, 2, 3])):
            recs, _, _ = host_brackets(es_ctx, photo, mode, orders, K3, W)
            t, n = searcher(es_ctx, photo, mode).find_roots(K3, W, orders=orders, n_bisect=40, tol_percent=1e-3)
            t = as_numpy(t)
            assert n == len(recs) == len(t["w"])
            model = []
            for m, r, j in recs:
                f = lambda w, m=m, r=r: oracle_point(photo, mode, m, K3[r], w)  # noqa: E731
                model.append(model_refine(f, K3[r] * W[j], K3[r] * W[j + 1], 40, 1e-3))
            out.append((mode, recs, t, model))
        _cache[photo] = out
    return _cache[photo]


# ---- Test 2 ------------------------------------------------------------------------------------------------------------
def test_roots_match_the_model_on_the_oracle_coronal(es_ctx):
    n_flag = n_pole = 0
    for mode, recs, t, model in searched(es_ctx, False):
        for i, ((m, r, j), (w_m, lo_m, hi_m, flag_m)) in enumerate(zip(recs, model)):
            w = t["w"][i]
            print(f"{mode} m={m} row={r} cell={j}: w={w!r} model={w_m!r} diff={abs(w - w_m) / abs(w):.2e} "
                  f"flag={t['flag'][i]}/{flag_m} resid={t['resid'][i]:.3e}")
            assert t["flag"][i] == flag_m, (mode, m, r, j)
            if flag_m:
                n_flag += 1
                assert abs(w - w_m) <= 1e-10 * abs(w), (mode, m, r, j, w, w_m)
                d_lo = oracle_point(False, mode, m, K3[r], w * (1.0 - 1e-10))[0]
                d_hi = oracle_point(False, mode, m, K3[r], w * (1.0 + 1e-10))[0]
                assert d_lo * d_hi < 0.0, (mode, m, r, j, w, d_lo, d_hi)
            else:
                n_pole += 1
                assert t["flag"][i] == 0
    assert n_flag >= 10 and n_pole >= 1


# ---- Test 3 ------------------------------------------------------------------------------------------------------------
def test_sign_change_nearest_the_lower_end_photospheric(es_ctx):
    """Photospheric grid: some bracketed cells hold more than one sign change; bracket and root must be the model's."""
    n = 0
    for mode, recs, t, model in searched(es_ctx, True):
        for i, ((m, r, j), (w_m, lo_m, hi_m, flag_m)) in enumerate(zip(recs, model)):
            got = (t["w"][i], t["w_lo"][i], t["w_hi"][i])
            err = max(abs(a - b) / abs(b) for a, b in zip(got, (w_m, lo_m, hi_m)))
            print(f"{mode} m={m} row={r} cell={j}: w={got[0]!r} model={w_m!r} err={err:.2e} flag={t['flag'][i]}/{flag_m}")
            if err > 1e-10:                                                     # diagnosis: the first differing round
                trace = []
                f = lambda w, m=m, r=r: oracle_point(True, mode, m, K3[r], w)  # noqa: E731
                W = speeds(0.52, 1.48, 65)
                model_refine(f, K3[r] * W[j], K3[r] * W[j + 1], 40, 1e-3, trace)
                for rnd, (lo, hi, flo, ds) in enumerate(trace):
                    if not (lo <= got[0] <= hi):
                        print(f"  model round {rnd}: lo={lo!r} hi={hi!r} D(lo)={flo!r} D={ds}")
                        break
            assert err <= 1e-10, (mode, m, r, j, got, (w_m, lo_m, hi_m))
            assert t["flag"][i] == flag_m
            n += 1
    assert n >= 20


# ---- Test 4 ------------------------------------------------------------------------------------------------------------
def concat(tables):
    return {c: np.concatenate([t[c] for t in tables]) for c in COLUMNS}


def test_tiling_over_rows_orders_and_w_mode_is_bit_identical(es_ctx):
    W = speeds(0.9, 4.95, 65)
    cu = searcher(es_ctx, False, "kink")
    orders = range(1, 4)
    full, n = cu.find_roots(K3, W, orders=orders)
    full = as_numpy(full)
    assert n >= 10
    # rows: three single-row calls per order, concatenated order outer (the row index of a tile is local)
    parts = []
    for m in orders:
        for r in range(3):
            t, _ = cu.find_roots(K3[r:r + 1], W, orders=[m])
            t = as_numpy(t)
            t["row"] += r
            parts.append(t)
    assert_tables_identical(full, concat(parts))
    one, _ = cu.find_roots(K3, W, orders=[1])
    assert_tables_identical(as_numpy(one), concat(parts[:3]))
    # orders: three n_orders = 1 calls
    assert_tables_identical(full, concat([as_numpy(cu.find_roots(K3, W, orders=[m])[0]) for m in orders]))
    # ES_W_PER_ROW with w[ik] = k[ik] W
    per_row, n2 = cu.find_roots(K3, K3[:, None] * W[None, :], orders=orders, w_mode=2)
    assert n2 == n
    assert_tables_identical(full, as_numpy(per_row))


# ---- Test 5 ------------------------------------------------------------------------------------------------------------
def raw_find_roots(cu, k, W, m_first, n_orders, capacity, with_order=True, n_bisect=40):
    """The synchronous entry point itself: (status, count, table dict)."""
    import torch
    from eigensolver_amd import _lib
    dev = f"cuda:{cu.ctx.device}"
    dk = torch.as_tensor(np.ascontiguousarray(k, dtype=np.float64), device=dev)
    dw = torch.as_tensor(np.ascontiguousarray(W, dtype=np.float64), device=dev)
    t, rt = cu.alloc_root_table(capacity)
    n = C.c_int(-1)
    rc = cu.ctx.lib.es_cyl_uniform_find_roots(cu.ctx.handle, C.byref(cu.params), m_first, n_orders, _lib.ptr(dk), dk.numel(),
                                              _lib.ptr(dw), dw.numel(), 1, n_bisect, 1e-3, None, None, C.byref(rt),
                                              _lib.ptr(t["order"]) if with_order else None, C.byref(n))
    return rc, n.value, t


def test_async_and_capacity(es_ctx):
    import torch
    W = speeds(0.9, 4.95, 65)
    cu = searcher(es_ctx, False, "kink")
    orders = range(1, 4)
    full, n = cu.find_roots(K3, W, orders=orders)
    full = as_numpy(full)
    assert n > 4
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ta = cu.find_roots_async(K3, W, cu.alloc_root_table(256), count, orders=orders)
    assert int(count.item()) == n
    assert_tables_identical(full, as_numpy(ta), n)
    # grid kept by the async form: the same table, D and status those of eval_grid
    D = torch.empty((3, 3, 65), dtype=torch.float64, device="cuda")
    st = torch.empty((3, 3, 65), dtype=torch.uint8, device="cuda")
    tb = cu.find_roots_async(K3, W, cu.alloc_root_table(256), count, orders=orders, D=D, status=st)
    assert int(count.item()) == n
    assert_tables_identical(full, as_numpy(tb), n)
    _, D_ref, st_ref = host_brackets(es_ctx, False, "kink", orders, K3, W)
    assert np.nan_to_num(D.cpu().numpy()).tobytes() == np.nan_to_num(D_ref).tobytes()
    assert st.cpu().numpy().tobytes() == st_ref.tobytes()
    # capacity below the count
    rc, cnt, t4 = raw_find_roots(cu, K3, W, 1, 3, 4)
    assert rc == ES_ERR_CAPACITY and cnt == n
    assert_tables_identical(full, as_numpy(t4), 4)
    t4a = cu.find_roots_async(K3, W, cu.alloc_root_table(4), count, orders=orders)
    assert int(count.item()) == n > 4
    assert_tables_identical(full, as_numpy(t4a), 4)


# ---- Test 6 ------------------------------------------------------------------------------------------------------------
def test_edges(es_ctx):
    import torch
    W = speeds(0.9, 4.95, 65)
    cu = searcher(es_ctx, False, "kink")
    for k, w, orders in ((np.zeros(0), W, [1]), (K3, np.zeros(0), [1]), (K3, W, [])):
        t, n = cu.find_roots(k, w, orders=orders)
        assert n == 0 and len(t["w"]) == 0
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        cu.find_roots_async(k, w, cu.alloc_root_table(8), count, orders=orders)
        assert int(count.item()) == 0
    assert raw_find_roots(cu, K3, W, 64, 2, 64)[0] == ES_ERR_INVALID_ARG            # orders 64, 65
    assert raw_find_roots(cu, K3, W, 60, 5, 1024)[0] == 0                           # orders 60 .. 64
    assert raw_find_roots(cu, K3, W, -1, 1, 64)[0] == ES_ERR_INVALID_ARG
    assert raw_find_roots(cu, K3, W, 1, 2, 64, with_order=False)[0] == ES_ERR_INVALID_ARG
    rc, n, t = raw_find_roots(cu, K3, W, 1, 1, 64, with_order=False)
    assert rc == 0
    ref, n_ref = cu.find_roots(K3, W, orders=[1])
    assert n == n_ref > 0
    ref, t = as_numpy(ref), as_numpy(t)
    for c in COLUMNS:
        if c != "order":
            assert ref[c].tobytes() == t[c][:n].tobytes(), c


# ---- Test 7 ------------------------------------------------------------------------------------------------------------
def test_more_rows_than_a_launch_dimension(es_ctx):
    nk = 70000
    k = np.linspace(0.05, 4.0, nk)
    W = speeds(0.9, 4.95, 3)
    recs, D_ref, st_ref = host_brackets(es_ctx, False, "kink", [1], k, W)
    t, n, D, st = searcher(es_ctx, False, "kink").find_roots(k, W, orders=[1], want_grid=True)
    t = as_numpy(t)
    print(f"nk={nk}: {n} brackets, last bracketed row {t['row'].max()}")
    assert n == len(recs) and n > 1000
    assert t["row"].tolist() == [r for _, r, _ in recs]
    # the final bracket of record i lies inside the i-th cell of the composition (a row has two cells, so this names the cell)
    lo = np.array([k[r] * W[j] for _, r, j in recs])
    hi = np.array([k[r] * W[j + 1] for _, r, j in recs])
    assert np.all((lo <= t["w_lo"]) & (t["w_lo"] <= t["w_hi"]) & (t["w_hi"] <= hi))
    # every row, those beyond 65 535 included, was evaluated as eval_grid evaluates it (the brackets of this coarse grid
    # all lie in lower rows, so the count alone says only that the upper rows flag nothing)
    D, st = D.cpu().numpy(), st.cpu().numpy()
    assert np.nan_to_num(D).tobytes() == np.nan_to_num(D_ref).tobytes()
    assert st.tobytes() == st_ref.tobytes()
    assert np.isfinite(D[0, 65536:]).any()

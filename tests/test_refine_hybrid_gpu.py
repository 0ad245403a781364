"""ES_REFINE_HYBRID on the GPU: against the GPU's own section tables (what the header guarantees, and what it calls
empirical), against the host model of the rule (tests/refine_hybrid_model.py over the CPU port), through all six search
entry points, tiled, asynchronous and at the edges.  The session's context is shared: every test that sets the rule
restores REFINE_SECTION."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cases, refine_hybrid_model as hm  # noqa: E402

CASES = cases.all_cases()
NAMES = ["CF_flow_kink", "CF_flow_sausage", "CF_uniform_kink", "CDC_w095_kink", "CR_kink", "SD_w15_kink", "SFG_flow_kink",
         "SFU_sausage", "CDP_kink", "CR_sausage"]
COLUMNS = ("k", "w", "w_lo", "w_hi", "resid", "row", "flag")
ROOT_RTOL = 1e-10          # tests/test_shoot_gpu.py
TOL = 1e-3


@contextlib.contextmanager
def rule(ctx, r):
    from eigensolver_amd import _lib
    ctx.refine_rule = r
    try:
        yield
    finally:
        ctx.refine_rule = _lib.REFINE_SECTION


def _grid(name):
    _, _, _, (lo, hi) = CASES[name]
    k = np.linspace(0.4, 3.9, 24)
    W = lo + (np.arange(192) + 0.5) * (hi - lo) / 192
    return k, W


def _problem(ctx, name):
    from eigensolver_amd import ShootProblem
    eq, mode, m, _ = CASES[name]
    return ShootProblem(eq, mode, m, ctx=ctx)


def _np(t):
    return {c: v.cpu().numpy() for c, v in t.items()}


def _rows_equal(a, b, cols=COLUMNS):
    """Per-row mask: every column of the row bit-identical."""
    same = np.ones(len(a["k"]), dtype=bool)
    for c in cols:
        x, y = np.ascontiguousarray(a[c]), np.ascontiguousarray(b[c])
        same &= (x.view(np.uint8).reshape(len(x), -1) == y.view(np.uint8).reshape(len(y), -1)).all(axis=1)
    return same


def _assert_same_table(a, b, n=None, what=""):
    for c in COLUMNS:
        x, y = a[c][:n], b[c][:n]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, c)


def _search(gp, k, W, D, st, n_bisect, r, **kw):
    with rule(gp.ctx, r):
        t, n = gp.find_roots(k, W, D, st, n_bisect=n_bisect, tol_percent=TOL, **kw)
        return _np(t), n


def test_default_rule_and_setter(es_ctx):
    from eigensolver_amd import EsError, _lib
    ctx = _lib.Context(0)
    assert ctx.refine_rule == _lib.REFINE_SECTION
    gp = _problem(ctx, "CF_flow_kink")
    k, W = _grid("CF_flow_kink")
    D, st = gp.eval_grid(k, W)
    before, n = gp.find_roots(k, W, D, st, n_bisect=16, tol_percent=TOL)
    before = _np(before)
    for bad in (2, -1, 17):
        with pytest.raises(EsError, match="invalid argument"):
            ctx.refine_rule = bad
        assert ctx.refine_rule == _lib.REFINE_SECTION
    ctx.refine_rule = _lib.REFINE_HYBRID
    assert ctx.refine_rule == _lib.REFINE_HYBRID
    with pytest.raises(EsError, match="invalid argument"):
        ctx.refine_rule = 2
    assert ctx.refine_rule == _lib.REFINE_HYBRID
    hyb, nh = gp.find_roots(k, W, D, st, n_bisect=16, tol_percent=TOL)
    ctx.refine_rule = _lib.REFINE_SECTION
    after, na = gp.find_roots(k, W, D, st, n_bisect=16, tol_percent=TOL)
    assert n == nh == na > 0
    _assert_same_table(before, _np(after), what="default rule after the hybrid rule was used")
    assert ctx.refine_stats().brackets == n
    gp.close()
    ctx.close()
    assert es_ctx.refine_rule == _lib.REFINE_SECTION


def _resid_error(gp, t, mask):
    """max |resid - rel(k, w)| over the masked rows, rel from es_shoot_eval_points at the reported root.  Absolute, not
    relative to rel: an iterate with D == 0 exactly has rel == 0, and the bound is 0 either way."""
    if not mask.any():
        return 0.0
    _, _, rel = gp.eval_points(t["k"][mask], t["w"][mask], want_rel=True)
    rel = rel.cpu().numpy()
    assert np.all(np.isfinite(rel)) and np.all(np.isfinite(t["resid"][mask]))
    return float(np.max(np.abs(t["resid"][mask] - rel)))


@pytest.mark.parametrize("n_bisect", [16, 44])
@pytest.mark.parametrize("name", NAMES)
def test_hybrid_against_section_tables_and_host_model(es_ctx, name, n_bisect):
    """Every figure is printed before it is asserted.  The residual of a reported root is the `rel` of the very evaluation
    that produced it (shoot_point at the reported omega, the function es_shoot_eval_points runs), so the bound on
    |resid - rel(k, w)| is 0 for the section table, and the hybrid table is held to what the section table meets."""
    from eigensolver_amd import _lib
    gp = _problem(es_ctx, name)
    k, W = _grid(name)
    D, st = gp.eval_grid(k, W)
    Ts, cs = _search(gp, k, W, D, st, n_bisect, _lib.REFINE_SECTION)
    Tc, cc = _search(gp, k, W, D, st, 44, _lib.REFINE_SECTION)
    es_ctx.refine_stats()
    Th, ch = _search(gp, k, W, D, st, n_bisect, _lib.REFINE_HYBRID)
    h = es_ctx.refine_stats()
    assert ch == cs == cc > 0
    assert h.brackets == ch and h.kept + h.fallback == h.brackets and h.brackets <= h.evaluations <= 8 * h.brackets
    # ---- against the GPU's own section tables ----
    assert Th["row"].tobytes() == Ts["row"].tobytes() and Th["k"].tobytes() == Ts["k"].tobytes()
    assert np.all(Th["flag"] >= Ts["flag"])
    same = _rows_equal(Th, Ts)
    assert np.all(same[Th["flag"] == 0]), "a row with flag 0 is not the section rule's row"
    new = ~same                                     # rows only the one-lane phase can have produced
    assert new.sum() <= h.kept
    assert np.all(Th["flag"][new] == 1)
    assert np.all(Tc["flag"][new] == 1), (name, np.nonzero(new & (Tc["flag"] != 1))[0])
    err = np.abs(Th["w"] - Tc["w"]) / np.abs(Tc["w"])
    worst = float(err[new].max()) if new.any() else 0.0
    cell_lo, cell_hi = hm.brackets_of(k, W, D.cpu().numpy(), st.cpu().numpy())[3:5]
    assert np.all((Th["w_lo"] <= Th["w"]) & (Th["w"] <= Th["w_hi"]))
    assert np.all((cell_lo <= Th["w_lo"]) & (Th["w_hi"] <= cell_hi))
    # residual = rel at the reported root; the bound is the one the section table meets (0: the same evaluation)
    e_s = _resid_error(gp, Ts, Ts["flag"] == 1)
    e_h = _resid_error(gp, Th, new)
    # the final bracket of a kept row holds a sign change or a zero
    if new.any():
        Dlo, _ = gp.eval_points(Th["k"][new], Th["w_lo"][new])
        Dhi, _ = gp.eval_points(Th["k"][new], Th["w_hi"][new])
        prod = Dlo.cpu().numpy() * Dhi.cpu().numpy()
    else:
        prod = np.zeros(0)
    # ---- against the host model over the CPU port ----
    eq, mode, m, _ = CASES[name]
    port = cases.port_problem(eq, mode, m)
    Dp, _, stp = port.eval_grid(k, W, w_mode=1, nthreads=8)
    Tm, cm, info = hm.find_roots(port, k, W, Dp, stp, n_bisect=n_bisect, tol=TOL, nthreads=8)
    assert cm == ch
    both = new & info["kept"]
    dm = np.abs(Th["w"] - Tm["w"]) / np.abs(Tm["w"])
    worst_m = float(dm[both].max()) if both.any() else 0.0
    # a bracket the GPU kept and the model sent to the fallback (or the reverse: D differs by ~1e-12 between the two): the
    # row is covered by the invariants above, which hold for EVERY row.  A kept row that happens to equal the section row
    # counts as "not new" here.
    differ = int((new != info["kept"]).sum())
    print(f"{name} n_bisect={n_bisect}: {ch} brackets, stats {tuple(h)}, {int(new.sum())} rows not the section rule's, "
          f"max |dw/w| vs converged {worst:.2e}, vs model {worst_m:.2e}, resid error section {e_s:.2e} hybrid {e_h:.2e}, "
          f"kept masks differ from the model's on {differ} rows")
    assert worst < ROOT_RTOL, (name, worst)
    assert e_s == 0.0, (name, e_s)
    assert e_h <= e_s, (name, e_h, e_s)
    assert np.all(prod <= 0.0), (name, prod[prod > 0])
    assert np.array_equal(Th["flag"], Tm["flag"]), (name, f"{differ} rows with different kept masks",
                                                    np.nonzero(Th["flag"] != Tm["flag"])[0])
    assert worst_m < ROOT_RTOL, (name, worst_m, f"{differ} rows with different kept masks")
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "CR_kink", "SFG_flow_kink"])
def test_shallow_refinements_are_the_section_rule(es_ctx, name):
    """n_bisect = 0, 3, 4 need at most one round (17 >= 2^4): R <= S, the same launches, the same table."""
    from eigensolver_amd import _lib
    assert hm.HYBRID_SECTIONS >= 1 and [hm.rounds_for(n) for n in (0, 3, 4, 5)] == [0, 1, 1, 2]
    gp = _problem(es_ctx, name)
    k, W = _grid(name)
    D, st = gp.eval_grid(k, W)
    es_ctx.refine_stats()
    for nb in (0, 3, 4):
        Ts, cs = _search(gp, k, W, D, st, nb, _lib.REFINE_SECTION)
        Th, ch = _search(gp, k, W, D, st, nb, _lib.REFINE_HYBRID)
        assert cs == ch > 0
        _assert_same_table(Th, Ts, what=(name, nb))
    assert tuple(es_ctx.refine_stats()) == (0, 0, 0, 0)
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "SD_w15_kink"])
def test_tiled_grid_gives_the_single_call_table(es_ctx, name):
    from eigensolver_amd import _lib
    gp = _problem(es_ctx, name)
    k, W = _grid(name)
    D, st = gp.eval_grid(k, W)
    whole, n = _search(gp, k, W, D, st, 16, _lib.REFINE_HYBRID)
    parts, off = [], 0
    for rows in (slice(0, 7), slice(7, 24)):
        t, c = _search(gp, k[rows], W, D[rows].contiguous(), st[rows].contiguous(), 16, _lib.REFINE_HYBRID)
        t["row"] = (t["row"] + rows.start).astype(np.int32)
        parts.append(t)
        off += c
    assert off == n > 0
    merged = {c: np.concatenate([p[c] for p in parts]) for c in COLUMNS}
    _assert_same_table(merged, whole, what=name)
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "CR_kink", "SFG_flow_kink"])
def test_async_equals_synchronous(es_ctx, name):
    import torch
    from eigensolver_amd import _lib
    gp = _problem(es_ctx, name)
    k, W = _grid(name)
    D, st = gp.eval_grid(k, W)
    ref, n = _search(gp, k, W, D, st, 16, _lib.REFINE_HYBRID, capacity=1 << 12)
    assert n > 5
    for cap in (2 * n, n, 5):
        count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        es_ctx.refine_stats()
        with rule(es_ctx, _lib.REFINE_HYBRID):
            t = gp.find_roots_async(k, W, D, st, gp.alloc_root_table(cap), count, n_bisect=16, tol_percent=TOL)
        h = es_ctx.refine_stats()
        assert count.item() == n
        m = min(n, cap)
        _assert_same_table(_np(t), ref, n=m, what=(name, cap))
        assert h.brackets == m and h.kept + h.fallback == m
        assert tuple(es_ctx.refine_stats()) == (0, 0, 0, 0)            # a read zeroes the counts
    gp.close()


def test_async_hybrid_has_no_host_synchronisation(es_ctx):
    """As test_mixed_async_gpu.py::test_no_host_synchronisation: the context's stream is held busy for about 0.2 s and the
    hybrid search must return while it still is."""
    import torch
    from eigensolver_amd import _lib
    name = "CR_kink"
    k, W = _grid(name)
    gp0 = _problem(es_ctx, name)
    D, st = gp0.eval_grid(k, W)
    ref, n = _search(gp0, k, W, D, st, 16, _lib.REFINE_HYBRID)
    gp0.close()
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream)
    ctx.refine_rule = _lib.REFINE_HYBRID
    gp = _problem(ctx, name)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        table = gp.alloc_root_table(2 * n)
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        dk, dW = gp._dev(k), gp._dev(W)
    gp.find_roots_async(dk, dW, D, st, table, count, n_bisect=16, tol_percent=TOL)     # warm-up: grows the scratch
    stream.synchronize()
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
    t = gp.find_roots_async(dk, dW, D, st, table, count, n_bisect=16, tol_percent=TOL)
    busy = not stream.query()
    stream.synchronize()
    assert busy, "the stream finished before the call returned: a host synchronisation inside it"
    assert count.item() == n
    _assert_same_table(_np(t), ref, n=n)
    gp.close()
    ctx.close()


@pytest.mark.parametrize("name", ["CR_kink", "SFG_flow_kink"])
def test_mixed_searches_refine_by_the_rule(es_ctx, name):
    import torch
    from eigensolver_amd import _lib
    _, _, _, (lo, hi) = CASES[name]
    k = np.linspace(0.1, 3.5, 40) if name.startswith("S") else np.linspace(0.05, 3.9, 40)
    W = lo + (np.arange(700) + 0.5) * (hi - lo) / 700
    gp = _problem(es_ctx, name)
    D, st = gp.eval_grid(k, W)
    ref, n = _search(gp, k, W, D, st, 24, _lib.REFINE_HYBRID, capacity=1 << 14)
    sec, ns = _search(gp, k, W, D, st, 24, _lib.REFINE_SECTION, capacity=1 << 14)
    assert n == ns > 0 and not _rows_equal(ref, sec).all(), "the hybrid rule kept nothing: the comparison shows nothing"
    with rule(es_ctx, _lib.REFINE_HYBRID):
        tm, nm, _, _, stats = gp.find_roots_mixed(k, W, n_bisect=24, tol_percent=TOL, capacity=1 << 14)
        counts = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        ta, _, _ = gp.find_roots_mixed_async(k, W, gp.alloc_root_table(2 * n), counts, n_bisect=24, tol_percent=TOL)
        torch.cuda.synchronize()
    assert nm == n and stats[2] == 0 and counts.cpu().tolist() == [n, *stats]
    _assert_same_table(_np(tm), ref, what=(name, "mixed"))
    _assert_same_table(_np(ta), ref, n=n, what=(name, "mixed async"))
    gp.close()


def test_refine_stats(es_ctx):
    from eigensolver_amd import _lib
    gp = _problem(es_ctx, "CF_flow_kink")
    k, W = _grid("CF_flow_kink")
    D, st = gp.eval_grid(k, W)
    es_ctx.refine_stats()
    _, n = _search(gp, k, W, D, st, 16, _lib.REFINE_SECTION)
    assert tuple(es_ctx.refine_stats()) == (0, 0, 0, 0)                # the section rule counts nothing
    _search(gp, k, W, D, st, 16, _lib.REFINE_HYBRID)
    _search(gp, k, W, D, st, 16, _lib.REFINE_HYBRID)
    h = es_ctx.refine_stats()
    assert h.brackets == 2 * n and h.kept + h.fallback == h.brackets and h.kept > 0
    assert h.brackets <= h.evaluations <= 8 * h.brackets
    assert tuple(es_ctx.refine_stats()) == (0, 0, 0, 0)
    gp.close()


def test_edges(es_ctx, monkeypatch):
    import torch
    from eigensolver_amd import EsError, _lib
    gp = _problem(es_ctx, "CF_flow_kink")
    k, W = _grid("CF_flow_kink")
    D, st = gp.eval_grid(k, W)
    ref, n = _search(gp, k, W, D, st, 16, _lib.REFINE_HYBRID)
    es_ctx.refine_stats()
    # no bracket at all: D of one sign
    ones, ok = torch.ones_like(D), torch.zeros_like(st)
    t, c = _search(gp, k, W, ones, ok, 16, _lib.REFINE_HYBRID)
    assert c == 0 and len(t["w"]) == 0
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    with rule(es_ctx, _lib.REFINE_HYBRID):
        gp.find_roots_async(k, W, ones, ok, gp.alloc_root_table(64), count, n_bisect=16, tol_percent=TOL)
    assert count.item() == 0 and tuple(es_ctx.refine_stats()) == (0, 0, 0, 0)
    # an empty grid
    with rule(es_ctx, _lib.REFINE_HYBRID):
        t, c = gp.find_roots(k[:0], W, D[:0].contiguous(), st[:0].contiguous(), n_bisect=16, tol_percent=TOL)
        assert c == 0
        gp.find_roots_async(k[:0], W, D[:0].contiguous(), st[:0].contiguous(), gp.alloc_root_table(8), count, n_bisect=16)
    assert count.item() == 0
    # a table of one entry: the first bracket, refined by the rule
    t, c = _search(gp, k, W, D, st, 16, _lib.REFINE_HYBRID, capacity=1)
    assert c == n and len(t["w"]) == 1
    _assert_same_table(t, ref, n=1, what="capacity 1")
    assert es_ctx.refine_stats().brackets == 1
    # the hybrid rule is defined on 17-section only
    monkeypatch.setenv("ES_REFINE_SECTIONS", "9")
    with rule(es_ctx, _lib.REFINE_HYBRID):
        with pytest.raises(EsError, match="unsupported configuration"):
            gp.find_roots(k, W, D, st, n_bisect=16, tol_percent=TOL)
        _, rt = gp.alloc_root_table(64)
        dk, dW = gp._dev(k), gp._dev(W)
        count.fill_(-7)
        rc = es_ctx.lib.es_shoot_find_roots_async(es_ctx.handle, gp.handle, _lib.ptr(dk), dk.numel(), _lib.ptr(dW),
                                                  dW.numel(), 1, _lib.ptr(D), _lib.ptr(st), 16, TOL, C.byref(rt),
                                                  _lib.ptr(count))
        assert rc == 5
        torch.cuda.synchronize()
        assert count.item() == -7                                      # nothing was enqueued
    # ... and the section rule still honours the variable
    t9, c9 = gp.find_roots(k, W, D, st, n_bisect=16, tol_percent=TOL)
    assert c9 == n
    monkeypatch.delenv("ES_REFINE_SECTIONS")
    gp.close()

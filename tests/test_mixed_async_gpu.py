"""es_shoot_find_roots_screened_async / es_shoot_find_roots_mixed_async: the mixed-precision search with its counts in
device memory -- the same D, status and root table, bit for bit, as the synchronous pair es_shoot_screen_grid +
es_shoot_find_roots_screened, the synchronous call's h_count / h_stats in the four count words, and no host
synchronisation."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLUMNS = ("k", "w", "w_lo", "w_hi", "resid", "row", "flag")
N_BISECT = 24


def _grid(name):
    import torch
    from tests import cases
    eq, mode, m, (lo, hi) = cases.all_cases()[name]
    k = np.linspace(0.1, 3.5, 40) if name.startswith("S") else np.linspace(0.05, 3.9, 40)
    nw = 700                                          # ragged: not a multiple of the segment width
    W = lo + (np.arange(nw) + 0.5) * (hi - lo) / nw
    return eq, mode, m, torch.as_tensor(k, device="cuda"), torch.as_tensor(W, device="cuda")


def _bits(t):
    return t.contiguous().cpu().numpy().tobytes()


def _same_records(ta, tb, n):
    for name in COLUMNS:
        assert _bits(ta[name][:n]) == _bits(tb[name][:n]), name


def _sync_screened(gp, dk, dW, D, st, cap, table=None):
    """es_shoot_find_roots_screened called directly: (status, table dict, h_count, h_stats), ES_ERR_SCREENING included."""
    from eigensolver_amd import _lib
    t, rt = table if table is not None else gp.alloc_root_table(cap)
    n = C.c_int(0)
    stats = (C.c_int * 3)()
    rc = gp.ctx.lib.es_shoot_find_roots_screened(gp.ctx.handle, gp.handle, _lib.ptr(dk), dk.numel(), _lib.ptr(dW),
                                                 dW.numel(), 1, N_BISECT, 1e-3, _lib.ptr(D), _lib.ptr(st), C.byref(rt),
                                                 C.byref(n), stats)
    return rc, t, n.value, tuple(stats)


def _counts():
    import torch
    return torch.full((4,), -7, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("name", ["CF_flow_kink", "CR_kink", "CR_sausage", "CDC_w095_kink", "SD_w15_kink", "SFG_flow_kink"])
def test_screened_async_equals_synchronous(es_ctx, name):
    import torch
    from eigensolver_amd import ShootProblem
    eq, mode, m, dk, dW = _grid(name)
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    D0, st0 = gp.screen_grid(dk, dW)
    rc, _, n, _ = _sync_screened(gp, dk, dW, D0.clone(), st0.clone(), 1 << 16)
    assert rc == 0 and n > 5, (rc, n)
    for cap in (2 * n, n, 5):
        Ds, sts, Da, sta = D0.clone(), st0.clone(), D0.clone(), st0.clone()
        rc, ts, hc, hs = _sync_screened(gp, dk, dW, Ds, sts, cap)
        assert rc == (3 if cap < n else 0), rc
        counts = _counts()
        ta = gp.find_roots_screened_async(dk, dW, Da, sta, gp.alloc_root_table(cap), counts, n_bisect=N_BISECT)
        torch.cuda.synchronize()
        assert _bits(Da) == _bits(Ds) and _bits(sta) == _bits(sts)
        assert tuple(counts.cpu().tolist()) == (hc, *hs), (cap, counts, hc, hs)
        assert counts[0].item() == n and counts[2].item() == 2 * min(n, cap)
        _same_records(ts, ta, min(n, cap))
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "SFG_flow_kink"])
def test_mixed_async_equals_mixed(es_ctx, name):
    import torch
    from eigensolver_amd import ShootProblem
    eq, mode, m, dk, dW = _grid(name)
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    rs, n, Ds, sts, stats = gp.find_roots_mixed(dk, dW, n_bisect=N_BISECT, capacity=1 << 16)
    counts = _counts()
    ta, Da, sta = gp.find_roots_mixed_async(dk, dW, gp.alloc_root_table(2 * n), counts, n_bisect=N_BISECT)
    torch.cuda.synchronize()
    assert n > 0 and tuple(counts.cpu().tolist()) == (n, *stats)
    assert _bits(Da) == _bits(Ds) and _bits(sta) == _bits(sts)
    _same_records(rs, ta, n)
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "SD_w15_kink"])
def test_no_unsure_points(es_ctx, name):
    """The unsure bit cleared at every point before the screened call: the synchronous call skips the re-evaluation stage,
    the async call runs it with a device count of 0, and neither touches D or status.  The brackets are then those of the
    fp32 values, so the synchronous call may return 0 or ES_ERR_SCREENING; the async counts[3] is its h_stats[2]."""
    import torch
    from eigensolver_amd import ShootProblem
    eq, mode, m, dk, dW = _grid(name)
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    D0, st0 = gp.screen_grid(dk, dW)
    st0 = st0 & 0x7F
    cap = 1 << 16
    Ds, sts, Da, sta = D0.clone(), st0.clone(), D0.clone(), st0.clone()
    rc, ts, hc, hs = _sync_screened(gp, dk, dW, Ds, sts, cap)
    assert rc == (7 if hs[2] else 0) and 0 < hc <= cap, (rc, hc, hs)
    counts = _counts()
    ta = gp.find_roots_screened_async(dk, dW, Da, sta, gp.alloc_root_table(cap), counts, n_bisect=N_BISECT)
    torch.cuda.synchronize()
    assert _bits(Ds) == _bits(D0) and _bits(sts) == _bits(st0)
    assert _bits(Da) == _bits(Ds) and _bits(sta) == _bits(sts)
    c = tuple(counts.cpu().tolist())
    assert c == (hc, *hs) and c[1] == 0 and c[3] == hs[2], (c, hc, hs)
    _same_records(ts, ta, hc)
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "SD_w15_kink"])
def test_capacity_zero(es_ctx, name):
    """A root table of capacity 0 with null arrays: both calls count the unsure points and the brackets and stop there."""
    import torch
    from eigensolver_amd import ShootProblem, _lib
    eq, mode, m, dk, dW = _grid(name)
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    D0, st0 = gp.screen_grid(dk, dW)
    rc, _, n, stats = _sync_screened(gp, dk, dW, D0.clone(), st0.clone(), 1 << 16)
    assert rc == 0 and n > 0 and stats[0] > 0, (rc, n, stats)
    null = ({}, _lib.RootTable(None, None, None, None, None, None, None, 0))
    Ds, sts, Da, sta = D0.clone(), st0.clone(), D0.clone(), st0.clone()
    rc, _, hc, hs = _sync_screened(gp, dk, dW, Ds, sts, 0, table=null)
    assert rc == 3 and hc == n and hs == (stats[0], 0, 0), (rc, hc, hs)
    counts = _counts()
    gp.find_roots_screened_async(dk, dW, Da, sta, null, counts, n_bisect=N_BISECT)
    torch.cuda.synchronize()
    assert tuple(counts.cpu().tolist()) == (n, stats[0], 0, 0)
    assert _bits(Da) == _bits(Ds) and _bits(sta) == _bits(sts)
    gp.close()


@pytest.mark.parametrize("name", ["CF_flow_kink", "SD_w15_kink"])
def test_eval_points_bounds(es_ctx, name):
    """es_shoot_eval_points on the first n of 513 points, n around the 256 points of a workgroup, with and without d_rel:
    the first n outputs are those of the n = 513 call bit for bit and nothing is written from element n on."""
    import torch
    from tests import cases
    from eigensolver_amd import ShootProblem, _lib
    eq, mode, m, (lo, hi) = cases.all_cases()[name]
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    N, SENT, SENT_ST = 513, -12345.678, 0xA5
    k = np.linspace(0.3, 3.4, N)
    dk = torch.as_tensor(k, device="cuda")
    dw = torch.as_tensor(k * (lo + (np.arange(N) + 0.5) * (hi - lo) / N), device="cuda")

    def call(n, want_rel):
        D = torch.full((N,), SENT, dtype=torch.float64, device="cuda")
        rel = torch.full((N,), SENT, dtype=torch.float64, device="cuda")
        st = torch.full((N,), SENT_ST, dtype=torch.uint8, device="cuda")
        rc = es_ctx.lib.es_shoot_eval_points(es_ctx.handle, gp.handle, _lib.ptr(dk), _lib.ptr(dw), n, _lib.ptr(D),
                                             _lib.ptr(rel) if want_rel else None, _lib.ptr(st))
        assert rc == 0
        torch.cuda.synchronize()
        return D, rel, st

    Df, relf, stf = call(N, True)
    assert (stf == 0).any() and SENT_ST not in stf.cpu().tolist()
    sent_d, sent_st = torch.full((N,), SENT, dtype=torch.float64), torch.full((N,), SENT_ST, dtype=torch.uint8)
    for n in (1, 255, 256, 257, 513):
        for want_rel in (True, False):
            D, rel, st = call(n, want_rel)
            assert _bits(D[:n]) == _bits(Df[:n]) and _bits(st[:n]) == _bits(stf[:n]), (n, want_rel)
            assert _bits(D[n:]) == _bits(sent_d[n:]) and _bits(st[n:]) == _bits(sent_st[n:]), (n, want_rel)
            nr = n if want_rel else 0
            assert _bits(rel[:nr]) == _bits(relf[:nr]) and _bits(rel[nr:]) == _bits(sent_d[nr:]), (n, want_rel)
    gp.close()


def test_no_host_synchronisation(es_ctx):
    """A context on its own stream, that stream held busy for about 0.2 s: the mixed call and the packing of its table
    return while the stream is still busy, and the result is the synchronous one."""
    import torch
    from eigensolver_amd import ShootProblem, _lib, distributed
    eq, mode, m, dk, dW = _grid("CR_kink")
    ref, n, Dr, str_, stats = ShootProblem(eq, mode, m, ctx=es_ctx).find_roots_mixed(dk, dW, n_bisect=N_BISECT,
                                                                                      capacity=1 << 16)
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream)
    gp = ShootProblem(eq, mode, m, ctx=ctx)
    with torch.cuda.stream(stream):
        table = gp.alloc_root_table(2 * n)
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        rows = torch.arange(dk.numel(), dtype=torch.int64, device="cuda")
    xcap = 2 * n
    gp.find_roots_mixed_async(dk, dW, table, counts, n_bisect=N_BISECT)      # warm-up: grows the context's scratch
    distributed.pack_fixed(table[0], counts[0:1], m or 1, rows, xcap, ctx=ctx)
    stream.synchronize()
    # torch.cuda._sleep(cycles) spins on the GPU; calibrate the cycles for about 0.2 s with events
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
    t, D, st = gp.find_roots_mixed_async(dk, dW, table, counts, n_bisect=N_BISECT)
    send = distributed.pack_fixed(t, counts[0:1], m or 1, rows, xcap, ctx=ctx)
    busy = not stream.query()
    stream.synchronize()
    assert busy, "the stream finished before the calls returned: a host synchronisation inside them"
    assert tuple(counts.cpu().tolist()) == (n, *stats)
    assert _bits(D) == _bits(Dr) and _bits(st) == _bits(str_)
    _same_records(ref, t, n)
    assert send[0, 0].item() == n and torch.equal(send[1:n + 1, 1], ref["w"])
    gp.close()
    ctx.close()


def test_screening_violation_is_reported_in_the_counts(es_ctx):
    """One sure point (status 0, unsure bit clear) of a bracket-free stretch of a row with its sign flipped: two brackets
    whose fp64 ends do not confirm them.  The synchronous call returns ES_ERR_SCREENING, the async call ES_SUCCESS with the
    same number in counts[3], and read_screen_counts raises."""
    import torch
    from eigensolver_amd import EsError, ShootProblem
    from eigensolver_amd.shooting import read_screen_counts
    eq, mode, m, dk, dW = _grid("CF_flow_kink")
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    D0, st0 = gp.screen_grid(dk, dW)
    Dm, stm = D0.clone(), st0.clone()
    rc, _, n, _ = _sync_screened(gp, dk, dW, Dm, stm, 1 << 16)
    assert rc == 0
    s0, Dn, sn = st0.cpu().numpy(), Dm.cpu().numpy(), stm.cpu().numpy()
    pick = None
    for r in range(s0.shape[0]):
        for j in range(2, s0.shape[1] - 2):
            if (s0[r, j - 1:j + 2] == 0).all() and (sn[r, j - 2:j + 3] == 0).all() and \
                    len(set(np.signbit(Dn[r, j - 2:j + 3]).tolist())) == 1 and Dn[r, j] != 0.0:
                pick = (r, j)
                break
        if pick:
            break
    assert pick is not None
    D0[pick] = -D0[pick]
    Ds, sts, Da, sta = D0.clone(), st0.clone(), D0.clone(), st0.clone()
    rc, ts, hc, hs = _sync_screened(gp, dk, dW, Ds, sts, 1 << 16)
    assert rc == 7 and hs[2] > 0 and hc == n + 2, (rc, hs, hc, n)
    counts = _counts()
    ta = gp.find_roots_screened_async(dk, dW, Da, sta, gp.alloc_root_table(1 << 16), counts, n_bisect=N_BISECT)
    torch.cuda.synchronize()
    assert tuple(counts.cpu().tolist()) == (hc, *hs)
    _same_records(ts, ta, hc)
    with pytest.raises(EsError, match="not confirmed in fp64"):
        read_screen_counts(counts, 1 << 16)
    gp.close()


def test_pipelined_lanes(es_ctx):
    """Two contexts on two streams take alternate steps of one problem, all enqueued from this thread."""
    import torch
    from eigensolver_amd import ShootProblem, _lib
    from eigensolver_amd.shooting import read_screen_counts
    eq, mode, m, dk, dW = _grid("CR_sausage")
    ref, n, Dr, str_, stats = ShootProblem(eq, mode, m, ctx=es_ctx).find_roots_mixed(dk, dW, n_bisect=N_BISECT,
                                                                                      capacity=1 << 16)
    torch.cuda.synchronize()
    lanes = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        ctx = _lib.Context(0, stream=stream)
        with torch.cuda.stream(stream):
            gp = ShootProblem(eq, mode, m, ctx=ctx)
            lanes.append(dict(stream=stream, ctx=ctx, gp=gp, table=gp.alloc_root_table(2 * n),
                              counts=torch.zeros(4, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    grids = []
    for step in range(4):
        ln = lanes[step % 2]
        _, D, st = ln["gp"].find_roots_mixed_async(dk, dW, ln["table"], ln["counts"], n_bisect=N_BISECT)
        grids.append((D, st))
    torch.cuda.synchronize()
    for D, st in grids:
        assert _bits(D) == _bits(Dr) and _bits(st) == _bits(str_)
    for ln in lanes:
        c = read_screen_counts(ln["counts"], 2 * n)
        assert (c.count, c.unsure, c.ends, c.violations, c.overflow) == (n, *stats, False)
        _same_records(ref, ln["table"][0], n)
        ln["gp"].close()
        ln["ctx"].close()


def _raw_call(fn, ctx, prob, dk, dW, w_mode, D, st, rt, counts):
    from eigensolver_amd import _lib
    return fn(ctx, prob, _lib.ptr(dk), dk.numel(), _lib.ptr(dW), dW.numel(), w_mode, N_BISECT, 1e-3, _lib.ptr(D),
              _lib.ptr(st), C.byref(rt), _lib.ptr(counts) if counts is not None else None)


def test_edges(es_ctx, monkeypatch):
    import torch
    from eigensolver_amd import ShootProblem, equilibrium as q
    eq, mode, m, dk, dW = _grid("CF_flow_kink")
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    lib, h = es_ctx.lib, es_ctx.handle
    # nk = 0 zeroes the four words
    counts = _counts()
    gp.find_roots_mixed_async(torch.zeros(0, dtype=torch.float64, device="cuda"), dW, gp.alloc_root_table(16), counts)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [0, 0, 0, 0]
    _, rt = gp.alloc_root_table(16)
    D = torch.empty((dk.numel(), dW.numel()), dtype=torch.float64, device="cuda")
    st = torch.empty((dk.numel(), dW.numel()), dtype=torch.uint8, device="cuda")
    counts = _counts()
    for fn in (lib.es_shoot_find_roots_screened_async, lib.es_shoot_find_roots_mixed_async):
        assert _raw_call(fn, h, gp.handle, dk, dW, 1, D, st, rt, None) == 1           # null d_counts
        assert _raw_call(fn, h, gp.handle, dk, dW, 5, D, st, rt, counts) == 1         # bad w_mode
        assert _raw_call(fn, None, gp.handle, dk, dW, 1, D, st, rt, counts) == 1      # null context
    gp.close()
    # a slab whose continuum flag needs per-node sign tracking: ES_ERR_UNSUPPORTED at once, nothing enqueued
    monkeypatch.setenv("ES_FORCE_SIGN_TRACKING", "1")
    gs = ShootProblem(q.SlabFlow(U_i0=0.35, width=1.5), "kink", ctx=es_ctx)
    monkeypatch.delenv("ES_FORCE_SIGN_TRACKING")
    for fn in (lib.es_shoot_find_roots_screened_async, lib.es_shoot_find_roots_mixed_async):
        assert _raw_call(fn, h, gs.handle, dk, dW, 1, D, st, rt, counts) == 5
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [-7] * 4
    gs.close()

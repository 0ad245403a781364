"""GPU timing aid: a dispersion diagram on 4096 wavenumbers by Newton tracing from a coarse scan (ShootProblem.trace_branches,
es_shoot_newton) against the route without it, marching and bracketing the whole fine grid, on one device.

Problem: the headline of bench.py (Gaussian flow cylinder, N = 1000 nodes, kink), its 4096 wavenumbers and its 4096 phase
speeds.  The coarse scan -- every --stride-th row (default 64: 65 rows) of that grid through eval_grid, find_roots,
label_roots and root_slopes into postprocess.curves_with_slopes -- is done once, before anything is timed.  Legs, each between
two device events on the context's stream, alternating repeat by repeat in one process so that drift hits all alike:

    trace         ShootProblem.trace_branches(curves, the 4096 k): host indexing, one pinned upload, the Hermite prediction in
                  torch, ONE es_shoot_newton over every branch and one es_shoot_mode_signature over the traced roots
    newton        es_shoot_newton alone on the same guesses, buffers allocated beforehand
    slopes        ONE es_shoot_root_slopes on the same pairs: the cost of one jet march, not a target
    grid_search   the route of a user without the call: eval_grid on the 4096 x 4096 grid and find_roots_async on it

Before timing, every flagged traced root is matched with the nearest root of grid_search in its row.  One JSON line with
median / min / max ms per leg over the repeats, the ratios and the match is printed and appended to --out.

    python tools/time_branch_tracing.py [--repeats 20] [--warmup 3] [--stride 64] [--out profiles/branch_tracing_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stride", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_tracing_timing.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import numpy as np
    import torch
    import bench
    from eigensolver_amd import ShootProblem, _lib
    from eigensolver_amd import postprocess as pp
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    kg, Wg = bench.workload_grid()
    rows = np.unique(np.concatenate([np.arange(0, len(kg), a.stride), [len(kg) - 1]]))
    with torch.cuda.stream(stream):
        gp = ShootProblem(bench.workload_equilibrium(), "kink", ctx=ctx)
        N = int(gp.desc.n_nodes)
        # the coarse scan
        D, st = gp.eval_grid(kg[rows], Wg)
        roots, cnt = gp.find_roots(kg[rows], Wg, D, st, n_bisect=bench.N_BISECT)
        curves = pp.curves_with_slopes(roots, gp.label_roots(roots), gp.root_slopes(roots["k"], roots["w"]))
        del D, st
        traced = gp.trace_branches(curves, kg)
        stream.synchronize()
        tk = torch.cat([b["k"] for b in traced.branches.values()]).contiguous()
        guess = torch.cat([b["predicted"] for b in traced.branches.values()]).contiguous()
        tw = torch.cat([b["w"] for b in traced.branches.values()]).contiguous()
        flag = torch.cat([b["flag"] for b in traced.branches.values()])
        iters = torch.cat([b["iters"] for b in traced.branches.values()])
        n = int(tk.numel())
        dkg, dWg = gp._dev(kg), gp._dev(Wg)
        table = gp.alloc_root_table(1 << 18)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        w, resid, dwdk = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        it_out, fl_out = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        st_out = torch.empty(n, dtype=torch.uint8, device=dev)
        outer, inner = (torch.empty((3, n), dtype=torch.float64, device=dev) for _ in range(2))
    lib, P, dmax = ctx.lib, _lib.ptr, sys.float_info.max

    def trace():
        gp.trace_branches(curves, kg)

    def newton():
        _lib.check(ctx.handle, lib.es_shoot_newton(ctx.handle, gp.handle, P(tk), P(guess), n, None, 8, dmax, dmax, 1e-3, P(w),
                                                   P(resid), P(dwdk), P(it_out), P(fl_out), P(st_out)))

    def slopes():
        _lib.check(ctx.handle, lib.es_shoot_root_slopes(ctx.handle, gp.handle, P(tk), P(tw), n, None, P(outer), P(inner), P(st_out)))

    def grid_search():
        Dg, sg = gp.eval_grid(dkg, dWg)
        gp.find_roots_async(dkg, dWg, Dg, sg, table, count, n_bisect=bench.N_BISECT)

    legs = {"trace": trace, "newton": newton, "slopes": slopes, "grid_search": grid_search}
    # every flagged traced root against the nearest root the grid search accepts in its row
    with torch.cuda.stream(stream):
        newton()
        grid_search()
    stream.synchronize()
    assert torch.equal(w, tw), "es_shoot_newton alone gives what trace_branches gave"
    nb = int(count.item())
    assert 0 < nb <= table[1].capacity
    acc = (table[0]["flag"][:nb] == 1).cpu().numpy()
    gw, grow = table[0]["w"][:nb].cpu().numpy()[acc], table[0]["row"][:nb].cpu().numpy()[acc]
    fl, twh = flag.cpu().numpy() == 1, tw.cpu().numpy()
    trow = np.searchsorted(kg, tk.cpu().numpy())
    by_row = {}
    for r, x in zip(grow.tolist(), gw.tolist()):
        by_row.setdefault(r, []).append(x)
    dist = np.array([min((abs(x - y) for y in by_row.get(int(r), [])), default=np.inf) / max(1.0, abs(x))
                     for r, x in zip(trow[fl], twh[fl])])
    matched = dist <= 1e-10
    ms = {name: [] for name in legs}
    for it in range(a.warmup + a.repeats):
        for name, run in legs.items():
            with torch.cuda.stream(stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    itc = iters.cpu().numpy()
    line = {"device": torch.cuda.get_device_name(dev), "nodes": N, "fine_rows": len(kg), "coarse_rows": len(rows),
            "phase_speeds": len(Wg), "coarse_roots": int(cnt), "branches_traced": len(traced.branches),
            "labels_skipped": [list(s) for s in traced.skipped], "fine_points": n, "flagged": int(fl.sum()),
            "newton_steps_mean": round(float(itc.mean()), 2), "newton_steps_max": int(itc.max()),
            "grid_search_brackets": nb, "grid_search_accepted": int(acc.sum()),
            "flagged_matched_within_1e-10": int(matched.sum()),
            "worst_matched_distance": float(dist[matched].max()) if matched.any() else None,
            "repeats": a.repeats, "warmup": a.warmup, "legs": {}}
    for name, v in ms.items():
        line["legs"][name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line["trace_over_grid_search"] = round(med["trace"] / med["grid_search"], 4)
    line["newton_over_slopes"] = round(med["newton"] / med["slopes"], 2)
    line["trace_over_newton"] = round(med["trace"] / med["newton"], 2)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    gp.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

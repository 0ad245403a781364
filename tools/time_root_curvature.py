"""GPU timing aid: the dispersion curvature (es_shoot_root_curvature, es_shoot_cg_extrema) against the routes it replaces, on
one device.  Problem: the headline of bench.py (Gaussian flow cylinder, N = 1000 nodes, kink).

(a) Pairs: the accepted roots of ONE pass of the headline grid (the mixed-precision search), tiled up to n = 2^17.  Legs:

    curvature     es_shoot_root_curvature: value, both first and the three second derivatives of both sides in one march of
                  6-component jets, 97 bytes per pair
    slopes        es_shoot_root_slopes on the same pairs: the 3-component march, the scale of the call
    difference    the route without the call: es_shoot_newton at k (1 + h) and k (1 - h), h = 1e-3, from the tangent of the
                  root, two es_shoot_root_slopes calls at the re-solved roots and the central difference of their c_g in torch

(b) The longest branch of the headline diagram traced on its 4096 wavenumbers (trace_branches from every 64th row).  Legs:

    extrema       ShootProblem.group_speed_extrema(branch): one es_shoot_root_curvature over the branch, the selection of the
                  sign changes in torch, one es_shoot_cg_extrema over them; nothing is read back
    trace_host    the route without the call: trace_branches again (the dwdk of its Newton launch), k, dwdk and flag of the
                  branch read to the host, the sign changes of the difference of c_g located there (to the k grid only)

Each leg runs between two device events on the context's stream (trace_host: plus the host work, timed by the wall clock after
a stream synchronisation), the legs alternate repeat by repeat in one process so that drift hits all alike, and every buffer of
(a) is allocated before anything is timed.  Before timing, the curvature of (a) is compared with the difference route.  One
JSON line with median / min / max ms per leg over the repeats and the ratios is printed and appended to --out.

    python tools/time_root_curvature.py [--repeats 20] [--warmup 3] [--log2n 17] [--out profiles/root_curvature_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=17)
    ap.add_argument("--stride", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "root_curvature_timing.jsonl"))
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
    n = 1 << a.log2n
    kg, Wg = bench.workload_grid()
    rows = np.unique(np.concatenate([np.arange(0, len(kg), a.stride), [len(kg) - 1]]))
    with torch.cuda.stream(stream):
        gp = ShootProblem(bench.workload_equilibrium(), "kink", ctx=ctx)
        N = int(gp.desc.n_nodes)
        roots, cnt = gp.find_roots_mixed(kg, Wg, n_bisect=bench.N_BISECT)[:2]
        acc = roots["flag"] == 1
        rk, rw = roots["k"][acc], roots["w"][acc]
        n_roots = int(rk.numel())
        assert n_roots > 0
        reps = (n + n_roots - 1) // n_roots
        dk, dw = rk.repeat(reps)[:n].contiguous(), rw.repeat(reps)[:n].contiguous()
        del roots
        outer6, inner6 = (torch.empty((6, n), dtype=torch.float64, device=dev) for _ in range(2))
        outer3, inner3 = (torch.empty((3, n), dtype=torch.float64, device=dev) for _ in range(2))
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        # the difference route: both neighbours in one array of 2 n
        cg0 = gp.root_slopes(dk, dw).group_velocity
        k2 = torch.cat([dk * (1.0 + H), dk * (1.0 - H)]).contiguous()
        g2 = torch.cat([dw + cg0 * dk * H, dw - cg0 * dk * H]).contiguous()
        w2, resid2, dwdk2 = (torch.empty(2 * n, dtype=torch.float64, device=dev) for _ in range(3))
        it2, fl2 = (torch.empty(2 * n, dtype=torch.int32, device=dev) for _ in range(2))
        st2 = torch.empty(2 * n, dtype=torch.uint8, device=dev)
        o2, i2 = (torch.empty((2, 3, n), dtype=torch.float64, device=dev) for _ in range(2))
        # (b) the coarse scan and the trace
        D, sg = gp.eval_grid(kg[rows], Wg)
        coarse, _ = gp.find_roots(kg[rows], Wg, D, sg, n_bisect=bench.N_BISECT)
        curves = pp.curves_with_slopes(coarse, gp.label_roots(coarse), gp.root_slopes(coarse["k"], coarse["w"]))
        del D, sg
        traced = gp.trace_branches(curves, kg)
        stream.synchronize()
        label = max(traced.branches, key=lambda lab: int((traced.branches[lab]["flag"] == 1).sum().item()))
        branch = traced.branches[label]
    lib, P, dmax = ctx.lib, _lib.ptr, sys.float_info.max
    q_diff = [None]

    def curvature():
        _lib.check(ctx.handle, lib.es_shoot_root_curvature(ctx.handle, gp.handle, P(dk), P(dw), n, None, P(outer6), P(inner6), P(st)))

    def slopes():
        _lib.check(ctx.handle, lib.es_shoot_root_slopes(ctx.handle, gp.handle, P(dk), P(dw), n, None, P(outer3), P(inner3), P(st)))

    def difference():
        _lib.check(ctx.handle, lib.es_shoot_newton(ctx.handle, gp.handle, P(k2), P(g2), 2 * n, None, 8, dmax, dmax, 1e-3, P(w2),
                                                   P(resid2), P(dwdk2), P(it2), P(fl2), P(st2)))
        for half in (0, 1):
            _lib.check(ctx.handle, lib.es_shoot_root_slopes(ctx.handle, gp.handle, P(k2[half * n:]), P(w2[half * n:]), n, None,
                                                            P(o2[half]), P(i2[half]), P(st2[half * n:])))
        d = o2 - i2
        cg = -d[:, 2] / d[:, 1]
        q_diff[0] = (cg[0] - cg[1]) / (2.0 * H * dk)

    def extrema():
        return gp.group_speed_extrema(branch)

    def host_extrema(b):
        k, cg, fl = (b[f].cpu().numpy() for f in ("k", "dwdk", "flag"))
        k, cg = k[fl == 1], cg[fl == 1]
        s = np.diff(cg) / np.diff(k)
        return k[1:-1][np.flatnonzero(s[:-1] * s[1:] < 0)]

    def trace_host():
        return host_extrema(gp.trace_branches(curves, kg).branches[label])

    with torch.cuda.stream(stream):
        curvature()
        difference()
        x = extrema()
        kh = trace_host()
        d6 = outer6 - inner6
        cg = -d6[2] / d6[1]
        q = -(d6[5] + 2.0 * d6[4] * cg + d6[3] * cg * cg) / d6[1]
        ok = (st == 0) & torch.isfinite(q) & torch.isfinite(q_diff[0]) & (fl2[:n] == 1) & (fl2[n:] == 1)
        dq = ((q - q_diff[0]).abs() / q.abs().clamp(min=1.0))[ok]
        q_vs_difference = (float(dq.median().item()), float(dq.max().item()))
        n_ext = int(x["count"].item())
        k_ext = x["k"][:n_ext].cpu().numpy()
    legs = {"curvature": curvature, "slopes": slopes, "difference": difference, "extrema": extrema, "trace_host": trace_host}
    ms = {name: [] for name in legs}
    for it in range(a.warmup + a.repeats):
        for name, run in legs.items():
            stream.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
            e1.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                ms[name].append(wall if name == "trace_host" else e0.elapsed_time(e1))
    line = {"device": torch.cuda.get_device_name(dev), "pairs": n, "nodes": N, "distinct_roots": n_roots, "brackets": int(cnt),
            "pairs_compared": int(ok.sum().item()), "difference_step": H, "curvature_vs_difference_median": q_vs_difference[0],
            "curvature_vs_difference_max": q_vs_difference[1], "branch": list(label), "branch_points": int(branch["k"].numel()),
            "extrema": n_ext, "extrema_flagged": int((x["flag"][:n_ext] == 1).sum().item()), "k_extrema": k_ext.tolist(),
            "k_extrema_host_difference": kh.tolist(), "repeats": a.repeats, "warmup": a.warmup, "legs": {}}
    for name, v in ms.items():
        line["legs"][name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line["curvature_over_slopes"] = round(med["curvature"] / med["slopes"], 3)
    line["curvature_over_difference"] = round(med["curvature"] / med["difference"], 3)
    line["extrema_over_trace_host"] = round(med["extrema"] / med["trace_host"], 3)
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

"""GPU timing aid: the dispersion slopes of a root table (es_shoot_root_slopes) against the difference stencil a user could run
without the call, and against one determinant evaluation of the same pairs, on one device.

Pairs: the accepted roots of ONE pass of the headline grid (bench.py: Gaussian flow cylinder, N = 1000 nodes, 4096 x 4096
points, the mixed-precision search), tiled up to n = 2^17.  Legs, each between two device events on the context's stream,
alternating repeat by repeat in one process so that drift hits all alike, every buffer allocated before anything is timed:

    slopes        es_shoot_root_slopes: value, d/d omega and d/dk of both sides in one march of 3-component jets, 49 bytes
                  per pair
    stencil       ONE es_shoot_eval_points on 9 n pairs: the centre and a 5-point stencil in omega and in k at relative step
                  2^-10 -- nine marches per root, and wrong at a root beside a pole of the exterior term
    eval_points   ONE es_shoot_eval_points on the n pairs -- the scale of the call, not a target

Before timing, D of the slopes leg is compared with D of eval_points on all n pairs, and the group speed of the slopes leg
with the one the stencil gives.  One JSON line with median / min / max ms per leg over the repeats and the ratios is printed and
appended to --out.

--lib: another build of the library (an earlier commit's, to time both in one visit in processes that take turns).

    python tools/time_root_slopes.py [--repeats 20] [--warmup 3] [--log2n 17] [--lib PATH] [--out profiles/root_slopes_timing.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP = 2.0 ** -10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=17)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "root_slopes_timing.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import torch
    import bench
    from eigensolver_amd import ShootProblem, _lib
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    other = None
    if a.lib:
        other = ctypes.CDLL(a.lib)
        _lib._sig(other)
    ctx = _lib.Context(dev.index or 0, stream=stream, lib=other)
    n = 1 << a.log2n
    with torch.cuda.stream(stream):
        gp = ShootProblem(bench.workload_equilibrium(), "kink", ctx=ctx)
        N = int(gp.desc.n_nodes)
        kg, Wg = bench.workload_grid()
        roots, cnt = gp.find_roots_mixed(kg, Wg, n_bisect=bench.N_BISECT)[:2]
        acc = roots["flag"] == 1
        rk, rw = roots["k"][acc], roots["w"][acc]
        n_roots = int(rk.numel())
        assert n_roots > 0
        reps = (n + n_roots - 1) // n_roots
        dk, dw = rk.repeat(reps)[:n].contiguous(), rw.repeat(reps)[:n].contiguous()
        del roots
        # the stencil: centre, omega (1 +- s), omega (1 +- 2 s), k (1 +- s), k (1 +- 2 s)
        fk = torch.tensor([0, 0, 0, 0, 0, 1, -1, 2, -2], dtype=torch.float64, device=dev)[:, None] * STEP
        fw = torch.tensor([0, 1, -1, 2, -2, 0, 0, 0, 0], dtype=torch.float64, device=dev)[:, None] * STEP
        dk9 = (dk[None, :] * (1.0 + fk)).reshape(-1).contiguous()
        dw9 = (dw[None, :] * (1.0 + fw)).reshape(-1).contiguous()
        outer = torch.empty((3, n), dtype=torch.float64, device=dev)
        inner = torch.empty((3, n), dtype=torch.float64, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        D9 = torch.empty(9 * n, dtype=torch.float64, device=dev)
        st9 = torch.empty(9 * n, dtype=torch.uint8, device=dev)
        D = torch.empty(n, dtype=torch.float64, device=dev)
        st_pts = torch.empty(n, dtype=torch.uint8, device=dev)
    lib, P = ctx.lib, _lib.ptr

    def slopes():
        _lib.check(ctx.handle, lib.es_shoot_root_slopes(ctx.handle, gp.handle, P(dk), P(dw), n, None, P(outer), P(inner), P(st)))

    def stencil():
        _lib.check(ctx.handle, lib.es_shoot_eval_points(ctx.handle, gp.handle, P(dk9), P(dw9), 9 * n, P(D9), None, P(st9)))

    def eval_points():
        _lib.check(ctx.handle, lib.es_shoot_eval_points(ctx.handle, gp.handle, P(dk), P(dw), n, P(D), None, P(st_pts)))

    legs = {"slopes": slopes, "stencil": stencil, "eval_points": eval_points}
    with torch.cuda.stream(stream):
        slopes()
        stencil()
        eval_points()
        ok = (st == 0) & torch.isfinite(D)
        d = outer - inner
        scale = torch.maximum(outer[0].abs(), inner[0].abs())
        value_err = float(((d[0] - D).abs() / scale)[ok].max().item())
        S9 = D9.reshape(9, n)
        Dw = (8.0 * (S9[1] - S9[2]) - (S9[3] - S9[4])) / (12.0 * STEP * dw)
        Dk = (8.0 * (S9[5] - S9[6]) - (S9[7] - S9[8])) / (12.0 * STEP * dk)
        cg, cg9 = -d[2] / d[1], -Dk / Dw
        both = ok & torch.isfinite(cg9)
        cg_diff = ((cg - cg9).abs() / cg.abs().clamp(min=1.0))[both]
        cg_diff_median, cg_diff_max = float(cg_diff.median().item()), float(cg_diff.max().item())
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
    line = {"device": torch.cuda.get_device_name(dev), "lib": os.path.basename(a.lib) if a.lib else "default", "pairs": n, "nodes": N, "distinct_roots": n_roots, "brackets": int(cnt),
            "pairs_ok": int(ok.sum().item()), "value_vs_eval_points": value_err, "stencil_step": STEP,
            "cg_vs_stencil_median": cg_diff_median, "cg_vs_stencil_max": cg_diff_max,
            "repeats": a.repeats, "warmup": a.warmup, "legs": {}}
    for name, v in ms.items():
        line["legs"][name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line["slopes_over_stencil"] = round(med["slopes"] / med["stencil"], 3)
    line["slopes_over_eval_points"] = round(med["slopes"] / med["eval_points"], 2)
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

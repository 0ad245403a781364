"""GPU timing aid: the root search of the closed-form uniform cylinder (es_cyl_uniform_find_roots_async) against the grid
evaluation it contains (es_cyl_uniform_eval), on one device.

Grid: n x n (default 4096 x 4096), coronal kink m = 1, k = linspace(0.01, 4, n), W = 0.9 + (j + 0.5) (4.95 - 0.9) / n (the
full-size grid of tests/test_cyl_uniform_gpu.py::test_uniform_edge_cases), phase-speed mode.  Four legs, each between two
device events on the context's stream, alternating repeat by repeat in one process so that drift hits all alike:

    eval          es_cyl_uniform_eval alone (D and status stored: 9 B per point)
    search        find_roots_async with d_D = d_status = NULL (bracket masks only)
    search_grid   find_roots_async with the grid stored
    flag_only     find_roots_async with d_D = d_status = NULL and a table of capacity 0: the fused evaluate-and-flag kernel
                  and the scan, nothing emitted or refined -- search minus flag_only is the refinement share of `search`

Per leg one JSON line: median / min / max ms over the repeats and det-evals/s (grid points per second of the median); the
search legs add brackets, accepted roots and roots/s.  A last line compares flag_only with eval: the fused kernel writes
1/64 of the bytes and evaluates 1/63 more points, so it should not exceed eval by more than eval's own min-to-max spread.

    python tools/time_cyl_uniform_roots.py [--n 4096] [--repeats 20] [--warmup 3] [--n-bisect 40]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-bisect", type=int, default=40)
    ap.add_argument("--tol-percent", type=float, default=1e-3)
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import numpy as np
    import torch
    from eigensolver_amd import CylinderUniform, _lib
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    n = a.n
    with torch.cuda.stream(stream):
        cu = CylinderUniform(mode="kink", m=1, ctx=ctx)
        k = torch.as_tensor(np.linspace(0.01, 4.0, n), dtype=torch.float64, device=dev)
        W = torch.as_tensor(0.9 + (np.arange(n) + 0.5) * (4.95 - 0.9) / n, dtype=torch.float64, device=dev)
        D = torch.empty((1, n, n), dtype=torch.float64, device=dev)
        st = torch.empty((1, n, n), dtype=torch.uint8, device=dev)
        # size the table for the data: about twice the count (one synchronous search; it also grows the scan scratch)
        t0, brackets = cu.find_roots(k, W, n_bisect=a.n_bisect, tol_percent=a.tol_percent)
        accepted = int(t0["flag"].sum().item())
        cap = 1024
        while cap < 2 * brackets:
            cap *= 2
        table, empty = cu.alloc_root_table(cap), cu.alloc_root_table(0)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(n_bisect=a.n_bisect, tol_percent=a.tol_percent)
    legs = {
        "eval": lambda: cu.ctx.lib.es_cyl_uniform_eval(ctx.handle, ctypes.byref(cu.params), _lib.ptr(k), n, _lib.ptr(W), n, 1,
                                                       _lib.ptr(D), None, _lib.ptr(st)),
        "search": lambda: cu.find_roots_async(k, W, table, count, **kw),
        "search_grid": lambda: cu.find_roots_async(k, W, table, count, D=D, status=st, **kw),
        "flag_only": lambda: cu.find_roots_async(k, W, empty, count, **kw),
    }
    ms = {name: [] for name in legs}
    for it in range(a.warmup + a.repeats):
        for name, run in legs.items():
            with torch.cuda.stream(stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = run()
                e1.record(stream)
            e1.synchronize()
            assert not isinstance(rc, int) or rc == 0, (name, rc)
            if name != "eval":
                assert int(count.item()) == brackets, (name, int(count.item()), brackets)
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    points = n * n
    res = {}
    for name, v in ms.items():
        med, lo, hi = statistics.median(v), min(v), max(v)
        res[name] = (med, lo, hi)
        line = {"leg": name, "grid": [n, n], "order": 1, "n_bisect": a.n_bisect, "repeats": len(v),
                "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                "det_evals_per_s": round(points / (med * 1e-3), 1)}
        if name in ("search", "search_grid"):
            line.update(brackets=brackets, accepted_roots=accepted, table_capacity=cap,
                        roots_per_s=round(accepted / (med * 1e-3), 1))
        print(json.dumps(line), flush=True)
    spread = res["eval"][2] - res["eval"][1]
    excess = res["flag_only"][0] - res["eval"][0]
    print(json.dumps({"refinement_share_ms": round(res["search"][0] - res["flag_only"][0], 4),
                      "flag_only_minus_eval_ms": round(excess, 4), "eval_spread_ms": round(spread, 4),
                      "flag_only_over_eval": round(res["flag_only"][0] / res["eval"][0], 4),
                      "verdict": "within the spread of eval" if excess <= spread else "slower than eval by more than its spread"}),
          flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

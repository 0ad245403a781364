"""GPU timing aid: the SEARCH stage of the four bench.py workloads under the two refinement rules of a context,
ES_REFINE_SECTION (the default) and ES_REFINE_HYBRID (include/eigensolver_amd.h).

The problems and grids are bench.py's own (workload_units, workload_equilibrium / workload_grid); configs[4] is also timed
on rank 0's tile of an E-GPU run, E = 1 and 8.  Per unit the grid values are computed ONCE (es_shoot_eval_grid, or the fp32
screening march for configs[4]); what is timed is es_shoot_find_roots_async (configs[1] - [3]) or
es_shoot_find_roots_screened_async (configs[4]) of every unit of the workload, one after the other on one stream, between
two device events.  The two rules alternate repeat by repeat in one process, so drift of the device hits both alike.

Per workload and rule one JSON line: median / min / max ms over the repeats, brackets, Context.refine_stats summed over
the units of one repeat, and marches per bracket = 16 S + h[3] / h[0] + (16 (R - S) + 2) h[2] / h[0] (16 R + 2 for the
section rule).  A last line per workload gives the verdict: the rules differ only if the medians differ by more than the
larger min-to-max spread of the two.  The row, k and count columns and every row the hybrid rule did not keep must equal the
section rule's (asserted).

Every workload runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python tools/time_refine_rules.py [--repeats 20] [--warmup 3] [--workloads config1,config2,config3,config4,config4/8]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("config1", "config2", "config3", "config4", "config4/8")
CHILD_TIMEOUT_S = 420
SECTIONS, HYBRID_SECTIONS = 17, 1          # kRefineSections, kHybridSections of es_refine.hip


def rounds_for(n_bisect):
    rounds, span = 0, 1.0
    while span < 2.0 ** n_bisect:
        span *= SECTIONS
        rounds += 1
    return rounds


def make_units(name, dev, ctx):
    import numpy as np
    import torch
    import bench
    from eigensolver_amd import ShootProblem
    from eigensolver_amd import distributed as D
    base, _, E = name.partition("/")
    E = int(E) if E else 1
    if base == "config3":
        k_np, W_np = bench.workload_grid()
        units = [("kink", 0, bench.workload_equilibrium(), "kink", None, k_np, W_np)]
    else:
        _, units = bench.workload_units(base)
    out = []
    for label, _, eq, mode, m, k_np, W_np in units:
        rows = D.tile_rows(len(k_np), 0, E, strided=True) if E > 1 else np.arange(len(k_np))
        k = torch.as_tensor(k_np[rows], dtype=torch.float64, device=dev)
        W = torch.as_tensor(W_np, dtype=torch.float64, device=dev)
        prob = ShootProblem(eq, mode, m=m, ctx=ctx)
        mixed = base == "config4"
        Dg, st = prob.screen_grid(k, W) if mixed else prob.eval_grid(k, W)
        D0, st0 = Dg.clone(), st.clone()
        if mixed:                                      # the screened search rewrites the unsure points: work on a copy
            _, nbr, _, _, _ = prob.find_roots_screened(k, W, Dg, st, n_bisect=bench.N_BISECT, tol_percent=bench.TOL_PERCENT,
                                                       capacity=1 << 18)
        else:
            _, nbr = prob.find_roots(k, W, Dg, st, n_bisect=bench.N_BISECT, tol_percent=bench.TOL_PERCENT, capacity=1 << 18)
        assert nbr <= 1 << 18, (label, nbr)
        cap = 1024
        while cap < 2 * nbr:
            cap *= 2
        out.append({"label": label, "prob": prob, "k": k, "W": W, "D0": D0, "st0": st0, "D": Dg, "st": st, "mixed": mixed,
                    "table": prob.alloc_root_table(cap), "cap": cap, "brackets": nbr,
                    "counts": torch.zeros(4, dtype=torch.int32, device=dev)})
    torch.cuda.synchronize()
    return out


def one_repeat(units, stream):
    """Every unit's search once, enqueued on the context's stream; -> ms between the device events around them."""
    import torch
    import bench
    with torch.cuda.stream(stream):
        for u in units:
            u["D"].copy_(u["D0"])
            u["st"].copy_(u["st0"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for u in units:
            if u["mixed"]:
                u["prob"].find_roots_screened_async(u["k"], u["W"], u["D"], u["st"], u["table"], u["counts"],
                                                    n_bisect=bench.N_BISECT, tol_percent=bench.TOL_PERCENT)
            else:
                u["prob"].find_roots_async(u["k"], u["W"], u["D"], u["st"], u["table"], u["counts"][0:1],
                                           n_bisect=bench.N_BISECT, tol_percent=bench.TOL_PERCENT)
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def child(name, repeats, warmup):
    import statistics
    import torch
    import bench
    from eigensolver_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    with torch.cuda.stream(stream):
        units = make_units(name, dev, ctx)
    rules = (("section", _lib.REFINE_SECTION), ("hybrid", _lib.REFINE_HYBRID))
    ms = {r: [] for r, _ in rules}
    stats, tables = {}, {}
    ctx.refine_stats()
    for it in range(warmup + repeats):
        for rname, rule in rules:
            ctx.refine_rule = rule
            t = one_repeat(units, stream)
            h = ctx.refine_stats()
            if it >= warmup:
                ms[rname].append(t)
            stats[rname] = h
            if it == 0:
                tables[rname] = [{c: v[:u["brackets"]].clone() for c, v in u["table"][0].items()} for u in units]
    ctx.refine_rule = _lib.REFINE_SECTION
    # the guaranteed part of the hybrid rule, on the full-size tables
    kept = 0
    for ts, th, u in zip(tables["section"], tables["hybrid"], units):
        for c in ("row", "k"):
            assert torch.equal(ts[c], th[c]), (name, u["label"], c)
        assert bool((th["flag"] >= ts["flag"]).all()), (name, u["label"])
        same = torch.ones_like(ts["flag"], dtype=torch.bool)
        for c in ("w", "w_lo", "w_hi", "resid", "flag"):
            same &= ts[c].view(torch.uint8).reshape(len(ts[c]), -1).eq(th[c].view(torch.uint8).reshape(len(th[c]), -1)).all(dim=1)
        assert bool(same[th["flag"] == 0].all()), (name, u["label"], "rows with flag 0 differ from the section rule's")
        kept += int((~same).sum())
    R, S = rounds_for(bench.N_BISECT), HYBRID_SECTIONS
    brackets = sum(u["brackets"] for u in units)
    res = {}
    for rname, _ in rules:
        v, h = ms[rname], stats[rname]
        mpb = 16 * R + 2 if rname == "section" or h.brackets == 0 else \
            16 * S + h.evaluations / h.brackets + (16 * (R - S) + 2) * h.fallback / h.brackets
        res[rname] = (statistics.median(v), min(v), max(v))
        print(json.dumps({"workload": name, "rule": rname, "units": len(units), "k_rows": int(units[0]["k"].numel()),
                          "repeats": len(v), "median_ms": round(res[rname][0], 4), "min_ms": round(res[rname][1], 4),
                          "max_ms": round(res[rname][2], 4), "brackets": brackets, "refine_stats": list(h),
                          "marches_per_bracket": round(mpb, 2)}), flush=True)
    spread = max(res["section"][2] - res["section"][1], res["hybrid"][2] - res["hybrid"][1])
    diff = res["hybrid"][0] - res["section"][0]
    verdict = "equal" if abs(diff) <= spread else ("hybrid faster" if diff < 0 else "hybrid slower")
    print(json.dumps({"workload": name, "hybrid_minus_section_ms": round(diff, 4), "larger_spread_ms": round(spread, 4),
                      "hybrid_over_section": round(res["hybrid"][0] / res["section"][0], 4), "verdict": verdict,
                      "rows_differing_from_section": kept}), flush=True)
    for u in units:
        u["prob"].close()
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--one", help=argparse.SUPPRESS)          # child mode: a single workload in this process
    a = ap.parse_args()
    assert a.repeats >= 20, "at least 20 timed repeats per rule"
    if a.one:
        return child(a.one, a.repeats, a.warmup)
    for name in a.workloads.split(","):
        assert name in WORKLOADS, name
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--one", name,
               "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                           # a fault or a time limit: start nothing more on the GPU
            print(json.dumps({"workload": name, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

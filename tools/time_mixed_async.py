"""GPU timing aid: the configs[4] units (bench.workload_units("config4"): rotational-flow cylinder, m = 0..10, 1024 x 1024
grid per order, fp32 screening + fp64 refinement) on rank 0's tile of an E-GPU run, E = 1, 2, 4, 8, in three variants:

  a  the synchronous path bench.py runs today: es_shoot_screen_grid + es_shoot_find_roots_screened, one lane (library
     context on its own stream) per unit, one host thread per unit, pack_fixed from the host count;
  b  es_shoot_find_roots_mixed_async, one lane per unit, every step of every unit enqueued from ONE host thread,
     pack_fixed from counts[0:1];
  c  as b with two lanes per unit (consecutive steps of a unit alternate between them).

Each (E, variant) prints one JSON line: ms per step (S steps after warm-up, device events; a step = every unit once),
brackets and fp64 re-evaluations per step.  Every variant's root tables and counts must equal those of a (asserted).
The last line compares the E = 8 tile with the aim 1.25 x (E = 1 ms per step) / 8.

    python tools/time_mixed_async.py [--steps 10] [--warmup 2] [--E 1,2,4,8] [--variants a,b,c]
"""
import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from eigensolver_amd import ShootProblem, _lib  # noqa: E402
from eigensolver_amd import distributed as D  # noqa: E402
from eigensolver_amd.shooting import read_screen_counts  # noqa: E402


def make_units(E, dev):
    """Two lanes per unit on rank 0's tile (strided rows), tables sized from the data as bench.py sizes them."""
    _, units = bench.workload_units("config4")
    out = []
    for label, uid, eq, mode, m, k_np, W_np in units:
        rows = D.tile_rows(len(k_np), 0, E, strided=True)
        k = torch.as_tensor(k_np[rows], dtype=torch.float64, device=dev)
        W = torch.as_tensor(W_np, dtype=torch.float64, device=dev)
        lanes = []
        for _ in range(2):
            stream = torch.cuda.Stream(device=dev)
            ctx = _lib.Context(dev.index or 0, stream=stream)
            lanes.append({"stream": stream, "ctx": ctx, "prob": ShootProblem(eq, mode, m=m, ctx=ctx)})
        with torch.cuda.stream(lanes[0]["stream"]):
            _, nbr, _, _, _ = lanes[0]["prob"].find_roots_mixed(k, W, n_bisect=bench.N_BISECT,
                                                                tol_percent=bench.TOL_PERCENT, capacity=1 << 17)
        cap = 1024
        while cap < 2 * nbr:
            cap *= 2
        xcap = D.exchange_capacity(nbr)
        for ln in lanes:
            with torch.cuda.stream(ln["stream"]):
                ln["table"] = ln["prob"].alloc_root_table(cap)
                ln["counts"] = torch.zeros(4, dtype=torch.int32, device=dev)
                ln["rows"] = torch.as_tensor(rows, dtype=torch.int64, device=dev)
        out.append({"label": label, "uid": uid, "k": k, "W": W, "cap": cap, "xcap": xcap, "lanes": lanes})
    torch.cuda.synchronize()
    return out


def step_sync(u, ln):
    """Variant a, one unit: screen + synchronous screened call (three host waits inside) + pack from the host count."""
    with torch.cuda.stream(ln["stream"]):
        Dg, st = ln["prob"].screen_grid(u["k"], u["W"])
        _, nbr, _, _, stats = ln["prob"].find_roots_screened(u["k"], u["W"], Dg, st, n_bisect=bench.N_BISECT,
                                                              tol_percent=bench.TOL_PERCENT, table=ln["table"])
        D.pack_fixed(ln["table"][0], nbr, u["uid"], ln["rows"], u["xcap"], ctx=ln["ctx"])
        done = torch.cuda.Event()
        done.record(ln["stream"])
    ln["host"] = (nbr, *stats)
    return done


def step_async(u, ln):
    """Variants b, c, one unit: everything enqueued, nothing read back."""
    with torch.cuda.stream(ln["stream"]):
        t, _, _ = ln["prob"].find_roots_mixed_async(u["k"], u["W"], ln["table"], ln["counts"], n_bisect=bench.N_BISECT,
                                                    tol_percent=bench.TOL_PERCENT)
        D.pack_fixed(t, ln["counts"][0:1], u["uid"], ln["rows"], u["xcap"], ctx=ln["ctx"])
        done = torch.cuda.Event()
        done.record(ln["stream"])
    return done


def run_steps(units, variant, nsteps, pool):
    """nsteps steps of every unit; returns the device time in ms from before the first launch to the last lane's end."""
    cur = torch.cuda.current_stream()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(cur)
    if variant == "a":
        def loop(u):
            return [step_sync(u, u["lanes"][0]) for _ in range(nsteps)][-1]
        dones = list(pool.map(loop, units))
    else:
        n_lanes = 1 if variant == "b" else 2
        dones = []
        for i in range(nsteps):
            for u in units:
                dones.append(step_async(u, u["lanes"][i % n_lanes]))
    for d in dones:
        cur.wait_event(d)
    e1.record(cur)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def records(ln, n):
    return {c: ln["table"][0][c][:n].clone() for c in ("k", "w", "w_lo", "w_hi", "resid", "row", "flag")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--E", default="1,2,4,8")
    ap.add_argument("--variants", default="a,b,c")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    variants = a.variants.split(",")
    assert variants[0] == "a", "variant a is the reference the others are checked against"
    results = {}
    for E in (int(x) for x in a.E.split(",")):
        units = make_units(E, dev)
        pool = ThreadPoolExecutor(max_workers=len(units))
        ref = None
        for v in variants:
            run_steps(units, v, max(a.warmup, 2), pool)          # warm-up: every lane at least once, scratch grown
            ms = run_steps(units, v, a.steps, pool) / a.steps
            got = []
            for u in units:
                lanes = u["lanes"][:1] if v in ("a", "b") else u["lanes"]
                for ln in lanes:
                    if v == "a":
                        c = ln["host"]
                    else:
                        r = read_screen_counts(ln["counts"], u["cap"])
                        c = (r.count, r.unsure, r.ends, r.violations)
                    got.append((u["label"], c, records(ln, min(c[0], u["cap"]))))
            if ref is None:
                ref = {lab: (c, rec) for lab, c, rec in got}
            for lab, c, rec in got:
                rc, rrec = ref[lab]
                assert c == rc, (E, v, lab, c, rc)
                for col in rec:
                    assert torch.equal(rec[col].view(torch.uint8), rrec[col].view(torch.uint8)), (E, v, lab, col)
            brackets = sum(rc[0] for rc, _ in ref.values())
            reevals = sum(rc[1] + rc[2] for rc, _ in ref.values())
            line = {"E": E, "variant": v, "k_rows": int(units[0]["k"].numel()), "units": len(units),
                    "lanes_per_unit": 2 if v == "c" else 1, "host_threads": len(units) if v == "a" else 1,
                    "steps": a.steps, "ms_per_step": round(ms, 3), "brackets": brackets, "fp64_reevals": reevals,
                    "tables_equal_a": True}
            results[(E, v)] = ms
            print(json.dumps(line), flush=True)
        pool.shutdown()
        for u in units:
            for ln in u["lanes"]:
                ln["prob"].close()
                ln["ctx"].close()
        del units
        torch.cuda.empty_cache()
    for v in variants:
        if (1, v) in results and (8, v) in results:
            aim = 1.25 * results[(1, v)] / 8
            print(json.dumps({"variant": v, "aim_E8_ms": round(aim, 3), "E8_ms": round(results[(8, v)], 3),
                              "E8_over_E1_div_8": round(results[(8, v)] / (results[(1, v)] / 8), 3),
                              "meets_aim": results[(8, v)] <= aim}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""GPU timing aid for C ABI section 14 (complex frequencies on the untwisted cylinder), on one device.  A record, no threshold.

The Kelvin-Helmholtz unstable kink mode of a cylinder with a Gaussian jet (CylinderFlow(c_i0=1, vA_i0=2, c_e=1.5, vA_e=0.5,
U_i0=3, width=1.5), N = 1000 nodes) on 64 wavenumbers in [1.5, 2.5] x 64 x 64 phase speeds (Re W in [1.0, 1.6], Im W in
[0.01, 0.2], ES_W_PHASE_SPEED): 262144 determinants.  Two legs, each between two device events on the context's stream,
alternating repeat by repeat, every input on the device before anything is timed:

  eval_grid    ONE es_cyl_complex_eval_grid over the 64 x 64 x 64 points
  find_roots   the es_cyl_complex_find_roots that follows it: flags, scan, 12 secant steps per flagged cell; the call reads
               its count back and synchronises

The comparison is the NumPy restatement tests/cyl_complex_model.py (scipy Bessel functions, all frequencies of a row marched
together as arrays) on one of the 64 k-rows, one process, its wall time multiplied by 64.

    python tools/time_cyl_complex.py [--repeats 10] [--warmup 2] [--out profiles/cyl_complex_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0, width=1.5)


def timed(torch, stream, a, legs):
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
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyl_complex_timing.jsonl"))
    a = ap.parse_args()
    import torch
    from eigensolver_amd import CylinderComplex, _lib, equilibrium as q
    from eigensolver_amd.shooting import W_PHASE_SPEED
    from tests.cyl_complex_model import model_for
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    eq = q.CylinderFlow(**KH, n_nodes=a.nodes)
    k = np.linspace(1.5, 2.5, a.rows)
    w_re, w_im = np.linspace(1.0, 1.6, 64), np.linspace(0.01, 0.2, 64)
    with torch.cuda.stream(stream):
        c = CylinderComplex(eq, ctx=ctx)
        p = c.problem("kink")
        dk, dre, dim = p._dev(k), p._dev(w_re), p._dev(w_im)
        D, st, _ = c.eval_grid("kink", dk, dre, dim, W_PHASE_SPEED)
        roots, count = c.find_roots("kink", dk, dre, dim, D, st, W_PHASE_SPEED, capacity=4096)
    flag, row = roots["flag"].cpu().numpy(), roots["row"].cpu().numpy()
    line = {"device": torch.cuda.get_device_name(dev), "nodes": a.nodes, "grid": [a.rows, 64, 64], "repeats": a.repeats,
            "warmup": a.warmup, "points_ok": int((st == 0).sum().item()), "cells_flagged": int(count),
            "roots_accepted": int((flag == 1).sum()), "rows_with_root": int(len(set(row[flag == 1].tolist())))}
    legs = {"eval_grid": lambda: c.eval_grid("kink", dk, dre, dim, W_PHASE_SPEED),
            "find_roots": lambda: c.find_roots("kink", dk, dre, dim, D, st, W_PHASE_SPEED, capacity=4096)}
    line["legs"] = timed(torch, stream, a, legs)
    # the NumPy model on one row of the 64, scaled
    M = model_for(eq, "kink")
    r = a.rows // 2
    t0 = time.perf_counter()
    Dm, relm, stm = M.eval_grid(k[r:r + 1], w_re, w_im, W_PHASE_SPEED)
    t_grid = time.perf_counter() - t0
    got = D[r].cpu().numpy()
    ok = stm[0] == 0
    line["row_vs_model_max"] = float(np.max(np.abs(got[ok] - Dm[0][ok]) / (np.abs(Dm[0][ok]) * 100.0 / relm[0][ok])))
    line["numpy_one_row_s"] = round(t_grid, 3)
    line["numpy_grid_scaled_s"] = round(t_grid * a.rows, 2)
    line["eval_grid_speedup_over_numpy"] = round(t_grid * a.rows * 1e3 / line["legs"]["eval_grid"]["median_ms"], 1)
    line["det_evals_per_s"] = round(a.rows * 64 * 64 / (line["legs"]["eval_grid"]["median_ms"] * 1e-3), 0)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    c.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""GPU timing aid for C ABI section 17 (complex frequencies on the twisted cylinder), on one device.  A record, no threshold.

Case A -- CylinderRotation(v_twist=2, power=1, r_axis=1e-2), kink, m = 3, unstable near omega = 1.555 + 0.792i at k = 1 -- on
64 wavenumbers in [0.8, 1.2] x 64 x 64 frequencies (Re omega in [1.2, 1.9], Im omega in [0.45, 1.15], ES_W_ABSOLUTE): 262144
determinants, at N = 1000 and N = 2000 nodes.  Beside it the zero-twist jet of DESIGN 8i at N = 1000 posed both ways -- as an
untwisted problem through es_cyl_complex_eval_grid and as a twisted one (v_phi = B_phi = 0) through
es_cylt_complex_eval_grid, on the same points: the ratio is what the larger coefficient set costs.
Every leg runs between two device events on the context's stream, legs alternating repeat by repeat, every input on the
device before anything is timed; medians with min - max:

  eval_grid_N     ONE es_cylt_complex_eval_grid over the 64 x 64 x 64 points of case A at N nodes
  find_roots_N    the es_cylt_complex_find_roots that follows it: flags, scan, 12 secant steps per flagged cell; the call reads
                  its count back and synchronises
  jet_untwisted   es_cyl_complex_eval_grid, the jet as CylinderFlow
  jet_twisted     es_cylt_complex_eval_grid, the same jet as a twisted problem

The comparison is the NumPy restatement tests/cylt_complex_model.py (all frequencies of a row marched together as arrays) on
one of the 64 k-rows of case A at N = 1000, one process, one core, its wall time multiplied by 64.

    python tools/time_cylt_complex.py [--repeats 20] [--warmup 3] [--out profiles/cylt_complex.jsonl]
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

JET = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0, width=1e5, r_sign=1.0, r_axis=1e-3)


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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cylt_complex.jsonl"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")              # the NumPy leg: one core
    import torch
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, _lib, equilibrium as q
    from eigensolver_amd.shooting import W_ABSOLUTE
    from tests.cylt_complex_model import model_for
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"

    class TwistedJet(q.CylinderFlow):
        twisted = True

    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    k = np.linspace(0.8, 1.2, a.rows)
    w_re, w_im = np.linspace(1.2, 1.9, 64), np.linspace(0.45, 1.15, 64)
    kj, wj_re, wj_im = np.linspace(1.5, 2.5, a.rows), np.linspace(1.8, 3.0, 64), np.linspace(0.3, 0.9, 64)
    line = {"device": torch.cuda.get_device_name(dev), "grid": [a.rows, 64, 64], "repeats": a.repeats, "warmup": a.warmup}
    legs, keep = {}, []
    with torch.cuda.stream(stream):
        for N in (1000, 2000):
            c = RotatingCylinderComplex(q.CylinderRotation(v_twist=2.0, power=1.0, r_axis=1e-2, n_nodes=N), ctx=ctx)
            p = c.problem("kink", 3)
            dk, dre, dim = p._dev(k), p._dev(w_re), p._dev(w_im)
            D, st, _ = c.eval_grid("kink", dk, dre, dim, W_ABSOLUTE, m=3)
            roots, count = c.find_roots("kink", dk, dre, dim, D, st, W_ABSOLUTE, capacity=4096, m=3)
            flag, row = roots["flag"].cpu().numpy(), roots["row"].cpu().numpy()
            line[f"case_A_N{N}"] = {"points_ok": int((st == 0).sum().item()), "cells_flagged": int(count),
                                    "roots_accepted": int((flag == 1).sum()),
                                    "rows_with_root": int(len(set(row[flag == 1].tolist())))}
            legs[f"eval_grid_{N}"] = (lambda c=c, dk=dk, dre=dre, dim=dim: c.eval_grid("kink", dk, dre, dim, W_ABSOLUTE, m=3))
            legs[f"find_roots_{N}"] = (lambda c=c, dk=dk, dre=dre, dim=dim, D=D, st=st:
                                       c.find_roots("kink", dk, dre, dim, D, st, W_ABSOLUTE, capacity=4096, m=3))
            keep.append((c, D))
        c0 = CylinderComplex(q.CylinderFlow(**JET, n_nodes=1000), ctx=ctx)
        ct = RotatingCylinderComplex(TwistedJet(**JET, n_nodes=1000), ctx=ctx)
        p0 = c0.problem("kink")
        djk, djre, djim = p0._dev(kj), p0._dev(wj_re), p0._dev(wj_im)
        D0, st0, rel0 = c0.eval_grid("kink", djk, djre, djim, W_ABSOLUTE)
        Dt, stt, _ = ct.eval_grid("kink", djk, djre, djim, W_ABSOLUTE)
        ok = (st0 == 0) & (stt == 0)
        sc = (D0.abs() * 100.0 / rel0)[ok]
        line["jet"] = {"nodes": 1000, "points_ok": int(ok.sum().item()),
                       "twisted_vs_untwisted_median": float(((Dt - D0).abs()[ok] / sc).median().item())}
        legs["jet_untwisted"] = lambda: c0.eval_grid("kink", djk, djre, djim, W_ABSOLUTE)
        legs["jet_twisted"] = lambda: ct.eval_grid("kink", djk, djre, djim, W_ABSOLUTE)
    line["legs"] = timed(torch, stream, a, legs)
    L = line["legs"]
    line["twisted_over_untwisted"] = round(L["jet_twisted"]["median_ms"] / L["jet_untwisted"]["median_ms"], 3)
    # the NumPy model on one row of case A at N = 1000, scaled
    M = model_for(q.CylinderRotation(v_twist=2.0, power=1.0, r_axis=1e-2, n_nodes=1000), "kink", 3)
    r = a.rows // 2
    t0 = time.perf_counter()
    Dm, relm, stm = M.eval_grid(k[r:r + 1], w_re, w_im, W_ABSOLUTE)
    t_grid = time.perf_counter() - t0
    got = keep[0][1][r].cpu().numpy()
    okm = stm[0] == 0
    line["row_vs_model_max"] = float(np.max(np.abs(got[okm] - Dm[0][okm]) / (np.abs(Dm[0][okm]) * 100.0 / relm[0][okm])))
    line["numpy_one_row_s"] = round(t_grid, 3)
    line["numpy_grid_scaled_s"] = round(t_grid * a.rows, 2)
    line["eval_grid_speedup_over_numpy"] = round(t_grid * a.rows * 1e3 / L["eval_grid_1000"]["median_ms"], 1)
    line["det_evals_per_s_N1000"] = round(a.rows * 64 * 64 / (L["eval_grid_1000"]["median_ms"] * 1e-3), 0)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    for c, _ in keep:
        c.close()
    c0.close()
    ct.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""GPU timing aid: the growth-rate curve of an unstable cylinder branch on 4096 wavenumbers by Newton tracing from a coarse
scan (CylinderComplex.densify: es_cyl_complex_root_slopes, the Hermite prediction, es_cyl_complex_newton) against the route
without it, a complex grid and the winding-number search at every fine wavenumber, on one device.

Problem: the Kelvin-Helmholtz unstable Gaussian jet of DESIGN.md section 8i at width 1.5, kink, N = 1000 nodes, k in
[1.5, 2.5].  The coarse scan -- 17 rows through unstable_roots -- is done once, before anything is timed.  Legs, each between
two device events on the context's stream, alternating repeat by repeat in one process so that drift hits all alike:

    densify       CylinderComplex.densify from the 17 coarse rows to the 4096 fine wavenumbers
    grid_search   eval_grid on a 64 x 64 (Re, Im) window of phase speeds and find_roots on it for 64 of the fine rows: what
                  every fine wavenumber costs without the tracing; the figure is reported scaled by 4096 / 64 as well
    slopes        ONE es_cyl_complex_root_slopes on 2^15 pairs along the branch
    stencil       es_cyl_complex_eval_points on the 5 x 2^15 points of a 5-point difference stencil in omega and k around the
                  same pairs: what D_w and D_k cost by differences (and they would still be inexact)

One JSON line with median / min / max ms per leg over the repeats and the ratios is printed and appended to --out.  Nothing
gates on these numbers: they are the record of DESIGN.md section 8j.

    python tools/time_cyl_complex_tracing.py [--repeats 10] [--warmup 2] [--out profiles/cyl_complex_tracing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0)
K_RANGE = (1.5, 2.5)
W_RE, W_IM = (1.0, 1.6), (0.005, 0.105)            # phase speeds: the window around the kink branch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyl_complex_tracing.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import numpy as np
    import torch
    from eigensolver_amd import CylinderComplex, _lib
    from eigensolver_amd import equilibrium as q
    from eigensolver_amd import postprocess as pp
    from eigensolver_amd.shooting import W_PHASE_SPEED
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    kf = np.linspace(K_RANGE[0], K_RANGE[1], 4096)
    kc = np.linspace(K_RANGE[0], K_RANGE[1], 17)
    k64 = kf[::64]
    npairs = 1 << 15
    with torch.cuda.stream(stream):
        c = CylinderComplex(q.CylinderFlow(**KH, width=1.5, n_nodes=a.nodes), ctx=ctx)
        rows = c.unstable_roots("kink", kc, np.linspace(W_RE[0], W_RE[1], 13), np.linspace(W_IM[0], W_IM[1], 11), W_PHASE_SPEED)
        assert [len(r) for r in rows] == [1] * len(kc), "one root per coarse row in the window"
        wc = np.array([r[0] for r in rows])
        p = c.problem("kink")
        dkc, dwc, dkf = p._dev(kc), torch.as_tensor(wc, device=dev), p._dev(kf)
        dk64 = p._dev(k64)
        dre, dim = p._dev(np.linspace(W_RE[0], W_RE[1], 64)), p._dev(np.linspace(W_IM[0], W_IM[1], 64))
        first = c.densify("kink", dkc, dwc, dkf)
        stream.synchronize()
        flagged = int(first["flag"].sum().item())
        iters = first["iters"].cpu().numpy()
        kstar, wstar = pp.most_unstable(first["k"].cpu().numpy(), first["w"].cpu().numpy(), first["dwdk"].cpu().numpy())
        # 2^15 pairs along the branch and their 5-point stencil
        sel = torch.arange(npairs, device=dev) % 4096
        pk, pw = first["k"][sel].contiguous(), first["w"][sel].contiguous()
        h = 1e-4
        sk = torch.cat([pk, pk, pk, pk + h, pk - h]).contiguous()
        sw = torch.cat([pw, pw + h, pw - h, pw, pw]).contiguous()
        sre, sim = sw.real.contiguous(), sw.imag.contiguous()
        ns = int(sk.numel())
        Dre, Dim, rel = (torch.empty(ns, dtype=torch.float64, device=dev) for _ in range(3))
        st = torch.empty(ns, dtype=torch.uint8, device=dev)
    lib, P = ctx.lib, _lib.ptr

    def densify():
        c.densify("kink", dkc, dwc, dkf)

    def grid_search():
        D, s, _ = c.eval_grid("kink", dk64, dre, dim, W_PHASE_SPEED)
        c.find_roots("kink", dk64, dre, dim, D, s, W_PHASE_SPEED)

    def slopes():
        c.root_slopes("kink", pk, pw)

    def stencil():
        _lib.check(ctx.handle, lib.es_cyl_complex_eval_points(ctx.handle, p.handle, P(sk), P(sre), P(sim), ns, P(Dre), P(Dim),
                                                              P(rel), P(st), None, None))

    legs = {"densify": densify, "grid_search": grid_search, "slopes": slopes, "stencil": stencil}
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
    line = {"device": torch.cuda.get_device_name(dev), "nodes": a.nodes, "fine_rows": len(kf), "coarse_rows": len(kc),
            "flagged": flagged, "newton_steps_mean": round(float(iters.mean()), 2), "newton_steps_max": int(iters.max()),
            "most_unstable_k": [float(x) for x in kstar], "grid_rows": len(k64), "grid_window": [64, 64], "pairs": npairs,
            "stencil_points": ns, "repeats": a.repeats, "warmup": a.warmup, "legs": {}}
    for name, v in ms.items():
        line["legs"][name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line["grid_search_scaled_to_4096_ms"] = round(med["grid_search"] * len(kf) / len(k64), 3)
    line["densify_over_scaled_grid_search"] = round(med["densify"] / (med["grid_search"] * len(kf) / len(k64)), 5)
    line["slopes_over_stencil"] = round(med["slopes"] / med["stencil"], 3)
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

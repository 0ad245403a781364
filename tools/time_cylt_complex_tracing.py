"""GPU timing aid: the growth-rate curve of an unstable branch of the rotating (twisted) cylinder on 4096 wavenumbers by Newton
tracing from a coarse scan (RotatingCylinderComplex.densify: es_cylt_complex_root_slopes, the Hermite prediction,
es_cylt_complex_newton) against the route without it, a complex grid and the winding-number search at every fine wavenumber,
on one device.

Problem: case A of DESIGN.md section 8l -- CylinderRotation(v_twist = 2, power = 1, r_axis = 1e-2), kink, m = 3 -- at N = 1000
nodes, k in [0.85, 1.1].  The coarse scan -- 17 rows through unstable_roots -- is done once, before anything is timed.  Legs,
each between two device events on the context's stream, alternating repeat by repeat in one process so that drift hits all alike:

    densify         RotatingCylinderComplex.densify from the 17 coarse rows to the 4096 fine wavenumbers
    grid_search     eval_grid on a 64 x 64 (Re, Im) window and find_roots on it for 64 of the fine rows: what every fine
                    wavenumber costs without the tracing; the figure is reported scaled by 4096 / 64 as well
    slopes          ONE es_cylt_complex_root_slopes on 2^15 pairs along the branch
    stencil         es_cylt_complex_eval_points on the 5 x 2^15 points of a 5-point difference stencil in omega and k around the
                    same pairs: what D_w and D_k cost by differences (and they would still be inexact)
    slopes_twist0   es_cylt_complex_root_slopes on 2^15 pairs of the zero-twist jet (the uniform jet of DESIGN.md section 8i
                    posed as a twisted problem: v_phi = B_phi = 0 through the 20-field table and the general coefficient set)
    slopes_plain    es_cyl_complex_root_slopes on the same pairs of the same jet as an untwisted problem: the difference of
                    the two is what the larger coefficient set costs

One JSON line with median / min / max ms per leg over the repeats and the ratios is printed and appended to --out.  Nothing
gates on these numbers: they are the record of DESIGN.md section 8m.

    python tools/time_cylt_complex_tracing.py [--repeats 10] [--warmup 2] [--out profiles/cylt_complex_tracing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE_A = dict(v_twist=2.0, power=1.0, r_axis=1e-2)
M_A = 3
K_RANGE = (0.85, 1.1)
W_RE, W_IM = (1.2, 1.9), (0.45, 1.15)              # absolute frequencies: case A's window
JET = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0, width=1e5, r_sign=1.0, r_axis=1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cylt_complex_tracing.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import numpy as np
    import torch
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, _lib
    from eigensolver_amd import equilibrium as q
    from eigensolver_amd import postprocess as pp
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"

    class TwistedJet(q.CylinderFlow):
        twisted = True

    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream)
    kf = np.linspace(K_RANGE[0], K_RANGE[1], 4096)
    kc = np.linspace(K_RANGE[0], K_RANGE[1], 17)
    k64 = kf[::64]
    npairs = 1 << 15
    with torch.cuda.stream(stream):
        c = RotatingCylinderComplex(q.CylinderRotation(**CASE_A, n_nodes=a.nodes), ctx=ctx)
        rows = c.unstable_roots("kink", kc, np.linspace(W_RE[0], W_RE[1], 8), np.linspace(W_IM[0], W_IM[1], 8), m=M_A)
        assert [len(r) for r in rows] == [1] * len(kc), "one root per coarse row in the window"
        wc = np.array([r[0] for r in rows])
        p = c.problem("kink", M_A)
        dkc, dwc, dkf = p._dev(kc), torch.as_tensor(wc, device=dev), p._dev(kf)
        dk64 = p._dev(k64)
        dre, dim = p._dev(np.linspace(W_RE[0], W_RE[1], 64)), p._dev(np.linspace(W_IM[0], W_IM[1], 64))
        first = c.densify("kink", dkc, dwc, dkf, m=M_A)
        stream.synchronize()
        flagged = int(first["flag"].sum().item())
        iters = first["iters"].cpu().numpy()
        kstar, _ = pp.most_unstable(first["k"].cpu().numpy(), first["w"].cpu().numpy(), first["dwdk"].cpu().numpy())
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
        # the zero-twist jet, as a twisted and as an untwisted problem, on the same pairs
        ct = RotatingCylinderComplex(TwistedJet(**JET, n_nodes=a.nodes), ctx=ctx)
        c0 = CylinderComplex(q.CylinderFlow(**JET, n_nodes=a.nodes), ctx=ctx)
        rng = np.random.default_rng(5)
        jk = rng.uniform(1.0, 2.5, npairs)
        jw = jk * rng.uniform(0.9, 1.45, npairs) + 1j * jk * rng.uniform(0.05, 0.4, npairs) * rng.choice([-1.0, 1.0], npairs)
        djk, djw = p._dev(jk), torch.as_tensor(jw, device=dev)
        ok_t = int((ct.root_slopes("kink", djk, djw).status == 0).sum().item())
        ok_0 = int((c0.root_slopes("kink", djk, djw).status == 0).sum().item())
        stream.synchronize()
    lib, P = ctx.lib, _lib.ptr

    def densify():
        c.densify("kink", dkc, dwc, dkf, m=M_A)

    def grid_search():
        D, s, _ = c.eval_grid("kink", dk64, dre, dim, m=M_A)
        c.find_roots("kink", dk64, dre, dim, D, s, m=M_A)

    def slopes():
        c.root_slopes("kink", pk, pw, m=M_A)

    def stencil():
        _lib.check(ctx.handle, lib.es_cylt_complex_eval_points(ctx.handle, p.handle, P(sk), P(sre), P(sim), ns, P(Dre), P(Dim),
                                                               P(rel), P(st), None, None))

    def slopes_twist0():
        ct.root_slopes("kink", djk, djw)

    def slopes_plain():
        c0.root_slopes("kink", djk, djw)

    legs = {"densify": densify, "grid_search": grid_search, "slopes": slopes, "stencil": stencil,
            "slopes_twist0": slopes_twist0, "slopes_plain": slopes_plain}
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
            "stencil_points": ns, "jet_pairs_ok": [ok_t, ok_0], "repeats": a.repeats, "warmup": a.warmup, "legs": {}}
    for name, v in ms.items():
        line["legs"][name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line["grid_search_scaled_to_4096_ms"] = round(med["grid_search"] * len(kf) / len(k64), 3)
    line["densify_over_scaled_grid_search"] = round(med["densify"] / (med["grid_search"] * len(kf) / len(k64)), 5)
    line["slopes_over_stencil"] = round(med["slopes"] / med["stencil"], 3)
    line["slopes_twist0_over_plain"] = round(med["slopes_twist0"] / med["slopes_plain"], 3)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    c.close()
    ct.close()
    c0.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""GPU timing aid: the eigenfunctions of unstable rotating-tube modes (C ABI section 19), on one device.  The protocol of
tools/time_cyl_complex_fields.py part 2: bare C calls on arrays that are already on the device, each between two device events
on the context's stream, the legs alternating repeat by repeat; warm-up, then the median of repeated launches; one JSON line
per leg.

    tube   2^15 (k, omega) pairs at N = 1000 without exterior points on the rotating tube of case A (v_twist = 2, power = 1,
           m = 3): es_cylt_complex_eigenfunction against es_cylt_complex_eval_points on the same pairs -- what its three passes
           (one outwards parking 2 x 16 B per node, two inwards with the step's 2 x 2 matrix formed and inverted, the last
           reading and writing every node) cost beyond the determinant's one adjoint march;
    jet    the same count on the zero-twist jet: es_cylt_complex_eigenfunction (the jet posed as a twisted problem: 20 base
           fields, the general coefficient set, the full-shape step, three passes) against es_cyl_complex_eigenfunction (7
           fields, the off-diagonal step, two outward marches) on the same pairs -- what the twisted path costs where both apply.

    python tools/time_cylt_complex_fields.py [--repeats 20] [--warmup 3] [--lib PATH] [--out profiles/cylt_complex_fields.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthesis_timing  # noqa: E402  (tools/, beside this file)

JET = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0, width=1e5, r_sign=1.0, r_axis=1e-3)
N_PAIRS, N_NODES = 1 << 15, 1000


def run_legs(torch, stream, a, group, legs, extra):
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
    lines = [dict(group=group, leg=name, pairs=N_PAIRS, n_nodes=N_NODES, repeats=len(v), median_ms=round(statistics.median(v), 4),
                  min_ms=round(min(v), 4), max_ms=round(max(v), 4), **extra) for name, v in ms.items()]
    first, second = list(legs)
    lines.append({"group": group, f"{first}_over_{second}": round(statistics.median(ms[first]) / statistics.median(ms[second]), 3)})
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    synthesis_timing.add_common_arguments(ap)
    a = ap.parse_args()
    torch, dev, stream, ctx = synthesis_timing.open_context(a)
    import numpy as np
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, _lib, equilibrium as q

    class TwistedJet(q.CylinderFlow):
        twisted = True

    lib, h, P, n = ctx.lib, ctx.handle, _lib.ptr, N_PAIRS
    rng = np.random.default_rng(19)
    k = rng.uniform(0.5, 2.0, n)
    with torch.cuda.stream(stream):
        Dre, Dim, rel = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        vi, fi = (torch.empty((n, N_NODES), dtype=torch.complex128, device=dev) for _ in range(2))
        up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)                # noqa: E731
        # the rotating tube of case A
        tube = RotatingCylinderComplex(q.CylinderRotation(v_twist=2.0, power=1.0, r_axis=1e-2, n_nodes=N_NODES), ctx=ctx)
        w = k * rng.uniform(1.2, 1.9, n) + 1j * k * rng.uniform(0.45, 1.15, n)
        ok = float((tube.eval_points("kink", k, w, m=3)[1] == 0).double().mean())
        pt = tube.problem("kink", 3)
        dk, dre, dim = up(k), up(w.real), up(w.imag)

    def eig(call, prob):                                 # an eigenfunction leg on the current pairs: no exterior points
        return lambda: _lib.check(h, call(h, prob.handle, P(dk), P(dre), P(dim), n, P(vi), P(fi), 0, None, None, None, P(st)))

    run_legs(torch, stream, a, "tube", {
        "cylt_eigenfunction": eig(lib.es_cylt_complex_eigenfunction, pt),
        "cylt_eval_points": lambda: _lib.check(h, lib.es_cylt_complex_eval_points(h, pt.handle, P(dk), P(dre), P(dim), n, P(Dre),
                                                                                  P(Dim), P(rel), P(st), None, None))},
             dict(device=torch.cuda.get_device_name(dev), ok_share=round(ok, 3)))
    tube.close()
    with torch.cuda.stream(stream):
        # the zero-twist jet through both families
        jt = RotatingCylinderComplex(TwistedJet(**JET, n_nodes=N_NODES), ctx=ctx)
        j0 = CylinderComplex(q.CylinderFlow(**JET, n_nodes=N_NODES), ctx=ctx)
        w = k * rng.uniform(0.9, 1.45, n) + 1j * k * rng.uniform(0.05, 0.4, n)
        ok = float((j0.eval_points("kink", k, w)[1] == 0).double().mean())
        pjt, pj0 = jt.problem("kink"), j0.problem("kink")
        dre, dim = up(w.real), up(w.imag)
    run_legs(torch, stream, a, "jet", {"cylt_eigenfunction": eig(lib.es_cylt_complex_eigenfunction, pjt),
                                       "cyl_eigenfunction": eig(lib.es_cyl_complex_eigenfunction, pj0)},
             dict(device=torch.cuda.get_device_name(dev), ok_share=round(ok, 3)))
    jt.close()
    j0.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

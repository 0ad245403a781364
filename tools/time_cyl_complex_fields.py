"""GPU timing aid: the perturbation fields of an unstable cylinder mode (C ABI section 16), on one device.

Part 1, in the manner of tools/time_field_synthesis.py -- the same mesh (1 200 radii = 500 interior nodes + 700 exterior points
x 60 angles x 16 heights, the ten `varlist` variables, chunks of 8 frames: 369 MB per call), the amplitude table that of
CylinderComplex.polarisation at the kink root k = 2 of the Kelvin-Helmholtz unstable jet.  Legs, all writing the same bytes
into one buffer, each between two device events on the context's stream, alternating repeat by repeat:

    kernel        es_cyl_complex_field_synthesis (points not requested)
    torch         the same expression A_re (Theta EC) - A_im (Theta ES) as broadcast torch code in fp64, cast to fp32
    fill          Tensor.fill_ of the buffer: the store-bandwidth yardstick of this device on this day
    polarisation  one CylinderComplex.polarisation call (eigenfunction + amplitudes of one mode, 1 200 radial points)

Part 2: es_cyl_complex_eigenfunction for 2^15 (k, omega) pairs at N = 1000 without exterior points against
es_cyl_complex_eval_points on the same pairs -- what the two outward marches, one of them writing 2 x 16 B per node, cost
beyond the determinant's one adjoint march.

Warm-up, then the median of repeated launches, stream-synchronised; one JSON line per leg.

    python tools/time_cyl_complex_fields.py [--repeats 20] [--warmup 3] [--frames 8] [--calls 1] [--lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthesis_timing  # noqa: E402  (tools/, beside this file)

VARLIST = ["xi_r", "xi_phi", "P_T", "v_r", "v_phi", "xi_x", "xi_y", "v_x", "v_y", "v_z"]
KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0)
MODE, K, W0 = "kink", 2.0, 2.673525 + 0.084845j


def torch_fields(torch, amp, m, k, w, theta, z, t, v_scale, out):
    """The fields of es_cyl_complex_field_synthesis as broadcast expressions, fp64, cast to fp32 (z-components with -sin)."""
    A = dict(zip(("xi_r", "xi_phi", "xi_z", "P_T", "v_r", "v_phi", "v_z"), amp))
    th, tt = theta[None, None, :, None], t[:, None, None, None]
    ph, E = k * z[None, :, None, None] - w.real * tt, torch.exp(w.imag * tt)
    EC, ES = E * torch.cos(ph), E * torch.sin(ph)
    cm, sm = torch.cos(m * th), -torch.sin(m * th)
    c1, s1 = torch.cos(th), torch.sin(th)

    def val(name, ang, s=1.0):
        a = A[name] * s
        return a.real[None, None, None, :] * (ang * EC) - a.imag[None, None, None, :] * (ang * ES)
    xi_r, xi_phi = val("xi_r", cm), val("xi_phi", sm)
    v_r, v_phi = val("v_r", cm, v_scale), val("v_phi", sm, v_scale)
    f = [xi_r, xi_phi, val("P_T", cm), v_r, v_phi, xi_r * c1 - xi_phi * s1, xi_r * s1 + xi_phi * c1, v_r * c1 - v_phi * s1,
         v_r * s1 + v_phi * c1, val("v_z", sm, v_scale)]
    for i, a in enumerate(f):
        out[:, i] = a.to(torch.float32)


def time_eigenfunction(torch, stream, a, ctx, n=1 << 15, n_nodes=1000):
    """es_cyl_complex_eigenfunction against es_cyl_complex_eval_points on the same n pairs."""
    import numpy as np
    from eigensolver_amd import CylinderComplex, equilibrium as q
    with torch.cuda.stream(stream):
        c = CylinderComplex(q.CylinderFlow(**KH, width=1.5, r_sign=1.0, n_nodes=n_nodes), ctx=ctx)
        rng = np.random.default_rng(16)
        k = rng.uniform(0.5, 2.5, n)
        w = k * rng.uniform(0.6, 1.45, n) + 1j * k * rng.uniform(0.01, 0.1, n)
        ok = float((c.eval_points(MODE, k, w)[1] == 0).double().mean())
        # both legs as bare C calls on arrays that are already on the device
        from eigensolver_amd import _lib
        P, p, dev = _lib.ptr, c.problem(MODE), f"cuda:{ctx.device}"
        dk, dre, dim = (torch.as_tensor(x.copy(), device=dev) for x in (k, w.real, w.imag))
        Dre, Dim, rel = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        vi, fi = (torch.empty((n, n_nodes), dtype=torch.complex128, device=dev) for _ in range(2))
    lib, h = ctx.lib, ctx.handle
    legs = {"eigenfunction": lambda: _lib.check(h, lib.es_cyl_complex_eigenfunction(h, p.handle, P(dk), P(dre), P(dim), n, P(vi),
                                                                                    P(fi), 0, None, None, None, P(st))),
            "eval_points": lambda: _lib.check(h, lib.es_cyl_complex_eval_points(h, p.handle, P(dk), P(dre), P(dim), n, P(Dre),
                                                                                P(Dim), P(rel), P(st), None, None))}
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
    lines = [{"leg": name, "pairs": n, "n_nodes": n_nodes, "ok_share": round(ok, 3), "repeats": len(v),
              "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
             for name, v in ms.items()]
    lines.append({"eigenfunction_over_eval_points":
                  round(statistics.median(ms["eigenfunction"]) / statistics.median(ms["eval_points"]), 3)})
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    c.close()


def main():
    ap = argparse.ArgumentParser()
    synthesis_timing.add_common_arguments(ap)
    a = ap.parse_args()
    torch, dev, stream, ctx = synthesis_timing.open_context(a)
    import numpy as np
    from eigensolver_amd import CylinderComplex, _lib, equilibrium as q
    v_scale = 25.0
    with torch.cuda.stream(stream):
        c = CylinderComplex(q.CylinderFlow(**KH, width=1.5, r_sign=1.0, n_nodes=500), ctx=ctx)
        r = c.newton(MODE, [K], [W0])
        assert int(r["flag"][0]) == 1, "the root did not converge"
        w = complex(r["w"][0].item())
        pol = c.polarisation(MODE, [K], [w], n_ext=700)
        radius, amp = pol["radius"][0].contiguous(), pol["amp"][0].contiguous()
        assert bool(torch.isfinite(amp.real).all()) and bool(torch.isfinite(amp.imag).all()), "the mode is not ES_PT_OK"
        T = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev)    # noqa: E731
        theta, z = T(np.linspace(0.0, 2.0 * np.pi, 60)), T(np.linspace(0.01, 5.0, 16))
        t = T(np.linspace(0.01, 2.0 * np.pi, 80)[:a.frames])
        n_r, m = radius.numel(), int(c.problem(MODE).desc.m)
        out = torch.empty((a.frames, len(VARLIST), 16, 60, n_r), dtype=torch.float32, device=dev)
    flags = _lib.FIELD_Z_REFERENCE_ANGLE
    legs = {
        "kernel": lambda: c.field_synthesis(radius, amp, m, K, w, theta, z, t, VARLIST, v_scale, flags, want_points=False,
                                            out=out),
        "torch": lambda: torch_fields(torch, amp, float(m), K, w, theta, z, t, v_scale, out),
        "fill": lambda: out.fill_(1.0),
        "polarisation": lambda: c.polarisation(MODE, [K], [w], n_ext=700),
    }
    ms, check = synthesis_timing.measure(torch, stream, a, legs, lambda: out[0, :, 3, 7])
    grow = float(np.exp(w.imag * float(t.max())))
    synthesis_timing.assert_same_fields(check, float(amp.abs().max()) * v_scale * grow)
    synthesis_timing.report(a, torch.cuda.get_device_name(dev), ms, out.numel() * 4,
                            dict(mesh=[n_r, 60, 16], variables=len(VARLIST), w=[w.real, w.imag]),
                            "polarisation", dict(modes=1, radial_points=n_r))
    c.close()
    del out
    time_eigenfunction(torch, stream, a, ctx)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

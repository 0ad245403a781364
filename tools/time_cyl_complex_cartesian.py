"""GPU timing aid: the Cartesian sampling of an unstable cylinder mode with its vorticity
(es_cyl_complex_cartesian_synthesis, C ABI section 20) against the real kernel of section 8 on the real part of the same
table, against what a user would write without it and against the store bandwidth of the device, on one device.

Mesh: the reference's 267 x 267 Cartesian slice (x, y in [-2, 2]; --nxy 268 for the mesh whose planes start on 16-byte
boundaries) x 31 heights, all ten variables, chunks of 8 frames: 8 x 10 x 31 x 267 x 267 float32 = 707 MB per call.  The
tables are those of CylinderComplex.vorticity_amplitudes at one complex (k, omega) of the coronal density cylinder (width
0.9), 500 interior nodes + 700 exterior points -- a pair, not a root: the cost does not depend on the values.  The legs all
write the same number of bytes into the same buffer, each between two device events on the context's stream, alternating
repeat by repeat in one process so that drift hits all alike:

    kernel   es_cyl_complex_cartesian_synthesis (its (z, t) table pre-pass included)
    real     es_cyl_cartesian_synthesis on the real part of the same table at Re omega: the kernel of section 8, the yardstick
    torch    the complex fields as a torch expression in fp64 (hypot / searchsorted / lerp / broadcast), cast to fp32 and
             copied into the buffer
    fill     Tensor.fill_ of the buffer: the store-bandwidth yardstick of this device on this day

Per leg one JSON line: median / min / max ms over the repeats and GB/s of the median; then the ratios, complex / real and
complex / fill among them, and the time of one es_cyl_complex_vorticity_amplitudes call (one mode, 1 200 radial points).

    python tools/time_cyl_complex_cartesian.py [--repeats 20] [--warmup 3] [--frames 8] [--nxy 267] [--calls 1] [--lib PATH] [--out profiles/cyl_complex_cartesian_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthesis_timing  # noqa: E402  (tools/, beside this file)


def torch_fields(torch, radius, amp, vort, N, m, k, w, x, y, z, t, v_scale, fill, out):
    """Section 20 as broadcast torch expressions, fp64 complex, cast to fp32: region by comparison, bracket by searchsorted
    per region, linear interpolation, the angle factors from atan2, Re[c e^{i (k z - w t)}]."""
    n_r = radius.numel()
    X, Y = x[None, :], y[:, None]
    r = torch.hypot(X, Y)
    inside = (r >= radius[0]) & (r <= radius[N - 1])
    outside = (r > radius[N - 1]) & (r <= radius[n_r - 1])
    valid = (inside | outside) & (r > 0)
    ji = (torch.searchsorted(radius[:N].contiguous(), r, right=True) - 1).clamp(0, N - 2)
    je = N + (torch.searchsorted(radius[N:].contiguous(), r, right=True) - 1).clamp(0, n_r - N - 2)
    j = torch.where(inside, ji, je)
    r0, r1 = radius[j], radius[j + 1]
    frac = (r - r0) / (r1 - r0)
    last = r >= r1
    lerp = lambda a: torch.where(last, a[j + 1], a[j] + (a[j + 1] - a[j]) * frac)      # noqa: E731
    A = {n: lerp(a) for n, a in zip(("xi_r", "xi_phi", "xi_z", "P_T", "v_r", "v_phi", "v_z"), amp)}
    V = {n: lerp(a) for n, a in zip(("W_r", "W_phi", "W_z"), vort)}
    th = torch.atan2(Y.expand_as(r), X.expand_as(r))
    ct, st, cm, sm = X / r, Y / r, torch.cos(m * th), torch.sin(m * th)
    vs = v_scale
    wr, wp = sm * V["W_r"], cm * V["W_phi"]
    coef = [A["P_T"] * cm,
            A["xi_r"] * cm * ct + A["xi_phi"] * sm * st, A["xi_r"] * cm * st - A["xi_phi"] * sm * ct,
            A["xi_z"] * cm,
            vs * (A["v_r"] * cm * ct + A["v_phi"] * sm * st), vs * (A["v_r"] * cm * st - A["v_phi"] * sm * ct),
            vs * A["v_z"] * cm,
            vs * (wr * ct - wp * st), vs * (wr * st + wp * ct), vs * sm * V["W_z"]]
    ph = k * z[None, :, None, None] - w.real * t[:, None, None, None]
    growth = torch.exp(w.imag * t[:, None, None, None])
    EC, ES = growth * torch.cos(ph), growth * torch.sin(ph)
    fill_t = torch.tensor(fill, dtype=torch.float64, device=r.device)
    for i, c in enumerate(coef):
        f = c.real[None, None] * EC - c.imag[None, None] * ES
        out[:, i] = torch.where(valid[None, None], f, fill_t).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    synthesis_timing.add_common_arguments(ap)
    ap.add_argument("--nxy", type=int, default=267, help="points along x and along y (267: the reference's slice)")
    a = ap.parse_args()
    torch, dev, stream, ctx = synthesis_timing.open_context(a)
    import numpy as np
    from eigensolver_amd import CylinderComplex, equilibrium as q, shooting
    k, w, v_scale, fill = 1.2, 3.741567685037965 + 0.05j, 25.0, 0.0
    N, n_ext, n_xy, n_z = 500, 700, a.nxy, 31
    with torch.cuda.stream(stream):
        c = CylinderComplex(q.CylinderDensity(width=0.9, r_sign=1.0, n_nodes=N, ic=(1e-8, 1e-8)), ctx=ctx)
        tab = c.vorticity_amplitudes("kink", [k], [w], n_ext=n_ext)
        radius, amp, vort = (tab[n][0].contiguous() for n in ("radius", "amp", "vort"))
        assert bool(torch.isfinite(torch.view_as_real(amp)).all()) and bool(torch.isfinite(torch.view_as_real(vort)).all()), \
            "the pair is not ES_PT_OK"
        T = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev)    # noqa: E731
        x, y, z = T(np.linspace(-2.0, 2.0, n_xy)), T(np.linspace(-2.0, 2.0, n_xy)), T(np.linspace(0.01, 5.0, n_z))
        t = T(np.linspace(0.01, 2.0 * np.pi, 80)[:a.frames])
        m = int(c.problem("kink").desc.m)
        out = torch.empty((a.frames, 10, n_z, n_xy, n_xy), dtype=torch.float32, device=dev)
        kk = T([k])
        amp_re = amp.real.contiguous()
        vort_re = shooting.vorticity_amplitudes(ctx, radius[None], amp_re[None], N, n_ext, m, kk)[0].contiguous()
    lib, h, P = ctx.lib, ctx.handle, lambda v: v.data_ptr()                  # noqa: E731
    legs = {
        "kernel": lambda: c.cartesian_synthesis(radius, amp, vort, N, n_ext, m, k, w, x, y, z, t, None, v_scale, fill, 0, out=out),
        "real": lambda: shooting.cartesian_synthesis(ctx, radius, amp_re, vort_re, N, n_ext, m, k, w.real, x, y, z, t, None,
                                                     v_scale, fill, 0, out=out),
        "torch": lambda: torch_fields(torch, radius, amp, vort, N, float(m), k, w, x, y, z, t, v_scale, fill, out),
        "fill": lambda: out.fill_(1.0),
        "vorticity_amplitudes": lambda: lib.es_cyl_complex_vorticity_amplitudes(h, P(tab["radius"]), P(tab["amp"]), 1, N, n_ext,
                                                                                m, P(kk), P(tab["vort"])),
    }
    ms, check = synthesis_timing.measure(torch, stream, a, legs, lambda: out[0, :, 3, n_xy // 3])
    top = max(float(amp.abs().max()), float(vort.abs().max())) * v_scale * float(np.exp(abs(w.imag) * float(t.max())))
    synthesis_timing.assert_same_fields(check, top)
    synthesis_timing.report(a, torch.cuda.get_device_name(dev), ms, out.numel() * 4,
                            dict(mesh=[n_xy, n_xy, n_z], variables=10),
                            "vorticity_amplitudes", dict(modes=1, radial_points=N + n_ext))
    med = {n: statistics.median(v) for n, v in ms.items()}
    line = {"mesh": [n_xy, n_xy, n_z], "complex_over_real": round(med["kernel"] / med["real"], 3),
            "complex_over_fill": round(med["kernel"] / med["fill"], 3), "real_over_fill": round(med["real"] / med["fill"], 3)}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    c.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

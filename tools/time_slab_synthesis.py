"""GPU timing aid: the frames of a slab mode (es_slab_field_synthesis) against what a user would write without it and
against the store bandwidth of the device, on one device.

Mesh: 1024 x 512 points in (x, z), all six variables, 8 frames: 8 x 6 x 512 x 1024 float32 = 101 MB per call.  The table is
that of SlabComplexFlow.polarisation at one complex (k, omega) of the Kelvin-Helmholtz slab (width 0.9, "sfx", kink), 500
interior nodes + 2 x 500 exterior points.  Three legs, all writing the same number of bytes into the same buffer, each
between two device events on the context's stream, alternating repeat by repeat in one process so that drift hits all
alike:

    kernel   es_slab_field_synthesis (its (z, t) table pre-pass included)
    torch    the same fields as a torch expression in fp64 (searchsorted / lerp / broadcast), cast to fp32 and copied
             into the buffer
    fill     Tensor.fill_ of the buffer: the store-bandwidth yardstick of this device on this day

Per leg one JSON line: median / min / max ms over the repeats and GB/s of the median; then the ratios kernel / fill and
torch / kernel, and the time of one es_slab_polarisation call (one mode, 1 500 table points, both launches).

    python tools/time_slab_synthesis.py [--repeats 20] [--warmup 3] [--frames 8] [--nx 1024] [--nz 512] [--calls 1] [--lib PATH] [--out profiles/slab_synthesis_timing.jsonl]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthesis_timing  # noqa: E402  (tools/, beside this file)


def torch_fields(torch, xtab, amp, N, n_ext, k, w, x, z, t, v_scale, fill, out):
    """Section 9's synthesis as broadcast torch expressions, fp64, cast to fp32: region by comparison, bracket by
    searchsorted per region, linear interpolation of the real and the imaginary part."""
    xm, xp = xtab[n_ext], xtab[n_ext + N - 1]
    inside = (x >= xm) & (x <= xp)
    left = (x >= xtab[0]) & (x < xm)
    right = (x > xp) & (x <= xtab[-1])
    valid = inside | left | right
    jl = (torch.searchsorted(xtab[:n_ext].contiguous(), x, right=True) - 1).clamp(0, n_ext - 2)
    ji = n_ext + (torch.searchsorted(xtab[n_ext:n_ext + N].contiguous(), x, right=True) - 1).clamp(0, N - 2)
    jr = n_ext + N + (torch.searchsorted(xtab[n_ext + N:].contiguous(), x, right=True) - 1).clamp(0, n_ext - 2)
    j = torch.where(inside, ji, torch.where(left, jl, jr))
    x0, x1 = xtab[j], xtab[j + 1]
    frac = (x - x0) / (x1 - x0)
    last = x >= x1
    ph = k * z[None, :, None] - w.real * t[:, None, None]
    E = torch.exp(w.imag * t)[:, None, None]
    EC, ES = E * torch.cos(ph), E * torch.sin(ph)
    fill_t = torch.tensor(fill, dtype=torch.float64, device=x.device)
    for i in range(6):
        s = v_scale if i >= 3 else 1.0                                       # v_x, v_z, vort_y
        re, im = amp[i].real, amp[i].imag
        a_re = torch.where(last, re[j + 1], re[j] + (re[j + 1] - re[j]) * frac) * s
        a_im = torch.where(last, im[j + 1], im[j] + (im[j + 1] - im[j]) * frac) * s
        f = a_re[None, None] * EC - a_im[None, None] * ES
        out[:, i] = torch.where(valid[None, None], f, fill_t).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    synthesis_timing.add_common_arguments(ap)
    ap.add_argument("--nx", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=512)
    a = ap.parse_args()
    torch, dev, stream, ctx = synthesis_timing.open_context(a)
    import numpy as np
    from eigensolver_amd import SlabComplexFlow, shooting
    k, w, v_scale, fill = 0.5, 0.2 + 0.1j, 25.0, 0.0
    N, n_ext, n_x, n_z = 500, 500, a.nx, a.nz
    with torch.cuda.stream(stream):
        flow = SlabComplexFlow(width=0.9, variant="sfx", n_nodes=N, ctx=ctx)
        cand = np.array([w, 0.35 - 0.05j, 0.1 + 0.2j, 0.5 + 0.02j])            # the first bound (ES_PT_OK) pair of these
        w = complex(cand[flow.eval_points("kink", k, cand)[1].cpu().numpy() == 0][0])
        tab = flow.polarisation("kink", k, [w], n_ext=n_ext)
        xtab, amp = tab["x"][0].contiguous(), tab["amp"][0].contiguous()
        assert int(tab["status"][0]) == 0 and bool(torch.isfinite(torch.view_as_real(amp)).all()), "the pair is not ES_PT_OK"
        T = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev)    # noqa: E731
        R = float(xtab[-1])
        x, z = T(np.linspace(-1.02 * R, 1.02 * R, n_x)), T(np.linspace(0.0, 4.0 * np.pi / k, n_z))
        t = T(np.linspace(0.0, 2.0 * np.pi / abs(w.real), 80)[:a.frames])
        out = torch.empty((a.frames, 6, n_z, n_x), dtype=torch.float32, device=dev)
        eig = flow.eigenfunction("kink", k, [w], n_ext=n_ext)
        p = flow.problem("kink")
        prof = p.slab_field_profiles()
        kk, wre, wim = T([k]), T([w.real]), T([w.imag])
        d = p.desc
    legs = {
        "kernel": lambda: shooting.slab_field_synthesis(ctx, xtab, amp, N, n_ext, k, w, x, z, t, None, v_scale, fill, 0,
                                                        out=out),
        "torch": lambda: torch_fields(torch, xtab, amp, N, n_ext, k, w, x, z, t, v_scale, fill, out),
        "fill": lambda: out.fill_(1.0),
        "polarisation": lambda: shooting.slab_polarisation(ctx, kk, wre, wim, eig, prof, d.rho_e, d.vA_e, d.c_e, d.U_e,
                                                           int(d.slab_mode), 0),
    }
    ms, check = synthesis_timing.measure(torch, stream, a, legs, lambda: out[:, :, n_z // 3])
    synthesis_timing.assert_same_fields(check, float(amp.abs().max()) * v_scale * float(np.exp(abs(w.imag) * float(t.max()))))
    synthesis_timing.report(a, torch.cuda.get_device_name(dev), ms, out.numel() * 4, dict(mesh=[n_x, n_z], variables=6),
                            "polarisation", dict(modes=1, table_points=N + 2 * n_ext))
    flow.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""GPU timing aid: the field synthesis of a cylinder mode (es_cyl_field_synthesis) against what a user would write
without it and against the store bandwidth of the device, on one device.

Mesh: the reference's own (Export_vtk.py:598, :180, :893-897): 1 200 radii (500 interior nodes + 700 exterior points) x
60 angles x 16 heights, the ten `varlist` variables, chunks of 8 frames: 8 x 10 x 16 x 60 x 1 200 float32 = 369 MB per
call.  The amplitude table is that of ShootProblem.polarisation at one (k, omega) of the coronal density cylinder
(width 0.9).  Three legs, all writing the same number of bytes into the same buffer, each between two device events on
the context's stream, alternating repeat by repeat in one process so that drift hits all alike:

    kernel   es_cyl_field_synthesis (points not requested)
    torch    the same fields as a broadcast torch expression in fp64, cast to fp32 and copied into the buffer
    fill     Tensor.fill_ of the buffer: the store-bandwidth yardstick of this device on this day

Per leg one JSON line: median / min / max ms over the repeats and GB/s of the median; then the ratios kernel / fill and
torch / kernel, and the time of one ShootProblem.polarisation call (es_shoot_eigenfunction + es_cyl_polarisation for one
mode, 1 200 radial points).

    python tools/time_field_synthesis.py [--repeats 20] [--warmup 3] [--frames 8] [--calls 1] [--lib PATH] [--out profiles/field_synthesis_timing.jsonl]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthesis_timing  # noqa: E402  (tools/, beside this file)

VARLIST = ["xi_r", "xi_phi", "P_T", "v_r", "v_phi", "xi_x", "xi_y", "v_x", "v_y", "v_z"]      # Export_vtk.py:986 less density


def torch_fields(torch, radius, amp, m, k, w, theta, z, t, v_scale, out):
    """The loop body of Export_vtk.py:934-946 as broadcast expressions, fp64, cast to fp32 (z-components with -sin)."""
    A = dict(zip(("xi_r", "xi_phi", "xi_z", "P_T", "v_r", "v_phi", "v_z"), amp))
    th = theta[None, None, :, None]
    C = torch.cos(k * z[None, :, None, None] - w * t[:, None, None, None])
    cm, sm = torch.cos(m * th), -torch.sin(m * th)
    c1, s1 = torch.cos(th), torch.sin(th)
    R = lambda a: a[None, None, None, :]                                     # noqa: E731
    xi_r, xi_phi = R(A["xi_r"]) * cm * C, R(A["xi_phi"]) * sm * C
    v_r, v_phi = v_scale * R(A["v_r"]) * cm * C, v_scale * R(A["v_phi"]) * sm * C
    f = [xi_r, xi_phi, R(A["P_T"]) * cm * C, v_r, v_phi, xi_r * c1 - xi_phi * s1, xi_r * s1 + xi_phi * c1,
         v_r * c1 - v_phi * s1, v_r * s1 + v_phi * c1, v_scale * R(A["v_z"]) * sm * C]
    for i, a in enumerate(f):
        out[:, i] = a.to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    synthesis_timing.add_common_arguments(ap)
    a = ap.parse_args()
    torch, dev, stream, ctx = synthesis_timing.open_context(a)
    import numpy as np
    from eigensolver_amd import ShootProblem, _lib, equilibrium as q, shooting
    k, w, v_scale = 1.2, 3.741567685037965, 25.0
    with torch.cuda.stream(stream):
        gp = ShootProblem(q.CylinderDensity(width=0.9, r_sign=1.0, n_nodes=500, ic=(1e-8, 1e-8)), "kink", ctx=ctx)
        pol = gp.polarisation([k], [w], n_ext=700)
        radius, amp = pol["radius"][0].contiguous(), pol["amp"][0].contiguous()
        assert bool(torch.isfinite(amp).all()), "the mode is not ES_PT_OK"
        T = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev)    # noqa: E731
        theta, z = T(np.linspace(0.0, 2.0 * np.pi, 60)), T(np.linspace(0.01, 5.0, 16))
        t = T(np.linspace(0.01, 2.0 * np.pi, 80)[:a.frames])
        n_r, m = radius.numel(), int(gp.desc.m)
        out = torch.empty((a.frames, len(VARLIST), 16, 60, n_r), dtype=torch.float32, device=dev)
    flags = _lib.FIELD_Z_REFERENCE_ANGLE
    legs = {
        "kernel": lambda: shooting.field_synthesis(ctx, radius, amp, m, k, w, theta, z, t, VARLIST, v_scale, flags,
                                                   want_points=False, out=out),
        "torch": lambda: torch_fields(torch, radius, amp, float(m), k, w, theta, z, t, v_scale, out),
        "fill": lambda: out.fill_(1.0),
        "polarisation": lambda: gp.polarisation([k], [w], n_ext=700),
    }
    ms, check = synthesis_timing.measure(torch, stream, a, legs, lambda: out[0, :, 3, 7])
    synthesis_timing.assert_same_fields(check, float(amp.abs().max()) * v_scale)
    synthesis_timing.report(a, torch.cuda.get_device_name(dev), ms, out.numel() * 4,
                            dict(mesh=[n_r, 60, 16], variables=len(VARLIST)),
                            "polarisation", dict(modes=1, radial_points=n_r))
    gp.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

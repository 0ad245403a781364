"""GPU timing aid for C ABI section 12 (slopes and Newton tracing of complex roots of the flow slab), on one device.

Two comparisons, each leg between two device events on the context's stream, the legs of a comparison alternating repeat by
repeat in one process so that drift hits all alike, every buffer allocated before anything is timed:

  slopes     n = 2^15 pairs around the Kelvin-Helmholtz branch of the sheared slab (width 0.9, kink, "sfx", N = 500):
      slopes        es_complex_root_slopes: value, d/d omega and d/dk of both sides in one march of 3-component complex jets
      stencil       ONE es_complex_eval_points on 5 n pairs: the centre, omega +- h and k +- h -- the central differences one
                    would otherwise take (h = 2^-10; beside a critical layer no step is safe)
      eval_points   ONE es_complex_eval_points on the n pairs -- the scale of the call, not a target
      eigenfunction es_complex_eigenfunction on the first 2^12 of the pairs with n_ext = 2: the adjoint march, the forward
                    march that writes every node and the exterior kernel -- with it every kernel that runs the formulas of
                    es_complex_shared.hpp has a timed leg
  densify    the unstable branch of the uniform-flow slab (kink, "sfx", N = 500) at 256 wavenumbers in [0.3, 0.6]:
      scan          the path without slopes: es_complex_eval_grid + es_complex_find_roots at the 256 rows on the 16 x 12
                    window of tests/complex_eigen_model.py (12 secant steps per flagged cell; the call reads its count back)
      densify       SlabComplexFlow.densify from 9 coarse rows (their roots by the scan path, before the clock starts):
                    slopes at 9 roots, the Hermite prediction in torch, one es_complex_newton over the 256 points
  Before timing, the roots of the two densify legs are compared row by row.

--lib: another build of the library.  One that lacks section 12 times the `eval_points`, `stencil`, `eigenfunction` and
`scan` legs only -- its line is the scan path's timing before that section existed.

    python tools/time_complex_slopes.py [--repeats 20] [--warmup 3] [--lib PATH] [--out profiles/complex_slopes_timing.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

STEP = 2.0 ** -10
KH_ROOT = 0.3128068480162605 + 0.09428139628771133j          # kink, uniform flow, k = 0.5


def load_library(path):
    """(library, has_section_12) of another build; the signatures of the sections it has are set"""
    import torch  # noqa: F401
    from eigensolver_amd import _lib
    lib = ctypes.CDLL(path)
    has = hasattr(lib, "es_complex_newton")
    try:
        _lib._sig(lib)
    except AttributeError:
        assert not has
    return lib, has


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


def unstable_root_per_row(roots, nk):
    """the accepted root of largest Im omega of every row of a find_roots table -> complex array [nk] (NaN: none)"""
    w, row, flag = (roots[f].cpu().numpy() for f in ("w", "row", "flag"))
    out = np.full(nk, np.nan + 0j)
    for i in np.nonzero(flag == 1)[0]:
        if np.isnan(out[row[i]]) or w[i].imag > out[row[i]].imag:
            out[row[i]] = w[i]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=15)
    ap.add_argument("--nodes", type=int, default=500)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_slopes_timing.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import torch
    from eigensolver_amd import SlabComplexFlow, _lib
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    lib, full = load_library(a.lib) if a.lib else (None, True)
    ctx = _lib.Context(dev.index or 0, stream=stream, lib=lib)
    lib, P = ctx.lib, _lib.ptr
    n = 1 << a.log2n
    line = {"device": torch.cuda.get_device_name(dev), "lib": os.path.basename(a.lib) if a.lib else "default",
            "section_12": full, "nodes": a.nodes, "repeats": a.repeats, "warmup": a.warmup}

    # ---- slopes against the stencil --------------------------------------------------------------------------------------
    with torch.cuda.stream(stream):
        s = SlabComplexFlow(width=0.9, variant="sfx", ctx=ctx, n_nodes=a.nodes)
        p = s.problem("kink")
        g = torch.Generator(device="cpu").manual_seed(12)
        k = (0.3 + 0.4 * torch.rand(n, generator=g, dtype=torch.float64)).to(dev)
        wre = (2.0 * KH_ROOT.real * k.cpu() + 0.05 * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        wim = (KH_ROOT.imag + 0.05 * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        fk = torch.tensor([0, 0, 0, 1, -1], dtype=torch.float64, device=dev)[:, None] * STEP
        fw = torch.tensor([0, 1, -1, 0, 0], dtype=torch.float64, device=dev)[:, None] * STEP
        k5 = (k[None, :] + fk).reshape(-1).contiguous()
        wre5 = (wre[None, :] + fw).reshape(-1).contiguous()
        wim5 = wim.repeat(5).contiguous()
        outer = torch.empty((3, n), dtype=torch.complex128, device=dev)
        inner = torch.empty((3, n), dtype=torch.complex128, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        D5 = [torch.empty(5 * n, dtype=torch.float64, device=dev) for _ in range(2)]
        st5 = torch.empty(5 * n, dtype=torch.uint8, device=dev)
        D1 = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)]
        st1 = torch.empty(n, dtype=torch.uint8, device=dev)
        ne, n_ext = min(n, 1 << 12), 2
        vi, fi = (torch.empty((ne, a.nodes), dtype=torch.complex128, device=dev) for _ in range(2))
        xe = torch.empty((ne, n_ext), dtype=torch.float64, device=dev)
        ve, fe = (torch.empty((ne, n_ext), dtype=torch.complex128, device=dev) for _ in range(2))
        ste = torch.empty(ne, dtype=torch.uint8, device=dev)

    def slopes():
        _lib.check(ctx.handle, lib.es_complex_root_slopes(ctx.handle, p.handle, s.variant, P(k), P(wre), P(wim), n, None,
                                                          P(outer), P(inner), P(st)))

    def stencil():
        _lib.check(ctx.handle, lib.es_complex_eval_points(ctx.handle, p.handle, s.variant, P(k5), P(wre5), P(wim5), 5 * n,
                                                          P(D5[0]), P(D5[1]), None, P(st5)))

    def eval_points():
        _lib.check(ctx.handle, lib.es_complex_eval_points(ctx.handle, p.handle, s.variant, P(k), P(wre), P(wim), n, P(D1[0]),
                                                          P(D1[1]), None, P(st1)))

    def eigenfunction():
        _lib.check(ctx.handle, lib.es_complex_eigenfunction(ctx.handle, p.handle, s.variant, P(k), P(wre), P(wim), ne, P(vi),
                                                            P(fi), n_ext, P(xe), P(ve), P(fe), P(ste)))

    legs = {"stencil": stencil, "eval_points": eval_points, "eigenfunction": eigenfunction}
    if full:
        legs = {"slopes": slopes, **legs}
    with torch.cuda.stream(stream):
        for run in legs.values():
            run()
        if full:
            S5 = torch.complex(D5[0], D5[1]).reshape(5, n)
            ok = (st == 0) & (st5.reshape(5, n) == 0).all(dim=0)
            d = outer - inner
            scale = torch.maximum(outer[0].abs(), inner[0].abs())
            line["pairs_ok"] = int(ok.sum().item())
            line["value_vs_eval_points"] = float(((d[0] - torch.complex(D1[0], D1[1])).abs() / scale)[ok].max().item())
            slope, slope5 = -d[2] / d[1], -(S5[3] - S5[4]) / (S5[1] - S5[2])
            diff = ((slope - slope5).abs() / slope.abs().clamp(min=1.0))[ok]
            line["slope_vs_stencil_median"], line["slope_vs_stencil_max"] = float(diff.median().item()), float(diff.max().item())
    line["pairs"], line["stencil_step"], line["eigenfunction_pairs"] = n, STEP, ne
    line["slopes_legs"] = timed(torch, stream, a, legs)

    # ---- densify against the scan ----------------------------------------------------------------------------------------
    nk = 256
    w_re, w_im = np.linspace(-0.25, 0.5, 16), np.linspace(-0.25, 0.25, 12)
    with torch.cuda.stream(stream):
        u = SlabComplexFlow(width=1e5, variant="sfx", ctx=ctx, n_nodes=a.nodes)
        kf = torch.linspace(0.3, 0.6, nk, dtype=torch.float64, device=dev)
        kc = torch.linspace(0.3, 0.6, 9, dtype=torch.float64, device=dev)
        Dc, stc, _ = u.eval_grid("kink", kc, w_re, w_im)
        coarse = unstable_root_per_row(u.find_roots("kink", kc, w_re, w_im, Dc, stc)[0], 9)
        assert np.isfinite(coarse).all(), "the scan found no unstable root in a coarse row"
        wc = torch.as_tensor(coarse, device=dev)

    def scan():
        D, stg, _ = u.eval_grid("kink", kf, w_re, w_im)
        return u.find_roots("kink", kf, w_re, w_im, D, stg, capacity=4096)[0]

    def densify():
        return u.densify("kink", kc, wc, kf)

    legs = {"scan": scan}
    if full:
        legs["densify"] = densify
    with torch.cuda.stream(stream):
        ref = unstable_root_per_row(scan(), nk)
        line["scan_rows_with_root"] = int(np.isfinite(ref).sum())
        if full:
            dd = densify()
            got, flag = dd["w"].cpu().numpy(), dd["flag"].cpu().numpy()
            line["densify_flags"] = int(flag.sum())
            line["densify_iters_max"] = int(dd["iters"].max().item())
            line["densify_vs_scan_max"] = float(np.nanmax(np.abs(got - ref)))
            line["densify_resid_max_percent"] = float(dd["resid"].max().item())
            line["scan_resid_note"] = "the scan's roots are 12 secant steps from a cell centre"
    line["fine_rows"], line["coarse_rows"], line["window"] = nk, 9, [16, 12]
    line["densify_legs"] = timed(torch, stream, a, legs)
    if full:
        sl, dl = line["slopes_legs"], line["densify_legs"]
        line["slopes_over_stencil"] = round(sl["slopes"]["median_ms"] / sl["stencil"]["median_ms"], 3)
        line["slopes_over_eval_points"] = round(sl["slopes"]["median_ms"] / sl["eval_points"]["median_ms"], 2)
        line["scan_over_densify"] = round(dl["scan"]["median_ms"] / dl["densify"]["median_ms"], 2)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    s.close()
    u.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

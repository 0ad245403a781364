"""GPU A/B of two builds of the library on the complex-frequency paths: the same calls on the same small inputs must give the
same numbers.  Written for changes to the complex scalar esb::cz, the complex jet esb::CJet and the texts built on them.

    python tools/compare_complex_builds.py --lib-a PATH --lib-b PATH [--time 5] [--out profiles/NAME.jsonl]

Prints, per call and output array, the number of elements that differ, and exits non-zero on any difference.  Two elements
are equal when they compare equal as numbers (so +0 and -0 are equal) or are both NaN; integer and status arrays compare
exactly.  A call that the library refuses counts by its error text.  No reference tree and no golden file: build A is the
reference of build B.

The inputs are the smallest at which these kernels can go wrong, not a workload:
  flow slab (SlabComplexFlow)   "sfx" and "sfg", kink and sausage, a sheared (width 0.9) and a uniform (width 1e5) jet;
      n_nodes 3, 129 and 130 (the LDS chunk is 128 steps: two steps, exactly one chunk, a second chunk of one step); three
      wavenumbers; frequencies with Im omega > 0, on the real axis, in the leaky region (Re m_e < 0) and at omega = k U_e
      (division by zero), so that every status is produced.  eval_points at n = 1, 64, 65; eval_grid on 3 x 4 x 5;
      find_roots on the 16 x 12 window around the Kelvin-Helmholtz root; eigenfunction with n_ext 3 and 8; root_slopes and
      newton at n = 65 under a device count word of 37 (the entries past the count are left as allocated and are not
      compared), newton with max_iter 0 and 8 and with a finite step_cap; polarisation and one frame of fields.
  real slab fields (ShootProblem.slab_polarisation, slab_fields)   a density slab and a flow slab, two pairs each.
  complex cylinder, untwisted and twisted   eval_points (with both sides), find_roots, root_slopes, newton, eigenfunction
      and polarisation at the same sizes.
  Cartesian sampling, real and complex (sections 8 and 20)   the vorticity amplitudes on tables of (3, 0), (0, 3), (3, 3)
      and (64, 65) points, m = 0, 1, 3, and with a NaN node; the synthesis on the five small meshes of the GPU tests (one
      live lane, the ragged narrow path, the wide path) and the 73 x 70 x 137 x 3 split, into an aligned output and one
      4 bytes past a 16-byte boundary, every variable, two of them and two without a vorticity table, both byte orders,
      Im omega > 0, < 0 and = 0, and the mesh of ties, origin, hole, far field and NaN with three fill values.  Frames
      compare as 32-bit patterns, sentinels around them included.

--time R: after the comparison, R timed passes per build over the flow-slab calls, the builds alternating pass by pass in
this one process; the line (per build: seconds of every pass, calls per pass, median milliseconds per call, over all calls
and by kind of call) is printed and, with --out, appended to that file.  The calls are tiny and latency-bound, each ends with a copy to the host: the figure
is what a call costs, not a throughput.
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

NODES = (3, 129, 130)
COUNT = 37
SLAB_K = np.array([0.3, 0.5, 0.6])
# growing, decaying, real axis, leaky (real and complex), omega = k U_e = 0
SLAB_W = np.array([0.3128 + 0.0943j, 0.21 + 0.05j, 0.4 - 0.07j, 0.45 + 0.0j, 0.1 + 0.0j, 5.0 + 0.0j, 5.0 + 0.1j, 0.0 + 0.0j,
                   0.35 + 0.2j, -0.2 + 0.02j, 0.33 + 1e-9j, 2.0 + 0.5j, 0.05 + 0.3j])
KH = dict(c_i0=1.0, vA_i0=2.0, c_e=1.5, vA_e=0.5, U_i0=3.0, width=1.5, r_sign=1.0)          # tools/time_cyl_complex_fields.py
CASE_A = dict(v_twist=2.0, power=1.0, r_axis=1e-2)                                          # tools/time_cylt_complex.py


def host(x):
    """a call's result as {name: numpy array}: tensors, tuples, named tuples and dicts of them"""
    import torch
    if isinstance(x, torch.Tensor):
        return {"": x.cpu().numpy()}
    if isinstance(x, dict):
        items = x.items()
    elif hasattr(x, "_fields"):
        items = zip(x._fields, x)
    elif isinstance(x, (tuple, list)):
        items = enumerate(x)
    else:
        return {"": np.asarray(x)}
    out = {}
    for name, v in items:
        if v is None or name == "names":                               # the variable names of a fields() dict
            continue
        for sub, a in host(v).items():
            out[f"{name}.{sub}" if sub else str(name)] = a
    return out


def points(n, k_values, w_values):
    """n (k, omega) pairs: the frequencies in turn, every pass a little further out, the wavenumbers in turn"""
    j = np.arange(n)
    return k_values[j % len(k_values)], w_values[j % len(w_values)] * (1.0 + 0.01 * (j // len(w_values)))


def counted(res, keep):
    """the entries of a counted call that the library wrote: the first COUNT along the last axis"""
    return {name: a[..., :keep] for name, a in host(res).items()}


def slab_calls(ctx, keep_open):
    """[(label, closure)] over the flow slab; the problems stay open in keep_open"""
    import torch
    from eigensolver_amd import SlabComplexFlow
    dev = f"cuda:{ctx.device}"
    count = torch.tensor([COUNT], dtype=torch.int32, device=dev)
    k65, w65 = points(65, SLAB_K, SLAB_W)
    g_re, g_im = np.linspace(-0.25, 0.5, 16), np.linspace(-0.25, 0.25, 12)
    calls = []
    for variant in ("sfx", "sfg"):
        for width in (0.9, 1e5):
            for n_nodes in NODES:
                s = SlabComplexFlow(width=width, variant=variant, ctx=ctx, n_nodes=n_nodes)
                keep_open.append(s)
                for mode in ("kink", "sausage"):
                    tag = f"slab {variant} width={width:g} N={n_nodes} {mode}"

                    def add(name, f, tag=tag):
                        calls.append((f"{tag} {name}", f))

                    for n in (1, 64, 65):
                        add(f"eval_points n={n}", lambda s=s, mode=mode, n=n: host(s.eval_points(mode, k65[:n], w65[:n])))
                    add("eval_grid 3x4x5", lambda s=s, mode=mode: host(
                        s.eval_grid(mode, SLAB_K, np.linspace(-0.25, 0.5, 5), np.linspace(-0.1, 0.25, 4))))

                    def find(s=s, mode=mode):
                        D, st, rel = s.eval_grid(mode, SLAB_K, g_re, g_im)
                        roots, total = s.find_roots(mode, SLAB_K, g_re, g_im, D, st)
                        return {**host(roots), "total": np.array([total])}
                    add("find_roots 3x12x16", find)
                    for n_ext in (3, 8):
                        add(f"eigenfunction n_ext={n_ext}",
                            lambda s=s, mode=mode, n_ext=n_ext: host(s.eigenfunction(mode, k65, w65, n_ext=n_ext)))
                    add("root_slopes n=65 count=37", lambda s=s, mode=mode: counted(s.root_slopes(mode, k65, w65, count=count), COUNT))
                    for kw in (dict(max_iter=0), dict(max_iter=8), dict(max_iter=8, step_cap=0.05)):
                        add(f"newton n=65 count=37 {kw}",
                            lambda s=s, mode=mode, kw=kw: counted(s.newton(mode, k65, w65, count=count, **kw), COUNT))
                    for quirks in ((True, False) if variant == "sfg" else (True,)):
                        add(f"polarisation n_ext=3 quirks={quirks}", lambda s=s, mode=mode, quirks=quirks: host(
                            s.polarisation(mode, k65[:5], w65[:5], n_ext=3, reference_quirks=quirks)))
                    add("fields one frame", lambda s=s, mode=mode: host(
                        s.fields(mode, 0.5, SLAB_W[0], np.linspace(-1.5, 1.5, 7), np.linspace(0.0, 2.0, 3), [0.3], n_ext=3)))
    return calls


def real_slab_calls(ctx, keep_open):
    from eigensolver_amd import ShootProblem, equilibrium as q
    calls = []
    for name, eq, (k, w) in (("density", q.SlabDensity(width=0.9, n_nodes=64), (1.5, 1.65)),
                             ("flow", q.SlabFlow(width=0.9, U_i0=0.35, n_nodes=64), (1.2, 1.92))):
        for mode in ("kink", "sausage"):
            p = ShootProblem(eq, mode, ctx=ctx)
            keep_open.append(p)
            ks, ws = [k, 0.9 * k], [w, 0.9 * w]
            for quirks in (True, False):
                calls.append((f"real slab {name} {mode} slab_polarisation quirks={quirks}", lambda p=p, ks=ks, ws=ws, quirks=quirks: host(
                    p.slab_polarisation(ks, ws, n_ext=3, reference_quirks=quirks))))
            calls.append((f"real slab {name} {mode} slab_fields one frame", lambda p=p, k=k, w=w: host(
                p.slab_fields(k, w, np.linspace(-1.5, 1.5, 7), np.linspace(0.0, 2.0, 3), [0.3], n_ext=3))))
    return calls


def cylinder_calls(ctx, keep_open):
    import torch
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex, equilibrium as q
    from eigensolver_amd.shooting import W_ABSOLUTE, W_PHASE_SPEED
    dev = f"cuda:{ctx.device}"
    count = torch.tensor([COUNT], dtype=torch.int32, device=dev)
    families = (
        ("cyl", lambda N: CylinderComplex(q.CylinderFlow(**KH, n_nodes=N), ctx=ctx), None, np.array([1.5, 2.0, 2.5]),
         np.array([2.673525 + 0.084845j, 2.5 + 0.2j, 2.6 + 0.0j, 10.0 + 0.0j, 10.0 + 0.3j, 2.8 - 0.1j, 0.0 + 0.0j, 3.1 + 0.05j]),
         (np.linspace(1.0, 1.6, 13), np.linspace(0.005, 0.105, 11), W_PHASE_SPEED)),
        ("cylt", lambda N: RotatingCylinderComplex(q.CylinderRotation(**CASE_A, n_nodes=N), ctx=ctx), 3, np.array([0.85, 1.0, 1.1]),
         np.array([1.555 + 0.792j, 1.4 + 0.6j, 1.5 + 0.0j, 10.0 + 0.0j, 10.0 + 0.3j, 1.7 - 0.2j, 0.0 + 0.0j, 1.8 + 1.0j]),
         (np.linspace(1.2, 1.9, 8), np.linspace(0.45, 1.15, 8), W_ABSOLUTE)),
    )
    calls = []
    for fam, make, m, kv, wv, (g_re, g_im, w_mode) in families:
        k65, w65 = points(65, kv, wv)
        for n_nodes in NODES:
            c = make(n_nodes)
            keep_open.append(c)
            tag = f"{fam} N={n_nodes} kink m={m}"

            def add(name, f, tag=tag):
                calls.append((f"{tag} {name}", f))

            for n in (1, 64, 65):
                add(f"eval_points n={n}", lambda c=c, n=n, m=m: host(c.eval_points("kink", k65[:n], w65[:n], m=m, parts=True)))

            def find(c=c, m=m, kv=kv, g_re=g_re, g_im=g_im, w_mode=w_mode):
                D, st, rel = c.eval_grid("kink", kv, g_re, g_im, w_mode, m=m)
                roots, total = c.find_roots("kink", kv, g_re, g_im, D, st, w_mode, m=m)
                return {**host((D, st, rel)), **host(roots), "total": np.array([total])}
            add("eval_grid + find_roots", find)
            add("root_slopes n=65 count=37", lambda c=c, m=m: counted(c.root_slopes("kink", k65, w65, count=count, m=m), COUNT))
            for kw in (dict(max_iter=0), dict(max_iter=8), dict(max_iter=8, step_cap=0.05)):
                add(f"newton n=65 count=37 {kw}", lambda c=c, m=m, kw=kw: counted(c.newton("kink", k65, w65, count=count, m=m, **kw), COUNT))
            for n_ext in (3, 8):
                add(f"eigenfunction n_ext={n_ext}", lambda c=c, m=m, n_ext=n_ext: host(c.eigenfunction("kink", k65, w65, n_ext=n_ext, m=m)))
            add("polarisation n_ext=3", lambda c=c, m=m: host(c.polarisation("kink", k65[:5], w65[:5], n_ext=3, m=m)))
    return calls


def cartesian_calls(ctx):
    """Cartesian sampling, real (section 8) and complex (section 20): the two vorticity-amplitude and the two synthesis
    calls on the shapes of tests/test_cartesian_gpu.py and tests/test_cyl_complex_cartesian_gpu.py.  Frames are returned
    as their 32-bit patterns, so that they compare exactly; the tables are finite, so every NaN in a frame is the fill."""
    import torch
    from eigensolver_amd import _lib, cyl_complex, shooting
    from tests.cyl_complex_cartesian_model import complex_table
    dev = f"cuda:{ctx.device}"
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)    # noqa: E731
    families = (("real", shooting, lambda a: np.ascontiguousarray(a.real), (3.7,)),
                ("complex", cyl_complex, lambda a: a, (3.7 + 0.6j, 3.7 - 0.6j, 3.7 + 0j)))
    meshes = [(1, 1, 1, 1), (5, 3, 2, 1), (64, 2, 1, 2), (257, 3, 2, 2), (66, 6, 3, 1)]
    masks = (("all", None, True), ("v_x+vort_y", ["v_x", "vort_y"], True), ("P_T+v_y no vort", ["P_T", "v_y"], False))
    calls = []

    def frames(mod, tabs, m, k, w, mesh, variables, v_scale, fill, flags, offset):
        """one synthesis call into a buffer that starts `offset` floats past a 16-byte boundary, sentinels around it"""
        shape = (len(mesh[3]), len(shooting.cartesian_var_mask(variables)[1]), len(mesh[2]), len(mesh[1]), len(mesh[0]))
        total = int(np.prod(shape))
        buf = torch.full((total + 12,), -777.0, dtype=torch.float32, device=dev)
        off = ((16 - buf.data_ptr() % 16) % 16) // 4 + 4 + offset
        out = buf[off:off + total].view(shape)
        assert out.data_ptr() % 16 == 4 * offset
        mod.cartesian_synthesis(ctx, *tabs, m, k, w, *(T(a) for a in mesh), variables, v_scale, fill, flags, out=out)
        return {"frames": buf.view(torch.int32).cpu().numpy()}

    def modes(part, n_nodes, n_ext, n):
        rad, amp = zip(*[complex_table(n_nodes, n_ext, seed=7 + i) for i in range(n)])
        return np.stack(rad), part(np.stack(amp) * (1.0 + 0.5 * np.arange(n))[:, None, None]), 0.9 + 0.6 * np.arange(n)

    def synth_group(tag, mod, part, ws, n_nodes, n_ext, m, k, mesh, mask_set, v_scale, fills):
        radius, amp = complex_table(n_nodes, n_ext)
        d_radius, d_amp = T(radius), T(part(amp))
        d_vort = mod.vorticity_amplitudes(ctx, d_radius[None], d_amp[None], n_nodes, n_ext, m, T(np.array([k])))[0].contiguous()
        for w in ws:
            for mname, variables, with_vort in mask_set:
                tabs = (d_radius, d_amp, d_vort if with_vort else None, n_nodes, n_ext)
                for fill in fills:
                    for flags in (0, _lib.FIELD_BIG_ENDIAN):
                        for offset in (0, 1):
                            calls.append((f"{tag} w={w} {mname} fill={fill} flags={flags} offset={offset}",
                                          lambda mod=mod, tabs=tabs, w=w, variables=variables, fill=fill, flags=flags,
                                          offset=offset: frames(mod, tabs, m, k, w, mesh, variables, v_scale, fill, flags, offset)))

    for fam, mod, part, ws in families:
        for n_nodes, n_ext in ((3, 0), (0, 3), (3, 3), (64, 65)):
            for m in (0, 1, 3):
                tag = f"cart {fam} N={n_nodes} n_ext={n_ext} m={m}"
                calls.append((f"{tag} vorticity_amplitudes n=3", lambda mod=mod, part=part, n_nodes=n_nodes, n_ext=n_ext, m=m: host(
                    mod.vorticity_amplitudes(ctx, *(T(a) for a in modes(part, n_nodes, n_ext, 3)[:2]), n_nodes, n_ext, m,
                                             T(modes(part, n_nodes, n_ext, 3)[2])))))
                for shape in meshes:
                    mesh = tuple(np.linspace(lo, hi, n) for (lo, hi), n in
                                 zip(((-1.7, 1.9), (-1.6, 1.45), (0.1, 2.3), (0.01, 1.7)), shape))
                    synth_group(f"{tag} synthesis {shape}", mod, part, ws, n_nodes, n_ext, m, 1.3, mesh, masks, 2.5, (-7.5,))
        # several planes per piece, several items per workgroup, a group across two frames
        mesh = (np.linspace(-1.7, 1.9, 73), np.linspace(-1.6, 1.45, 70), np.linspace(0.0, 4.0, 137), np.array([0.01, 0.8, 1.7]))
        synth_group(f"cart {fam} N=64 n_ext=65 m=2 synthesis (73, 70, 137, 3)", mod, part, ws, 64, 65, 2, 1.3, mesh,
                    (("xi_z+v_x+vort_y", ["xi_z", "v_x", "vort_y"], True),), 2.5, (-7.5,))
        # ties on r == r_b, the origin, the hole, the far field and a NaN coordinate
        mesh = (np.array([-1.0, 0.0, 1.0, 0.05, 3.5, np.nan]), np.array([-1.0, 0.0, 1.0]), np.array([0.0]), np.array([0.0]))
        synth_group(f"cart {fam} N=7 n_ext=6 m=0 ties", mod, part, (2.0 + 0.3j,) if fam == "complex" else (2.0,), 7, 6, 0, 1.0,
                    mesh, masks[:1], 1.5, (float("nan"), 0.0, -7.5))
        # a NaN node reaches the nodes whose stencil holds it
        for h in range(2 if fam == "complex" else 1):
            def nan_node(mod=mod, part=part, h=h):
                radius, amp, k = modes(lambda a: a, 64, 65, 1)
                for j in (2, 64 + 30):
                    (amp.real if h == 0 else amp.imag)[0, :, j] = np.nan
                return host(mod.vorticity_amplitudes(ctx, T(radius), T(part(amp)), 64, 65, 1, T(k)))
            calls.append((f"cart {fam} N=64 n_ext=65 m=1 vorticity_amplitudes NaN node part {h}", nan_node))
    return calls


KINDS = ("eval_points", "eval_grid", "find_roots", "eigenfunction", "root_slopes", "newton", "polarisation", "fields")


def run(calls, seconds=None):
    """{label: {array: numpy}}; a refused call is recorded by its message.  seconds: {kind: [s per call]} to add to."""
    from eigensolver_amd import _lib
    out = {}
    for label, f in calls:
        t0 = time.perf_counter()
        try:
            out[label] = f()
        except (_lib.EsError, ValueError) as e:
            out[label] = {"error": np.array([str(e)])}
        if seconds is not None:
            kind = next(name for name in KINDS if f" {name}" in label)
            seconds.setdefault(kind, []).append(time.perf_counter() - t0)
    return out


def differing(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return max(a.size, b.size, 1)
    if a.dtype.kind in "fc":
        return int(np.count_nonzero(~((a == b) | (np.isnan(a) & np.isnan(b)))))
    return int(np.count_nonzero(a != b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a", required=True, help="the reference build")
    ap.add_argument("--lib-b", required=True, help="the build under test")
    ap.add_argument("--time", type=int, default=0, help="timed passes per build over the flow-slab calls")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quiet", action="store_true", help="print only the calls with a difference, and the totals")
    a = ap.parse_args()
    import torch
    from eigensolver_amd import _lib
    assert torch.cuda.is_available(), "this tool compares on the GPU; there is nothing to fall back to"
    results, slab, keep_open, contexts = {}, {}, [], []
    for tag, path in (("a", a.lib_a), ("b", a.lib_b)):
        ctx = _lib.Context(0, lib=_lib.load_variant(path))
        contexts.append(ctx)
        slab[tag] = slab_calls(ctx, keep_open)
        results[tag] = run(slab[tag] + real_slab_calls(ctx, keep_open) + cylinder_calls(ctx, keep_open) + cartesian_calls(ctx))
    assert list(results["a"]) == list(results["b"])
    bad = elements = statuses = 0
    seen = set()
    for label, ra in results["a"].items():
        rb = results["b"][label]
        assert list(ra) == list(rb), label
        parts = []
        for name, x in ra.items():
            d = differing(x, rb[name])
            bad += d
            elements += x.size
            parts.append(f"{name} {d}/{x.size}")
            if x.dtype == np.uint8:                                    # the status arrays
                seen.update(np.unique(x).tolist())
        accepted = f"  [accepted roots {int(ra['flag'].sum())} of {int(ra['total'][0])} cells]" if "total" in ra else ""
        if not a.quiet or any(not p.split()[-1].startswith("0/") for p in parts):
            print(f"{label}: differing " + ", ".join(parts) + accepted)
    print(f"calls {len(results['a'])}  arrays {sum(len(r) for r in results['a'].values())}  elements {elements}  "
          f"statuses seen {sorted(seen)}  DIFFERING ELEMENTS {bad}", flush=True)

    if a.time > 0:
        secs, kinds = {"a": [], "b": []}, {"a": {}, "b": {}}
        for it in range(a.time + 1):                                   # the first pass of each build warms up
            for tag in ("a", "b"):
                t0 = time.perf_counter()
                run(slab[tag], kinds[tag] if it > 0 else None)
                if it > 0:
                    secs[tag].append(time.perf_counter() - t0)
        n_calls = len(slab["a"])
        line = {"device": torch.cuda.get_device_name(0), "tool": "compare_complex_builds", "slab_calls_per_pass": n_calls,
                "passes": a.time, "differing_elements": bad}
        for tag, path in (("a", a.lib_a), ("b", a.lib_b)):
            line[tag] = {"lib": path, "pass_s": [round(s, 4) for s in secs[tag]],
                         "median_ms_per_call": round(1e3 * statistics.median(secs[tag]) / n_calls, 4),
                         "slowest_ms_per_call": round(1e3 * max(secs[tag]) / n_calls, 4),
                         "median_ms_by_kind": {k: round(1e3 * statistics.median(v), 4) for k, v in kinds[tag].items()}}
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
    for x in keep_open:
        x.close()
    for ctx in contexts:
        ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""GPU timing aid: the branch labels of a root table (es_shoot_mode_signature) against what a user would write without the
call and against one determinant evaluation of the same pairs, on one device.

Pairs: the accepted roots of ONE pass of the headline grid (bench.py: Gaussian flow cylinder, N = 1000 nodes, 4096 x 4096
points, the mixed-precision search), tiled up to n = 2^17.  Legs, each between two device events on the context's stream,
alternating repeat by repeat in one process so that drift hits all alike, every output buffer allocated before anything is
timed:

    signature           es_shoot_mode_signature: seven outputs, 33 bytes per pair
    eigenfunction       es_shoot_eigenfunction with n_ext = 0: the same marches, 2 N doubles per pair (2.1 GB at the default
                        sizes, lane i at stride N)
    eigenfunction+torch the same call followed by the count rule and the peaks as torch expressions on the two arrays
    eval_points         es_shoot_eval_points: ONE march per pair where the signature takes three (cylinder) -- the scale of
                        the call, not a target

Before timing, the labels of the signature leg are compared with those of the torch leg on all n pairs.  One JSON line with
median / min / max ms per leg over the repeats and the ratios is printed and appended to --out.

    python tools/time_mode_signature.py [--repeats 20] [--warmup 3] [--log2n 17] [--out profiles/mode_signature_timing.jsonl]
                                        [--lib another/libeigensolver_amd.so]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_signature(torch, value, flux):
    """The count rule and the peaks of include/eigensolver_amd.h section 10 on [n, N] arrays."""
    out = []
    idx = torch.arange(value.shape[1], device=value.device)[None, :]
    for x in (value, flux):
        s = torch.sign(x)
        keep = (s != 0) & ~torch.isnan(x)
        last = torch.cummax(torch.where(keep, idx, -1), dim=1).values           # node of the last entry kept up to here
        prev = torch.gather(s, 1, last[:, :-1].clamp(min=0))                     # its sign (no entry kept yet: unused)
        change = keep[:, 1:] & (last[:, :-1] >= 0) & (s[:, 1:] != prev)
        peak, node = torch.abs(x).max(dim=1)
        out += [change.sum(dim=1).to(torch.int32), peak, node.to(torch.int32)]
    return out                                                                   # nodes, peak, peak node of value, then of flux


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=17)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mode_signature_timing.jsonl"))
    ap.add_argument("--lib", default=None, help="another build of the library to time (e.g. the parent commit's) instead "
                                                "of eigensolver_amd/lib/libeigensolver_amd.so")
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import numpy as np
    import torch
    import bench
    from eigensolver_amd import ShootProblem, _lib
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream, lib=_lib.load_variant(a.lib) if a.lib else None)
    n = 1 << a.log2n
    with torch.cuda.stream(stream):
        gp = ShootProblem(bench.workload_equilibrium(), "kink", ctx=ctx)
        N = int(gp.desc.n_nodes)
        kg, Wg = bench.workload_grid()
        roots, cnt = gp.find_roots_mixed(kg, Wg, n_bisect=bench.N_BISECT)[:2]
        acc = roots["flag"] == 1
        rk, rw = roots["k"][acc], roots["w"][acc]
        n_roots = int(rk.numel())
        assert n_roots > 0
        reps = (n + n_roots - 1) // n_roots
        dk, dw = rk.repeat(reps)[:n].contiguous(), rw.repeat(reps)[:n].contiguous()
        del roots
        ints = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
        peaks = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)]
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        vi = torch.empty((n, N), dtype=torch.float64, device=dev)
        fi = torch.empty((n, N), dtype=torch.float64, device=dev)
        D = torch.empty(n, dtype=torch.float64, device=dev)
        st_pts = torch.empty(n, dtype=torch.uint8, device=dev)
    lib, P = ctx.lib, _lib.ptr

    def signature():
        _lib.check(ctx.handle, lib.es_shoot_mode_signature(ctx.handle, gp.handle, P(dk), P(dw), n, None,
                                                           *[P(t) for t in ints + peaks], P(st)))

    def eigenfunction():
        _lib.check(ctx.handle, lib.es_shoot_eigenfunction(ctx.handle, gp.handle, P(dk), P(dw), n, P(vi), P(fi), 0, None,
                                                          None, None))

    held = {}

    def eigenfunction_torch():
        eigenfunction()
        held["t"] = torch_signature(torch, vi, fi)

    def eval_points():
        _lib.check(ctx.handle, lib.es_shoot_eval_points(ctx.handle, gp.handle, P(dk), P(dw), n, P(D), None, P(st_pts)))

    legs = {"signature": signature, "eigenfunction": eigenfunction, "eigenfunction+torch": eigenfunction_torch,
            "eval_points": eval_points}
    # the two ways to the labels agree on every pair (the entries reduced in registers are the ones the arrays hold)
    with torch.cuda.stream(stream):
        signature()
        eigenfunction_torch()
        tv, _, _, tf, _, _ = held["t"]
        ok = st == 0
        differ = int(((ints[0] != tv) | (ints[1] != tf))[ok].sum().item())
        labels = sorted(set(zip(ints[0][ok].tolist(), ints[1][ok].tolist())))
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
    line = {"device": torch.cuda.get_device_name(dev), "lib": os.path.basename(a.lib) if a.lib else "default",
            "pairs": n, "nodes": N, "distinct_roots": n_roots, "brackets": int(cnt),
            "pairs_ok": int(ok.sum().item()), "labels": [list(x) for x in labels], "labels_differ_from_torch": differ,
            "repeats": a.repeats, "warmup": a.warmup, "legs": {}}
    for name, v in ms.items():
        line["legs"][name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line["signature_over_eigenfunction"] = round(med["signature"] / med["eigenfunction"], 3)
    line["eigenfunction_torch_over_signature"] = round(med["eigenfunction+torch"] / med["signature"], 2)
    line["signature_over_eval_points"] = round(med["signature"] / med["eval_points"], 2)
    line["eigenfunction_bytes"] = 2 * n * N * 8
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    gp.close()
    ctx.close()
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

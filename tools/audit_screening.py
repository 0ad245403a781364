"""GPU measuring aid: the fp32 screening of the mixed-precision root search audited against the fp64 grid
(es_shoot_audit_screening, DESIGN.md section 4a') on the problems of BASELINE.json configs[1], [2], [4] and the headline,
at the grids bench.py runs them on.

Per problem (one mode or azimuthal order of a workload) the grid is evaluated in fp64 (es_shoot_eval_grid with rel) and
screened in fp32 (es_shoot_screen_grid), the full audit is run, and one JSON line is appended to the output file: the
counts, the least sign margin and the largest fp32 error with their cells, and the device-event time of the audit.
Beside that time, on the same arrays, alternating repeat by repeat in one process so that drift hits all alike:

    audit   es_shoot_audit_screening (counts, extrema and a table of 1024 cells; nothing read back)
    torch   the missed / false bracket masks of the same definitions as torch expressions on the device, summed
    copy    Tensor.copy_ of the same 26 bytes per cell into buffers of the same size: the bandwidth yardstick (it writes
            the 26 bytes as well, the audit only reads them)

With --rows S the line also holds the audit of the sample of every S-th k-row (ShootProblem.audit_screening(rows=S), which
evaluates and screens only those rows) and the event time of that whole call.

    python tools/audit_screening.py [--workloads config1,config2,config4,headline] [--rows 16] [--repeats 20]
                                    [--out profiles/screen_audit.jsonl]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problems(workloads):
    """(workload, label, equilibrium, mode, m, k, W) of every unit bench.py runs for the named workloads."""
    import bench
    for name in workloads:
        if name == "headline":
            k, W = bench.workload_grid()
            yield name, "m=1", bench.workload_equilibrium(), "kink", 1, k, W
        else:
            for label, _, eq, mode, m, k, W in bench.workload_units(name)[1]:
                yield name, label, eq, mode, m, k, W


def torch_masks(torch, Ds, sts, D64, st64):
    """(missed, false) of include/eigensolver_amd.h as a user would write them without the kernel."""
    unsure = (sts & 0x80) != 0
    Dm, stm = torch.where(unsure, D64, Ds), torch.where(unsure, st64, sts)

    def B(D, st):
        return (st[:, :-1] == 0) & (st[:, 1:] == 0) & (D[:, :-1] * D[:, 1:] < 0)
    b64, bm = B(D64, st64), B(Dm, stm)
    return (b64 & ~bm).sum(), (bm & ~b64).sum()


def report_dict(r):
    return {"flagged": r.flagged, "missed": r.missed, "false": r.false, "status": r.status, "sign": r.sign,
            "vouched_ok": r.vouched_ok, "unsure": r.unsure, "brackets64": r.brackets64, "ok": r.ok,
            "min_margin": r.min_margin, "min_margin_at": r.min_margin_at, "max_err": r.max_err, "max_err_at": r.max_err_at}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="config1,config2,config4,headline")
    ap.add_argument("--rows", type=int, default=0, metavar="S", help="also audit the sample of every S-th k-row")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_audit.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import torch
    from eigensolver_amd import ShootProblem, _lib, shooting
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = _lib.Context(dev.index or 0)
    stream = ctx.torch_stream
    where = {"device": torch.cuda.get_device_name(dev), "date": datetime.date.today().isoformat()}
    cap = 1024
    counts = torch.empty(10, dtype=torch.int64, device=dev)
    worst = torch.empty(2, dtype=torch.float64, device=dev)
    cell = torch.empty(cap, dtype=torch.int64, device=dev)
    kind = torch.empty(cap, dtype=torch.uint8, device=dev)
    all_ok = True
    for workload, label, eq, mode, m, k, W in problems(a.workloads.split(",")):
        gp = ShootProblem(eq, mode, m=m, ctx=ctx)
        D64, st64, rel = gp.eval_grid(k, W, want_rel=True)
        Ds, sts = gp.screen_grid(k, W)
        nk, nw = D64.shape
        full = shooting.audit_arrays(ctx, Ds, sts, D64, st64, rel, capacity=cap)
        src = (Ds, D64, rel, sts, st64)
        dst = tuple(torch.empty_like(t) for t in src)
        nbytes = sum(t.numel() * t.element_size() for t in src)

        def audit():
            _lib.check(ctx.handle, ctx.lib.es_shoot_audit_screening(
                ctx.handle, nk, nw, _lib.ptr(Ds), _lib.ptr(sts), _lib.ptr(D64), _lib.ptr(st64), _lib.ptr(rel), cap,
                _lib.ptr(cell), _lib.ptr(kind), _lib.ptr(counts), _lib.ptr(worst)))

        def copy():
            for d, s in zip(dst, src):
                d.copy_(s)
        masks = []
        legs = {"audit": audit, "torch": lambda: masks.append(torch_masks(torch, Ds, sts, D64, st64)), "copy": copy}
        ms = {name: [] for name in legs}
        for it in range(a.warmup + a.repeats):
            for name, run in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                e1.synchronize()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        # the three ways of counting agree
        assert [int(x) for x in counts.tolist()[:3]] == [full.flagged, full.missed, full.false]
        assert (int(masks[-1][0]), int(masks[-1][1])) == (full.missed, full.false)
        del masks[:]
        line = dict(where, workload=workload, problem=label, nk=nk, nw=nw, rows="all", **report_dict(full))
        line["bytes_read"] = nbytes
        for name, v in ms.items():
            med = statistics.median(v)
            line[name + "_ms"] = {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                  "repeats": len(v), "GB_per_s_read": round(nbytes / (med * 1e-3) / 1e9, 1)}
        if a.rows > 0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sampled = gp.audit_screening(k, W, rows=a.rows, capacity=cap)
            e1.record(stream)
            e1.synchronize()
            line["sampled"] = dict(report_dict(sampled), rows=f"0::{a.rows}", rows_audited=len(range(0, nk, a.rows)),
                                   whole_call_ms=round(e0.elapsed_time(e1), 3))
            all_ok = all_ok and sampled.ok
        all_ok = all_ok and full.ok
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)
        del D64, st64, rel, Ds, sts, src, dst
        gp.close()
    ctx.close()
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())

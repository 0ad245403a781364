"""What tools/time_field_synthesis.py, tools/time_cartesian_synthesis.py and tools/time_slab_synthesis.py share: their
common arguments, the context on a stream of its own, the measuring loop and the JSON summary.

The legs of a tool ("kernel", "torch", "fill" and one auxiliary leg) write into one buffer, each between two device events
on the context's stream, alternating repeat by repeat in one process so that drift hits all alike.  Per leg one JSON
line: median / min / max ms over the repeats and GB/s of the median; then the ratios kernel / fill, torch / kernel and
auxiliary / kernel.
"""
import json
import os
import statistics


def add_common_arguments(ap):
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=1, help="calls per timed window (times are per call); above 1 the host's "
                    "launch latency hides behind the previous call")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--lib", default=None, help="another build of the library to time, e.g. one made with "
                    "ES_BUILD_EXTRA_FLAGS=-DES_SLAB_SYNTH_WAVES=1024 (its file name goes into the JSON lines)")


def open_context(a):
    """(torch, device, stream, context) for the parsed arguments `a`: a stream of its own, the library of --lib."""
    assert a.repeats >= 10, "at least 10 timed repeats per leg"
    import torch
    from eigensolver_amd import _lib
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(dev.index or 0, stream=stream, lib=_lib.load_variant(a.lib) if a.lib else None)
    return torch, dev, stream, ctx


def measure(torch, stream, a, legs, sample):
    """Times of every leg in ms per call, {leg: [a.repeats values]}, and sample() cloned after the first run of the
    "kernel" and of the "torch" leg, {leg: tensor}."""
    ms = {name: [] for name in legs}
    check = {}
    for it in range(a.warmup + a.repeats):
        for name, run in legs.items():
            with torch.cuda.stream(stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    run()
                e1.record(stream)
                if it == 0 and name in ("kernel", "torch"):
                    check[name] = sample().clone()
            e1.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1) / a.calls)
    return ms, check


def assert_same_fields(check, top):
    """The kernel and the torch leg compute the same fields (one fp32 rounding each); top: the largest magnitude."""
    dk, dt = check["kernel"].double(), check["torch"].double()
    assert bool(((dk - dt).abs() <= 2.0 ** -22 * dt.abs() + 1e-12 * top).all())


def report(a, device_name, ms, nbytes, frame_entries, aux, aux_entries):
    """Print (and append to --out) one line per leg and the ratio line.  frame_entries: what describes the mesh of the
    three frame legs; aux, aux_entries: the name of the auxiliary leg and what describes its input."""
    res, lines = {}, []
    for name, v in ms.items():
        med = res[name] = statistics.median(v)
        line = {"leg": name, "repeats": len(v), "calls_per_window": a.calls, "median_ms": round(med, 4),
                "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if name == aux:
            line.update(aux_entries)
        else:
            line.update(frame_entries, frames=a.frames, bytes=nbytes, GB_per_s=round(nbytes / (med * 1e-3) / 1e9, 1))
        lines.append(line)
    lines.append({"device": device_name, "lib": os.path.basename(a.lib) if a.lib else "default",
                  "kernel_over_fill": round(res["kernel"] / res["fill"], 3),
                  "torch_over_kernel": round(res["torch"] / res["kernel"], 2),
                  aux + "_over_kernel": round(res[aux] / res["kernel"], 4)})
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

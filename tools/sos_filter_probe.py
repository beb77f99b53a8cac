"""The recursive-filter kernel (sos_filter.hip) against a copy of the same tensor, in one process, the legs of a comparison
alternated per round (device-synchronised, warmed up, K calls per timed region; median, min and max over the rounds), with
the helpers of tools/resample_probe.py:

  kernel    ops.sos_filter forward and reverse at 1, 2, 4, 8 and 16 sections against x.clone() -- the same 8 bytes per
            sample with no arithmetic -- with the bytes/s achieved, and the section count from which the time grows with
            the sections: where the kernel leaves the memory bound
  train     forward + backward through SOSFilter
  stream    one RealtimeSOSFilter.forward call at --streams streams x chunks of 256 / 1024 / 4096
  long      one row of --long-row samples: what a single workgroup costs (there is no dispatch that splits a row)

at --clips clips x --seconds s.  Nobody measured this kernel before: no ratio is expected, the figures are recorded.  Writes
a markdown report (--out, default profiles/sos_filter_probe.md) and prints one JSON line per stage."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_probe import alternate, fmt  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402
from acids_transforms_amd.utils import filter_design as fd  # noqa: E402

SR = 44100


def cascade(n):
    """n sections: the 20 Hz high-pass first, then peaks and dips of 3 dB between 100 Hz and 15 kHz."""
    rows = [fd.highpass(SR, 20.0)] + [fd.equalizer(SR, 100.0 * 1.4 ** i, 3.0 if i % 2 else -3.0, 2.0) for i in range(1, n)]
    return ops.sos_coefficients(np.concatenate(rows))


def outside(a, b):
    """Is the median of `a` outside the (min .. max) of `b`?"""
    return not (b["min_ms"] <= a["ms"] <= b["max_ms"])


def kernel_stage(args, dev, ev):
    B, L = args.clips, int(SR * args.seconds)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    out = {"stage": "kernel", "clips": B, "L": L, "bytes": B * L * 8, "plan": ops.sos_filter_plan(B, L, 1), "rows": []}
    for n in args.sections:
        co = cascade(n)
        legs = {"forward": lambda: ops.sos_filter(x, co), "clone": lambda: x.clone(),
                "reverse": lambda: ops.sos_filter(x, co, reverse=True)}
        ms = alternate(legs, args.calls, args.rounds, args.warmup, ev)
        out["rows"].append({"sections": n, "ms": ms,
                            "TBps": {k: out["bytes"] / (v["ms"] * 1e-3) / 1e12 for k, v in ms.items()}})
    base = out["rows"][0]["ms"]["forward"]
    out["leaves_memory_bound_at"] = next((r["sections"] for r in out["rows"][1:]
                                          if r["ms"]["forward"]["min_ms"] > base["max_ms"] * 1.05), None)
    print(json.dumps(out), flush=True)
    return out


def train_stage(args, dev, ev):
    B, L = args.clips, int(SR * args.seconds)
    gen = torch.Generator(device=dev).manual_seed(1)
    xr = (torch.randn(B, L, device=dev, generator=gen) * 0.1).requires_grad_()
    g = torch.randn(B, L, device=dev, generator=gen)
    out = {"stage": "train", "clips": B, "L": L, "rows": []}

    def fb(m):
        xr.grad = None
        m(xr).backward(g)

    for n in args.sections:
        m, zp = A.SOSFilter(cascade(n)).to(dev), A.SOSFilter(cascade(n), zero_phase=True).to(dev)
        legs = {"forward+backward": lambda: fb(m), "zero-phase forward+backward": lambda: fb(zp)}
        out["rows"].append({"sections": n, "ms": alternate(legs, args.train_calls, args.rounds, args.warmup, ev)})
    print(json.dumps(out), flush=True)
    return out


def stream_stage(args, dev, ev):
    out = {"stage": "stream", "streams": args.streams, "rows": []}
    gen = torch.Generator(device=dev).manual_seed(2)
    for n in (1, 4):
        legs = {}
        for C in (256, 1024, 4096):
            rt = A.RealtimeSOSFilter(cascade(n)).to(dev)
            chunk = torch.randn(args.streams, C, device=dev, generator=gen) * 0.1
            legs["%d" % C] = (lambda rt=rt, chunk=chunk: rt(chunk))
        out["rows"].append({"sections": n, "ms": alternate(legs, args.stream_calls, args.rounds, args.warmup, ev)})
    print(json.dumps(out), flush=True)
    return out


def long_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(1, args.long_row, device=dev, generator=gen) * 0.1
    legs = {"%d" % n: (lambda co=cascade(n): ops.sos_filter(x, co)) for n in (1, 4, 16)}
    out = {"stage": "long", "L": args.long_row, "ms": alternate(legs, 1, args.rounds, args.warmup, ev)}
    print(json.dumps(out), flush=True)
    return out


def report(args, kernel, train, stream, long_row):
    lines = ["# Recursive-filter probe (tools/sos_filter_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one"
             % args.rounds, "process.  %d clips x %.1f s at %d Hz.  No ratio was expected: recorded only." %
             (args.clips, args.seconds, SR), ""]
    if kernel:
        tile, per_lane, dispatch = kernel["plan"]
        lines += ["## ops.sos_filter against x.clone() (%d x %d samples, %.2f GB moved; tile %d = 256 x %d, dispatch %d)"
                  % (kernel["clips"], kernel["L"], kernel["bytes"] / 1e9, tile, per_lane, dispatch), "",
                  "| sections | forward ms | reverse ms | clone ms | forward TB/s | reverse TB/s | clone TB/s | forward / clone | reverse outside the forward's spread |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in kernel["rows"]:
            f, v, c = r["ms"]["forward"], r["ms"]["reverse"], r["ms"]["clone"]
            lines.append("| %d | %s | %s | %s | %.2f | %.2f | %.2f | %.2f | %s |" % (
                r["sections"], fmt(f), fmt(v), fmt(c), r["TBps"]["forward"], r["TBps"]["reverse"], r["TBps"]["clone"],
                f["ms"] / c["ms"], "yes" if outside(v, f) else "no"))
        at = kernel["leaves_memory_bound_at"]
        lines += ["", "The forward time first exceeds the one-section time by more than its spread and 5 %% at %s."
                  % ("%d sections: from there the kernel is bound by its fp64 arithmetic, not by memory" % at if at else
                     "no measured section count: memory-bound throughout"), ""]
    if train:
        lines += ["## forward + backward through SOSFilter (the backward is the same kernel, reversed)", "",
                  "| sections | forward + backward ms | zero-phase forward + backward ms |", "|---|---|---|"]
        for r in train["rows"]:
            lines.append("| %d | %s | %s |" % (r["sections"], fmt(r["ms"]["forward+backward"]),
                                               fmt(r["ms"]["zero-phase forward+backward"])))
        lines.append("")
    if stream:
        lines += ["## one RealtimeSOSFilter.forward call, %d streams" % stream["streams"], "",
                  "| sections | chunk 256 ms | chunk 1024 ms | chunk 4096 ms |", "|---|---|---|---|"]
        for r in stream["rows"]:
            lines.append("| %d | %s | %s | %s |" % (r["sections"], fmt(r["ms"]["256"]), fmt(r["ms"]["1024"]), fmt(r["ms"]["4096"])))
        lines.append("")
    if long_row:
        lines += ["## one row of %d samples: one workgroup walks it (no dispatch splits a row)" % long_row["L"], "",
                  "| sections | ms |", "|---|---|"]
        lines += ["| %s | %s |" % (k, fmt(v)) for k, v in long_row["ms"].items()]
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--sections", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--legs", nargs="+", default=["kernel", "train", "stream", "long"],
                    choices=["kernel", "train", "stream", "long"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--train-calls", type=int, default=2)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-calls", type=int, default=20)
    ap.add_argument("--long-row", type=int, default=2 ** 24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "sos_filter_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel = kernel_stage(args, dev, ev) if "kernel" in args.legs else None
    train = train_stage(args, dev, ev) if "train" in args.legs else None
    stream = stream_stage(args, dev, ev) if "stream" in args.legs else None
    long_row = long_stage(args, dev, ev) if "long" in args.legs else None
    report(args, kernel, train, stream, long_row)


if __name__ == "__main__":
    main()

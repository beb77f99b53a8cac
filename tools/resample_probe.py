"""The differentiable and the streaming Resample against their yardsticks, in one process, the legs of a comparison
alternated per round (device-synchronised, warmed up, K calls per timed region; median, min and max over the rounds):

  kernel    at_resample_sinc_backward against at_resample_sinc on the same shape (the same multiply-adds), through ops,
            with the bytes/s achieved against out_len * 4 + L * 4 per row
  train     forward + backward through utils.Resample against the same bank as torch conv1d (pad, stride orig,
            transpose, reshape, crop) with torch's own backward, on the device; and the peak memory above the inputs
  stream    utils.RealtimeResample.forward against the route available without it: torch.cat([state, chunk]) ->
            Resample -> the slice of the chunk's blocks -> the copy of the new state; compared to the bit

at --clips clips x --seconds s for the offline ratios, --streams streams x chunks of orig, 8 orig and 32 orig samples for
the stream.  Writes a markdown report (--out, default profiles/resample_probe.md) and prints one JSON line per stage."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402

RATES = {(147, 160): 44100, (160, 147): 48000, (1, 2): 22050, (2, 1): 44100, (441, 160): 44100}


def timed(fn, K, ev):
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(K):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / K


def spread(v):
    return {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def alternate(legs, K, rounds, warmup, ev):
    times = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for name, fn in legs.items():
            ms = timed(fn, K, ev)
            if r >= warmup:
                times[name].append(ms)
    return {k: spread(v) for k, v in times.items()}


def conv_route(x, bank, orig, new, width):
    """The converter as torch ops: what a user writes without the kernel, differentiable by torch."""
    rows, L = x.shape
    xp = torch.nn.functional.pad(x[:, None], (width, width + orig))
    y = torch.nn.functional.conv1d(xp, bank[:, None], stride=orig)
    return y.transpose(1, 2).reshape(rows, -1)[:, :-(-new * L // orig)]


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def offline_stage(args, dev, ev, ratio):
    orig, new = ratio
    rs = A.Resample(orig, new).to(dev)
    width, taps = rs.width, 2 * rs.width + orig
    L = int(RATES[ratio] * args.seconds) // orig * orig
    B, olen = args.clips, -(-new * L // orig)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    g = torch.randn(B, olen, device=dev, generator=gen)
    tile, in_lds = ops.resample_backward_plan(orig, new, taps, width)
    out = {"stage": "offline", "orig": orig, "new": new, "clips": B, "L": L, "out_len": olen, "taps": taps,
           "tile_blocks": tile, "bank_in_lds": in_lds}
    if "kernel" in args.legs:
        legs = {"backward": lambda: ops.resample_sinc_backward(g, L, orig, new, taps, width, rs.kernel),
                "forward": lambda: ops.resample_sinc(x, orig, new, width, rs.kernel)}
        out["kernel_ms"] = alternate(legs, args.calls, args.rounds, args.warmup, ev)
        out["kernel_GBps"] = {k: B * 4 * (olen + L) / (v["ms"] * 1e-3) / 1e9 for k, v in out["kernel_ms"].items()}
    if "train" in args.legs:
        Bt = min(B, args.train_clips)
        xr = x[:Bt].clone().requires_grad_()
        gt = g[:Bt]

        def fb(fn):
            xr.grad = None
            fn(xr).backward(gt)

        hip, conv = (lambda: fb(rs)), (lambda: fb(lambda v: conv_route(v, rs.kernel, orig, new, width)))
        hip()
        g_hip = xr.grad.clone()
        conv()
        out["train_clips"] = Bt
        out["train_grad_rel_max"] = float((g_hip - xr.grad).abs().max() / xr.grad.abs().max())
        out["train_ms"] = alternate({"hip": hip, "conv1d": conv}, args.train_calls, args.rounds, args.warmup, ev)
        out["train_peak_bytes"] = {"hip": peak_above(hip), "conv1d": peak_above(conv)}
    print(json.dumps(out), flush=True)
    return out


def stream_stage(args, dev, ev, ratio):
    orig, new = ratio
    rs = A.Resample(orig, new).to(dev)
    D, Ha = ops.resample_stream_sizes(orig, rs.width)
    B = args.streams
    gen = torch.Generator(device=dev).manual_seed(2)
    results = []
    for mult in args.chunk_blocks:
        C = mult * orig
        rt = rs.streaming()
        state = {"s": torch.zeros(B, Ha, device=dev)}
        x = [torch.randn(B, C, device=dev, generator=gen) * 0.1 for _ in range(3)]

        def composed_call(v):
            buf = torch.cat([state["s"], v], -1)                   # (B, Ha + C), Ha = D orig + width
            # offline block i of buf reads buf[i orig - width + k]; the chunk's block t reads buf[t orig + k]: pad
            # D orig - width >= 0 zeros in front, then block t of the chunk is offline block t + D of the padded buffer
            padded = torch.nn.functional.pad(buf, (D * orig - rs.width, 0)) if D * orig > rs.width else buf
            y = rs(padded)[..., D * new:D * new + C // orig * new]
            state["s"] = buf[..., -Ha:].clone()
            return y

        same = all(torch.equal(rt(v), composed_call(v)) for v in x)
        legs = {"stream": lambda: rt(x[0]), "composed": lambda: composed_call(x[0])}
        ms = alternate(legs, args.stream_calls, args.rounds, args.warmup, ev)
        bytes_call = 4 * B * (C + C // orig * new + 2 * Ha)
        out = {"stage": "stream", "orig": orig, "new": new, "streams": B, "chunk": C, "bit_identical_to_composed": same,
               "ms": ms, "bytes_per_call": bytes_call, "GBps": bytes_call / (ms["stream"]["ms"] * 1e-3) / 1e9}
        print(json.dumps(out), flush=True)
        results.append(out)
    return results


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["ms"], s["min_ms"], s["max_ms"])


def verdict(a, b):
    """`a` is expected not to be slower than `b` beyond the larger of the two spreads."""
    return "met" if a["ms"] <= b["ms"] + max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"]) else "MISSED"


def report(args, offline, stream):
    lines = ["# Resample probe (tools/resample_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one"
             % args.rounds, "process.  %d clips x %.1f s offline; %d streams." % (args.clips, args.seconds, args.streams), ""]
    if any("kernel_ms" in r for r in offline):
        lines += ["## at_resample_sinc_backward against at_resample_sinc (same shape, same multiply-adds)", "",
                  "| (orig, new) | L | tile blocks | bank in LDS | backward ms | forward ms | backward / forward | backward GB/s | expectation (same time or better) |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in offline:
            if "kernel_ms" in r:
                b, f = r["kernel_ms"]["backward"], r["kernel_ms"]["forward"]
                lines.append("| (%d, %d) | %d | %d | %s | %s | %s | %.2f | %.0f | %s |" % (
                    r["orig"], r["new"], r["L"], r["tile_blocks"], r["bank_in_lds"], fmt(b), fmt(f), b["ms"] / f["ms"],
                    r["kernel_GBps"]["backward"], verdict(b, f)))
        lines.append("")
    if any("train_ms" in r for r in offline):
        lines += ["## forward + backward through Resample against conv1d with torch's backward", "",
                  "| (orig, new) | clips | HIP ms | conv1d ms | HIP / conv1d | HIP peak MiB above inputs | conv1d peak MiB | gradients differ by (normwise) |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in offline:
            if "train_ms" in r:
                h, c = r["train_ms"]["hip"], r["train_ms"]["conv1d"]
                lines.append("| (%d, %d) | %d | %s | %s | %.2f | %.1f | %.1f | %.1e |" % (
                    r["orig"], r["new"], r["train_clips"], fmt(h), fmt(c), h["ms"] / c["ms"],
                    r["train_peak_bytes"]["hip"] / 2 ** 20, r["train_peak_bytes"]["conv1d"] / 2 ** 20, r["train_grad_rel_max"]))
        lines.append("")
    if stream:
        lines += ["## RealtimeResample.forward against cat + Resample + slice + state copy", "",
                  "| (orig, new) | chunk | stream ms | composed ms | stream / composed | bit-identical | stream GB/s | expectation (not slower) |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in stream:
            s, c = r["ms"]["stream"], r["ms"]["composed"]
            lines.append("| (%d, %d) | %d | %s | %s | %.2f | %s | %.2f | %s |" % (
                r["orig"], r["new"], r["chunk"], fmt(s), fmt(c), s["ms"] / c["ms"], r["bit_identical_to_composed"], r["GBps"],
                verdict(s, c)))
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--ratios", type=int, nargs="+", default=[147, 160, 160, 147, 1, 2, 2, 1, 441, 160])
    ap.add_argument("--stream-ratios", type=int, nargs="+", default=[147, 160])
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--chunk-blocks", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--legs", nargs="+", default=["kernel", "train", "stream"], choices=["kernel", "train", "stream"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--train-clips", type=int, default=1024)
    ap.add_argument("--train-calls", type=int, default=2)
    ap.add_argument("--stream-calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "resample_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    pairs = lambda v: list(zip(v[::2], v[1::2]))  # noqa: E731
    offline = [offline_stage(args, dev, ev, r) for r in pairs(args.ratios)] if {"kernel", "train"} & set(args.legs) else []
    stream = []
    if "stream" in args.legs:
        for r in pairs(args.stream_ratios):
            stream += stream_stage(args, dev, ev, r)
    report(args, offline, stream)


if __name__ == "__main__":
    main()

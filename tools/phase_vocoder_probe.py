"""The phase vocoder kernels against their yardsticks, in one process, the legs of a comparison alternated per round
(device-synchronised, warmed up, K calls per timed region; median, min and max over the rounds), at --clips x --frames x
--bins and each of --rates:

  forward   at_phase_vocoder in its default layout (one block per clip where rows are no whole 64-byte segments) and on
            flat columns (AT_VARIANT_SCAN_LAYOUT = 1), against
              the byte floor  (T + N) F 8 bytes per clip, as bytes/s achieved and as a share of the 8 TB/s HBM peak,
              the IF scan     ops.phase_scan(X, "forward") of the same tree at the same shape (T F (8 + 4) bytes per clip):
                              the expectation is that the vocoder reaches at least the scan's share of HBM,
              torch ops       the textbook algorithm (angle, wrap, advance, cumsum, polar) composed on the same device
  backward  at_phase_vocoder_backward (flat columns) against its byte floor (2 T + N) F 8 + F 8 bytes per clip, and forward + backward
            through TimeStretch against torch's autograd of the composed textbook (--train-clips clips: the composition
            keeps about twenty (B, N, F) tensors alive)

The composed textbook runs in fp32 on the device, so its distance from the kernel is printed too: that is the angle
route's error, not the kernel's (tests/test_phase_vocoder_gpu.py holds the kernel to 1e-5 of float64).  Writes a markdown
report (--out, default profiles/phase_vocoder_probe.md) and prints one JSON line per rate."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12


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


def textbook(X, idx, alpha, hop):
    """torchaudio.functional.phase_vocoder in the time-major layout, from torch ops on X's device and in its precision"""
    F = X.shape[-1]
    advance = torch.linspace(0, math.pi * hop, F, device=X.device)
    phase_0 = X[..., :1, :].angle()
    Xp = torch.nn.functional.pad(torch.view_as_real(X), (0, 0, 0, 0, 0, 2))
    Xp = torch.view_as_complex(Xp)
    X0, X1 = Xp.index_select(-2, idx), Xp.index_select(-2, idx + 1)
    a0, a1, n0, n1 = X0.angle(), X1.angle(), X0.abs(), X1.abs()
    ph = a1 - a0 - advance
    ph = ph - 2 * math.pi * torch.round(ph / (2 * math.pi))
    ph = ph + advance
    acc = torch.cumsum(torch.cat([phase_0, ph[..., :-1, :]], -2), -2)
    al = alpha.unsqueeze(-1)
    return torch.polar(al * n1 + (1 - al) * n0, acc)


def normwise(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


def stage(args, dev, ev, rate):
    B, T, F = args.clips, args.frames, args.bins
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.complex(torch.randn(B, T, F, device=dev, generator=gen), torch.randn(B, T, F, device=dev, generator=gen))
    idx_h, alpha_h = ops.phase_vocoder_steps(T, rate)
    idx, alpha, N = idx_h.to(dev).long(), alpha_h.to(dev), idx_h.numel()
    g = torch.complex(torch.randn(B, N, F, device=dev, generator=gen), torch.randn(B, N, F, device=dev, generator=gen))
    out, fin = ops.phase_vocoder(X, rate, want_phasor=True)

    def flat():
        with _lib.variant("scan_layout", 1):
            return ops.phase_vocoder(X, rate)

    res = {"rate": rate, "clips": B, "T": T, "F": F, "N": N,
           "flat_bits_equal": bool(torch.equal(torch.view_as_real(flat()), torch.view_as_real(out))),
           "torch_fp32_vs_kernel": normwise(textbook(X[:8], idx, alpha, args.hop), out[:8])}
    legs = {"vocoder": lambda: ops.phase_vocoder(X, rate), "vocoder_flat": flat,
            "if_scan": lambda: ops.phase_scan(X, "forward"), "torch_ops": lambda: textbook(X, idx, alpha, args.hop),
            "backward": lambda: ops.phase_vocoder_backward(X, g, rate, fin)}
    res["ms"] = alternate(legs, args.calls, args.rounds, args.warmup, ev)
    floor = {"vocoder": B * (T + N) * F * 8, "vocoder_flat": B * (T + N) * F * 8, "if_scan": B * T * F * 12,
             "backward": B * ((2 * T + N) * F * 8 + F * 8)}
    res["bytes"] = floor
    res["TBps"] = {k: floor[k] / (res["ms"][k]["ms"] * 1e-3) / 1e12 for k in floor}
    del out, g
    # training step: forward + backward, the module against torch's autograd of the composition
    Bt = min(B, args.train_clips)
    Xr = X[:Bt].clone().requires_grad_()
    ts = A.TimeStretch(rate)
    gt = torch.complex(torch.randn(Bt, N, F, device=dev, generator=gen), torch.randn(Bt, N, F, device=dev, generator=gen))

    def fb(fn):
        Xr.grad = None
        fn(Xr).backward(gt)

    hip, composed = (lambda: fb(ts)), (lambda: fb(lambda v: textbook(v, idx, alpha, args.hop)))
    hip()
    g_hip = Xr.grad.clone()
    composed()
    res["train_clips"] = Bt
    res["train_grad_torch_fp32_vs_kernel"] = normwise(Xr.grad, g_hip)
    res["train_ms"] = alternate({"hip": hip, "torch_ops": composed}, args.train_calls, args.rounds, args.warmup, ev)
    print(json.dumps(res), flush=True)
    return res


def fmt(s):
    return "%.3f (%.3f .. %.3f)" % (s["ms"], s["min_ms"], s["max_ms"])


def report(args, results):
    lines = ["# Phase vocoder probe (tools/phase_vocoder_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds of %d calls, device-synchronised, the legs of a row alternated"
             % (args.rounds, args.calls),
             "in one process.  %d clips x %d frames x %d bins, complex64.  Shares are of the %.0f TB/s HBM peak, over the bytes"
             % (args.clips, args.frames, args.bins, HBM_PEAK / 1e12),
             "each kernel has to move: (T + N) F 8 per clip for the vocoder, T F 12 for the IF scan, (2 T + N) F 8 + F 8 for the",
             "backward.", "",
             "## forward", "",
             "| rate | N | vocoder ms | TB/s | share | flat columns ms | TB/s | IF scan ms | TB/s | share | torch ops ms | torch / vocoder | "
             "expectation (the scan's share or better) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        m, t = r["ms"], r["TBps"]
        best = max(t["vocoder"], t["vocoder_flat"])
        lines.append("| %g | %d | %s | %.2f | %.0f %% | %s | %.2f | %s | %.2f | %.0f %% | %s | %.1f | %s |" % (
            r["rate"], r["N"], fmt(m["vocoder"]), t["vocoder"], 100 * t["vocoder"] * 1e12 / HBM_PEAK, fmt(m["vocoder_flat"]),
            t["vocoder_flat"], fmt(m["if_scan"]), t["if_scan"], 100 * t["if_scan"] * 1e12 / HBM_PEAK, fmt(m["torch_ops"]),
            m["torch_ops"]["ms"] / m["vocoder"]["ms"], "met" if t["vocoder"] >= t["if_scan"] else
            ("MISSED (flat columns meet it)" if best >= t["if_scan"] else "MISSED")))
    lines += ["", "Flat columns and one block per clip give the same bits: %s.  The composed fp32 textbook is %s off the kernel"
              % (all(r["flat_bits_equal"] for r in results), ", ".join("%.1e" % r["torch_fp32_vs_kernel"] for r in results)),
              "(normwise, 8 clips, hop %d): the angle route's error in fp32." % args.hop, "",
              "## backward", "",
              "| rate | backward ms | TB/s | share | clips | TimeStretch fwd + bwd ms | torch ops fwd + bwd ms | torch / HIP | "
              "gradients differ by (normwise) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        m, t, tr = r["ms"], r["TBps"], r["train_ms"]
        lines.append("| %g | %s | %.2f | %.0f %% | %d | %s | %s | %.1f | %.1e |" % (
            r["rate"], fmt(m["backward"]), t["backward"], 100 * t["backward"] * 1e12 / HBM_PEAK, r["train_clips"], fmt(tr["hip"]),
            fmt(tr["torch_ops"]), tr["torch_ops"]["ms"] / tr["hip"]["ms"], r["train_grad_torch_fp32_vs_kernel"]))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=690)
    ap.add_argument("--bins", type=int, default=513)
    ap.add_argument("--rates", type=float, nargs="+", default=[0.8, 1.25, 2.0])
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--train-clips", type=int, default=256)
    ap.add_argument("--train-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "phase_vocoder_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    report(args, [stage(args, dev, ev, r) for r in args.rates])


if __name__ == "__main__":
    main()

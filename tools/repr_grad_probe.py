"""The forward backward of the phase-side representations at the bench size (1024 clips x 4 s: 690 frames x 513 bins per
clip), one process, legs alternated per round.  Each backward is timed next to the forward kernel of the same shape:

  angle_fwd / angle_bwd          Phase()           ops.phase_scan "angle" (12 B per bin) / ops.phase_scan_backward (20 B)
  unwrap_fwd / unwrap_bwd        Phase(unwrap)     the column walk forward / the same flat backward
  if_<m>_fwd / if_<m>_bwd        IF(method=m)      the column walk forward / the three-row stencil backward
  angle_bwd_accum                                  the backward adding a spectrum gradient in place (28 B)
  angle_bwd_stacked                                the backward reading the phase half of a stacked gradient (ld_g = 2 F)
  cart_fwd / cart_bwd            Cartesian()       ops.cartesian_forward / ops.cartesian_forward_backward (16 B both)
  polar_fwd / polar_bwd          Polar()           ops.polar_forward / the scan backward + the Magnitude backward
  chain_fwd / chain_fwd+bwd      STFT() + Polar()  the fused forward / the same with requires_grad, plus the chunked backward

The yardstick is the byte ratio: Phase() forward moves 12 B per bin and its backward 20 B, so the backward should cost
at most 1.67 x the flat forward angle pass.  Prints one JSON line (medians over the rounds, ms) and writes the report
(--out, default profiles/repr_grad_probe.md)."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402

BYTE_RATIO = 20.0 / 12.0


def report(out):
    ms, n = out["ms"], out["frames"] * out["bins"]
    tbs = lambda key, nbytes: n * nbytes / (ms[key] * 1e-3) / 1e12   # noqa: E731
    ratio = ms["angle_bwd"] / ms["angle_fwd"]
    lines = [
        "# Forward backward of Phase / IF / Cartesian / Polar at the bench size (`tools/repr_grad_probe.py`)",
        "",
        "Measured %s.  %d clips x %d samples, n_fft 1024 / hop 256 (%d frames of %d bins), one MI355X, one process,"
        % (out["date"], out["clips"], out["samples"], out["frames"], out["bins"]),
        "medians of %d alternated rounds (ms).  Every backward is timed next to the forward kernel of the same shape from"
        % out["rounds"],
        "the same tree.  The yardstick is the byte ratio: `Phase()` forward moves 12 B per bin, its backward 20 B, so the",
        "expectation is a backward at most %.2f x the flat forward angle pass." % BYTE_RATIO,
        "",
        "| representation | forward (ms) | backward (ms) | backward / forward | forward TB/s | backward TB/s |",
        "|---|---|---|---|---|---|",
    ]
    rows = [("`Phase()`, flat angle pass", "angle", 12, 20), ("`Phase(unwrap=True)`, column walk forward", "unwrap", 12, 20)]
    rows += [("`IF(method=\"%s\")`" % m, "if_" + m, 12, 20) for m in ("forward", "backward", "central")]
    rows += [("`Cartesian()` in one pass", "cart", 16, 16)]
    for label, key, fb, bb in rows:
        f, b = ms[key + "_fwd"], ms[key + "_bwd"]
        lines.append("| %s | %.3f | %.3f | %.2f x | %.2f | %.2f |" % (label, f, b, b / f, tbs(key + "_fwd", fb),
                                                                     tbs(key + "_bwd", bb)))
    lines += [
        "",
        "Against the flat forward angle pass (%.3f ms): `Phase()` backward %.2f x (%s the %.2f x the bytes predict);"
        % (ms["angle_fwd"], ratio, "within" if ratio <= BYTE_RATIO else "MISSES", BYTE_RATIO),
        "IF backward " + ", ".join("%s %.2f x" % (m, ms["if_%s_bwd" % m] / ms["angle_fwd"])
                                   for m in ("forward", "backward", "central")) + ".",
        "",
        "| form | ms | TB/s |",
        "|---|---|---|",
        "| `angle` backward adding a spectrum gradient in place (`accum == out`, 28 B per bin) | %.3f | %.2f |"
        % (ms["angle_bwd_accum"], tbs("angle_bwd_accum", 28)),
        "| `angle` backward reading the phase half of a stacked gradient (`ld_g = 2 F`, 20 B per bin) | %.3f | %.2f |"
        % (ms["angle_bwd_stacked"], tbs("angle_bwd_stacked", 20)),
        "",
        "`Polar()` on a spectrum: forward %.3f ms, backward (scan backward, then the Magnitude backward adding it) %.3f ms."
        % (ms["polar_fwd"], ms["polar_bwd"]),
        "`STFT() + Polar()` from audio (fused forward, audio-only graph, backward in chunks of %d clips): forward %.3f ms,"
        % (out["chunk_clips"], ms["chain_fwd"]),
        "forward + backward %.3f ms = %.2f x the forward." % (ms["chain_fwd+bwd"], ms["chain_fwd+bwd"] / ms["chain_fwd"]),
        "",
        "Raw probe line: `%s`" % json.dumps(out),
        "",
    ]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=176400)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repr_grad_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L = args.clips, args.samples
    g = torch.Generator(device=dev).manual_seed(0)
    stft = A.STFT().to(dev)
    x = torch.randn(B, L, device=dev, generator=g) * 0.1
    X = stft(x)
    T, F = X.shape[1], X.shape[2]
    gout = torch.randn(B, T, F, device=dev, generator=g)
    stacked = torch.randn(B, T, 2, F, device=dev, generator=g)
    acc = torch.randn(B, T, F, dtype=torch.complex64, device=dev, generator=g)
    window = (torch.rand(T, device=dev, generator=g) + 0.5)

    legs = {}
    legs["angle_fwd"] = lambda: ops.phase_scan(X, "angle")
    legs["angle_bwd"] = lambda: ops.phase_scan_backward(X, "angle", gout)
    legs["unwrap_fwd"] = lambda: ops.phase_scan(X, "unwrap")
    legs["unwrap_bwd"] = lambda: ops.phase_scan_backward(X, "unwrap", gout)
    for m in ("forward", "backward", "central"):
        legs["if_%s_fwd" % m] = lambda m=m: ops.phase_scan(X, m, frame_window=window)
        legs["if_%s_bwd" % m] = lambda m=m: ops.phase_scan_backward(X, m, gout, window)
    legs["angle_bwd_accum"] = lambda: ops.phase_scan_backward(X, "angle", gout, accum=acc, out=acc)
    legs["angle_bwd_stacked"] = lambda: ops.phase_scan_backward(X, "angle", stacked[..., 1, :])

    cart = A.Cartesian().to(dev)
    cart.scale_data(X)
    re_aff, im_aff = cart.magnitude._affine(X), cart.phase._affine(X)
    legs["cart_fwd"] = lambda: ops.cartesian_forward(X, *re_aff, *im_aff)
    legs["cart_bwd"] = lambda: ops.cartesian_forward_backward(stacked, re_aff[1], im_aff[1])

    polar = A.Polar().to(dev)
    polar.scale_data(X)
    Xr = X.detach().requires_grad_()
    with torch.enable_grad():
        yp = polar(Xr)
    legs["polar_fwd"] = lambda: polar(X)
    legs["polar_bwd"] = lambda: torch.autograd.grad(yp, Xr, stacked, retain_graph=True)

    chain = stft + polar
    xr = x.detach().requires_grad_()

    def chain_fwd_bwd():
        chain(xr).backward(stacked)
        xr.grad = None

    legs["chain_fwd"] = lambda: chain(x)
    legs["chain_fwd+bwd"] = chain_fwd_bwd

    times = {k: [] for k in legs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(ev[0].elapsed_time(ev[1]))
    from acids_transforms_amd.autograd import mfcc_chunk_clips
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"date": datetime.date.today().isoformat(), "clips": B, "samples": L, "frames": B * T, "bins": F,
           "rounds": args.rounds, "chunk_clips": mfcc_chunk_clips(B, T, 1024), "ms": med,
           "min_ms": {k: min(v) for k, v in times.items()}}
    print(json.dumps(out))
    with open(args.out, "w") as fh:
        fh.write(report(out))


if __name__ == "__main__":
    main()

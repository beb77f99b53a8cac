"""The bankless sample-rate converter (sinc_interp.hip) and PitchShift against their yardsticks, in one process, the legs
of a comparison alternated per round (device-synchronised, warmed up, K calls per timed region; median, min and max over
the rounds), with the helpers of tools/resample_probe.py:

  forward   ops.resample_direct against at_resample_sinc (the bank route) on the same shape, compared to the bit, with the
            bytes/s achieved against the floor (L + out_len) * 4 per row
  train     forward + backward through Resample(direct=True) against the same converter as torch conv1d with torch's own
            backward (resample_probe.conv_route), and against Resample() with the bank
  pitch     PitchShift(n_steps) forward and forward + backward, and each stage of the chain alone on the tensors the chain
            hands it (no comparator exists: recorded only)

at --clips clips x --seconds s.  Writes a markdown report (--out, default profiles/sinc_interp_probe.md) and prints one JSON
line per stage."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_probe import RATES, alternate, conv_route, fmt, peak_above, verdict  # noqa: E402
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402


def converter_stage(args, dev, ev, ratio):
    orig, new = ratio
    bank, direct = A.Resample(orig, new).to(dev), A.Resample(orig, new, direct=True).to(dev)
    taps = 2 * bank.width + orig
    L = int(RATES[ratio] * args.seconds) // orig * orig
    B, olen = args.clips, -(-new * L // orig)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    g = torch.randn(B, olen, device=dev, generator=gen)
    tile, in_lds = ops.sinc_interp_plan(orig, new, direct.Qi)
    live = int((bank.kernel != 0).sum(1).max())
    out = {"stage": "converter", "orig": orig, "new": new, "clips": B, "L": L, "out_len": olen, "taps": taps,
           "live_taps": live, "Qi": direct.Qi, "tile_outputs": tile, "table_in_lds": in_lds,
           "floor_bytes": B * 4 * (L + olen)}
    if "forward" in args.legs:
        out["forward_bit_identical"] = torch.equal(direct(x), bank(x))
        legs = {"direct": lambda: ops.sinc_interp(x, orig, new, direct.table, direct.Qi, olen),
                "bank": lambda: ops.resample_sinc(x, orig, new, bank.width, bank.kernel)}
        out["forward_ms"] = alternate(legs, args.calls, args.rounds, args.warmup, ev)
        out["forward_GBps"] = {k: out["floor_bytes"] / (v["ms"] * 1e-3) / 1e9 for k, v in out["forward_ms"].items()}
        back = {"direct": lambda: ops.sinc_interp(g, new, orig, direct.table, direct.Qi, L),
                "bank": lambda: ops.resample_sinc_backward(g, L, orig, new, taps, bank.width, bank.kernel)}
        out["backward_bit_identical"] = torch.equal(back["direct"](), back["bank"]())
        out["backward_ms"] = alternate(back, args.calls, args.rounds, args.warmup, ev)
    if "train" in args.legs:
        xr = x.clone().requires_grad_()

        def fb(fn):
            xr.grad = None
            fn(xr).backward(g)

        legs = {"direct": lambda: fb(direct), "conv1d": lambda: fb(lambda v: conv_route(v, bank.kernel, orig, new, bank.width)),
                "bank": lambda: fb(bank)}
        legs["direct"]()
        g_direct = xr.grad.clone()
        legs["conv1d"]()
        out["train_grad_rel_max"] = float((g_direct - xr.grad).abs().max() / xr.grad.abs().max())
        out["train_ms"] = alternate(legs, args.train_calls, args.rounds, args.warmup, ev)
        out["train_peak_bytes"] = {k: peak_above(v) for k, v in legs.items()}
    print(json.dumps(out), flush=True)
    return out


def pitch_stage(args, dev, ev):
    sr, B = 44100, args.pitch_clips
    L = int(sr * args.seconds)
    ps = A.PitchShift(sr, args.n_steps).to(dev)
    resample = A.Resample(ps.orig_freq, sr, direct=True).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    g = torch.randn(B, L, device=dev, generator=gen)
    # the tensors the chain hands each stage
    X = ps.stft(x)
    Xs = ps.stretch(X)
    yi = ps.stft.invert(Xs)
    ys = ps._fit(yi, int(round(L / ps.rate)))
    yr = resample(ys)
    gr = torch.randn_like(yr)
    stages = {"stft": (ps.stft, x, torch.randn_like(X)), "vocoder": (ps.stretch, X, torch.randn_like(Xs)),
              "istft": (ps.stft.invert, Xs, torch.randn_like(yi)),
              "resample": (resample, ys, gr)}
    out = {"stage": "pitch", "n_steps": args.n_steps, "clips": B, "L": L, "orig": resample.orig, "new": resample.new,
           "Qi": resample.Qi, "table_bytes": resample.table.numel() * 4, "frames": X.shape[-2], "stretched": Xs.shape[-2],
           "table_in_lds": ops.sinc_interp_plan(resample.orig, resample.new, resample.Qi)[1]}
    del X, Xs, yi, yr

    def fb(fn, v, gy):
        v.grad = None
        fn(v).backward(gy)

    xr = x.clone().requires_grad_()
    legs = {"forward": lambda: ps(x), "forward+backward": lambda: fb(ps, xr, g)}
    out["whole_ms"] = alternate(legs, args.pitch_calls, args.rounds, args.warmup, ev)
    out["peak_bytes"] = {k: peak_above(v) for k, v in legs.items()}
    fwd, both = {}, {}
    for name, (fn, v, gy) in stages.items():
        vr = v.detach().clone().requires_grad_()
        fwd[name] = (lambda fn=fn, v=v: fn(v))
        both[name] = (lambda fn=fn, vr=vr, gy=gy: fb(fn, vr, gy))
    out["stage_forward_ms"] = alternate(fwd, args.pitch_calls, args.rounds, args.warmup, ev)
    out["stage_both_ms"] = alternate(both, args.pitch_calls, args.rounds, args.warmup, ev)
    print(json.dumps(out), flush=True)
    return out


def report(args, conv, pitch):
    lines = ["# Bankless converter and PitchShift probe (tools/sinc_interp_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one"
             % args.rounds, "process.  %d clips x %.1f s." % (args.clips, args.seconds), ""]
    if any("forward_ms" in r for r in conv):
        lines += ["## ops.resample_direct against at_resample_sinc (same shape, same bits)", "",
                  "| (orig, new) | L | taps, of them not zero | table in LDS | direct ms | bank ms | bank / direct | direct GB/s of the floor | bit-identical | expectation (not slower) |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for r in conv:
            if "forward_ms" in r:
                d, b = r["forward_ms"]["direct"], r["forward_ms"]["bank"]
                lines.append("| (%d, %d) | %d | %d, %d | %s | %s | %s | %.1f | %.0f | %s | %s |" % (
                    r["orig"], r["new"], r["L"], r["taps"], r["live_taps"], r["table_in_lds"], fmt(d), fmt(b),
                    b["ms"] / d["ms"], r["forward_GBps"]["direct"], r["forward_bit_identical"], verdict(d, b)))
        lines += ["", "## the same kernel with the rates exchanged against at_resample_sinc_backward", "",
                  "| (orig, new) | direct ms | bank ms | bank / direct | bit-identical | expectation (not slower) |", "|---|---|---|---|---|---|"]
        for r in conv:
            if "backward_ms" in r:
                d, b = r["backward_ms"]["direct"], r["backward_ms"]["bank"]
                lines.append("| (%d, %d) | %s | %s | %.2f | %s | %s |" % (
                    r["orig"], r["new"], fmt(d), fmt(b), b["ms"] / d["ms"], r["backward_bit_identical"], verdict(d, b)))
        lines.append("")
    if any("train_ms" in r for r in conv):
        lines += ["## forward + backward through Resample(direct=True) against conv1d with torch's backward, and against the bank route", "",
                  "| (orig, new) | direct ms | conv1d ms | bank ms | direct / conv1d | peak MiB above inputs: direct, conv1d | gradients differ by (normwise) | expectation (not slower than conv1d) |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in conv:
            if "train_ms" in r:
                d, c, b = (r["train_ms"][k] for k in ("direct", "conv1d", "bank"))
                lines.append("| (%d, %d) | %s | %s | %s | %.2f | %.1f, %.1f | %.1e | %s |" % (
                    r["orig"], r["new"], fmt(d), fmt(c), fmt(b), d["ms"] / c["ms"], r["train_peak_bytes"]["direct"] / 2 ** 20,
                    r["train_peak_bytes"]["conv1d"] / 2 ** 20, r["train_grad_rel_max"], verdict(d, c)))
        lines.append("")
    for r in pitch:
        w = r["whole_ms"]
        lines += ["## PitchShift(n_steps=%g), %d clips x %d samples: %d -> %d, table %d B (in LDS: %s), %d -> %d frames"
                  % (r["n_steps"], r["clips"], r["L"], r["orig"], r["new"], r["table_bytes"], r["table_in_lds"], r["frames"],
                     r["stretched"]), "",
                  "forward %s ms, peak %.0f MiB above the input; forward + backward %s ms, peak %.0f MiB.  Recorded only."
                  % (fmt(w["forward"]), r["peak_bytes"]["forward"] / 2 ** 20, fmt(w["forward+backward"]),
                     r["peak_bytes"]["forward+backward"] / 2 ** 20), "",
                  "| stage alone | forward ms | share of the stages | forward + backward ms | share of the stages |", "|---|---|---|---|---|"]
        tf = sum(v["ms"] for v in r["stage_forward_ms"].values())
        tb = sum(v["ms"] for v in r["stage_both_ms"].values())
        for k in r["stage_forward_ms"]:
            f, b = r["stage_forward_ms"][k], r["stage_both_ms"][k]
            lines.append("| %s | %s | %.0f %% | %s | %.0f %% |" % (k, fmt(f), 100 * f["ms"] / tf, fmt(b), 100 * b["ms"] / tb))
        lines += ["| sum | %.4f | | %.4f | |" % (tf, tb), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--ratios", type=int, nargs="+", default=[147, 160, 160, 147, 441, 160, 1, 2, 2, 1])
    ap.add_argument("--legs", nargs="+", default=["forward", "train", "pitch"], choices=["forward", "train", "pitch"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--train-calls", type=int, default=2)
    ap.add_argument("--n-steps", type=float, default=4.0)
    ap.add_argument("--pitch-clips", type=int, default=1024)
    ap.add_argument("--pitch-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "sinc_interp_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    pairs = list(zip(args.ratios[::2], args.ratios[1::2]))
    conv = [converter_stage(args, dev, ev, r) for r in pairs] if {"forward", "train"} & set(args.legs) else []
    pitch = [pitch_stage(args, dev, ev)] if "pitch" in args.legs else []
    report(args, conv, pitch)


if __name__ == "__main__":
    main()

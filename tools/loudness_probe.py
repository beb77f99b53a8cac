"""Gated loudness (sos_filter.hip's hop endings, loudness.hip) against what it replaces, in one process, the legs of a
comparison alternated per round (device-synchronised, warmed up, K calls per timed region; median, min and max over the
rounds), with the helpers of tools/resample_probe.py:

  kernel    at_sos_hop_power against at_sos_filter on the same input with the same two K-weighting sections: the same chains
            without the store.  Expected: not slower, beyond the spread the probe measures.  at_sos_filter_hop_scaled too.
  forward   Loudness.forward against the composed route -- ops.sos_filter, then square, reshape into hops, mean, unfold into
            blocks, mean, masked means in torch -- with the peak memory above the input.  Expected: not slower, less memory.
  train     forward + backward against torch autograd of the composed route (SosFilterFunction underneath): time, peak memory,
            and how far the two gradients are apart.
  long      one row of --long-row samples: a row is one workgroup, here as for SOSFilter.
  parent    with --parent-lib (a library built from the commit before, `make BUILD=... OUT=...`): at_sos_filter forward and
            reverse of both libraries on the same input, compared with torch.equal and timed against each other.

at --clips stereo clips x --seconds s at 48 kHz.  Nobody measured any of this before: whatever misses is written down as a
miss.  Writes a markdown report (--out, default profiles/loudness_probe.md) and prints one JSON line per stage."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_probe import alternate, fmt, peak_above, verdict  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402
from acids_transforms_amd.autograd import SosFilterFunction  # noqa: E402
from acids_transforms_amd.utils import filter_design as fd  # noqa: E402

SR = 48000
HOP = 4800


def clips_of(args, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(args.clips, 2, int(SR * args.seconds), device=dev, generator=gen) * 0.1
    x[::2, :, x.shape[-1] // 2:] *= 0.01                  # every other clip: a second half that the relative gate drops
    return x


def composed(x, co, grad=False):
    """Integrated loudness from existing ops and torch: what a user writes without the fused kernels."""
    clips, C, L = x.shape
    nh = L // HOP
    y = SosFilterFunction.apply(x, co, False) if grad else ops.sos_filter(x, co)
    s = (y[..., :nh * HOP] ** 2).reshape(clips, C, nh, HOP).mean(-1)
    blocks = s.unfold(-1, 4, 1).mean(-1)                                 # (clips, C, nb) from a (clips, C, nb, 4) view
    G = torch.tensor(ops.LOUDNESS_CHANNEL_WEIGHTS[:C], device=x.device)
    p = (blocks * G[:, None]).sum(-2)
    J1 = p > ops.LOUDNESS_ABS_THRESHOLD
    p_abs = (p * J1).sum(-1) / J1.sum(-1)
    J2 = J1 & (p > ops.LOUDNESS_REL_RATIO * p_abs[..., None])
    return -0.691 + 10.0 * torch.log10((p * J2).sum(-1) / J2.sum(-1))


def kernel_stage(args, dev, ev):
    x = clips_of(args, dev, 0).reshape(-1, int(SR * args.seconds))
    rows, L = x.shape
    co = ops.sos_coefficients(fd.k_weighting(SR))
    w = torch.rand(rows, L // HOP, dtype=torch.float64, device=dev)
    legs = {"hop_power": lambda: ops.sos_hop_power(x, co, HOP), "filter": lambda: ops.sos_filter(x, co),
            "hop_scaled": lambda: ops.sos_filter_hop_scaled(x, co, HOP, w)}
    out = {"stage": "kernel", "rows": rows, "L": L, "hop": HOP, "plan": ops.sos_hop_power_plan(rows, L, co.n, HOP),
           "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev)}
    out["read_TBps"] = rows * L * 4 / (out["ms"]["hop_power"]["ms"] * 1e-3) / 1e12
    print(json.dumps(out), flush=True)
    return out


def forward_stage(args, dev, ev):
    x = clips_of(args, dev, 1)
    co = ops.sos_coefficients(fd.k_weighting(SR))
    m = A.Loudness(sr=SR).to(dev)
    legs = {"fused": lambda: m(x), "composed": lambda: composed(x, co)}
    out = {"stage": "forward", "clips": x.shape[0], "L": x.shape[-1], "input_MiB": x.numel() * 4 / 2 ** 20,
           "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev),
           "peak_MiB": {k: peak_above(fn) / 2 ** 20 for k, fn in legs.items()},
           "differ_LU": float((m(x).double() - composed(x, co).double()).abs().max())}
    print(json.dumps(out), flush=True)
    return out


def train_stage(args, dev, ev):
    x = clips_of(args, dev, 2)
    co = ops.sos_coefficients(fd.k_weighting(SR))
    m = A.Loudness(sr=SR).to(dev)
    xr = x.clone().requires_grad_()

    def fb(fn):
        xr.grad = None
        fn(xr).sum().backward()
        return xr.grad

    legs = {"fused": lambda: fb(m), "composed": lambda: fb(lambda t: composed(t, co, grad=True))}
    ga, gb = legs["fused"]().clone(), legs["composed"]().clone()
    out = {"stage": "train", "clips": x.shape[0], "L": x.shape[-1], "input_MiB": x.numel() * 4 / 2 ** 20,
           "ms": alternate(legs, args.train_calls, args.rounds, args.warmup, ev),
           "peak_MiB": {k: peak_above(fn) / 2 ** 20 for k, fn in legs.items()},
           "gradients_differ": float((ga - gb).abs().max() / gb.abs().max())}
    print(json.dumps(out), flush=True)
    return out


def long_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(1, args.long_row, device=dev, generator=gen) * 0.1
    co = ops.sos_coefficients(fd.k_weighting(SR))
    legs = {"hop_power": lambda: ops.sos_hop_power(x, co, HOP), "filter": lambda: ops.sos_filter(x, co)}
    out = {"stage": "long", "L": args.long_row, "ms": alternate(legs, 1, args.rounds, args.warmup, ev)}
    print(json.dumps(out), flush=True)
    return out


def parent_stage(args, dev, ev):
    """at_sos_filter of this build against a library built from the parent commit: same bits, same time?"""
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    sig = _lib._SIGNATURES["at_sos_filter"]
    parent.at_sos_filter.argtypes, parent.at_sos_filter.restype = sig, ctypes.c_int
    parent.at_init.argtypes, parent.at_init.restype = [ctypes.c_int], ctypes.c_int
    assert parent.at_init(0) == 0
    x = clips_of(args, dev, 4).reshape(-1, int(SR * args.seconds))
    rows, L = x.shape
    equal = {}
    timed = {}
    for name, n in (("kweighting", None), ("cascade16", 16)):
        sos = fd.k_weighting(SR) if n is None else \
            np.concatenate([fd.equalizer(SR, 100.0 * 1.4 ** i, 3.0 if i % 2 else -3.0, 2.0) for i in range(n)])
        co = ops.sos_coefficients(sos)

        def old(reverse, co=co):
            y = torch.empty_like(x)
            rc = parent.at_sos_filter(_lib.ptr(x), rows, L, co.ptr, co.n, int(reverse), None, None, _lib.ptr(y), _lib.stream_ptr())
            assert rc == 0
            return y

        equal[name] = bool(torch.equal(old(False), ops.sos_filter(x, co)) and
                           torch.equal(old(True), ops.sos_filter(x, co, reverse=True)))
        legs = {"this": lambda co=co: ops.sos_filter(x, co), "parent": lambda: old(False)}
        timed[name] = alternate(legs, args.calls, args.rounds, args.warmup, ev)
    zi = torch.randn(rows, 2, 2, dtype=torch.float64, device=dev)
    co = ops.sos_coefficients(fd.k_weighting(SR))
    y_new, zf_new = ops.sos_filter(x, co, zi=zi, return_state=True)
    y_old, zf_old = torch.empty_like(x), torch.empty_like(zi)
    assert parent.at_sos_filter(_lib.ptr(x), rows, L, co.ptr, co.n, 0, _lib.ptr(zi), _lib.ptr(zf_old), _lib.ptr(y_old),
                                _lib.stream_ptr()) == 0
    equal["with state"] = bool(torch.equal(y_new, y_old) and torch.equal(zf_new, zf_old))
    out = {"stage": "parent", "rows": rows, "L": L, "equal": equal, "ms": timed}
    print(json.dumps(out), flush=True)
    return out


def report(args, kernel, forward, train, long_row, parent):
    lines = ["# Loudness probe (tools/loudness_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one"
             % args.rounds, "process.  %d stereo clips x %.1f s at %d Hz, hop %d.  An expectation is met when the median is no"
             % (args.clips, args.seconds, SR, HOP), "slower than the other leg's beyond the larger of the two spreads.", ""]
    if kernel:
        hp, f, hs = kernel["ms"]["hop_power"], kernel["ms"]["filter"], kernel["ms"]["hop_scaled"]
        lines += ["## (a) at_sos_hop_power against at_sos_filter (%d rows x %d samples, two sections; tile %d, dispatch %d)"
                  % (kernel["rows"], kernel["L"], kernel["plan"][0], kernel["plan"][2]), "",
                  "| hop power ms | filter ms | hop power / filter | audio read TB/s | expectation (not slower) | hop scaled ms |",
                  "|---|---|---|---|---|---|",
                  "| %s | %s | %.2f | %.2f | %s | %s |" % (fmt(hp), fmt(f), hp["ms"] / f["ms"], kernel["read_TBps"],
                                                           verdict(hp, f), fmt(hs)), ""]
    if forward:
        a, b = forward["ms"]["fused"], forward["ms"]["composed"]
        lines += ["## (b) Loudness.forward against the composed route (input %.0f MiB)" % forward["input_MiB"], "",
                  "| fused ms | composed ms | fused / composed | expectation (not slower) | fused peak MiB above the input | composed peak MiB | results differ by (LU) |",
                  "|---|---|---|---|---|---|---|",
                  "| %s | %s | %.2f | %s | %.1f | %.1f | %.1e |" % (fmt(a), fmt(b), a["ms"] / b["ms"], verdict(a, b),
                                                                    forward["peak_MiB"]["fused"],
                                                                    forward["peak_MiB"]["composed"], forward["differ_LU"]), ""]
    if train:
        a, b = train["ms"]["fused"], train["ms"]["composed"]
        lines += ["## (c) forward + backward against torch autograd of the composed route", "",
                  "| fused ms | composed ms | fused / composed | fused peak MiB above the input | composed peak MiB | gradients differ by (normwise) |",
                  "|---|---|---|---|---|---|",
                  "| %s | %s | %.2f | %.1f | %.1f | %.1e |" % (fmt(a), fmt(b), a["ms"] / b["ms"], train["peak_MiB"]["fused"],
                                                              train["peak_MiB"]["composed"], train["gradients_differ"]), ""]
    if long_row:
        lines += ["## (d) one row of %d samples: one workgroup walks it (no dispatch splits a row)" % long_row["L"], "",
                  "| hop power ms | filter ms |", "|---|---|",
                  "| %s | %s |" % (fmt(long_row["ms"]["hop_power"]), fmt(long_row["ms"]["filter"])), ""]
    if parent:
        lines += ["## at_sos_filter against the parent commit's library (%d rows x %d samples)" % (parent["rows"], parent["L"]),
                  "", "| filter | forward and reverse torch.equal | this build ms | parent ms | this / parent | within the spread |",
                  "|---|---|---|---|---|---|"]
        for name, ms in parent["ms"].items():
            lines.append("| %s | %s | %s | %s | %.3f | %s |" % (name, "yes" if parent["equal"][name] else "NO", fmt(ms["this"]),
                                                                fmt(ms["parent"]), ms["this"]["ms"] / ms["parent"]["ms"],
                                                                "yes" if verdict(ms["this"], ms["parent"]) == "met" else "NO"))
        lines += ["", "With zi and zf (K-weighting): output and final state torch.equal: %s."
                  % ("yes" if parent["equal"]["with state"] else "NO"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--legs", nargs="+", default=["kernel", "forward", "train", "long"],
                    choices=["kernel", "forward", "train", "long"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--train-calls", type=int, default=2)
    ap.add_argument("--long-row", type=int, default=2 ** 24)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "loudness_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel = kernel_stage(args, dev, ev) if "kernel" in args.legs else None
    forward = forward_stage(args, dev, ev) if "forward" in args.legs else None
    train = train_stage(args, dev, ev) if "train" in args.legs else None
    long_row = long_stage(args, dev, ev) if "long" in args.legs else None
    parent = parent_stage(args, dev, ev) if args.parent_lib else None
    report(args, kernel, forward, train, long_row, parent)


if __name__ == "__main__":
    main()

"""Streaming PQMF against the route that was available without it, in one process, the two alternated per round:

  stream    transforms.RealtimePQMF: one launch per call, the window staged from [state buffer | chunk], the new state
            written by the kernel
  composed  torch.cat([state, chunk]) -> the offline PQMF.forward / invert -> the slice of the chunk's blocks -> the copy
            of the new state (what a user had to write before; the same sums, so the outputs are compared to the bit)

at 256 streams, 16 bands, 513 taps and chunks of 16, 1024 and 4096 samples, for forward, invert and forward + backward
of each (the backward through torch autograd on both routes).  Device-synchronised, warmed up, K calls per timed
region; median, min and max over the rounds, and the bytes a streaming call must move over its time.

With --parent-lib PATH (a libacids_hip.so built from the parent commit) the offline kernels are timed through the C ABI
of both libraries, alternated, at 1024 clips x 176 400 samples, and their outputs compared to the bit.

Writes a markdown report (--out, default profiles/pqmf_stream_probe.md) and prints one JSON line per stage."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402


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


class Composed:
    """The streaming bank written with the offline module: state tensors, cat, slice, copy.  P must be a multiple of M
    (it is at the defaults), so that the delayed blocks are blocks of the offline module on [state | chunk]."""

    def __init__(self, pq):
        self.pq, self.M = pq, pq.n_band
        P = (pq.taps - 1) // 2
        assert P % self.M == 0
        self.D, self.Ha, self.Hs = ops.pqmf_stream_sizes(pq.n_band, pq.taps)
        self.state = self.bstate = None

    def forward(self, x):
        if self.state is None:
            self.state = x.new_zeros(x.shape[:-1] + (self.Ha,))
        buf = torch.cat([self.state, x], -1)
        c = x.shape[-1] // self.M
        y = self.pq(buf)[..., self.D:self.D + c]
        self.state = buf[..., -self.Ha:].detach().clone()
        return y

    def invert(self, y):
        if self.bstate is None:
            self.bstate = y.new_zeros(y.shape[:-1] + (self.Hs,))
        buf = torch.cat([self.bstate, y], -1)
        lo = (self.Hs - self.D) * self.M
        x = self.pq.invert(buf)[..., lo:lo + y.shape[-1] * self.M]
        self.bstate = buf[..., -self.Hs:].detach().clone()
        return x


def stream_stage(args, dev, ev):
    B, M, N = args.streams, args.n_band, args.taps
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []
    for C in args.chunks:
        c = C // M
        rt, pq = A.RealtimePQMF(M, N).to(dev), A.PQMF(M, N).to(dev)
        comp = Composed(pq)
        x = [torch.randn(B, C, device=dev, generator=gen) * 0.1 for _ in range(3)]
        y = [torch.randn(B, M, c, device=dev, generator=gen) * 0.1 for _ in range(3)]
        # the two routes compute the same sums: to the bit over three chunks
        same = all(torch.equal(rt(v), comp.forward(v)) for v in x) and all(torch.equal(rt.invert(v), comp.invert(v)) for v in y)
        gy, gx = torch.randn(B, M, c, device=dev, generator=gen), torch.randn(B, C, device=dev, generator=gen)
        xr, yr = x[0].clone().requires_grad_(), y[0].clone().requires_grad_()

        def fb(fn, leaf, g):
            leaf.grad = None
            fn(leaf).backward(g)

        legs = {"stream_forward": lambda: rt(x[0]), "composed_forward": lambda: comp.forward(x[0]),
                "stream_invert": lambda: rt.invert(y[0]), "composed_invert": lambda: comp.invert(y[0]),
                "stream_forward+backward": lambda: fb(rt, xr, gy), "composed_forward+backward": lambda: fb(comp.forward, xr, gy),
                "stream_invert+backward": lambda: fb(rt.invert, yr, gx), "composed_invert+backward": lambda: fb(comp.invert, yr, gx)}
        ms = alternate(legs, args.calls, args.rounds, args.warmup, ev)
        # what a streaming call must move: chunk in, chunk out, state in, state out (fp32)
        bytes_call = {"forward": 4 * B * (2 * C + 2 * comp.Ha), "invert": 4 * B * (2 * C + 2 * M * comp.Hs)}
        out = {"stage": "stream", "streams": B, "n_band": M, "taps": N, "chunk": C, "bit_identical_to_composed": same,
               "calls_per_region": args.calls, "rounds": args.rounds, "ms": ms,
               "GBps": {k: bytes_call[k] / (ms["stream_" + k]["ms"] * 1e-3) / 1e9 for k in bytes_call},
               "bytes_per_call": bytes_call}
        print(json.dumps(out), flush=True)
        results.append(out)
    return results


def offline_stage(args, dev, ev):
    B, L, M, N = args.clips, args.samples, args.n_band, args.taps
    pq = A.PQMF(M, N).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    z = torch.randn(B, M, L // M, device=dev, generator=gen) * 0.1
    libs = {"this": _lib.lib()}
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("at_pqmf_analysis", "at_pqmf_synthesis"):
            getattr(parent, name).argtypes = _lib._SIGNATURES[name]
            getattr(parent, name).restype = ctypes.c_int
        libs["parent"] = parent
    outs, legs = {}, {}
    for tag, lib in libs.items():
        ya, xs = torch.empty(B, M, L // M, device=dev), torch.empty(B, L, device=dev)
        outs[tag] = (ya, xs)

        def analysis(lib=lib, ya=ya):
            _lib.check(lib.at_pqmf_analysis(_lib.ptr(x), B, L, _lib.ptr(pq.prototype), N, M, _lib.ptr(pq.modulation), 1.0,
                                            _lib.ptr(ya), _lib.stream_ptr()), "at_pqmf_analysis")

        def synthesis(lib=lib, xs=xs):
            _lib.check(lib.at_pqmf_synthesis(_lib.ptr(z), B, L, _lib.ptr(pq.prototype), N, M, _lib.ptr(pq.modulation),
                                             float(M), _lib.ptr(xs), _lib.stream_ptr()), "at_pqmf_synthesis")

        legs[tag + "_analysis"], legs[tag + "_synthesis"] = analysis, synthesis
    ms = alternate(legs, args.offline_calls, args.rounds, args.warmup, ev)
    out = {"stage": "offline", "clips": B, "samples": L, "n_band": M, "taps": N, "ms": ms}
    if args.parent_lib:
        out["bit_identical_to_parent"] = {"analysis": torch.equal(outs["this"][0], outs["parent"][0]),
                                          "synthesis": torch.equal(outs["this"][1], outs["parent"][1])}
    print(json.dumps(out), flush=True)
    return out


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["ms"], s["min_ms"], s["max_ms"])


def report(args, stream, offline):
    lines = ["# Streaming PQMF probe (tools/pqmf_stream_probe.py)", "",
             "%d streams, %d bands, %d taps; ms per call as median (min .. max) over %d rounds of %d calls, device-synchronised,"
             % (args.streams, args.n_band, args.taps, args.rounds, args.calls),
             "the two routes alternated in one process.  `composed` = torch.cat([state, chunk]) + offline PQMF + slice + state copy.", ""]
    met_all = True
    for r in stream:
        lines += ["## chunk of %d samples (bit-identical to the composed route: %s)" % (r["chunk"], r["bit_identical_to_composed"]), "",
                  "| leg | stream ms | composed ms | stream / composed | expectation (not slower beyond the spread) |", "|---|---|---|---|---|"]
        for leg in ("forward", "invert", "forward+backward", "invert+backward"):
            s, c = r["ms"]["stream_" + leg], r["ms"]["composed_" + leg]
            met = s["ms"] <= c["ms"] + max(s["max_ms"] - s["min_ms"], c["max_ms"] - c["min_ms"])
            met_all = met_all and met
            lines.append("| %s | %s | %s | %.2f | %s |" % (leg, fmt(s), fmt(c), s["ms"] / c["ms"], "met" if met else "MISSED"))
        lines += ["", "Bytes a streaming call must move: forward %d, invert %d -> %.1f GB/s and %.1f GB/s over the call's time."
                  % (r["bytes_per_call"]["forward"], r["bytes_per_call"]["invert"], r["GBps"]["forward"], r["GBps"]["invert"]), ""]
    lines += ["Every expectation met: %s." % ("yes" if met_all else "NO"), ""]
    if offline is not None:
        lines += ["## offline kernels, %d clips x %d samples, through the C ABI" % (offline["clips"], offline["samples"]), "",
                  "| kernel | ms |", "|---|---|"]
        lines += ["| %s | %s |" % (k, fmt(v)) for k, v in offline["ms"].items()]
        if "bit_identical_to_parent" in offline:
            lines += ["", "Outputs bit-identical to the parent build's: analysis %s, synthesis %s."
                      % (offline["bit_identical_to_parent"]["analysis"], offline["bit_identical_to_parent"]["synthesis"])]
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--n-band", type=int, default=16)
    ap.add_argument("--taps", type=int, default=513)
    ap.add_argument("--chunks", type=int, nargs="+", default=[16, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=176400)
    ap.add_argument("--offline-calls", type=int, default=5)
    ap.add_argument("--skip-offline", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pqmf_stream_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = stream_stage(args, dev, ev)
    offline = None if args.skip_offline else offline_stage(args, dev, ev)
    report(args, stream, offline)


if __name__ == "__main__":
    main()

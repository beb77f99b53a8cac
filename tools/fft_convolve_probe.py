"""The long-filter convolution (fft_convolve.hip through ops.fft_convolve / autograd.FFTConvolveFunction) against the routes
a user had before it, in one process, the legs of a comparison alternated per round (device-synchronised, warmed up, K calls
per timed region; median, min and max over the rounds), with the helpers of tools/resample_probe.py:

  routes    forward, forward + backward with x requiring grad, and with h requiring grad too, against (1) one full-length
            torch.fft.rfft . irfft convolution with torch's autograd, at n = L + K - 1 as torchaudio.functional.fftconvolve
            takes it and at the next power of two, and (2) at the taps in --conv1d-taps, torch.nn.functional.conv1d and its
            backward with respect to the signal (its gradient with respect to a long filter is too slow to time here);
            the peak memory above the inputs of every route; the forward results compared normwise
  kernel    at_spectral_fir alone on one chunk of rows against a copy of the same spectrum: time, bytes moved over the floor
            (2 rows T F + P F) x 8, complex multiply-adds per second
  blocks    the forward at the rule's block against its neighbours in the ladder, by block=

at --clips clips x --seconds s of 44.1 kHz audio, one shared filter of each of --taps taps.  Nothing here was measured before:
the expectation is "not slower than what a user can do today, and less memory", and every miss is written down as a miss.
Writes a markdown report (--out, default profiles/fft_convolve_probe.md), whose last sections list the misses worked out from
the figures and any --note lines, and prints one JSON line per leg and stage.  An error other than "this build cannot run
the route" ends the probe."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_probe import alternate, fmt, peak_above, verdict  # noqa: E402
import torch  # noqa: E402

from acids_transforms_amd import ops  # noqa: E402
from acids_transforms_amd.autograd import FFTConvolveFunction  # noqa: E402

SR = 44100


def fft_route(x, h, n):
    """One transform of n >= L + K - 1 points per row: what torchaudio.functional.fftconvolve does (n = L + K - 1)."""
    M = x.shape[-1] + h.shape[-1] - 1
    return torch.fft.irfft(torch.fft.rfft(x, n=n) * torch.fft.rfft(h, n=n), n=n)[..., :M]


def conv1d_route(x, h):
    K = h.shape[-1]
    return torch.nn.functional.conv1d(torch.nn.functional.pad(x[:, None], (K - 1, K - 1)), h.flip(-1)[None, None])[:, 0]


def _inputs(args, dev, K, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    L = int(SR * args.seconds)
    x = torch.randn(args.clips, L, device=dev, generator=gen) * 0.1
    h = torch.randn(K, device=dev, generator=gen) * torch.exp(-torch.arange(K, device=dev) / (K / 4.0))
    return x, h / h.abs().sum()


def _unsupported(e):
    """Is this the error of a route that this build of torch does not have (torch.fft without a backend, say)?"""
    text = str(e).lower()
    return isinstance(e, NotImplementedError) or (isinstance(e, RuntimeError) and any(
        w in text for w in ("not implemented", "not supported", "not compiled", "not available")))


def _try(fn, what):
    """Run a leg once (its first run: libraries pick their algorithms here) and once more on the host clock: (reason or None,
    seconds of the second run).  Only "this build cannot run the route" is recorded and passed over; every other error --
    a device fault among them -- ends the probe, which starts nothing more on the card."""
    try:
        fn()
        torch.cuda.synchronize()
    except (NotImplementedError, RuntimeError) as e:
        if not _unsupported(e):
            raise
        err = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:160])
        print(json.dumps({"leg": what, "unsupported": err}), flush=True)
        return err, 0.0
    t = time.time()
    fn()
    torch.cuda.synchronize()
    t = time.time() - t
    print(json.dumps({"leg": what, "one_run_s": round(t, 4)}), flush=True)
    return None, t


def routes_stage(args, dev, ev, K):
    x, h = _inputs(args, dev, K, K)
    L = x.shape[1]
    M = L + K - 1
    pow2 = 1 << (M - 1).bit_length()
    g = torch.randn(args.clips, M, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    routes = {"hip": lambda a, b: FFTConvolveFunction.apply(a, b, "full", None),
              "fft n=L+K-1": lambda a, b: fft_route(a, b, M), "fft n=2^k": lambda a, b: fft_route(a, b, pow2)}
    if K in args.conv1d_taps:
        routes["conv1d"] = conv1d_route
    no_weight_grad = ("conv1d",)              # its gradient with respect to a long filter is not timed here: too slow

    def train(route, both):
        xr.grad = hr.grad = None
        route(xr, hr if both else h).backward(g)

    out = {"stage": "routes", "K": K, "clips": args.clips, "L": L, "plan": ops.fft_convolve_plan(L, K), "pow2": pow2,
           "skipped": {}, "ms": {}, "peak_MiB": {}, "differ": {}}
    with torch.no_grad():
        ref = ops.fft_convolve(x, h)
    for kind in ("forward", "forward+gx", "forward+gx+gh"):
        legs = {}
        for name, route in routes.items():
            if kind.endswith("gh") and name in no_weight_grad:
                out["skipped"]["%s %s" % (name, kind)] = "not timed by this tool (slow)"
                continue
            if kind == "forward":
                fn = (lambda route=route: route(x, h))
            else:
                fn = (lambda route=route, both=kind.endswith("gh"): train(route, both))
            err, one = _try(fn, "%d taps, %s, %s" % (K, name, kind))
            if err is None and one > args.slow_leg:
                err = "one run took %.1f s: too slow to alternate with the others, timed once" % one
            if err:
                out["skipped"]["%s %s" % (name, kind)] = err
                continue
            legs[name] = fn
            out["peak_MiB"]["%s %s" % (name, kind)] = peak_above(fn) / 2 ** 20
            if kind == "forward" and name != "hip":
                with torch.no_grad():
                    out["differ"][name] = float((route(x, h) - ref).abs().max() / ref.abs().max())
        out["ms"][kind] = alternate(legs, args.calls, args.rounds, args.warmup, ev)
        xr.grad = hr.grad = None
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def kernel_stage(args, dev, ev, K):
    L = int(SR * args.seconds)
    B, T, P, tile, chunk = ops.fft_convolve_plan(L, K)
    rows, F = min(chunk, args.clips), B + 1
    gen = torch.Generator(device=dev).manual_seed(K)
    X = torch.view_as_complex(torch.randn(rows, T, F, 2, device=dev, generator=gen))
    H = torch.view_as_complex(torch.randn(P, F, 2, device=dev, generator=gen))
    legs = {"spectral_fir": lambda: ops.spectral_fir(X, H), "anticausal conj": lambda: ops.spectral_fir(X, H, True, True),
            "copy": lambda: X.clone()}
    ms = alternate(legs, args.kernel_calls, args.rounds, args.warmup, ev)
    floor = (2 * rows * T * F + P * F) * 8
    cmacs = rows * F * sum(min(t + 1, P) for t in range(T))
    out = {"stage": "kernel", "K": K, "B": B, "T": T, "P": P, "rows": rows, "tile": tile, "floor_bytes": floor,
           "cmacs": cmacs, "ms": ms, "TBps": floor / (ms["spectral_fir"]["ms"] * 1e-3) / 1e12,
           "copy_TBps": 2 * rows * T * F * 8 / (ms["copy"]["ms"] * 1e-3) / 1e12,
           "Tcmacs": cmacs / (ms["spectral_fir"]["ms"] * 1e-3) / 1e12}
    print(json.dumps(out), flush=True)
    return out


def blocks_stage(args, dev, ev, K):
    x, h = _inputs(args, dev, K, K + 7)
    rule = ops.fft_convolve_plan(x.shape[1], K)[0]
    i = ops.FFT_CONVOLVE_BLOCKS.index(rule)
    legs = {}
    for b in ops.FFT_CONVOLVE_BLOCKS[max(i - 1, 0):i + 2]:
        legs["%d" % b] = (lambda b=b: ops.fft_convolve(x, h, block=b))
    out = {"stage": "blocks", "K": K, "rule": rule, "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev)}
    print(json.dumps(out), flush=True)
    return out


def misses(routes, kernels, blocks):
    """What the figures say against the expectations, worked out from them: a leg on which the HIP route is slower than an
    earlier route or needs more memory, a neighbour of the rule's block that wins beyond both spreads, and the partitions from
    which at_spectral_fir takes more than 1.5 x a copy of its spectrum (the counting said: memory-bound up to 16)."""
    out = []
    for r in routes:
        for kind, ms in r["ms"].items():
            for name, v in ms.items():
                if name == "hip" or "hip" not in ms:
                    continue
                if verdict(ms["hip"], v) != "met":
                    out.append("* %d taps, %s: slower than %s (%.2f against %.2f ms)." % (r["K"], kind, name, ms["hip"]["ms"], v["ms"]))
                mine, theirs = r["peak_MiB"]["hip %s" % kind], r["peak_MiB"]["%s %s" % (name, kind)]
                if mine > theirs:
                    out.append("* %d taps, %s: %.0f MiB above the inputs against %.0f for %s." % (r["K"], kind, mine, theirs, name))
    for b in blocks:
        rule = b["ms"]["%d" % b["rule"]]
        for k, v in b["ms"].items():
            if v["max_ms"] < rule["min_ms"]:
                out.append("* %d taps: block %s (%.2f ms) beats the rule's %d (%.2f ms) beyond both spreads."
                           % (b["K"], k, v["ms"], b["rule"], rule["ms"]))
    over = sorted((k["P"], k["ms"]["spectral_fir"]["ms"] / k["ms"]["copy"]["ms"]) for k in kernels)
    if over:
        out.append("* at_spectral_fir against a copy of its spectrum: %s."
                   % ", ".join("%.2f x at %d partitions" % (x, P) for P, x in over))
        anti = ["%.0f %% at %d" % (100 * (k["ms"]["anticausal conj"]["ms"] / k["ms"]["spectral_fir"]["ms"] - 1), k["P"])
                for k in sorted(kernels, key=lambda k: k["P"])]
        out.append("* the anticausal conjugate form against the causal one: +%s partitions." % ", +".join(anti))
    return ["## Misses and what the counting did not foresee", ""] + (out or ["* none."]) + [""]


def report(args, routes, kernels, blocks):
    lines = ["# Long-filter convolution probe (tools/fft_convolve_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one"
             % args.rounds, "process.  %d clips x %.1f s at %d Hz, one shared filter.  Expectation: the HIP route is not slower"
             % (args.clips, args.seconds, SR), "than a route a user had before (beyond the larger spread), and needs less memory.", ""]
    for r in routes:
        B, T, P, tile, chunk = r["plan"]
        lines += ["## %d taps: block %d, %d frames, %d partitions, chunks of %d rows (torch.fft at n = %d and n = %d)"
                  % (r["K"], B, T, P, chunk, r["L"] + r["K"] - 1, r["pow2"]), "",
                  "| leg | route | ms | peak MiB above the inputs | HIP against it | forward differs from HIP by (normwise) |",
                  "|---|---|---|---|---|---|"]
        for kind, ms in r["ms"].items():
            for name, v in ms.items():
                against = "" if name == "hip" or "hip" not in ms else "%.2f x, %s" % (ms["hip"]["ms"] / v["ms"], verdict(ms["hip"], v))
                differ = "%.1e" % r["differ"][name] if kind == "forward" and name in r["differ"] else ""
                lines.append("| %s | %s | %s | %.0f | %s | %s |" % (kind, name, fmt(v), r["peak_MiB"]["%s %s" % (name, kind)],
                                                                   against, differ))
        for what, err in r["skipped"].items():
            lines.append("| %s | did not run: %s | | | | |" % (what, err))
        lines.append("")
    if kernels:
        lines += ["## at_spectral_fir alone on one chunk of rows, against a copy of the spectrum", "",
                  "| taps | block | frames | partitions | rows | forward ms | anticausal conj ms | copy ms | floor MB | floor TB/s | copy TB/s | complex multiply-adds T/s | time / copy |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for k in kernels:
            m = k["ms"]
            lines.append("| %d | %d | %d | %d | %d | %s | %s | %s | %.0f | %.2f | %.2f | %.2f | %.2f |" % (
                k["K"], k["B"], k["T"], k["P"], k["rows"], fmt(m["spectral_fir"]), fmt(m["anticausal conj"]), fmt(m["copy"]),
                k["floor_bytes"] / 1e6, k["TBps"], k["copy_TBps"], k["Tcmacs"], m["spectral_fir"]["ms"] / m["copy"]["ms"]))
        lines.append("")
    if blocks:
        lines += ["## the block rule against its neighbours (forward, by block=)", "", "| taps | rule | block: ms |", "|---|---|---|"]
        for b in blocks:
            lines.append("| %d | %d | %s |" % (b["K"], b["rule"],"; ".join("%s: %s" % (k, fmt(v)) for k, v in b["ms"].items())))
        lines.append("")
    lines += misses(routes, kernels, blocks)
    if args.note:
        lines += ["## Notes", ""] + ["* " + n for n in args.note] + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--taps", type=int, nargs="+", default=[513, 4096, 22050, 66150])
    ap.add_argument("--conv1d-taps", type=int, nargs="*", default=[513])
    ap.add_argument("--legs", nargs="+", default=["routes", "kernel", "blocks"], choices=["routes", "kernel", "blocks"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--kernel-calls", type=int, default=5)
    ap.add_argument("--note", action="append", default=[], help="a line for the report's Notes section (repeatable)")
    ap.add_argument("--slow-leg", type=float, default=2.0, help="a leg whose one run takes longer (s) is timed once only")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "fft_convolve_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    routes, kernels, blocks = [], [], []
    for name, stage, into in (("kernel", kernel_stage, kernels), ("blocks", blocks_stage, blocks), ("routes", routes_stage, routes)):
        for K in args.taps if name in args.legs else ():
            into.append(stage(args, dev, ev, K))
            report(args, routes, kernels, blocks)          # after every stage: a run that is cut short leaves what it has


if __name__ == "__main__":
    main()

"""The streaming partitioned convolution (transforms.RealtimeImpulseResponse, at_spectral_fir_stream of fft_convolve.hip)
against the route a user had before it, at --streams streams, with the helpers of tools/resample_probe.py (device-
synchronised, warmed up, K calls per timed region; median, min and max over the rounds; the legs alternated per round):

  call      RealtimeImpulseResponse.forward on a chunk of 1 block and of 8 blocks against torch.cat([the last K - 1 samples,
            chunk]) -> the offline ops.fft_convolve(., "full", block=B) -> the slice of the chunk's samples -> the copy of the
            new K - 1 samples; the two outputs compared normwise
  kernel    at_spectral_fir_stream alone at Tc = 1 and Tc = 8 against its byte floor rows (P - 1 + 2 Tc) F 8 + P F 8

for every (taps, block) of --taps x (the plan's block, 128, 256).  The driver never opens the device: every (taps, block) runs
in a child process of its own under a time limit (--leg-timeout), and after a child that failed or ran out of time nothing
more is started.  Expectation: the streaming form is not slower on any leg beyond the larger spread; nothing here was
measured before, and every miss is written down as a miss.  Writes a markdown report (--out, default
profiles/convolve_stream_probe.md) and prints one JSON line per leg."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def leg(args, K, block):
    import torch
    from resample_probe import alternate
    import acids_transforms_amd as A
    from acids_transforms_amd import ops

    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    gen = torch.Generator(device=dev).manual_seed(K)
    h = torch.randn(K, device=dev, generator=gen) * torch.exp(-torch.arange(K, device=dev) / (K / 4.0))
    h = h / h.abs().sum()
    m = A.RealtimeImpulseResponse(h.cpu(), block=block).to(dev)
    B, P, R, F = m.block, m.partitions, m.ring_slots, m.block + 1
    rows = args.streams
    out = {"K": K, "B": B, "P": P, "R": R, "rows": rows, "plan": block is None, "call": {}, "kernel": {}, "differ": {}}
    for n in (1, 8):
        C = n * B
        x = torch.randn(rows, C, device=dev, generator=gen) * 0.1
        state = {"hist": torch.zeros(rows, K - 1, device=dev)}

        def before():
            buf = torch.cat([state["hist"], x], dim=-1)
            y = ops.fft_convolve(buf, h, "full", block=B)[..., K - 1:K - 1 + C]
            state["hist"] = buf[..., C:].clone()
            return y

        with torch.no_grad():
            m.reset()
            state["hist"].zero_()
            for _ in range(3):                                       # the same three chunks through both: compared once
                a, b = m(x), before()
            out["differ"][str(n)] = float((a - b).abs().max() / b.abs().max())
            out["call"][str(n)] = alternate({"stream": lambda: m(x), "before": before}, args.calls, args.rounds, args.warmup, ev)
        Xc = torch.view_as_complex(torch.randn(rows, n, F, 2, device=dev, generator=gen))
        ring = torch.view_as_complex(torch.randn(rows, R, F, 2, device=dev, generator=gen))
        H = torch.view_as_complex(torch.randn(P, F, 2, device=dev, generator=gen))
        ms = alternate({"kernel": lambda: ops.spectral_fir_stream(Xc, ring, 3 % R, H)}, args.calls, args.rounds, args.warmup, ev)
        floor = rows * (P - 1 + 2 * n) * F * 8 + P * F * 8
        out["kernel"][str(n)] = dict(ms["kernel"], floor_bytes=floor, TBps=floor / (ms["kernel"]["ms"] * 1e-3) / 1e12)
    print("LEG " + json.dumps(out), flush=True)


def report(args, legs, stopped):
    from resample_probe import fmt, verdict
    lines = ["# Streaming convolution probe (tools/convolve_stream_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds of %d calls, device-synchronised, the two legs of a row alternated"
             % (args.rounds, args.calls), "in one process; every (taps, block) in a process of its own.  %d streams, one shared"
             % args.streams, "response.  `before`: torch.cat([last K - 1 samples, chunk]) -> ops.fft_convolve(., \"full\", block=B) -> slice ->",
             "copy of the new K - 1 samples.  Expectation: the streaming form is not slower beyond the larger spread.", "",
             "## RealtimeImpulseResponse.forward against the route before it", "",
             "| taps | block | partitions | chunk (blocks) | stream ms | before ms | stream / before | expectation | outputs differ by (normwise) |",
             "|---|---|---|---|---|---|---|---|---|"]
    missed = []
    for r in legs:
        for n, ms in r["call"].items():
            v = verdict(ms["stream"], ms["before"])
            lines.append("| %d | %d%s | %d | %s | %s | %s | %.2f | %s | %.1e |" % (
                r["K"], r["B"], " (plan)" if r["plan"] else "", r["P"], n, fmt(ms["stream"]), fmt(ms["before"]),
                ms["stream"]["ms"] / ms["before"]["ms"], v, r["differ"][n]))
            if v != "met":
                missed.append("* %d taps, block %d, chunks of %s: slower than the route before (%.3f against %.3f ms)."
                              % (r["K"], r["B"], n, ms["stream"]["ms"], ms["before"]["ms"]))
    lines += ["", "## at_spectral_fir_stream alone against its byte floor rows (P - 1 + 2 Tc) F 8 + P F 8", "",
              "| taps | block | partitions | Tc | ms | floor MB | floor TB/s |", "|---|---|---|---|---|---|---|"]
    slow = []
    for r in legs:
        for n, k in r["kernel"].items():
            lines.append("| %d | %d | %d | %s | %s | %.2f | %.3f |" % (r["K"], r["B"], r["P"], n, fmt(k), k["floor_bytes"] / 1e6, k["TBps"]))
            slow.append((k["TBps"], r["K"], r["B"], n))
    lines += ["", "## Misses and what the counting did not foresee", ""] + (missed or ["* no leg slower than the route before."])
    if slow:
        lo, hi = min(slow), max(slow)
        lines.append("* the kernel against its byte floor: from %.3f TB/s (%d taps, block %d, Tc %s) to %.3f TB/s (%d taps, block %d, "
                     "Tc %s); a launch that moves a few MB costs its launch, not its bytes." % (lo + hi))
    if stopped:
        lines.append("* the probe stopped early: %s." % stopped)
    if args.note:
        lines += ["", "## Notes", ""] + ["* " + n for n in args.note]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--taps", type=int, nargs="+", default=[513, 22050, 66150])
    ap.add_argument("--blocks", nargs="+", default=["plan", "128", "256"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--leg", nargs=2, metavar=("TAPS", "BLOCK"), help="run one (taps, block) in this process (the driver's child)")
    ap.add_argument("--note", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "convolve_stream_probe.md"))
    args = ap.parse_args()
    if args.leg:
        leg(args, int(args.leg[0]), None if args.leg[1] == "plan" else int(args.leg[1]))
        return 0
    legs, stopped = [], None
    common = ["--streams", str(args.streams), "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--calls", str(args.calls)]
    for K in args.taps:
        for block in args.blocks:
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", str(K), block] + common
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            got = [json.loads(line[4:]) for line in p.stdout.splitlines() if line.startswith("LEG ")]
            if p.returncode != 0 or not got:
                stopped = "%d taps, block %s ended with status %d: %s" % (K, block, p.returncode, p.stderr.strip().splitlines()[-1:] or "")
                break
            print(json.dumps(got[0]), flush=True)
            if not any(r["K"] == got[0]["K"] and r["B"] == got[0]["B"] for r in legs):       # the plan's block may be 128 or 256
                legs.append(got[0])
            report(args, legs, None)
        if stopped:
            break
    report(args, legs, stopped)
    print("stopped: %s" % stopped if stopped else "done", flush=True)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())

"""True peak (true_peak.hip) against what it replaces, in one process, the legs of a comparison alternated per round
(device-synchronised, warmed up, K calls per timed region; median, min and max over the rounds), with the helpers of
tools/resample_probe.py:

  offline   at_true_peak (ops.true_peak, the BS.1770 table) at --clips stereo clips x --seconds s at 48 kHz against the composed
            torch route on the same table (conv1d to P channels, abs, amax: time and peak memory), against a torch reduction
            that only reads the input (the 4-bytes-per-sample floor, measured) and against at_sos_filter at two sections on
            the same input, the neighbouring streaming-filter yardstick.  The generic copy ((2, 12) Kaiser) and the sample
            peak ride along.  Expected: not slower than the composed route.
  long      one row of --long-row samples: rows x tiles share one index, so a long row spreads over the chip.
  stream    RealtimeTruePeak.forward at --streams stereo streams with chunks of 256, 1024, 4800 and 48000 samples against the
            route a user could compose: torch.cat with a kept tail, conv1d, abs, amax, maximum.  Expected: not slower.
  parent    with --parent-lib (a library built from the commit before, `make BUILD=... OUT=...`): at_sos_filter,
            at_sos_hop_power and at_loudness_gate of both libraries on the same input, torch.equal and timed.

Nobody measured any of this before: whatever misses is written down as a miss.  Writes a markdown report (--out, default
profiles/true_peak_probe.md) and prints one JSON line per stage."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_probe import alternate, fmt, peak_above, verdict  # noqa: E402
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402
from acids_transforms_amd.utils import filter_design as fd  # noqa: E402

SR = 48000
CHUNKS = (256, 1024, 4800, 48000)


def composed(x, w):
    """The linear true peak of every row of x (rows, L) from torch ops: w is the table (P, 1, K), taps reversed."""
    K = w.shape[-1]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (K - 1, 0))[:, None], w)
    return y.abs().amax(dim=(1, 2))


def offline_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(args.clips * 2, int(SR * args.seconds), device=dev, generator=gen) * 0.1
    rows, L = x.shape
    m, k2 = A.TruePeak(sr=SR).to(dev), A.TruePeak(sr=96000).to(dev)
    w = m.taps.flip(-1)[:, None, :].contiguous()
    co = ops.sos_coefficients(fd.k_weighting(SR))
    legs = {"true_peak": lambda: ops.true_peak(x, m.taps), "composed": lambda: composed(x, w),
            "read_floor": lambda: x.amax(-1), "sos_filter": lambda: ops.sos_filter(x, co),
            "kaiser_2x12": lambda: ops.true_peak(x, k2.taps), "sample_peak": lambda: ops.true_peak(x, m._identity)}
    a, b = ops.true_peak(x, m.taps), composed(x, w)
    out = {"stage": "offline", "rows": rows, "L": L, "plan": ops.true_peak_plan(rows, L, 4, 12), "input_MiB": x.numel() * 4 / 2 ** 20,
           "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev),
           "peak_MiB": {k: peak_above(legs[k]) / 2 ** 20 for k in ("true_peak", "composed")},
           "differ": float((a - b).abs().max() / b.abs().max())}
    out["read_TBps"] = {k: rows * L * 4 / (out["ms"][k]["ms"] * 1e-3) / 1e12 for k in ("true_peak", "read_floor", "sample_peak")}
    out["fma_TFLOPS"] = 2 * 48 * rows * L / (out["ms"]["true_peak"]["ms"] * 1e-3) / 1e12
    print(json.dumps(out), flush=True)
    return out


def long_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(1, args.long_row, device=dev, generator=gen) * 0.1
    m = A.TruePeak(sr=SR).to(dev)
    w = m.taps.flip(-1)[:, None, :].contiguous()
    co = ops.sos_coefficients(fd.k_weighting(SR))
    legs = {"true_peak": lambda: ops.true_peak(x, m.taps), "composed": lambda: composed(x, w), "read_floor": lambda: x.amax(-1),
            "sos_filter": lambda: ops.sos_filter(x, co)}
    out = {"stage": "long", "L": args.long_row, "plan": ops.true_peak_plan(1, args.long_row, 4, 12),
           "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev),
           "equal_to_pieces": bool(torch.equal(ops.true_peak(x, m.taps)[0], torch.maximum(
               ops.true_peak(x[:, :args.long_row // 2].contiguous(), m.taps)[0],
               ops.true_peak_stream(x[:, args.long_row // 2:].contiguous(), m.taps,
                                    x[:, args.long_row // 2 - 11:args.long_row // 2].contiguous(), torch.empty(1, 11, device=dev),
                                    torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), 0)[0])))}
    print(json.dumps(out), flush=True)
    return out


def stream_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(5)
    rows = {}
    for n in CHUNKS:
        x = torch.randn(args.streams, 2, n, device=dev, generator=gen) * 0.1
        rt = A.RealtimeTruePeak(sr=SR).to(dev)
        w = rt.taps.flip(-1)[:, None, :].contiguous()
        K = rt.taps.shape[1]
        state = {"tail": torch.zeros(args.streams, 2, K - 1, device=dev), "max": torch.zeros(args.streams, 2, device=dev)}

        def user(x=x, w=w, K=K, state=state):
            xc = torch.cat([state["tail"], x], -1)
            y = torch.nn.functional.conv1d(xc.reshape(-1, 1, xc.shape[-1]), w)
            peak = y.abs().amax(dim=(1, 2)).reshape(x.shape[:-1])
            state["max"] = torch.maximum(state["max"], peak)
            state["tail"] = xc[..., -(K - 1):]
            return 20.0 * torch.log10(peak)

        legs = {"module": lambda rt=rt, x=x: rt(x), "composed": user}
        a, b = rt(x), user()
        rows[n] = {"ms": alternate(legs, args.stream_calls, args.rounds, args.warmup, ev), "launches": ops.true_peak_plan(args.streams * 2, n, 4, 12)[2],
                   "differ_dB": float((a - b).abs().max())}
    out = {"stage": "stream", "streams": args.streams, "chunks": rows}
    print(json.dumps(out), flush=True)
    return out


def parent_stage(args, dev, ev):
    """The entries this work could disturb, of this build against a library built from the parent commit."""
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ("at_sos_filter", "at_sos_hop_power", "at_loudness_gate"):
        getattr(parent, name).argtypes, getattr(parent, name).restype = _lib._SIGNATURES[name], ctypes.c_int
    parent.at_init.argtypes, parent.at_init.restype = [ctypes.c_int], ctypes.c_int
    assert parent.at_init(0) == 0
    this = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(4)
    clips, L, hop = args.clips, int(SR * args.seconds), 4800
    x = torch.randn(clips * 2, L, device=dev, generator=gen) * 0.1
    rows, nh = clips * 2, L // hop
    co = ops.sos_coefficients(fd.k_weighting(SR))
    power = ops.sos_hop_power(x, co, hop)
    wts = (ctypes.c_double * 2)(1.0, 1.0)

    def filt(lib):
        y = torch.empty_like(x)
        assert lib.at_sos_filter(_lib.ptr(x), rows, L, co.ptr, co.n, 0, None, None, _lib.ptr(y), _lib.stream_ptr()) == 0
        return y

    def hops(lib):
        p = torch.empty(rows, nh, dtype=torch.float64, device=dev)
        assert lib.at_sos_hop_power(_lib.ptr(x), rows, L, co.ptr, co.n, hop, _lib.ptr(p), _lib.stream_ptr()) == 0
        return p

    def gate(lib):
        lufs, stats = torch.empty(clips, device=dev), torch.empty(clips, 3, dtype=torch.float64, device=dev)
        assert lib.at_loudness_gate(_lib.ptr(power), clips, 2, nh, hop, 4, ctypes.cast(wts, ctypes.c_void_p), ops.LOUDNESS_ABS_THRESHOLD,
                                    ops.LOUDNESS_REL_RATIO, _lib.ptr(lufs), _lib.ptr(stats), None, _lib.stream_ptr()) == 0
        return torch.cat([lufs.double()[:, None], stats], -1)

    out = {"stage": "parent", "rows": rows, "L": L, "equal": {}, "ms": {}}
    for name, fn in (("at_sos_filter", filt), ("at_sos_hop_power", hops), ("at_loudness_gate", gate)):
        out["equal"][name] = bool(torch.equal(fn(this), fn(parent)))
        out["ms"][name] = alternate({"this": lambda fn=fn: fn(this), "parent": lambda fn=fn: fn(parent)}, args.calls, args.rounds,
                                    args.warmup, ev)
    print(json.dumps(out), flush=True)
    return out


def report(args, offline, long_row, stream, parent):
    lines = ["# True-peak probe (tools/true_peak_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one" % args.rounds,
             "process.  An expectation is met when the median is no slower than the other leg's beyond the larger of the two",
             "spreads.", ""]
    if offline:
        ms = offline["ms"]
        lines += ["## (a) offline: %d rows x %d samples (input %.0f MiB; tile %d, %d per lane, %d launches)"
                  % (offline["rows"], offline["L"], offline["input_MiB"], offline["plan"][0], offline["plan"][1], offline["plan"][2]), "",
                  "| leg | ms | relative to at_true_peak |", "|---|---|---|"]
        for k, label in (("true_peak", "at_true_peak, (4, 12) compiled copy"), ("composed", "conv1d, abs, amax on the same table"),
                         ("read_floor", "torch amax over the input (reads 4 bytes per sample)"), ("sos_filter", "at_sos_filter, two sections"),
                         ("kaiser_2x12", "at_true_peak, (2, 12) generic copy"), ("sample_peak", "at_true_peak, (1, 1): the sample peak")):
            lines.append("| %s | %s | %.2f |" % (label, fmt(ms[k]), ms[k]["ms"] / ms["true_peak"]["ms"]))
        lines += ["", "at_true_peak against the composed route: %s (%.3f x); the two differ by %.1e normwise.  Peak memory above the"
                  % (verdict(ms["true_peak"], ms["composed"]), ms["true_peak"]["ms"] / ms["composed"]["ms"], offline["differ"]),
                  "input: %.1f MiB against %.1f MiB.  Input read at %.2f TB/s (the torch reduction: %.2f TB/s; the sample peak: %.2f"
                  % (offline["peak_MiB"]["true_peak"], offline["peak_MiB"]["composed"], offline["read_TBps"]["true_peak"],
                     offline["read_TBps"]["read_floor"], offline["read_TBps"]["sample_peak"]),
                  "TB/s), %.1f TFLOP/s of fp32 multiply-adds." % offline["fma_TFLOPS"], ""]
    if long_row:
        ms = long_row["ms"]
        lines += ["## (b) one row of %d samples (%d launches)" % (long_row["L"], long_row["plan"][2]), "",
                  "| at_true_peak ms | composed ms | torch amax ms | at_sos_filter ms (one workgroup per row) | equal to the maximum over two pieces |",
                  "|---|---|---|---|---|",
                  "| %s | %s | %s | %s | %s |" % (fmt(ms["true_peak"]), fmt(ms["composed"]), fmt(ms["read_floor"]), fmt(ms["sos_filter"]),
                                                "yes" if long_row["equal_to_pieces"] else "NO"), "",
                  "Against the composed route: %s." % verdict(ms["true_peak"], ms["composed"]), ""]
    if stream:
        lines += ["## (c) RealtimeTruePeak.forward at %d stereo streams against cat + conv1d + abs + amax + maximum" % stream["streams"], "",
                  "| chunk | launches | module ms | composed ms | module / composed | expectation (not slower) | readings differ by (dB) |",
                  "|---|---|---|---|---|---|---|"]
        for n, r in stream["chunks"].items():
            a, b = r["ms"]["module"], r["ms"]["composed"]
            lines.append("| %s | %d | %s | %s | %.2f | %s | %.1e |" % (n, r["launches"], fmt(a), fmt(b), a["ms"] / b["ms"], verdict(a, b),
                                                                       r["differ_dB"]))
        lines.append("")
    if parent:
        lines += ["## (d) earlier entries against the parent commit's library (%d rows x %d samples)" % (parent["rows"], parent["L"]), "",
                  "| entry | torch.equal | this build ms | parent ms | this / parent | within the spread |", "|---|---|---|---|---|---|"]
        for name, ms in parent["ms"].items():
            lines.append("| %s | %s | %s | %s | %.3f | %s |" % (name, "yes" if parent["equal"][name] else "NO", fmt(ms["this"]),
                                                                fmt(ms["parent"]), ms["this"]["ms"] / ms["parent"]["ms"],
                                                                "yes" if verdict(ms["this"], ms["parent"]) == "met" else "NO"))
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--legs", nargs="+", default=["offline", "long", "stream"], choices=["offline", "long", "stream"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--stream-calls", type=int, default=20)
    ap.add_argument("--long-row", type=int, default=2 ** 24)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "true_peak_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    offline = offline_stage(args, dev, ev) if "offline" in args.legs else None
    long_row = long_stage(args, dev, ev) if "long" in args.legs else None
    stream = stream_stage(args, dev, ev) if "stream" in args.legs else None
    parent = parent_stage(args, dev, ev) if args.parent_lib else None
    report(args, offline, long_row, stream, parent)


if __name__ == "__main__":
    main()

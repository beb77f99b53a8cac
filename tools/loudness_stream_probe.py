"""The streaming R128 meter and loudness range (sos_filter.hip's stream ending, loudness.hip's strided gate and range kernel)
against what they replace, in one process, the legs of a comparison alternated per round (device-synchronised, warmed up, K
calls per timed region; median, min and max over the rounds), with the helpers of tools/resample_probe.py:

  stream    RealtimeLoudness.forward against the route a user could compose before it -- RealtimeSOSFilter(k_weighting),
            torch.cat with the kept remainder, square, per-hop reshape().sum(), cat onto a history, unfold for the blocks --
            at --streams stereo streams at 48 kHz and chunks of 256 / 1024 / 4800 / 48000 samples.  Expected: not slower on any
            leg; the two agree within 1e-4 LU.  By every earlier streaming stage a call costs its launches (two here).
  kernel    at_sos_hop_power_stream on --clips stereo clips x --seconds s in one chunk against at_sos_hop_power on the same
            input.  Expected: inside the spread (the same walk plus one state store).
  range     at_loudness_range on --clips clips x 60 s (571 short-term blocks) against torch.sort + gather on the same block
            powers.  Recorded, no ratio set.
  parent    with --parent-lib (a library built from the commit before): at_sos_filter, at_sos_hop_power,
            at_sos_filter_hop_scaled and at_loudness_gate of both libraries on the same input, compared with torch.equal and
            timed against each other.

Nobody measured any of this before: whatever misses is written down as a miss.  Writes a markdown report (--out, default
profiles/loudness_stream_probe.md) and prints one JSON line per stage."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_probe import alternate, fmt, verdict  # noqa: E402
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402
from acids_transforms_amd.utils import filter_design as fd  # noqa: E402

SR = 48000
HOP = 4800
CHUNKS = (256, 1024, 4800, 48000)


class Composed:
    """The meter from what the package had before: the streaming filter, then torch."""

    def __init__(self, dev):
        self.filter = A.RealtimeSOSFilter(fd.k_weighting(SR), sr=SR).to(dev)
        self.rest = self.history = None

    def __call__(self, x):
        y = self.filter(x)
        if self.rest is not None:
            y = torch.cat([self.rest, y], -1)
        nh = y.shape[-1] // HOP
        self.rest = y[..., nh * HOP:]
        if nh == 0:
            return y.new_empty(x.shape[:-2] + (0,))
        s = (y[..., :nh * HOP].double() ** 2).reshape(x.shape[:-1] + (nh, HOP)).sum(-1)
        before = 0 if self.history is None else self.history.shape[-1]
        self.history = s if self.history is None else torch.cat([self.history, s], -1)
        k = max(0, before + nh - 3) - max(0, before - 3)
        if k == 0:
            return y.new_empty(x.shape[:-2] + (0,))
        window = self.history[..., max(0, before - 3):]
        p = window.unfold(-1, 4, 1).sum(-1).sum(-2) / (4 * HOP)
        return (-0.691 + 10.0 * torch.log10(p)).float()


def stream_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"stage": "stream", "streams": args.streams, "ms": {}, "differ_LU": {}, "blocks": {}}
    for n in CHUNKS:
        x = torch.randn(args.streams, 2, n, device=dev, generator=gen) * 0.1
        meter, composed = A.RealtimeLoudness(SR).to(dev), Composed(dev)
        a = torch.cat([meter(x) for _ in range(-(-8 * HOP // n))], -1)         # the same eight hops through both
        b = torch.cat([composed(x) for _ in range(-(-8 * HOP // n))], -1)
        out["differ_LU"][n], out["blocks"][n] = float((a.double() - b.double()).abs().max()), a.shape[-1]
        legs = {"meter": lambda: meter(x), "composed": lambda: composed(x)}
        out["ms"][n] = alternate(legs, args.stream_calls, args.rounds, args.warmup, ev)
    print(json.dumps(out), flush=True)
    return out


def kernel_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.clips * 2, int(SR * args.seconds), device=dev, generator=gen) * 0.1
    rows, L = x.shape
    co = ops.sos_coefficients(fd.k_weighting(SR))
    zi = torch.zeros(rows, co.n, 2, dtype=torch.float64, device=dev)
    op = torch.zeros(rows, dtype=torch.float64, device=dev)
    hist = torch.zeros(rows, L // HOP, dtype=torch.float64, device=dev)

    def stream():
        zi.zero_()
        op.zero_()
        ops.sos_hop_power_stream(x, co, HOP, 0, zi, op, hist, 0)

    legs = {"stream": stream, "hop_power": lambda: ops.sos_hop_power(x, co, HOP)}
    stream()
    out = {"stage": "kernel", "rows": rows, "L": L, "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev),
           "differ": float(((hist - ops.sos_hop_power(x, co, HOP)).abs().max() / hist.abs().max()))}
    print(json.dumps(out), flush=True)
    return out


def range_stage(args, dev, ev):
    gen = torch.Generator(device=dev).manual_seed(2)
    nh = 600
    power = torch.rand(args.clips, 2, nh, device=dev, generator=gen, dtype=torch.float64) * HOP * 1e-2
    power[:, :, nh // 2:] *= 0.05

    def sort_route():
        p = power.unfold(-1, 30, 1).sum(-1).sum(-2) / (30 * HOP)
        J1 = p > ops.LOUDNESS_ABS_THRESHOLD
        p_abs = (p * J1).sum(-1) / J1.sum(-1)
        J2 = J1 & (p > ops.LOUDNESS_RANGE_REL_RATIO * p_abs[..., None])
        n = J2.sum(-1)
        q = torch.sort(torch.where(J2, p, torch.full_like(p, float("inf"))), -1).values
        lo = q.gather(-1, torch.floor(0.10 * (n - 1) + 0.5).long()[..., None])
        hi = q.gather(-1, torch.floor(0.95 * (n - 1) + 0.5).long()[..., None])
        return (10.0 * torch.log10(hi / lo))[..., 0].float()

    legs = {"select": lambda: ops.loudness_range_from_power(power, nh, SR), "sort": sort_route}
    out = {"stage": "range", "clips": args.clips, "blocks": nh - 29,
           "ms": alternate(legs, args.calls, args.rounds, args.warmup, ev),
           "differ_LU": float((legs["select"]().double() - sort_route().double()).abs().max())}
    print(json.dumps(out), flush=True)
    return out


def parent_stage(args, dev, ev):
    """The four entries that existed before, of this build against a library built from the parent commit."""
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ("at_sos_filter", "at_sos_hop_power", "at_sos_filter_hop_scaled", "at_loudness_gate"):
        getattr(parent, name).argtypes, getattr(parent, name).restype = _lib._SIGNATURES[name], ctypes.c_int
    parent.at_init.argtypes, parent.at_init.restype = [ctypes.c_int], ctypes.c_int
    assert parent.at_init(0) == 0
    this = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn(args.clips * 2, int(SR * args.seconds), device=dev, generator=gen) * 0.1
    x[::4, x.shape[-1] // 2:] *= 0.01
    rows, L = x.shape
    nh = L // HOP
    co = ops.sos_coefficients(fd.k_weighting(SR))
    plan = ops.loudness_plan((2, L), SR)
    w = torch.rand(rows, nh, dtype=torch.float64, device=dev, generator=gen)
    zi = torch.randn(rows, 2, 2, dtype=torch.float64, device=dev, generator=gen) * 1e-3
    power = ops.sos_hop_power(x, co, HOP)
    st = _lib.stream_ptr

    def run(lib, entry):
        if entry == "at_sos_filter":
            y, zf = torch.empty_like(x), torch.empty_like(zi)
            rc = lib.at_sos_filter(_lib.ptr(x), rows, L, co.ptr, co.n, 0, _lib.ptr(zi), _lib.ptr(zf), _lib.ptr(y), st())
            out = (y, zf)
        elif entry == "at_sos_hop_power":
            p = torch.empty(rows, nh, dtype=torch.float64, device=dev)
            rc = lib.at_sos_hop_power(_lib.ptr(x), rows, L, co.ptr, co.n, HOP, _lib.ptr(p), st())
            out = (p,)
        elif entry == "at_sos_filter_hop_scaled":
            u = torch.empty_like(x)
            rc = lib.at_sos_filter_hop_scaled(_lib.ptr(x), rows, L, co.ptr, co.n, HOP, _lib.ptr(w), _lib.ptr(u), st())
            out = (u,)
        else:
            lufs = torch.empty(rows // 2, dtype=torch.float32, device=dev)
            stats = torch.empty(rows // 2, 3, dtype=torch.float64, device=dev)
            blocks = torch.empty(rows // 2, nh - 3, dtype=torch.float32, device=dev)
            rc = lib.at_loudness_gate(_lib.ptr(power), rows // 2, 2, nh, HOP, 4, plan.wptr, ops.LOUDNESS_ABS_THRESHOLD,
                                      ops.LOUDNESS_REL_RATIO, _lib.ptr(lufs), _lib.ptr(stats), _lib.ptr(blocks), st())
            out = (lufs, stats, blocks)
        assert rc == 0
        return out

    equal, timed = {}, {}
    for entry in ("at_sos_filter", "at_sos_hop_power", "at_sos_filter_hop_scaled", "at_loudness_gate"):
        equal[entry] = all(bool(torch.equal(a, b)) for a, b in zip(run(this, entry), run(parent, entry)))
        legs = {"this": lambda e=entry: run(this, e), "parent": lambda e=entry: run(parent, e)}
        timed[entry] = alternate(legs, args.calls, args.rounds, args.warmup, ev)
    out = {"stage": "parent", "rows": rows, "L": L, "equal": equal, "ms": timed}
    print(json.dumps(out), flush=True)
    return out


def report(args, stream, kernel, rng, parent):
    lines = ["# Streaming loudness probe (tools/loudness_stream_probe.py)", "",
             "ms per call as median (min .. max) over %d rounds, device-synchronised, the legs of a row alternated in one"
             % args.rounds, "process.  An expectation is met when the median is no slower than the other leg's beyond the larger "
             "of the two spreads.", ""]
    if stream:
        lines += ["## (a) RealtimeLoudness.forward against the composed route (%d stereo streams at %d Hz)" % (stream["streams"], SR),
                  "", "| chunk | meter ms | composed ms | meter / composed | expectation (not slower) | results differ by (LU) over blocks |",
                  "|---|---|---|---|---|---|"]
        for n in CHUNKS:
            a, b = stream["ms"][n]["meter"], stream["ms"][n]["composed"]
            lines.append("| %d | %s | %s | %.2f | %s | %.1e over %d |" % (n, fmt(a), fmt(b), a["ms"] / b["ms"], verdict(a, b),
                                                                      stream["differ_LU"][n], stream["blocks"][n]))
        lines.append("")
    if kernel:
        a, b = kernel["ms"]["stream"], kernel["ms"]["hop_power"]
        lines += ["## (b) at_sos_hop_power_stream in one chunk against at_sos_hop_power (%d rows x %d samples)"
                  % (kernel["rows"], kernel["L"]), "",
                  "| stream ms (with two small state clears) | hop power ms | stream / hop power | expectation (inside the spread) | hop powers differ by (normwise) |",
                  "|---|---|---|---|---|",
                  "| %s | %s | %.3f | %s | %.1e |" % (fmt(a), fmt(b), a["ms"] / b["ms"], verdict(a, b), kernel["differ"]), ""]
    if rng:
        a, b = rng["ms"]["select"], rng["ms"]["sort"]
        lines += ["## (c) at_loudness_range against torch.sort + gather (%d clips, %d short-term blocks)" % (rng["clips"], rng["blocks"]),
                  "", "| radix select ms | sort route ms | select / sort | results differ by (LU) |", "|---|---|---|---|",
                  "| %s | %s | %.2f | %.1e |" % (fmt(a), fmt(b), a["ms"] / b["ms"], rng["differ_LU"]), ""]
    if parent:
        lines += ["## (d) the entries that existed before, against the parent commit's library (%d rows x %d samples)"
                  % (parent["rows"], parent["L"]), "",
                  "| entry | outputs torch.equal | this build ms | parent ms | this / parent | within the spread |", "|---|---|---|---|---|---|"]
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
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--legs", nargs="+", default=["stream", "kernel", "range"], choices=["stream", "kernel", "range"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--stream-calls", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "loudness_stream_probe.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = stream_stage(args, dev, ev) if "stream" in args.legs else None
    kernel = kernel_stage(args, dev, ev) if "kernel" in args.legs else None
    rng = range_stage(args, dev, ev) if "range" in args.legs else None
    parent = parent_stage(args, dev, ev) if args.parent_lib else None
    report(args, stream, kernel, rng, parent)


if __name__ == "__main__":
    main()

"""The backward passes of the streaming path at the shapes StreamingDGTSession is benchmarked at (256 streams, chunks of
1024 and 4096 samples, n_fft 1024 / hop 256), one process, legs alternated per round.  Each backward is timed next to the
forward kernel of the same shape:

  oadd_fwd / oadd_fwd_bwd      ops.oadd_forward ([history | chunk | pad])   ops.oadd_forward_backward (one gather pass)
  rfft_fwd / rfft_bwd          RealtimeDGT._rt_forward on the frame view    ops.rfft_frames_backward (window, irFFT, edge)
  irfft_fwd / irfft_bwd        ops.irfft_frames(X)                          ops.irfft_frames_backward (window, rFFT, halve)
  polar_fwd / polar_bwd        ops.irfft_frames(mag, phase)                 the same with a phase (rFFT rows in the workspace)
  oinv_fwd / oinv_bwd          ops.oadd_invert                              ops.oadd_invert_backward (one pass)

A call at these shapes lasts microseconds, so a leg is `--inner` calls between two device events and the figure is the
window over the calls: it includes the launch, the ctypes call and the allocation of the result, as a training step
pays them.  `bytes_per_frame` is what the algorithm has to move (computed from the shapes, the window and twiddles
aside); `gb_per_s` is that over the time.  Prints one JSON line (medians over the rounds, microseconds per call)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402


def bytes_per_frame(N, h, n, C):
    """Bytes each backward has to move per frame, by leg (float32 / complex64)."""
    F, keep = N // 2 + 1, (N // h - 1) * h
    out_len = (n - 1) * h + N - keep
    return {"oadd_fwd_bwd": 4 * N + 4 * C / n,                      # the dense frame gradient in, the chunk's out
            "rfft_bwd": 8 * F + 4 * N + 8 * N,                      # G in, frames out, one more pass for the edge term
            "irfft_bwd": 4 * N + 8 * F,                             # frames in, rows out (DC / Nyquist halved in place)
            "polar_bwd": 4 * N + 8 * F + 8 * F + 4 * F + 4 * F,     # rows to the workspace and back, phase in, gmag out
            "oinv_bwd": 4 * out_len / n + 4 * N}


def legs_for(C, S, N, h, dev, g):
    keep, F = (N // h - 1) * h, N // 2 + 1
    dgt = A.RealtimeDGT(n_fft=N, hop_length=h).to(dev)
    w, wd = dgt.window[:N], dgt.inv_window[:N]
    x = torch.randn(S, C, device=dev, generator=g) * 0.1
    hist = torch.randn(S, keep, device=dev, generator=g) * 0.1
    buf, _, n = ops.oadd_forward(x, hist, keep, N, h)
    frames = torch.as_strided(buf, (S, n, N), (buf.stride(0), h, 1))
    X = dgt._rt_forward(frames)
    mag, phase = X.abs(), ops.angle(X)
    gf = torch.randn(S, n, N, device=dev, generator=g)
    G = torch.randn(S, n, F, dtype=torch.complex64, device=dev, generator=g)
    tail = torch.randn(S, keep, device=dev, generator=g)
    gain = torch.ones((), device=dev) * 1.5
    gy = torch.randn(S, (n - 1) * h + N - keep, device=dev, generator=g)
    legs = {"oadd_fwd": lambda: ops.oadd_forward(x, hist, keep, N, h),
            "oadd_fwd_bwd": lambda: ops.oadd_forward_backward(gf, N, h, keep, C),
            "rfft_fwd": lambda: dgt._rt_forward(frames),
            "rfft_bwd": lambda: ops.rfft_frames_backward(G, w, N),
            "irfft_fwd": lambda: ops.irfft_frames(X, wd, N),
            "irfft_bwd": lambda: ops.irfft_frames_backward(gf, wd, N),
            "polar_fwd": lambda: ops.irfft_frames(None, wd, N, mag=mag, phase=phase),
            "polar_bwd": lambda: ops.irfft_frames_backward(gf, wd, N, phase=phase),
            "oinv_fwd": lambda: ops.oadd_invert(gf, tail, N, h, keep, gain),
            "oinv_bwd": lambda: ops.oadd_invert_backward(gy, n, N, h, keep, gain)}
    return legs, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    S, N, h = args.streams, args.n_fft, args.hop
    out = {"streams": S, "n_fft": N, "hop": h, "rounds": args.rounds, "inner": args.inner, "chunks": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for C in args.chunks:
        legs, n = legs_for(C, S, N, h, dev, g)
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                ev[0].record()
                for _ in range(args.inner):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[name].append(1e3 * ev[0].elapsed_time(ev[1]) / args.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        bpf = bytes_per_frame(N, h, n, C)
        pairs = {"oadd_fwd_bwd": "oadd_fwd", "rfft_bwd": "rfft_fwd", "irfft_bwd": "irfft_fwd", "polar_bwd": "polar_fwd",
                 "oinv_bwd": "oinv_fwd"}
        out["chunks"][str(C)] = {
            "frames": S * n, "us": med, "min_us": {k: min(v) for k, v in times.items()},
            "bwd_over_fwd": {b: med[b] / med[f] for b, f in pairs.items()},
            "bytes_per_frame": bpf,
            "gb_per_s": {b: bpf[b] * S * n / (med[b] * 1e-6) / 1e9 for b in pairs}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

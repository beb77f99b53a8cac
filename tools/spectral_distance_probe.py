"""SpectralDistance at the bench size (1024 clips x 4 s, the default five scales, x requiring grad), one process, the two
routes alternated per round:

  fused     losses.SpectralDistance (audio-only graph, chunked backward)
  composed  the same loss from STFT(n, n // 4) + Magnitude(mel=False, mode=None, contrast=None) per scale on both signals
            plus torch expressions -- code the fused route does not touch

For each: forward time (no graph), forward + backward time, and the rise of torch.cuda.max_memory_allocated over the
level before the call (inputs excluded).  Then the two new kernels alone on one chunk at n_fft 1024: time, bytes per
bin over time, share of the 8 TB/s HBM peak.  The one assertion is the derived bound: the fused route's peak above the
inputs is the gradient + two chunk spectra + one (chunk, L) scratch + the STFT adjoint's own workspace for a chunk,
and what lies above the gradient does not grow with B.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402
from acids_transforms_amd.autograd import _specdist_chunks  # noqa: E402

MiB = float(1 << 20)
SLACK = 16 << 20        # the sums, the per-clip vectors, the allocator's rounding


def composed_loss(scales, dev, eps):
    stages = [(A.STFT(n_fft=n, hop_length=h).to(dev), A.Magnitude(mel=False, mode=None, contrast=None, n_fft=n).to(dev))
              for n, h in scales]

    def loss(x, y):
        total = 0
        for stft, mag in stages:
            a, b = mag(stft(x)), mag(stft(y))
            lin = ((a - b) ** 2).sum((1, 2)) / (b ** 2).sum((1, 2))
            log = (torch.log(a + eps) - torch.log(b + eps)).abs().mean((1, 2))
            total = total + lin + log
        return total.mean()
    return loss


def fused_bound(B, L, scales):
    """(gradient bytes, bytes above it) of the fused backward, derived from the shapes."""
    lib = _lib.lib()
    above, rows = 0, 0
    for s, (n, hop) in enumerate(scales):
        b0, b1 = _specdist_chunks(B, L, n, hop)[0]
        T, F = 1 + L // hop, n // 2 + 1
        above = max(above, 2 * 8 * (b1 - b0) * T * F + lib.at_stft_backward_workspace_bytes(b1 - b0, T, n, hop))
        rows = max(rows, b1 - b0) if s else rows
    return 4 * B * L, above + 4 * rows * L


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def timed(fn, ev):
    torch.cuda.synchronize()
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=176400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-launches", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L = args.clips, args.samples
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    y = torch.randn(B, L, device=dev, generator=gen) * 0.1
    crit = A.SpectralDistance().to(dev)
    composed = composed_loss(crit.scales, dev, crit.eps)

    def fwd_bwd(loss):
        def run():
            xr = x.detach().requires_grad_()
            loss(xr, y).backward()
        return run

    legs = {"fused_fwd": lambda: crit(x, y), "fused_fwd+bwd": fwd_bwd(crit),
            "composed_fwd": lambda: composed(x, y), "composed_fwd+bwd": fwd_bwd(composed)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            ms = timed(fn, ev)
            if r >= args.warmup:
                times[name].append(ms)
    values = {"fused": float(crit(x, y)), "composed": float(composed(x, y))}
    peaks = {k: peak_of(fn) for k, fn in legs.items()}

    # the derived bound, and its independence of B
    grad_bytes, above = fused_bound(B, L, crit.scales)
    assert peaks["fused_fwd+bwd"] <= grad_bytes + above + SLACK, (peaks["fused_fwd+bwd"], grad_bytes, above)
    assert peaks["fused_fwd"] <= 2 * 8 * (1 << 26) + SLACK, peaks["fused_fwd"]
    half = B // 2
    xh, yh = x[:half].contiguous(), y[:half].contiguous()

    def half_run():
        xr = xh.detach().requires_grad_()
        crit(xr, yh).backward()
    half_peak = peak_of(half_run)
    half_grad, half_above = fused_bound(half, L, crit.scales)
    assert half_peak <= half_grad + half_above + SLACK, (half_peak, half_grad, half_above)
    del xh, yh

    # the two kernels alone, one chunk at n_fft 1024 / hop 256
    n, hop = 1024, 256
    b0, b1 = _specdist_chunks(B, L, n, hop)[0]
    w = crit._windows()[crit.scales.index((n, hop))]
    X = ops.stft_forward(x[b0:b1], w, n, hop, center=True)
    Y = ops.stft_forward(y[b0:b1], w, n, hop, center=True)
    nbins = X.numel()
    sums = ops.spectral_distance_sums(X, Y, crit.eps)
    g = torch.full((b1 - b0,), 1.0 / B, device=dev)
    N = args.kernel_launches
    kern = {"sums": (lambda: ops.spectral_distance_sums(X, Y, crit.eps), 16),
            # in place: the values change from launch to launch, the traffic does not
            "backward_x": (lambda: ops.spectral_distance_backward(X, Y, sums, g, 1.0, 1.0, crit.eps, True, False), 24),
            "backward_xy": (lambda: ops.spectral_distance_backward(X, Y, sums, g, 1.0, 1.0, crit.eps, True, True), 32)}
    kernels = {}
    for name, (fn, bytes_per_bin) in kern.items():
        fn()
        runs = [timed(lambda: [fn() for _ in range(N)], ev) / N for _ in range(args.rounds)]
        ms = statistics.median(runs)
        rate = nbins * bytes_per_bin / (ms * 1e-3)
        kernels[name] = {"ms": ms, "min_ms": min(runs), "max_ms": max(runs), "bytes_per_bin": bytes_per_bin,
                         "TBps": rate / 1e12, "share_of_8TBps": rate / 8e12}

    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "clips": B, "samples": L, "scales": crit.scales, "rounds": args.rounds, "loss": values,
        "ms": med, "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
        "fused_over_composed_fwd": med["fused_fwd"] / med["composed_fwd"],
        "fused_over_composed_fwd_bwd": med["fused_fwd+bwd"] / med["composed_fwd+bwd"],
        "peak_MiB": {k: v / MiB for k, v in peaks.items()},
        "fused_bound_MiB": {"gradient": grad_bytes / MiB, "above_gradient": above / MiB},
        "fused_above_gradient_MiB": {str(B): (peaks["fused_fwd+bwd"] - grad_bytes) / MiB,
                                     str(half): (half_peak - half_grad) / MiB},
        "kernel_chunk_clips": b1 - b0, "kernel_bins": nbins, "kernels": kernels}))


if __name__ == "__main__":
    main()

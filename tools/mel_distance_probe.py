"""MelSpectralDistance at the bench size (1024 clips x 4 s, the default five scales, x requiring grad), one process, the
three routes alternated per round:

  mel       losses.MelSpectralDistance (audio-only graph, chunked backward, one spectrum alive at a time)
  composed  the same loss from STFT(n, hop) + Magnitude(mel=True, n_mels, mode=None, contrast=None) per scale on both
            signals (the module's bank copied into the Magnitude) plus torch expressions
  stft      losses.SpectralDistance at the same (n_fft, hop): another loss, the neighbouring route

For each: forward time (no graph), forward + backward time, and the rise of torch.cuda.max_memory_allocated over the
level before the call (inputs excluded); for the mel route also what it holds above the gradient at B and at B / 2.
Then the kernels alone on one chunk at (1024, 256, 160), each against its neighbour on the same spectrum and bank,
alternated inside every round: at_mel_distance_backward against at_magnitude_backward (no contrast), at_mel_rows against
at_mel_project_banded (no contrast), and at_mel_distance_sums.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import _lib, ops  # noqa: E402
from acids_transforms_amd.autograd import _meldist_tables, _specdist_chunks  # noqa: E402
from acids_transforms_amd.utils.banded import BandedBank  # noqa: E402

MiB = float(1 << 20)


def composed_loss(crit, dev):
    stages = []
    for i, (n, h, m) in enumerate(crit.scales):
        mag = A.Magnitude(mel=True, mode=None, contrast=None, n_fft=n, n_mels=m, sr=crit.sr).to(dev)
        with torch.no_grad():
            mag.mel_bank.copy_(getattr(crit, "mel_bank_%d" % i).unsqueeze(0))      # the loss's bank, not a normalised one
        stages.append((A.STFT(n_fft=n, hop_length=h).to(dev), mag))
    eps = crit.eps

    def loss(x, y):
        total = 0
        for stft, mag in stages:
            a, b = mag(stft(x)), mag(stft(y))
            lin = ((a - b) ** 2).sum((1, 2)) / (b ** 2).sum((1, 2))
            log = (torch.log(a + eps) - torch.log(b + eps)).abs().mean((1, 2))
            total = total + lin + log
        return total.mean()
    return loss


def mel_bound(B, L, scales):
    """(gradient bytes, bytes above it) the x-only backward of the mel route may hold, derived from the shapes: one
    chunk spectrum, the other signal's mel rows of the chunk, one (chunk, L) scratch, the STFT adjoint's workspace."""
    lib = _lib.lib()
    above, rows = 0, 0
    for s, (n, hop, m) in enumerate(scales):
        b0, b1 = _specdist_chunks(B, L, n, hop)[0]
        T, F = 1 + L // hop, n // 2 + 1
        above = max(above, (8 * F + 4 * m) * (b1 - b0) * T + lib.at_stft_backward_workspace_bytes(b1 - b0, T, n, hop))
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


def spread(v):
    return {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


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
    crit = A.MelSpectralDistance().to(dev)
    composed = composed_loss(crit, dev)
    stft_crit = A.SpectralDistance(scales=tuple((n, h) for n, h, _ in crit.scales)).to(dev)

    def fwd_bwd(loss):
        def run():
            xr = x.detach().requires_grad_()
            loss(xr, y).backward()
        return run

    legs = {"mel_fwd": lambda: crit(x, y), "mel_fwd+bwd": fwd_bwd(crit),
            "composed_fwd": lambda: composed(x, y), "composed_fwd+bwd": fwd_bwd(composed),
            "stft_fwd": lambda: stft_crit(x, y), "stft_fwd+bwd": fwd_bwd(stft_crit)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            ms = timed(fn, ev)
            if r >= args.warmup:
                times[name].append(ms)
    values = {"mel": float(crit(x, y)), "composed": float(composed(x, y)), "stft": float(stft_crit(x, y))}
    peaks = {k: peak_of(fn) for k, fn in legs.items()}
    grad_bytes, above = mel_bound(B, L, crit.scales)
    half = B // 2
    xh, yh = x[:half].contiguous(), y[:half].contiguous()

    def half_run():
        xr = xh.detach().requires_grad_()
        crit(xr, yh).backward()
    half_peak = peak_of(half_run)
    half_grad, half_above = mel_bound(half, L, crit.scales)
    del xh, yh

    # the kernels alone, one chunk at (1024, 256, 160), each next to its neighbour on the same spectrum and bank
    n, hop, m = 1024, 256, 160
    s = crit.scales.index((n, hop, m))
    b0, b1 = _specdist_chunks(B, L, n, hop)[0]
    w = crit._windows()[s]
    cols, cols_t = _meldist_tables(crit, dev)[s]
    bank = getattr(crit, "mel_bank_%d" % s)
    band = BandedBank(bank)
    assert band.eligible
    X = ops.stft_forward(x[b0:b1], w, n, hop, center=True)
    Y = ops.stft_forward(y[b0:b1], w, n, hop, center=True)
    nbins, K = X.numel(), X.shape[-1]
    M, Q = ops.mel_rows(X, cols), ops.mel_rows(Y, cols)
    del Y
    sums = ops.mel_distance_sums(M, Q, crit.eps)
    g = torch.full((b1 - b0,), 1.0 / B, device=dev)
    dF = torch.randn(M.shape, device=dev, generator=gen)
    S = X.clone()
    rows_out, proj_out = torch.empty_like(M), torch.empty_like(M)
    N = args.kernel_launches
    # bytes per bin the algorithm must move: spectrum in (8) and out (8), rows of N floats per K bins in or out
    per_row = 4.0 * m / K
    kern = {
        # in place: the values change from launch to launch, the traffic does not
        "mel_distance_backward": (lambda: ops.mel_distance_backward(S, Q, sums, g, cols, cols_t, 1.0, 1.0, crit.eps, 0),
                                  16 + per_row),
        "magnitude_backward": (lambda: ops.magnitude_backward(X, dF, cols, cols_t, None, None, crit.eps), 16 + per_row),
        "mel_rows": (lambda: ops.mel_rows(X, cols, out=rows_out), 8 + per_row),
        "mel_project_banded": (lambda: ops.mel_forward(X, bank, contrast=None, band=band, out=proj_out), 8 + per_row),
        "mel_distance_sums": (lambda: ops.mel_distance_sums(M, Q, crit.eps, out=sums), 2 * per_row),
    }
    ktimes = {k: [] for k in kern}
    for r in range(args.warmup + args.rounds):
        for name, (fn, _) in kern.items():
            ms = timed(lambda: [fn() for _ in range(N)], ev) / N
            if r >= args.warmup:
                ktimes[name].append(ms)
    kernels = {}
    for name, (_, bytes_per_bin) in kern.items():
        k = spread(ktimes[name])
        rate = nbins * bytes_per_bin / (k["ms"] * 1e-3)
        kernels[name] = dict(k, bytes_per_bin=bytes_per_bin, TBps=rate / 1e12)

    def ratio(a, b):
        """median of the per-round ratios a / b, with their range: both were timed inside every round"""
        r = [p / q for p, q in zip(ktimes[a], ktimes[b])]
        return {"median": statistics.median(r), "min": min(r), "max": max(r)}

    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "clips": B, "samples": L, "scales": crit.scales, "rounds": args.rounds, "loss": values,
        "ms": med, "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
        "mel_over_composed_fwd": med["mel_fwd"] / med["composed_fwd"],
        "mel_over_composed_fwd_bwd": med["mel_fwd+bwd"] / med["composed_fwd+bwd"],
        "mel_over_stft_fwd": med["mel_fwd"] / med["stft_fwd"],
        "mel_over_stft_fwd_bwd": med["mel_fwd+bwd"] / med["stft_fwd+bwd"],
        "peak_MiB": {k: v / MiB for k, v in peaks.items()},
        "mel_bound_MiB": {"gradient": grad_bytes / MiB, "above_gradient": above / MiB},
        "mel_above_gradient_MiB": {str(B): (peaks["mel_fwd+bwd"] - grad_bytes) / MiB,
                                   str(half): (half_peak - half_grad) / MiB, "bound_%d" % half: half_above / MiB},
        "kernel_chunk_clips": b1 - b0, "kernel_bins": nbins, "kernel_launches": N, "kernels": kernels,
        "backward_over_magnitude_backward": ratio("mel_distance_backward", "magnitude_backward"),
        "mel_rows_over_mel_project_banded": ratio("mel_rows", "mel_project_banded")}))


if __name__ == "__main__":
    main()

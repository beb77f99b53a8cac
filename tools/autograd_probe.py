"""Backward passes at the bench size (1024 clips x 4 s, n_fft 1024 / hop 256), one process, legs alternated per round:

  adjoint   ops.stft_backward (the STFT's gradient)      against  istft  (the ISTFT: same bytes, 4104 B in / 1024 B out
                                                                          per frame)
  magbwd    the Magnitude(n_mels=128) backward alone     as a share of 8 TB/s on X in + dF in + dX out (8720 B per frame)
  fwd       the fused STFT -> Magnitude forward          against  fwd+bwd (the same with requires_grad, plus backward)
  istft_adj ops.istft_backward (invert's gradient)       against  stft_fwd (the plain ops.stft_forward: the same bytes,
            istft_adj_polar (the magnitude's gradient)            1024 B in / 4104 B out per frame)
  mfcc_fwd  MFCC() on the audio (the fused kernel)       against  mfcc_fwd+bwd (the same with requires_grad, plus the
                                                                  chunked backward: STFT, at_mfcc_backward, STFT adjoint)
  mfcc_bwd_kernel / mfcc_bwd_kernel_dct  at_mfcc_backward alone, in place on one 189-clip chunk, for MFCC() and
            MFCC(n_mfcc=40): X in + dF in + dX out, 8720 B per frame without the DCT (as magbwd), 8368 B with it

Prints one JSON line (medians over the rounds, ms).  Run under `rocprofv3 --kernel-trace --stats -- python ...` for the
per-kernel split."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402
from acids_transforms_amd.autograd import _magnitude_grad, _mfcc_tables, mfcc_chunk_clips  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=176400)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L = args.clips, args.samples
    g = torch.Generator(device=dev).manual_seed(0)
    stft = A.STFT().to(dev)
    mag = A.Magnitude(n_mels=128).to(dev)
    x = torch.randn(B, L, device=dev, generator=g) * 0.1
    X = stft(x)
    mag.scale_data(X)
    T = X.shape[1]
    G = torch.randn(X.shape, dtype=torch.complex64, device=dev, generator=g)
    dF = torch.randn(B, T, 128, device=dev, generator=g)
    window = stft.window[:1024]

    def fwd_bwd():
        xr = x.detach().requires_grad_()
        mag.forward_fused(stft, xr).backward(dF)

    inv_window, env = stft.inv_window[:1024], stft._env16
    gy = torch.randn(B, 256 * (T - 1), device=dev, generator=g)
    phase = torch.rand(X.shape, device=dev, generator=g) * 6.283

    mfcc, mfcc40 = A.MFCC().to(dev), A.MFCC(n_mfcc=40).to(dev)
    dFm = torch.randn(B, 128, T, device=dev, generator=g)
    nb = mfcc_chunk_clips(B, T, 1024)
    Xc = X[:nb].clone()                 # overwritten in place by each call: the kernel's time does not depend on the values
    dFc, dFc40 = dFm[:nb].contiguous(), dFm[:nb, :40].contiguous()
    _, inv_t, _ = _mfcc_tables(mfcc, dev)
    fwd40, inv40, dct_t = _mfcc_tables(mfcc40, dev)

    def mfcc_fwd_bwd():
        xr = x.detach().requires_grad_()
        mfcc(xr).backward(dFm)

    legs = {
        "adjoint": lambda: ops.stft_backward(G, window, 1024, 256, L),
        "istft": lambda: stft.invert(X),
        "magbwd": lambda: _magnitude_grad(mag, X, dF),
        "fwd": lambda: mag.forward_fused(stft, x),
        "fwd+bwd": fwd_bwd,
        "stft_fwd": lambda: ops.stft_forward(x, window, 1024, 256),
        "istft_adj": lambda: ops.istft_backward(gy, inv_window, 1024, 256, T, env16=env),
        "istft_adj_polar": lambda: ops.istft_backward(gy, inv_window, 1024, 256, T, env16=env, phase=phase),
        "mfcc_fwd": lambda: mfcc(x),
        "mfcc_fwd+bwd": mfcc_fwd_bwd,
        "mfcc_bwd_kernel": lambda: ops.mfcc_backward(Xc, dFc, inv_t, 2, inplace=True),
        "mfcc_bwd_kernel_dct": lambda: ops.mfcc_backward(Xc, dFc40, inv40, 2, fwd40, dct_t, inplace=True),
    }
    times = {k: [] for k in legs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(ev[0].elapsed_time(ev[1]))
    med = {k: statistics.median(v) for k, v in times.items()}
    frames = B * T
    out = {
        "clips": B, "samples": L, "frames": frames, "rounds": args.rounds, "ms": med,
        "adjoint_over_istft": med["adjoint"] / med["istft"],
        "magbwd_TBps": frames * 8720 / (med["magbwd"] * 1e-3) / 1e12,
        "magbwd_share_of_8TBps": frames * 8720 / (med["magbwd"] * 1e-3) / 8e12,
        "fwd_bwd_over_fwd": med["fwd+bwd"] / med["fwd"],
        "istft_adj_over_stft_fwd": med["istft_adj"] / med["stft_fwd"],
        "istft_adj_polar_over_stft_fwd": med["istft_adj_polar"] / med["stft_fwd"],
        "mfcc_fwd_bwd_over_fwd": med["mfcc_fwd+bwd"] / med["mfcc_fwd"],
        "mfcc_chunk_clips": nb,
        "mfcc_bwd_kernel_TBps": nb * T * 8720 / (med["mfcc_bwd_kernel"] * 1e-3) / 1e12,
        "mfcc_bwd_kernel_dct_TBps": nb * T * 8368 / (med["mfcc_bwd_kernel_dct"] * 1e-3) / 1e12,
        # the same bytes per frame as magbwd: per-frame time of the two, same process
        "mfcc_bwd_kernel_ns_per_frame": med["mfcc_bwd_kernel"] * 1e6 / (nb * T),
        "magbwd_ns_per_frame": med["magbwd"] * 1e6 / frames,
        "min_ms": {k: min(v) for k, v in times.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()

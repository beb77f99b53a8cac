"""PQMF at the bench size (1024 clips x 176 400 samples, n_band 16, taps 513), one process, the two routes alternated per
round:

  pqmf      transforms.PQMF: the two kernels of csrc/pqmf.hip (fold + modulation), a graph that keeps no tensor
  composed  the same bank as a dense (n_band, 1, taps) kernel: torch.nn.functional.conv1d(stride=n_band, padding=P) and
            n_band x conv_transpose1d(stride=n_band, padding=P, output_padding=n_band - 1), torch autograd

For each: the analysis and the synthesis alone (no graph), forward + backward of invert(forward(x)) with x requiring
grad, and the rise of torch.cuda.max_memory_allocated over the level before the call (inputs excluded).  The two
kernels are also given as a share of 8 TB/s on the 8 bytes per sample they must move, and as an FMA rate on the
taps / n_band + 2 n_band multiply-adds per sample they spend.  Prints one JSON line per stage (kernels first, so that a
composed route that runs out of memory or time does not take the kernels' figures with it)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402

MiB = float(1 << 20)
HBM_BYTES_PER_S = 8e12


def dense_bank(pq):
    """h_k (n_band, 1, taps) float32 from the module's own buffers, as conv1d takes it: the modulation's phase advances
    by an odd multiple of pi every 2 n_band taps, so h_k[n] = h[n] C[k, n mod 2M] (-1)^(n div 2M)."""
    M, N = pq.n_band, pq.taps
    n = torch.arange(N, device=pq.prototype.device)
    mod = pq.modulation.double()[:, (n % (2 * M))] * (1.0 - 2.0 * ((n // (2 * M)) % 2)).double()
    return (pq.prototype.double() * mod).float().unsqueeze(1).contiguous()


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
    ap.add_argument("--n-band", type=int, default=16)
    ap.add_argument("--taps", type=int, default=513)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-launches", type=int, default=10)
    ap.add_argument("--skip-composed", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, M, N = args.clips, args.samples, args.n_band, args.taps
    assert L % M == 0
    P = (N - 1) // 2
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, L, device=dev, generator=gen) * 0.1
    pq = A.PQMF(n_band=M, taps=N).to(dev)
    proto, mod = pq.prototype, pq.modulation
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    samples = B * L

    # the two kernels alone, output buffers included in the timed region's allocator traffic only once (warm cache)
    y = pq(x)
    K = args.kernel_launches
    kern = {"analysis": lambda: ops.pqmf_analysis(x, proto, mod, 1.0),
            "synthesis": lambda: ops.pqmf_synthesis(y, proto, mod, float(M))}
    ktimes = {k: [] for k in kern}
    for r in range(args.warmup + args.rounds):
        for name, fn in kern.items():
            ms = timed(lambda: [fn() for _ in range(K)], ev) / K
            if r >= args.warmup:
                ktimes[name].append(ms)
    fma_per_sample = N / M + 2 * M
    kernels = {}
    for name in kern:
        k = spread(ktimes[name])
        sec = k["ms"] * 1e-3
        kernels[name] = dict(k, TBps=samples * 8 / sec / 1e12, share_of_8TBps=samples * 8 / sec / HBM_BYTES_PER_S,
                             TFMAps=samples * fma_per_sample / sec / 1e12)
    print(json.dumps({"stage": "kernels", "clips": B, "samples": L, "n_band": M, "taps": N,
                      "tile_blocks": ops.pqmf_tile_blocks(M, N), "byte_floor_ms": samples * 8 / HBM_BYTES_PER_S * 1e3,
                      "fma_per_sample": fma_per_sample, "kernel_launches": K, "kernels": kernels}), flush=True)

    def pq_round_trip():
        xr = x.detach().requires_grad_()
        pq.invert(pq(xr)).sum().backward()

    legs = {"pqmf_forward": lambda: pq(x), "pqmf_invert": lambda: pq.invert(y), "pqmf_fwd+bwd": pq_round_trip}
    if not args.skip_composed:
        hk = dense_bank(pq)

        def c_forward(v):
            return F.conv1d(v.unsqueeze(1), hk, stride=M, padding=P)

        def c_invert(v):
            return M * F.conv_transpose1d(v, hk, stride=M, padding=P, output_padding=M - 1).squeeze(1)

        def c_round_trip():
            xr = x.detach().requires_grad_()
            c_invert(c_forward(xr)).sum().backward()

        small = x[:2, :M * 400]
        parity = {"forward": float((c_forward(small) - pq(small)).abs().max() / pq(small).abs().max()),
                  "invert": float((c_invert(pq(small)) - pq.invert(pq(small))).abs().max() / pq.invert(pq(small)).abs().max())}
        legs.update({"composed_forward": lambda: c_forward(x), "composed_invert": lambda: c_invert(y),
                     "composed_fwd+bwd": c_round_trip})
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            ms = timed(fn, ev)
            if r >= args.warmup:
                times[name].append(ms)
    peaks = {k: peak_of(fn) for k, fn in legs.items()}
    out = {"stage": "routes", "rounds": args.rounds, "ms": {k: spread(v) for k, v in times.items()},
           "peak_MiB": {k: v / MiB for k, v in peaks.items()}, "input_MiB": 4 * samples / MiB}
    if not args.skip_composed:
        med = {k: statistics.median(v) for k, v in times.items()}
        out["composed_vs_pqmf_rel_max"] = parity
        out["pqmf_over_composed"] = {k: med["pqmf_" + k] / med["composed_" + k] for k in ("forward", "invert", "fwd+bwd")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

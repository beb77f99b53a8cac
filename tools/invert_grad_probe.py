"""The invert backward passes at the bench size (1024 clips x 4 s: 690 frames x 513 bins per clip), one process, legs
alternated per round.  Each new backward is timed next to the forward kernel it is the adjoint of:

  mag513_fwd / mag513_bwd    Magnitude().invert (513 features)        ops.magnitude_invert_backward, real form
  mag128_fwd / mag128_bwd    Magnitude(n_mels=128).invert             the same, 128 features in, 513 out
  polar_fwd / polar_bwd      Polar().invert in one pass               the polar form (both halves of the stacked gradient)
  cart_fwd / cart_bwd        Cartesian().invert in one pass           ops.cartesian_inverse_backward
  chain_fwd / chain_fwd+bwd  (STFT() + Polar()).invert                the same with requires_grad, plus backward
  step                       the bench's step for context: the fused STFT -> Magnitude(n_mels=128) forward, then the ISTFT

By bytes moved a backward should cost about 1.5 x its forward (the Magnitude form reads g and y and writes dy where the
forward reads one and writes one; the polar form moves 24 F bytes per row against 16 F).  Prints one JSON line (medians
over the rounds, ms)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import acids_transforms_amd as A  # noqa: E402
from acids_transforms_amd import ops  # noqa: E402
from acids_transforms_amd.autograd import _inverse_bank_tables  # noqa: E402


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
    x = torch.randn(B, L, device=dev, generator=g) * 0.1
    X = stft(x)
    T, F = X.shape[1], X.shape[2]

    mags = {"mag513": A.Magnitude().to(dev), "mag128": A.Magnitude(n_mels=128).to(dev)}
    legs = {}
    for name, mod in mags.items():
        mod.scale_data(X)
        y = mod(X)
        gout = torch.randn(B, T, F, device=dev, generator=g)
        off, sc = mod._affine()
        tables = _inverse_bank_tables(mod, dev)
        legs[name + "_fwd"] = lambda mod=mod, y=y: mod.invert(y)
        legs[name + "_bwd"] = lambda mod=mod, y=y, gout=gout, off=off, sc=sc, tables=tables: \
            ops.magnitude_invert_backward(y, gout, tables, mod.contrast_mode, off, sc, mod._eps)

    polar = A.Polar().to(dev)
    polar.scale_data(X)
    yp = polar(X)
    gX = torch.randn(B, T, F, dtype=torch.complex64, device=dev, generator=g)
    pm = polar.magnitude
    m_off, m_sc = pm._affine()
    p_off, p_sc = polar.phase._affine(yp)
    t_cols, f_cols = _inverse_bank_tables(pm, dev), _inverse_bank_tables(pm, dev, forward=True)
    legs["polar_fwd"] = lambda: polar.invert(yp)
    legs["polar_bwd"] = lambda: ops.magnitude_invert_backward(yp, gX, t_cols, pm.contrast_mode, m_off, m_sc, pm._eps,
                                                             bank_cols=f_cols, phase_offset=p_off, phase_scale=p_sc)

    cart = A.Cartesian().to(dev)
    cart.scale_data(X)
    yc = cart(X)
    re_sc, im_sc = cart.magnitude._affine(yc)[1], cart.phase._affine(yc)[1]
    legs["cart_fwd"] = lambda: cart.invert(yc)
    legs["cart_bwd"] = lambda: ops.cartesian_inverse_backward(gX, re_sc, im_sc)

    chain = (stft + polar)
    gy = torch.randn(B, 256 * (T - 1), device=dev, generator=g)

    def chain_fwd_bwd():
        yr = yp.detach().requires_grad_()
        chain.invert(yr).backward(gy)

    legs["chain_fwd"] = lambda: chain.invert(yp)
    legs["chain_fwd+bwd"] = chain_fwd_bwd

    def step():
        Xs, _ = mags["mag128"].forward_fused(stft, x, return_spectrum=True)
        stft.invert(Xs)

    legs["step"] = step

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
    out = {"clips": B, "samples": L, "frames": B * T, "bins": F, "rounds": args.rounds, "ms": med,
           "bwd_over_fwd": {k: med[k + "_bwd"] / med[k + "_fwd"] for k in ("mag513", "mag128", "polar", "cart")},
           "chain_fwd_bwd_over_fwd": med["chain_fwd+bwd"] / med["chain_fwd"],
           "min_ms": {k: min(v) for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

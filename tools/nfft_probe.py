"""Dev timing: STFT forward / inverse at other FFT sizes (1024 clips x 4 s, hop = n_fft / 4).

    python tools/nfft_probe.py [sizes] [--libs name=path,...] [--rounds R] [--extras]

--libs loads further builds of libacids_hip.so next to the in-tree one (as tools/step_probe.py `ab` does) and times
every entry under each of them in turn, R rounds, inside this one process: numbers from different processes or boxes
are not comparable (NOTES).  Give the same build twice under two file names for the A/A spread.  --extras adds, at
n_fft 512, the forward with phase output and the features-only MelSpectrogram (hop 128, 64 mels).  Only the symbols a
library exports are bound, so an older build of the same ABI version loads too.

    python tools/nfft_probe.py 512,2048,4096 --equal --libs parent=tools/ab/libacids_parent.so

--equal times nothing: it runs every entry the n_fft 512 / 2048 / 4096 kernels serve (equal_entries) under the in-tree
library and under each of --libs on the same seeded inputs, 3 short clips and the 1024 x 176400 batch, and exits
non-zero unless every output is bit-identical (torch.equal) -- the check of a refactor of those kernels.  At n_fft 1024
the entries are the two forwards that write the spectrum as an aligned stream (csrc/row_stream.h): the plain forward
and the fused 128-mel forward with the spectrum stored."""
import argparse
import ctypes
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import acids_transforms_amd as A
from acids_transforms_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="?", default="512,1024,2048,4096")
ap.add_argument("--libs", default="")
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--extras", action="store_true")
ap.add_argument("--equal", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, L_ = 1024, 176400
x = torch.randn(B, L_, device=dev) * 0.1


def timeit(fn, n=int(os.environ.get("PERF_N", "5")), warm=int(os.environ.get("PERF_WARM", "2"))):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


handles = {"tree": L.lib()}
for kv in filter(None, args.libs.split(",")):
    name, path = kv.split("=")
    h = ctypes.CDLL(os.path.abspath(path))
    for fn, argtypes in L._SIGNATURES.items():
        f = getattr(h, fn, None)
        if f is not None:
            f.argtypes = argtypes
            f.restype = L._RESTYPES.get(fn, L.c_int)
    assert h.at_abi_version() == L.ABI_VERSION, path
    L.check(h.at_init(torch.cuda.current_device()), "at_init " + name)
    handles[name] = h

def equal_entries(n, xs):
    """Every entry the n_fft = 512 / 2048 / 4096 kernels serve, as (name, thunk) on the clips xs (B, L), L a multiple of 4
    and not of the hop: plain forward (odd clip stride; center both ways; with phase), hop-n/4 sliding forward,
    irfft_frames and istft (complex and polar; hops n/8, n/4, n/2; T <= R, T = R + 2 and the full clip), features-only
    forward (512 / 2048: one- and two-pass banks, with and without room for the window in LDS, both layouts)."""
    from acids_transforms_amd import ops
    from acids_transforms_amd.utils.banded import BandedBank
    from oracle import oracle as O
    B, Lx = xs.shape
    w = torch.hann_window(n, device=dev)
    if n == 1024:
        band = BandedBank(A.Magnitude(n_mels=128).mel_bank.reshape(513, -1))
        return [("forward run", lambda: ops.stft_forward(xs, w, n, n // 4)),
                ("fused mel 128 + spectrum", lambda: ops.stft_mel_forward(xs, w, band, "log1p", power=1, want_spectrum=True))]
    odd = xs[:, :Lx - 1].contiguous()
    out = [("forward run", lambda: ops.stft_forward(xs, w, n, n // 4))]
    for hop in (n // 4, 100):
        out.append(("forward plain hop %d" % hop, lambda hop=hop: ops.stft_forward(odd, w, n, hop)))
        out.append(("forward plain hop %d +phase" % hop, lambda hop=hop: ops.stft_forward(odd, w, n, hop, want_phase=True)))
        out.append(("forward plain hop %d center=False" % hop, lambda hop=hop: ops.stft_forward(
            odd, w, n, hop, center=False, T=1 + (Lx - 1 - n) // hop, clip_stride=Lx - 1, L=Lx - 1, B=B)))
    X = ops.stft_forward(xs, w, n, n // 4)
    T = X.shape[1]
    mag, ph = X.abs(), X.angle()
    out.append(("irfft_frames complex", lambda: ops.irfft_frames(X, w, n)))
    out.append(("irfft_frames polar", lambda: ops.irfft_frames(None, w, n, mag=mag, phase=ph)))
    for hop in (n // 8, n // 4, n // 2):
        R = n // hop
        for Tc in sorted({min(R, T), min(R + 2, T), T}):
            out.append(("istft hop %d T %d complex" % (hop, Tc), lambda hop=hop, Tc=Tc: ops.istft(X[:, :Tc].contiguous(), w, n, hop)))
            out.append(("istft hop %d T %d polar" % (hop, Tc), lambda hop=hop, Tc=Tc: ops.istft(
                None, w, n, hop, mag=mag[:, :Tc].contiguous(), phase=ph[:, :Tc].contiguous())))
    banks = {512: ((40, 44100), (128, 44100)), 2048: ((64, 16000), (60, 4000), (128, 44100), (100, 44100))}.get(n, ())
    for n_mels, sr in banks:
        band = BandedBank(O.melscale_fbanks(n // 2 + 1, 0.0, sr / 2.0, n_mels, sr))
        assert band.fusable512 if n == 512 else band.fusable2048, (n, n_mels, sr)
        for cm in (False, True):
            out.append(("mel %d @ %d %s" % (n_mels, sr, "channel-major" if cm else "rows"), lambda band=band, cm=cm: ops.stft_mel_forward(
                xs, w, band, contrast="log1p", power=2, want_spectrum=False, channel_major=cm, hop=n // 4, n_fft=n)[2]))
    return out


def same(a, b):
    if isinstance(a, tuple):
        return all(same(u, v) for u, v in zip(a, b))
    if a is None or b is None:
        return a is b
    return torch.equal(a, b) or torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                            b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


if args.equal:
    g = torch.Generator().manual_seed(7)
    bad = total = 0
    for n_fft in [int(v) for v in args.sizes.split(",")]:
        small = (torch.randn(3, 66 * (n_fft // 4) + 4, generator=g) * 0.1).to(dev)
        for tag, xs in (("small", small), ("1024 x 176400", x)):
            for what, fn in equal_entries(n_fft, xs):
                L._lib = handles["tree"]
                ref = fn()
                for name, h in handles.items():
                    if name == "tree":
                        continue
                    L._lib = h
                    ok = same(fn(), ref)
                    total += 1
                    bad += not ok
                    if not ok:
                        print("n_fft %5d  %-14s %-40s tree != %s" % (n_fft, tag, what, name), flush=True)
                L._lib = handles["tree"]
                del ref
            torch.cuda.empty_cache()
        print("n_fft %5d  compared, %d mismatches so far" % (n_fft, bad), flush=True)
    print("equal: %d comparisons, %d mismatches" % (total, bad))
    sys.exit(1 if bad or total == 0 else 0)

for n_fft in [int(v) for v in args.sizes.split(",")]:
    st = A.STFT(n_fft=n_fft, hop_length=n_fft // 4).to(dev)
    X = st(x)
    T, F = X.shape[-2], X.shape[-1]
    fwd_bytes = B * T * (n_fft // 4 * 4 + F * 8)
    entries = [("forward", lambda: st(x)), ("inverse", lambda: st.invert(X))]
    if args.extras and n_fft == 512:
        sp = A.STFT(n_fft=512, hop_length=128).to(dev)
        sp.eager_phase = True
        mel = A.MFCC(n_fft=512, hop_length=128, n_mels=64).to(dev)
        entries += [("forward+phase", lambda: sp(x)), ("mel 512/128/64", lambda: mel(x))]
    if len(handles) == 1 and args.rounds == 1:
        tf, ti = timeit(entries[0][1]), timeit(entries[1][1])
        print("n_fft %5d  frames/clip %4d  forward %.3f ms (%.2f TB/s)  inverse %.3f ms (%.2f TB/s)"
              % (n_fft, T, tf, fwd_bytes / tf / 1e9, ti, fwd_bytes / ti / 1e9), flush=True)
        entries = entries[2:]
        if not entries:
            continue
    for what, fn in entries:
        ms = {name: [] for name in handles}
        for r in range(args.rounds):
            for name, h in handles.items():
                L._lib = h
                ms[name].append(timeit(fn))
        L._lib = handles["tree"]
        print("n_fft %5d  %-15s " % (n_fft, what) + "  ".join(
            "%s %s ms (mean %.3f)" % (name, "/".join("%.3f" % v for v in vals), sum(vals) / len(vals))
            for name, vals in ms.items()), flush=True)
    del X

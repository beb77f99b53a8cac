"""Dev timing: STFT forward / inverse at other FFT sizes (1024 clips x 4 s, hop = n_fft / 4).

    python tools/nfft_probe.py [sizes] [--libs name=path,...] [--rounds R] [--extras]

--libs loads further builds of libacids_hip.so next to the in-tree one (as tools/step_probe.py `ab` does) and times
every entry under each of them in turn, R rounds, inside this one process: numbers from different processes or boxes
are not comparable (NOTES).  Give the same build twice under two file names for the A/A spread.  --extras adds, at
n_fft 512, the forward with phase output and the features-only MelSpectrogram (hop 128, 64 mels).  Only the symbols a
library exports are bound, so an older build of the same ABI version loads too."""
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

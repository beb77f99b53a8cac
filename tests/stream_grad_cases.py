"""Shared by test_stream_grad_cpu.py and test_stream_grad_gpu.py: the sweep of the streaming-path backward passes, the
reference's own statements written out of place in torch (any dtype; the tests run them in float64 on the CPU and take
torch autograd of them as the reference for every gradient), and numpy restatements of the four adjoint formulas.

The statements (reference transforms/oadd.py:69-104, stft.py:251 / 266, dgt.py:287 / 302):
    frames = unfold(pad(cat([history, x])))      X = rfft(frames * w)      f = irfft(X, n=N) * w~
    out    = (cat([tail, 0]) + sum_i shift(f[i], i h))[:out_len] / gain
History, tail and phase are constants: the gradient of a chunk covers that chunk's own samples.
"""
import itertools

import numpy as np
import torch

SIZES = [(1024, 256), (512, 128), (128, 32), (400, 100), (405, 135)]
FRAMES = [1, 2, 3, 9]           # 3 and 9 end a shared register FFT (2 / 4 / 8 frames) inside a stream
STREAMS = [1, 3]
FORMS = ["complex", "polar"]
FACTORS = {"size": SIZES, "n": FRAMES, "S": STREAMS, "form": FORMS}

# the kernel sweep: the full cross
SWEEP = [dict(size=z, n=n, S=S) for z, n, S in itertools.product(SIZES, FRAMES, STREAMS)]
SYNTH_SWEEP = [dict(c, form=f) for c in SWEEP for f in FORMS]


def sweep_id(c):
    return "N%d-h%d-n%d-S%d" % (c["size"] + (c["n"], c["S"])) + ("-" + c["form"] if "form" in c else "")


def keep_of(N, h):
    return (N // h - 1) * h


def n_frames(length, N, h):
    """Number of frames the reference's frame() makes (utils/misc.py:153-155)."""
    n = (length - N) // h
    if length >= n * h + N:
        n += 1
    return n


def chunk_lengths(N, h):
    """The OverlapAdd chunks: one hop, keep exactly, 4096 samples, and 1000 samples at 1024/256 (three frames, the last
    232 samples covered by none)."""
    out = [h, keep_of(N, h), 4096]
    if (N, h) == (1024, 256):
        out.append(1000)
    return out


def hann(N, dtype=torch.float64):
    return torch.hann_window(N, dtype=dtype)


def rand_window(N, seed=0, dtype=torch.float64):
    """A synthesis window without symmetry or zeros."""
    g = torch.Generator().manual_seed(1000 + seed)
    return (0.25 + torch.rand(N, generator=g, dtype=torch.float64)).to(dtype)


# ---- the reference's statements, out of place ----------------------------------------------------------------------------

def ref_frames(x, hist, N, h):
    """OverlapAdd.forward: x (..., C), hist (..., keep) -> (..., n, N)."""
    buf = torch.cat([hist, x], -1)
    nw = n_frames(buf.shape[-1], N, h)
    want = nw * h + N
    if buf.shape[-1] < want:
        buf = torch.cat([buf, buf.new_zeros(buf.shape[:-1] + (want - buf.shape[-1],))], -1)
    return buf.unfold(-1, N, h)[..., :nw, :]


def ref_analysis(frames, w):
    return torch.fft.rfft(frames * w, dim=-1)


def ref_synthesis(X, w_dual, N):
    return torch.fft.irfft(X, n=N, dim=-1) * w_dual


def ref_oadd_invert(frames, tail, N, h, gain):
    """OverlapAdd.invert: frames (..., n, N), tail (..., keep) -> (out (..., out_len), new tail (..., keep))."""
    n, keep = frames.shape[-2], tail.shape[-1]
    rec_len = (n - 1) * h + N
    rec = torch.cat([tail, tail.new_zeros(tail.shape[:-1] + (rec_len - keep,))], -1)
    for i in range(n):
        rec = rec + torch.nn.functional.pad(frames[..., i, :], (i * h, rec_len - i * h - N))
    return rec[..., :rec_len - keep] / gain, rec[..., rec_len - keep:]


def autograd_of(fn, x, upstream):
    """Gradient of fn(x) against `upstream` (torch's convention for a complex tensor) by torch autograd."""
    x = x.detach().clone().requires_grad_()
    y = fn(x)
    assert y.shape == upstream.shape, (y.shape, upstream.shape)
    y.backward(upstream)
    return x.grad


# ---- the four adjoints, restated in numpy ---------------------------------------------------------------------------------

def np_rfft_frames_backward(G, w, N):
    """q[r, m] = (N/2) w[m] irfft(G[r])[m] + w[m] (Re G[r,0] / 2 + Re G[r,N/2] (-1)^m / 2)."""
    G, w = np.asarray(G), np.asarray(w)
    edge = 0.5 * G[..., :1].real * np.ones(N)
    if N % 2 == 0:
        edge = edge + 0.5 * G[..., N // 2:N // 2 + 1].real * (-1.0) ** np.arange(N)
    return (N / 2) * w * np.fft.irfft(G, n=N, axis=-1) + w * edge


def np_irfft_frames_backward(gf, w_dual, N, phase=None):
    """gX[r, k] = (c_k / N) rfft(w~ gf[r])[k]; with a phase, gmag = Re gX cos phi + Im gX sin phi."""
    c = np.full(N // 2 + 1, 2.0)
    c[0] = 1.0
    if N % 2 == 0:
        c[N // 2] = 1.0
    gX = np.fft.rfft(np.asarray(gf) * np.asarray(w_dual), axis=-1) * (c / N)
    if phase is None:
        return gX
    phase = np.asarray(phase)
    return gX.real * np.cos(phase) + gX.imag * np.sin(phase)


def np_oadd_forward_backward(gf, N, h, keep, C):
    """gx[s, c] = sum_t gf[s, t, keep + c - t h] over the frames that cover the sample."""
    gf = np.asarray(gf)
    S, n, _ = gf.shape
    gx = np.zeros((S, C), dtype=gf.dtype)
    for t in range(n):
        c0, c1 = max(0, t * h - keep), min(C, t * h - keep + N)
        if c0 < c1:
            gx[:, c0:c1] += gf[:, t, keep + c0 - t * h:keep + c1 - t * h]
    return gx


def np_oadd_invert_backward(gy, n, N, h, keep, gain):
    """gf[s, t, o] = gy[s, t h + o] / gain where t h + o < out_len, else 0."""
    gy = np.asarray(gy)
    out_len = (n - 1) * h + N - keep
    gf = np.zeros((gy.shape[0], n, N), dtype=gy.dtype)
    for t in range(n):
        live = max(0, min(N, out_len - t * h))
        gf[:, t, :live] = gy[:, t * h:t * h + live] / gain
    return gf


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    denom = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (denom if denom > 0 else 1.0)

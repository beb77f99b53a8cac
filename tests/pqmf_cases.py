"""Float64 restatement of the PQMF (transforms/pqmf.py, csrc/pqmf.hip), written from the definition and shared by
test_pqmf_cpu.py and test_pqmf_gpu.py, and the case table of the GPU tests.

M = n_band, N = taps (odd), P = (N - 1) / 2:
    prototype   h[n] = (w / pi) sinc(w (n - P) / pi) kaiser(N, beta),  beta = 0.1102 (attenuation - 8.7)
    objective   phi(w) = max over l = 2M, 4M, ... < N of |sum_n h[n + l] h[n]|, on the grid w_i = pi / (2M) (1 + i / 1024)
    bank        h_k[n] = 2 h[n] cos((2k+1) pi / (2M) (n - P) + (-1)^k pi / 4)
    analysis    conv1d(x, h_k, stride=M, padding=P)
    synthesis   M sum_k conv1d(zero-stuffed y_k, flipped h_k, padding=P)
The prototype and the objective are numpy, analysis and synthesis float64 torch (so that torch autograd gives the
gradients the kernels are compared with)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

GRID = 1024
# (n_band, taps) of the parity sweep: the smallest legal filter; a non-power-of-two M with N = 51 not 1 mod 2M (a partial
# last fold group); the defaults; N = 257 = 1 mod 32; the LDS maximum of the defaults' family; an odd M with a 2-group fold
PARITY = ((2, 5), (3, 51), (16, 513), (16, 257), (64, 2049), (5, 11))
SPECIALISED = ((4, 65), (8, 99), (32, 1025), (6, 97))          # band counts with a kernel of their own, and a neighbour without
DESIGNS = ((16, None, 100.0), (4, 65, 100.0), (3, 51, 80.0))      # (n_band, taps, attenuation) of the design tests
GRAD = ((3, 51, "tile+1"), (16, 513, "2tile+1"))
MANY_ROWS = (65537, 2, 5, 4)                                      # rows, n_band, taps, L: past a 16-bit grid dimension


def block_counts(tile):
    """T of the parity sweep for a tile of `tile` blocks: a clip shorter than the filter, both sides of a tile boundary,
    and a third, one-block tile."""
    return (1, 2, tile - 1, tile, tile + 1, 2 * tile + 1)


def default_taps(n_band):
    return 32 * n_band + 1


def grid(n_band):
    return math.pi / (2 * n_band) * (1.0 + np.arange(GRID + 1) / GRID)


def prototype(cutoff, taps, attenuation):
    P = (taps - 1) // 2
    n = np.arange(taps, dtype=np.float64) - P
    beta = 0.1102 * (attenuation - 8.7)
    return (cutoff / np.pi) * np.sinc(cutoff * n / np.pi) * np.kaiser(taps, beta)


def phi(h, n_band):
    N = h.size
    return max(abs(float(np.dot(h[lag:], h[:N - lag]))) for lag in range(2 * n_band, N, 2 * n_band))


def phi_grid(n_band, taps, attenuation):
    return np.array([phi(prototype(w, taps, attenuation), n_band) for w in grid(n_band)])


def modulation(n_band, taps):
    """C (M, 2M) float64."""
    P = (taps - 1) // 2
    k = np.arange(n_band, dtype=np.float64)[:, None]
    r = np.arange(2 * n_band, dtype=np.float64)[None, :]
    return 2.0 * np.cos((2 * k + 1) * np.pi / (2 * n_band) * (r - P) + (-1.0) ** k * np.pi / 4)


def bank(h, n_band):
    """h_k (M, N) float64 from a prototype h (N,) (numpy or torch, any float dtype)."""
    h = np.asarray(h, dtype=np.float64)
    N = h.size
    P = (N - 1) // 2
    k = np.arange(n_band, dtype=np.float64)[:, None]
    n = np.arange(N, dtype=np.float64)[None, :]
    return 2.0 * h[None, :] * np.cos((2 * k + 1) * np.pi / (2 * n_band) * (n - P) + (-1.0) ** k * np.pi / 4)


def analysis(x, hk):
    """x (..., L) float64 torch, hk (M, N) numpy -> (..., M, L / M) float64 torch."""
    M, N = hk.shape
    w = torch.from_numpy(hk).unsqueeze(1)
    lead, L = x.shape[:-1], x.shape[-1]
    y = F.conv1d(x.reshape(-1, 1, L), w, stride=M, padding=(N - 1) // 2)
    return y.reshape(tuple(lead) + (M, L // M))


def synthesis(y, hk):
    """y (..., M, T) float64 torch, hk (M, N) numpy -> (..., M T) float64 torch: the definition read as a scatter,
    x^[tM + n - P] += M sum_k h_k[n] y[k, t] -- what synthesis_stuffed computes without its multiplications by the
    stuffed zeros (float64 conv1d takes seconds at n_band 64; test_pqmf_cpu.py holds the two together)."""
    M, N = hk.shape
    lead, T = y.shape[:-2], y.shape[-1]
    frames = torch.einsum("bkt,kn->bnt", y.reshape(-1, M, T), torch.from_numpy(hk))
    full = F.fold(frames, output_size=(1, (T - 1) * M + N), kernel_size=(1, N), stride=(1, M)).reshape(-1, (T - 1) * M + N)
    P = (N - 1) // 2
    x = M * full[:, P:P + T * M]                      # P >= M, so the slice lies inside the (T - 1) M + N samples
    return x.reshape(tuple(lead) + (T * M,))


def synthesis_stuffed(y, hk):
    """The same by the letter: zero-stuffing by M, then the time-reversed bank with padding P, summed over the bands,
    times M."""
    M, N = hk.shape
    lead, T = y.shape[:-2], y.shape[-1]
    y3 = y.reshape(-1, M, T)
    zeros = y3.new_zeros(y3.shape[0], M, T, M - 1)
    z = torch.cat([y3.unsqueeze(-1), zeros], -1).reshape(-1, M, T * M)                              # zero-stuffing by M
    w = torch.from_numpy(hk[:, ::-1].copy()).unsqueeze(0)                                           # (1, M, N), flipped
    x = M * F.conv1d(z, w, padding=(N - 1) // 2)
    return x.reshape(tuple(lead) + (T * M,))


def interior_rel_rms(xh, x, taps):
    """Relative rms of xh - x on the samples at least `taps` away from both ends."""
    a, b = np.asarray(xh)[..., taps:-taps], np.asarray(x)[..., taps:-taps]
    return float(np.sqrt(np.mean((a - b) ** 2) / np.mean(b ** 2)))


def audio(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    denom = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (denom if denom > 0 else 1.0)

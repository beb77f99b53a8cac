"""Shared by test_spectral_distance_cpu.py and test_spectral_distance_gpu.py: a float64 numpy model of the two kernels of
csrc/spectral_distance.hip, float64 torch autograd of the stated expression, the chunk rule of
autograd.specdist_chunk_clips restated, and the case tables."""
import numpy as np
import torch

EPS = float(torch.finfo(torch.float32).eps)
SLICE = 4096                    # kDistSlice of csrc/distance_core.h: bins one workgroup reduces
CHUNK_ELEMS = 1 << 26           # autograd.SPECDIST_CHUNK_ELEMS

DEFAULT_SCALES = ((2048, 512), (1024, 256), (512, 128), (256, 64), (128, 32))
# the module-level sweep: the default five, a mixed-radix size, a hop other than n / 4
SCALES = DEFAULT_SCALES + ((400, 100), (1024, 128))
MODULE_B, MODULE_L = 3, 4096

# (B, T, F) of the op-level spectra: n = 65 and 455, below one slice and odd, so clip 1 is only 8-byte aligned;
# n = 9225, odd again, three slices with a short last one; n = 353970, even, the 87 slices of a 4 s clip at n_fft 1024
OP_SHAPES = ((3, 1, 65), (2, 7, 65), (3, 9, 1025), (2, 690, 513))


def frames(n_fft, hop, L):
    return 1 + (L - (n_fft & 1)) // hop


def bins(n_fft, hop, L):
    return frames(n_fft, hop, L) * (n_fft // 2 + 1)


def chunk_clips(B, T, n_fft, elems=CHUNK_ELEMS):
    """The most clips whose one spectrum stays within `elems` complex64 elements, at least one."""
    return min(max(elems // (T * (n_fft // 2 + 1)), 1), B)


def chunks(B, T, n_fft, elems=CHUNK_ELEMS):
    c = chunk_clips(B, T, n_fft, elems)
    return [min(c, B - b0) for b0 in range(0, B, c)]


def slices(n):
    return (n + SLICE - 1) // SLICE


def spectra(shape, seed):
    """Two random complex64 spectra of `shape` (B, T, F) with exact zeros planted in both: bins where only X, only Y
    and both vanish, in the first and in the last clip."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    Y = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    F = shape[-1]
    for b in (0, shape[0] - 1):
        X[b, 0, 3:9] = 0
        Y[b, 0, 6:12] = 0
        X[b, -1, F - 2:] = 0
        Y[b, -1, F - 1:] = 0
    return X, Y


# ---- the float64 model of the kernels ---------------------------------------------------------------------------------------

def model_sums(X, Y, eps=EPS):
    """What at_spectral_distance_sums computes: (B, 3) float64 of S_D, S_B, S_L.  X, Y (B, ...) complex."""
    B = X.shape[0]
    A, Bm = np.abs(X.astype(np.complex128)).reshape(B, -1), np.abs(Y.astype(np.complex128)).reshape(B, -1)
    return np.stack([((A - Bm) ** 2).sum(1), (Bm ** 2).sum(1), np.abs(np.log(A + eps) - np.log(Bm + eps)).sum(1)], 1)


def model_loss(sums, n, lin_weight=1.0, log_weight=1.0):
    """loss_b of one scale from its sums (B, 3) and its n bins per clip."""
    return lin_weight * sums[:, 0] / sums[:, 1] + log_weight * sums[:, 2] / n


def model_backward(X, Y, g, lin_weight=1.0, log_weight=1.0, eps=EPS, need_x=True, need_y=True):
    """What at_spectral_distance_backward writes over X and Y: (G_X or None, G_Y or None), complex128 of X's shape,
    dRe + i dIm.  g (B,): the gradient of the per-clip loss."""
    B = X.shape[0]
    X, Y = X.astype(np.complex128), Y.astype(np.complex128)
    sums = model_sums(X, Y, eps)
    n = X[0].size
    tail = (1,) * (X.ndim - 1)
    gb, S_D, S_B = (np.asarray(v, dtype=np.float64).reshape((B,) + tail) for v in (g, sums[:, 0], sums[:, 1]))
    A, Bm = np.abs(X), np.abs(Y)
    d = A - Bm
    sg = np.sign(d)
    GX = GY = None
    with np.errstate(divide="ignore", invalid="ignore"):
        if need_x:
            dA = gb * (lin_weight * 2 * d / S_B + log_weight * sg / (n * (A + eps)))
            GX = np.where(A > 0, dA / np.where(A > 0, A, 1.0), 0.0) * X
        if need_y:
            dB = gb * (lin_weight * (-2 * d / S_B - 2 * Bm * S_D / S_B ** 2) - log_weight * sg / (n * (Bm + eps)))
            GY = np.where(Bm > 0, dB / np.where(Bm > 0, Bm, 1.0), 0.0) * Y
    return GX, GY


# ---- float64 torch autograd of the stated expression --------------------------------------------------------------------------

def torch_loss(Xt, Yt, lin_weight=1.0, log_weight=1.0, eps=EPS):
    """loss_b (B,) of one scale, as the issue states it, on complex128 torch spectra (B, ...)."""
    B = Xt.shape[0]
    A, Bm = Xt.abs().reshape(B, -1), Yt.abs().reshape(B, -1)
    lin = ((A - Bm) ** 2).sum(1) / (Bm ** 2).sum(1)
    log = (torch.log(A + eps) - torch.log(Bm + eps)).abs().sum(1) / A.shape[1]
    return lin_weight * lin + log_weight * log


def autograd_backward(X, Y, g, lin_weight=1.0, log_weight=1.0, eps=EPS):
    """(G_X, G_Y) complex128 numpy: torch autograd of torch_loss weighted by g (B,), in float64."""
    Xt = torch.from_numpy(X.astype(np.complex128)).requires_grad_()
    Yt = torch.from_numpy(Y.astype(np.complex128)).requires_grad_()
    loss = torch_loss(Xt, Yt, lin_weight, log_weight, eps)
    loss.backward(torch.as_tensor(np.asarray(g, dtype=np.float64)))
    return Xt.grad.numpy(), Yt.grad.numpy()


# ---- the float64 torch.stft chain (the module-level reference) ------------------------------------------------------------------

def stft64(x64, n_fft, hop, window="hann"):
    """(B, T, F) complex128 of (B, L) float64 audio with STFT's conventions."""
    w = getattr(torch, "%s_window" % window)(n_fft, dtype=torch.float64)
    return torch.stft(x64, n_fft, hop, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(-2, -1)


def chain_loss(x64, y64, scales, lin_weight=1.0, log_weight=1.0, eps=EPS):
    """The per-clip multi-scale loss (B,) float64 of the torch.stft chain."""
    return sum(torch_loss(stft64(x64, n, h), stft64(y64, n, h), lin_weight, log_weight, eps) for n, h in scales)


def stft_adjoint64(x64, n_fft, hop, G):
    """x.grad of stft64(x) fed the upstream gradient G (B, T, F) complex128."""
    xr = x64.detach().clone().requires_grad_()
    X = stft64(xr, n_fft, hop)
    X.backward(torch.as_tensor(G).reshape(X.shape))
    return xr.grad

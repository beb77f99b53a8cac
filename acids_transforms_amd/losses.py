"""Losses on MI355X: SpectralDistance, the multi-scale STFT distance a generative-audio model is trained with, and
MelSpectralDistance, the same distance between mel-band magnitudes (csrc/mel_distance.hip).

The transforms of this package make a model differentiable THROUGH a spectrum; this is the distance it is trained
WITH.  Composed from STFT + Magnitude + torch expressions, every scale keeps its spectrum for the backward; here the
graph keeps the two audio tensors and three sums per clip and scale, and the backward rebuilds the spectra a chunk of
clips at a time (autograd.SpectralDistanceFunction, csrc/spectral_distance.hip).
"""
import torch
from torch import nn

from . import ops
from ._lib import device_scoped, require_device
from .autograd import (MelSpectralDistanceFunction, SpectralDistanceFunction, _meldist_tables, meldist_loss, meldist_sums,
                       specdist_loss, specdist_sums)
from .transforms.stft import MAX_NFFT
from .utils.melbank import melscale_fbanks

__all__ = ["SpectralDistance", "MelSpectralDistance"]

DEFAULT_SCALES = ((2048, 512), (1024, 256), (512, 128), (256, 64), (128, 32))
DEFAULT_MEL_SCALES = ((2048, 512, 320), (1024, 256, 160), (512, 128, 80), (256, 64, 40), (128, 32, 20))


class _MultiScaleDistance(nn.Module):
    """What the two distances share: the constructor's checks, the buffers of a scale (a window, then bank(*scale) as
    mel_bank_i when a bank is given), the checks of a call, the flattening of the clips, the grad-mode branch and the
    reduction.  A scale is a tuple that starts with n_fft, hop.  A subclass names its fields, its autograd.Function and
    the sums and loss functions behind it, and gives _extra, the arguments they take after the scales."""

    def __init__(self, scales, window, lin_weight, log_weight, eps, reduction, bank=None):
        super().__init__()
        if not hasattr(torch, "%s_window" % window):
            raise ValueError("Window %s is not known" % window)
        if reduction not in ("none", "sum", "mean"):
            raise ValueError("reduction %s not known (none, sum, mean)" % reduction)
        self.scales = tuple(scales)
        if not self.scales:
            raise ValueError("at least one (%s) scale is needed" % self._FIELDS)
        for scale in self.scales:
            name = "scale (%s)" % ", ".join("%d" % v for v in scale)
            if not (1 < scale[0] <= MAX_NFFT and scale[1] > 0):
                raise ValueError("%s: n_fft must lie in 2 .. %d and hop be positive" % (name, MAX_NFFT))
            if bank is not None and scale[2] < 1:
                raise ValueError("%s: n_mels must be at least 1" % name)
        if eps < 0:
            raise ValueError("eps must not be negative")
        self.lin_weight, self.log_weight, self.eps, self.reduction = float(lin_weight), float(log_weight), float(eps), reduction
        for i, scale in enumerate(self.scales):
            self.register_buffer("window_%d" % i, getattr(torch, "%s_window" % window)(scale[0]))
            if bank is not None:
                self.register_buffer("mel_bank_%d" % i, bank(*scale))

    def _windows(self):
        return tuple(getattr(self, "window_%d" % i) for i in range(len(self.scales)))

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if x.shape != y.shape:
            raise ValueError("x and y must have one shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        longest = max(scale[0] for scale in self.scales)
        if x.dim() < 1 or x.shape[-1] <= longest // 2:
            raise ValueError("clips of %d samples are too short for n_fft %d (reflect padding needs more than n_fft // 2)"
                             % (x.shape[-1] if x.dim() else 0, longest))
        device_scoped(require_device)(x, y)      # no CPU route, and one device for both
        if self.window_0.device != x.device:
            self.to(x.device)
        L = x.shape[-1]
        # torch's own reshape / float / contiguous: they carry the gradient back to the caller's tensors
        xb, yb = (ops._no_fp64(t).reshape(-1, L).float().contiguous() for t in (x, y))
        args = (xb, yb, self._windows(), self.scales) + self._extra(x.device)
        if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            per_clip = self._function.apply(*args, self.lin_weight, self.log_weight, self.eps)
        else:
            per_clip = self._loss(self._sums(*args, self.eps), L, self.scales, self.lin_weight, self.log_weight)
        per_clip = per_clip.reshape(x.shape[:-1])
        if self.reduction == "none":
            return per_clip
        return per_clip.sum() if self.reduction == "sum" else per_clip.mean()


class SpectralDistance(_MultiScaleDistance):
    """loss = crit(x, y): x the generated audio, y the target, one shape (..., L), float32, on the GPU.

    A scale is (n_fft, hop), any pair STFT accepts, with STFT's conventions (periodic window, center=True, reflect
    padding, T = 1 + L // hop).  For clip b and scale s, A = |STFT_s(x_b)| and Bm = |STFT_s(y_b)| of n = T_s F_s bins:

        S_D = sum (A - Bm)^2        S_B = sum Bm^2        S_L = sum |log(A + eps) - log(Bm + eps)|
        loss_b = sum_s [ lin_weight * S_D / S_B  +  log_weight * S_L / n ]

    reduction: "none" (shape x.shape[:-1]), "sum" or "mean" over the clips.  A silent target clip (S_B == 0) gives the
    IEEE result (inf or nan) in that clip only; a clip's value and gradient never depend on the rest of the batch.

    Gradients: for whichever of x and y requires one when grad mode is on (first order only); every other call runs
    the same kernels without a graph, to the same bits."""

    _FIELDS, _function = "n_fft, hop", SpectralDistanceFunction
    _sums, _loss = staticmethod(specdist_sums), staticmethod(specdist_loss)

    def __init__(self, scales=DEFAULT_SCALES, window: str = "hann", lin_weight: float = 1.0, log_weight: float = 1.0,
                 eps: float = torch.finfo(torch.float32).eps, reduction: str = "mean"):
        super().__init__(((int(n), int(h)) for n, h in scales), window, lin_weight, log_weight, eps, reduction)

    def __repr__(self):
        return "SpectralDistance(scales=%s, lin_weight=%g, log_weight=%g, reduction=%s)" % (
            self.scales, self.lin_weight, self.log_weight, self.reduction)

    def _extra(self, device):
        return ()


class MelSpectralDistance(_MultiScaleDistance):
    """loss = crit(x, y): x the generated audio, y the target, one shape (..., L), float32, on the GPU.

    A scale is (n_fft, hop, n_mels), with STFT's conventions (periodic window, center=True, reflect padding,
    T = 1 + L // hop) and the HTK bank W_s = melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sr), a constant
    buffer.  For clip b and scale s, M = |STFT_s(x_b)| @ W_s and Q = |STFT_s(y_b)| @ W_s of n = T_s n_mels cells:

        S_D = sum (M - Q)^2        S_B = sum Q^2        S_L = sum |log(M + eps) - log(Q + eps)|
        loss_b = sum_s [ lin_weight * S_D / S_B  +  log_weight * S_L / n ]

    An empty filter counts in n and adds 0 to the three sums.  reduction: "none" (shape x.shape[:-1]), "sum" or "mean"
    over the clips.  A silent target clip (S_B == 0) gives the IEEE result (inf or nan) in that clip only; a clip's
    value and gradient never depend on the rest of the batch.  f_max None: sr // 2.

    Gradients: for whichever of x and y requires one when grad mode is on (first order only); every other call runs
    the same kernels without a graph, to the same bits."""

    _FIELDS, _function = "n_fft, hop, n_mels", MelSpectralDistanceFunction
    _sums, _loss = staticmethod(meldist_sums), staticmethod(meldist_loss)

    def __init__(self, scales=DEFAULT_MEL_SCALES, sr: int = 44100, f_min: float = 0.0, f_max=None, window: str = "hann",
                 lin_weight: float = 1.0, log_weight: float = 1.0, eps: float = torch.finfo(torch.float32).eps,
                 reduction: str = "mean"):
        self.sr, self.f_min = int(sr), float(f_min)
        self.f_max = float(self.sr // 2 if f_max is None else f_max)
        super().__init__(((int(n), int(h), int(m)) for n, h, m in scales), window, lin_weight, log_weight, eps, reduction,
                         bank=lambda n, _, m: melscale_fbanks(n // 2 + 1, self.f_min, self.f_max, m, self.sr))

    def __repr__(self):
        return "MelSpectralDistance(scales=%s, sr=%d, lin_weight=%g, log_weight=%g, reduction=%s)" % (
            self.scales, self.sr, self.lin_weight, self.log_weight, self.reduction)

    def _extra(self, device):
        return (_meldist_tables(self, device),)

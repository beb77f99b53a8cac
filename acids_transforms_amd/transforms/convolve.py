"""FFTConvolve, Convolve and ImpulseResponse: convolution of audio with a long filter along the last axis (not in the
reference package; the signatures and the three modes are torchaudio's transforms.FFTConvolve / Convolve and
functional.fftconvolve).

The route is a uniformly partitioned overlap-save convolution: with block B (ops.fft_convolve_plan: the smallest of 512,
1024, 2048 with at most 4 partitions), frames of 2 B samples every B samples and the filter cut into partitions of B taps,

    Y[t] = sum_p H[p] X[t - p],        block t of the result = the last B samples of irfft(Y[t]).

The transforms on both sides are the library's STFT kernels with a rectangular window; the sum over p is fft_convolve.hip,
one lane per bin, and the filter's gradient is its correlation kernel.  `Convolve` runs the same route as `FFTConvolve` (a
direct time-domain kernel for filters of a few taps is not built), so the two agree to the bit.

Gradients: a call in which x or the filter requires grad (with grad mode on) goes through autograd.FFTConvolveFunction,
which saves the two inputs and rebuilds the spectra in its backward; every other call is the plain route with the same
bits.  First order only.

Not built: a streaming form (it needs a frequency-domain delay line carried across chunks), a direct time-domain kernel for
short filters, time-varying filters, a non-uniform partition, second-order gradients.
"""
import warnings
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..autograd import FFTConvolveFunction, wants_grad
from .base import AudioTransform, InversionEnumType, NotInvertibleError

__all__ = ["FFTConvolve", "Convolve", "ImpulseResponse", "fftconvolve"]

_SELFTEST_TAPS = 300      # the self-test hooks convolve with a decaying burst when the module has no response of its own


def fftconvolve(x: torch.Tensor, y: torch.Tensor, mode: str = "full", block: Optional[int] = None) -> torch.Tensor:
    """torchaudio.functional.fftconvolve(x, y, mode): x (..., L), y (K,) -- shared by every row -- or (..., K) with x's
    leading shape.  Differentiable in both."""
    if wants_grad(x) or wants_grad(y):
        return FFTConvolveFunction.apply(x, y, mode, block)
    return ops.fft_convolve(x, y, mode, block)


class FFTConvolve(nn.Module):
    """torchaudio.transforms.FFTConvolve: forward(x, y) convolves x (..., L) with y (..., K) along the last axis."""

    def __init__(self, mode: str = "full"):
        super().__init__()
        if mode not in ops.FFT_CONVOLVE_MODES:
            raise ValueError("mode must be one of %s, got %r" % (ops.FFT_CONVOLVE_MODES, mode))
        self.mode = mode

    def extra_repr(self) -> str:
        return "mode=%r" % self.mode

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return fftconvolve(x, y, self.mode)


class Convolve(FFTConvolve):
    """torchaudio.transforms.Convolve: the same result, and here the same kernels, as FFTConvolve."""


class ImpulseResponse(AudioTransform):
    """(..., L) -> (..., L): the full convolution with the 1-D response `ir`, cut to the first L samples; with tail=True all
    L + K - 1 samples.  `ir` is a buffer, or with learnable=True an nn.Parameter that receives a gradient.  ir=None is the
    pass-through and returns x itself; it has nothing to learn, so ir=None with learnable=True is a ValueError."""
    invertible = False
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "ImpulseResponse(taps=%d, tail=%s, learnable=%s)" % (self.taps, self.tail, self.learnable)

    def __init__(self, ir=None, tail: bool = False, learnable: bool = False, sr: int = 44100):
        super().__init__(sr=sr)
        self.tail, self.learnable = bool(tail), bool(learnable)
        self.passthrough = ir is None
        if ir is None:
            if self.learnable:
                raise ValueError("learnable=True needs a response to start from: pass ir (torch.ones(1) is the identity)")
            ir = torch.ones(1)
        ir = torch.as_tensor(ir).detach().clone()
        if ir.dim() != 1 or ir.numel() < 1:
            raise ValueError("ir must be 1-D with at least one tap, got shape %s" % (tuple(ir.shape),))
        if not ir.is_floating_point():
            ir = ir.float()
        if self.learnable:
            self.ir = nn.Parameter(ir)
        else:
            self.register_buffer("ir", ir)

    @property
    def taps(self) -> int:
        return int(self.ir.shape[-1])

    def _run(self, x: torch.Tensor, ir: torch.Tensor) -> torch.Tensor:
        if x.dim() < 1 or x.shape[-1] < 1:
            raise ValueError("ImpulseResponse takes (..., L >= 1), got %s" % (tuple(x.shape),))
        y = fftconvolve(x, ir, "full")
        return y if self.tail else y[..., :x.shape[-1]]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.passthrough:
            return x
        return self._run(x, self.ir)

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

    def realtime(self):
        warnings.warn("ImpulseResponse has no streaming form: realtime() returns the offline module, which starts every "
                      "chunk from silence and drops the tail of the one before", stacklevel=2)
        return self

    # -- self-test hooks (the reference's test file drives every class through them) with a response that is not the
    # pass-through, so that the kernels run ----------------------------------------------------------------------------------
    def _selftest_ir(self, device) -> torch.Tensor:
        if not self.passthrough:
            return self.ir
        g = torch.Generator().manual_seed(0)
        burst = torch.randn(_SELFTEST_TAPS, generator=g) * torch.exp(-torch.arange(_SELFTEST_TAPS) / 60.0)
        return (burst / burst.abs().sum()).to(device)

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        y = self._run(x, self._selftest_ir(x.device))
        return y if time is None else (y, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(2, 2, 4101, generator=g) * 2 - 1).to("cuda")
        n = x.shape[-1] + (_SELFTEST_TAPS - 1 if transform.tail and transform.passthrough else
                           transform.taps - 1 if transform.tail else 0)
        y = transform.test_forward(x)
        assert y.shape == x.shape[:-1] + (n,) and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert y.shape == x.shape[:-1] + (n,) and time.shape == (2, 2)

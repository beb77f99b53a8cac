"""TimeStretch: the phase vocoder, the stage between `STFT()` and `STFT.invert` that changes a signal's duration.

The counterpart of torchaudio.transforms.TimeStretch / torchaudio.functional.phase_vocoder (algorithm restated; torchaudio
is not a dependency) in this package's time-major layout: a complex spectrum (..., T, F) in, (..., N, F) out, N the
number of j = 0, 1, ... with j * rate < T, so rate > 1 shortens and rate < 1 lengthens.  Output frame j interpolates the
magnitudes of input frames floor(j rate) and floor(j rate) + 1 (a frame of zeros past the end) and carries the phase
accumulated over the steps before it.

The arithmetic is phase_vocoder.hip, one scan per call.  The textbook phase increment wrap(a1 - a0 - advance) + advance
is congruent to a1 - a0 and only ever goes through exp(i .), so the expected advance -- pi hop_length f / (F - 1) --
cancels: the accumulated phase is a running product of unit phasors and `hop_length` has provably no effect on the result.
It is accepted for call sites written against torchaudio, as is `n_freq`, which is checked against the input when given.
Zero bins come out as zeros; the one divergence from the angle route is a bin that is exactly -0 + 0i, whose angle
torch.angle reports as pi and which counts as zero phase here.

`forward` is differentiable: a call whose input requires grad (with grad mode on) runs the same kernel through
autograd.PhaseVocoderFunction, whose backward is the second kernel of phase_vocoder.hip (first order only); every other
call is the plain route, bit for bit.  There is no inverse (a stretch by 1 / rate is not one) and no streaming form: a
streaming vocoder would carry the phasor across chunks.
"""
import warnings
from typing import Optional

import torch

from .. import ops
from ..autograd import PhaseVocoderFunction, wants_grad
from .base import AudioTransform, InversionEnumType, NotInvertibleError

__all__ = ["TimeStretch"]

_SELFTEST_RATE = 0.8      # the self-test hooks stretch by this when the module's own rate is 1 (which runs no kernel)


class TimeStretch(AudioTransform):
    invertible = False
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "TimeStretch(rate=%s)" % self.rate

    def __init__(self, rate: float = 1.0, n_freq: Optional[int] = None, hop_length: Optional[int] = None, sr: int = 44100):
        super().__init__(sr=sr)
        self.rate = self._checked(rate)
        self.n_freq = None if n_freq is None else int(n_freq)
        self.hop_length = hop_length          # no effect: the expected phase advance cancels (module docstring)

    @staticmethod
    def _checked(rate) -> float:
        rate = float(rate)
        if not (rate == rate and 0.0 < rate < float("inf")):
            raise ValueError("rate must be finite and > 0, got %r" % (rate,))
        return rate

    @property
    def ratio(self):
        return 1.0 / self.rate

    def forward(self, x: torch.Tensor, overriding_rate: Optional[float] = None) -> torch.Tensor:
        """x (..., T, F) complex -> (..., N, F) complex64.  `rate == 1.0` returns x itself."""
        rate = self.rate if overriding_rate is None else self._checked(overriding_rate)
        if not x.is_complex():
            raise ValueError("TimeStretch takes a complex spectrum (..., frames, bins), got %s"
                             % str(x.dtype).replace("torch.", ""))
        if x.ndim < 2:
            raise ValueError("TimeStretch takes (..., frames, bins), got shape %s" % (tuple(x.shape),))
        if self.n_freq is not None and x.shape[-1] != self.n_freq:
            raise ValueError("the spectrum has %d bins, n_freq is %d" % (x.shape[-1], self.n_freq))
        if rate == 1.0:
            return x
        if wants_grad(x):
            return PhaseVocoderFunction.apply(x, rate)
        return ops.phase_vocoder(x, rate)

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

    def realtime(self):
        warnings.warn("TimeStretch has no streaming form: realtime() returns the offline module, which starts the "
                      "accumulated phase afresh at every chunk", stacklevel=2)
        return self

    # -- self-test hooks (the reference's test file drives every class through them): STFT() of the audio, or a random
    # spectrum, stretched by a rate that is not 1 so that the kernel runs ------------------------------------------------
    def _selftest_rate(self) -> float:
        return self.rate if self.rate != 1.0 else _SELFTEST_RATE

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        from .stft import STFT
        stage = STFT().to(x.device)
        if time is None:
            return self.forward(stage(x), self._selftest_rate())
        X, time = stage.forward_with_time(x, time)
        return self.forward(X, self._selftest_rate()), time

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        from ._selftest import random_spectrum
        X = random_spectrum("cuda")
        y = transform.forward(X, transform._selftest_rate())
        assert y.shape[:-2] == X.shape[:-2] and y.shape[-1] == X.shape[-1] and y.shape[-2] != X.shape[-2]

"""TimeStretch: the phase vocoder, the stage between `STFT()` and `STFT.invert` that changes a signal's duration -- and
PitchShift, which stretches audio with it and resamples the result back to its length (the class's docstring).

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
import math
import warnings
from typing import Optional

import torch

from .. import ops
from ..autograd import PhaseVocoderFunction, ResampleDirectFunction, wants_grad
from .base import AudioTransform, InversionEnumType, NotInvertibleError

__all__ = ["TimeStretch", "PitchShift"]

_SELFTEST_RATE = 0.8      # the self-test hooks stretch by this when the module's own rate is 1 (which runs no kernel)
_SELFTEST_STEPS = 4.0     # and shift the pitch by this when the module's own n_steps is 0


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


class PitchShift(AudioTransform):
    """torchaudio.transforms.PitchShift (algorithm restated; torchaudio is not a dependency): audio (..., L) shifted by
    `n_steps` steps of an octave of `bins_per_octave`, same length out.  With rate = 2 ** (-n_steps / bins_per_octave) in
    host float64 and orig_freq = int(sr / rate), in torchaudio's order:
        STFT(sr, n_fft, hop_length) -> TimeStretch(rate) -> STFT.invert -> crop or zero-pad at the end to round(L / rate)
        -> resample orig_freq -> sr -> crop or zero-pad at the end to L.
    The converter is the bankless one (ops.resample_direct, sinc_interp.hip): at 4 steps and 44100 Hz orig_freq is 55562
    and the rates reduce to 27781 -> 22050, whose polyphase bank would hold 2.4 GB where the half-table holds 673 KB.
    `orig_freq == sr` (n_steps = 0) returns x itself.

    Differentiable: every stage has a HIP backward or is torch's own slice or pad, so a call whose input requires grad
    carries a gradient back to x (first order only); every other call is the plain route with the same bits.  There is no
    inverse and no streaming form (the vocoder would carry its phasor, the converter its window, across chunks)."""
    invertible = False
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "PitchShift(sr=%d, n_steps=%s, bins_per_octave=%d, n_fft=%d, hop_length=%d)" % (
            self.sr, self.n_steps, self.bins_per_octave, self.n_fft, self.hop_length)

    def __init__(self, sr: int = 44100, n_steps: float = 0.0, bins_per_octave: int = 12, n_fft: int = 512,
                 hop_length: Optional[int] = None, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        from .stft import STFT
        super().__init__(sr=sr)
        self.bins_per_octave = int(bins_per_octave)
        if self.bins_per_octave < 1:
            raise ValueError("bins_per_octave must be >= 1, got %r" % (bins_per_octave,))
        self.n_steps = float(n_steps)
        self.n_fft = int(n_fft)
        self.hop_length = self.n_fft // 4 if hop_length is None else int(hop_length)
        self.lowpass_filter_width, self.rolloff = lowpass_filter_width, rolloff
        self.rate, self.orig_freq = self._rates(self.n_steps)
        self.stft = STFT(sr=sr, n_fft=self.n_fft, hop_length=self.hop_length)
        self.stretch = TimeStretch(self.rate, sr=sr)

    def _rates(self, n_steps: float):
        """(rate, orig_freq) of a shift by n_steps."""
        if not math.isfinite(n_steps):
            raise ValueError("n_steps must be finite, got %r" % (n_steps,))
        rate = 2.0 ** (-n_steps / self.bins_per_octave)
        orig_freq = int(self.sr / rate)
        if orig_freq < 1:
            raise ValueError("a shift by %r steps leaves no sample rate to convert from" % (n_steps,))
        return rate, orig_freq

    def _resample(self, y: torch.Tensor, orig_freq: int) -> torch.Tensor:
        if not wants_grad(y):
            return ops.resample_direct(y, orig_freq, self.sr, self.lowpass_filter_width, self.rolloff)
        orig, new = ops._reduced_rates(orig_freq, self.sr)
        table, Qi = ops._sinc_table_on(y.device, orig, new, self.lowpass_filter_width, self.rolloff)
        out = ResampleDirectFunction.apply(y.reshape(math.prod(y.shape[:-1]), y.shape[-1]), table, Qi, orig, new)
        return out.reshape(tuple(y.shape[:-1]) + (out.shape[-1],))

    @staticmethod
    def _fit(y: torch.Tensor, n: int) -> torch.Tensor:
        """Crop, or zero-pad at the end, to n samples."""
        if y.shape[-1] > n:
            return y[..., :n]
        return torch.nn.functional.pad(y, (0, n - y.shape[-1])) if y.shape[-1] < n else y

    def _shift(self, x: torch.Tensor, rate: float, orig_freq: int) -> torch.Tensor:
        if orig_freq == self.sr:
            return x
        L = x.shape[-1]
        y = self.stft.invert(self.stretch(self.stft(x), rate))
        y = self._resample(self._fit(y, int(round(L / rate))), orig_freq)
        return self._fit(y, L)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (..., L) -> (..., L).  `n_steps == 0` returns x itself."""
        return self._shift(x, self.rate, self.orig_freq)

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

    def realtime(self):
        warnings.warn("PitchShift has no streaming form: realtime() returns the offline module, which starts the "
                      "vocoder's phase and the converter's window afresh at every chunk", stacklevel=2)
        return self

    # -- self-test hooks: a shift that is not 0, so that every kernel of the chain runs ----------------------------------
    def _selftest_shift(self, x: torch.Tensor) -> torch.Tensor:
        if self.n_steps != 0.0:
            return self.forward(x)
        return self._shift(x, *self._rates(_SELFTEST_STEPS))

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        y = self._selftest_shift(x)
        return y if time is None else (y, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(2, 4096, generator=g) * 2 - 1).to("cuda")
        y = transform._selftest_shift(x)
        assert y.shape == x.shape and bool(torch.isfinite(y).all())

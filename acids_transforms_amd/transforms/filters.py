"""SOSFilter, RealtimeSOSFilter and Preemphasis: recursive (IIR) filtering along the last axis, as cascades of second-order
sections (not in the reference package; the recurrence and state layout are scipy.signal.sosfilt's).

    y = b0 v + z1,   z1' = b1 v - a1 y + z2,   z2' = b2 v - a2 y        per section, a0 == 1, v the section before's output

The arithmetic is sos_filter.hip, one launch per call (two with `zero_phase`): a workgroup per row walks the row in tiles,
every lane runs its own samples from a zero state and a scan over the lanes' end states supplies the rest.  State,
coefficients and the signal between sections are double -- an fp32 state or fp32 coefficients are 1e-4 off on a 20 Hz
high-pass -- and only the audio is float32.  The coefficients the kernel uses are the float64 values given at construction:
the authoritative copy lives on the host (nothing synchronises in a call), `.to()`, `.float()` and `.half()` on the module do
not touch it, and `state_dict` carries it exactly, as the float64 entry `sos`.  utils.filter_design makes the usual ones.

Gradients: a call whose input requires grad (with grad mode on) goes through autograd.SosFilterFunction -- the backward is
the same kernel run the other way in time -- and every other call is the plain route with the same bits.  Coefficients are
constants of the graph.  First order only.

`zero_phase=True` filters forwards, then backwards, both from ZERO state and without edge padding: the squared magnitude
response, no phase, and its own adjoint.  It equals scipy.signal.sosfilt applied twice with flips; it is NOT
scipy.signal.sosfiltfilt(padtype=None), which still primes both passes with the sections' step-response steady state
times the edge sample (a priming that is not self-adjoint, and that the reverse kernel, which takes no state, has no
way in for).

Streaming: RealtimeSOSFilter carries the sections' state across chunks of any length >= 1.  A causal filter needs no
look-ahead: `latency` is 0.  The outputs of any chunking concatenate to the one-call result within rounding (1e-6), NOT to
the bit: the kernel's tile grid starts at each chunk's first sample, so the lanes' partial sums meet in another order.

Not built: gradients with respect to the coefficients, per-row or time-varying coefficients, bit-equal chunking, second-order
gradients.  (The gated loudness measure on top of filter_design.k_weighting is transforms/loudness.py.)
"""
import warnings
from typing import Optional

import torch

from .. import ops
from ..autograd import SosFilterFunction, SosFilterStreamFunction, wants_grad
from .base import AudioTransform, InversionEnumType, NotInvertibleError
from .carried import CarriedState

__all__ = ["SOSFilter", "RealtimeSOSFilter", "Preemphasis"]


def _selftest_sos(sr):
    """What the self-test hooks filter with when the module's own filter is the pass-through: a 20 Hz high-pass, the case
    that needs the double state, and a peak."""
    import numpy as np
    from ..utils import filter_design as fd
    return ops.sos_coefficients(np.concatenate([fd.highpass(sr, 20.0), fd.equalizer(sr, 1000.0, 6.0, 4.0)]))


class SOSFilter(AudioTransform):
    """(..., L) -> (..., L) through the sections `sos` (anything array-like of shape (n, 6), scipy's layout; n <= 16).
    `sos=None` is the pass-through and returns x itself."""
    invertible = False
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "%s(n_sections=%d, zero_phase=%s)" % (type(self).__name__, self.n_sections, self.zero_phase)

    def __init__(self, sos=None, zero_phase: bool = False, sr: int = 44100):
        super().__init__(sr=sr)
        self.zero_phase = bool(zero_phase)
        self._set_coefficients(None if sos is None else ops.sos_coefficients(sos))

    def _set_coefficients(self, co) -> None:
        self._co = co                                        # the host copy the kernel reads
        shown = torch.zeros(0, 6, dtype=torch.float64) if co is None else torch.from_numpy(co.array.copy())
        self.register_buffer("sos", shown)                   # for state_dict and inspection; no call reads it

    @property
    def n_sections(self) -> int:
        return 0 if self._co is None else self._co.n

    @property
    def coefficients(self):
        """The (n, 6) float64 host array in use (None: the pass-through)."""
        return None if self._co is None else self._co.array.copy()

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self._co is not None:                             # whatever a cast made of the buffer: the exact values
            destination[prefix + "sos"] = torch.from_numpy(self._co.array.copy())

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        got = state_dict.get(prefix + "sos")
        if got is not None:
            self._set_coefficients(ops.sos_coefficients(got.double()) if got.numel() else None)
            state_dict = dict(state_dict)
            state_dict[prefix + "sos"] = self.sos            # the shape matches now
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _run(self, x: torch.Tensor, co, zero_phase: bool) -> torch.Tensor:
        if wants_grad(x):
            y = SosFilterFunction.apply(x, co, False)
            return SosFilterFunction.apply(y, co, True) if zero_phase else y
        y = ops.sos_filter(x, co)
        return ops.sos_filter(y, co, reverse=True) if zero_phase else y

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._co is None:
            return x
        return self._run(x, self._co, self.zero_phase)

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

    def streaming(self) -> "RealtimeSOSFilter":
        """The streaming form of this filter: a RealtimeSOSFilter that shares its coefficients."""
        if self.zero_phase:
            raise ValueError("zero-phase filtering runs backwards over the whole signal: it has no streaming form")
        rt = RealtimeSOSFilter(self._co, sr=self.sr)
        return rt.to(self.sos.device)

    def realtime(self):
        if self.zero_phase:
            warnings.warn("zero-phase filtering has no streaming form: realtime() returns the offline module, which "
                          "filters every chunk on its own", stacklevel=2)
            return self
        return self.streaming()

    # -- self-test hooks (the reference's test file drives every class through them) with a filter that is not the
    # pass-through, so that the kernel runs --------------------------------------------------------------------------------
    def _selftest_co(self):
        return self._co if self._co is not None else _selftest_sos(self.sr)

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        y = self._run(x, self._selftest_co(), self.zero_phase)
        return y if time is None else (y, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(2, 2, 4101, generator=g) * 2 - 1).to("cuda")
        y = transform.test_forward(x)
        assert y.shape == x.shape and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert y.shape == x.shape and time.shape == (2, 2)
        if invert:
            z = transform.invert(y)
            assert z.shape == x.shape and bool(torch.isfinite(z).all())


class RealtimeSOSFilter(CarriedState, SOSFilter):
    """SOSFilter over a stream.  `forward` takes the next (..., C) chunk, any C >= 1, and returns (..., C); the sections'
    state after the chunk -- scipy's zf -- is carried in the float64 buffer `state` (lead..., n_sections, 2).  It is zeros
    on a new leading shape or device and after `reset()`, accepts any batch shape from a `state_dict`, and is taken back
    to float64 if a module cast (`.half()`, `.float()`) changed it.  The next state is written by the same launch into a
    fresh buffer that replaces the module's: no torch.cat, one launch per call.  `latency` is 0.

    Chunked outputs concatenate to the one-call result within rounding, not to the bit (module docstring).  Gradients
    (autograd.SosFilterStreamFunction): the carried state is a constant of the graph and is stored detached, so a chunk's
    gradient is the zero-state adjoint over that chunk -- truncated back-propagation at chunk boundaries, as for
    OverlapAdd, RealtimePQMF and RealtimeResample."""

    def __init__(self, sos=None, zero_phase: bool = False, sr: int = 44100):
        if zero_phase:
            raise ValueError("zero-phase filtering runs backwards over the whole signal: it has no streaming form")
        super().__init__(sos, False, sr)
        self.register_buffer("state", torch.zeros(self.n_sections, 2, dtype=torch.float64))
        self._carries("state")

    def _carried_tail(self, name: str) -> tuple:
        return (self.n_sections, 2)                          # of the coefficients in use: a state_dict may bring others

    @property
    def latency(self) -> int:
        return 0

    def streaming(self) -> "RealtimeSOSFilter":
        return self

    def realtime(self):
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim < 1:
            raise ValueError("RealtimeSOSFilter.forward takes a (..., C) chunk, got a scalar")
        if self._co is None:
            return x
        lead = tuple(x.shape[:-1])
        if x.numel() == 0:                                   # nothing arrived: no launch, the state stays
            ops._no_fp64(x)
            return torch.empty(x.shape, dtype=torch.float32, device=x.device)
        (zi,) = self._carried_rows(("state",), lead, x) or (None,)
        if zi is not None:
            zi = zi.reshape(lead + (self._co.n, 2))          # ops.sos_filter takes x, and so the state, with its leading shape
        if wants_grad(x):
            y, zf = SosFilterStreamFunction.apply(x, zi, self._co)
        else:
            y, zf = ops.sos_filter(x, self._co, zi=zi, return_state=True)
        self._carry("state", zf, lead)
        return y

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        stage = self if self._co is not None else RealtimeSOSFilter(self._selftest_co(), sr=self.sr)
        y = stage.forward(x)
        return y if time is None else (y, time)


class Preemphasis(SOSFilter):
    """y[n] = x[n] - coeff x[n - 1], the first-order high-pass in front of speech features, with x[-1] = 0.  `invert` is
    the de-emphasis y[n] = x[n] + coeff y[n - 1], a one-pole recursion through the same kernel (and the exact inverse up
    to rounding).  Both carry gradients.  ValueError for |coeff| >= 1, where the inverse is not stable."""
    invertible = True

    def __repr__(self):
        return "Preemphasis(coeff=%s)" % self.coeff

    def __init__(self, coeff: float = 0.97, sr: int = 44100):
        coeff = float(coeff)
        if not abs(coeff) < 1.0:
            raise ValueError("|coeff| must be < 1, got %r" % (coeff,))
        super().__init__([[1.0, -coeff, 0.0, 1.0, 0.0, 0.0]], False, sr)
        self._derive()

    def _derive(self) -> None:
        self.coeff = -float(self._co.array[0, 1])
        self._inverse = ops.sos_coefficients([[1.0, 0.0, 0.0, 1.0, -self.coeff, 0.0]])

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        out = super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._derive()
        return out

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        return self._run(x, self._inverse, False)

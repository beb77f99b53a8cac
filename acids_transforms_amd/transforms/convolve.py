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

Streaming: RealtimeImpulseResponse carries the last B input samples and, per stream, a ring of the spectra of the last
frames (a frequency-domain delay line) across chunks of whole blocks; block t of the result needs input blocks <= t only,
so the latency is 0 and any chunking concatenates to the offline result.  The sum over p is at_spectral_fir_stream, which
reads the P - 1 frames before the chunk from the ring and writes the chunk's frames into it in the same launch.

Not built: a direct time-domain kernel for short filters, time-varying filters, a non-uniform partition (low latency with
long responses), per-row responses in the streaming form, gradient through the carried state, second-order gradients.
"""
import math
import warnings
from typing import Optional

import torch
from torch import nn

from .. import ops
from .._lib import device_scoped, require_device
from ..autograd import FFTConvolveFunction, ImpulseResponseStreamFunction, wants_grad
from .base import AudioTransform, InversionEnumType, NotInvertibleError
from .carried import CarriedState

__all__ = ["FFTConvolve", "Convolve", "ImpulseResponse", "RealtimeImpulseResponse", "fftconvolve"]

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

    def streaming(self, block: Optional[int] = None) -> "RealtimeImpulseResponse":
        """The streaming form of this module: a RealtimeImpulseResponse that shares `ir` (buffer or Parameter).  It returns
        chunks of the chunk's own length, so `tail` does not carry over."""
        if self.passthrough:
            return RealtimeImpulseResponse(None, block=block, sr=self.sr)
        rt = RealtimeImpulseResponse(self.ir.detach().cpu(), block=block, learnable=self.learnable, sr=self.sr)
        if self.learnable:
            rt._parameters["ir"] = self.ir
        else:
            rt._buffers["ir"] = self.ir
        return rt.to(self.ir.device)

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


class RealtimeImpulseResponse(CarriedState, ImpulseResponse):
    """ImpulseResponse over a stream.  `forward` takes the next (..., C) chunk, C a positive multiple of the block B
    (`block`: ops.fft_convolve_stream_plan; None is the offline rule, 128 and 256 by request), and returns (..., C): the
    outputs of any chunking concatenate to fftconvolve(x_all, ir, "full", block=B)[..., :L].  `latency` is 0.

    State: `input_buffer` (lead..., B), the last B input samples; `spectrum_ring` (lead..., R, F) complex64, R = P - 1 + 8,
    the spectra of the last frames; `head`, the ring slot of the next frame, a host integer that is never read back from
    the device (no call synchronises) and travels through get_extra_state / set_extra_state.  State is zeros with head 0 on
    a new leading shape or device and after `reset()`, accepts any batch shape from a `state_dict`, and is stored detached.

    Per call, for every sub-chunk of at most 8 blocks: two copies into a staging buffer ([input_buffer | blocks]), one
    at_stft_forward, one at_spectral_fir_stream (which also updates the ring), one at_irfft_frames_streams and the copy of
    the last halves; one more copy per call keeps the new tail.  The spectrum of `ir` is cached per device and `ir._version`
    and rebuilt on every call while `ir` requires grad.

    Gradients (autograd.ImpulseResponseStreamFunction, first order): the carried state is a constant of the graph --
    truncated back-propagation at chunk boundaries, as for OverlapAdd and RealtimePQMF.  When `ir` requires grad the graph
    of a call keeps the chunk's frames and a copy of the P - 1 history frames, rows (P - 1) F 8 bytes.  A call where nothing
    requires grad is the plain route with the same bits."""

    def __repr__(self):
        return "RealtimeImpulseResponse(taps=%d, block=%d, learnable=%s)" % (self.taps, self.block, self.learnable)

    def __init__(self, ir=None, block: Optional[int] = None, learnable: bool = False, sr: int = 44100):
        super().__init__(ir, False, learnable, sr)
        self._block_arg = block
        self._plan()
        self.head = 0
        self._H = None                                           # ((device, ir._version, ir's address), H)
        self.register_buffer("input_buffer", torch.zeros(self.block))
        self.register_buffer("spectrum_ring", torch.zeros(self.ring_slots, self.block + 1, dtype=torch.complex64))
        self._carries("input_buffer", "spectrum_ring")

    def _plan(self) -> None:
        self.block, self.partitions, self.ring_slots, self.max_frames = ops.fft_convolve_stream_plan(self.taps, self._block_arg)

    @property
    def latency(self) -> int:
        return 0

    def get_extra_state(self):
        return {"head": int(self.head)}

    def set_extra_state(self, state) -> None:
        self.head = int(state["head"])

    def streaming(self, block: Optional[int] = None) -> "RealtimeImpulseResponse":
        return self

    def realtime(self):
        return self

    def _reset_extra(self) -> None:
        self.head = 0

    def _filter_spectrum(self, ir: torch.Tensor) -> torch.Tensor:
        """H (P, F) of `ir`, cached per device and ir._version; built anew on every call while ir requires grad."""
        key = (ir.device, ir._version, ir.data_ptr())
        if self._H is not None and self._H[0] == key and not ir.requires_grad:
            return self._H[1]
        H = ops._conv_filter_spectrum(ops._f32c(ir.detach()).reshape(1, -1), self.block, self.partitions)[0]
        self._H = (key, H)
        return H

    def _stream(self, x: torch.Tensor, ir: torch.Tensor) -> torch.Tensor:
        B = self.block
        if x.ndim < 1 or x.shape[-1] < B or x.shape[-1] % B:
            raise ValueError("RealtimeImpulseResponse.forward takes a (..., C) chunk with C a positive multiple of the block "
                             "%d, got shape %s" % (B, tuple(x.shape)))
        ops._no_fp64(x)
        ops._no_fp64(ir, "ir")
        device_scoped(require_device)(x, ir)
        lead, C = tuple(x.shape[:-1]), x.shape[-1]
        rows = math.prod(lead)
        if rows == 0:                                            # nothing arrived: no launch, the state stays
            return torch.empty(x.shape, dtype=torch.float32, device=x.device)
        R, F = self.ring_slots, B + 1
        state = self._carried_rows(("input_buffer", "spectrum_ring"), lead, x)      # the two are one stream
        if state is None:
            state = [torch.zeros(rows, B, dtype=torch.float32, device=x.device),
                     torch.zeros(rows, R, F, dtype=torch.complex64, device=x.device)]
            self.head = 0
        tail, ring = state                                       # the kernel updates the ring in place
        with torch.cuda.device(x.device):
            H = self._filter_spectrum(ir)
            x2 = x.reshape(rows, C)
            if wants_grad(x) or wants_grad(ir):
                y, new_tail = ImpulseResponseStreamFunction.apply(x2, ir, H, tail, ring, self.head, B)
            else:
                y, new_tail, _ = ops.fft_convolve_stream(x2, tail, ring, self.head, H, B)
        self.head = (self.head + C // B) % R
        self._carry("input_buffer", new_tail, lead)
        self._carry("spectrum_ring", ring, lead)
        return y.reshape(lead + (C,))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.passthrough:
            return x
        return self._stream(x, self.ir)

    # -- self-test hooks: audio cut to whole blocks, and the offline module's burst when this one is the pass-through ----------
    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        stage = self
        if self.passthrough:
            stage = RealtimeImpulseResponse(self._selftest_ir(x.device), block=self._block_arg, sr=self.sr).to(x.device)
        whole = x[..., :x.shape[-1] - x.shape[-1] % stage.block]
        y = stage.forward(whole) if whole.shape[-1] else whole           # less than one block: nothing to hand over yet
        return y if time is None else (y, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(2, 2, 4101, generator=g) * 2 - 1).to("cuda")
        y = transform.test_forward(x)
        assert y.shape[:-1] == x.shape[:-1] and 0 < y.shape[-1] <= 4101 and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert y.shape[:-1] == x.shape[:-1] and time.shape == (2, 2)

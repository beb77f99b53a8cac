"""PQMF: the pseudo-quadrature mirror filterbank of multiband waveform models (not in the reference package).

`forward` splits (..., L) audio into `n_band` critically sampled sub-band signals (..., n_band, L / n_band); `invert`
resynthesises (..., n_band, T) into (..., n_band * T) with the mirrored bank.  With M = n_band, N = taps (odd),
P = (N - 1) / 2 and a real low-pass prototype h:

    h_k[n]        = 2 h[n] cos((2k+1) pi / (2M) (n - P) + (-1)^k pi / 4)
    forward  y[k, t] = sum_n h_k[n] x[tM + n - P]                     = conv1d(x, h_k, stride=M, padding=P)
    invert   x^[m]   = M sum_k sum_t h_k[m + P - tM] y[k, t]          = M x the transpose of forward

with x zero outside [0, L).  The bank is centred and N is odd, so there is no delay.  Two HIP kernels (csrc/pqmf.hip)
serve forward, invert and both backward passes: synthesis is M x analysis transposed, so the backward of `forward` is
the synthesis kernel with scale 1 and the backward of `invert` the analysis kernel with scale M.  The kernels fold the
taps that share a modulation phase before they modulate: N / M + 2M multiply-adds per sample, not N.

The default prototype is a Kaiser-windowed sinc, designed on the host in float64:
h[n] = (w / pi) sinc(w (n - P) / pi) kaiser(N, beta), beta = 0.1102 (attenuation - 8.7), a symmetric window.  The cutoff
w is the first minimum over the 1025-point grid w_i = pi / (2M) (1 + i / 1024) of
phi(w) = max over l = 2M, 4M, ... < N of |sum_n h[n + l] h[n]| -- an exhaustive scan that assumes nothing about phi.

Reconstruction is NEAR perfect: `invert(forward(x))` differs from x by a relative rms of about 1e-3 (1.1e-3 at the
defaults, 1.0e-3 at n_band 4, taps 65, on white noise) on the samples at least N away from both ends -- the floor of
this design, the same in float64, not a kernel error -- and the first and last P samples are further affected by the
zero padding.

Gradients: `forward` and `invert` carry a gradient when grad mode is on and the input requires grad
(autograd.PqmfFunction / PqmfInvertFunction: the same kernels forward, the transposed kernel backward; the graph keeps
no tensor but the module's two buffers).  First order only.

Streaming: `RealtimePQMF` (also `PQMF.streaming()`) is the same bank made causal by a delay of D = ceil(P / M) whole
blocks in each direction, with the filter state carried in two module buffers:

    forward  chunk (..., C), C a multiple of M, down to one block -> (..., M, C / M); block t of the stream is
             y_ext[k, t - D], y_ext[k, t'] = sum_n h_k[n] x[t'M + n - P] with x zero before the stream's start, so the
             outputs of ANY chunking of x (..., L) concatenate to PQMF.forward(cat([zeros(D M), x], -1))[..., :L / M]
    invert   chunk (..., M, c), c >= 1 -> (..., c M); sample m of the stream is the offline synthesis sum at m - D M, so
             the outputs concatenate to PQMF.invert(cat([zeros(..., M, D), y], -1))[..., :T M]
    state    `input_buffer` (lead..., Ha), the last Ha = D M + P input samples; `band_buffer` (lead..., M, Hs), the last
             Hs = D + floor(P / M) blocks of every band (input history, not an output tail: every output stays one
             fmaf chain).  Zeros on a new leading batch shape or device and after `reset()`; float32 whatever a module
             cast (`.double()`, `.half()`) made of the buffers -- the rule of transforms.carried.CarriedState.

At the defaults (16 bands, 513 taps) D = 16, Ha = 512, Hs = 32: `analysis_delay` = `synthesis_delay` = 256 samples,
`latency` = 512 = taps - 1 for the round trip.  The kernels are the offline ones with another staging (a tile's window
comes from the state buffer, then the chunk, then zeros; csrc/pqmf.hip), so for finite input the chunked outputs are
the bits of the one-call result and of the delayed offline module.  (Finite only: the prototype's zero padding up to a
multiple of 2M multiplies samples that the stream has not received yet, which streaming reads as zeros.)  The new
state is written by the kernel into a second buffer that replaces the module's: no torch.cat, one launch per call.
Gradients (autograd.PqmfStreamFunction / PqmfStreamInvertFunction): the carried state is a constant of the graph and
is stored detached, so a chunk's gradient covers that chunk's own samples -- truncated back-propagation at chunk
boundaries, as for OverlapAdd.  The backward is the other kernel advanced by D blocks, without state.

`PQMF.realtime()` itself still warns and returns the offline module, which filters every chunk as a whole clip (zero
state at both chunk edges, so the P samples on either side of a chunk boundary differ from the offline result); it does
not raise, because the package's contract -- the reference's own suite, replayed on every transform -- is that
`realtime()` hands back a working module.  For the same reason the self-test hooks (`test_forward`, `test_inversion`,
`test_scripted_transform`) drop the last L % n_band samples of their audio, where `forward` itself raises.  Not built: a
hipGraph-captured streaming session (the state buffers change place every call), gradient flow through the carried
state, a fast DCT-IV modulation, bf16, optimised non-Kaiser prototypes."""
import math
import warnings
from typing import Optional, Union

import torch

from .. import ops
from .._lib import device_scoped, require_device
from ..autograd import PqmfFunction, PqmfInvertFunction, PqmfStreamFunction, PqmfStreamInvertFunction, wants_grad
from .base import AudioTransform
from .carried import CarriedState

__all__ = ["PQMF", "RealtimePQMF", "MIN_BANDS", "MAX_BANDS", "MAX_TAPS", "CUTOFF_GRID", "kaiser_prototype", "design_cutoff",
           "modulation_matrix"]

MIN_BANDS, MAX_BANDS, MAX_TAPS = 2, 64, 4097      # the range of the kernels (csrc/pqmf.hip)
CUTOFF_GRID = 1024                                # the cutoff is one of pi / (2M) (1 + i / CUTOFF_GRID), i = 0 .. CUTOFF_GRID


def _kaiser_beta(attenuation: float) -> float:
    return 0.1102 * (float(attenuation) - 8.7)


def kaiser_prototype(cutoff, taps: int, attenuation: float) -> torch.Tensor:
    """The Kaiser-windowed sinc low-pass of `taps` taps at the cutoff(s) `cutoff` (radians per sample; a float or a
    float64 tensor of any shape) -> float64 (..., taps)."""
    w = torch.as_tensor(cutoff, dtype=torch.float64)
    n = torch.arange(taps, dtype=torch.float64) - (taps - 1) // 2
    window = torch.kaiser_window(taps, periodic=False, beta=_kaiser_beta(attenuation), dtype=torch.float64)
    w = w.unsqueeze(-1)
    return (w / math.pi) * torch.sinc(w * n / math.pi) * window


def _phi(h: torch.Tensor, n_band: int) -> torch.Tensor:
    """max over the lags l = 2M, 4M, ... < N of |sum_n h[n + l] h[n]| for every prototype of h (..., N)."""
    N = h.shape[-1]
    worst = torch.zeros(h.shape[:-1], dtype=h.dtype)
    for lag in range(2 * n_band, N, 2 * n_band):
        worst = torch.maximum(worst, (h[..., lag:] * h[..., :N - lag]).sum(-1).abs())
    return worst


def design_cutoff(n_band: int, taps: int, attenuation: float) -> float:
    """The cutoff of the default prototype: the first argmin of phi over the whole grid (no bracketing search: phi is a
    maximum over lags and is not known to be unimodal between pi / 2M and pi / M)."""
    grid = math.pi / (2 * n_band) * (1.0 + torch.arange(CUTOFF_GRID + 1, dtype=torch.float64) / CUTOFF_GRID)
    phi = _phi(kaiser_prototype(grid, taps, attenuation), n_band)
    return float(grid[int(torch.argmin(phi))])


def modulation_matrix(n_band: int, taps: int) -> torch.Tensor:
    """C[k, r] = 2 cos((2k+1) pi / (2M) (r - P) + (-1)^k pi / 4), (M, 2M) float64."""
    k = torch.arange(n_band, dtype=torch.float64).unsqueeze(1)
    r = torch.arange(2 * n_band, dtype=torch.float64).unsqueeze(0)
    sign = 1.0 - 2.0 * (torch.arange(n_band) % 2).to(torch.float64).unsqueeze(1)
    return 2.0 * torch.cos((2 * k + 1) * math.pi / (2 * n_band) * (r - (taps - 1) // 2) + sign * math.pi / 4)


class PQMF(AudioTransform):
    invertible = True
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "PQMF(n_band=%s, taps=%s, cutoff=%s)" % (self.n_band, self.taps, self.cutoff)

    def __init__(self, n_band: int = 16, taps: Optional[int] = None, attenuation: float = 100.0,
                 prototype: Optional[torch.Tensor] = None, sr: int = 44100) -> None:
        super().__init__(sr=sr)
        n_band = int(n_band)
        if not MIN_BANDS <= n_band <= MAX_BANDS:
            raise ValueError("n_band must be in %d .. %d, got %d" % (MIN_BANDS, MAX_BANDS, n_band))
        if prototype is not None:
            prototype = torch.as_tensor(prototype)
            if prototype.ndim != 1:
                raise ValueError("prototype must be a 1-D tensor, got shape %s" % (tuple(prototype.shape),))
            taps = prototype.numel()
        elif taps is None:
            taps = 32 * n_band + 1
        taps = int(taps)
        if taps % 2 == 0:
            raise ValueError("taps must be odd (the bank is centred), got %d" % taps)
        if taps < 2 * n_band + 1:
            raise ValueError("taps must be at least 2 n_band + 1 = %d, got %d" % (2 * n_band + 1, taps))
        if taps > MAX_TAPS:
            raise ValueError("taps must be at most %d, got %d" % (MAX_TAPS, taps))
        self.n_band, self.taps, self.attenuation = n_band, taps, float(attenuation)
        if prototype is not None:
            self.cutoff = None
            h = prototype.detach().to("cpu", torch.float64)
        else:
            self.cutoff = design_cutoff(n_band, taps, attenuation)
            h = kaiser_prototype(self.cutoff, taps, attenuation)
        self.register_buffer("prototype", h.to(torch.float32).contiguous())
        self.register_buffer("modulation", modulation_matrix(n_band, taps).to(torch.float32).contiguous())

    @property
    def ratio(self):
        return self.n_band

    def realtime(self):
        warnings.warn("PQMF has no streaming form of its own: realtime() returns the offline module, which filters every "
                      "chunk as a whole clip with zero state at its edges; RealtimePQMF (or PQMF.streaming()) carries "
                      "the filter state across chunks", stacklevel=2)
        return self

    def streaming(self) -> "RealtimePQMF":
        """The streaming form of this bank: a RealtimePQMF that shares this module's prototype and modulation."""
        rt = RealtimePQMF(n_band=self.n_band, attenuation=self.attenuation, prototype=self.prototype, sr=self.sr)
        rt.cutoff = self.cutoff
        rt._buffers["prototype"], rt._buffers["modulation"] = self.prototype, self.modulation
        return rt.to(self.prototype.device)

    # the self-test hooks of the base class, on audio cut to a whole number of blocks (forward raises otherwise)
    def _whole_blocks(self, x: torch.Tensor) -> torch.Tensor:
        return x[..., :x.shape[-1] - x.shape[-1] % self.n_band]

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        return super().test_forward(self._whole_blocks(x), time)

    def test_inversion(self, x: torch.Tensor):
        return super().test_inversion(self._whole_blocks(x))

    @classmethod
    def test_scripted_transform(cls, transform, batch_size=(2, 2), invert=True):
        x = torch.zeros(*batch_size, 44100 - 44100 % transform.n_band, device="cuda")
        x_t = transform.forward(x)
        x_t, _ = transform.forward_with_time(x, torch.zeros(*batch_size, device="cuda"))
        if invert:
            transform.invert(x_t)

    def _tables(self, x):
        """The two buffers as the kernels read them, on x's device (the module follows its input)."""
        if self.prototype.device != x.device:
            self.to(x.device)
        proto, mod = self.prototype, self.modulation
        if proto.dtype != torch.float32 or not proto.is_contiguous():      # after module.double() / .half()
            proto = proto.float().contiguous()
        if mod.dtype != torch.float32 or not mod.is_contiguous():
            mod = mod.float().contiguous()
        return proto, mod

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim < 1 or x.shape[-1] % self.n_band:
            raise ValueError("PQMF.forward takes (..., L) audio with L a multiple of n_band = %d, got shape %s"
                             % (self.n_band, tuple(x.shape)))
        ops._no_fp64(x)
        device_scoped(require_device)(x)
        proto, mod = self._tables(x)
        lead, L = tuple(x.shape[:-1]), x.shape[-1]
        x2 = x.reshape(math.prod(lead), L)                     # torch's own ops: a gradient reaches the caller's tensor
        if wants_grad(x):
            y = PqmfFunction.apply(x2, proto, mod)
        else:
            y = ops.pqmf_analysis(x2, proto, mod, 1.0)
        return y.reshape(lead + (self.n_band, L // self.n_band))

    def invert(self, x: torch.Tensor, inversion_mode: Union[str, None] = None, **kwargs) -> torch.Tensor:
        if x.ndim < 2 or x.shape[-2] != self.n_band:
            raise ValueError("PQMF.invert takes (..., n_band = %d, T) sub-band signals, got shape %s"
                             % (self.n_band, tuple(x.shape)))
        ops._no_fp64(x)
        device_scoped(require_device)(x)
        proto, mod = self._tables(x)
        lead, T = tuple(x.shape[:-2]), x.shape[-1]
        y3 = x.reshape((math.prod(lead), self.n_band, T))
        if wants_grad(x):
            out = PqmfInvertFunction.apply(y3, proto, mod)
        else:
            out = ops.pqmf_synthesis(y3, proto, mod, float(self.n_band))
        return out.reshape(lead + (self.n_band * T,))


class RealtimePQMF(CarriedState, PQMF):
    """The causal PQMF with carried filter state (the module docstring): `forward` and `invert` take the next chunk of
    a stream and answer the offline bank delayed by `analysis_delay` / `synthesis_delay` samples."""

    def __repr__(self):
        return "Realtime" + super().__repr__()

    def __init__(self, n_band: int = 16, taps: Optional[int] = None, attenuation: float = 100.0,
                 prototype: Optional[torch.Tensor] = None, sr: int = 44100) -> None:
        super().__init__(n_band=n_band, taps=taps, attenuation=attenuation, prototype=prototype, sr=sr)
        self.delay_blocks, self._keep_in, self._keep_band = ops.pqmf_stream_sizes(self.n_band, self.taps)
        self.register_buffer("input_buffer", torch.zeros(self._keep_in))
        self.register_buffer("band_buffer", torch.zeros(self.n_band, self._keep_band))
        self._carries("input_buffer", "band_buffer")

    @property
    def analysis_delay(self) -> int:
        """Samples by which `forward` lags the offline bank."""
        return self.delay_blocks * self.n_band

    @property
    def synthesis_delay(self) -> int:
        """Samples by which `invert` lags the offline bank."""
        return self.delay_blocks * self.n_band

    @property
    def latency(self) -> int:
        """Samples by which invert(forward(x)) lags x."""
        return self.analysis_delay + self.synthesis_delay

    def realtime(self):
        return self

    def streaming(self) -> "RealtimePQMF":
        return self

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time - self.analysis_delay / self.sr

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim < 1 or x.shape[-1] % self.n_band:
            raise ValueError("RealtimePQMF.forward takes a (..., C) chunk with C a multiple of n_band = %d, got shape %s"
                             % (self.n_band, tuple(x.shape)))
        ops._no_fp64(x)
        device_scoped(require_device)(x)
        lead, C = tuple(x.shape[:-1]), x.shape[-1]
        if x.numel() == 0:                                      # nothing arrived: no launch, the state stays
            return torch.empty(lead + (self.n_band, C // self.n_band), dtype=torch.float32, device=x.device)
        (state,) = self._carried_rows(("input_buffer",), lead, x) or (None,)      # forward and invert: separate streams
        proto, mod = self._tables(x)
        x2 = x.reshape(math.prod(lead), C)
        if wants_grad(x):
            y, new_state = PqmfStreamFunction.apply(x2, state, proto, mod)      # the state is a constant of the graph
        else:
            y, new_state = ops.pqmf_analysis_stream(x2, state, proto, mod, 1.0)
        self._carry("input_buffer", new_state, lead)
        return y.reshape(lead + (self.n_band, C // self.n_band))

    def invert(self, x: torch.Tensor, inversion_mode: Union[str, None] = None, **kwargs) -> torch.Tensor:
        if x.ndim < 2 or x.shape[-2] != self.n_band:
            raise ValueError("RealtimePQMF.invert takes a (..., n_band = %d, c) chunk of sub-band signals, got shape %s"
                             % (self.n_band, tuple(x.shape)))
        ops._no_fp64(x)
        device_scoped(require_device)(x)
        lead, c = tuple(x.shape[:-2]), x.shape[-1]
        if x.numel() == 0:
            return torch.empty(lead + (self.n_band * c,), dtype=torch.float32, device=x.device)
        (state,) = self._carried_rows(("band_buffer",), lead, x) or (None,)
        proto, mod = self._tables(x)
        y3 = x.reshape((math.prod(lead), self.n_band, c))
        if wants_grad(x):
            out, new_state = PqmfStreamInvertFunction.apply(y3, state, proto, mod)
        else:
            out, new_state = ops.pqmf_synthesis_stream(y3, state, proto, mod, float(self.n_band))
        self._carry("band_buffer", new_state, lead)
        return out.reshape(lead + (self.n_band * c,))

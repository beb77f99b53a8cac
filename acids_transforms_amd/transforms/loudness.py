"""Loudness and LoudnessNormalize: programme loudness of ITU-R BS.1770-4 / EBU R128 (torchaudio.transforms.Loudness and
pyloudnorm measure the same thing; not in the reference package).

    hop H = round(sr / 10) samples (100 ms), a block = hb hops, nh = L // H whole hops, nb = nh - hb + 1
    y_c     = sosfilt(k_weighting(sr), x_c)                        from zero state
    s[c][h] = sum over hop h of y_c[n]^2
    p_j     = sum_c G_c (s[c][j] + ... + s[c][j + hb - 1]) / (hb H),    l_j = -0.691 + 10 log10 p_j
    integrated (hb = 4):  J1 = {j: p_j > 10^((-70 + 0.691) / 10)},  J2 = {j in J1: p_j > mean_J1(p) / 10},
                          loudness = -0.691 + 10 log10 mean_J2(p),   -inf when J1 is empty

The input is (..., C, L) float32 with the channel axis at -2 (a 1-D tensor is one mono clip); the channel weights G default
to (1, 1, 1, 1.41, 1.41)[:C] -- left, right, centre, the two surrounds; an LFE channel is left out by the caller.  The
samples past nh H belong to no block.

Two launches: sos_filter.hip's walk with the hop-power ending squares the K-weighted samples in double, in registers, before
they are rounded, and sums them per hop -- the filtered signal is never written -- and loudness.hip gates the (..., C, nh)
float64 powers.  The gates compare powers against thresholds computed on the host in double; no logarithm decides one.  A
clip's bits do not depend on the batch it rides in.  A NaN in a clip makes that clip NaN and no other.

Gradients: a call whose input requires grad (with grad mode on) goes through autograd.LoudnessFunction /
LoudnessBlocksFunction, every other call is the plain route with the same bits.  The gates are piecewise constant, so
they are constants of the graph; a clip that reads -inf has an exactly zero gradient; a silent BLOCK passes nothing back
from `momentary` / `short_term`.  The channel weights are constants of the graph.  First order only.

The pre-filter is utils.filter_design.k_weighting: the standard's own table at 48 kHz (to 9e-16), and the same analogue
prototypes through the bilinear transform at every other rate.  torchaudio approximates it with cookbook biquads instead,
so the two differ by that approximation; parity with torchaudio is unpinned.

Loudness range (EBU Tech 3342, `Loudness.loudness_range`): the same hop powers, 3 s blocks one hop apart, the absolute gate,
a relative gate 20 LU below the mean of what passed it, and 10 log10 of the ratio of two order statistics of the n gated
block powers q in ascending order, q[rnd(0.95 (n - 1))] / q[rnd(0.10 (n - 1))] with rnd(v) = floor(v + 0.5) -- Tech 3342's own
index rule.  The two are picked by an exact radix select in loudness.hip (no sort), a function of the clip's hop powers
alone.  It has no graph.

Streaming: RealtimeLoudness (also `Loudness.streaming()`) is the meter over a stream of chunks of any length >= 1.  It
carries the K-weighting filter's state, the partial sum of the open hop and every whole hop's power since the stream began,
all float64, and the number of samples seen as a host integer; no call synchronises and nothing of the audio is kept.  A
`forward` is two launches -- sos_filter.hip's stream ending writes the hops that complete straight into the history, and
loudness.hip's gate reads the window of history the new blocks cover where it lies -- or one when no block completes.  The
kernel's tile grid starts at each chunk's first sample, so a chunked stream's hop powers agree with the one-call
measurement WITHIN ROUNDING (1e-5 normwise, 1e-4 LU), not to the bit; the same chunking gives the same bits in any batch.

True peak (`TruePeak`, `RealtimeTruePeak`, `LoudnessNormalize(peak_limit=...)`): R128's fourth figure, ITU-R BS.1770-4 Annex 2.
With a polyphase table h of P phases (the oversampling factor) and K taps per phase, and x[n] = 0 for n < 0,
    y[P n + p] = sum over k = 0 .. K - 1 ascending of h[p][k] x[n - k],    peak = max_m |y[m]|,    dBTP = 20 log10 peak
-- causal, with no flush past the last sample, so a stream of the same samples gives the same values, and the filter's delay
does not move a maximum.  The default table is the standard's own 4 x 12 (utils.filter_design.true_peak_filter); at 96 kHz
and above a 2 x 12 Kaiser design, at 192 kHz and above the sample peak, as the standard allows.  On the five true-peak
signals of EBU Tech 3341 (cases 15 to 19), each with a 480-sample raised-cosine fade-in, it reads -6.218, -5.976, -6.316,
-6.028 and +3.029 dBTP, inside Tech 3341's +0.2 / -0.4 dB; WITHOUT the fade the abrupt onset of case 18 overshoots to -5.32
dBTP -- a property of the signal's step, which has energy above its nominal frequency, not of the meter.  true_peak.hip
reads each sample once and writes one number per row: every y[m] is one fmaf chain in k ascending and the reduction is an
exact integer maximum of |y|'s bits with the smallest index, so a row's bits depend on neither the batch nor the tiling nor
the chunking: RealtimeTruePeak equals the one-call measurement TO THE BIT.  One launch where a row fits a tile of 2048
samples, else two; the dBTP reading is a torch expression on the (..., C) peaks.  A NaN in a row makes that row NaN and no
other; +-inf reads +inf; silence -inf.  Gradient (autograd.TruePeakFunction): the subgradient at the attained maximum, K taps
under one index; a silent row gets exactly +0.

Not built: a true-peak limiter with look-ahead gain smoothing, a per-hop true-peak envelope, true peak inside
RealtimeLoudness (compose the two meters), the oversampled signal itself, gradients through RealtimeTruePeak, a
hipGraph-captured session, a bounded-memory (histogram) form of the integrated measure for streams of days (the history grows
by one float64 per channel per 100 ms), gradients through the streaming meter or the loudness range, bit-equal chunking, a
row-splitting dispatch for one very long row (a row is one workgroup, as for SOSFilter), gradients with respect to the
channel weights, torchaudio's approximate pre-filter, second-order gradients.  `Loudness.realtime()` still warns and returns
the offline module (the reference's protocol drives `realtime()` with whole clips); the streaming form is `streaming()`.
"""
import warnings
from typing import Optional

import torch

from .. import ops
from .._lib import device_scoped, require_device
from ..autograd import LoudnessBlocksFunction, LoudnessFunction, TruePeakFunction, dbtp, wants_grad
from ..utils.filter_design import true_peak_filter
from .base import AudioTransform, InversionEnumType, NotInvertibleError
from .carried import CarriedState

__all__ = ["Loudness", "LoudnessNormalize", "RealtimeLoudness", "TruePeak", "RealtimeTruePeak"]


class Loudness(AudioTransform):
    """(..., C, L) -> (...,) integrated loudness in LUFS.  `momentary(x)` and `short_term(x)` give the ungated loudness of
    every 400 ms / 3 s block, (..., nb), one per 100 ms.  ValueError: more than five channels without `channel_weights`
    (also what a (batch, L) tensor runs into: give it a channel axis), weights that do not match the channels, a clip
    shorter than one block, a sample rate below k_weighting's limit."""
    invertible = False
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "%s(sr=%s, channel_weights=%s)" % (type(self).__name__, self.sr, self.channel_weights)

    def __init__(self, sr: int = 44100, channel_weights=None):
        super().__init__(sr=sr)
        self.channel_weights = None if channel_weights is None else tuple(float(g) for g in channel_weights)
        ops.loudness_plan((1, ops.LOUDNESS_BLOCK_HOPS * int(round(float(sr) / 10.0))), sr)     # the rate's own check

    def _blocks(self, x: torch.Tensor, hops_per_block: int) -> torch.Tensor:
        if wants_grad(x):
            return LoudnessBlocksFunction.apply(x, self.sr, hops_per_block, self.channel_weights)
        return ops.loudness_blocks(x, self.sr, hops_per_block, self.channel_weights)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if wants_grad(x):
            return LoudnessFunction.apply(x, self.sr, self.channel_weights)
        return ops.loudness(x, self.sr, self.channel_weights)

    def momentary(self, x: torch.Tensor) -> torch.Tensor:
        return self._blocks(x, ops.LOUDNESS_BLOCK_HOPS)

    def short_term(self, x: torch.Tensor) -> torch.Tensor:
        return self._blocks(x, ops.LOUDNESS_SHORT_TERM_HOPS)

    def loudness_range(self, x: torch.Tensor) -> torch.Tensor:
        """(..., C, L) -> (...,) loudness range (EBU Tech 3342) in LU.  ValueError below one 3 s block.  No graph: an
        input that requires grad gets a tensor without one."""
        return ops.loudness_range(x.detach(), self.sr, self.channel_weights)

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

    def streaming(self) -> "RealtimeLoudness":
        """The streaming meter of this measure: a RealtimeLoudness with the same rate and channel weights."""
        return RealtimeLoudness(sr=self.sr, channel_weights=self.channel_weights)

    def realtime(self):
        warnings.warn("%s has no streaming form (a streaming meter is not built): realtime() returns the offline module, "
                      "which measures every chunk on its own" % type(self).__name__, stacklevel=2)
        return self

    # -- self-test hooks (the reference's test file drives every class through them) --------------------------------------
    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        return self.forward(x) if time is None else self.forward_with_time(x, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        L = 5 * int(round(float(transform.sr) / 10.0)) + 7
        x = (0.1 * torch.randn(2, 2, L, generator=g)).to("cuda")
        y = transform.test_forward(x)
        assert y.shape[:1] == (2,) and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert bool(torch.isfinite(y).all()) and time.shape == (2, 2)
        if invert:
            transform.invert(y)


class LoudnessNormalize(Loudness):
    """(..., C, L) -> (..., C, L): every clip scaled to `target` LUFS, x 10^((target - Loudness(x)) / 20).  A clip whose
    loudness is -inf (nothing above the absolute gate) keeps gain 1.  The multiply is a torch expression, as the channel
    stages are, so gradients flow through both factors; `detach_gain=True` makes the gain a constant of the graph (the
    usual choice for augmentation).  Not invertible: the gain is not kept.

    `peak_limit` (dBTP, e.g. -1.0; None: no limit, the code path and the bits without the argument): the gain becomes
    min(loudness gain, 10^((peak_limit - programme true peak) / 20)) -- scaling is linear, so one measurement of the clip's
    true peak (a TruePeak of the same rate, over all channels) suffices -- and a quiet, peaky clip ends at the limit instead
    of over full scale.  `detach_gain` covers both factors."""

    def __repr__(self):
        limit = "" if self.peak_limit is None else ", peak_limit=%s" % self.peak_limit
        return "LoudnessNormalize(target=%s, sr=%s, channel_weights=%s, detach_gain=%s%s)" % (
            self.target, self.sr, self.channel_weights, self.detach_gain, limit)

    def __init__(self, target: float = -23.0, sr: int = 44100, channel_weights=None, detach_gain: bool = False,
                 peak_limit: Optional[float] = None):
        super().__init__(sr=sr, channel_weights=channel_weights)
        self.target, self.detach_gain = float(target), bool(detach_gain)
        if not self.target == self.target or self.target in (float("inf"), float("-inf")):
            raise ValueError("target must be a finite loudness in LUFS, got %r" % (target,))
        self.peak_limit = None if peak_limit is None else float(peak_limit)
        if self.peak_limit is not None:
            if not self.peak_limit == self.peak_limit or self.peak_limit in (float("inf"), float("-inf")):
                raise ValueError("peak_limit must be a finite level in dBTP or None, got %r" % (peak_limit,))
            self.true_peak = TruePeak(sr=sr)

    def gain(self, x: torch.Tensor) -> torch.Tensor:
        """The linear gain per clip, (...,)."""
        lufs = Loudness.forward(self, x.detach() if self.detach_gain else x)
        gain = torch.pow(10.0, (self.target - lufs) / 20.0)
        gain = torch.where(torch.isinf(lufs), torch.ones_like(gain), gain)
        if self.peak_limit is None:
            return gain
        dbtp_now = self.true_peak.programme(x.detach() if self.detach_gain else x)
        return torch.minimum(gain, torch.pow(10.0, (self.peak_limit - dbtp_now) / 20.0))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        gain = self.gain(x)
        return x * (gain if x.ndim == 1 else gain[..., None, None])

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        return self.forward(x) if time is None else self.forward_with_time(x, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        L = 5 * int(round(float(transform.sr) / 10.0)) + 7
        x = (0.1 * torch.randn(2, 2, L, generator=g)).to("cuda")
        y = transform.test_forward(x)
        assert y.shape == x.shape and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert y.shape == x.shape and time.shape == (2, 2)
        if invert:
            transform.invert(y)


class RealtimeLoudness(CarriedState, Loudness):
    """An EBU R128 meter over a stream.  `forward` takes the next (..., C, n) chunk, any n >= 1 (a 1-D chunk is one mono
    stream), and returns (..., k) float32: the momentary loudness in LUFS of the k 400 ms blocks that completed in this
    chunk, k = max(0, hops_after - 3) - max(0, hops_before - 3), empty when k is 0 -- the outputs of any chunking
    concatenate to `Loudness.momentary` of the whole signal (within rounding: module docstring).  `momentary()` and
    `short_term()` give (...,), the latest 400 ms / 3 s block, -inf before the first is complete; `integrated()` the gated
    loudness of everything since the stream began (-inf before the first block); `block_loudness(hops_per_block)` every
    block so far, (..., nb); `loudness_range()` the range in LU, 0 before the first 3 s block.

    Carried, all float64 whatever `.half()` did to the module: `filter_state` (lead..., C, 2, 2), the K-weighting filter's
    state; `open_power` (lead..., C), the partial sum of the open hop; `hop_power` (lead..., C, cap), every whole hop since
    the stream began, cap = 1024 doubled by a copy when the host count says it is full.  `samples_seen`, a host integer that
    is never read back from the device, gives the hop count and where the next chunk falls, and travels through
    get_extra_state / set_extra_state.  Zeros and 0 on a new leading shape (lead..., C) or device and after `reset()`; any
    batch shape from a `state_dict`.  A call is two launches (one when no block completes), updates the state in place and
    allocates nothing but its result, except where a chunk is not float32 and contiguous or the history grows.  `latency`
    is 0.  The outputs carry no graph: it is a meter, the offline Loudness keeps its gradient."""

    def __repr__(self):
        return "RealtimeLoudness(sr=%s, channel_weights=%s)" % (self.sr, self.channel_weights)

    def __init__(self, sr: int = 44100, channel_weights=None, _cap: int = 1024):
        super().__init__(sr=sr, channel_weights=channel_weights)
        self._cap0 = int(_cap)
        self._kw = ops._k_weighting(sr)
        self.samples_seen = 0
        self.register_buffer("filter_state", torch.zeros(self._kw.n, 2, dtype=torch.float64))
        self.register_buffer("open_power", torch.zeros((), dtype=torch.float64))
        self.register_buffer("hop_power", torch.zeros(self._cap0, dtype=torch.float64))
        self._carries("filter_state", "open_power", "hop_power")

    _STATE = ("filter_state", "open_power", "hop_power")

    def _carried_tail(self, name: str) -> tuple:
        if name == "hop_power":
            return (self.hop_power.shape[-1],)               # of what it holds now: the history grows
        return self._carried[name][0]

    def get_extra_state(self):
        return {"samples_seen": int(self.samples_seen)}

    def set_extra_state(self, state) -> None:
        self.samples_seen = int(state["samples_seen"])

    def _reset_extra(self) -> None:
        self.samples_seen = 0

    @property
    def latency(self) -> int:
        return 0

    @property
    def hops(self) -> int:
        """Whole hops since the stream began."""
        return self.samples_seen // int(round(float(self.sr) / 10.0))

    def streaming(self) -> "RealtimeLoudness":
        return self

    def realtime(self):
        return self

    def _stream(self, lead, x: torch.Tensor) -> None:
        """Makes the buffers those of the stream of x: zeros, and no sample seen, on a new leading shape or device; float64
        and contiguous."""
        rows = self._carried_rows(self._STATE, lead, x)
        if rows is None:
            ops.loudness_plan(lead[-1:] + (1 << 30,), self.sr, ops.LOUDNESS_BLOCK_HOPS, self.channel_weights)    # the channels
            self.samples_seen = 0
            for k in self._STATE:
                tail = (self._cap0,) if k == "hop_power" else self._carried[k][0]
                setattr(self, k, torch.zeros(lead + tail, dtype=torch.float64, device=x.device))
        else:
            for k, r in zip(self._STATE, rows):              # what a module cast or a strided state_dict entry changed
                if r.data_ptr() != self._buffers[k].data_ptr() or self._buffers[k].dtype != torch.float64:
                    self._carry(k, r, lead)

    def _room(self, need: int) -> None:
        """Room for `need` hops in the history: doubled by a copy when the host count says it is full."""
        cap = self.hop_power.shape[-1]
        if need > cap:
            while cap < need:
                cap *= 2
            grown = torch.zeros(tuple(self.hop_power.shape[:-1]) + (cap,), dtype=torch.float64, device=self.hop_power.device)
            grown[..., :self.hop_power.shape[-1]] = self.hop_power
            self.hop_power = grown

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim < 1:
            raise ValueError("RealtimeLoudness.forward takes a (..., C, n) chunk, got a scalar")
        ops._no_fp64(x)
        x = x.detach()
        if x.ndim == 1:
            x = x[None]
        lead, n = tuple(x.shape[:-1]), x.shape[-1]
        if n == 0:                                           # nothing arrived: no launch, the state stays
            return torch.empty(lead[:-1] + (0,), dtype=torch.float32, device=x.device)
        device_scoped(require_device)(x)                     # before any state is touched: there is no CPU route
        self._stream(lead, x)
        hop, filled, first, done, k = ops.loudness_stream_plan(self.sr, self.samples_seen, n)
        self._room(first + done)
        ops.sos_hop_power_stream(x, self._kw, hop, filled, self.filter_state, self.open_power, self.hop_power, first)
        self.samples_seen += n
        if k == 0:
            return torch.empty(lead[:-1] + (0,), dtype=torch.float32, device=x.device)
        j0 = max(0, first - (ops.LOUDNESS_BLOCK_HOPS - 1))   # the first new block, and the first hop it reads
        return ops.loudness_gate_window(self.hop_power, lead[-1], j0, first + done - j0, self.sr, ops.LOUDNESS_BLOCK_HOPS,
                                        self.channel_weights)

    def _no_stream(self, fill: float, tail=()) -> Optional[torch.Tensor]:
        if self.hop_power.ndim < 2:                          # no chunk yet: no batch shape either
            return torch.full(tuple(tail), fill, dtype=torch.float32, device=self.hop_power.device)
        return None

    def _history(self) -> torch.Tensor:
        h = self.hop_power
        return h if h.dtype == torch.float64 and h.is_contiguous() else h.double().contiguous()

    def block_loudness(self, hops_per_block: int = ops.LOUDNESS_BLOCK_HOPS) -> torch.Tensor:
        """(..., nb) float32: the ungated loudness of every block of `hops_per_block` hops so far, one per 100 ms."""
        early = self._no_stream(0.0, (0,))
        if early is not None:
            return early
        return ops.loudness_gate_window(self._history(), self.hop_power.shape[-2], 0, self.hops, self.sr, hops_per_block,
                                        self.channel_weights)

    def _latest(self, hb: int) -> torch.Tensor:
        early = self._no_stream(float("-inf"))
        if early is not None:
            return early
        if self.hops < hb:
            return torch.full(tuple(self.hop_power.shape[:-2]), float("-inf"), dtype=torch.float32, device=self.hop_power.device)
        return ops.loudness_gate_window(self._history(), self.hop_power.shape[-2], self.hops - hb, hb, self.sr, hb,
                                        self.channel_weights)[..., 0]

    def momentary(self) -> torch.Tensor:
        return self._latest(ops.LOUDNESS_BLOCK_HOPS)

    def short_term(self) -> torch.Tensor:
        return self._latest(ops.LOUDNESS_SHORT_TERM_HOPS)

    def integrated(self) -> torch.Tensor:
        """(...,) float32: the gated loudness (BS.1770) of everything since the stream began; -inf before the first block."""
        early = self._no_stream(float("-inf"))
        if early is not None:
            return early
        return ops.loudness_gate_window(self._history(), self.hop_power.shape[-2], 0, self.hops, self.sr,
                                        ops.LOUDNESS_BLOCK_HOPS, self.channel_weights, gated=True)

    def loudness_range(self) -> torch.Tensor:
        """(...,) float32: the loudness range (EBU Tech 3342) in LU of everything so far; 0 before the first 3 s block."""
        early = self._no_stream(0.0)
        if early is not None:
            return early
        if self.hops < ops.LOUDNESS_SHORT_TERM_HOPS:
            return torch.zeros(tuple(self.hop_power.shape[:-2]), dtype=torch.float32, device=self.hop_power.device)
        return ops.loudness_range_from_power(self._history(), self.hops, self.sr, self.channel_weights)

    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        return self.forward(x) if time is None else self.forward_with_time(x, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        H = int(round(float(transform.sr) / 10.0))
        x = (0.1 * torch.randn(2, 2, 5 * H + 7, generator=g)).to("cuda")
        transform.reset()
        y = transform.test_forward(x)
        assert y.shape == (2, 2) and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert y.shape == (2, 5) and bool(torch.isfinite(y).all()) and time.shape == (2, 2)
        assert bool(torch.isfinite(transform.integrated()).all()) and transform.loudness_range().shape == (2,)
        if invert:
            transform.invert(y)


def _true_peak_table(sr, oversample, taps) -> torch.Tensor:
    """The (P, K) float32 table of a meter: `taps` as given, else by `oversample` (None: 4 below 96 kHz, 2 below 192 kHz, 1
    above) -- 4: the table of BS.1770-4 Annex 2; 2 and 8: the Kaiser design with 12 taps per phase; 1: the sample peak.
    Designed in float64 and rounded once, here."""
    if taps is not None:
        table = torch.as_tensor(taps).detach().to("cpu", torch.float64)
        if table.ndim != 2 or not (1 <= table.shape[0] <= ops.TRUE_PEAK_MAX_PHASES and 1 <= table.shape[1] <= ops.TRUE_PEAK_MAX_TAPS):
            raise ValueError("taps must be a (phases <= %d, taps per phase <= %d) table, got shape %s"
                             % (ops.TRUE_PEAK_MAX_PHASES, ops.TRUE_PEAK_MAX_TAPS, tuple(table.shape)))
        if not bool(torch.isfinite(table).all()):
            raise ValueError("taps has non-finite entries")
        return table.float().contiguous()
    if oversample is None:
        oversample = 4 if float(sr) < 96000.0 else (2 if float(sr) < 192000.0 else 1)
    if oversample == 1:
        return torch.ones(1, 1)
    if oversample == 4:
        return torch.from_numpy(true_peak_filter(4, 12, "bs1770")).float()
    if oversample in (2, 8):
        return torch.from_numpy(true_peak_filter(int(oversample), 12, "kaiser")).float()
    raise ValueError("oversample must be 1, 2, 4, 8 or None, got %r" % (oversample,))


class TruePeak(AudioTransform):
    """(..., C, L) -> (..., C) maximum true peak in dBTP (module docstring); a 1-D tensor is one mono clip and reads a
    scalar.  `linear(x)` gives the linear peak, `programme(x)` (...,) the maximum over the channels in dBTP, `sample_peak(x)`
    the same reading through the identity table (dBFS of the largest sample), `index(x)` the oversampled index P n + p of
    the maximum, int64.  Silence reads -inf.  `taps` is a (P, K) table instead of the built-in ones, P <= 8, K <= 64; the
    buffer `taps` is float32.  ValueError: a scalar input, an `oversample` outside {1, 2, 4, 8}, a malformed table.  Not
    invertible.  A call whose input requires grad goes through autograd.TruePeakFunction, every other call is the plain
    route with the same bits; `index` has no graph."""
    invertible = False
    scriptable = False
    needs_scaling = False

    def __repr__(self):
        return "%s(sr=%s, oversample=%d, taps_per_phase=%d)" % (type(self).__name__, self.sr, self.taps.shape[0], self.taps.shape[1])

    def __init__(self, sr: int = 44100, oversample: Optional[int] = None, taps=None):
        super().__init__(sr=sr)
        self.register_buffer("taps", _true_peak_table(sr, oversample, taps))
        self.register_buffer("_identity", torch.ones(1, 1), persistent=False)

    @property
    def oversample(self) -> int:
        return int(self.taps.shape[0])

    def _measure(self, x: torch.Tensor, taps: torch.Tensor, db: bool) -> torch.Tensor:
        if x.ndim < 1:
            raise ValueError("%s takes (..., C, L), got a scalar" % type(self).__name__)
        if wants_grad(x):
            return TruePeakFunction.apply(x, taps, db)
        peak = ops.true_peak(x, taps)
        return dbtp(peak) if db else peak

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._measure(x, self.taps, True)

    def linear(self, x: torch.Tensor) -> torch.Tensor:
        return self._measure(x, self.taps, False)

    def programme(self, x: torch.Tensor) -> torch.Tensor:
        y = self.forward(x)
        return y if y.ndim == 0 else y.amax(dim=-1)

    def sample_peak(self, x: torch.Tensor) -> torch.Tensor:
        return self._measure(x, self._identity, True)

    def index(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim < 1:
            raise ValueError("%s takes (..., C, L), got a scalar" % type(self).__name__)
        return ops.true_peak(x.detach(), self.taps, return_state=True)[1]

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

    def streaming(self) -> "RealtimeTruePeak":
        """The streaming meter of this measure: a RealtimeTruePeak with the same rate and table."""
        return RealtimeTruePeak(sr=self.sr, taps=self.taps)

    def realtime(self):
        return self.streaming()                              # chunk-safe, unlike Loudness.realtime()

    # -- self-test hooks (the reference's test file drives every class through them) --------------------------------------
    def test_forward(self, x: torch.Tensor, time: Optional[torch.Tensor] = None):
        return self.forward(x) if time is None else self.forward_with_time(x, time)

    @classmethod
    def test_scripted_transform(cls, transform, invert: bool = True):
        g = torch.Generator().manual_seed(0)
        x = (0.1 * torch.randn(2, 2, 4103, generator=g)).to("cuda")
        if isinstance(transform, CarriedState):
            transform.reset()
        y = transform.test_forward(x)
        assert y.shape == (2, 2) and bool(torch.isfinite(y).all())
        y, time = transform.test_forward(x, torch.zeros(2, 2, device="cuda"))
        assert y.shape == (2, 2) and bool(torch.isfinite(y).all()) and time.shape == (2, 2)
        if invert:
            transform.invert(y)


class RealtimeTruePeak(CarriedState, TruePeak):
    """A true-peak meter over a stream.  `forward` takes the next (..., C, n) chunk, any n >= 1 -- shorter than the filter
    too; a 1-D chunk is one mono stream -- and returns (..., C) float32: the true peak in dBTP of the oversampled values
    this chunk completes, -inf (and no launch) for n == 0.  `peak()` gives the maximum since the stream began per channel in
    dBTP, `programme()` that over the channels, `linear()` the running maximum as it is kept, `index()` its oversampled
    index in the stream.  All of them have the bits of the one-call TruePeak on the concatenated signal, whatever the
    chunking: every oversampled value is the same fmaf chain on the same samples, and a maximum is exact.

    Carried: `input_buffer` (lead..., C, K - 1) float32, the samples before the next chunk; `max_peak` (lead..., C) float32,
    linear; `max_index` (lead..., C) int64; and `samples_seen`, a host integer that is never read back from the device,
    through get_extra_state / set_extra_state.  Zeros and 0 on a new leading shape (lead..., C) or device and after `reset()`;
    any batch shape from a `state_dict`.  A call is one launch where the chunk fits a tile of 2048 samples (else two, with
    16 bytes of workspace per tile) plus the dBTP expression; no torch.cat, no synchronisation, no allocation but the result:
    the kernel writes the next `input_buffer` into a second buffer and the two change places.  `latency` is 0.  The outputs
    carry no graph: it is a meter, the offline TruePeak keeps its gradient."""

    _STATE = ("input_buffer", "max_peak", "max_index")

    def __init__(self, sr: int = 44100, oversample: Optional[int] = None, taps=None):
        super().__init__(sr=sr, oversample=oversample, taps=taps)
        self.samples_seen = 0
        self._spare = None
        self.register_buffer("input_buffer", torch.zeros(self.taps.shape[1] - 1))
        self.register_buffer("max_peak", torch.zeros(()))
        self.register_buffer("max_index", torch.zeros((), dtype=torch.int64))
        self._carries(*self._STATE)

    def get_extra_state(self):
        return {"samples_seen": int(self.samples_seen)}

    def set_extra_state(self, state) -> None:
        self.samples_seen = int(state["samples_seen"])

    def _reset_extra(self) -> None:
        self.samples_seen = 0

    @property
    def latency(self) -> int:
        return 0

    def streaming(self) -> "RealtimeTruePeak":
        return self

    def realtime(self):
        return self

    def _stream(self, lead, x: torch.Tensor) -> None:
        """Makes the buffers those of the stream of x: zeros, and no sample seen, on a new leading shape or device; of
        their own dtype and contiguous."""
        spare = self._spare
        if spare is not None and spare.device == x.device and all(
                b.device == x.device and tuple(b.shape) == tuple(lead) + self._carried[k][0]
                and b.dtype == self._carried[k][1] and b.is_contiguous() for k, b in ((k, self._buffers[k]) for k in self._STATE)) \
                and spare.shape == self.input_buffer.shape and spare.data_ptr() != self.input_buffer.data_ptr():
            return                                           # the stream goes on: nothing to make
        rows = self._carried_rows(self._STATE, lead, x)
        if rows is None:
            self.samples_seen = 0
            for k in self._STATE:
                tail, dtype = self._carried[k]
                setattr(self, k, torch.zeros(tuple(lead) + tail, dtype=dtype, device=x.device))
        else:
            for k, r in zip(self._STATE, rows):              # what a module cast or a strided state_dict entry changed
                if r.data_ptr() != self._buffers[k].data_ptr() or self._buffers[k].dtype != self._carried[k][1]:
                    self._carry(k, r, lead)
        if self._spare is None or self._spare.shape != self.input_buffer.shape or self._spare.device != x.device \
                or self._spare.data_ptr() == self.input_buffer.data_ptr():
            self._spare = torch.empty_like(self.input_buffer)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim < 1:
            raise ValueError("RealtimeTruePeak.forward takes a (..., C, n) chunk, got a scalar")
        ops._no_fp64(x)
        x = x.detach()
        lead, n = tuple(x.shape[:-1]), x.shape[-1]
        if n == 0:                                           # nothing arrived: no launch, the state stays
            return torch.full(lead, float("-inf"), dtype=torch.float32, device=x.device)
        device_scoped(require_device)(x)                     # before any state is touched: there is no CPU route
        self._stream(lead, x)
        peak = ops.true_peak_stream(x, self.taps, self.input_buffer, self._spare, self.max_peak, self.max_index,
                                    self.oversample * self.samples_seen)
        if self.taps.shape[1] > 1:                           # the kernel wrote the next state: the two change places
            filled, self._spare = self._spare, self.input_buffer
            self.input_buffer = filled
        self.samples_seen += n
        return dbtp(peak)

    def peak(self) -> torch.Tensor:
        """(..., C) float32: the maximum true peak since the stream began, in dBTP; -inf before the first chunk."""
        return dbtp(self.max_peak.float())

    def programme(self) -> torch.Tensor:
        y = self.peak()
        return y if y.ndim == 0 else y.amax(dim=-1)

    def linear(self) -> torch.Tensor:
        return self.max_peak.float().clone()

    def index(self) -> torch.Tensor:
        return self.max_index.clone()

    def sample_peak(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError("RealtimeTruePeak carries one table: a sample-peak stream is RealtimeTruePeak(oversample=1)")

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

Not built: a streaming meter (it would carry the filter state, a partial hop and a ring of hop sums; `realtime()` says so
and returns the offline module), loudness range (LRA) and true peak, a row-splitting dispatch for one very long row (a row
is one workgroup, as for SOSFilter), gradients with respect to the channel weights, torchaudio's approximate pre-filter,
second-order gradients.
"""
import warnings
from typing import Optional

import torch

from .. import ops
from ..autograd import LoudnessBlocksFunction, LoudnessFunction, wants_grad
from .base import AudioTransform, InversionEnumType, NotInvertibleError

__all__ = ["Loudness", "LoudnessNormalize"]


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

    def invert(self, x: torch.Tensor, inversion_mode: InversionEnumType = None, **kwargs) -> torch.Tensor:
        raise NotInvertibleError

    def forward_with_time(self, x: torch.Tensor, time: torch.Tensor):
        return self.forward(x), time

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
    usual choice for augmentation).  Not invertible: the gain is not kept."""

    def __repr__(self):
        return "LoudnessNormalize(target=%s, sr=%s, channel_weights=%s, detach_gain=%s)" % (
            self.target, self.sr, self.channel_weights, self.detach_gain)

    def __init__(self, target: float = -23.0, sr: int = 44100, channel_weights=None, detach_gain: bool = False):
        super().__init__(sr=sr, channel_weights=channel_weights)
        self.target, self.detach_gain = float(target), bool(detach_gain)
        if not self.target == self.target or self.target in (float("inf"), float("-inf")):
            raise ValueError("target must be a finite loudness in LUFS, got %r" % (target,))

    def gain(self, x: torch.Tensor) -> torch.Tensor:
        """The linear gain per clip, (...,)."""
        lufs = Loudness.forward(self, x.detach() if self.detach_gain else x)
        gain = torch.pow(10.0, (self.target - lufs) / 20.0)
        return torch.where(torch.isinf(lufs), torch.ones_like(gain), gain)

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

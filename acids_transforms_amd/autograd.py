"""Autograd for STFT / DGT (forward and invert), Magnitude and MFCC, for the invert of Magnitude, Polar, Cartesian,
Real / Imaginary / Phase and Normalize, for the forward of Normalize, Phase, IF, Cartesian, Polar and PolarIF, and for the
streaming path (OverlapAdd, RealtimeSTFT and RealtimeDGT, forward and invert):
torch.autograd.Functions whose backward passes are the HIP adjoints of autograd.hip, mfcc_grad.hip, invert_grad.hip,
repr_grad.hip and stream_grad.hip (through ops.stft_backward / ops.istft_backward / ops.magnitude_backward /
ops.mfcc_backward / ops.magnitude_invert_backward / ops.polar_to_complex_backward / ops.cartesian_inverse_backward /
ops.phase_scan_backward / ops.cartesian_forward_backward / ops.rfft_frames_backward / ops.irfft_frames_backward /
ops.oadd_forward_backward / ops.oadd_invert_backward).

The reference is plain torch, so its STFT, DGT and Magnitude (and their composition) sit inside a training loss.  Here
the forward kernels write into fresh tensors through ctypes, which cuts the graph; the modules therefore route a call
through these Functions when -- and only when -- grad mode is on and the input requires grad.  Every other call runs
the plain forward, bit for bit the same kernels.  The forward values of the autograd route are those same kernels too.

On the streaming path the carried state (OverlapAdd's history and tail, the phase buffer, the PGHI history) is a
constant of the graph, stored detached: the gradient of a chunk covers that chunk's own samples (truncated
back-propagation at chunk boundaries).

SpectralDistanceFunction is the one Function of two inputs: the multi-scale spectral distance of losses.py, whose
backward (spectral_distance.hip through ops.spectral_distance_backward) rebuilds both spectra from the saved audio.
MelSpectralDistanceFunction is its mel-scale sibling (mel_distance.hip through ops.mel_rows / ops.mel_distance_sums /
ops.mel_distance_backward): to differentiate one signal it rebuilds that signal's spectrum and the other's mel rows.

PqmfFunction and PqmfInvertFunction are PQMF's forward and invert (pqmf.hip): synthesis is n_band x the transpose of
analysis, so each one's backward is the other's kernel with the transposed scale, and neither saves a tensor.
PqmfStreamFunction and PqmfStreamInvertFunction are RealtimePQMF's (ops.pqmf_analysis_stream /
ops.pqmf_synthesis_stream): the causal bank delayed by D blocks forward, the other kernel ADVANCED by D blocks and
without state backward; the carried filter state is a constant of the graph like every other streaming state.

ResampleFunction and ResampleStreamFunction are utils.Resample's and utils.RealtimeResample's (resample.hip): sample-rate
conversion is linear, so both backward passes are one kernel, the transposed polyphase filter (ops.resample_sinc_backward),
which the streaming form calls with the state's length as the lead of its window; neither saves a tensor.
ResampleDirectFunction is the bankless route (sinc_interp.hip) of Resample(direct=True) and PitchShift: forward and backward
are one kernel with the two rates exchanged.

PhaseVocoderFunction is transforms.TimeStretch's (phase_vocoder.hip): the forward also hands back the phasor after its last
step, and the backward (ops.phase_vocoder_backward) walks the steps downwards from it; the graph keeps the spectrum and
that (..., F) phasor.

SosFilterFunction and SosFilterStreamFunction are transforms.SOSFilter's and RealtimeSOSFilter's (sos_filter.hip): the
adjoint of a recursive filter with zero state is the same filter run backwards in time, so the backward is the forward
kernel with its direction flag flipped; coefficients and carried state are constants of the graph, and neither saves a tensor.

LoudnessFunction and LoudnessBlocksFunction are transforms.Loudness's (loudness.hip on the hop powers of sos_filter.hip):
the gates are piecewise constant, hence constants of the graph, and the rest is a function of the hop powers, so the
backward is a weight per hop, the K-weighted signal times it (recomputed, never stored) and the reverse filter.  They keep
x, the (..., C, hops) powers and the three gating statistics per clip.

TruePeakFunction is transforms.TruePeak's (true_peak.hip): a maximum is piecewise linear, so the backward is the subgradient
at the attained maximum -- the K taps of one phase, scaled and signed, under one oversampled index -- and the graph keeps a
peak, an index and a sign per row.

FFTConvolveFunction is ops.fft_convolve's (fft_convolve.hip), the one Function here with two differentiable inputs that are
both audio-like: it saves x and h and nothing else, and the backward (ops.fft_convolve_backward) rebuilds the spectra chunk
by chunk and computes only the gradients that are asked for.

ImpulseResponseStreamFunction is transforms.RealtimeImpulseResponse's: one chunk of a stream through
ops.fft_convolve_stream.  The carried state (the tail of the input and the ring of spectra) is a constant of the graph;
the graph keeps the filter's spectrum and, only when the response requires grad, the chunk's frames and a copy of the
P - 1 history frames, taken out of the ring before the launch overwrites anything.

All backward passes are first-order only (@once_differentiable): create_graph=True raises.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["wants_grad", "StftFunction", "IstftFunction", "IstftPolarFunction", "MagnitudeFunction",
           "StftMagnitudeFunction", "MfccFunction", "mfcc_chunk_clips", "MagnitudeInvertFunction", "PolarInvertFunction",
           "CartesianInvertFunction", "PolarToComplexFunction", "AffineInvertFunction", "AffineForwardFunction",
           "PhaseScanFunction", "CartesianFunction", "PolarFunction", "PolarIFFunction", "StftPolarFunction",
           "RtStftFunction", "RtIstftFunction", "RtIstftPolarFunction", "OaddFramesFunction", "OaddInvertFunction",
           "SpectralDistanceFunction", "specdist_chunk_clips", "MelSpectralDistanceFunction", "meldist_sums",
           "meldist_loss", "PqmfFunction", "PqmfInvertFunction", "PqmfStreamFunction", "PqmfStreamInvertFunction",
           "ResampleFunction", "ResampleStreamFunction", "ResampleDirectFunction", "PhaseVocoderFunction",
           "SosFilterFunction", "SosFilterStreamFunction", "LoudnessFunction", "LoudnessBlocksFunction", "FFTConvolveFunction", "ImpulseResponseStreamFunction",
           "TruePeakFunction", "dbtp"]


def wants_grad(x: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and x.requires_grad


class StftFunction(torch.autograd.Function):
    """x (B, L) float32 -> (X (B, T, F) complex64, phase (B, T, F) float32 or an empty tensor).
    Saves nothing but shapes (and the module's window buffer, which is not part of the graph)."""

    @staticmethod
    def forward(ctx, x, window, n_fft, hop, want_phase):
        ctx.window, ctx.n_fft, ctx.hop, ctx.L = window, n_fft, hop, x.shape[-1]
        if want_phase:
            X, phase = ops.stft_forward(x, window, n_fft, hop, center=True, want_phase=True)
        else:
            X, phase = ops.stft_forward(x, window, n_fft, hop, center=True), x.new_empty(0)
        ctx.mark_non_differentiable(phase)
        return X, phase

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _gphase):
        if G is None:
            return None, None, None, None, None
        return ops.stft_backward(G, ctx.window, ctx.n_fft, ctx.hop, ctx.L), None, None, None, None


class IstftFunction(torch.autograd.Function):
    """X (B, T, F) complex -> ops.istft(X), whose backward is the ISTFT adjoint.  Saves the frame count and the
    module's window and envelope table (buffers, not part of the graph)."""

    @staticmethod
    def forward(ctx, X, inv_window, n_fft, hop, env16):
        ctx.inv_window, ctx.n_fft, ctx.hop, ctx.env16, ctx.T = inv_window, n_fft, hop, env16, X.shape[-2]
        return ops.istft(X, inv_window, n_fft, hop, env16=env16)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gX = ops.istft_backward(gy, ctx.inv_window, ctx.n_fft, ctx.hop, ctx.T, env16=ctx.env16)
        return gX, None, None, None, None


class IstftPolarFunction(torch.autograd.Function):
    """ops.istft(mag e^{i phase}) for a magnitude mag (B, T, F) and a constant phase (anything that broadcasts to mag):
    the gradient of mag is Re(gX e^{-i phase}), the phase gets none.  Saves the phase (as ops.istft read it)."""

    @staticmethod
    def forward(ctx, mag, phase, inv_window, n_fft, hop, env16):
        phase = ops._f32c(phase.detach())
        if phase.shape != mag.shape:
            phase = phase.expand_as(mag).contiguous()
        ctx.inv_window, ctx.n_fft, ctx.hop, ctx.env16, ctx.phase = inv_window, n_fft, hop, env16, phase
        return ops.istft(None, inv_window, n_fft, hop, env16=env16, mag=mag, phase=phase)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gmag = ops.istft_backward(gy, ctx.inv_window, ctx.n_fft, ctx.hop, ctx.phase.shape[-2], env16=ctx.env16,
                                  phase=ctx.phase)
        return gmag, None, None, None, None, None


def _cached(module, slot, src, device, make):
    """make(src), kept on the module under `slot` until the tensor src is replaced or edited in place."""
    key = (src.data_ptr(), src._version, str(device))
    cache = module.__dict__.setdefault("_grad_cols", {})
    hit = cache.get(slot)
    if hit is None or hit[0] != key:
        hit = cache[slot] = (key, make(src))
    return hit[1]


def _bank_cols(module, name, device, transposed=False):
    """utils.banded.bank_columns of the module's bank `name` (of its transpose with transposed=True) as tensors on
    `device`: built on first use, cached per bank version."""
    from .utils.banded import bank_columns

    def make(bank):
        cols = bank_columns(bank.transpose(-2, -1) if transposed else bank)
        return tuple(torch.from_numpy(a).to(device) for a in cols)
    return _cached(module, (name, transposed), getattr(module, name), device, make)


def _bank_tables(module, device):
    """(forward bank, transposed bank) by-column tables of a Magnitude's mel_bank on `device`, or (None, None) when
    mel=False."""
    if not module.mel:
        return None, None
    return _bank_cols(module, "mel_bank", device), _bank_cols(module, "mel_bank", device, transposed=True)


def _magnitude_grad(module, x, dF, dx_accum=None):
    fwd, inv = _bank_tables(module, x.device)
    _, sc = module._affine()
    return ops.magnitude_backward(x, dF, fwd, inv, module.contrast_mode, sc, module._eps,
                                  col_off=0 if module.keep_nyquist else 1, dx_accum=dx_accum)


class MagnitudeFunction(torch.autograd.Function):
    """Magnitude.forward with its backward.  Saves its input (the backward recomputes M from it)."""

    @staticmethod
    def forward(ctx, x, module):
        ctx.module = module
        ctx.save_for_backward(x)
        return module._forward_plain(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, dF):
        (x,) = ctx.saved_tensors
        dx = _magnitude_grad(ctx.module, x, dF.contiguous())
        return dx.reshape(x.shape), None


class StftMagnitudeFunction(torch.autograd.Function):
    """The fused n_fft = 1024 STFT -> Magnitude forward (ops.stft_mel_forward, spectrum kept) with its backward: the
    Magnitude backward on the saved spectrum (plus the spectrum's own gradient, when the caller used it), then the
    STFT adjoint.  x (B, L) -> (X (B, T, 513) complex64, features (B, T, N), phase or an empty tensor)."""

    @staticmethod
    def forward(ctx, x, stage, module, want_phase):
        off, sc = module._affine()
        X, phase, feat = ops.stft_mel_forward(x, stage.window[:1024], module._banded(), module.contrast_mode, off, sc,
                                              module._eps, want_phase=want_phase, hop=stage._hop)
        ctx.stage, ctx.module, ctx.L = stage, module, x.shape[-1]
        ctx.save_for_backward(X)
        phase = phase if phase is not None else x.new_empty(0)
        ctx.mark_non_differentiable(phase)
        ctx.set_materialize_grads(False)
        return X, feat, phase

    @staticmethod
    @once_differentiable
    def backward(ctx, gX, gfeat, _gphase):
        (X,) = ctx.saved_tensors
        if gfeat is not None:
            gX = _magnitude_grad(ctx.module, X, gfeat.contiguous(), dx_accum=gX)
        if gX is None:
            return None, None, None, None
        stage = ctx.stage
        return ops.stft_backward(gX, stage.window[:stage._n_fft], stage._n_fft, stage._hop, ctx.L), None, None, None


MFCC_CHUNK_ELEMS = 1 << 26      # complex64 elements of spectrum per chunk of MfccFunction.backward: 512 MiB


def _chunk_clips(elems, B, T, n_fft):
    """The most of B clips whose spectrum (T frames of n_fft // 2 + 1 bins per clip) stays within elems, at least 1."""
    return min(max(elems // (T * (n_fft // 2 + 1)), 1), B)


def mfcc_chunk_clips(B, T, n_fft):
    """Clips per chunk of MfccFunction.backward: _chunk_clips under MFCC_CHUNK_ELEMS as it stands at the call (189 at
    n_fft 1024 / hop 256 and 4 s clips)."""
    return _chunk_clips(MFCC_CHUNK_ELEMS, B, T, n_fft)


def _mfcc_tables(module, device):
    """(forward bank tables or None, transposed bank tables, DCT matrix transposed or None) of an MFCC on `device`;
    the forward bank is walked only on the n_mfcc route.  The DCT matrix follows its own version."""
    inv = _bank_cols(module, "fbank", device, transposed=True)
    if module.n_mfcc is None:
        return None, inv, None
    dct_t = _cached(module, "dct_t", module.dct, device, lambda dct: dct.to(device).t().contiguous())
    return _bank_cols(module, "fbank", device), inv, dct_t


class MfccFunction(torch.autograd.Function):
    """MFCC.forward with its backward.  Saves the audio only: the fused forward never writes a spectrum, so the backward
    rebuilds it from the audio, a chunk of clips at a time (mfcc_chunk_clips), turns it into its own gradient in place
    (ops.mfcc_backward) and runs the STFT adjoint into the chunk's rows of dx.  The window, bank, DCT and Normalize
    statistics are constants of the graph."""

    @staticmethod
    def forward(ctx, x, module):
        y = module._forward_plain(x)
        ctx.window, ctx.n_fft, ctx.hop, ctx.power = module.window, module.n_fft, module.hop_length, int(module.power)
        ctx.tables = _mfcc_tables(module, x.device)
        ctx.scale = module.norm._params(x)[1] if module.norm is not None else None
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dF):
        (x,) = ctx.saved_tensors
        n, hop = ctx.n_fft, ctx.hop
        xb = ops._f32c(x.reshape(-1, x.shape[-1]))
        B, L = xb.shape
        T = 1 + (L - (n & 1)) // hop
        dF = ops._f32c(dF).reshape(B, dF.shape[-2], T)
        fwd, inv, dct_t = ctx.tables
        dx = torch.empty((B, L), dtype=torch.float32, device=x.device)
        chunk = mfcc_chunk_clips(B, T, n)
        for b0 in range(0, B, chunk):
            X = ops.stft_forward(xb[b0:b0 + chunk], ctx.window, n, hop, center=True)
            ops.mfcc_backward(X, dF[b0:b0 + chunk], inv, ctx.power, fwd, dct_t, ctx.scale, inplace=True)
            ops.stft_backward(X, ctx.window, n, hop, L, out=dx[b0:b0 + chunk])
            del X
        dx = dx if x.shape == dx.shape else dx.view(x.shape)
        return dx.to(x.dtype), None


# ---- the multi-scale distances (losses.SpectralDistance, losses.MelSpectralDistance) -----------------------------------------
# One driver for both: a scale is (n_fft, hop) or (n_fft, hop, n_mels), and the two differ in the cells whose distance is
# taken -- the bins of a spectrum, or its mel rows -- and in which spectra the backward holds together.

SPECDIST_CHUNK_ELEMS = 1 << 26      # complex64 elements of ONE spectrum per chunk: 512 MiB, so x's and y's peak at 1 GiB


def specdist_chunk_clips(B, T, n_fft):
    """Clips per chunk of both distances, forward and backward: _chunk_clips of ONE spectrum under SPECDIST_CHUNK_ELEMS
    as it stands at the call."""
    return _chunk_clips(SPECDIST_CHUNK_ELEMS, B, T, n_fft)


def _frames(L, n_fft, hop):
    return 1 + (L - (n_fft & 1)) // hop


def _specdist_chunks(B, L, n_fft, hop):
    """(b0, b1) of every chunk of B clips of L samples at one scale."""
    chunk = max(specdist_chunk_clips(B, _frames(L, n_fft, hop), n_fft), 1)
    return [(b0, min(b0 + chunk, B)) for b0 in range(0, B, chunk)]


def _dist_sums(x, y, scales, cells_of, sums_op, eps):
    """x, y (B, L) float32 -> (B, n_scales, 3) float64, the sums S_D, S_B, S_L of every clip at every scale: sums_op on
    cells_of(s, clips) of x's and then of y's rows of a chunk of clips, both freed before the next chunk."""
    B, L = x.shape
    per_scale = []
    for s, (n, hop, *_) in enumerate(scales):
        out = torch.empty((B, 3), dtype=torch.float64, device=x.device)
        for b0, b1 in _specdist_chunks(B, L, n, hop):
            X = cells_of(s, x[b0:b1])
            Y = cells_of(s, y[b0:b1])
            sums_op(X, Y, eps, out=out[b0:b1])
            del X, Y
        per_scale.append(out)
    return torch.stack(per_scale, 1)


def _dist_loss(sums, cells, lin_weight, log_weight):
    """The per-clip loss (B,) float32 of the sums: sum over scales of lin_weight S_D / S_B + log_weight S_L / n, n the
    scale's cells per clip."""
    loss = (sums[:, :, 0] / sums[:, :, 1]).sum(1) * lin_weight
    for s, n in enumerate(cells):
        loss = loss + sums[:, s, 2] * (log_weight / n)
    return loss.float()


class _DistBackward:
    """What the two backward passes share.  Allocates the (B, L) gradient of every input that needs one and the
    (chunk, L) scratch of the later scales; chunks() walks scales and chunks of clips; put() runs the STFT adjoint of one
    spectrum gradient -- into the result for the first scale, into the scratch that is added to it for every later one.
    Which spectra are built, alive together and freed is the caller's, between two calls."""

    def __init__(self, x, gclip, need, scales, windows):
        B, L = x.shape
        self.B, self.L, self.scales, self.windows = B, L, scales, windows
        self.g = ops._f32c(gclip)
        self.grads = [torch.empty((B, L), dtype=torch.float32, device=x.device) if nd else None for nd in need]
        rows = max([b1 - b0 for n, hop, *_ in scales[1:] for b0, b1 in _specdist_chunks(B, L, n, hop)[:1]], default=0)
        self.scratch = torch.empty((rows, L), dtype=torch.float32, device=x.device)

    def chunks(self, sums):
        """(s, b0, b1, the sums and the upstream gradient of clips b0:b1 at scale s) of every scale and chunk of clips."""
        for s, (n, hop, *_) in enumerate(self.scales):
            sums_s = sums[:, s].contiguous()
            for b0, b1 in _specdist_chunks(self.B, self.L, n, hop):
                yield s, b0, b1, sums_s[b0:b1], self.g[b0:b1]

    def put(self, k, G, s, b0, b1):
        """Input k's gradient of clips b0:b1 at scale s from the gradient G of their spectrum."""
        n, hop = self.scales[s][:2]
        out = self.grads[k][b0:b1] if s == 0 else self.scratch[:b1 - b0]      # stft_backward overwrites its out
        ops.stft_backward(G, self.windows[s], n, hop, self.L, out=out)
        if s:
            self.grads[k][b0:b1].add_(out)


def specdist_sums(x, y, windows, scales, eps):
    """_dist_sums of the two spectra of a chunk of clips (ops.spectral_distance_sums), which are alive together."""
    return _dist_sums(x, y, scales, lambda s, c: ops.stft_forward(c, windows[s], *scales[s], center=True),
                      ops.spectral_distance_sums, eps)


def specdist_loss(sums, L, scales, lin_weight, log_weight):
    """_dist_loss with n = T F bins per clip."""
    return _dist_loss(sums, [_frames(L, n, hop) * (n // 2 + 1) for n, hop in scales], lin_weight, log_weight)


class SpectralDistanceFunction(torch.autograd.Function):
    """The per-clip multi-scale spectral distance of x (generated) and y (target), both (B, L) float32, with its backward.
    Saves the two audios and the (B, n_scales, 3) sums, and nothing else: the backward rebuilds both spectra per scale
    and chunk of clips (specdist_chunk_clips), turns them into their own gradients in place
    (ops.spectral_distance_backward) and runs the STFT adjoint -- into the result for the first scale, into a (chunk, L)
    scratch that is added to it for every later one (_DistBackward).  Only the inputs that require a gradient get one;
    the windows are constants of the graph."""

    @staticmethod
    def forward(ctx, x, y, windows, scales, lin_weight, log_weight, eps):
        sums = specdist_sums(x, y, windows, scales, eps)
        ctx.windows, ctx.scales, ctx.weights, ctx.eps = windows, scales, (lin_weight, log_weight), eps
        ctx.save_for_backward(x, y, sums)
        return specdist_loss(sums, x.shape[-1], scales, lin_weight, log_weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, gclip):
        x, y, sums = ctx.saved_tensors
        need = ctx.needs_input_grad[:2]
        bwd = _DistBackward(x, gclip, need, ctx.scales, ctx.windows)
        for s, b0, b1, sums_c, g in bwd.chunks(sums):
            (n, hop), w = ctx.scales[s], ctx.windows[s]
            X = ops.stft_forward(x[b0:b1], w, n, hop, center=True)
            Y = ops.stft_forward(y[b0:b1], w, n, hop, center=True)
            ops.spectral_distance_backward(X, Y, sums_c, g, *ctx.weights, ctx.eps, *need)
            for k, G in enumerate((X, Y)):
                if need[k]:
                    bwd.put(k, G, s, b0, b1)
            del X, Y
        return bwd.grads[0], bwd.grads[1], None, None, None, None, None


def _meldist_tables(module, device):
    """Per scale, (bank by column, transposed bank by column) of a MelSpectralDistance's mel_bank_i on `device`: built
    on first use, cached per bank version."""
    return tuple((_bank_cols(module, "mel_bank_%d" % i, device), _bank_cols(module, "mel_bank_%d" % i, device, transposed=True))
                 for i in range(len(module.scales)))


def _mel_of(x, w, n, hop, cols):
    """The mel rows (chunk, T, N) of a chunk of clips; the spectrum is freed before the return."""
    X = ops.stft_forward(x, w, n, hop, center=True)
    M = ops.mel_rows(X, cols)
    del X
    return M


def meldist_sums(x, y, windows, scales, tables, eps):
    """_dist_sums of the two arrays of mel rows of a chunk of clips (ops.mel_distance_sums).  One spectrum is alive at a
    time, so the peak is 512 MiB."""
    return _dist_sums(x, y, scales, lambda s, c: _mel_of(c, windows[s], *scales[s][:2], tables[s][0]),
                      ops.mel_distance_sums, eps)


def meldist_loss(sums, L, scales, lin_weight, log_weight):
    """_dist_loss with n = T n_mels cells per clip."""
    return _dist_loss(sums, [_frames(L, n, hop) * n_mels for n, hop, n_mels in scales], lin_weight, log_weight)


class MelSpectralDistanceFunction(torch.autograd.Function):
    """The per-clip multi-scale mel distance of x (generated) and y (target), both (B, L) float32, with its backward.
    Saves the two audios and the (B, n_scales, 3) sums, and nothing else.  Per scale, chunk of clips and input that
    needs a gradient, the backward rebuilds the OTHER signal's mel rows (spectrum, ops.mel_rows, spectrum freed), then
    this signal's spectrum, turns it into its own gradient in place (ops.mel_distance_backward) and runs the STFT
    adjoint -- into the result for the first scale, into a (chunk, L) scratch that is added to it for every later one
    (_DistBackward).  The x-only backward never holds two spectra and never runs a backward kernel over Y.  The windows
    and the banks are constants of the graph."""

    @staticmethod
    def forward(ctx, x, y, windows, scales, tables, lin_weight, log_weight, eps):
        sums = meldist_sums(x, y, windows, scales, tables, eps)
        ctx.windows, ctx.scales, ctx.tables, ctx.weights, ctx.eps = windows, scales, tables, (lin_weight, log_weight), eps
        ctx.save_for_backward(x, y, sums)
        return meldist_loss(sums, x.shape[-1], scales, lin_weight, log_weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, gclip):
        x, y, sums = ctx.saved_tensors
        need = ctx.needs_input_grad[:2]
        bwd = _DistBackward(x, gclip, need, ctx.scales, ctx.windows)
        for s, b0, b1, sums_c, g in bwd.chunks(sums):
            (n, hop, _), w, (cols, cols_t) = ctx.scales[s], ctx.windows[s], ctx.tables[s]
            for side, (own, other) in enumerate(((x, y), (y, x))):
                if not need[side]:
                    continue
                O = _mel_of(other[b0:b1], w, n, hop, cols)
                S = ops.stft_forward(own[b0:b1], w, n, hop, center=True)
                ops.mel_distance_backward(S, O, sums_c, g, cols, cols_t, *ctx.weights, ctx.eps, side)
                bwd.put(side, S, s, b0, b1)
                del S, O
        return bwd.grads[0], bwd.grads[1], None, None, None, None, None, None


# ---- PQMF (transforms.PQMF): analysis and synthesis are each other's transpose up to n_band ---------------------------------

class PqmfFunction(torch.autograd.Function):
    """PQMF.forward: x (rows, L) float32 -> ops.pqmf_analysis(x) (rows, M, L / M).  Saves nothing but the module's two
    buffers (prototype, modulation: constants of the graph); the backward is the synthesis kernel with scale 1."""

    @staticmethod
    def forward(ctx, x, proto, mod):
        ctx.proto, ctx.mod, ctx.dtype = proto, mod, x.dtype
        return ops.pqmf_analysis(x, proto, mod, 1.0)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return ops.pqmf_synthesis(gy, ctx.proto, ctx.mod, 1.0).to(ctx.dtype), None, None


class PqmfInvertFunction(torch.autograd.Function):
    """PQMF.invert: y (rows, M, T) float32 -> ops.pqmf_synthesis(y, scale M) (rows, M T).  Saves nothing but the
    module's two buffers; the backward is the analysis kernel with scale M."""

    @staticmethod
    def forward(ctx, y, proto, mod):
        ctx.proto, ctx.mod, ctx.dtype = proto, mod, y.dtype
        return ops.pqmf_synthesis(y, proto, mod, float(mod.shape[0]))

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        return ops.pqmf_analysis(gx, ctx.proto, ctx.mod, float(ctx.mod.shape[0])).to(ctx.dtype), None, None


class PqmfStreamFunction(torch.autograd.Function):
    """RealtimePQMF.forward: chunk x (rows, C) float32, state (rows, Ha) or None -> (y (rows, M, C / M), new_state
    (rows, Ha)) by ops.pqmf_analysis_stream.  The state is a constant of the graph and the new state is not
    differentiable, so the gradient covers the chunk's own samples: y[k, t] = sum_n h_k[n] x[(t - D) M + n - P] gives
    gx[s] = the offline synthesis of gy (scale 1) at sample s + D M, i.e. the synthesis kernel advanced by D blocks
    with no state.  Saves no tensor: the two tables hang on the node."""

    @staticmethod
    def forward(ctx, x, state, proto, mod):
        ctx.proto, ctx.mod, ctx.dtype = proto, mod, x.dtype
        y, new_state = ops.pqmf_analysis_stream(x, state, proto, mod, 1.0)
        ctx.mark_non_differentiable(new_state)
        return y, new_state

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gstate):
        D = ops.pqmf_stream_sizes(ctx.mod.shape[0], ctx.proto.numel())[0]
        gx, _ = ops.pqmf_synthesis_stream(gy, None, ctx.proto, ctx.mod, 1.0, shift=D, want_state=False)
        return gx.to(ctx.dtype), None, None, None


class PqmfStreamInvertFunction(torch.autograd.Function):
    """RealtimePQMF.invert: chunk y (rows, M, c) float32, state (rows, M, Hs) or None -> (x (rows, M c), new_state) by
    ops.pqmf_synthesis_stream with scale M.  The backward is the analysis kernel with scale M, advanced by D blocks,
    over the zero-extended gx and with no state.  Saves no tensor."""

    @staticmethod
    def forward(ctx, y, state, proto, mod):
        ctx.proto, ctx.mod, ctx.dtype = proto, mod, y.dtype
        x, new_state = ops.pqmf_synthesis_stream(y, state, proto, mod, float(mod.shape[0]))
        ctx.mark_non_differentiable(new_state)
        return x, new_state

    @staticmethod
    @once_differentiable
    def backward(ctx, gx, _gstate):
        M = ctx.mod.shape[0]
        D = ops.pqmf_stream_sizes(M, ctx.proto.numel())[0]
        gy, _ = ops.pqmf_analysis_stream(gx, None, ctx.proto, ctx.mod, float(M), shift=D, want_state=False)
        return gy.to(ctx.dtype), None, None, None


# ---- Resample (utils.Resample / RealtimeResample): the backward is the transposed polyphase filter ------------------------

class ResampleFunction(torch.autograd.Function):
    """Resample.forward: x (rows, L) float32 -> ops.resample_sinc(x) (rows, ceil(new L / orig)).  Saves no tensor: L,
    the three integers and the module's bank (a constant of the graph) hang on the node; the backward is
    ops.resample_sinc_backward with lead = width."""

    @staticmethod
    def forward(ctx, x, bank, orig, new, width):
        ctx.bank, ctx.orig, ctx.new, ctx.width, ctx.L, ctx.dtype = bank, orig, new, width, x.shape[-1], x.dtype
        return ops.resample_sinc(x, orig, new, width, bank)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gx = ops.resample_sinc_backward(gy, ctx.L, ctx.orig, ctx.new, 2 * ctx.width + ctx.orig, ctx.width, ctx.bank)
        return gx.to(ctx.dtype), None, None, None, None


class ResampleStreamFunction(torch.autograd.Function):
    """RealtimeResample.forward: chunk x (rows, C) float32, state (rows, Ha) or None -> (y (rows, C new / orig),
    new_state (rows, Ha)) by ops.resample_sinc_stream.  The state is a constant of the graph and the new state is not
    differentiable, so the gradient covers the chunk's own samples: output block t reads chunk sample n at tap n + Ha -
    t orig, which is ops.resample_sinc_backward with lead = Ha over the chunk's own output blocks.  Saves no tensor."""

    @staticmethod
    def forward(ctx, x, state, bank, orig, new, width):
        ctx.bank, ctx.orig, ctx.new, ctx.width, ctx.C, ctx.dtype = bank, orig, new, width, x.shape[-1], x.dtype
        y, new_state = ops.resample_sinc_stream(x, state, orig, new, width, bank)
        ctx.mark_non_differentiable(new_state)
        return y, new_state

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gstate):
        Ha = ops.resample_stream_sizes(ctx.orig, ctx.width)[1]
        gx = ops.resample_sinc_backward(gy, ctx.C, ctx.orig, ctx.new, 2 * ctx.width + ctx.orig, Ha, ctx.bank)
        return gx.to(ctx.dtype), None, None, None, None, None


class ResampleDirectFunction(torch.autograd.Function):
    """Resample(direct=True).forward and PitchShift's last stage: x (rows, L) float32 -> ops.sinc_interp(x, orig, new)
    (rows, ceil(new L / orig)) through the converter's half-table (sinc_interp.hip), no bank.  Saves no tensor: L, the
    three integers and the table (a constant of the graph) hang on the node; the backward is the same kernel with the
    rates exchanged."""

    @staticmethod
    def forward(ctx, x, table, Qi, orig, new):
        ctx.table, ctx.Qi, ctx.orig, ctx.new, ctx.L, ctx.dtype = table, Qi, orig, new, x.shape[-1], x.dtype
        return ops.sinc_interp(x, orig, new, table, Qi, -(-new * x.shape[-1] // orig))

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gx = ops.sinc_interp(gy, ctx.new, ctx.orig, ctx.table, ctx.Qi, ctx.L)
        return gx.to(ctx.dtype), None, None, None, None


# ---- TimeStretch: the phase vocoder, a scan up the steps forward and down them backward -------------------------------------

class PhaseVocoderFunction(torch.autograd.Function):
    """ops.phase_vocoder of a complex spectrum X (..., T, F) at `rate` -> (..., N, F), with its backward
    (ops.phase_vocoder_backward).  Saves X and the (..., F) phasor after the last step; the step table is a constant of
    the graph.  The forward values are the plain route's: the same kernel, which writes the phasor on the side."""

    @staticmethod
    def forward(ctx, X, rate):
        ctx.rate = float(rate)
        out, fin = ops.phase_vocoder(X, rate, want_phasor=True)
        ctx.save_for_backward(X, fin)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        X, fin = ctx.saved_tensors
        gX = ops.phase_vocoder_backward(X, g, ctx.rate, fin)
        return gX.reshape(X.shape).to(X.dtype), None


# ---- SOSFilter / RealtimeSOSFilter: the adjoint is the same cascade run the other way in time ---------------------------------

class SosFilterFunction(torch.autograd.Function):
    """ops.sos_filter(x, sos, reverse=reverse) with zero state, x (..., L) -> (..., L).  The backward is the same op with
    `reverse` flipped (gx = flip(H flip(g))), so forward followed by reverse -- zero-phase filtering -- is its own backward.
    Saves no tensor: the checked coefficients (a constant of the graph) and the flag hang on the node."""

    @staticmethod
    def forward(ctx, x, sos, reverse):
        ctx.sos, ctx.reverse, ctx.dtype = ops.sos_coefficients(sos), bool(reverse), x.dtype
        return ops.sos_filter(x, ctx.sos, reverse=ctx.reverse)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return ops.sos_filter(gy, ctx.sos, reverse=not ctx.reverse).to(ctx.dtype), None, None


class SosFilterStreamFunction(torch.autograd.Function):
    """RealtimeSOSFilter.forward: chunk x (..., C), state zi (..., n_sections, 2) float64 or None -> (y (..., C), zf) by
    ops.sos_filter.  The state is a constant of the graph and the new state is not differentiable, so the gradient covers
    the chunk's own samples: the zero-state adjoint over the chunk, ops.sos_filter(g, reverse=True).  Saves no tensor."""

    @staticmethod
    def forward(ctx, x, zi, sos):
        ctx.sos, ctx.dtype = ops.sos_coefficients(sos), x.dtype
        y, zf = ops.sos_filter(x, ctx.sos, zi=zi, return_state=True)
        ctx.mark_non_differentiable(zf)
        return y, zf

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gstate):
        return ops.sos_filter(gy, ctx.sos, reverse=True).to(ctx.dtype), None, None


class LoudnessFunction(torch.autograd.Function):
    """ops.loudness(x, sr, channel_weights): x (..., C, L) -> (...,) LUFS.  The forward is the plain route, bit for bit.
    Saves x, the hop powers and the gating statistics; the backward is ops.loudness_backward (three launches).  A clip that
    reads -inf has an exactly zero gradient."""

    @staticmethod
    def forward(ctx, x, sr, channel_weights):
        ctx.sr, ctx.weights = sr, channel_weights
        lufs, power, stats = ops.loudness(x, sr, channel_weights, return_state=True)
        ctx.save_for_backward(x, power, stats)
        return lufs

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, power, stats = ctx.saved_tensors
        return ops.loudness_backward(x, power, stats, g, ctx.sr, ctx.weights).reshape(x.shape).to(x.dtype), None, None


class LoudnessBlocksFunction(torch.autograd.Function):
    """ops.loudness_blocks(x, sr, hops_per_block, channel_weights): x (..., C, L) -> (..., nb) LUFS, ungated.  Saves x and the
    hop powers; the backward is ops.loudness_blocks_backward.  Silent blocks (-inf) pass nothing back."""

    @staticmethod
    def forward(ctx, x, sr, hops_per_block, channel_weights):
        ctx.sr, ctx.hb, ctx.weights = sr, hops_per_block, channel_weights
        blocks, power = ops.loudness_blocks(x, sr, hops_per_block, channel_weights, return_state=True)
        ctx.save_for_backward(x, power)
        return blocks

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, power = ctx.saved_tensors
        gx = ops.loudness_blocks_backward(x, power, g, ctx.sr, ctx.hb, ctx.weights)
        return gx.reshape(x.shape).to(x.dtype), None, None, None


def dbtp(peak: torch.Tensor) -> torch.Tensor:
    """A linear peak in dBTP, 20 log10 peak: -inf for silence.  The one expression every true-peak reading goes through, so
    equal peaks read equal."""
    return 20.0 * torch.log10(peak)


class TruePeakFunction(torch.autograd.Function):
    """ops.true_peak(x, taps): x (..., L) -> (...,) the linear true peak, or with db=True that peak in dBTP.  The forward is the
    plain route, bit for bit.  Saves one peak, one oversampled index and one sign per row -- nothing of the audio's size; the
    backward is ops.true_peak_backward, the subgradient at the attained maximum (one launch).  dBTP multiplies the incoming
    gradient by 20 / (ln 10 peak); a row that reads -inf (or NaN) gets exactly +0, by selection in the kernel."""

    @staticmethod
    def forward(ctx, x, taps, db):
        peak, index, sign = ops.true_peak(x, taps, return_state=True)
        ctx.taps, ctx.L, ctx.db, ctx.dtype = taps, x.shape[-1], bool(db), x.dtype
        ctx.save_for_backward(peak, index, sign)
        return dbtp(peak) if db else peak

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        peak, index, sign = ctx.saved_tensors
        if ctx.db:
            g = g * (8.685889638065035 / peak)                   # 20 / ln 10
        return ops.true_peak_backward(g, sign, index, ctx.taps, ctx.L).to(ctx.dtype), None, None


class FFTConvolveFunction(torch.autograd.Function):
    """ops.fft_convolve(x, h, mode, block): x (..., L), h (K,) shared or with x's leading shape -> (..., n).  The forward is
    the plain route, bit for bit.  Saves x and h and nothing else: the backward rebuilds the spectra per chunk of rows and
    computes gx (conj H, anticausal, then the adjoint of framing + rfft) and gh (at_spectral_fir_corr, a shared filter's
    chunks added in ascending order in double) only where needed."""

    @staticmethod
    def forward(ctx, x, h, mode, block):
        ctx.mode, ctx.block = mode, block
        ctx.save_for_backward(x, h)
        return ops.fft_convolve(x, h, mode, block)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, h = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_h):
            return None, None, None, None
        gx, gh = ops.fft_convolve_backward(x, h, g, ctx.mode, ctx.block, need_x=need_x, need_h=need_h)
        return (gx.to(x.dtype) if need_x else None), (gh.to(h.dtype) if need_h else None), None, None


class ImpulseResponseStreamFunction(torch.autograd.Function):
    """RealtimeImpulseResponse.forward: chunk x (rows, n B), response ir (K,), its spectrum H (P, F), and the carried state --
    tail (rows, B), ring (rows, R, F) (updated in place), head -- -> (y (rows, n B), new_tail) by ops.fft_convolve_stream, bit
    for bit the plain route.  The state is a constant of the graph and the new state is not differentiable: gx is the
    offline formula over the chunk's own frames with the part that falls on the tail dropped, gh the correlation of
    [history | the chunk's frames] with gY (ops.fft_convolve_stream_backward).  Saves H; when ir requires grad also the
    chunk's frames, rows n F 8 bytes, and the history, rows (P - 1) F 8 bytes."""

    @staticmethod
    def forward(ctx, x, ir, H, tail, ring, head, B):
        need_h = ctx.needs_input_grad[1]
        ctx.B, ctx.K, ctx.x_dtype, ctx.ir_dtype = B, ir.shape[-1], x.dtype, ir.dtype
        history = ops.ring_history(ring, head, H.shape[0] - 1) if need_h else None
        res = ops.fft_convolve_stream(x, tail, ring, head, H, B, keep_spectra=need_h)
        ctx.save_for_backward(H, history, res[3] if need_h else None)
        ctx.mark_non_differentiable(res[1])
        return res[0], res[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gtail):
        H, history, X = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_h):
            return (None,) * 7
        gx, gh = ops.fft_convolve_stream_backward(g, H, ctx.B, ctx.K, history, X, need_x=need_x, need_h=need_h)
        return (gx.to(ctx.x_dtype) if need_x else None), (gh.to(ctx.ir_dtype) if need_h else None), None, None, None, None, None


# ---- the invert side: Magnitude, Polar, Cartesian, polar_to_complex, Normalize -----------------------------------------

def _inverse_bank_tables(module, device, forward=False):
    """By-column tables of a Magnitude's inverse_mel_bank TRANSPOSED on `device` (the walk of the invert's backward), or
    with forward=True those of the inverse bank itself (the polar form recomputes the magnitude with them, and only it
    has them built); None when mel=False."""
    if not module.mel:
        return None
    return _bank_cols(module, "inverse_mel_bank", device, transposed=not forward)


class MagnitudeInvertFunction(torch.autograd.Function):
    """Magnitude.invert with its backward (ops.magnitude_invert_backward): mel or not, any contrast / norm,
    keep_nyquist both ways.  Saves y; the bank tables and the Normalize statistics are constants of the graph."""

    @staticmethod
    def forward(ctx, y, module):
        ctx.tables = _inverse_bank_tables(module, y.device)
        ctx.off, ctx.sc = module._affine()
        ctx.contrast, ctx.eps, ctx.pad_last = module.contrast_mode, module._eps, not module.keep_nyquist
        ctx.save_for_backward(y)
        return module._invert_plain(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        dy = ops.magnitude_invert_backward(y, g, ctx.tables, ctx.contrast, ctx.off, ctx.sc, ctx.eps,
                                           pad_last=ctx.pad_last)
        return dy.reshape(y.shape).to(y.dtype), None


class PolarInvertFunction(torch.autograd.Function):
    """The one-pass Polar.invert (ops.polar_inverse) with its backward, the polar form of
    ops.magnitude_invert_backward: both halves of the stacked gradient from one kernel.  Saves the stacked y."""

    @staticmethod
    def forward(ctx, y, magnitude, band, m_off, m_sc, p_off, p_sc):
        ctx.t_cols = _inverse_bank_tables(magnitude, y.device)
        ctx.f_cols = _inverse_bank_tables(magnitude, y.device, forward=True)
        ctx.args = (magnitude.contrast_mode, m_off, m_sc, magnitude._eps)
        ctx.p_off, ctx.p_sc = p_off, p_sc
        ctx.save_for_backward(y)
        return ops.polar_inverse(y, band, magnitude.contrast_mode, m_off, m_sc, magnitude._eps, p_off, p_sc)

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        (y,) = ctx.saved_tensors
        dy = ops.magnitude_invert_backward(y, gX, ctx.t_cols, *ctx.args, bank_cols=ctx.f_cols, phase_offset=ctx.p_off,
                                           phase_scale=ctx.p_sc)
        return dy.reshape(y.shape).to(y.dtype), None, None, None, None, None, None


class CartesianInvertFunction(torch.autograd.Function):
    """The one-pass Cartesian.invert (ops.cartesian_inverse) with its backward.  Saves nothing."""

    @staticmethod
    def forward(ctx, y, re_off, re_sc, im_off, im_sc):
        ctx.re_sc, ctx.im_sc, ctx.shape, ctx.dtype = re_sc, im_sc, y.shape, y.dtype
        return ops.cartesian_inverse(y, re_off, re_sc, im_off, im_sc)

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        dy = ops.cartesian_inverse_backward(gX, ctx.re_sc, ctx.im_sc)
        return dy.reshape(ctx.shape).to(ctx.dtype), None, None, None, None


class PolarToComplexFunction(torch.autograd.Function):
    """ops.polar_to_complex(mag, phase) of two tensors of one shape, with gradients for whichever of the two require
    them.  Saves mag and phase."""

    @staticmethod
    def forward(ctx, mag, phase):
        ctx.save_for_backward(mag, phase)
        return ops.polar_to_complex(mag, phase)

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        mag, phase = ctx.saved_tensors
        need_mag, need_phase = ctx.needs_input_grad
        gmag, gphase = ops.polar_to_complex_backward(gX, mag, phase, need_mag, need_phase)
        return (gmag.reshape(mag.shape).to(mag.dtype) if need_mag else None,
                gphase.reshape(phase.shape).to(phase.dtype) if need_phase else None)


class AffineInvertFunction(torch.autograd.Function):
    """Normalize.invert, x * scale + offset (ops.affine, inverse): the invert of Real / Imaginary / Phase before their
    zero pad.  The gradient is g * scale -- the same kernel with a zero offset.  Saves nothing."""

    @staticmethod
    def forward(ctx, x, offset, scale):
        ctx.scale, ctx.dtype = scale, x.dtype
        return ops.affine(x, offset, scale, inverse=True)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.affine(g, torch.zeros_like(ctx.scale), ctx.scale, inverse=True).to(ctx.dtype), None, None


# ---- the forward of the phase-side representations: Normalize, Phase / IF, Cartesian, Polar, PolarIF ---------------------

class AffineForwardFunction(torch.autograd.Function):
    """Normalize.forward, (x - offset) / scale (ops.affine): Real / Imaginary behind torch's own .real / .imag, and the
    single-frame central IF.  The gradient is g / scale -- the same kernel with a zero offset.  Saves nothing."""

    @staticmethod
    def forward(ctx, x, offset, scale):
        ctx.scale, ctx.dtype = scale, x.dtype
        return ops.affine(x, offset, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.affine(g, torch.zeros_like(ctx.scale), ctx.scale).to(ctx.dtype), None, None


class PhaseScanFunction(torch.autograd.Function):
    """ops.phase_scan of a complex spectrum X (..., T, F) for any mode, frame weight and Normalize affine, with its
    backward (ops.phase_scan_backward: unwrap's derivative is the identity, so the backward of the scan is a three-row
    stencil and the angle's derivative).  Saves X; the window and the Normalize statistics are constants of the graph."""

    @staticmethod
    def forward(ctx, X, mode, frame_window, offset, scale):
        ctx.mode, ctx.window, ctx.scale = mode, frame_window, scale
        ctx.save_for_backward(X)
        return ops.phase_scan(X, mode, frame_window=frame_window, offset=offset, scale=scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (X,) = ctx.saved_tensors
        gX = ops.phase_scan_backward(X, ctx.mode, g, ctx.window, ctx.scale)
        return gX.reshape(X.shape).to(X.dtype), None, None, None, None


class CartesianFunction(torch.autograd.Function):
    """The one-pass Cartesian.forward (ops.cartesian_forward) with its backward.  Saves nothing."""

    @staticmethod
    def forward(ctx, X, re_off, re_sc, im_off, im_sc):
        ctx.re_sc, ctx.im_sc, ctx.shape, ctx.dtype = re_sc, im_sc, X.shape, X.dtype
        return ops.cartesian_forward(X, re_off, re_sc, im_off, im_sc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gX = ops.cartesian_forward_backward(g, ctx.re_sc, ctx.im_sc)
        return gX.reshape(ctx.shape).to(ctx.dtype), None, None, None, None


def _stacked_grad(module, X, dF, mode, frame_window, phase_scale, inplace=False):
    """Gradient of a stacked (..., T, 2, F) Polar / PolarIF tensor with respect to the spectrum X: the scan backward reads
    the phase half of dF where it lies, the Magnitude backward handles the magnitude half and adds the two.
    inplace=True: the sum is formed in the Magnitude backward's result (the audio-only chain, whose X is a scratch)."""
    dF = dF if dF.is_contiguous() else dF.contiguous()
    if inplace:
        dX = _magnitude_grad(module, X, dF[..., 0, :])
        return ops.phase_scan_backward(X, mode, dF[..., 1, :], frame_window, phase_scale, accum=dX, out=dX)
    gX = ops.phase_scan_backward(X, mode, dF[..., 1, :], frame_window, phase_scale)
    return _magnitude_grad(module, X, dF[..., 0, :], dx_accum=gX)


class PolarFunction(torch.autograd.Function):
    """The one-pass Polar.forward (ops.polar_forward: banded Magnitude next to a plain Phase, stacked on dim -2) with its
    backward.  Saves X."""

    @staticmethod
    def forward(ctx, X, magnitude, band, m_off, m_sc, p_off, p_sc):
        ctx.magnitude, ctx.p_sc = magnitude, p_sc
        ctx.save_for_backward(X)
        return ops.polar_forward(X, band, magnitude.contrast_mode, m_off, m_sc, magnitude._eps, p_off, p_sc)

    @staticmethod
    @once_differentiable
    def backward(ctx, dF):
        (X,) = ctx.saved_tensors
        dX = _stacked_grad(ctx.magnitude, X, dF, "angle", None, ctx.p_sc)
        return dX.reshape(X.shape).to(X.dtype), None, None, None, None, None, None


class PolarIFFunction(torch.autograd.Function):
    """The in-place PolarIF.forward (ops.polarif_forward, either of its internal routes) with its backward.  Saves X."""

    @staticmethod
    def forward(ctx, X, magnitude, band, m_off, m_sc, method, frame_window, p_off, p_sc):
        ctx.magnitude, ctx.method, ctx.window, ctx.p_sc = magnitude, method, frame_window, p_sc
        ctx.save_for_backward(X)
        return ops.polarif_forward(X, band, magnitude.contrast_mode, m_off, m_sc, magnitude._eps, method, frame_window,
                                   p_off, p_sc)

    @staticmethod
    @once_differentiable
    def backward(ctx, dF):
        (X,) = ctx.saved_tensors
        dX = _stacked_grad(ctx.magnitude, X, dF, ctx.method, ctx.window, ctx.p_sc)
        return dX.reshape(X.shape).to(X.dtype), None, None, None, None, None, None, None, None


class StftPolarFunction(torch.autograd.Function):
    """The fused STFT -> Polar forward (ops.stft_polar_forward) with its backward.  Saves the audio only, as MfccFunction:
    the fused forward never writes a spectrum, so the backward rebuilds it from the audio a chunk of clips at a time
    (mfcc_chunk_clips), runs the Magnitude backward on it, adds the phase half's gradient in place
    (ops.phase_scan_backward) and runs the STFT adjoint into the chunk's rows of dx."""

    @staticmethod
    def forward(ctx, x, stage, magnitude, m_off, m_sc, p_off, p_sc):
        ctx.stage, ctx.magnitude, ctx.p_sc = stage, magnitude, p_sc
        ctx.save_for_backward(x)
        return ops.stft_polar_forward(x, stage.window[:1024], magnitude._banded(), magnitude.contrast_mode, m_off, m_sc,
                                      magnitude._eps, p_off, p_sc)

    @staticmethod
    @once_differentiable
    def backward(ctx, dF):
        (x,) = ctx.saved_tensors
        stage = ctx.stage
        n, hop = stage._n_fft, stage._hop
        window = stage.window[:n]
        xb = ops._f32c(x)
        B, L = xb.shape
        T = 1 + L // hop
        dF = ops._f32c(dF)
        dx = torch.empty((B, L), dtype=torch.float32, device=x.device)
        chunk = mfcc_chunk_clips(B, T, n)
        for b0 in range(0, B, chunk):
            X = ops.stft_forward(xb[b0:b0 + chunk], window, n, hop, center=True)
            dX = _stacked_grad(ctx.magnitude, X, dF[b0:b0 + chunk], "angle", None, ctx.p_sc, inplace=True)
            ops.stft_backward(dX, window, n, hop, L, out=dx[b0:b0 + chunk])
            del X, dX
        return dx.to(x.dtype), None, None, None, None, None, None


# ---- the streaming path: OverlapAdd, RealtimeSTFT, RealtimeDGT ------------------------------------------------------------

class RtStftFunction(torch.autograd.Function):
    """RealtimeSTFT / RealtimeDGT.forward of frames x (..., n_fft) -- dense, or an overlapping frame() view --
    -> rfft(x * window) (..., F) complex64, with the frame-analysis adjoint as backward: a DENSE gradient of x's logical
    shape (torch's own as_strided backward folds it when x is a view).  Saves nothing but x's shape and type."""

    @staticmethod
    def forward(ctx, x, module):
        ctx.window, ctx.n_fft, ctx.shape, ctx.dtype = module.window[:module._n_fft], module._n_fft, x.shape, x.dtype
        return module._rt_forward(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        gx = ops.rfft_frames_backward(G, ctx.window, ctx.n_fft)
        return gx.reshape(ctx.shape).to(ctx.dtype), None


class RtIstftFunction(torch.autograd.Function):
    """X (..., n, F) complex -> ops.irfft_frames(X), the windowed frames, with the frame-synthesis adjoint as backward."""

    @staticmethod
    def forward(ctx, X, inv_window, n_fft):
        ctx.inv_window, ctx.n_fft, ctx.shape, ctx.dtype = inv_window, n_fft, X.shape, X.dtype
        return ops.irfft_frames(X, inv_window, n_fft)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gX = ops.irfft_frames_backward(g, ctx.inv_window, ctx.n_fft)
        return gX.reshape(ctx.shape).to(ctx.dtype), None, None


class RtIstftPolarFunction(torch.autograd.Function):
    """ops.irfft_frames(mag e^{i phase}) for a magnitude mag (..., n, F) and a constant phase: the gradient of mag is
    Re(gX e^{-i phase}), the phase gets none.  mag_hist given (RealtimeDGT): the same fused ops.rt_polar_irfft_update as
    the plain route, whose refreshed PGHI history comes back as two non-differentiable outputs (empty tensors
    otherwise).  Saves the phase as the kernel read it."""

    @staticmethod
    def forward(ctx, mag, phase, inv_window, n_fft, mag_hist):
        phase = ops._f32c(phase.detach())
        if phase.shape != mag.shape:
            phase = phase.expand_as(mag).contiguous()
        ctx.inv_window, ctx.n_fft, ctx.phase, ctx.dtype = inv_window, n_fft, phase, mag.dtype
        if mag_hist is not None:
            frames, hist, prev = ops.rt_polar_irfft_update(mag, phase, inv_window, n_fft, mag_hist.detach())
        else:
            frames = ops.irfft_frames(None, inv_window, n_fft, mag=mag, phase=phase)
            hist, prev = mag.new_empty(0), mag.new_empty(0)
        ctx.mark_non_differentiable(hist, prev)
        ctx.set_materialize_grads(False)
        return frames, hist, prev

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _ghist, _gprev):
        if g is None:
            return None, None, None, None, None
        gmag = ops.irfft_frames_backward(g, ctx.inv_window, ctx.n_fft, phase=ctx.phase)
        return gmag.to(ctx.dtype), None, None, None, None


class OaddFramesFunction(torch.autograd.Function):
    """OverlapAdd.forward of a chunk x (S, C) behind a constant history (S, keep) or None: the frames, the same zero-copy
    strided view of [history | chunk | zero pad] as the plain route (shaped lead + (n, n_fft)), and the next history
    (non-differentiable).  Its backward receives a dense gradient of the view's logical shape and sums, for every chunk
    sample, the frames that cover it; the history's share is dropped."""

    @staticmethod
    def forward(ctx, x, hist, module, lead):
        keep, n_fft, hop = module._keep, module._n_fft, module._hop
        buf, new_hist, nw = ops.oadd_forward(x, hist, keep, n_fft, hop)
        ctx.args, ctx.dtype = (n_fft, hop, keep, x.shape[-1]), x.dtype
        ctx.mark_non_differentiable(new_hist)
        ctx.set_materialize_grads(False)
        return module._frames_view(buf, nw, lead), new_hist

    @staticmethod
    @once_differentiable
    def backward(ctx, gframes, _ghist):
        if gframes is None:
            return None, None, None, None
        g3 = gframes.reshape((-1,) + tuple(gframes.shape[-2:]))
        return ops.oadd_forward_backward(g3, *ctx.args).to(ctx.dtype), None, None, None


class OaddInvertFunction(torch.autograd.Function):
    """OverlapAdd.invert of frames (S, n, n_fft) on a constant tail (S, keep) or None -> (out, new tail); the tail is
    non-differentiable.  The gradient of a frame is gy / gain where the frame reaches this call's output and exactly 0
    where it only reaches the new tail."""

    @staticmethod
    def forward(ctx, frames, tail, module):
        n_fft, hop, keep, gain = module._n_fft, module._hop, module._keep, module.gain_compensation
        ctx.args, ctx.dtype = (frames.shape[-2], n_fft, hop, keep, gain), frames.dtype
        out, new_tail = ops.oadd_invert(frames, tail, n_fft, hop, keep, gain)
        ctx.mark_non_differentiable(new_tail)
        ctx.set_materialize_grads(False)
        return out, new_tail

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gtail):
        if gy is None:
            return None, None, None
        return ops.oadd_invert_backward(gy, *ctx.args).to(ctx.dtype), None, None

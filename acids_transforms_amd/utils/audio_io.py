"""Audio front end of the reference's examples and tests: `import_data` (utils/misc.py:29-59) and the sample-rate
conversion it applies (`torchaudio.transforms.Resample`, default arguments).

torchaudio is not part of the reference tree (requirements.txt:3, unpinned) and is absent from this image, so
  * wav files are decoded with scipy.io.wavfile and normalised the way `torchaudio.load(normalize=True)` does
    (integer PCM divided by its full scale, float left alone), channels first;
  * Resample restates torchaudio's published algorithm (`_get_sinc_resample_kernel` /
    `_apply_sinc_resample_kernel`: Hann-windowed sinc polyphase bank built in float64, zero padding by `width`
    in front and `width + orig` behind, output cropped to ceil(new * L / orig)) -- **parity unpinned**;
    the convolution itself is resample.hip.
`import_data` keeps the reference's quirks: files inside a directory are always brought to 44100 Hz (the
recursive call drops `sr`), a folder with any stereo file turns every clip stereo (mono is duplicated), clips are
zero-padded to the longest one, and files that fail to load are skipped silently.
"""
import math
import os

import numpy as np
import torch

from .. import ops
from .._lib import device_scoped, require_device
from ..autograd import ResampleDirectFunction, ResampleFunction, ResampleStreamFunction, wants_grad
from ..transforms.carried import CarriedState

__all__ = ["Resample", "RealtimeResample", "resample", "import_data", "load_wav"]


def sinc_filter_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(filters (new, 2*width + orig) float32, width, orig, new) for rates already divided by their gcd."""
    base_freq = min(orig_freq, new_freq) * rolloff
    width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
    idx = torch.arange(-width, width + orig_freq, dtype=torch.float64)[None, :] / orig_freq
    t = torch.arange(0, -new_freq, -1, dtype=torch.float64)[:, None] / new_freq + idx
    t = (t * base_freq).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base_freq / orig_freq
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels = kernels * window * scale
    return kernels.to(torch.float32).contiguous(), width


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its default interpolation.

    Differentiable: when grad mode is on and the waveform requires grad the call goes through
    autograd.ResampleFunction -- the same forward kernel, to the bit, and the transposed polyphase filter backward
    (at_resample_sinc_backward; first order only, the graph keeps no tensor).  `streaming()` is the causal form.

    `direct=True` builds no bank: the module keeps the converter's half-table (`table`, ops.sinc_table: a few KB where
    the bank has new x (2 width + orig) entries, so any pair of rates is affordable) and both passes are sinc_interp.hip,
    which walks only the taps of a bank row that are not zero -- for finite input the same bits, forward and backward.
    It has no streaming form."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, direct: bool = False):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = lowpass_filter_width, rolloff
        self.direct = bool(direct)
        g = math.gcd(self.orig_freq, self.new_freq)
        self.orig, self.new = self.orig_freq // g, self.new_freq // g
        if self.orig != self.new and self.direct:
            table, self.Qi = ops.sinc_table(self.orig, self.new, lowpass_filter_width, rolloff)
            self.register_buffer("table", table, persistent=False)
        elif self.orig != self.new:
            bank, self.width = sinc_filter_bank(self.orig, self.new, lowpass_filter_width, rolloff)
            self.register_buffer("kernel", bank, persistent=False)

    def _forward_direct(self, waveform: torch.Tensor) -> torch.Tensor:
        lead, L = tuple(waveform.shape[:-1]), waveform.shape[-1]
        x = waveform.reshape(math.prod(lead), L)
        out_len = -(-self.new * L // self.orig)
        if wants_grad(waveform):
            y = ResampleDirectFunction.apply(x, self.table.to(x.device), self.Qi, self.orig, self.new)
        else:
            y = ops.sinc_interp(x, self.orig, self.new, self.table.to(x.device), self.Qi, out_len)
        return y if waveform.ndim == 2 else y.reshape(lead + (out_len,))

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        if self.orig == self.new:
            return waveform
        if self.direct:
            return self._forward_direct(waveform)
        lead = waveform.shape[:-1]
        x = waveform.reshape(-1, waveform.shape[-1])
        if wants_grad(waveform):
            y = ResampleFunction.apply(x, self.kernel.to(x.device), self.orig, self.new, self.width)
        else:
            y = ops.resample_sinc(x, self.orig, self.new, self.width, self.kernel.to(x.device))
        # (rows, L) audio gets the node itself back (its grad_fn names ResampleFunction), not a view of it
        return y if waveform.ndim == 2 else y.reshape(tuple(lead) + (y.shape[-1],))

    def streaming(self) -> "RealtimeResample":
        """The causal form of this converter: a RealtimeResample that shares this module's bank."""
        if self.direct:
            raise ValueError("Resample(direct=True) has no streaming form: build the module with direct=False")
        rt = RealtimeResample(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
        if self.orig != self.new:
            rt._buffers["kernel"] = self.kernel
            rt = rt.to(self.kernel.device)
        return rt


class RealtimeResample(CarriedState, Resample):
    """The converter made causal by a delay of D = ceil(width / orig) whole blocks, with the last Ha = D orig + width
    input samples carried in `input_buffer` (lead..., Ha).

    `forward` takes the next (..., C) chunk of a stream, C a multiple of `orig` down to one block, and returns
    (..., C new / orig): out[t new + j] = sum_k h[j][k] v[t orig + k] over v = [input_buffer | chunk].  Output block t of
    the stream is offline block t - D with zeros before the stream's start, so the outputs of ANY chunking of x (..., L)
    concatenate to Resample(cat([zeros(D orig), x], -1))[..., :L new / orig] -- for finite input to the bit: the kernel
    is the offline chain reading another source, and the offline call's zero padding behind the clip is never reached
    (D orig >= width).  The next state is written by the same launch into a second buffer that replaces the module's:
    no torch.cat, one launch per call.  The state is zeros on a new leading batch shape or device and after `reset()`, and
    float32 whatever a module cast (`.double()`, `.half()`) made of the buffer (transforms.carried.CarriedState).  The bank
    is read as float32 too: exactly after `.double()`; after `.half()` it keeps the precision of the fp16 values the cast
    left, as RealtimePQMF's tables do.

    `delay` is D orig input samples (`output_delay` = D new output samples), `ratio` = new / orig.

    Gradients (autograd.ResampleStreamFunction): the carried state is a constant of the graph and is stored detached, so
    a chunk's gradient covers that chunk's own samples -- truncated back-propagation at chunk boundaries, as for
    OverlapAdd and RealtimePQMF.  Not built: chunks that are not whole blocks, gradient through the carried state, a
    hipGraph-captured session (the state buffer changes place every call)."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, direct: bool = False):
        if direct:
            raise ValueError("RealtimeResample has no direct (bankless) form: the streaming kernel reads the bank")
        super().__init__(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.delay_blocks, self._keep = (0, 0) if self.orig == self.new else ops.resample_stream_sizes(self.orig, self.width)
        self.register_buffer("input_buffer", torch.zeros(self._keep))
        self._carries("input_buffer")

    @property
    def delay(self) -> int:
        """Input samples by which `forward` lags the offline converter."""
        return self.delay_blocks * self.orig

    @property
    def output_delay(self) -> int:
        """The same delay in output samples."""
        return self.delay_blocks * self.new

    @property
    def ratio(self) -> float:
        return self.new / self.orig

    def streaming(self) -> "RealtimeResample":
        return self

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        if waveform.ndim < 1 or waveform.shape[-1] % self.orig:
            raise ValueError("RealtimeResample.forward takes a (..., C) chunk with C a multiple of orig = %d, got shape %s"
                             % (self.orig, tuple(waveform.shape)))
        if self.orig == self.new:
            return waveform
        ops._no_fp64(waveform)
        device_scoped(require_device)(waveform)
        lead, C = tuple(waveform.shape[:-1]), waveform.shape[-1]
        out_c = C // self.orig * self.new
        if waveform.numel() == 0:                                 # nothing arrived: no launch, the state stays
            return torch.empty(lead + (out_c,), dtype=torch.float32, device=waveform.device)
        (state,) = self._carried_rows(("input_buffer",), lead, waveform) or (None,)
        bank = self.kernel.to(waveform.device, torch.float32)     # float32 again after module.double() / .half()
        x = waveform.reshape(math.prod(lead), C)
        if wants_grad(waveform):
            y, new_state = ResampleStreamFunction.apply(x, state, bank, self.orig, self.new, self.width)
        else:
            y, new_state = ops.resample_sinc_stream(x, state, self.orig, self.new, self.width, bank)
        self._carry("input_buffer", new_state, lead)
        return y if waveform.ndim == 2 else y.reshape(lead + (out_c,))


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    return Resample(orig_freq, new_freq)(waveform)


def load_wav(path: str):
    """(waveform (channels, samples) float32 in [-1, 1), sample rate)."""
    from scipy.io import wavfile
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sr, a = wavfile.read(path)
    a = np.asarray(a)
    if a.ndim == 1:
        a = a[:, None]
    if a.dtype == np.uint8:
        x = (a.astype(np.float32) - 128.0) / 128.0
    elif np.issubdtype(a.dtype, np.integer):
        x = a.astype(np.float32) / float(2 ** (8 * a.dtype.itemsize - 1))
    else:
        x = a.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.T)), int(sr)


def import_data(path: str, sr=44100, device=None):
    """File: (waveform (C, L) at `sr`, file name).  Directory: (stacked (N, C, Lmax) clips, names).
    Resampling runs on the GPU (`device`, default the current ROCm device); results come back on the CPU like
    the reference's unless `device` is given."""
    if os.path.isfile(path):
        x, sr_file = load_wav(path)
        if sr_file != sr:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            x = Resample(sr_file, sr)(x.to(dev))
            if device is None:
                x = x.cpu()
        elif device is not None:
            x = x.to(device)
        return x, os.path.basename(path)
    if os.path.isdir(path):
        data, names = [], []
        for f in os.listdir(path):
            try:
                x, n = import_data("%s/%s" % (path, f), device=device)      # sr not forwarded: always 44100
                data.append(x)
                names.append(os.path.splitext(os.path.basename(n))[0])
            except Exception:
                pass
        max_size = max(d.shape[1] for d in data)
        stereo = 2 in [d.shape[0] for d in data]
        for i, d in enumerate(data):
            if d.shape[0] > 1:
                d = d if stereo else d[0].unsqueeze(0)
            else:
                d = torch.cat([d, d]) if stereo else d
            if d.shape[1] <= max_size:
                d = torch.cat([d, torch.zeros(d.shape[0], max_size - d.shape[1], dtype=d.dtype, device=d.device)], 1)
            data[i] = d
        return torch.stack(data), names
    raise FileNotFoundError(path)

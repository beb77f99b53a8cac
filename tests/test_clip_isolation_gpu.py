"""No clip leaks into its neighbour where frames share one FFT (n_fft 128 / 256 / 512).

At these sizes K = 8 / 4 / 2 frames go through ONE 512-point register FFT (csrc/stft_small.hip, csrc/stft512.hip).  The
groups are formed per clip (shared_fft_cases.py; its geometry and the float32 model behind the inputs are checked on
the CPU by test_shared_fft_cases_cpu.py), so for every route that reaches those kernels this file holds:

  a. bits      -- clip b inside a batch is torch.equal to the same clip run as a batch of one (first / middle / last);
  b. accuracy  -- on a batch whose clips alternate between randn * 0.1 and randn * 1e-5 (80 dB), every clip meets the
                  project's bar against the float64 oracle relative to ITS OWN maximum (rel_max_per_clip; conftest.rel_max
                  divides by the maximum of the whole tensor, behind which a wrong quiet clip hides);
  c. non-finite -- a NaN or Inf sample in one clip leaves every other clip finite and bit-identical to the launch with
                  the bad clips zeroed, and is never lost in the clip that owns it.

Within ONE clip frames still share transforms: a frame's rounding and a NaN reach the up to K - 1 frames of its group
(documented deviations); 2c asserts exactly that set.  With launch-wide groups (f = K g + r over all
B T frames, the kernels until this file existed) a, b and c fail at every T % K != 0.

Measured on an MI355X (worst per-clip error of each route, printed by the tests): see DESIGN section 5."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import shared_fft_cases as S
from acids_transforms_amd import ops
from acids_transforms_amd._lib import VARIANTS, check, lib, ptr, stream_ptr, variant
from acids_transforms_amd.streaming import StreamingDGTSession
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5              # forward, complex inverse, mel features
TOL_POLAR = 2e-5        # polar inverse (test_register_core_sizes_512_and_2048)
LOUD, QUIET = 0.1, 1e-5
GUARD = 256
SENTINEL = -7777.0
NFFTS = (128, 256, 512)
KINDS = ("stft", "dgt")


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def _variants_back_to_default():
    yield
    assert all(lib().at_get_variant(w) == 0 for w in VARIANTS.values())


def module(kind, n_fft, hop, dev):
    m = (A.STFT if kind == "stft" else A.DGT)(n_fft=n_fft, hop_length=hop)
    return m.to(dev)


def realtime(kind, n_fft, hop, dev, S_):
    m = A.RealtimeSTFT(n_fft=n_fft, hop_length=hop) if kind == "stft" else A.RealtimeDGT(n_fft=n_fft, hop_length=hop,
                                                                                        batch_size=S_)
    return m.to(dev)


def gains(B, loud=LOUD, quiet=QUIET):
    """Clips alternate loud / quiet; the clip in the middle of a batch of five is loud, its neighbours quiet."""
    g = torch.full((B,), loud)
    g[1::2] = quiet
    return g


def audio(B, L, seed, loud=LOUD, quiet=QUIET):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, generator=g) * gains(B, loud, quiet)[:, None]


def spectra(B, T, F, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g))
    return X * gains(B)[:, None, None]


def same_rows(batch, single, B, what):
    """2a: `single(b)` runs clip b as a batch of one."""
    batch = batch if isinstance(batch, tuple) else (batch,)
    for b in S.tested_clips(B):
        one = single(b)
        one = one if isinstance(one, tuple) else (one,)
        for full, alone in zip(batch, one):
            assert alone.shape[0] == 1
            assert torch.equal(full[b], alone[0]), (what, "clip %d of %d differs from the batch of one" % (b, B))


class Worst:
    """Worst per-clip error of a route, loud and quiet clips apart; printed, then asserted."""

    def __init__(self, what, tol):
        self.what, self.tol, self.loud, self.quiet, self.at = what, tol, 0.0, 0.0, None

    def add(self, got, want, where):
        per = S.rel_max_per_clip(cpu(got) if torch.is_tensor(got) else got, want)
        lo, qu = float(per[0::2].max()), float(per[1::2].max()) if len(per) > 1 else 0.0
        if max(lo, qu) > max(self.loud, self.quiet):
            self.at = where
        self.loud, self.quiet = max(self.loud, lo), max(self.quiet, qu)

    def check(self):
        print("%-46s worst per-clip error: loud clips %.2e, quiet clips %.2e (bar %.0e) at %s"
              % (self.what, self.loud, self.quiet, self.tol, self.at))
        assert max(self.loud, self.quiet) < self.tol, (self.what, self.loud, self.quiet, self.at)


def framed(x, n_fft, hop, T):
    return x.unfold(-1, n_fft, hop)[:, :T]


# ---- forward ------------------------------------------------------------------------------------------------------------
def forward_call(m, x, n_fft, hop, center, T, L):
    if center:
        return m(x)
    return ops.stft_forward(x, m.window[:n_fft], n_fft, hop, center=False, T=T, clip_stride=x.stride(0), L=L, B=x.shape[0])


def forward_ref(m, x, n_fft, hop, center, T):
    w = m.window[:n_fft].cpu().double()
    if center:
        return O.stft_forward(x.double(), w, n_fft, hop).numpy()
    return O.rt_forward(framed(x.double(), n_fft, hop, T), w).numpy()


@pytest.mark.parametrize("n_fft", NFFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_every_geometry(dev, kind, n_fft):
    """STFT / DGT forward (center=True, torch.stft's framing) and ops.stft_forward(center=False) with explicit
    T / clip_stride / L: every T % K, every T < K, hops n/4, n/8, n/2 and one that does not divide n_fft, a launch whose
    workgroups take more than WS groups.  At n_fft 512 the hop-128 center=True cases take the sliding kernel (a control)."""
    worst = Worst("%s forward n_fft %d" % (kind, n_fft), TOL)
    for i, (B, T, hop, center, L) in enumerate(S.forward_cases(n_fft)):
        m = module(kind, n_fft, hop, dev)
        xc = audio(B, L, 1000 * n_fft + i)
        x = xc.to(dev)
        X = forward_call(m, x, n_fft, hop, center, T, L)
        assert X.shape == (B, T, n_fft // 2 + 1)
        same_rows(X, lambda b: forward_call(m, x[b:b + 1].contiguous(), n_fft, hop, center, T, L), B, (kind, n_fft, B, T, hop, center))
        worst.add(X, forward_ref(m, xc, n_fft, hop, center, T), (B, T, hop, center))
    worst.check()


@pytest.mark.parametrize("n_fft", NFFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_with_phase_output(dev, kind, n_fft):
    """eager_phase=True: spectrum and phase from the forward kernel (n_fft 512: off the sliding kernel at hop 128)."""
    K = S.K_OF[n_fft]
    worst = Worst("%s forward + phase n_fft %d" % (kind, n_fft), TOL)
    for T in (K + 1, 2 * K + 1, 2 * K + 3, 3):
        hop, L = S.center_shape(n_fft, T, n_fft // 4)
        m = module(kind, n_fft, hop, dev)
        m.eager_phase = True
        xc = audio(S.B_SWEEP, L, 77 * n_fft + T)
        x = xc.to(dev)

        def run(xx):
            X = m(xx)
            return X, m.phase_buffer.clone()
        X, ph = run(x)
        assert ph.shape == X.shape and bool(torch.isfinite(ph).all())
        same_rows((X, ph), lambda b: run(x[b:b + 1]), S.B_SWEEP, (kind, n_fft, T, "phase"))
        worst.add(X, forward_ref(m, xc, n_fft, hop, True, T), (T, hop))
    worst.check()


def guarded(n, fn, dev, offset=0, complex_out=False):
    """fn(out) into n floats pre-filled with NaN between guard bands, `offset` floats off the 1 KB alignment."""
    buf = torch.full((n + 2 * GUARD + offset,), SENTINEL, dtype=torch.float32, device=dev)
    lo = GUARD + offset
    buf[lo:lo + n] = float("nan")
    out = buf[lo:lo + n]
    fn(out)
    assert bool((torch.cat([buf[:lo], buf[lo + n:]]) == SENTINEL).all()), "guard band written"
    res = out.clone()
    assert not bool(torch.isnan(res).any()), "element left unwritten"
    return torch.view_as_complex(res.view(-1, 2)) if complex_out else res


# the conditions of launch_stft512_fwd that the swept shapes do not give (test_shared_fft_cases_cpu.py lists them)
DISPATCH_EXTRA = ("L_lt_512", "odd_clip_stride", "unaligned_input", "unaligned_output", "variant_frame_kernels")


@pytest.mark.parametrize("reason", DISPATCH_EXTRA)
def test_forward_512_every_dispatch_condition(dev, reason):
    """n_fft 512, hop 128, center=True leaves the sliding kernel for stft512_fwd_kernel when L < 512, the clip stride is
    odd, the input is not 8-byte or the output not 512-byte aligned, or variant frame_kernels is set.  Odd T, so a pair
    of launch-wide frames would straddle two clips.  The frame_kernels result is held to the sliding kernel's at 1e-5 as
    well (two kernels: equal bits are not claimed)."""
    n, hop, B, F = 512, 128, S.B_SWEEP, 257
    L = 300 if reason == "L_lt_512" else 128 * 6 + 4                  # T = 3 / 7
    T = 1 + L // hop
    assert T % 2 == 1
    w = torch.hann_window(n, device=dev)
    xc = audio(B, L, 512 + len(reason))
    stride = L + 1 if reason == "odd_clip_stride" else L
    assert reason != "odd_clip_stride" or stride % 2 == 1
    off_in = 1 if reason == "unaligned_input" else 0
    off_out = 2 if reason == "unaligned_output" else 0
    kw = dict(L=L, clip_stride_odd=stride % 2 == 1, x_aligned=not off_in, out_aligned=not off_out,
              frame_kernels=reason == "variant_frame_kernels")
    assert S.forward_kernel(n, hop, **kw) == "stft512_fwd_kernel" and S.forward_reason(n, hop, **kw) == {reason}

    def run(xs):
        b = xs.shape[0]
        store = torch.zeros(b * stride + off_in + 2, device=dev)
        x = store[off_in:off_in + b * stride].view(b, stride)
        x[:, :L] = xs
        assert (x.data_ptr() % 8 != 0) == bool(off_in)

        def fn(out):
            assert (out.data_ptr() % 512 != 0) == bool(off_out)
            check(lib().at_stft_forward(ptr(x), b, L, stride, T, n, hop, 1, ptr(w), ptr(out), None, stream_ptr()),
                  "at_stft_forward")
        with variant("frame_kernels", int(reason == "variant_frame_kernels")):
            return guarded(b * T * F * 2, fn, dev, offset=off_out, complex_out=True).view(b, T, F)
    x = xc.to(dev)
    X = run(x)
    same_rows(X, lambda b: run(x[b:b + 1]), B, reason)
    ref = O.stft_forward(xc.double(), torch.hann_window(n, dtype=torch.float64), n, hop).numpy()
    worst = Worst("n_fft 512 forward, %s" % reason, TOL)
    worst.add(X, ref, (B, T))
    if reason == "variant_frame_kernels":
        sliding = ops.stft_forward(x, w, n, hop)
        worst.add(X, cpu(sliding).astype(np.complex128), "against the sliding kernel")
    worst.check()


# ---- pre-framed input: the realtime classes -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", NFFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_realtime_forward_and_invert(dev, kind, n_fft):
    """RealtimeSTFT / RealtimeDGT on (S, n, n_fft) frames and (S, n, F) spectra: a stream's frames alone against the
    same stream among others, 1 and 5 frames per stream and every n of the sweep.  invert: complex input, and polar input
    through ops.irfft_frames with phases near 3e4 rad."""
    F = n_fft // 2 + 1
    wf = Worst("%s realtime forward n_fft %d" % (kind, n_fft), TOL)
    wi = Worst("%s realtime invert n_fft %d" % (kind, n_fft), TOL)
    wp = Worst("%s realtime polar invert n_fft %d" % (kind, n_fft), TOL_POLAR)
    for i, (S_, n) in enumerate(S.frames_cases(n_fft)):
        m = realtime(kind, n_fft, n_fft // 4, dev, S_)
        fc = audio(S_, n * n_fft, 31 * n_fft + i).view(S_, n, n_fft)
        fr = fc.to(dev)
        X = m(fr)
        assert X.shape == (S_, n, F)
        same_rows(X, lambda b: m(fr[b:b + 1]), S_, (kind, n_fft, S_, n, "forward"))
        wf.add(X, O.rt_forward(fc.double(), m.window[:n_fft].cpu().double()).numpy(), (S_, n))
        Xc = spectra(S_, n, F, 57 * n_fft + i)
        Xd = Xc.to(dev)
        y = m.invert(Xd)
        assert y.shape == (S_, n, n_fft)
        same_rows(y, lambda b: m.invert(Xd[b:b + 1]), S_, (kind, n_fft, S_, n, "invert"))
        iw = m.inv_window[:n_fft].cpu().double()
        wi.add(y, O.rt_invert(Xc.to(torch.complex128), iw).numpy(), (S_, n))
        g = torch.Generator().manual_seed(i)
        mag = Xc.abs()
        phase = 3e4 + 6.28 * torch.rand(S_, n, F, generator=g)
        magd, phd = mag.to(dev), phase.to(dev)
        yp = ops.irfft_frames(None, m.inv_window[:n_fft], n_fft, mag=magd, phase=phd)
        same_rows(yp, lambda b: ops.irfft_frames(None, m.inv_window[:n_fft], n_fft, mag=magd[b:b + 1], phase=phd[b:b + 1]),
                  S_, (kind, n_fft, S_, n, "polar"))
        Xp = mag.double() * torch.exp(1j * phase.double())
        wp.add(yp, O.rt_invert(Xp, iw).numpy(), (S_, n))
        # ops.irfft_frames, complex: the route the modules take, called directly
        assert torch.equal(ops.irfft_frames(Xd, m.inv_window[:n_fft], n_fft), y)
    wf.check()
    wi.check()
    wp.check()


# ---- inverse ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", NFFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_invert_every_geometry(dev, kind, n_fft):
    """STFT / DGT invert from complex input and _istft(mag=, phase=) polar input with phases near 3e4 rad: the frames
    kernel in front of the gather (n_fft 128 / 256 at every hop, n_fft 512 at the hop that does not divide it); the fused
    n_fft-512 kernel at hops 64 / 128 / 256 runs through the same checks as a control."""
    F = n_fft // 2 + 1
    wc = Worst("%s invert n_fft %d" % (kind, n_fft), TOL)
    wp = Worst("%s polar invert n_fft %d" % (kind, n_fft), TOL_POLAR)
    for i, (B, T, hop) in enumerate(S.inverse_cases(n_fft)):
        m = module(kind, n_fft, hop, dev)
        iw = m.inv_window[:n_fft].cpu().double()
        Xc = spectra(B, T, F, 91 * n_fft + i)
        Xd = Xc.to(dev)
        y = m.invert(Xd)
        assert y.shape == (B, hop * (T - 1))
        same_rows(y, lambda b: m.invert(Xd[b:b + 1]), B, (kind, n_fft, B, T, hop, "complex"))
        wc.add(y, O.istft(Xc.to(torch.complex128), iw, n_fft, hop).numpy(), (B, T, hop))
        if B > S.B_SWEEP and kind == "dgt":
            continue                              # the large launch in polar form: once is enough
        g = torch.Generator().manual_seed(i)
        mag = Xc.abs()
        phase = 3e4 + 6.28 * torch.rand(B, T, F, generator=g)
        magd, phd = mag.to(dev), phase.to(dev)
        yp = m._istft(mag=magd, phase=phd)
        same_rows(yp, lambda b: m._istft(mag=magd[b:b + 1], phase=phd[b:b + 1]), B, (kind, n_fft, B, T, hop, "polar"))
        Xp = mag.double() * torch.exp(1j * phase.double())
        wp.add(yp, O.istft(Xp, iw, n_fft, hop).numpy(), (B, T, hop))
    wc.check()
    wp.check()


def test_istft_512_without_envelope_table(dev):
    """at_istft at n_fft 512, hop 128 with env16 = NULL: irfft512_frames_kernel into the workspace, then the gather."""
    n, hop, B, T, F = 512, 128, S.B_SWEEP, 7, 257
    assert S.istft_kernel(n, hop, env=False) == "irfft512_frames_kernel"
    iw = torch.hann_window(n, device=dev)
    Xc = spectra(B, T, F, 5)

    def run(Xs):
        b = Xs.shape[0]
        Xd = Xs.to(dev).contiguous()
        ws = torch.empty(b * T * n, device=dev)

        def fn(out):
            check(lib().at_istft(ptr(Xd), None, None, b, T, n, hop, ptr(iw), None, ptr(out), ptr(ws), ws.numel() * 4,
                                 stream_ptr()), "at_istft")
        return guarded(b * hop * (T - 1), fn, dev).view(b, hop * (T - 1))
    y = run(Xc)
    same_rows(y, lambda b: run(Xc[b:b + 1]), B, "istft 512 without the envelope table")
    w = Worst("n_fft 512 istft, no envelope table", TOL)
    w.add(y, O.istft(Xc.to(torch.complex128), torch.hann_window(n, dtype=torch.float64), n, hop).numpy(), (B, T))
    w.check()


# ---- mel features at n_fft 512 ------------------------------------------------------------------------------------------
def mel_ref(xc, bank, hop, power, contrast, off=None, sc=None):
    X = torch.stft(xc.double(), 512, hop, window=torch.hann_window(512, dtype=torch.float64), return_complex=True)
    mel = (X.abs() ** power).transpose(-1, -2) @ bank.double()                          # (B, T, n_mels)
    want = O.contrast(mel, contrast)
    if off is not None:
        want = (want - off) / sc
    return want


F32_MARGIN = 10      # a draw is kept if float32 torch.stft on the CPU meets the bar with this factor to spare


def mel_audio(B, L, seed, loud, quiet, bank, hop, power, contrast):
    """The alternating batch for a mel route, and its float64 reference.  The banks at n_fft 512 have filters of a
    single bin (and weights near zero at a triangle's foot), and |X_k|^2 of noise is exponentially distributed: now and
    then a band comes out 70 dB below its frame's peak, where log turns the float32 FFT's own error (a few 1e-7 of the
    frame's peak, whatever kernel computes it) into 1e-5 of the clip's maximum -- float32 torch.stft, one frame per
    transform, reaches 5e-6 on such a draw.  That measures the conditioning of log on that draw, not whether clips leak.
    So a draw is kept only if the float32 transform of the CPU (torch.stft in float32, nothing of this project) stays
    F32_MARGIN inside the bar on every clip; otherwise the next seed is taken.  The choice reads the references alone."""
    w32, eps = torch.hann_window(512), 1.1920929e-07
    for k in range(32):
        xc = audio(B, L, seed + 100000 * k, loud, quiet)
        want = mel_ref(xc, bank, hop, power, contrast).numpy()
        X32 = torch.stft(xc, 512, hop, window=w32, return_complex=True)
        m32 = (X32.abs() ** power).transpose(-1, -2) @ bank
        f32 = (torch.log1p(m32) if contrast == "log1p" else O.contrast(m32, contrast, eps)).numpy()
        if S.rel_max_per_clip(f32, want).max() * F32_MARGIN < TOL:
            return xc, want
    raise AssertionError("no well-conditioned draw in 32 seeds")


# power, contrast, loud and quiet amplitude: the quiet clips must not be flattened by the clamp at eps
MEL_CONTRASTS = [(1, None, LOUD, QUIET), (1, "log1p", LOUD, QUIET), (2, "log", 10.0, 1e-3)]


@pytest.mark.parametrize("n_mels", (40, 128))
def test_mel_features_512(dev, n_mels):
    """stft512_mel_kernel through ops.stft_mel_forward (time-major and channel-major, with and without an affine
    normalisation) under the default plan and AT_VARIANT_ROW_RUN = 1 / 3 pairs per wave, and through MFCC (channel-major,
    with and without Normalize).  Accuracy per clip without the normalisation, which would flatten the quiet clips."""
    from acids_transforms_amd.utils.banded import BandedBank
    bank = O.melscale_fbanks(257, 0.0, 22050.0, n_mels, 44100).float()
    band = BandedBank(bank)
    assert band.fusable512 and S.mel_kernel(512) == "stft512_mel_kernel"
    w = torch.hann_window(512, device=dev)
    off, sc = torch.tensor(0.375, device=dev), torch.tensor(1.625, device=dev)
    for power, contrast, loud, quiet in MEL_CONTRASTS:
        worst = Worst("mel 512 / %d power %d contrast %s" % (n_mels, power, contrast), TOL)
        for i, (B, T, hop, L) in enumerate(S.mel_cases()):
            xc, want = mel_audio(B, L, 4000 + 10 * n_mels + i, loud, quiet, bank, hop, power, contrast)
            x = xc.to(dev)
            assert all(np.ptp(want[b]) > 0.1 * np.abs(want[b]).max() for b in range(1, B, 2)), "quiet clips are flattened"
            for cm in (False, True):
                for norm in (False, True):
                    def run(xx, v):
                        with variant("row_run", v):
                            return ops.stft_mel_forward(xx, w, band, contrast, off if norm else None, sc if norm else None,
                                                        power=power, want_spectrum=False, channel_major=cm, hop=hop,
                                                        n_fft=512)[2]
                    base = run(x, 0)
                    for v in S.MEL_ROW_RUNS:
                        feat = run(x, v)
                        assert torch.equal(feat, base), ("row_run", v)
                        same_rows(feat, lambda b: run(x[b:b + 1], v), B, ("mel", n_mels, B, T, cm, norm, v))
                    if not norm:
                        got = cpu(base).transpose(0, 2, 1) if cm else cpu(base)
                        worst.add(got, want, (B, T, cm))
        worst.check()
    # the module: MFCC is the mel power spectrogram, channel-major
    for norm_mode in (None, "gaussian"):
        m = A.MFCC(n_fft=512, hop_length=128, power=2, n_mels=n_mels, norm_mode=norm_mode).to(dev)
        if norm_mode:
            m.norm.set_affine(off, sc)
        worst = Worst("MFCC 512 / 128 / %d norm %s" % (n_mels, norm_mode), TOL)
        for i, (B, T, hop, L) in enumerate(S.mel_cases()):
            if hop != 128:
                continue
            xc, want = mel_audio(B, L, 9000 + i, 10.0, 1e-3, bank, hop, 2, None)
            x = xc.to(dev)
            feat = m(x)
            assert feat.shape == (B, n_mels, T)
            same_rows(feat, lambda b: m(x[b:b + 1]), B, ("MFCC", n_mels, B, T, norm_mode))
            if not norm_mode:
                worst.add(cpu(feat).transpose(0, 2, 1), want, (B, T))
        if not norm_mode:
            worst.check()


# ---- the streaming session ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames_per_step", (1, 3))
@pytest.mark.parametrize("n_fft", (256, 512))
def test_streaming_session_streams_are_independent(dev, n_fft, frames_per_step):
    """StreamingDGTSession: stream s of an S-stream session against a one-stream session fed the same chunks, mag_out
    and y_out after each of four steps.  Its analysis is ops.stft_forward(center=False, T=n, B=S), its synthesis
    ops.irfft_frames: at one frame per step every stream has a transform of its own."""
    hop, S_ = n_fft // 4, 5
    chunk = hop * frames_per_step
    kw = dict(n_fft=n_fft, hop_length=hop, device=dev, random_phase_below_tolerance=False, use_graph=False)
    big = StreamingDGTSession(S_, chunk, **kw)
    ones = {s: StreamingDGTSession(1, chunk, **kw) for s in S.tested_clips(S_)}
    for step in range(4):
        x = audio(S_, chunk, 100 * n_fft + step).to(dev)
        y = big.step(x)
        for s, one in ones.items():
            y1 = one.step(x[s:s + 1])
            assert torch.equal(big.mag_out[s], one.mag_out[0]), (n_fft, frames_per_step, step, s, "mag_out")
            assert torch.equal(y[s], y1[0]), (n_fft, frames_per_step, step, s, "y_out")
    assert bool(torch.isfinite(big.y_out).all()) and float(big.y_out.abs().max()) > 0


# ---- one frame per transform: controls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", (1024, 2048, 4096, 64, 400))
def test_per_clip_accuracy_controls(dev, n_fft):
    """The same per-clip check where every frame has a transform of its own (register kernels at 1024 / 2048 / 4096, the
    generic kernel at 64, mixed radix at 400)."""
    hop, B, T = n_fft // 4, S.B_SWEEP, 9
    m = module("stft", n_fft, hop, dev)
    xc = audio(B, hop * (T - 1) + 4, n_fft)
    x = xc.to(dev)
    X = m(x)
    same_rows(X, lambda b: m(x[b:b + 1]), B, ("control forward", n_fft))
    w = Worst("control forward n_fft %d" % n_fft, TOL)
    w.add(X, O.stft_forward(xc.double(), m.window[:n_fft].cpu().double(), n_fft, hop).numpy(), (B, T))
    w.check()
    Xc = spectra(B, T, n_fft // 2 + 1, n_fft + 1)
    Xd = Xc.to(dev)
    y = m.invert(Xd)
    same_rows(y, lambda b: m.invert(Xd[b:b + 1]), B, ("control invert", n_fft))
    w = Worst("control invert n_fft %d" % n_fft, TOL)
    w.add(y, O.istft(Xc.to(torch.complex128), m.inv_window[:n_fft].cpu().double(), n_fft, hop).numpy(), (B, T))
    w.check()


# ---- non-finite samples -------------------------------------------------------------------------------------------------
BAD = {1: float("nan"), 3: float("inf")}          # clip -> what it holds


def group_closure(bad_frames, T, K):
    """Frames of a clip that share a transform with one of `bad_frames` under the per-clip grouping."""
    grp = S.groups(1, T, K)
    out = set()
    for t in bad_frames:
        out |= {u for _, u in S.mates(grp, 0, t)}
    return out


@pytest.mark.parametrize("n_fft", NFFTS)
def test_non_finite_forward(dev, n_fft):
    """One clip holds a NaN, another an Inf: one sample in the middle and one in the last n_fft / 2 samples (the reflect
    padding repeats it).  Every other clip: finite, and the bits of the launch with the bad clips zeroed.  In the bad
    clips every frame the float64 oracle makes non-finite is non-finite here too, and nothing beyond the frames that
    share a transform with one of those (up to K - 1 frames of the same clip).  n_fft 512 at hop 128
    takes the sliding kernel, which pairs frames (2 i, 2 i + 1) of a clip likewise: a control."""
    K, B = S.K_OF[n_fft], S.B_SWEEP
    for hop, T, center in ((n_fft // 4, 2 * K + 3, True), (n_fft // 2, K + 1, True), (n_fft // 4 + 8, 2 * K + 1, False),
                           (n_fft // 2, 3, True)):
        L = S.center_shape(n_fft, T, hop)[1] if center else hop * (T - 1) + n_fft
        if center:
            hop = S.center_shape(n_fft, T, hop)[0]
        m = module("stft", n_fft, hop, dev)
        xc = audio(B, L, 13 * n_fft + T)
        clean = xc.clone()
        for b, v in BAD.items():
            xc[b, L // 2] = v
            xc[b, L - 3] = v
            clean[b] = 0
        X = forward_call(m, xc.to(dev), n_fft, hop, center, T, L)
        X0 = forward_call(m, clean.to(dev), n_fft, hop, center, T, L)
        ref = forward_ref(m, xc, n_fft, hop, center, T)
        fin = torch.isfinite(torch.view_as_real(X)).all(-1).all(-1).cpu().numpy()        # (B, T)
        for b in range(B):
            if b not in BAD:
                assert fin[b].all(), (n_fft, hop, T, b, "a clean clip turned non-finite")
                assert torch.equal(X[b], X0[b]), (n_fft, hop, T, b, "a clean clip's bits depend on its neighbours")
                continue
            bad_ref = {t for t in range(T) if not np.isfinite(ref[b, t]).all()}
            bad_gpu = {t for t in range(T) if not fin[b, t]}
            assert bad_ref and bad_ref <= bad_gpu, (n_fft, hop, T, b, "a non-finite frame was lost", bad_ref - bad_gpu)
            assert bad_gpu <= group_closure(bad_ref, T, K), (n_fft, hop, T, b, sorted(bad_gpu), sorted(bad_ref))


@pytest.mark.parametrize("n_fft", NFFTS)
def test_non_finite_inverse(dev, n_fft):
    """A NaN / Inf bin in one frame of two clips, through invert (complex), polar input and ops.irfft_frames: the other
    clips stay finite with the bits of the launch with the bad clips zeroed; in the bad clips every sample / frame the
    oracle makes non-finite is non-finite here, and nothing beyond what the frame's group covers."""
    K, B, F = S.K_OF[n_fft], S.B_SWEEP, n_fft // 2 + 1
    for hop, T in ((n_fft // 4, 2 * K + 3), (n_fft // 4 + 8, 2 * K + 1), (n_fft // 2, K + 1)):
        m = module("stft", n_fft, hop, dev)
        iw = m.inv_window[:n_fft]
        Xc = spectra(B, T, F, 17 * n_fft + T)
        clean = Xc.clone()
        tb = T // 2
        for b, v in BAD.items():
            Xc[b, tb, 5] = complex(v, 1.0)
            clean[b] = 0
        reach = group_closure({tb}, T, K)
        # frames: ops.irfft_frames on (B, T, F), complex and polar
        for polar in (False, True):
            def run(Xs):
                if polar:
                    return ops.irfft_frames(None, iw, n_fft, mag=Xs.real.contiguous().to(dev), phase=Xs.imag.contiguous().to(dev))
                return ops.irfft_frames(Xs.to(dev), iw, n_fft)
            y, y0 = run(Xc), run(clean)
            fin = torch.isfinite(y).all(-1).cpu().numpy()                                  # (B, T)
            for b in range(B):
                if b not in BAD:
                    assert fin[b].all() and torch.equal(y[b], y0[b]), (n_fft, T, b, polar, "frames")
                else:
                    bad_gpu = {t for t in range(T) if not fin[b, t]}
                    assert tb in bad_gpu and bad_gpu <= reach, (n_fft, T, b, polar, sorted(bad_gpu), sorted(reach))
        # overlap-added audio
        y, y0 = m.invert(Xc.to(dev)), m.invert(clean.to(dev))
        ref = O.istft(Xc.to(torch.complex128), iw.cpu().double(), n_fft, hop).numpy()
        fin = torch.isfinite(y).cpu().numpy()
        covered = np.zeros(hop * (T - 1), dtype=bool)
        for t in reach:
            lo, hi = t * hop - n_fft // 2, t * hop + n_fft // 2
            covered[max(lo, 0):max(min(hi, covered.size), 0)] = True
        for b in range(B):
            if b not in BAD:
                assert fin[b].all() and torch.equal(y[b], y0[b]), (n_fft, hop, T, b, "istft")
            else:
                assert (~np.isfinite(ref[b])).any()
                assert not (fin[b] & ~np.isfinite(ref[b])).any(), (n_fft, hop, T, b, "a non-finite sample was lost")
                assert not (~fin[b] & ~covered).any(), (n_fft, hop, T, b, "non-finite samples outside the group's frames")

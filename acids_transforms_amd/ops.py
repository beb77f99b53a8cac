"""Tensor-level wrappers over the C ABI (include/acids_hip.h).

Each function takes ROCm-device tensors, allocates the output with torch
(device memory + stream plumbing only) and launches the HIP kernels on the
current torch stream.  No arithmetic happens in Python.
"""
import ctypes
import math

import torch

from ._lib import AT_EUNSUPPORTED, AcidsHipError, check, device_scoped, lib, ptr, require_device, stream_ptr


_FP64_NARROWING = False


class allow_fp64_narrowing:
    """Opt-in for call sites written against the reference that hand over float64 audio (numpy / soundfile default) or
    complex128 spectra: `acids_transforms_amd.allow_fp64_narrowing(True)` (process-wide), or as a context manager
    `with allow_fp64_narrowing(): ...`.  Operands are then narrowed to float32 / complex64 on entry and RESULTS ARE
    FLOAT32 -- the reference would have stayed in double (stft.py:36-47, torch.stft promotes).  Off by default: a silent
    loss of digits is an error here (documented divergence with an explicit way in)."""

    def __init__(self, enabled: bool = True):
        global _FP64_NARROWING
        self.prev = _FP64_NARROWING
        _FP64_NARROWING = bool(enabled)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _FP64_NARROWING
        _FP64_NARROWING = self.prev
        return False


def _no_fp64(t, what="input"):
    """The kernels compute in fp32 / complex64.  The reference run on float64 data stays in double precision
    (torch.stft promotes: complex128 out, reference stft.py:98-104); narrowing that silently would hand back fewer
    digits than the caller asked for, so it is an error with the way out in the message."""
    if t.dtype in (torch.float64, torch.complex128) and not _FP64_NARROWING:
        raise AcidsHipError("%s is %s: the MI355X kernels compute in float32 / complex64 and do not narrow silently -- "
                            "convert explicitly (x.float() / X.to(torch.complex64)), or opt in once with "
                            "acids_transforms_amd.allow_fp64_narrowing(True), if single precision is acceptable"
                            % (what, str(t.dtype).replace("torch.", "")))
    return t


def _f32c(t):
    _no_fp64(t)
    if t.dtype != torch.float32:
        t = t.float()         # integer / half inputs: widening only
    return t if t.is_contiguous() else t.contiguous()


def _c64(X):
    _no_fp64(X, "spectrum")
    return X if X.dtype == torch.complex64 else X.to(torch.complex64)


def stft_forward(x, window, n_fft, hop, center=True, want_phase=False, T=None, clip_stride=None, L=None, B=None):
    """x: (B, L) float32 -> (B, T, F) complex64 [, phase (B, T, F) float32].

    With center=False and explicit T / clip_stride / L the kernel frames an
    overlapping strided view directly (OverlapAdd.forward output) without a copy.
    """
    require_device(x, window)
    if B is None:
        B = x.shape[0]
    if L is None:
        x = _f32c(x)
        L = x.shape[1]
        clip_stride = L
    if T is None:
        T = 1 + (L - (n_fft & 1)) // hop if center else None      # torch.stft pads n_fft // 2 (floor) on both sides
    F = n_fft // 2 + 1
    out = torch.empty((B, T, F), dtype=torch.complex64, device=x.device)
    phase = torch.empty((B, T, F), dtype=torch.float32, device=x.device) if want_phase else None
    check(lib().at_stft_forward(ptr(x), B, L, clip_stride, T, n_fft, hop, int(bool(center)), ptr(window),
                                ptr(out), ptr(phase), stream_ptr()), "at_stft_forward")
    return (out, phase) if want_phase else out


def istft_envelope_table(inv_window, n_fft, hop):
    require_device(inv_window)
    env = torch.empty((1 << (n_fft // hop), hop), dtype=torch.float32, device=inv_window.device)
    check(lib().at_istft_envelope_table(ptr(inv_window), n_fft, hop, ptr(env), stream_ptr()), "at_istft_envelope_table")
    return env


def istft(X, inv_window, n_fft, hop, env16=None, mag=None, phase=None):
    """(B, T, F) complex64 -- or mag & phase float32 -- -> (B, hop*(T-1) + (n_fft & 1)) float32 (torch.istft's length)."""
    src = X if X is not None else mag
    require_device(src, inv_window)
    if X is not None:
        X = X if X.is_contiguous() else X.contiguous()
        X = _c64(X)
    else:
        mag, phase = _f32c(mag), _f32c(phase)
        if phase.shape != mag.shape:
            phase = phase.expand_as(mag).contiguous()
    B, T, F = src.shape
    assert F == n_fft // 2 + 1, "last dim must be n_fft/2+1"
    # torch.istft trims n_fft // 2 at both ends of the n_fft + hop (T - 1) overlap-added samples
    y = torch.empty((B, hop * (T - 1) + (n_fft & 1) if T > 0 else 0), dtype=torch.float32, device=src.device)
    if env16 is None and n_fft in (512, 1024, 2048, 4096) and hop in (n_fft // 8, n_fft // 4, n_fft // 2):
        env16 = istft_envelope_table(inv_window, n_fft, hop)      # the fused kernel's table (modules cache theirs)
    wsb = lib().at_istft_workspace_bytes(B, T, n_fft, hop)
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=src.device) if wsb else None
    check(lib().at_istft(ptr(X), ptr(mag), ptr(phase), B, T, n_fft, hop, ptr(inv_window), ptr(env16), ptr(y),
                         ptr(ws), wsb, stream_ptr()), "at_istft")
    return y


def irfft_frames(X, inv_window, n_fft, mag=None, phase=None):
    """(..., n, F) spectra -> (..., n, n_fft) windowed frames (no overlap-add).  Each leading-index row of n frames is
    one stream: frames share a register FFT (n_fft 128 / 256 / 512) within a stream only."""
    src = X if X is not None else mag
    require_device(src, inv_window)
    if X is not None:
        X = X if X.is_contiguous() else X.contiguous()
        X = _c64(X)
    else:
        mag, phase = _f32c(mag), _f32c(phase)
        if phase.shape != mag.shape:
            phase = phase.expand_as(mag).contiguous()
    lead = src.shape[:-1]
    n = 1
    for d in lead:
        n *= d
    out = torch.empty(tuple(lead) + (n_fft,), dtype=torch.float32, device=src.device)
    per_stream = max(int(lead[-1]), 1) if len(lead) >= 2 else max(n, 1)
    check(lib().at_irfft_frames_streams(ptr(X), ptr(mag), ptr(phase), n, per_stream, n_fft, ptr(inv_window), ptr(out),
                                        stream_ptr()), "at_irfft_frames_streams")
    return out


def angle(X):
    """complex64 -> float32 atan2(im, re), same shape."""
    require_device(X)
    X = X if X.is_contiguous() else X.contiguous()
    out = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    check(lib().at_angle(ptr(X), X.numel(), ptr(out), stream_ptr()), "at_angle")
    return out


_CONTRAST = {None: 0, "none": 0, "log1p": 1, "log": 2, "log10": 3}


def contrast_code(mode):
    if mode not in _CONTRAST:
        raise TypeError("unknown contrast type %s" % mode)
    return _CONTRAST[mode]


def _a_kind(x, power=1):
    if torch.is_complex(x):
        return 1 if power == 2 else 0
    return 3


def _prep_in(x):
    if torch.is_complex(x):
        x = _c64(x)
    else:
        x = _f32c(x)
    return x if x.is_contiguous() else x.contiguous()


def _project_banded(x, a_kind, band, contrast, inverse, offset, scale, eps, out, N, channel_major_T, ld_out=None,
                    phase_out=None, ld_phase=0, phase_offset=None, phase_scale=None, phase_in=None, rows=None, lda=None):
    lane_filter, lane_start, weights = band.on(x.device)
    K = band.K
    check(lib().at_mel_project_banded(ptr(x), a_kind, x.numel() // K if rows is None else rows, K if lda is None else lda,
                                      K, ptr(lane_filter), ptr(lane_start),
                                      ptr(weights), N, band.n_passes, band.pass_len.ctypes.data,
                                      contrast_code(contrast), int(inverse), ptr(offset), ptr(scale), eps, ptr(out),
                                      N if ld_out is None else ld_out, channel_major_T, phase_out, ld_phase,
                                      ptr(phase_offset), ptr(phase_scale), phase_in, stream_ptr()),
          "at_mel_project_banded")
    return out


def polar_inverse(y, inv_band, contrast=None, mag_offset=None, mag_scale=None, eps=1.1920929e-07, phase_offset=None,
                  phase_scale=None):
    """Polar.invert in one pass: y (..., T, 2, F) stacked -> (..., T, F) complex64 =
    (invert_contrast(y[.., 0, :] * s + o) @ inverse_bank) * exp(i * (y[.., 1, :] * ps + po))."""
    import ctypes
    require_device(y)
    y = _f32c(y)
    F = y.shape[-1]
    assert inv_band.K == F and inv_band.N == F and inv_band.eligible
    rows = y.numel() // (2 * F)
    out = torch.empty(y.shape[:-2] + (F,), dtype=torch.complex64, device=y.device)
    phase_ptr = ctypes.c_void_p(y.data_ptr() + 4 * F)
    _project_banded(y, 2, inv_band, contrast, True, mag_offset, mag_scale, eps, out, F, 0, ld_out=F, ld_phase=2 * F,
                    phase_offset=phase_offset, phase_scale=phase_scale, phase_in=phase_ptr, rows=rows, lda=2 * F)
    return out


def polar_forward(x, band, contrast=None, mag_offset=None, mag_scale=None, eps=1.1920929e-07, phase_offset=None,
                  phase_scale=None):
    """Polar.forward in one pass: x (..., T, F) complex64 -> (..., T, 2, F) with [..., 0, :] =
    normalise(contrast(|x| @ bank)) (banded bank with F filters) and [..., 1, :] = normalise(angle(x))."""
    import ctypes
    require_device(x)
    x = _prep_in(x)
    F = x.shape[-1]
    assert band.N == F and band.eligible
    out = torch.empty(x.shape[:-1] + (2, F), dtype=torch.float32, device=x.device)
    phase_ptr = ctypes.c_void_p(out.data_ptr() + 4 * F)
    _project_banded(x, 0, band, contrast, False, mag_offset, mag_scale, eps, out, F, 0, ld_out=2 * F,
                    phase_out=phase_ptr, ld_phase=2 * F, phase_offset=phase_offset, phase_scale=phase_scale)
    return out


def mel_forward(x, bank, contrast=None, offset=None, scale=None, eps=1.1920929e-07, power=1, channel_major_T=0,
                band=None, out=None):
    """normalise(contrast(|x|^power @ bank)); x: (..., K) complex64/float32, bank: (K, N).
    channel_major_T = T > 0 stores (..., N, T) for x of shape (..., T, K) (MelSpectrogram layout).
    band: utils.banded.BandedBank of `bank` (eligible) -> the HBM-bound banded walk instead of the dense MFMA
    contraction."""
    require_device(x, bank)
    x = _prep_in(x)
    K, N = bank.shape[-2], bank.shape[-1]
    assert x.shape[-1] == K, "last dim of the input (%d) must match the bank (%d)" % (x.shape[-1], K)
    if band is not None and band.eligible:
        shape = (x.shape[:-2] + (N, channel_major_T)) if channel_major_T else (x.shape[:-1] + (N,))
        out = _out_buffer(out, shape, x.device)
        return _project_banded(x, _a_kind(x, power), band, contrast, False, offset, scale, eps, out, N, channel_major_T)
    bank2 = bank.reshape(K, N)
    bank2 = bank2 if bank2.is_contiguous() else bank2.contiguous()
    rows = x.numel() // K
    if channel_major_T:
        out = _out_buffer(out, x.shape[:-2] + (N, channel_major_T), x.device)
    else:
        out = _out_buffer(out, x.shape[:-1] + (N,), x.device)
    check(lib().at_mel_project(ptr(x), _a_kind(x, power), rows, K, K, ptr(bank2), N, N, contrast_code(contrast), 0,
                               ptr(offset), ptr(scale), eps, ptr(out), N, channel_major_T, stream_ptr()),
          "at_mel_project")
    return out


def mel_bf16_pack_bank(bank):
    """(K, N) fp32 bank -> the bf16 operand image of at_mel_project_bf16 (a uint8 tensor, opaque)."""
    require_device(bank)
    K, N = bank.shape[-2], bank.shape[-1]
    b2 = _f32c(bank.reshape(K, N))
    img = torch.empty(lib().at_mel_bf16_bank_bytes(K, N), dtype=torch.uint8, device=bank.device)
    check(lib().at_mel_bf16_pack_bank(ptr(b2), K, N, N, ptr(img), stream_ptr()), "at_mel_bf16_pack_bank")
    return img


def mel_forward_bf16(x, bank_image, K, N, contrast=None, offset=None, scale=None, eps=1.1920929e-07, power=1,
                     out=None):
    """normalise(contrast(bf16(|x|^power) @ bf16(bank))), fp32 accumulation on the bf16 matrix cores.
    x: (..., K) complex64 / float32; bank_image: mel_bf16_pack_bank(bank) of a (K, N) bank."""
    require_device(x, bank_image)
    x = _prep_in(x)
    assert x.shape[-1] == K, "last dim of the input (%d) must match the bank (%d)" % (x.shape[-1], K)
    out = _out_buffer(out, x.shape[:-1] + (N,), x.device)
    check(lib().at_mel_project_bf16(ptr(x), _a_kind(x, power), x.numel() // K, K, K, ptr(bank_image), N,
                                    contrast_code(contrast), ptr(offset), ptr(scale), eps, ptr(out), N, stream_ptr()),
          "at_mel_project_bf16")
    return out


def mel_inverse(y, inv_bank, contrast=None, offset=None, scale=None, eps=1.1920929e-07, band=None):
    """invert_contrast(y*scale+offset) @ inv_bank; y: (..., K) float32, inv_bank: (K, N).
    band: BandedBank of `inv_bank` (eligible) -> banded walk."""
    require_device(y, inv_bank)
    y = _prep_in(y)
    K, N = inv_bank.shape[-2], inv_bank.shape[-1]
    assert y.shape[-1] == K
    if band is not None and band.eligible:
        out = torch.empty(y.shape[:-1] + (N,), dtype=torch.float32, device=y.device)
        return _project_banded(y, 2, band, contrast, True, offset, scale, eps, out, N, 0)
    b2 = inv_bank.reshape(K, N)
    b2 = b2 if b2.is_contiguous() else b2.contiguous()
    rows = y.numel() // K
    out = torch.empty(y.shape[:-1] + (N,), dtype=torch.float32, device=y.device)
    check(lib().at_mel_project(ptr(y), 2, rows, K, K, ptr(b2), N, N, contrast_code(contrast), 1, ptr(offset),
                               ptr(scale), eps, ptr(out), N, 0, stream_ptr()), "at_mel_project")
    return out


def _out_buffer(out, shape, device):
    """Caller-supplied result buffer (persistent outputs of a captured streaming step) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError("out= must be a contiguous float32 tensor of shape %s on %s" % (tuple(shape), device))
    return out


def mag_pointwise(x, contrast=None, offset=None, scale=None, eps=1.1920929e-07, inverse=False, out=None):
    """mel=False chains: normalise(contrast(|x|)) or invert_contrast(x*scale+offset)."""
    require_device(x)
    x = _prep_in(x)
    kind = 2 if inverse else _a_kind(x)
    out = _out_buffer(out, x.shape, x.device)
    check(lib().at_mag_pointwise(ptr(x), kind, x.numel(), contrast_code(contrast), int(inverse), ptr(offset),
                                 ptr(scale), eps, ptr(out), stream_ptr()), "at_mag_pointwise")
    return out


def stats(x, contrast=None, eps=1.1920929e-07, take_abs=True):
    """float64 tensor [min, max, sum, sumsq] of contrast(|x|) (take_abs) or of real x."""
    require_device(x)
    x = _prep_in(x)
    kind = _a_kind(x) if (take_abs or torch.is_complex(x)) else 2
    out = torch.empty(4, dtype=torch.float64, device=x.device)
    wsb = lib().at_stats_workspace_bytes()
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=x.device)
    check(lib().at_stats(ptr(x), kind, x.numel(), contrast_code(contrast), eps, ptr(out), ptr(ws), wsb, stream_ptr()),
          "at_stats")
    return out


def affine(x, offset, scale, inverse=False):
    require_device(x, offset, scale)
    x = _prep_in(x)
    out = torch.empty_like(x)
    check(lib().at_affine(ptr(x), x.numel(), ptr(offset), ptr(scale), int(inverse), ptr(out), stream_ptr()), "at_affine")
    return out


def mel_forward_real(x, mat, offset=None, scale=None, channel_major_T=0):
    """normalise(x @ mat) for real x (no |.|): second projection of the MFCC extension."""
    require_device(x, mat)
    x = _prep_in(x)
    K, N = mat.shape
    rows = x.numel() // K
    if channel_major_T:
        out = torch.empty(x.shape[:-2] + (N, channel_major_T), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    mat = _f32c(mat)
    if K <= 128 and N <= 64:      # narrow matrix: columns in registers, one wavefront per row
        check(lib().at_project_small(ptr(x), rows, K, ptr(mat), N, ptr(offset), ptr(scale), ptr(out), channel_major_T,
                                     stream_ptr()), "at_project_small")
        return out
    check(lib().at_mel_project(ptr(x), 2, rows, K, K, ptr(mat), N, N, 0, 0, ptr(offset), ptr(scale), 0.0, ptr(out), N,
                               channel_major_T, stream_ptr()), "at_mel_project")
    return out


def _workspace(nbytes, device):
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)


def pghi_gradients(mag, gamma, n_fft, hop, eps=1.1920929e-07):
    """(B, T, F) magnitudes -> (tgradw, fgradw), each (B, T, F)."""
    require_device(mag)
    mag = _f32c(mag)
    B, T, F = mag.shape
    tg = torch.empty_like(mag)
    fg = torch.empty_like(mag)
    check(lib().at_pghi_gradients(ptr(mag), B, T, F, gamma, n_fft, hop, eps, ptr(tg), ptr(fg), ptr(None),
                                  stream_ptr()), "at_pghi_gradients")
    return tg, fg


def pghi_offline(mag, gamma, n_fft, hop, tol, eps=1.1920929e-07, debug=False):
    """(B, T, F) magnitudes -> phase (B, T, F); debug=True also returns (npops, order)."""
    require_device(mag)
    mag = _f32c(mag)
    B, T, F = mag.shape
    phase = torch.empty_like(mag)
    wsb = lib().at_pghi_offline_workspace_bytes(B, T, F)
    ws = _workspace(wsb, mag.device)
    npops = torch.zeros(B, dtype=torch.int64, device=mag.device) if debug else None
    order = torch.full((B, T * F), -1, dtype=torch.int32, device=mag.device) if debug else None
    check(lib().at_pghi_offline(ptr(mag), B, T, F, gamma, n_fft, hop, tol, eps, ptr(phase), ptr(ws), wsb, ptr(npops),
                                ptr(order), stream_ptr()), "at_pghi_offline")
    return (phase, npops, order) if debug else phase


def pghi_integrate(mag, tgradw, fgradw, tol, abstol=1.1920929e-07, debug=False):
    """DGT.perform_hgi: heap integration of (B, T, F) magnitudes along caller-supplied gradients -> phase (B, T, F);
    debug=True also returns (npops, order).  `mag` is left untouched."""
    require_device(mag, tgradw, fgradw)
    mag, tgradw, fgradw = _f32c(mag), _f32c(tgradw), _f32c(fgradw)
    assert tgradw.shape == mag.shape and fgradw.shape == mag.shape
    B, T, F = mag.shape
    phase = torch.empty_like(mag)
    wsb = lib().at_pghi_offline_workspace_bytes(B, T, F)
    ws = _workspace(wsb, mag.device)
    npops = torch.zeros(B, dtype=torch.int64, device=mag.device) if debug else None
    order = torch.full((B, T * F), -1, dtype=torch.int32, device=mag.device) if debug else None
    check(lib().at_pghi_integrate(ptr(mag), ptr(tgradw), ptr(fgradw), B, T, F, tol, abstol, ptr(phase), ptr(ws), wsb,
                                  ptr(npops), ptr(order), stream_ptr()), "at_pghi_integrate")
    return (phase, npops, order) if debug else phase


def pghi_realtime(mag_hist, mag, prev_phase, noise, gamma, n_fft, hop, tol, eps=1.1920929e-07, debug=False):
    """streaming PGHI for S streams: (S,2,F), (S,n,F), (S,F), (S,n,F) -> phase (S,n,F)."""
    require_device(mag, mag_hist, prev_phase, noise)
    mag_hist, mag, prev_phase, noise = _f32c(mag_hist), _f32c(mag), _f32c(prev_phase), _f32c(noise)
    S, n, F = mag.shape
    phase = torch.empty_like(mag)
    wsb = lib().at_pghi_rt_workspace_bytes(S, n, F)
    ws = _workspace(wsb, mag.device)
    tg = torch.empty((S, n + 2, F), dtype=torch.float32, device=mag.device) if debug else None
    fg = torch.empty((S, n + 2, F), dtype=torch.float32, device=mag.device) if debug else None
    check(lib().at_pghi_realtime(ptr(mag_hist), ptr(mag), ptr(prev_phase), ptr(noise), S, n, F, gamma, n_fft, hop, tol,
                                 eps, ptr(phase), ptr(tg), ptr(fg), ptr(ws), wsb, stream_ptr()), "at_pghi_realtime")
    return (phase, tg, fg) if debug else phase


def pghi_realtime_seeded(mag_hist, mag, prev_phase, rng_state, gamma, n_fft, hop, tol, eps=1.1920929e-07):
    """pghi_realtime with the below-tolerance draws made on the device (Philox keyed by `rng_state`, a 4-element int32
    tensor {seed lo, seed hi, step counter, 0} that the call advances): nothing but the kernels in a captured step."""
    require_device(mag, mag_hist, prev_phase, rng_state)
    mag_hist, mag, prev_phase = _f32c(mag_hist), _f32c(mag), _f32c(prev_phase)
    assert rng_state.dtype == torch.int32 and rng_state.numel() == 4 and rng_state.is_contiguous()
    S, n, F = mag.shape
    phase = torch.empty_like(mag)
    wsb = lib().at_pghi_rt_workspace_bytes(S, n, F)
    ws = _workspace(wsb, mag.device)
    check(lib().at_pghi_realtime_seeded(ptr(mag_hist), ptr(mag), ptr(prev_phase), ptr(rng_state), S, n, F, gamma, n_fft, hop,
                                        tol, eps, ptr(phase), ptr(ws), wsb, stream_ptr()), "at_pghi_realtime_seeded")
    return phase


def rt_update_buffers_(mag, phase, mag_hist, prev_phase):
    """RealtimeDGT.update_buffers (dgt.py:330-336) IN PLACE on the state tensors mag_hist (S, 2, F) and
    prev_phase (S, F), for x = mag * exp(i * phase) with mag / phase (S, n, F)."""
    require_device(mag, phase, mag_hist, prev_phase)
    mag, phase = _f32c(mag), _f32c(phase)
    S, n, F = mag.shape
    assert mag_hist.is_contiguous() and prev_phase.is_contiguous() and mag_hist.dtype == torch.float32
    assert tuple(mag_hist.shape) == (S, 2, F) and tuple(prev_phase.shape) == (S, F)
    check(lib().at_rt_update_buffers(ptr(mag), ptr(phase), S, n, F, ptr(mag_hist), ptr(mag_hist), ptr(prev_phase),
                                     stream_ptr()), "at_rt_update_buffers")


def rt_polar_irfft_update(mag, phase, inv_window, n_fft, mag_hist):
    """x = mag*exp(i*phase): windowed irfft frames (..., n, n_fft) plus the refreshed PGHI
    history buffers (|x[-2:]|, angle(x[-1]))."""
    require_device(mag, phase, inv_window, mag_hist)
    mag, phase = _f32c(mag), _f32c(phase)
    frames = irfft_frames(None, inv_window, n_fft, mag=mag, phase=phase)
    lead = mag.shape[:-2]
    n, F = mag.shape[-2], mag.shape[-1]
    S = 1
    for d in lead:
        S *= d
    hist_in = _f32c(mag_hist)
    hist_out = torch.empty(tuple(lead) + (2, F), dtype=torch.float32, device=mag.device)
    ph_out = torch.empty(tuple(lead) + (F,), dtype=torch.float32, device=mag.device)
    check(lib().at_rt_update_buffers(ptr(mag), ptr(phase), S, n, F, ptr(hist_in), ptr(hist_out), ptr(ph_out),
                                     stream_ptr()), "at_rt_update_buffers")
    return frames, hist_out, ph_out


def oadd_forward(x2d, hist, keep, n_fft, hop):
    """x2d (S, C), hist (S, keep) or None -> (buf (S, buf_len), new_hist (S, keep), n_frames)."""
    from .utils.misc import n_frames
    require_device(x2d)
    x2d = _f32c(x2d)
    S, C = x2d.shape
    if C < keep and C % hop:
        # reference granularity is keep samples (oadd.py:41); shorter chunks are an extension for whole hops only
        raise ValueError("OverlapAdd needs chunks of at least %d samples, or a whole number of hops (got %d)" % (keep, C))
    total = keep + C
    nw = n_frames(total, n_fft, hop)
    buf_len = max(total, nw * hop + n_fft)
    buf = torch.empty((S, buf_len), dtype=torch.float32, device=x2d.device)
    new_hist = torch.empty((S, keep), dtype=torch.float32, device=x2d.device)
    check(lib().at_oadd_forward(ptr(x2d), ptr(hist), S, C, keep, buf_len, ptr(buf), ptr(new_hist), stream_ptr()),
          "at_oadd_forward")
    return buf, new_hist, nw


def oadd_push_(buf, x2d, keep):
    """Streaming input state in place: buf (S, >= keep + C) = [history | chunk | pad] <- [last keep samples of
    (history | old chunk) | x2d | pad]."""
    require_device(buf, x2d)
    x2d = _f32c(x2d)
    S, C = x2d.shape
    assert buf.is_contiguous() and buf.dtype == torch.float32 and buf.shape[0] == S and buf.shape[1] >= keep + C
    check(lib().at_oadd_push(ptr(x2d), S, C, keep, buf.shape[1], ptr(buf), stream_ptr()), "at_oadd_push")


def oadd_invert(frames3d, tail, n_fft, hop, keep, gain, out=None, in_place=False):
    """frames (S, n, n_fft), tail (S, keep) or None -> (out (S, (n-1)*hop+n_fft-keep), new_tail (S, keep)).
    in_place=True: `tail` itself is updated (and returned)."""
    require_device(frames3d, gain)
    frames3d = _f32c(frames3d)
    S, n, _ = frames3d.shape
    out_len = (n - 1) * hop + n_fft - keep
    out = _out_buffer(out, (S, out_len), frames3d.device)
    if in_place:
        assert tail is not None and tail.is_contiguous() and tuple(tail.shape) == (S, keep)
        new_tail = tail
    else:
        new_tail = torch.empty((S, keep), dtype=torch.float32, device=frames3d.device)
    check(lib().at_oadd_invert(ptr(frames3d), ptr(tail), S, n, n_fft, hop, keep, ptr(gain), ptr(out), ptr(new_tail),
                               stream_ptr()), "at_oadd_invert")
    return out, new_tail


def mulaw_encode(x, channels):
    require_device(x)
    if not x.is_floating_point():
        raise TypeError("The input Tensor must be of floating type.")
    x = _f32c(x)
    out = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    check(lib().at_mulaw_encode(ptr(x), x.numel(), channels, ptr(out), stream_ptr()), "at_mulaw_encode")
    return out


def mulaw_decode(codes, channels):
    require_device(codes)
    codes = codes if codes.is_contiguous() else codes.contiguous()
    ci = cf = None
    if codes.is_floating_point():
        cf = _f32c(codes)
    else:
        ci = codes.long()
    out = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    check(lib().at_mulaw_decode(ptr(ci), ptr(cf), codes.numel(), channels, ptr(out), stream_ptr()), "at_mulaw_decode")
    return out


def onehot(x, classes, channel_major=False):
    require_device(x)
    if x.dtype != torch.int64:
        raise RuntimeError("one_hot is only applicable to index tensor of type LongTensor.")
    x = x if x.is_contiguous() else x.contiguous()
    if channel_major:
        inner = x.shape[-1]
        out = torch.empty(x.shape[:-1] + (classes, inner), dtype=torch.int64, device=x.device)
    else:
        inner = 0
        out = torch.empty(x.shape + (classes,), dtype=torch.int64, device=x.device)
    check(lib().at_onehot(ptr(x), x.numel(), classes, inner, ptr(out), stream_ptr()), "at_onehot")
    return out


def argmax_last(x):
    require_device(x)
    x = x if x.is_contiguous() else x.contiguous()
    xi = xf = None
    if x.is_floating_point():
        xf = _f32c(x)
    else:
        xi = x.long()
    cols = x.shape[-1]
    out = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    check(lib().at_argmax_last(ptr(xi), ptr(xf), x.numel() // cols, cols, ptr(out), stream_ptr()), "at_argmax_last")
    return out


def scale_complex(mag, z):
    """mag (real) * z (complex64), same shape -> complex64."""
    require_device(mag, z)
    mag = _f32c(mag)
    z = z if z.is_contiguous() else z.contiguous()
    out = torch.empty(mag.shape, dtype=torch.complex64, device=mag.device)
    check(lib().at_scale_complex(ptr(mag), ptr(z), mag.numel(), ptr(out), stream_ptr()), "at_scale_complex")
    return out


def griffinlim_update(mag, rebuilt, tprev, momentum_over_1p):
    """One Griffin-Lim phase update: mag * normalise(rebuilt - m * tprev) -> complex64."""
    require_device(mag, rebuilt)
    mag = _f32c(mag)
    out = torch.empty(mag.shape, dtype=torch.complex64, device=mag.device)
    check(lib().at_griffinlim_update(ptr(mag), ptr(rebuilt), ptr(tprev), momentum_over_1p, mag.numel(), ptr(out),
                                     stream_ptr()), "at_griffinlim_update")
    return out


def istft_griffinlim(mag, rebuilt, tprev, momentum_over_1p, inv_window, n_fft, hop, env16):
    """istft(griffinlim_update(mag, rebuilt, tprev, m)) in one kernel (n_fft 1024, hop 128 / 256 / 512)."""
    require_device(mag, rebuilt, inv_window, env16)
    mag = _f32c(mag)
    B, T, F = mag.shape
    y = torch.empty((B, hop * max(T - 1, 0)), dtype=torch.float32, device=mag.device)
    check(lib().at_istft_griffinlim(ptr(mag), ptr(rebuilt), ptr(tprev), momentum_over_1p, B, T, n_fft, hop,
                                    ptr(inv_window), ptr(env16), ptr(y), stream_ptr()), "at_istft_griffinlim")
    return y


def stft_mel_forward(x, window, band, contrast=None, offset=None, scale=None, eps=1.1920929e-07, power=1,
                     want_spectrum=True, want_phase=False, channel_major=False, hop=256, n_fft=1024):
    """Fused n_fft=1024 forward (hop 256; 128 / 512 without channel_major): x (B, L) -> (X (B,T,513) complex64 or
    None, phase or None, features).  `band` is a utils.banded.BandedBank (fusable).  features: (B, T, N), or
    (B, N, T) when channel_major.  n_fft=2048 / 512 (any hop): features only (want_spectrum=False)."""
    require_device(x, window)
    x = _f32c(x)
    B, L = x.shape
    T = 1 + L // hop
    F = n_fft // 2 + 1
    assert n_fft == 1024 or (n_fft in (2048, 512) and not want_spectrum)
    lane_filter, lane_start, weights = band.on(x.device)
    N = band.N
    X = torch.empty((B, T, F), dtype=torch.complex64, device=x.device) if want_spectrum else None
    phase = torch.empty((B, T, F), dtype=torch.float32, device=x.device) if (want_phase and want_spectrum) else None
    feat = torch.empty((B, N, T) if channel_major else (B, T, N), dtype=torch.float32, device=x.device)
    check(lib().at_stft_mel_forward(ptr(x), B, L, L, T, n_fft, hop, ptr(window), ptr(lane_filter), ptr(lane_start),
                                    ptr(weights), N, band.n_passes, band.pass_len.ctypes.data,
                                    contrast_code(contrast), int(power == 2),
                                    ptr(offset), ptr(scale), eps, ptr(X), ptr(phase), ptr(feat), int(channel_major),
                                    stream_ptr()), "at_stft_mel_forward")
    return X, phase, feat


# ----------------------------------------------------------------------------------------------
# backward passes (autograd.hip; the autograd.Functions of autograd.py call these)
# ----------------------------------------------------------------------------------------------
def stft_backward(G, window, n_fft, hop, L, out=None):
    """Adjoint of stft_forward(center=True): G (B, T, F) complex64, the gradient of the spectrum -> dx (B, L) float32
    (written into `out`, a contiguous (B, L) float32 tensor, when given)."""
    require_device(G, window, out)
    G = _c64(G)
    G = G if G.is_contiguous() else G.contiguous()
    B, T, F = G.shape
    assert F == n_fft // 2 + 1, "last dim must be n_fft/2+1"
    if out is not None:
        assert out.shape == (B, L) and out.dtype == torch.float32 and out.is_contiguous()
    dx = out if out is not None else torch.empty((B, L), dtype=torch.float32, device=G.device)
    wsb = lib().at_stft_backward_workspace_bytes(B, T, n_fft, hop)
    ws = _workspace(wsb, G.device)
    check(lib().at_stft_backward(ptr(G), B, T, L, n_fft, hop, ptr(window), ptr(dx), ptr(ws), wsb, stream_ptr()),
          "at_stft_backward")
    return dx


def istft_backward(gy, inv_window, n_fft, hop, T, env16=None, phase=None):
    """Adjoint of istft: gy (B, hop*(T-1) + (n_fft & 1)) float32, the gradient of its output -> the gradient of the
    spectrum, (B, T, F) complex64; with phase (B, T, F) float32 (polar input mag e^{i phase}), the gradient of mag,
    (B, T, F) float32."""
    require_device(gy, inv_window, phase)
    gy = _f32c(gy)
    B, F = gy.shape[0], n_fft // 2 + 1
    assert gy.shape[-1] == (hop * (T - 1) + (n_fft & 1) if T > 0 else 0), "gy does not match istft's output length"
    if phase is not None:
        phase = _f32c(phase)
        assert phase.shape == (B, T, F), "phase must be (B, T, n_fft/2+1)"
        out = torch.empty((B, T, F), dtype=torch.float32, device=gy.device)
    else:
        out = torch.empty((B, T, F), dtype=torch.complex64, device=gy.device)
    # env16 (the modules pass theirs) is not read: the prep kernel sums the envelope per sample
    wsb = lib().at_istft_backward_workspace_bytes(B, T, n_fft, hop)
    ws = _workspace(wsb, gy.device)
    check(lib().at_istft_backward(ptr(gy), B, T, n_fft, hop, ptr(inv_window), ptr(env16), ptr(phase), ptr(out),
                                  ptr(ws), wsb, stream_ptr()), "at_istft_backward")
    return out


def _frames_per_stream(t):
    """Frames per stream of a (..., n, K) tensor of frames, as irfft_frames and RealtimeSTFT.forward count them: each
    leading-index row of n frames is one stream (a 1-D tensor is one frame)."""
    return max(int(t.shape[-2]), 1) if t.dim() >= 2 else 1


def rfft_frames_backward(G, window, n_fft):
    """Adjoint of the streaming analysis rfft(frames * window): G (..., n, F) complex64, the gradient of the spectrum ->
    the dense gradient of the frames, (..., n, n_fft) float32.  Frames share a register FFT within a stream only."""
    require_device(G, window)
    G = _c64_grad(G)
    assert G.shape[-1] == n_fft // 2 + 1, "last dim must be n_fft/2+1"
    out = torch.empty(tuple(G.shape[:-1]) + (n_fft,), dtype=torch.float32, device=G.device)
    nframes = out.numel() // n_fft
    wsb = lib().at_rfft_frames_backward_workspace_bytes(nframes, n_fft)
    ws = _workspace(wsb, G.device)
    check(lib().at_rfft_frames_backward(ptr(G), nframes, _frames_per_stream(G), n_fft, ptr(window), ptr(out), ptr(ws), wsb,
                                        stream_ptr()), "at_rfft_frames_backward")
    return out


def irfft_frames_backward(gframes, inv_window, n_fft, phase=None):
    """Adjoint of irfft_frames: gframes (..., n, n_fft) float32, the gradient of the windowed frames -> the gradient of
    the spectrum, (..., n, F) complex64; with phase (..., n, F) float32 (polar input mag e^{i phase}), the gradient of
    mag, (..., n, F) float32."""
    require_device(gframes, inv_window, phase)
    gframes = _f32c(gframes)
    assert gframes.shape[-1] == n_fft, "last dim must be n_fft"
    F = n_fft // 2 + 1
    shape = tuple(gframes.shape[:-1]) + (F,)
    if phase is not None:
        phase = _f32c(phase)
        assert tuple(phase.shape) == shape, "phase must be (..., n, n_fft/2+1)"
    out = torch.empty(shape, dtype=torch.float32 if phase is not None else torch.complex64, device=gframes.device)
    nframes, per_stream = gframes.numel() // n_fft, _frames_per_stream(gframes)
    wsb = lib().at_irfft_frames_backward_workspace_bytes(nframes, per_stream, n_fft, int(phase is not None))
    ws = _workspace(wsb, gframes.device)
    check(lib().at_irfft_frames_backward(ptr(gframes), ptr(phase), nframes, per_stream, n_fft, ptr(inv_window), ptr(out),
                                         ptr(ws), wsb, stream_ptr()), "at_irfft_frames_backward")
    return out


def oadd_forward_backward(gframes, n_fft, hop, keep, C):
    """Adjoint of oadd_forward with respect to the chunk: gframes (S, n, n_fft) float32, a dense gradient of the frames
    -> (S, C) float32.  The history's share is dropped; samples that no frame covers get exactly 0."""
    require_device(gframes)
    gframes = _f32c(gframes)
    S, n, N = gframes.shape
    assert N == n_fft, "last dim must be n_fft"
    gx = torch.empty((S, C), dtype=torch.float32, device=gframes.device)
    check(lib().at_oadd_forward_backward(ptr(gframes), S, n, n_fft, hop, keep, C, ptr(gx), stream_ptr()),
          "at_oadd_forward_backward")
    return gx


def oadd_invert_backward(gy, n, n_fft, hop, keep, gain):
    """Adjoint of oadd_invert with respect to the frames: gy (S, (n-1)*hop + n_fft - keep) float32 -> (S, n, n_fft)
    float32 = gy / gain where a frame reaches the output, exactly 0 where it only reaches the new tail."""
    require_device(gy, gain)
    gy = _f32c(gy)
    S = gy.shape[0]
    assert gy.shape[-1] == (n - 1) * hop + n_fft - keep, "gy does not match oadd_invert's output length"
    gframes = torch.empty((S, n, n_fft), dtype=torch.float32, device=gy.device)
    check(lib().at_oadd_invert_backward(ptr(gy), S, n, n_fft, hop, keep, ptr(gain), ptr(gframes), stream_ptr()),
          "at_oadd_invert_backward")
    return gframes


def _cols_args(cols):
    """The five C arguments of one bank's by-column tables (start, len, off, w, nnz); None: no bank."""
    start, length, off, w = cols if cols is not None else (None,) * 4
    return ptr(start), ptr(length), ptr(off), ptr(w), w.numel() if w is not None else 0


def magnitude_backward(x, dF, bank_cols=None, bank_t_cols=None, contrast=None, scale=None, eps=1.1920929e-07,
                       col_off=0, dx_accum=None):
    """Gradient of Magnitude.forward with respect to x (..., K) complex64 / float32, given dF (..., N - col_off).
    bank_cols / bank_t_cols: utils.banded.bank_columns of the (K, N) bank and of its transpose, on x's device
    (None: mel=False).  dx_accum (x's shape and type) is added to the result."""
    require_device(x, dF, scale, dx_accum)
    x = _prep_in(x)
    dF = _f32c(dF)
    K = x.shape[-1]
    N = bank_cols[0].numel() if bank_cols is not None else K
    rows = x.numel() // K
    assert dF.numel() == rows * (N - col_off), "dF does not match the forward's output"
    if dx_accum is not None:
        dx_accum = dx_accum if dx_accum.is_contiguous() else dx_accum.contiguous()
        assert dx_accum.shape == x.shape and dx_accum.dtype == x.dtype
    dx = torch.empty_like(x)
    check(lib().at_magnitude_backward(ptr(x), 0 if torch.is_complex(x) else 3, rows, K, ptr(dF), N, col_off,
                                      *_cols_args(bank_cols), *_cols_args(bank_t_cols), contrast_code(contrast),
                                      ptr(scale), eps, ptr(dx_accum), ptr(dx), stream_ptr()), "at_magnitude_backward")
    return dx


def mfcc_backward(X, dF, bank_t_cols, power=2, bank_cols=None, dct_t=None, scale=None, inplace=False):
    """Gradient of MFCC.forward with respect to the spectrum X (B, T, K) complex64 of its STFT, given dF (B, C, T), the
    gradient of the channel-major output.  bank_t_cols / bank_cols: utils.banded.bank_columns of the transposed
    (K, N) bank and of the bank itself, on X's device; dct_t (C, N): the module's DCT matrix transposed (None: the mel
    power route, C == N, bank_cols not read).  inplace=True writes the result over X and returns X."""
    require_device(X, dF, dct_t, scale)
    X = _c64(X)
    dF = _f32c(dF)
    assert X.is_contiguous() and X.ndim == 3, "X must be a contiguous (B, T, K) spectrum"
    B, T, K = X.shape
    assert bank_t_cols[0].numel() == K, "the transposed bank's tables do not match the spectrum"
    N = dct_t.shape[1] if dct_t is not None else dF.shape[1]
    C = dF.shape[1]
    assert dF.shape == (B, C, T), "dF does not match the forward's output"
    if dct_t is not None:
        assert dct_t.is_contiguous() and dct_t.shape[0] == C and bank_cols is not None and bank_cols[0].numel() == N
    dX = X if inplace else torch.empty_like(X)
    check(lib().at_mfcc_backward(ptr(X), B, T, K, ptr(dF), C, N, int(power),
                                 *_cols_args(bank_cols if dct_t is not None else None), *_cols_args(bank_t_cols),
                                 ptr(dct_t), ptr(scale), ptr(dX), stream_ptr()), "at_mfcc_backward")
    return dX


def _sd_spectra(X, Y):
    """The two spectra of a spectral distance as the kernels read them: contiguous complex64 of one shape (B, ...)."""
    X, Y = _c64(X), _c64(Y)
    assert X.shape == Y.shape and X.ndim >= 2, "X and Y must be spectra of one shape (B, ...)"
    assert X.is_contiguous() and Y.is_contiguous(), "X and Y must be contiguous"
    n = 1
    for d in X.shape[1:]:
        n *= d
    return X, Y, X.shape[0], n


def _distance_sums(workspace_bytes, entry, what, A, Bm, B, n, eps, out):
    """The library's sums `entry` (named `what`) on the cells A, Bm of B clips of n cells, with its workspace."""
    if out is not None:
        assert out.shape == (B, 3) and out.dtype == torch.float64 and out.is_contiguous()
    sums = out if out is not None else torch.empty((B, 3), dtype=torch.float64, device=A.device)
    wsb = workspace_bytes(B, n)
    ws = _workspace(wsb, A.device)
    check(entry(ptr(A), ptr(Bm), B, n, eps, ptr(sums), ptr(ws), wsb, stream_ptr()), what)
    return sums


def spectral_distance_sums(X, Y, eps=1.1920929e-07, out=None):
    """Per-clip sums of the spectral distance between X (generated) and Y (target), both (B, T, F) or (B, n) complex64:
    (B, 3) float64 holding S_D = sum (|X| - |Y|)^2, S_B = sum |Y|^2 and S_L = sum |ln(|X| + eps) - ln(|Y| + eps)|
    (written into `out`, a contiguous (B, 3) float64 tensor, when given).  A clip's bits depend on its own bins only."""
    require_device(X, Y, out)
    X, Y, B, n = _sd_spectra(X, Y)
    return _distance_sums(lib().at_spectral_distance_workspace_bytes, lib().at_spectral_distance_sums,
                          "at_spectral_distance_sums", X, Y, B, n, eps, out)


def spectral_distance_backward(X, Y, sums, gclip, lin_weight=1.0, log_weight=1.0, eps=1.1920929e-07, need_x=True,
                               need_y=False):
    """Backward of lin_weight S_D / S_B + log_weight S_L / n, IN PLACE: X becomes the gradient of its spectrum (need_x)
    and Y of its own (need_y), in the convention stft_backward takes; a spectrum that is not needed is left as it is.
    sums (B, 3) float64: what spectral_distance_sums gave for these spectra; gclip (B,) float32: the gradient of the
    per-clip loss.  Returns (X, Y)."""
    require_device(X, Y, sums, gclip)
    assert X.dtype == torch.complex64 and Y.dtype == torch.complex64, "in place: the spectra must be complex64"
    X, Y, B, n = _sd_spectra(X, Y)
    gclip = _f32c(gclip)
    assert sums.shape == (B, 3) and sums.dtype == torch.float64 and sums.is_contiguous() and gclip.shape == (B,)
    check(lib().at_spectral_distance_backward(ptr(X), ptr(Y), B, n, ptr(sums), ptr(gclip), lin_weight, log_weight, eps,
                                              int(bool(need_x)), int(bool(need_y)), stream_ptr()),
          "at_spectral_distance_backward")
    return X, Y


def mel_rows(X, bank_cols, out=None):
    """Mel rows of a spectrum: X (..., K) complex64 -> |X| @ bank, (..., N) float32 (written into `out`, a contiguous
    float32 tensor of that shape, when given).  bank_cols: utils.banded.bank_columns of the (K, N) bank, on X's device."""
    require_device(X, out, *bank_cols)
    X = _c64(X)
    assert X.is_contiguous(), "X must be contiguous"
    K, N = X.shape[-1], bank_cols[0].numel()
    shape = tuple(X.shape[:-1]) + (N,)
    if out is not None:
        assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous()
    M = out if out is not None else torch.empty(shape, dtype=torch.float32, device=X.device)
    check(lib().at_mel_rows(ptr(X), X.numel() // K, K, N, *_cols_args(bank_cols), ptr(M), stream_ptr()), "at_mel_rows")
    return M


def mel_distance_sums(M, Q, eps=1.1920929e-07, out=None):
    """Per-clip sums of the mel distance between the mel rows M (generated) and Q (target), both (B, T, N) or (B, n)
    float32: (B, 3) float64 holding S_D = sum (M - Q)^2, S_B = sum Q^2 and S_L = sum |ln(M + eps) - ln(Q + eps)|
    (written into `out`, a contiguous (B, 3) float64 tensor, when given).  A clip's bits depend on its own cells only."""
    require_device(M, Q, out)
    M, Q = _f32c(M), _f32c(Q)
    assert M.shape == Q.shape and M.ndim >= 2, "M and Q must be mel rows of one shape (B, ...)"
    B = M.shape[0]
    n = M[0].numel() if B else max(M.numel(), 1)
    return _distance_sums(lib().at_mel_distance_workspace_bytes, lib().at_mel_distance_sums, "at_mel_distance_sums",
                          M, Q, B, n, eps, out)


def mel_distance_backward(S, other, sums, gclip, bank_cols, bank_t_cols, lin_weight=1.0, log_weight=1.0,
                          eps=1.1920929e-07, side=0):
    """Backward of lin_weight S_D / S_B + log_weight S_L / n with respect to ONE spectrum, IN PLACE: S (B, T, K)
    complex64 becomes the gradient of its spectrum, in the convention stft_backward takes.  side 0: S is the generated
    signal's spectrum and `other` (B, T, N) float32 the target's mel rows; side 1: S is the target's spectrum and
    `other` the generated signal's mel rows.  sums (B, 3) float64: what mel_distance_sums gave; gclip (B,) float32: the
    gradient of the per-clip loss; bank_cols / bank_t_cols: utils.banded.bank_columns of the (K, N) bank and of its
    transpose, on S's device.  Returns S."""
    require_device(S, other, sums, gclip, *bank_cols, *bank_t_cols)
    assert S.dtype == torch.complex64 and S.is_contiguous() and S.ndim == 3, "in place: a contiguous (B, T, K) complex64"
    B, T, K = S.shape
    N = bank_cols[0].numel()
    assert bank_t_cols[0].numel() == K, "the transposed bank's tables do not match the spectrum"
    other, gclip = _f32c(other), _f32c(gclip)
    assert other.numel() == B * T * N, "the other signal's mel rows do not match the spectrum"
    assert sums.shape == (B, 3) and sums.dtype == torch.float64 and sums.is_contiguous() and gclip.shape == (B,)
    check(lib().at_mel_distance_backward(ptr(S), ptr(other), B, T, K, N, *_cols_args(bank_cols), *_cols_args(bank_t_cols),
                                         ptr(sums), ptr(gclip), lin_weight, log_weight, eps, int(side), stream_ptr()),
          "at_mel_distance_backward")
    return S


def pqmf_tile_blocks(n_band, taps):
    """Blocks t that one workgroup of the PQMF kernels handles at (n_band, taps); AcidsHipError outside their range."""
    tile = lib().at_pqmf_tile_blocks(int(n_band), int(taps))
    if tile <= 0:
        check(tile, "at_pqmf_tile_blocks")
    return tile


def pqmf_analysis(x, proto, mod, scale=1.0):
    """PQMF analysis: x (rows, L) float32 -> (rows, M, L / M) float32, y[row, k, t] = scale sum_n h_k[n] x[row, tM + n - P]
    with h_k the bank of the prototype `proto` (N,) and the modulation `mod` (M, 2M) (include/acids_hip.h).  The
    backward of pqmf_synthesis with respect to its input, too."""
    require_device(x, proto, mod)
    x = _f32c(x)
    assert x.ndim == 2 and proto.dtype == mod.dtype == torch.float32 and proto.is_contiguous() and mod.is_contiguous()
    M, N = mod.shape[0], proto.numel()
    rows, L = x.shape
    if L % M:
        raise ValueError("the audio length %d is no multiple of n_band = %d" % (L, M))
    y = torch.empty((rows, M, L // M), dtype=torch.float32, device=x.device)
    check(lib().at_pqmf_analysis(ptr(x), rows, L, ptr(proto), N, M, ptr(mod), float(scale), ptr(y), stream_ptr()),
          "at_pqmf_analysis")
    return y


def pqmf_synthesis(y, proto, mod, scale=1.0):
    """PQMF synthesis: y (rows, M, T) float32 -> (rows, M T) float32, x[row, m] = scale sum_k sum_t h_k[m + P - tM]
    y[row, k, t]: the transpose of pqmf_analysis, and so the backward of it with respect to its input."""
    require_device(y, proto, mod)
    y = _f32c(y)
    assert y.ndim == 3 and proto.dtype == mod.dtype == torch.float32 and proto.is_contiguous() and mod.is_contiguous()
    M, N = mod.shape[0], proto.numel()
    rows, bands, T = y.shape
    if bands != M:
        raise ValueError("the band axis holds %d bands, the bank has n_band = %d" % (bands, M))
    x = torch.empty((rows, M * T), dtype=torch.float32, device=y.device)
    check(lib().at_pqmf_synthesis(ptr(y), rows, M * T, ptr(proto), N, M, ptr(mod), float(scale), ptr(x), stream_ptr()),
          "at_pqmf_synthesis")
    return x


def pqmf_stream_sizes(n_band, taps):
    """(D, Ha, Hs) of the streaming PQMF at (n_band, taps): the blocks of delay D = ceil(P / M), the samples of carried
    analysis state Ha = D M + P and the blocks per band of carried synthesis state Hs = D + floor(P / M)."""
    M, P = int(n_band), (int(taps) - 1) // 2
    D = -(-P // M)
    return D, D * M + P, D + P // M


def _stream_state(state, shape, like):
    """The carried float32 state of a streaming stage as its kernel reads it (None: zeros), on `like`'s device."""
    if state is None:
        return None
    require_device(like, state)
    state = _f32c(state)
    assert tuple(state.shape) == shape, "the carried state is %s, the stream needs %s" % (tuple(state.shape), shape)
    return state


def pqmf_analysis_stream(x, state, proto, mod, scale=1.0, shift=None, want_state=True):
    """PQMF analysis of a chunk of a stream: x (rows, C) float32, state (rows, Ha) float32 -- the samples before the
    chunk -- or None for zeros -> (y (rows, M, C / M), new_state (rows, Ha) or None), y[row, k, t] = scale sum_n h_k[n]
    s[row, (t + shift) M + n - P] over s = [state | x | zeros] (include/acids_hip.h).  shift=None is -D, the causal
    bank delayed by D blocks; shift=+D with state=None and want_state=False is the backward of pqmf_synthesis_stream
    with respect to its chunk.  new_state is a fresh tensor, the last Ha samples of [state | x], written by the kernel:
    no torch.cat, one launch.  An empty chunk or batch launches nothing and hands the state back as it came."""
    require_device(x, proto, mod)
    x = _f32c(x)
    assert x.ndim == 2 and proto.dtype == mod.dtype == torch.float32 and proto.is_contiguous() and mod.is_contiguous()
    M, N = mod.shape[0], proto.numel()
    rows, C = x.shape
    if C % M:
        raise ValueError("the chunk length %d is no multiple of n_band = %d" % (C, M))
    D, Ha, _ = pqmf_stream_sizes(M, N)
    state = _stream_state(state, (rows, Ha), x)
    y = torch.empty((rows, M, C // M), dtype=torch.float32, device=x.device)
    if rows == 0 or C == 0:
        return y, (state if want_state else None)
    new_state = torch.empty((rows, Ha), dtype=torch.float32, device=x.device) if want_state else None
    check(lib().at_pqmf_analysis_stream(ptr(x), rows, C, ptr(state), ptr(new_state), -D if shift is None else int(shift),
                                        ptr(proto), N, M, ptr(mod), float(scale), ptr(y), stream_ptr()),
          "at_pqmf_analysis_stream")
    return y, new_state


def pqmf_synthesis_stream(y, state, proto, mod, scale=1.0, shift=None, want_state=True):
    """PQMF synthesis of a chunk of a stream: y (rows, M, c) float32, state (rows, M, Hs) float32 -- the blocks before
    the chunk -- or None for zeros -> (x (rows, M c), new_state (rows, M, Hs) or None), x[row, m] = scale sum_k sum_t
    h_k[m + shift M + P - tM] s[row, k, t] over s = [state | y | zeros] with the chunk's first block at t = 0.
    shift=None is -D; shift=+D with state=None and want_state=False is the backward of pqmf_analysis_stream with
    respect to its chunk.  new_state is a fresh tensor, the last Hs blocks of [state | y], written by the kernel."""
    require_device(y, proto, mod)
    y = _f32c(y)
    assert y.ndim == 3 and proto.dtype == mod.dtype == torch.float32 and proto.is_contiguous() and mod.is_contiguous()
    M, N = mod.shape[0], proto.numel()
    rows, bands, c = y.shape
    if bands != M:
        raise ValueError("the band axis holds %d bands, the bank has n_band = %d" % (bands, M))
    D, _, Hs = pqmf_stream_sizes(M, N)
    state = _stream_state(state, (rows, M, Hs), y)
    x = torch.empty((rows, M * c), dtype=torch.float32, device=y.device)
    if rows == 0 or c == 0:
        return x, (state if want_state else None)
    new_state = torch.empty((rows, M, Hs), dtype=torch.float32, device=y.device) if want_state else None
    check(lib().at_pqmf_synthesis_stream(ptr(y), rows, M * c, ptr(state), ptr(new_state), -D if shift is None else int(shift),
                                         ptr(proto), N, M, ptr(mod), float(scale), ptr(x), stream_ptr()),
          "at_pqmf_synthesis_stream")
    return x, new_state


def _c64_grad(g):
    """A complex gradient as the kernels read it: complex64, contiguous, 8-byte aligned (a slice of a cat's gradient
    always is: complex64 elements)."""
    g = _c64(g)
    return g if g.is_contiguous() else g.contiguous()


def magnitude_invert_backward(y, g, bank_t_cols=None, contrast=None, offset=None, scale=None, eps=1.1920929e-07,
                              pad_last=False, bank_cols=None, phase_offset=None, phase_scale=None):
    """Gradient of Magnitude.invert with respect to y (..., K - pad_last) float32, given g (..., N), the gradient of its
    output.  bank_t_cols: utils.banded.bank_columns of the (K, N) inverse bank TRANSPOSED, on y's device (None:
    mel=False, N == K).  pad_last: keep_nyquist=False (the reference's zero pad is the last of the K columns).
    bank_cols given (bank_columns of the inverse bank itself): the one-pass Polar.invert -- y (..., 2, F) stacked, g the
    complex gradient (..., F), the result has y's shape with both halves written."""
    polar = bank_cols is not None
    require_device(y, g, offset, scale, phase_offset, phase_scale)
    y = _f32c(y)
    g = _c64_grad(g) if polar else _f32c(g)
    pad = int(bool(pad_last))
    if polar:
        K = N = y.shape[-1]
        assert y.ndim >= 2 and y.shape[-2] == 2 and bank_t_cols is not None and not pad
        assert bank_cols[0].numel() == N and bank_t_cols[0].numel() == K, "the tables do not match the stacked tensor"
        rows = y.numel() // (2 * K)
    else:
        K = y.shape[-1] + pad
        N = g.shape[-1]
        if bank_t_cols is not None:
            assert bank_t_cols[0].numel() == K, "the transposed bank's tables do not match the input"
        else:
            assert N == K, "mel=False: the gradient has the input's columns (plus the pad)"
        rows = g.numel() // N
        assert y.numel() == rows * (K - pad), "g does not match the forward's output"
    assert g.numel() == rows * N, "g does not match the forward's output"
    dy = torch.empty_like(y)
    check(lib().at_magnitude_invert_backward(ptr(y), rows, K, N, pad, ptr(g), int(polar),
                                             *_cols_args(bank_cols), *_cols_args(bank_t_cols),
                                             contrast_code(contrast), ptr(offset), ptr(scale), eps, ptr(phase_offset),
                                             ptr(phase_scale), ptr(dy), stream_ptr()), "at_magnitude_invert_backward")
    return dy


def polar_to_complex_backward(gX, mag, phase, need_mag=True, need_phase=True):
    """Gradient of polar_to_complex: gX complex64 of mag's (contiguous float32) shape -> (gmag, gphase), None for the
    one that is not needed."""
    require_device(gX, mag, phase)
    gX = _c64_grad(gX)
    mag, phase = _f32c(mag), _f32c(phase)
    assert gX.shape == mag.shape == phase.shape
    gmag = torch.empty_like(mag) if need_mag else None
    gphase = torch.empty_like(phase) if need_phase else None
    check(lib().at_polar_to_complex_backward(ptr(gX), ptr(mag), ptr(phase), gX.numel(), ptr(gmag), ptr(gphase),
                                             stream_ptr()), "at_polar_to_complex_backward")
    return gmag, gphase


def cartesian_inverse_backward(gX, re_scale=None, im_scale=None):
    """Gradient of cartesian_inverse: gX (..., F) complex64 -> (..., 2, F) float32 = [Re gX * re_scale, Im gX * im_scale]."""
    require_device(gX, re_scale, im_scale)
    gX = _c64_grad(gX)
    F = gX.shape[-1]
    dy = torch.empty(gX.shape[:-1] + (2, F), dtype=torch.float32, device=gX.device)
    check(lib().at_cartesian_unpack_backward(ptr(gX), gX.numel() // F if F else 0, F, ptr(re_scale), ptr(im_scale),
                                             ptr(dy), stream_ptr()), "at_cartesian_unpack_backward")
    return dy


# ----------------------------------------------------------------------------------------------
# phase-side representations (phase_repr.hip)
# ----------------------------------------------------------------------------------------------
SCAN_MODES = {"unwrap": 0, "forward": 1, "backward": 2, "central": 3, "angle": 4}


def _btf(x):
    if x.ndim < 2:
        raise IndexError("expected (..., frames, bins), got shape %s" % (tuple(x.shape),))
    T, F = x.shape[-2], x.shape[-1]
    return x.numel() // max(T * F, 1) if T * F else 0, T, F


def phase_scan(x, mode, frame_window=None, offset=None, scale=None, bare=False):
    """Scan along dim -2 of x (..., T, F): complex64 spectrum (the angle is taken inside) or float32 phase.
    mode: "angle" | "unwrap" | "forward" | "backward" | "central" (IF of the unwrapped phase, reference row
    scaling included); bare=True: the plain fdiff_* of a real signal.  Optional per-frame weight (T,) and
    Normalize affine are applied last.  Returns float32 of x's shape."""
    if mode not in SCAN_MODES:
        raise AttributeError("method %s not known" % mode)
    require_device(x)
    cplx = x.is_complex()
    x = _c64(x) if cplx else _f32c(x)
    x = x if x.is_contiguous() else x.contiguous()
    B, T, F = _btf(x)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if frame_window is not None:
        frame_window = _f32c(frame_window.to(x.device))
        assert frame_window.numel() == T
    check(lib().at_phase_scan(ptr(x) if cplx else None, None if cplx else ptr(x), B, T, F, SCAN_MODES[mode], int(bare),
                              ptr(frame_window), ptr(offset), ptr(scale), ptr(out), stream_ptr()), "at_phase_scan")
    return out


def _grad_rows(g, F):
    """(g, ld_g): a float32 gradient (..., T, F) as evenly spaced rows of ld_g >= F floats.  The half of a stacked
    (..., T, 2, F) gradient that torch's stack / select hand back (ld_g = 2 F) is read where it lies; anything else that
    is not contiguous is copied."""
    _no_fp64(g, "gradient")
    g = g if g.dtype == torch.float32 else g.float()
    if g.is_contiguous():
        return g, F
    if g.ndim >= 2 and (F == 1 or g.stride(-1) == 1):
        ld, want = None, None
        for d in range(g.ndim - 2, -1, -1):
            if g.shape[d] == 1:
                continue
            if ld is None:
                ld = want = g.stride(d)
            elif g.stride(d) != want:
                ld = -1
                break
            want = want * g.shape[d]
        if ld is None:
            return g, F
        if ld >= F:
            return g, ld
    return g.contiguous(), F


def phase_scan_backward(x, mode, g, frame_window=None, scale=None, accum=None, out=None):
    """Gradient of phase_scan(x, mode, frame_window, offset, scale) with respect to the complex64 spectrum x (..., T, F),
    given g (..., T, F) float32, the gradient of its output -- the phase half of a stacked (..., T, 2, F) gradient,
    `g_stacked[..., 1, :]`, is read in place.  accum (complex64, x's shape) is added to the result; out (complex64, x's
    shape, contiguous) receives it and may be x or accum.  Returns complex64 of x's shape."""
    if mode not in SCAN_MODES:
        raise AttributeError("method %s not known" % mode)
    require_device(x, g, scale, accum, out)
    assert x.is_complex(), "the gradient is that of a complex spectrum"
    x = _c64(x)
    x = x if x.is_contiguous() else x.contiguous()
    B, T, F = _btf(x)
    g, ld_g = _grad_rows(g, F)
    assert g.shape == x.shape, "g does not match the forward's output"
    if frame_window is not None:
        frame_window = _f32c(frame_window.to(x.device))
        assert frame_window.numel() == T
    for t in (accum, out):
        assert t is None or (t.shape == x.shape and t.dtype == torch.complex64 and t.is_contiguous())
    if out is None:
        out = torch.empty_like(x)
    check(lib().at_phase_scan_backward(ptr(x), B, T, F, SCAN_MODES[mode], ptr(g), ld_g, ptr(frame_window), ptr(scale),
                                       ptr(accum), ptr(out), stream_ptr()), "at_phase_scan_backward")
    return out


def cartesian_forward_backward(g, re_scale=None, im_scale=None):
    """Gradient of cartesian_forward: g (..., 2, F) float32 -> (..., F) complex64 = g[.., 0, :] / re_scale +
    i g[.., 1, :] / im_scale."""
    require_device(g, re_scale, im_scale)
    g = _f32c(g)
    assert g.ndim >= 2 and g.shape[-2] == 2, "g must be the stacked (..., 2, F) gradient"
    F = g.shape[-1]
    out = torch.empty(g.shape[:-2] + (F,), dtype=torch.complex64, device=g.device)
    check(lib().at_cartesian_pack_backward(ptr(g), g.numel() // (2 * F) if F else 0, F, ptr(re_scale), ptr(im_scale),
                                           ptr(out), stream_ptr()), "at_cartesian_pack_backward")
    return out


def phase_integrate(y, method, offset=None, scale=None, rescale=True):
    """IF.invert's tail: (de-normalise,) undo the row scaling of `method` (rescale) and integrate along dim -2."""
    if method not in ("forward", "backward", "central"):
        raise AttributeError("method %s not known" % method)
    require_device(y)
    y = _f32c(y)
    B, T, F = _btf(y)
    out = torch.empty_like(y)
    check(lib().at_phase_integrate(ptr(y), B, T, F, SCAN_MODES[method], int(rescale), ptr(offset), ptr(scale), ptr(out),
                                   stream_ptr()), "at_phase_integrate")
    return out


def polarif_forward(x, band, contrast, mag_offset, mag_scale, eps, method, frame_window=None, if_offset=None,
                    if_scale=None):
    """PolarIF.forward written straight into the stacked tensor: x (..., T, F) complex64 -> (..., T, 2, F) with
    [..., 0, :] = normalise(contrast(|x| @ bank)) (banded bank with F filters) and [..., 1, :] = normalise(IF(x))."""
    import ctypes
    require_device(x)
    x = _prep_in(x)
    B, T, F = _btf(x)
    assert band.N == F and band.K == F and band.eligible and method in ("forward", "backward", "central")
    out = torch.empty(x.shape[:-1] + (2, F), dtype=torch.float32, device=x.device)
    if frame_window is not None:
        frame_window = _f32c(frame_window.to(x.device))
        assert frame_window.numel() == T
    # one pass over the spectrum where the clip-per-block scan applies (>= 64 clips, 256..2048 bins; the library answers
    # AT_EUNSUPPORTED otherwise, and under variant("scan_layout", 1)); same bits as the two kernels below
    start, length, woff, w = band.by_filter(x.device)
    err = lib().at_polarif_forward(ptr(x), B, T, F, SCAN_MODES[method], ptr(frame_window), ptr(if_offset), ptr(if_scale),
                                   ptr(start), ptr(length), ptr(woff), ptr(w), w.numel(), contrast_code(contrast),
                                   ptr(mag_offset), ptr(mag_scale), float(eps), ptr(out), stream_ptr())
    if err != AT_EUNSUPPORTED:
        check(err, "at_polarif_forward")
        return out
    _project_banded(x, 0, band, contrast, False, mag_offset, mag_scale, eps, out, F, 0, ld_out=2 * F)
    check(lib().at_phase_scan_strided(ptr(x), None, B, T, F, SCAN_MODES[method], 0, ptr(frame_window), ptr(if_offset),
                                      ptr(if_scale), ctypes.c_void_p(out.data_ptr() + 4 * F), 2 * F, stream_ptr()),
          "at_phase_scan_strided")
    return out


def polarif_inverse(y, inv_band, contrast, mag_offset, mag_scale, eps, method, if_offset=None, if_scale=None):
    """PolarIF.invert reading the stacked tensor in place: y (..., T, 2, F) -> (..., T, F) complex64 =
    Magnitude.invert(y[.., 0, :]) * exp(i * IF.invert(y[.., 1, :]))."""
    import ctypes
    require_device(y)
    y = _f32c(y)
    F = y.shape[-1]
    T = y.shape[-3]
    rows = y.numel() // (2 * F)
    assert inv_band.K == F and inv_band.N == F and inv_band.eligible and method in ("forward", "backward", "central")
    mag = torch.empty(y.shape[:-2] + (F,), dtype=torch.float32, device=y.device)
    _project_banded(y, 2, inv_band, contrast, True, mag_offset, mag_scale, eps, mag, F, 0, rows=rows, lda=2 * F)
    out = torch.empty(y.shape[:-2] + (F,), dtype=torch.complex64, device=y.device)
    check(lib().at_phase_integrate_polar(ctypes.c_void_p(y.data_ptr() + 4 * F), 2 * F, rows // T, T, F, SCAN_MODES[method],
                                         ptr(if_offset), ptr(if_scale), ptr(mag), ptr(out), stream_ptr()),
          "at_phase_integrate_polar")
    return out


def cartesian_forward(x, re_offset=None, re_scale=None, im_offset=None, im_scale=None):
    """Cartesian.forward in one pass: x (..., F) complex64 -> (..., 2, F) = [normalise(x.real), normalise(x.imag)]."""
    require_device(x)
    x = _prep_in(x)
    F = x.shape[-1]
    out = torch.empty(x.shape[:-1] + (2, F), dtype=torch.float32, device=x.device)
    check(lib().at_cartesian_pack(ptr(x), x.numel() // F, F, ptr(re_offset), ptr(re_scale), ptr(im_offset), ptr(im_scale),
                                  ptr(out), stream_ptr()), "at_cartesian_pack")
    return out


def cartesian_inverse(y, re_offset=None, re_scale=None, im_offset=None, im_scale=None):
    """Cartesian.invert in one pass: y (..., 2, F) float32 -> (..., F) complex64."""
    require_device(y)
    y = _f32c(y)
    F = y.shape[-1]
    out = torch.empty(y.shape[:-2] + (F,), dtype=torch.complex64, device=y.device)
    check(lib().at_cartesian_unpack(ptr(y), y.numel() // (2 * F), F, ptr(re_offset), ptr(re_scale), ptr(im_offset),
                                    ptr(im_scale), ptr(out), stream_ptr()), "at_cartesian_unpack")
    return out


def polar_to_complex(mag, phase):
    """mag * exp(1j * phase) as complex64."""
    require_device(mag, phase)
    mag, phase = torch.broadcast_tensors(mag, phase)
    mag, phase = _f32c(mag), _f32c(phase)
    out = torch.empty(mag.shape, dtype=torch.complex64, device=mag.device)
    check(lib().at_polar_to_complex(ptr(mag), ptr(phase), mag.numel(), ptr(out), stream_ptr()), "at_polar_to_complex")
    return out


# ----------------------------------------------------------------------------------------------
# sinebank inversion (sinebank.hip)
# ----------------------------------------------------------------------------------------------
def sinebank_offline(x, c, t, phi, block_frame_offset, W3, max_abs, n_pass):
    """x (B, T, F) magnitudes -> (B, L) oscillator-bank resynthesis before the final max-normalisation.
    c (F,), t (L,), phi (F,), W3 (n_pass, L) float32 and block_frame_offset (n_pass, ceil(L/128)) int64 on x's
    device."""
    require_device(x, c, t, phi, block_frame_offset, W3, max_abs)
    c, t, phi, W3 = _f32c(c), _f32c(t), _f32c(phi), _f32c(W3)
    block_frame_offset = block_frame_offset.contiguous()
    x = _f32c(x)
    B, T, F = x.shape
    L = t.numel()
    out = torch.empty((B, L), dtype=torch.float32, device=x.device)
    wsb = lib().at_sinebank_workspace_bytes(B, F, L, n_pass)
    ws = _workspace(wsb, x.device)
    check(lib().at_sinebank_offline(ptr(x), B, T, F, ptr(c), ptr(t), ptr(phi), L, n_pass, ptr(block_frame_offset), ptr(W3),
                                    ptr(max_abs), ptr(out), ptr(ws), wsb, stream_ptr()), "at_sinebank_offline")
    return out


def sinebank_realtime(x, c, tau, phi, window=None):
    """x (S, T, F), tau (T, N), phi (S, F) -> (S, T, N) frames (times window (N,) when given)."""
    require_device(x, c, tau, phi, window)
    window = _f32c(window) if window is not None else None
    x, c, tau, phi = _f32c(x), _f32c(c), _f32c(tau), _f32c(phi)
    S, T, F = x.shape
    N = tau.shape[-1]
    out = torch.empty((S, T, N), dtype=torch.float32, device=x.device)
    check(lib().at_sinebank_realtime(ptr(x), S, T, F, N, ptr(c), ptr(tau), ptr(phi), ptr(window), ptr(out),
                                     stream_ptr()), "at_sinebank_realtime")
    return out


def resample_sinc(x, orig, new, width, filters):
    """x (rows, L) -> (rows, ceil(new * L / orig)) through the (new, 2*width + orig) polyphase bank."""
    require_device(x, filters)
    x, filters = _f32c(x), _f32c(filters)
    rows, L = x.shape
    out_len = -(-new * L // orig)
    out = torch.empty((rows, out_len), dtype=torch.float32, device=x.device)
    check(lib().at_resample_sinc(ptr(x), rows, L, orig, new, width, ptr(filters), out_len, ptr(out), stream_ptr()),
          "at_resample_sinc")
    return out


def resample_backward_plan(orig, new, taps, lead):
    """(tile_blocks, bank_in_lds) of at_resample_sinc_backward at a shape: the whole input blocks one workgroup handles,
    and whether the bank sits in LDS beside the window of g or is read through L1 / L2.  Reads no device state."""
    import ctypes
    tile, in_lds = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().at_resample_backward_plan(int(orig), int(new), int(taps), int(lead), ctypes.byref(tile),
                                          ctypes.byref(in_lds)), "at_resample_backward_plan")
    return tile.value, bool(in_lds.value)


def resample_sinc_backward(g, L, orig, new, taps, lead, filters):
    """The adjoint of resample_sinc with respect to its input: g (rows, out_len) -> gx (rows, L), gx[n] = sum over the
    output samples o = i new + j that read input n of filters[j][n - i orig + lead] g[o] (include/acids_hip.h).  lead =
    width is the offline converter's; lead = Ha over a chunk's own output blocks is resample_sinc_stream's."""
    require_device(g, filters)
    g, filters = _f32c(g), _f32c(filters)
    assert g.ndim == 2 and tuple(filters.shape) == (new, taps)
    rows, out_len = g.shape
    gx = torch.empty((rows, int(L)), dtype=torch.float32, device=g.device)
    check(lib().at_resample_sinc_backward(ptr(g), rows, int(L), orig, new, taps, lead, ptr(filters), out_len, ptr(gx),
                                          stream_ptr()), "at_resample_sinc_backward")
    return gx


def resample_stream_sizes(orig, width):
    """(D, Ha) of the streaming converter: the blocks of delay D = ceil(width / orig) and the samples of carried state
    Ha = D orig + width."""
    D = -(-int(width) // int(orig))
    return D, D * int(orig) + int(width)


def resample_sinc_stream(x, state, orig, new, width, filters, want_state=True):
    """Sample-rate conversion of a chunk of a stream: x (rows, C) float32, C a multiple of orig, state (rows, Ha)
    float32 -- the samples before the chunk -- or None for zeros -> (y (rows, C new / orig), new_state (rows, Ha) or
    None): resample_sinc's chain over [state | x], delayed by D blocks (include/acids_hip.h).  new_state is a fresh
    tensor, the last Ha samples of [state | x], written by the same launch: no torch.cat.  An empty chunk or batch
    launches nothing and hands the state back as it came."""
    require_device(x, filters)
    x, filters = _f32c(x), _f32c(filters)
    assert x.ndim == 2 and tuple(filters.shape) == (new, 2 * width + orig)
    rows, C = x.shape
    if C % orig:
        raise ValueError("the chunk length %d is no multiple of orig = %d" % (C, orig))
    _, Ha = resample_stream_sizes(orig, width)
    state = _stream_state(state, (rows, Ha), x)
    y = torch.empty((rows, C // orig * new), dtype=torch.float32, device=x.device)
    if rows == 0 or C == 0:
        return y, (state if want_state else None)
    new_state = torch.empty((rows, Ha), dtype=torch.float32, device=x.device) if want_state else None
    check(lib().at_resample_sinc_stream(ptr(x), rows, C, ptr(state), ptr(new_state), orig, new, width, ptr(filters),
                                        ptr(y), stream_ptr()), "at_resample_sinc_stream")
    return y, new_state


# ----------------------------------------------------------------------------------------------
# sample-rate conversion without the bank (sinc_interp.hip)
# ----------------------------------------------------------------------------------------------
SINC_TABLE_MAX = 2 ** 24           # entries of a half-table: 64 MB, rates up to about 2.7 million after the gcd


def _reduced_rates(orig_freq, new_freq):
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError("sample rates must be >= 1, got %d and %d" % (orig_freq, new_freq))
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def sinc_table(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """The half-table of the converter orig -> new (reduced by their gcd here): (table float32 (Qi + 1,) on the CPU, Qi).
    An entry h[j][k] of utils.audio_io.sinc_filter_bank depends only on q = n new - o orig:
        table[q] = (min(orig, new) rolloff / orig) sinc(pi q rho) cos^2(pi q rho / (2 lpw)),   rho = rolloff / max(orig, new)
    in float64 with sinc(0) = 1, rounded to float32; Qi is the largest integer < lpw / rho, beyond which the bank is
    exactly 0.  ValueError: rates < 1, lpw < 1, a rolloff outside (0, 1], more than SINC_TABLE_MAX entries."""
    orig, new = _reduced_rates(orig, new)
    lpw, rolloff = int(lowpass_filter_width), float(rolloff)
    if lpw < 1 or not 0.0 < rolloff <= 1.0:
        raise ValueError("lowpass_filter_width must be >= 1 and rolloff in (0, 1], got %r and %r"
                         % (lowpass_filter_width, rolloff))
    base_freq = min(orig, new) * rolloff
    edge = lpw * orig * new / base_freq                   # lpw / rho
    Qi = math.ceil(edge) - 1
    if Qi + 1 > SINC_TABLE_MAX:
        raise ValueError("the converter %d -> %d needs a table of %d entries, more than %d" % (orig, new, Qi + 1,
                                                                                              SINC_TABLE_MAX))
    t = torch.arange(0, Qi + 1, dtype=torch.float64) / orig / new
    t = (t * base_freq).clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    return (kernels * window * (base_freq / orig)).to(torch.float32).contiguous(), Qi


_sinc_tables = {}


def _sinc_table_on(device, orig, new, lowpass_filter_width=6, rolloff=0.99):
    """sinc_table on `device`, for reduced rates; the last few tables stay (one upload per converter and device)."""
    key = (str(device), int(orig), int(new), int(lowpass_filter_width), float(rolloff))
    hit = _sinc_tables.get(key)
    if hit is None:
        table, Qi = sinc_table(orig, new, lowpass_filter_width, rolloff)
        if len(_sinc_tables) >= 16:
            _sinc_tables.pop(next(iter(_sinc_tables)))
        hit = _sinc_tables[key] = (table.to(device), Qi)
    return hit


def sinc_interp_plan(a, b, Qi):
    """(tile_outputs, table_in_lds) of at_sinc_interp at a shape: the consecutive outputs one workgroup handles, and
    whether the table sits in LDS beside the input window or is read from global memory.  Reads no device state."""
    import ctypes
    tile, in_lds = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().at_sinc_interp_plan(int(a), int(b), int(Qi), ctypes.byref(tile), ctypes.byref(in_lds)),
          "at_sinc_interp_plan")
    return tile.value, bool(in_lds.value)


def sinc_interp(x, a, b, table, Qi, out_len):
    """x (rows, in_len) -> (rows, out_len), out[r][o] = sum over n ascending with |n b - o a| <= Qi of
    table[|n b - o a|] x[r][n] (include/acids_hip.h, at_sinc_interp): the converter with (a, b) = (orig, new) and its
    adjoint with (a, b) = (new, orig)."""
    require_device(x, table)
    x, table = _f32c(x), _f32c(table)
    assert x.ndim == 2 and table.ndim == 1 and table.numel() == int(Qi) + 1
    rows, in_len = x.shape
    out = torch.empty((rows, int(out_len)), dtype=torch.float32, device=x.device)
    check(lib().at_sinc_interp(ptr(x), rows, in_len, int(a), int(b), ptr(table), int(Qi), int(out_len), ptr(out),
                               stream_ptr()), "at_sinc_interp")
    return out


def resample_direct(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio.functional.resample with its default interpolation, for any pair of rates: x (..., L) -> (...,
    ceil(new L / orig)) through the half-table of the converter, no bank (sinc_interp.hip).  For finite input the bits
    of utils.Resample.  Equal rates return x itself.  No graph: autograd.ResampleDirectFunction is the differentiable
    form."""
    orig, new = _reduced_rates(orig_freq, new_freq)
    if orig == new:
        return x
    require_device(x)
    _no_fp64(x)
    table, Qi = _sinc_table_on(x.device, orig, new, lowpass_filter_width, rolloff)
    lead, L = tuple(x.shape[:-1]), x.shape[-1]
    out_len = -(-new * L // orig)
    y = sinc_interp(x.reshape(math.prod(lead), L), orig, new, table, Qi, out_len)
    return y.reshape(lead + (out_len,))


def resample_direct_backward(g, L, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The adjoint of resample_direct with respect to its input: g (..., ceil(new L / orig)) -> gx (..., L), the same
    kernel with the two rates exchanged.  For finite g the bits of resample_sinc_backward."""
    orig, new = _reduced_rates(orig_freq, new_freq)
    if orig == new:
        return g
    require_device(g)
    _no_fp64(g, "gradient")
    lead, out_len = tuple(g.shape[:-1]), g.shape[-1]
    assert out_len == -(-new * int(L) // orig), "g does not match the forward's output"
    table, Qi = _sinc_table_on(g.device, orig, new, lowpass_filter_width, rolloff)
    gx = sinc_interp(g.reshape(math.prod(lead), out_len), new, orig, table, Qi, int(L))
    return gx.reshape(lead + (int(L),))


# ----------------------------------------------------------------------------------------------
# time stretching (phase_vocoder.hip)
# ----------------------------------------------------------------------------------------------
PV_MAX_ROWS = 2 ** 31 - 1 - 8      # at_phase_vocoder's int row indices, a batch of rows ahead included


def phase_vocoder_steps(T, rate):
    """The step table of the phase vocoder on the host, in float64: s_j = j * rate for j = 0, 1, ... while s_j < T ->
    (idx int32 (N,), alpha float32 (N,)) CPU tensors, idx_j = floor(s_j), alpha_j = s_j - idx_j rounded to float32.  N is
    ceil(T / rate) except for rounding at the edge; idx_j + 1 may be T, the frame of zeros.  ValueError: a rate that is not
    finite and > 0, a negative T, more rows than the kernel's index range (PV_MAX_ROWS)."""
    import math
    rate, T = float(rate), int(T)
    if not (math.isfinite(rate) and rate > 0.0):
        raise ValueError("rate must be finite and > 0, got %r" % (rate,))
    if T < 0:
        raise ValueError("a clip has T >= 0 frames, got %d" % T)
    if T / rate > PV_MAX_ROWS:
        raise ValueError("%d frames at rate %g are more than %d output frames" % (T, rate, PV_MAX_ROWS))
    s = torch.arange(int(math.ceil(T / rate)) + 2, dtype=torch.float64) * rate      # monotone in j
    s = s[:int((s < T).sum())]
    idx = s.floor()
    return idx.to(torch.int32), (s - idx).to(torch.float32)


_pv_tables = {}


def _pv_table(T, rate, device):
    """phase_vocoder_steps on `device`; the last few tables stay (one upload per shape, rate and device)."""
    key = (int(T), float(rate), str(device))
    hit = _pv_tables.get(key)
    if hit is None:
        idx, alpha = phase_vocoder_steps(T, rate)
        if len(_pv_tables) >= 16:
            _pv_tables.pop(next(iter(_pv_tables)))
        hit = _pv_tables[key] = (idx.to(device), alpha.to(device))
    return hit


def _pv_spectrum(x, rate):
    rate = float(rate)
    if not (rate == rate and 0.0 < rate < float("inf")):
        raise ValueError("rate must be finite and > 0, got %r" % (rate,))
    if not x.is_complex():
        raise ValueError("the phase vocoder stretches a complex spectrum (..., frames, bins), got %s"
                         % str(x.dtype).replace("torch.", ""))
    require_device(x)
    x = _c64(x)
    return x if x.is_contiguous() else x.contiguous()


def phase_vocoder(x, rate, want_phasor=False):
    """Time-stretch the complex spectrum x (..., T, F) by `rate` (> 1: shorter) along dim -2: the phase vocoder of
    torchaudio.functional.phase_vocoder in the package's time-major layout, as a running product of unit phasors
    (include/acids_hip.h, at_phase_vocoder; hop_length cancels).  Returns complex64 (..., N, F), N rows of
    phase_vocoder_steps(T, rate); with want_phasor=True also the phasor after the last step (..., F), which
    phase_vocoder_backward starts from.  Zero bins come out as zeros; -0 + 0i counts as zero, where torch.angle says pi."""
    x = _pv_spectrum(x, rate)
    B, T, F = _btf(x)
    idx, alpha = _pv_table(T, rate, x.device)
    N = idx.numel()
    out = torch.empty(x.shape[:-2] + (N, F), dtype=torch.complex64, device=x.device)
    fin = torch.empty(x.shape[:-2] + (F,), dtype=torch.complex64, device=x.device) if want_phasor else None
    check(lib().at_phase_vocoder(ptr(x), B, T, F, ptr(idx), ptr(alpha), N, ptr(out), ptr(fin), stream_ptr()),
          "at_phase_vocoder")
    return (out, fin) if want_phasor else out


def phase_vocoder_backward(x, g, rate, phasor):
    """Gradient of phase_vocoder(x, rate) with respect to x (..., T, F) complex64, given g (..., N, F), the gradient of
    its output, and the final phasor (..., F) the forward handed back (include/acids_hip.h, at_phase_vocoder_backward).
    Returns complex64 of x's shape: zeros where x == 0 and in frames no step reads."""
    x = _pv_spectrum(x, rate)
    require_device(x, g, phasor)
    B, T, F = _btf(x)
    idx, alpha = _pv_table(T, rate, x.device)
    N = idx.numel()
    g, phasor = _c64_grad(g), _c64_grad(phasor)
    assert tuple(g.shape) == tuple(x.shape[:-2]) + (N, F), "g does not match the forward's output"
    assert tuple(phasor.shape) == tuple(x.shape[:-2]) + (F,), "the phasor does not match the forward's"
    gx = torch.empty_like(x)
    check(lib().at_phase_vocoder_backward(ptr(x), ptr(g), ptr(idx), ptr(alpha), ptr(phasor), B, T, F, N, ptr(gx),
                                          stream_ptr()), "at_phase_vocoder_backward")
    return gx


# ----------------------------------------------------------------------------------------------
# recursive filters (sos_filter.hip)
# ----------------------------------------------------------------------------------------------
SOS_MAX_SECTIONS = 16


class _Sos:
    """Coefficients that sos_coefficients has checked: (n, 6) float64 on the host, C order, a0 == 1."""

    def __init__(self, array):
        import ctypes
        self.array = array
        self.n = array.shape[0]
        self.ptr = ctypes.c_void_p(array.ctypes.data)


def sos_coefficients(sos):
    """Anything array-like of shape (n, 6) -- b0 b1 b2 a0 a1 a2 per section, scipy's layout -> the float64 host array the
    kernel takes, each section divided by its a0.  ValueError: a shape that is not (n >= 1, 6), a0 == 0, a non-finite
    entry.  (More than SOS_MAX_SECTIONS sections are the library's AT_EUNSUPPORTED.)"""
    import numpy as np
    if isinstance(sos, _Sos):
        return sos
    if isinstance(sos, torch.Tensor):
        sos = sos.detach().cpu().numpy()
    a = np.array(sos, dtype=np.float64, order="C", ndmin=1)
    if a.ndim != 2 or a.shape[1] != 6 or a.shape[0] < 1:
        raise ValueError("sos must have shape (n_sections >= 1, 6), got %s" % (tuple(a.shape),))
    if not np.isfinite(a).all():
        raise ValueError("sos has non-finite entries")
    if (a[:, 3] == 0.0).any():
        raise ValueError("a section of sos has a0 == 0")
    a = np.ascontiguousarray(a / a[:, 3:4])
    if not np.isfinite(a).all():
        raise ValueError("sos has non-finite entries after the division by a0")
    a[:, 3] = 1.0
    return _Sos(a)


def sos_filter_plan(rows, L, n_sections):
    """(tile, per_lane, dispatch) of at_sos_filter at a shape: the samples a workgroup handles per step of its walk along a
    row, the consecutive samples of one lane, and which dispatch runs (there is one: 0).  Reads no device state."""
    import ctypes
    tile, per_lane, dispatch = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
    check(lib().at_sos_filter_plan(int(rows), int(L), int(n_sections), ctypes.byref(tile), ctypes.byref(per_lane),
                                   ctypes.byref(dispatch)), "at_sos_filter_plan")
    return tile.value, per_lane.value, dispatch.value


def sos_filter(x, sos, zi=None, reverse=False, return_state=False):
    """A cascade of second-order sections along the last axis of x (..., L) float32 -> (..., L) float32: scipy.signal.sosfilt's
    recurrence and state layout, computed in double and rounded once (include/acids_hip.h, at_sos_filter).  sos: see
    sos_coefficients.  zi (..., n_sections, 2) FLOAT64 on x's device is the state before the first sample (None: zeros);
    with return_state=True the result is (y, zf), zf the float64 state after the last sample, written by the same launch.
    reverse=True filters from the last sample to the first with zero state -- the adjoint of the forward filter, bit for
    bit flip -> forward -> flip -- and takes neither zi nor return_state (ValueError)."""
    import math
    co = sos_coefficients(sos)
    if reverse and (zi is not None or return_state):
        raise ValueError("reverse filtering starts from zero state and hands none back: no zi, no return_state")
    if x.ndim < 1:
        raise ValueError("sos_filter takes (..., L), got a scalar")
    require_device(x, zi)
    x = _f32c(x)
    lead, L = tuple(x.shape[:-1]), x.shape[-1]
    rows = math.prod(lead)
    state_shape = lead + (co.n, 2)
    if zi is not None:
        if zi.dtype != torch.float64:
            raise AcidsHipError("zi is %s: the filter state is float64 (it is no audio: nothing narrows it)"
                                % str(zi.dtype).replace("torch.", ""))
        if tuple(zi.shape) != state_shape:
            raise ValueError("zi is %s, x %s with %d sections needs %s" % (tuple(zi.shape), tuple(x.shape), co.n, state_shape))
        zi = zi if zi.is_contiguous() else zi.contiguous()
    y = torch.empty_like(x)
    zf = torch.empty(state_shape, dtype=torch.float64, device=x.device) if return_state else None
    check(lib().at_sos_filter(ptr(x), rows, L, co.ptr, co.n, int(bool(reverse)), ptr(zi), ptr(zf), ptr(y),
                              stream_ptr()), "at_sos_filter")
    return (y, zf) if return_state else y


SOS_MIN_HOP = 16


def sos_hop_power_plan(rows, L, n_sections, hop):
    """(tile, per_lane, dispatch) of at_sos_hop_power at a shape: sos_filter_plan's answer -- it is the same walk -- after
    the checks on hop (per_lane is also the smallest hop).  Reads no device state."""
    tile, per_lane, dispatch = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
    check(lib().at_sos_hop_power_plan(int(rows), int(L), int(n_sections), int(hop), ctypes.byref(tile), ctypes.byref(per_lane),
                                      ctypes.byref(dispatch)), "at_sos_hop_power_plan")
    return tile.value, per_lane.value, dispatch.value


def _hop_rows(x, hop, what):
    if x.ndim < 1:
        raise ValueError("%s takes (..., L), got a scalar" % what)
    hop = int(hop)
    if hop < 1:
        raise ValueError("hop must be >= 1, got %d" % hop)
    return hop


def sos_hop_power(x, sos, hop):
    """The energy envelope of an SOS-filtered signal: x (..., L) float32 -> (..., L // hop) FLOAT64, entry h the sum over
    samples [h hop, (h + 1) hop) of y^2 with y = sos_filter(x, sos) taken in double BEFORE it is rounded to float; y itself
    is never written (include/acids_hip.h, at_sos_hop_power).  The samples past (L // hop) hop belong to no hop.  hop >=
    SOS_MIN_HOP (smaller: the library's AT_EUNSUPPORTED).  The section [1, 0, 0, 1, 0, 0] gives the envelope of x itself
    (divide by hop and take the root for an RMS envelope).  A row's bits do not depend on the batch."""
    co = sos_coefficients(sos)
    hop = _hop_rows(x, hop, "sos_hop_power")
    require_device(x)
    x = _f32c(x)
    lead, L = tuple(x.shape[:-1]), x.shape[-1]
    power = torch.empty(lead + (L // hop,), dtype=torch.float64, device=x.device)
    check(lib().at_sos_hop_power(ptr(x), math.prod(lead), L, co.ptr, co.n, hop, ptr(power), stream_ptr()), "at_sos_hop_power")
    return power


def sos_filter_hop_scaled(x, sos, hop, w):
    """x (..., L) float32, w (..., L // hop) FLOAT64 -> u (..., L) float32, u[n] = (float)(w[n // hop] y[n]) with y as in
    sos_hop_power and +0 past the last whole hop: the gradient of a function of the hop powers with respect to y (its
    gradient with respect to x is sos_filter(u, sos, reverse=True))."""
    co = sos_coefficients(sos)
    hop = _hop_rows(x, hop, "sos_filter_hop_scaled")
    require_device(x, w)
    x = _f32c(x)
    lead, L = tuple(x.shape[:-1]), x.shape[-1]
    if w.dtype != torch.float64:
        raise AcidsHipError("w is %s: the hop weights are float64" % str(w.dtype).replace("torch.", ""))
    if tuple(w.shape) != lead + (L // hop,):
        raise ValueError("w is %s, x %s with hop %d needs %s" % (tuple(w.shape), tuple(x.shape), hop, lead + (L // hop,)))
    w = w if w.is_contiguous() else w.contiguous()
    u = torch.empty_like(x)
    check(lib().at_sos_filter_hop_scaled(ptr(x), math.prod(lead), L, co.ptr, co.n, hop, ptr(w), ptr(u), stream_ptr()),
          "at_sos_filter_hop_scaled")
    return u


# ----------------------------------------------------------------------------------------------
# gated loudness, ITU-R BS.1770 / EBU R128 (loudness.hip on top of at_sos_hop_power)
# ----------------------------------------------------------------------------------------------
LOUDNESS_CHANNEL_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)               # L R C Ls Rs
LOUDNESS_ABS_THRESHOLD = 10.0 ** ((-70.0 + 0.691) / 10.0)            # -70 LUFS as a block power
LOUDNESS_REL_RATIO = 0.1                                             # -10 LU
LOUDNESS_BLOCK_HOPS = 4                                              # 400 ms blocks of 100 ms hops: 75 % overlap
LOUDNESS_SHORT_TERM_HOPS = 30                                        # 3 s


class _Loud:
    """What loudness_plan has checked for one call: the K-weighting sections, the hop, the block, the channel weights on
    the host, and the shape."""

    def __init__(self, co, hop, hb, weights, lead, C, L, mono):
        self.co, self.hop, self.hb, self.weights = co, hop, hb, weights
        self.wptr = ctypes.c_void_p(weights.ctypes.data)
        self.lead, self.C, self.L, self.mono = lead, C, L, mono
        self.clips, self.nh = math.prod(lead), L // hop
        self.nb = self.nh - hb + 1


_K_WEIGHTING = {}


def _k_weighting(sr):
    from .utils.filter_design import k_weighting
    key = float(sr)
    if key not in _K_WEIGHTING:
        _K_WEIGHTING[key] = sos_coefficients(k_weighting(key))       # ValueError below 3364 Hz
    return _K_WEIGHTING[key]


def loudness_plan(shape, sr, hops_per_block=LOUDNESS_BLOCK_HOPS, channel_weights=None):
    """The checks of loudness and loudness_blocks on a shape (..., C, L) -- (L,) is one mono clip -- without a device.
    ValueError: sr at which filter_design.k_weighting raises; hops_per_block < 1; C > 5 without explicit channel_weights
    (BS.1770 names five weights; it is also what catches a (batch, L) tensor read as `batch` channels); weights that are
    not C finite numbers; L < hops_per_block round(sr / 10), no block."""
    import numpy as np
    co = _k_weighting(sr)
    hop, hb = int(round(float(sr) / 10.0)), int(hops_per_block)
    if hb < 1:
        raise ValueError("hops_per_block must be >= 1, got %d" % hb)
    shape = tuple(shape)
    if len(shape) < 1:
        raise ValueError("loudness takes (..., C, L), got a scalar")
    mono = len(shape) == 1
    lead, C, L = (shape[:-2], shape[-2], shape[-1]) if not mono else ((), 1, shape[-1])
    if channel_weights is None:
        if C > len(LOUDNESS_CHANNEL_WEIGHTS):
            raise ValueError("%d channels and no channel_weights: BS.1770 names weights for up to %d channels (input is "
                             "(..., C, L): a (batch, L) tensor needs a channel axis, x[:, None])"
                             % (C, len(LOUDNESS_CHANNEL_WEIGHTS)))
        weights = np.array(LOUDNESS_CHANNEL_WEIGHTS[:C], dtype=np.float64)
    else:
        weights = np.array(channel_weights, dtype=np.float64, ndmin=1)
        if weights.ndim != 1 or weights.shape[0] != C:
            raise ValueError("channel_weights has shape %s, the input has %d channels" % (tuple(weights.shape), C))
        if not np.isfinite(weights).all():
            raise ValueError("channel_weights has non-finite entries")
    if C < 1:
        raise ValueError("loudness needs at least one channel, got shape %s" % (shape,))
    if L < hb * hop:
        raise ValueError("%d samples hold no block of %d hops of %d samples (sr %g)" % (L, hb, hop, sr))
    return _Loud(co, hop, hb, np.ascontiguousarray(weights), tuple(lead), C, L, mono)


def _loudness_power(x, plan):
    _no_fp64(x)
    require_device(x)
    x = _f32c(x)
    power = torch.empty(plan.lead + (plan.C, plan.nh), dtype=torch.float64, device=x.device)
    check(lib().at_sos_hop_power(ptr(x), plan.clips * plan.C, plan.L, plan.co.ptr, plan.co.n, plan.hop, ptr(power),
                                 stream_ptr()), "at_sos_hop_power")
    return x, power


def loudness(x, sr, channel_weights=None, return_state=False):
    """Integrated loudness of ITU-R BS.1770-4 / EBU R128 in LUFS: x (..., C, L) float32 -> (...,) float32; (L,) is one mono
    clip.  K-weighting (utils.filter_design.k_weighting(sr), the standard's table at 48 kHz) and the mean squares of the
    100 ms hops in one launch (at_sos_hop_power: the filtered signal is never written), then 400 ms blocks with 75 %
    overlap, the -70 LUFS absolute and the -10 LU relative gate in a second (at_loudness_gate).  -inf when no block passes
    the absolute gate; NaN when the clip holds one.  channel_weights: C numbers, None for (1, 1, 1, 1.41, 1.41)[:C].
    return_state=True: (lufs, power (..., C, L // hop) float64, stats (..., 3) float64 = Pabs, P, N2), what the backward
    reads.  ValueError: see loudness_plan."""
    plan = loudness_plan(x.shape, sr, LOUDNESS_BLOCK_HOPS, channel_weights)
    x, power = _loudness_power(x, plan)
    lufs = torch.empty(plan.lead, dtype=torch.float32, device=x.device)
    stats = torch.empty(plan.lead + (3,), dtype=torch.float64, device=x.device)
    check(lib().at_loudness_gate(ptr(power), plan.clips, plan.C, plan.nh, plan.hop, plan.hb, plan.wptr,
                                 LOUDNESS_ABS_THRESHOLD, LOUDNESS_REL_RATIO, ptr(lufs), ptr(stats), None, stream_ptr()),
          "at_loudness_gate")
    return (lufs, power, stats) if return_state else lufs


def loudness_blocks(x, sr, hops_per_block=LOUDNESS_BLOCK_HOPS, channel_weights=None, return_state=False):
    """Ungated block loudness in LUFS: x (..., C, L) float32 -> (..., nb) float32 with nb = L // hop - hops_per_block + 1,
    one value per 100 ms step.  hops_per_block = 4 is momentary loudness (400 ms), 30 short-term (3 s).  -inf for a silent
    block.  return_state=True: (blocks, power).  ValueError: see loudness_plan."""
    plan = loudness_plan(x.shape, sr, hops_per_block, channel_weights)
    x, power = _loudness_power(x, plan)
    blocks = torch.empty(plan.lead + (plan.nb,), dtype=torch.float32, device=x.device)
    check(lib().at_loudness_gate(ptr(power), plan.clips, plan.C, plan.nh, plan.hop, plan.hb, plan.wptr, 0.0, 0.0, None, None,
                                 ptr(blocks), stream_ptr()), "at_loudness_gate")
    return (blocks, power) if return_state else blocks


def _loudness_finish(x, plan, w):
    """w (..., C, nh) -> gx: the weighted K-weighted signal, then the reverse K-weighting filter (its adjoint)."""
    u = torch.empty_like(x)
    check(lib().at_sos_filter_hop_scaled(ptr(x), plan.clips * plan.C, plan.L, plan.co.ptr, plan.co.n, plan.hop, ptr(w), ptr(u),
                                         stream_ptr()), "at_sos_filter_hop_scaled")
    return sos_filter(u, plan.co, reverse=True)


def loudness_backward(x, power, stats, g, sr, channel_weights=None):
    """The gradient of loudness with respect to x: g (...,) = dL/dlufs -> (..., C, L) float32, from what return_state
    handed out.  Three launches: the hop weights (the gates recomputed from power and stats, constants of the graph),
    the K-weighted signal times them, the reverse filter.  A clip that read -inf gets exactly zero."""
    plan = loudness_plan(x.shape, sr, LOUDNESS_BLOCK_HOPS, channel_weights)
    require_device(x, power, stats, g)
    x, g = _f32c(x), _f32c(g)
    if tuple(g.shape) != plan.lead or tuple(power.shape) != plan.lead + (plan.C, plan.nh) or \
            tuple(stats.shape) != plan.lead + (3,) or power.dtype != torch.float64 or stats.dtype != torch.float64:
        raise ValueError("loudness_backward: g, power and stats are not those of loudness(x, return_state=True)")
    w = torch.empty_like(power)
    check(lib().at_loudness_gate_backward(ptr(power.contiguous()), ptr(stats.contiguous()), ptr(g), plan.clips, plan.C,
                                          plan.nh, plan.hop, plan.hb, plan.wptr, LOUDNESS_ABS_THRESHOLD, LOUDNESS_REL_RATIO,
                                          ptr(w), stream_ptr()), "at_loudness_gate_backward")
    return _loudness_finish(x, plan, w)


def loudness_blocks_backward(x, power, g, sr, hops_per_block=LOUDNESS_BLOCK_HOPS, channel_weights=None):
    """The gradient of loudness_blocks with respect to x: g (..., nb) -> (..., C, L) float32.  Silent blocks (-inf)
    contribute nothing."""
    plan = loudness_plan(x.shape, sr, hops_per_block, channel_weights)
    require_device(x, power, g)
    x, g = _f32c(x), _f32c(g)
    if tuple(g.shape) != plan.lead + (plan.nb,) or tuple(power.shape) != plan.lead + (plan.C, plan.nh) or \
            power.dtype != torch.float64:
        raise ValueError("loudness_blocks_backward: g and power are not those of loudness_blocks(x, return_state=True)")
    w = torch.empty_like(power)
    check(lib().at_loudness_blocks_backward(ptr(power.contiguous()), ptr(g), plan.clips, plan.C, plan.nh, plan.hop, plan.hb,
                                            plan.wptr, ptr(w), stream_ptr()), "at_loudness_blocks_backward")
    return _loudness_finish(x, plan, w)


LOUDNESS_RANGE_REL_RATIO = 0.01                                      # -20 LU (EBU Tech 3342)


def _state64(t, shape, what):
    if t.dtype != torch.float64:
        raise AcidsHipError("%s is %s: the carried state is float64 (it is no audio: nothing narrows it)"
                            % (what, str(t.dtype).replace("torch.", "")))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s is %s, the chunk needs %s" % (what, tuple(t.shape), tuple(shape)))
    if not t.is_contiguous():
        raise ValueError("%s is updated in place: it must be contiguous" % what)


def sos_hop_power_stream(x, sos, hop, filled, zi, open_sum, power, first):
    """The next chunk of a stream through sos_hop_power (include/acids_hip.h, at_sos_hop_power_stream): x (..., n) float32,
    n >= 1; `filled` (0 <= filled < hop) samples of the open hop came with earlier chunks.  UPDATES IN PLACE, all FLOAT64
    and contiguous on x's device: zi (..., n_sections, 2), the filter state; open_sum (...,), the partial sum of the open
    hop; power (..., cap), of which entries [first, first + done) receive the hops that complete inside this chunk and no
    other entry is touched.  Returns done = (filled + n) // hop, computed on the host.  One launch, no allocation.  The
    hop powers of a chunked stream agree with sos_hop_power of the whole signal within rounding, not to the bit; the same
    chunking gives the same bits in any batch.  ValueError: shapes that do not match, filled outside [0, hop), first + done
    past cap, an empty chunk."""
    co = sos_coefficients(sos)
    hop = _hop_rows(x, hop, "sos_hop_power_stream")
    filled, first = int(filled), int(first)
    lead, n = tuple(x.shape[:-1]), x.shape[-1]
    if n < 1:
        raise ValueError("sos_hop_power_stream takes a chunk of at least one sample")
    if not 0 <= filled < hop:
        raise ValueError("filled must lie in [0, hop = %d), got %d" % (hop, filled))
    if power.ndim != len(lead) + 1:
        raise ValueError("power is %s, the chunk %s needs %s" % (tuple(power.shape), tuple(x.shape), lead + ("cap",)))
    cap = power.shape[-1]
    _state64(zi, lead + (co.n, 2), "zi")
    _state64(open_sum, lead, "open_sum")
    _state64(power, lead + (cap,), "power")
    done = (filled + n) // hop
    if first < 0 or first + done > cap:
        raise ValueError("hops [%d, %d) do not fit power's %d columns" % (first, first + done, cap))
    require_device(x, zi, open_sum, power)
    x = _f32c(x)
    check(lib().at_sos_hop_power_stream(ptr(x), math.prod(lead), n, co.ptr, co.n, hop, filled, ptr(zi), ptr(zi), ptr(open_sum),
                                        ptr(open_sum), ptr(power), cap, first, stream_ptr()), "at_sos_hop_power_stream")
    return done


def loudness_stream_plan(sr, samples_seen, n, hops_per_block=LOUDNESS_BLOCK_HOPS):
    """(hop, filled, first, done, new_blocks) of a chunk of n samples that follows samples_seen samples of a stream at rate
    sr: the 100 ms hop, the samples the open hop already holds, the index of that hop, the hops that complete inside the
    chunk, and the blocks of hops_per_block hops that do.  Host arithmetic; reads no device.  ValueError: negative counts,
    hops_per_block < 1, a rate at which filter_design.k_weighting raises."""
    _k_weighting(sr)
    hop, hb, seen, n = int(round(float(sr) / 10.0)), int(hops_per_block), int(samples_seen), int(n)
    if seen < 0 or n < 0:
        raise ValueError("samples_seen and n must be >= 0, got %d and %d" % (seen, n))
    if hb < 1:
        raise ValueError("hops_per_block must be >= 1, got %d" % hb)
    filled, first = seen % hop, seen // hop
    done = (filled + n) // hop
    new_blocks = max(0, first + done - hb + 1) - max(0, first - hb + 1)
    return hop, filled, first, done, new_blocks


def loudness_gate_window(power, C, offset, nh, sr, hops_per_block=LOUDNESS_BLOCK_HOPS, channel_weights=None, gated=False):
    """at_loudness_gate_ld on the hops [offset, offset + nh) of a history power (..., C, cap) float64, contiguous, read
    where it lies: the block loudnesses (..., nh - hops_per_block + 1) float32, or with gated=True the gated loudness
    (...,) of that window (-inf when it holds no block)."""
    plan = loudness_plan((C, max(int(nh), int(hops_per_block)) * int(round(float(sr) / 10.0))), sr, hops_per_block, channel_weights)
    require_device(power)
    if power.dtype != torch.float64 or power.ndim < 2 or power.shape[-2] != C or not power.is_contiguous():
        raise ValueError("power must be a contiguous (..., C = %d, cap) float64 tensor, got %s %s" % (C, tuple(power.shape), power.dtype))
    lead, cap, offset, nh = tuple(power.shape[:-2]), power.shape[-1], int(offset), int(nh)
    if offset < 0 or nh < 0 or offset + nh > cap:
        raise ValueError("hops [%d, %d) are not inside the history's %d" % (offset, offset + nh, cap))
    clips, nb = math.prod(lead), nh - plan.hb + 1
    base = ctypes.c_void_p(power.data_ptr() + 8 * offset)
    if gated:
        if nb < 1:
            return torch.full(lead, float("-inf"), dtype=torch.float32, device=power.device)
        lufs = torch.empty(lead, dtype=torch.float32, device=power.device)
        stats = torch.empty(lead + (3,), dtype=torch.float64, device=power.device)
        check(lib().at_loudness_gate_ld(base, clips, C, nh, cap, plan.hop, plan.hb, plan.wptr, LOUDNESS_ABS_THRESHOLD,
                                        LOUDNESS_REL_RATIO, ptr(lufs), ptr(stats), None, stream_ptr()), "at_loudness_gate_ld")
        return lufs
    blocks = torch.empty(lead + (max(nb, 0),), dtype=torch.float32, device=power.device)
    if nb >= 1:
        check(lib().at_loudness_gate_ld(base, clips, C, nh, cap, plan.hop, plan.hb, plan.wptr, 0.0, 0.0, None, None,
                                        ptr(blocks), stream_ptr()), "at_loudness_gate_ld")
    return blocks


def loudness_range_from_power(power, nh, sr, channel_weights=None, ld=None, return_state=False):
    """Loudness range (EBU Tech 3342) in LU from hop powers: power (..., C, ld) float64, contiguous, of which the first nh
    hops of every row are read (ld: the row length, None for power.shape[-1]) -> (...,) float32.  3 s blocks one hop
    apart, the -70 LUFS absolute gate, a relative gate 20 LU below the mean of what passed, then
    10 log10(q[rnd(0.95 (n - 1))] / q[rnd(0.10 (n - 1))]) over the n gated block powers in ascending order, the two picked by
    an exact radix select (at_loudness_range).  0 when nothing passes (also: no 3 s block); NaN for a clip that holds one.
    return_state=True: (lra, stats (..., 4) float64 = P_low, P_high, n, Pabs)."""
    if power.dtype != torch.float64 or power.ndim < 2 or not power.is_contiguous():
        raise ValueError("power must be a contiguous (..., C, ld) float64 tensor, got %s %s" % (tuple(power.shape), power.dtype))
    lead, C, nh = tuple(power.shape[:-2]), power.shape[-2], int(nh)
    ld = power.shape[-1] if ld is None else int(ld)
    if ld != power.shape[-1] or not 0 <= nh <= ld:
        raise ValueError("nh = %d hops of rows of ld = %d do not match power %s" % (nh, ld, tuple(power.shape)))
    hb = LOUDNESS_SHORT_TERM_HOPS
    plan = loudness_plan((C, hb * int(round(float(sr) / 10.0))), sr, hb, channel_weights)
    require_device(power)
    lra = torch.empty(lead, dtype=torch.float32, device=power.device)
    stats = torch.empty(lead + (4,), dtype=torch.float64, device=power.device)
    work = torch.empty(lead + (max(nh - hb + 1, 0),), dtype=torch.float64, device=power.device)
    check(lib().at_loudness_range(ptr(power), math.prod(lead), C, nh, ld, plan.hop, hb, plan.wptr, LOUDNESS_ABS_THRESHOLD,
                                  LOUDNESS_RANGE_REL_RATIO, ptr(lra), ptr(stats), ptr(work), stream_ptr()), "at_loudness_range")
    return (lra, stats) if return_state else lra


def loudness_range(x, sr, channel_weights=None, return_state=False):
    """Loudness range (LRA, EBU Tech 3342) of x (..., C, L) float32 -> (...,) float32 in LU; (L,) is one mono clip.  Two
    launches: the K-weighted hop powers (at_sos_hop_power), then loudness_range_from_power.  ValueError below one 3 s
    block (see loudness_plan).  return_state=True: (lra, power (..., C, L // hop), stats (..., 4))."""
    plan = loudness_plan(x.shape, sr, LOUDNESS_SHORT_TERM_HOPS, channel_weights)
    x, power = _loudness_power(x, plan)
    lra, stats = loudness_range_from_power(power, plan.nh, sr, channel_weights, return_state=True)
    return (lra, power, stats) if return_state else lra


# ----------------------------------------------------------------------------------------------
# true peak, ITU-R BS.1770-4 Annex 2 (true_peak.hip)
# ----------------------------------------------------------------------------------------------
TRUE_PEAK_MAX_PHASES = 8
TRUE_PEAK_MAX_TAPS = 64


def true_peak_plan(rows, L, P, K):
    """(tile, per_lane, launches, dispatch) of at_true_peak at a shape: the samples of a tile, the consecutive samples of a
    lane, the launches of a call (0 for empty work, 1 where a row is one tile, else 2) and which copy runs (0: the compiled
    (4, 12) one, 1: the generic one).  Reads no device state."""
    tile, per_lane, launches, dispatch = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib().at_true_peak_plan(int(rows), int(L), int(P), int(K), ctypes.byref(tile), ctypes.byref(per_lane),
                                  ctypes.byref(launches), ctypes.byref(dispatch)), "at_true_peak_plan")
    return tile.value, per_lane.value, launches.value, dispatch.value


def _true_peak_taps(taps, x):
    if not isinstance(taps, torch.Tensor) or taps.ndim != 2:
        raise ValueError("taps must be a (phases, taps per phase) tensor")
    P, K = int(taps.shape[0]), int(taps.shape[1])
    if not (1 <= P <= TRUE_PEAK_MAX_PHASES and 1 <= K <= TRUE_PEAK_MAX_TAPS):
        raise ValueError("taps is %s: 1 <= phases <= %d and 1 <= taps per phase <= %d"
                         % (tuple(taps.shape), TRUE_PEAK_MAX_PHASES, TRUE_PEAK_MAX_TAPS))
    require_device(x, taps)
    if taps.dtype != torch.float32 or not taps.is_contiguous():
        taps = taps.detach().float().contiguous()
    return taps, P, K


def _true_peak_workspace(rows, L, P, K, device):
    nbytes = lib().at_true_peak_workspace_bytes(rows, L, P, K)
    return (torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None), nbytes


def true_peak(x, taps, return_state=False):
    """The true peak of every row: x (..., L) float32, taps (P, K) float32 -> (...,) float32, LINEAR, the maximum of |y| over
    the P L values y[P n + p] = sum_k taps[p][k] x[n - k] (include/acids_hip.h, at_true_peak); one launch where a row is one
    tile of 2048 samples, else two.  A row's bits depend neither on the batch nor on the tiling.  Zeros (and L == 0) give +0, a
    NaN in a row makes that row NaN and no other.  return_state=True: (peak, index (...,) int64 the smallest oversampled
    index that attains it, sign (...,) float32 the sign of y there, 0 where the peak is 0 or NaN)."""
    if x.ndim < 1:
        raise ValueError("true_peak takes (..., L), got a scalar")
    taps, P, K = _true_peak_taps(taps, x)
    x = _f32c(x)
    lead, L = tuple(x.shape[:-1]), x.shape[-1]
    rows = math.prod(lead)
    new = torch.zeros if rows * L == 0 else torch.empty
    peak = new(lead, dtype=torch.float32, device=x.device)
    index = new(lead, dtype=torch.int64, device=x.device) if return_state else None
    sign = new(lead, dtype=torch.float32, device=x.device) if return_state else None
    ws, nbytes = _true_peak_workspace(rows, L, P, K, x.device)
    check(lib().at_true_peak(ptr(x), rows, L, ptr(taps), P, K, None, None, ptr(peak), ptr(index), ptr(sign), None, None, 0,
                             ptr(ws), nbytes, stream_ptr()), "at_true_peak")
    return (peak, index, sign) if return_state else peak


def true_peak_stream(x, taps, state, state_next, max_peak, max_index, offset):
    """The next chunk of a stream through true_peak: x (..., n) float32, n >= 1; state (..., K - 1) float32 the samples before
    it, oldest first; state_next (same shape, another tensor) receives the last K - 1 samples of [state | x]; max_peak (...,)
    float32 and max_index (...,) int64, the running maximum and its index in the stream, are updated in place, the index of
    this chunk's first oversampled value being `offset`.  Returns the chunk's own peak, (...,) float32, linear.  All of them
    contiguous; with K == 1 there is no state and both may be None.  No torch.cat, no synchronisation, and no allocation but
    the result (and the partials of a chunk longer than a tile).  The peak of a chunked stream has the bits of the one-call
    true_peak of the whole signal."""
    if x.ndim < 1:
        raise ValueError("true_peak_stream takes (..., n), got a scalar")
    taps, P, K = _true_peak_taps(taps, x)
    require_device(x, state, state_next, max_peak, max_index)
    x = _f32c(x)
    lead, n = tuple(x.shape[:-1]), x.shape[-1]
    if n < 1:
        raise ValueError("true_peak_stream takes a chunk of at least one sample")
    for t, shape, dtype, what in ((state, lead + (K - 1,), torch.float32, "state"), (state_next, lead + (K - 1,), torch.float32,
                                  "state_next"), (max_peak, lead, torch.float32, "max_peak"), (max_index, lead, torch.int64,
                                                                                                "max_index")):
        if t is None and K == 1 and what.startswith("state"):
            continue
        if t is None or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s" % (what, str(dtype).replace("torch.", ""), shape))
    if K > 1 and state.data_ptr() == state_next.data_ptr():
        raise ValueError("state_next must not be state: a long chunk's tiles read the state while its last tile writes")
    rows = math.prod(lead)
    peak = torch.empty(lead, dtype=torch.float32, device=x.device)
    ws, nbytes = _true_peak_workspace(rows, n, P, K, x.device)
    check(lib().at_true_peak(ptr(x), rows, n, ptr(taps), P, K, ptr(state) if K > 1 else None,
                             ptr(state_next) if K > 1 else None, ptr(peak), None, None, ptr(max_peak), ptr(max_index),
                             int(offset), ptr(ws), nbytes, stream_ptr()), "at_true_peak")
    return peak


def true_peak_backward(g, sign, index, taps, L):
    """The subgradient of true_peak with respect to x: g (...,) = dL/dpeak (linear), sign and index as return_state gave them
    -> (..., L) float32, g sign taps[p*][n* - n] on the at most K samples under the attained maximum and +0 elsewhere; a row
    whose sign is 0 (peak 0 or NaN) gets +0 whatever g holds.  One launch, every element written."""
    taps, P, K = _true_peak_taps(taps, g)
    require_device(g, sign, index)
    lead = tuple(g.shape)
    if tuple(sign.shape) != lead or tuple(index.shape) != lead or index.dtype != torch.int64:
        raise ValueError("true_peak_backward: g, sign and index are not those of true_peak(x, taps, return_state=True)")
    g, sign, index = _f32c(g), _f32c(sign), index.contiguous()
    gx = torch.empty(lead + (int(L),), dtype=torch.float32, device=g.device)
    check(lib().at_true_peak_backward(ptr(g), ptr(sign), ptr(index), ptr(taps), P, K, math.prod(lead), int(L), ptr(gx),
                                      stream_ptr()), "at_true_peak_backward")
    return gx


# ----------------------------------------------------------------------------------------------
# long-filter convolution (fft_convolve.hip): uniformly partitioned overlap-save
# ----------------------------------------------------------------------------------------------
FFT_CONVOLVE_BLOCKS = (128, 256, 512, 1024, 2048)
FFT_CONVOLVE_MODES = ("full", "same", "valid")


def fft_convolve_plan(L, K, block=None):
    """(B, T, P, frame_tile, chunk_rows) of a convolution of L samples with K taps: the block (None: the smallest of
    512, 1024, 2048 with ceil(K / B) <= 4, else 2048; 128 and 256 only by request), the frames ceil((L + K - 1) / B), the partitions ceil(K / B),
    the output frames a lane of at_spectral_fir holds, and the rows of one chunk (one spectrum within 2^26 complex64
    elements, at least one row).  Reads no device state.  ValueError: L < 1, K < 1, a block outside the ladder."""
    if int(L) < 1 or int(K) < 1:
        raise ValueError("fft_convolve needs at least one sample and one tap, got L = %d, K = %d" % (L, K))
    if block is not None and (isinstance(block, bool) or int(block) != block or int(block) not in FFT_CONVOLVE_BLOCKS):
        raise ValueError("block must be one of %s or None, got %r" % (FFT_CONVOLVE_BLOCKS, block))
    B, T, P, tile, chunk = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    check(lib().at_fft_convolve_plan(int(L), int(K), 0 if block is None else int(block), ctypes.byref(B), ctypes.byref(T),
                                     ctypes.byref(P), ctypes.byref(tile), ctypes.byref(chunk)), "at_fft_convolve_plan")
    return B.value, T.value, P.value, tile.value, chunk.value


def fft_convolve_cut(L, K, mode):
    """(offset, length) of torchaudio's `mode` inside the full result of L + K - 1 samples."""
    if mode == "full":
        return 0, L + K - 1
    if mode == "same":
        return (K - 1) // 2, L
    if mode == "valid":
        return min(L, K) - 1, max(L, K) - min(L, K) + 1
    raise ValueError("mode must be one of %s, got %r" % (FFT_CONVOLVE_MODES, mode))


def spectral_fir(X, H, anticausal=False, conj=False, T=None):
    """Y[r, t, f] = sum_p Hc[p, f] X[r, s, f], s = t - p or (anticausal) t + p inside [0, T), Hc = H or (conj) its conjugate
    (include/acids_hip.h, at_spectral_fir).  X (rows, >= T, F) complex64 whose rows may be a slice along the frame axis (T
    defaults to all its frames), H (P, F) shared or (rows, P, F) -> (rows, T, F) complex64."""
    require_device(X, H)
    X, H = _c64(X), _c64_grad(H)
    if X.dim() != 3 or H.dim() not in (2, 3) or H.shape[-1] != X.shape[-1] or (H.dim() == 3 and H.shape[0] != X.shape[0]):
        raise ValueError("spectral_fir takes X (rows, T, F) and H (P, F) or (rows, P, F), got %s and %s"
                         % (tuple(X.shape), tuple(H.shape)))
    rows, F = X.shape[0], X.shape[2]
    T = X.shape[1] if T is None else int(T)
    if X.stride(2) != 1 or X.stride(1) != F or T > X.shape[1] or (rows > 1 and X.stride(0) < T * F):
        X = X[:, :T].contiguous()
    stride = X.stride(0) if rows > 1 else max(T * F, 1)
    P = H.shape[-2]
    Y = torch.empty((rows, T, F), dtype=torch.complex64, device=X.device)
    check(lib().at_spectral_fir(ptr(X), stride, ptr(H), P * F if H.dim() == 3 else 0, rows, T, P, F, int(bool(anticausal)),
                                int(bool(conj)), ptr(Y), stream_ptr()), "at_spectral_fir")
    return Y


def spectral_fir_corr(X, gY, P, shared):
    """gH[rh, p, f] = sum_r sum_{t >= p} conj(X[r, t - p, f]) gY[r, t, f] (at_spectral_fir_corr): X (rows, >= T, F) as in
    spectral_fir, gY (rows, T, F) -> (P, F) with the rows added in ascending order (shared) or (rows, P, F)."""
    require_device(X, gY)
    X, gY = _c64(X), _c64_grad(gY)
    if X.dim() != 3 or gY.dim() != 3 or X.shape[0] != gY.shape[0] or X.shape[2] != gY.shape[2] or X.shape[1] < gY.shape[1]:
        raise ValueError("spectral_fir_corr takes X (rows, >= T, F) and gY (rows, T, F), got %s and %s"
                         % (tuple(X.shape), tuple(gY.shape)))
    rows, T, F = gY.shape
    if X.stride(2) != 1 or X.stride(1) != F or (rows > 1 and X.stride(0) < T * F):
        X = X[:, :T].contiguous()
    stride = X.stride(0) if rows > 1 else max(T * F, 1)
    P, shared = int(P), bool(shared)
    gH = torch.empty((P, F) if shared else (rows, P, F), dtype=torch.complex64, device=X.device)
    wsb = lib().at_spectral_fir_corr_workspace_bytes(rows, T, P, F, int(shared))
    ws = _workspace(max(wsb, 8), X.device)
    check(lib().at_spectral_fir_corr(ptr(X), stride, ptr(gY), rows, T, P, F, int(shared), ptr(gH), ptr(ws), wsb,
                                     stream_ptr()), "at_spectral_fir_corr")
    return gH


def _conv_ones(N, device):
    """The rectangular window of the convolution's transforms."""
    return torch.ones(N, dtype=torch.float32, device=device)


def _conv_streams(B, n):
    """Frames per stream of the convolution's transforms: at n_fft 256 / 512 the register FFTs share a transform among
    the frames of a stream, which would carry a frame's NaN to blocks the convolution does not reach -- one frame each."""
    return 1 if 2 * B <= 512 else max(int(n), 1)


def _conv_signal_spectrum(x, B, T):
    """x (rows, L) float32 contiguous -> X[r, t] = rfft(x[r, tB - B : tB + B], zero outside [0, L)), t < T, as a (rows, T, F)
    view (at n_fft 256 / 512 of a (rows, T + 1, F) tensor: every frame is a clip of its own there, see _conv_streams, and
    the frame that straddles two rows is never read)."""
    rows, L = x.shape
    N, F = 2 * B, B + 1
    ones = _conv_ones(N, x.device)
    if _conv_streams(B, T) == 1:
        buf = torch.zeros(rows * (T + 1) * B + B, dtype=torch.float32, device=x.device)
        buf[:rows * (T + 1) * B].view(rows, (T + 1) * B)[:, B:B + L] = x
        out = torch.empty((rows, T + 1, F), dtype=torch.complex64, device=x.device)
        check(lib().at_stft_forward(ptr(buf), rows * (T + 1), N, B, 1, N, B, 0, ptr(ones), ptr(out), ptr(None),
                                    stream_ptr()), "at_stft_forward")
        return out[:, :T]
    buf = torch.nn.functional.pad(x, (B, 0))
    return stft_forward(buf, ones, N, B, center=False, T=T, clip_stride=B + L, L=B + L, B=rows)


def _conv_filter_spectrum(h, B, P):
    """h (rows_h, K) float32 -> H[r, p] = rfft(h[r, pB : pB + B] then B zeros), (rows_h, P, F): each partition is a clip of B
    samples and one frame, which at_stft_forward pads with zeros."""
    rows, K = h.shape
    N, F = 2 * B, B + 1
    if P * B != K:
        h = torch.nn.functional.pad(h, (0, P * B - K))
    h = h.contiguous()
    out = torch.empty((rows, P, F), dtype=torch.complex64, device=h.device)
    check(lib().at_stft_forward(ptr(h), rows * P, B, B, 1, N, B, 0, ptr(_conv_ones(N, h.device)), ptr(out), ptr(None),
                                stream_ptr()), "at_stft_forward")
    return out


def _conv_blocks(Y, B):
    """Y (rows, T, F) -> (rows, T B): the last B samples of irfft(Y[r, t]), block after block."""
    rows, T, F = Y.shape
    N = 2 * B
    frames = torch.empty((rows, T, N), dtype=torch.float32, device=Y.device)
    check(lib().at_irfft_frames_streams(ptr(Y), ptr(None), ptr(None), rows * T, _conv_streams(B, T), N,
                                        ptr(_conv_ones(N, Y.device)), ptr(frames), stream_ptr()), "at_irfft_frames_streams")
    return frames[..., B:].reshape(rows, T * B)


def _conv_blocks_adjoint(g, B):
    """g (rows, T B) float32 -> gY (rows, T, F): the adjoint of _conv_blocks."""
    rows, T = g.shape[0], g.shape[1] // B
    N, F = 2 * B, B + 1
    gframes = torch.zeros((rows, T, N), dtype=torch.float32, device=g.device)
    gframes[..., B:] = g.view(rows, T, B)
    out = torch.empty((rows, T, F), dtype=torch.complex64, device=g.device)
    per_stream = _conv_streams(B, T)
    wsb = lib().at_irfft_frames_backward_workspace_bytes(rows * T, per_stream, N, 0)
    ws = _workspace(wsb, g.device)
    check(lib().at_irfft_frames_backward(ptr(gframes), ptr(None), rows * T, per_stream, N, ptr(_conv_ones(N, g.device)),
                                         ptr(out), ptr(ws), wsb, stream_ptr()), "at_irfft_frames_backward")
    return out


def _conv_rfft_adjoint(G, B):
    """G (rows, n, F) complex64 -> (rows, n, N) float32: the adjoint of the frames' rfft."""
    rows, n, F = G.shape
    N = 2 * B
    out = torch.empty((rows, n, N), dtype=torch.float32, device=G.device)
    wsb = lib().at_rfft_frames_backward_workspace_bytes(rows * n, N)
    ws = _workspace(wsb, G.device)
    check(lib().at_rfft_frames_backward(ptr(G), rows * n, _conv_streams(B, n), N, ptr(_conv_ones(N, G.device)), ptr(out),
                                        ptr(ws), wsb, stream_ptr()), "at_rfft_frames_backward")
    return out


def _conv_operands(x, h, mode):
    """Shapes of fft_convolve: -> (x2 (rows, L), h2 (K,) shared or (rows, K), lead, shared), checked before any device is
    touched."""
    if mode not in FFT_CONVOLVE_MODES:
        raise ValueError("mode must be one of %s, got %r" % (FFT_CONVOLVE_MODES, mode))
    if x.dim() < 1 or h.dim() < 1 or x.shape[-1] < 1 or h.shape[-1] < 1:
        raise ValueError("fft_convolve takes x (..., L >= 1) and h (..., K >= 1), got %s and %s" % (tuple(x.shape), tuple(h.shape)))
    shared = h.dim() == 1
    lead = tuple(x.shape[:-1])
    if not shared:
        try:
            lead = tuple(torch.broadcast_shapes(x.shape[:-1], h.shape[:-1]))
        except RuntimeError:
            raise ValueError("the leading shapes of x %s and h %s do not broadcast" % (tuple(x.shape), tuple(h.shape))) from None
    return lead, shared


@device_scoped
def fft_convolve(x, h, mode="full", block=None):
    """torchaudio.functional.fftconvolve(x, h, mode) by partitioned overlap-save (include/acids_hip.h, at_spectral_fir): x
    (..., L) float32, h (K,) -- one filter for every row -- or h with x's leading shape (any other broadcastable leading
    shape is expanded first).  "full": L + K - 1 samples; "same": L samples from (K - 1) // 2; "valid": max(L, K) - min(L, K)
    + 1 samples from min(L, K) - 1.  block: see fft_convolve_plan.  Rows go through in chunks of the plan's chunk_rows, so
    peak memory does not grow with the batch; a shared filter is transformed once per call."""
    lead, shared = _conv_operands(x, h, mode)
    L, K = x.shape[-1], h.shape[-1]
    B, T, P, _tile, chunk = fft_convolve_plan(L, K, block)
    off, n = fft_convolve_cut(L, K, mode)
    require_device(x, h)
    x2 = _f32c(x.expand(lead + (L,))).reshape(-1, L)
    h2 = _f32c(h if shared else h.expand(lead + (K,))).reshape(-1, K)
    rows = x2.shape[0]
    out = torch.empty((rows, n), dtype=torch.float32, device=x.device)
    H = _conv_filter_spectrum(h2, B, P) if shared else None
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        X = _conv_signal_spectrum(x2[r0:r1], B, T)
        Hc = H[0] if shared else _conv_filter_spectrum(h2[r0:r1], B, P)
        out[r0:r1] = _conv_blocks(spectral_fir(X, Hc), B)[:, off:off + n]
    return out.reshape(lead + (n,))


@device_scoped
def fft_convolve_backward(x, h, g, mode="full", block=None, need_x=True, need_h=True):
    """The gradients of fft_convolve(x, h, mode, block) given g, the gradient of its result: (gx like x or None, gh like h
    or None).  The spectra are rebuilt chunk by chunk; gx = framing^T rfft^T (conj H . gY, anticausal), gh = the first B
    samples of rfft^T of at_spectral_fir_corr(X, gY), a shared filter's chunks added in ascending order in double."""
    lead, shared = _conv_operands(x, h, mode)
    L, K = x.shape[-1], h.shape[-1]
    B, T, P, _tile, chunk = fft_convolve_plan(L, K, block)
    off, n = fft_convolve_cut(L, K, mode)
    require_device(x, h, g)
    if tuple(g.shape) != lead + (n,):
        raise ValueError("g is %s, the result of fft_convolve is %s" % (tuple(g.shape), lead + (n,)))
    x2 = _f32c(x.expand(lead + (L,))).reshape(-1, L)
    h2 = _f32c(h if shared else h.expand(lead + (K,))).reshape(-1, K)
    g2 = _f32c(g).reshape(-1, n)
    rows = x2.shape[0]
    gx = torch.empty((rows, L), dtype=torch.float32, device=x.device) if need_x else None
    gh = torch.empty((rows, K), dtype=torch.float32, device=x.device) if need_h and not shared else None
    gH_sum = None
    H = _conv_filter_spectrum(h2, B, P) if shared and need_x else None
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        gfull = torch.zeros((r1 - r0, T * B), dtype=torch.float32, device=x.device)
        gfull[:, off:off + n] = g2[r0:r1]
        gY = _conv_blocks_adjoint(gfull, B)
        if need_x:
            Hc = H[0] if shared else _conv_filter_spectrum(h2[r0:r1], B, P)
            gfr = _conv_rfft_adjoint(spectral_fir(gY, Hc, anticausal=True, conj=True), B)
            acc = torch.zeros((r1 - r0, T + 1, B), dtype=torch.float32, device=x.device)
            acc[:, :T] = gfr[..., :B]                    # the two frames that cover a sample
            acc[:, 1:] += gfr[..., B:]
            gx[r0:r1] = acc.view(r1 - r0, -1)[:, B:B + L]
        if need_h:
            gH = spectral_fir_corr(_conv_signal_spectrum(x2[r0:r1], B, T), gY, P, shared)
            if shared:
                gH_sum = gH.to(torch.complex128) if gH_sum is None else gH_sum + gH
            else:
                gh[r0:r1] = _conv_rfft_adjoint(gH, B)[..., :B].reshape(r1 - r0, P * B)[:, :K]
    if need_h and shared:
        gh = _conv_rfft_adjoint(gH_sum.to(torch.complex64).unsqueeze(0), B)[0, :, :B].reshape(P * B)[:K]
    if need_x:
        gx = gx.reshape(lead + (L,))
        if tuple(x.shape) != lead + (L,):
            gx = gx.sum_to_size(x.shape)
    if need_h and not shared:
        gh = gh.reshape(lead + (K,))
        if tuple(h.shape) != lead + (K,):
            gh = gh.sum_to_size(h.shape)
    return gx, gh


# ---- the streaming form: a ring of spectra per stream (at_spectral_fir_stream) ----------------------------------------------
def fft_convolve_stream_plan(K, block=None):
    """(B, P, R, max_frames) of a stream convolved with K taps: the block (None: fft_convolve_plan's rule; 128 and 256 by
    request), the partitions ceil(K / B), the slots of the ring of spectra P - 1 + max_frames, and the most frames one launch
    of at_spectral_fir_stream takes.  Reads no device state.  ValueError: K < 1, a block outside the ladder."""
    if int(K) < 1:
        raise ValueError("a streaming convolution needs at least one tap, got K = %d" % K)
    if block is not None and (isinstance(block, bool) or int(block) != block or int(block) not in FFT_CONVOLVE_BLOCKS):
        raise ValueError("block must be one of %s or None, got %r" % (FFT_CONVOLVE_BLOCKS, block))
    B, P, R, n = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().at_fft_convolve_stream_plan(int(K), 0 if block is None else int(block), ctypes.byref(B), ctypes.byref(P),
                                            ctypes.byref(R), ctypes.byref(n)), "at_fft_convolve_stream_plan")
    return B.value, P.value, R.value, n.value


def spectral_fir_stream(Xc, ring, head, H):
    """Y[r, t, f] = sum_p H[p, f] V[r, t - p, f] over a chunk of a stream (include/acids_hip.h, at_spectral_fir_stream): Xc
    (rows, Tc, F) complex64, the chunk's frames (its rows may be a slice along the frame axis of a longer tensor), ring
    (rows, R, F) complex64 contiguous, head the slot of the next frame, H (P, F) -> Y (rows, Tc, F).  MUTATES ring: slots
    head .. head + Tc - 1 (modulo R) receive Xc.  The caller owns head and advances it by Tc modulo R."""
    if (Xc.dim() != 3 or ring.dim() != 3 or H.dim() != 2 or ring.shape[0] != Xc.shape[0] or ring.shape[2] != Xc.shape[2]
            or H.shape[1] != Xc.shape[2]):
        raise ValueError("spectral_fir_stream takes Xc (rows, Tc, F), ring (rows, R, F) and H (P, F), got %s, %s and %s"
                         % (tuple(Xc.shape), tuple(ring.shape), tuple(H.shape)))
    if ring.dtype != torch.complex64 or not ring.is_contiguous():
        raise ValueError("ring must be a contiguous complex64 tensor (it is updated in place), got %s%s"
                         % (str(ring.dtype).replace("torch.", ""), "" if ring.is_contiguous() else ", not contiguous"))
    require_device(Xc, ring, H)
    Xc, H = _c64(Xc), _c64(H)
    rows, Tc, F = Xc.shape
    if Xc.stride(2) != 1 or Xc.stride(1) != F or (rows > 1 and Xc.stride(0) < Tc * F):
        Xc = Xc.contiguous()
    stride = Xc.stride(0) if rows > 1 else max(Tc * F, 1)
    H = H if H.is_contiguous() else H.contiguous()
    Y = torch.empty((rows, Tc, F), dtype=torch.complex64, device=Xc.device)
    check(lib().at_spectral_fir_stream(ptr(Xc), stride, ptr(ring), ptr(H), rows, Tc, H.shape[0], ring.shape[1], int(head), F,
                                       ptr(Y), stream_ptr()), "at_spectral_fir_stream")
    return Y


def _conv_stream_spectrum(tail, x, B):
    """tail (rows, B) and x (rows, Tc B) float32 -> (stage, Xc): stage (rows, (Tc + 1) B) = [tail | x] and Xc[r, t] =
    rfft(stage[r, tB : tB + 2 B]), t < Tc, as a (rows, Tc, F) view (at n_fft 256 / 512 of a (rows, Tc + 1, F) tensor: one
    frame per clip, see _conv_streams; the frame that straddles two rows is never read)."""
    rows, Tc = x.shape[0], x.shape[1] // B
    N, F = 2 * B, B + 1
    ones = _conv_ones(N, x.device)
    n = rows * (Tc + 1) * B
    # + B: the last row's straddling frame stays inside the buffer (those B samples are never set: nobody reads that frame)
    buf = torch.empty(n + B, dtype=torch.float32, device=x.device)
    stage = buf[:n].view(rows, (Tc + 1) * B)
    stage[:, :B] = tail
    stage[:, B:] = x
    if _conv_streams(B, Tc) == 1:
        out = torch.empty((rows, Tc + 1, F), dtype=torch.complex64, device=x.device)
        check(lib().at_stft_forward(ptr(buf), rows * (Tc + 1), N, B, 1, N, B, 0, ptr(ones), ptr(out), ptr(None),
                                    stream_ptr()), "at_stft_forward")
        return stage, out[:, :Tc]
    return stage, stft_forward(stage, ones, N, B, center=False, T=Tc, clip_stride=(Tc + 1) * B, L=(Tc + 1) * B, B=rows)


@device_scoped
def fft_convolve_stream(x, tail, ring, head, H, B, keep_spectra=False):
    """The next chunk of a stream through the partitioned convolution: x (rows, n B) float32, n >= 1, tail (rows, B) the B
    samples before it, ring (rows, R, F) and head as in spectral_fir_stream, H (P, F) the filter's spectrum -> (y (rows, n B),
    new_tail (rows, B), new_head[, X (rows, n, F)]).  The chunk is walked in sub-chunks of at most max_frames blocks: [tail |
    blocks] -> frames (at_stft_forward, a window of ones, center = 0), at_spectral_fir_stream, the last halves of the inverse
    transforms.  MUTATES ring; tail is left alone.  keep_spectra: also the chunk's own frames, for the filter's gradient."""
    rows, C = x.shape
    P, F = H.shape
    R = ring.shape[1]
    step = R - (P - 1)
    if C < B or C % B or step < 1 or F != B + 1 or tuple(tail.shape) != (rows, B) or tuple(ring.shape) != (rows, R, F):
        raise ValueError("fft_convolve_stream takes x (rows, n B), tail (rows, B), ring (rows, R >= P, B + 1), H (P, B + 1); got "
                         "%s, %s, %s, %s at B = %d" % (tuple(x.shape), tuple(tail.shape), tuple(ring.shape), tuple(H.shape), B))
    require_device(x, tail, ring, H)
    x, tail = _f32c(x), _f32c(tail)
    step = min(step, lib_max_stream_frames())
    n = C // B
    out = torch.empty((rows, C), dtype=torch.float32, device=x.device) if n > step else None
    spectra = []
    for b0 in range(0, n, step):
        b1 = min(n, b0 + step)
        stage, Xc = _conv_stream_spectrum(tail, x[:, b0 * B:b1 * B], B)
        y = _conv_blocks(spectral_fir_stream(Xc, ring, head, H), B)
        head = (head + (b1 - b0)) % R
        tail = stage[:, (b1 - b0) * B:]
        if keep_spectra:
            spectra.append(Xc)
        if out is None:
            out = y
        else:
            out[:, b0 * B:b1 * B] = y
    res = (out, tail.contiguous(), head)
    if keep_spectra:
        res += (spectra[0] if len(spectra) == 1 else torch.cat(spectra, dim=1),)
    return res


_MAX_STREAM_FRAMES = None


def lib_max_stream_frames():
    """max_frames of at_fft_convolve_stream_plan (a constant of the library)."""
    global _MAX_STREAM_FRAMES
    if _MAX_STREAM_FRAMES is None:
        _MAX_STREAM_FRAMES = fft_convolve_stream_plan(1)[3]
    return _MAX_STREAM_FRAMES


def ring_history(ring, head, n):
    """The n frames before slot head of ring (rows, R, F), oldest first, as a new tensor (the ring in ring order)."""
    R = ring.shape[1]
    start = (head - n) % R
    if start + n <= R:
        return ring[:, start:start + n].clone()
    return torch.cat([ring[:, start:], ring[:, :start + n - R]], dim=1)     # the range wraps: two pieces


@device_scoped
def fft_convolve_stream_backward(g, H, B, K, history=None, X=None, need_x=True, need_h=False):
    """The gradients of one chunk of fft_convolve_stream with the carried state a constant: g (rows, n B), H (P, F) ->
    (gx (rows, n B) or None, gh (K,) or None).  gx is the offline formula over the chunk's own n frames (the part that falls
    on the tail is dropped); gh is at_spectral_fir_corr of [history | X] (history (rows, P - 1, F): ring_history before the
    forward's launch; X: the chunk's frames) against gY preceded by P - 1 frames of zeros, then rfft^T and the cut to K taps."""
    require_device(g, H)
    g = _f32c(g)
    rows, C = g.shape
    n, P = C // B, H.shape[0]
    gY = _conv_blocks_adjoint(g, B)
    gx = gh = None
    if need_x:
        gfr = _conv_rfft_adjoint(spectral_fir(gY, H, anticausal=True, conj=True), B)
        acc = torch.zeros((rows, n + 1, B), dtype=torch.float32, device=g.device)
        acc[:, :n] = gfr[..., :B]                        # the two frames that cover a sample
        acc[:, 1:] += gfr[..., B:]
        gx = acc.view(rows, -1)[:, B:]
    if need_h:
        Xall = torch.cat([history, X], dim=1) if P > 1 else X
        gYall = torch.cat([torch.zeros_like(history), gY], dim=1) if P > 1 else gY
        gH = spectral_fir_corr(Xall, gYall, P, True)
        gh = _conv_rfft_adjoint(gH.unsqueeze(0), B)[0, :, :B].reshape(P * B)[:K]
    return gx, gh


def stft_polar_forward(x, window, band, contrast=None, mag_offset=None, mag_scale=None, eps=1.1920929e-07,
                       phase_offset=None, phase_scale=None):
    """Compose(STFT -> Polar) in one kernel: x (B, L) -> (B, T, 2, F): [.., 0, :] = normalise(contrast(|X| @ bank)),
    [.., 1, :] = normalise(angle X).  n_fft = 1024, hop = 256, bank with F = 513 banded filters."""
    require_device(x, window)
    x = _f32c(x)
    B, L = x.shape
    T = 1 + L // 256
    lane_filter, lane_start, weights = band.on(x.device)
    out = torch.empty((B, T, 2, 513), dtype=torch.float32, device=x.device)
    check(lib().at_stft_polar_forward(ptr(x), B, L, L, T, 1024, 256, ptr(window), ptr(lane_filter), ptr(lane_start),
                                      ptr(weights), band.N, band.n_passes, band.pass_len.ctypes.data,
                                      contrast_code(contrast), ptr(mag_offset), ptr(mag_scale), eps, ptr(phase_offset),
                                      ptr(phase_scale), ptr(out), stream_ptr()), "at_stft_polar_forward")
    return out


# every public op enters the device of its operands (see _lib.device_scoped)
for _name, _fn in list(globals().items()):
    if callable(_fn) and not _name.startswith("_") and getattr(_fn, "__module__", None) == __name__ \
            and _name not in ("contrast_code",):
        globals()[_name] = device_scoped(_fn)
del _name, _fn

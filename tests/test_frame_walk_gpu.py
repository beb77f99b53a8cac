"""Every frame walk and radix plan of the fallback STFT kernels (stft_generic.hip, stft_mixed.hip) and of the
overlap-add gather behind the unfused inverse, forced through AT_VARIANT_FRAME_WALKERS.

These kernels are the correctness path of every n_fft without a register-core kernel, of the register-core sizes when
a caller's window is only 4-byte aligned, of the inverse at any hop that is not fused, and of the adjoints.  A default
launch gives every frame its own workgroup up to 4096 frames, so at the suite's sizes no workgroup ever walked to a
second frame.  The cases of frame_walk_cases.py (their coverage is checked on the CPU by test_frame_walk_cases_cpu.py)
run every walker count against the default plan bit for bit -- which localises a bad frame -- and the default plan
against a float64 numpy restatement of torch.stft / torch.istft written here (neither the oracle nor torch).  Windows are
asymmetric, so a window read back to front or with its pairs swapped fails.  Every output lies between guard bands,
pre-filled with NaN: a missing store or a stray one fails."""
import numpy as np
import pytest
import torch

import frame_walk_cases as W
from acids_transforms_amd import ops
from acids_transforms_amd._lib import AT_EWORKSPACE, VARIANTS, AcidsHipError, check, lib, ptr, require_device, stream_ptr, variant
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5              # the project's parity bar (conftest.rel_max)
POLAR_TOL = 2e-5        # polar input: fast_sincosf, as test_sizes_that_are_not_powers_of_two grants
PHASE_TOL = 5e-7        # rad: what test_fast_atan2_accuracy_and_edge_cases holds fast_atan2f to
GUARD = 256             # floats of guard band on either side of an output (keeps the output 1 KB aligned)
SENTINEL = -7777.0
NAN = float("nan")
IDS = [c.name for c in W.CASES]


@pytest.fixture(autouse=True)
def _variants_back_to_default():
    yield
    assert all(lib().at_get_variant(w) == 0 for w in VARIANTS.values())


# ---- float64 reference ------------------------------------------------------------------------------------------------
def window64(n):
    """Periodic Hann x (1 + 0.3 k / n), rounded to fp32: positive past k = 0, asymmetric, NOLA at every hop <= n / 2."""
    k = np.arange(n, dtype=np.float64)
    return ((0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)) * (1.0 + 0.3 * k / n)).astype(np.float32)


def ref_forward(x, w, n, hop, center=True, T=None):
    """x: (B, L) -> (B, T, n // 2 + 1).  center: reflect pad by n // 2; otherwise T frames from sample 0, zeros past L."""
    x = np.asarray(x, dtype=np.float64)
    if center:
        xp = np.pad(x, ((0, 0), (n // 2, n // 2)), mode="reflect")
        T = 1 + (xp.shape[1] - n) // hop
    else:
        xp = np.pad(x, ((0, 0), (0, max(0, (T - 1) * hop + n - x.shape[1]))))
    idx = hop * np.arange(T)[:, None] + np.arange(n)[None, :]
    return np.fft.rfft(xp[:, idx] * w.astype(np.float64), axis=-1)


def ref_frames(X, w, n):
    """(..., F) -> (..., n): a real signal's DC (and Nyquist) bins carry no imaginary part; irfft; synthesis window."""
    X = np.array(X, dtype=np.complex128)
    X[..., 0] = X[..., 0].real
    if n % 2 == 0:
        X[..., -1] = X[..., -1].real
    return np.fft.irfft(X, n, axis=-1) * w.astype(np.float64)


def ref_istft(X, w, n, hop):
    """(B, T, F) -> (B, hop (T - 1) + (n & 1)): overlap-add over the envelope of the frames that exist, n // 2 trimmed."""
    fr = ref_frames(X, w, n)
    B, T, _ = fr.shape
    y = np.zeros((B, n + hop * (T - 1)))
    env = np.zeros(n + hop * (T - 1))
    w2 = w.astype(np.float64) ** 2
    for t in range(T):
        y[:, t * hop:t * hop + n] += fr[:, t]
        env[t * hop:t * hop + n] += w2
    lo, ln = n // 2, hop * (T - 1) + (n & 1)
    return y[:, lo:lo + ln] / env[lo:lo + ln]


# ---- harness ------------------------------------------------------------------------------------------------------------
def cpu(t):
    return t.detach().cpu().numpy()


def c128(t):
    """(..., 2 F) floats of interleaved complex64 -> complex128"""
    a = cpu(t).astype(np.float64)
    return a[..., 0::2] + 1j * a[..., 1::2]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def device_window(n, dev, alignment=16):
    w = torch.from_numpy(window64(n))
    if alignment == 4:                      # a view one float into its buffer, as a C-ABI caller's pointer may be
        buf = torch.zeros(n + 4, device=dev)
        buf[1:1 + n] = w.to(dev)
        w = buf[1:1 + n]
    else:
        w = w.to(dev)
    assert w.data_ptr() % 16 == (4 if alignment == 4 else 0)
    return w


class Guarded:
    """n floats pre-filled with NaN between guard bands, `offset` floats past the aligned start."""

    def __init__(self, n, dev, offset=0):
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.buf = torch.full((n + 2 * GUARD + offset,), SENTINEL, dtype=torch.float32, device=dev)
        self.out = self.buf[self.lo:self.hi]
        self.out.fill_(NAN)
        assert self.out.data_ptr() % 16 == 4 * (offset % 4)

    def result(self, what):
        g = torch.cat([self.buf[:self.lo], self.buf[self.hi:]])
        assert bool((g == SENTINEL).all()), ("guard band written", what)
        res = self.out.clone()
        assert not bool(torch.isnan(res).any()), ("element left unwritten", what)
        return res


def sweep(run, plans, what):
    """run(v) -> tuple of outputs under AT_VARIANT_FRAME_WALKERS = v.  Every plan: the bits of the default plan, which
    is returned."""
    assert plans[0] == 0 and W.ONE_TRIP in plans
    ref = run(0)
    for v in plans[1:]:
        for r, g in zip(ref, run(v)):
            if r is not None and not same_bits(r, g):
                bad = (r.view(torch.int32) != g.view(torch.int32)).nonzero()[:4].tolist()
                raise AssertionError((what, "walkers", v, "first differing elements", bad))
    return ref


def forward_run(x, B, L, stride, T, n, hop, center, w, want_phase=True):
    require_device(x, w)
    F = n // 2 + 1

    def run(v):
        spec = Guarded(2 * B * T * F, x.device)
        ph = Guarded(B * T * F, x.device) if want_phase else None
        with variant("frame_walkers", v):
            check(lib().at_stft_forward(ptr(x), B, L, stride, T, n, hop, int(center), ptr(w), ptr(spec.out),
                                        ptr(ph.out if ph else None), stream_ptr()), "at_stft_forward")
        return spec.result(("spectrum", v)).view(B, T, 2 * F), ph.result(("phase", v)).view(B, T, F) if ph else None
    return run


def frames_run(X, mag, phase, B, T, n, w):
    src = X if X is not None else mag
    require_device(src, w)

    def run(v):
        out = Guarded(B * T * n, src.device)
        with variant("frame_walkers", v):
            check(lib().at_irfft_frames_streams(ptr(X), ptr(mag), ptr(phase), B * T, T, n, ptr(w), ptr(out.out),
                                                stream_ptr()), "at_irfft_frames_streams")
        return (out.result(("frames", v)).view(B, T, n),)
    return run


def istft_run(X, mag, phase, B, T, n, hop, w, y_offset=0):
    """at_istft on its workspace path (no envelope table): the frames kernel of the size, then the gather."""
    src = X if X is not None else mag
    require_device(src, w)
    ln = W.out_len(n, hop, T)
    ws = torch.empty(B * T * n, dtype=torch.float32, device=src.device)

    def run(v):
        y = Guarded(B * ln, src.device, y_offset)
        with variant("frame_walkers", v):
            check(lib().at_istft(ptr(X), ptr(mag), ptr(phase), B, T, n, hop, ptr(w), ptr(None), ptr(y.out), ptr(ws),
                                 4 * ws.numel(), stream_ptr()), "at_istft")
        return (y.result(("istft", v, y_offset)).view(B, ln),)
    return run


def check_phase(spec, phase):
    """The phase side output against float64 atan2 of the spectrum the kernel itself wrote, wrapped to (-pi, pi]."""
    Xw = c128(spec)
    d = cpu(phase).astype(np.float64) - np.arctan2(Xw.imag, Xw.real)
    d = np.pi - np.mod(np.pi - d, 2.0 * np.pi)
    assert np.abs(d).max() < PHASE_TOL, np.abs(d).max()


def noise(shape, seed, dev, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def spectrum(B, T, F, seed, dev):
    """Finite noise with imaginary parts in the DC and Nyquist bins too (the inverse must ignore them)."""
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)).to(dev)


def polar(B, T, F, seed, dev):
    """Magnitudes in [0.1, 1.1), phases drawn up to +-1e5 rad."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(B, T, F, generator=g) + 0.1
    phase = (torch.rand(B, T, F, generator=g) * 2.0 - 1.0) * 1e5
    return mag.to(dev), phase.to(dev)


def polar128(mag, phase):
    return cpu(mag).astype(np.float64) * np.exp(1j * cpu(phase).astype(np.float64))


# ---- A: forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_forward_every_walk(dev, case):
    """at_stft_forward (what ops.stft_forward calls) with the phase side output: every walker count gives the bits of
    the default plan; the default plan is within the bar of float64, its phase within fast_atan2f's bound of atan2 of
    the spectrum it wrote.  The 4-byte-offset window takes 128 / 1024 / 2048 to the generic kernel; the aligned window
    (register core) is the control."""
    n, hop, B, T, L = case.n_fft, case.hop, case.B, case.T, case.L
    x = noise((B, L), n + hop, dev)
    w = device_window(n, dev, case.window_alignment)
    spec, phase = sweep(forward_run(x, B, L, L, T, n, hop, 1, w), W.plans(case), case.name)
    want = ref_forward(cpu(x), window64(n), n, hop)
    assert want.shape == (B, T, n // 2 + 1)
    err = rel_max(c128(spec), want)
    print(case.name, "forward rel_max", err)
    assert err < TOL, err
    check_phase(spec, phase)
    X, ph = ops.stft_forward(x, w, n, hop, want_phase=True)
    assert same_bits(torch.view_as_real(X).reshape(B, T, -1), spec) and same_bits(ph, phase)
    if case.window_alignment == 4:
        Xc, phc = ops.stft_forward(x, device_window(n, dev), n, hop, want_phase=True)
        assert rel_max(cpu(Xc).astype(np.complex128), want) < TOL
        check_phase(torch.view_as_real(Xc).reshape(B, T, -1), phc)


# ---- B: inverse frames --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_inverse_frames_every_walk(dev, case):
    """at_irfft_frames_streams (what ops.irfft_frames calls) from a complex spectrum and from magnitude + phase with
    phases up to +-1e5 rad: every walker count against the default plan, the default plan against float64."""
    n, B, T = case.n_fft, case.B, case.T
    F = n // 2 + 1
    w = device_window(n, dev, case.window_alignment)
    w64 = window64(n)
    X = spectrum(B, T, F, n, dev)
    (fr,) = sweep(frames_run(X, None, None, B, T, n, w), W.plans(case), (case.name, "complex"))
    want = ref_frames(cpu(X), w64, n)
    err = rel_max(cpu(fr).astype(np.float64), want)
    print(case.name, "frames rel_max", err)
    assert err < TOL, err
    assert same_bits(ops.irfft_frames(X, w, n), fr)
    mag, phase = polar(B, T, F, n + 1, dev)
    (fp,) = sweep(frames_run(None, mag, phase, B, T, n, w), W.plans(case), (case.name, "polar"))
    want_p = ref_frames(polar128(mag, phase), w64, n)
    err = rel_max(cpu(fp).astype(np.float64), want_p)
    print(case.name, "polar frames rel_max", err)
    assert err < POLAR_TOL, err
    assert same_bits(ops.irfft_frames(None, w, n, mag=mag, phase=phase), fp)
    if case.window_alignment == 4:
        wa = device_window(n, dev)
        assert rel_max(cpu(ops.irfft_frames(X, wa, n)).astype(np.float64), want) < TOL
        assert rel_max(cpu(ops.irfft_frames(None, wa, n, mag=mag, phase=phase)).astype(np.float64), want_p) < POLAR_TOL


# ---- C: the whole inverse -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_istft_every_walk(dev, case):
    """at_istft on its workspace path (what ops.istft calls at these sizes): frames kernel + gather under every walker
    and block count.  Where the gather takes four outputs per thread, an output 4 bytes off forces the scalar kernel:
    the same bits (the float4 form documents the same summation order).  This comparison found the two forms an ulp
    apart: the compiler fused the envelope's w * w + env in the float4 kernel and not in the scalar one, so a caller's
    pointer alignment showed in the result; both kernels now spell the fma out."""
    n, hop, B, T = case.n_fft, case.hop, case.B, case.T
    F = n // 2 + 1
    w = device_window(n, dev, case.window_alignment)
    X = spectrum(B, T, F, n + 2, dev)
    (y,) = sweep(istft_run(X, None, None, B, T, n, hop, w), W.plans(case), case.name)
    want = ref_istft(cpu(X), window64(n), n, hop)
    assert want.shape == tuple(y.shape)
    err = rel_max(cpu(y).astype(np.float64), want)
    print(case.name, "istft rel_max", err)
    assert err < TOL, err
    mag, phase = polar(B, T, F, n + 3, dev)
    (yp,) = sweep(istft_run(None, mag, phase, B, T, n, hop, w), (0, W.ONE_TRIP, 1), (case.name, "polar"))
    err = rel_max(cpu(yp).astype(np.float64), ref_istft(polar128(mag, phase), window64(n), n, hop))
    print(case.name, "polar istft rel_max", err)
    assert err < POLAR_TOL, err
    if case.window_alignment == 16:
        assert same_bits(ops.istft(X, w, n, hop), y)
    else:
        assert rel_max(cpu(ops.istft(X, device_window(n, dev), n, hop)).astype(np.float64), want) < TOL
    if W.gather_float4(n, hop) and case.window_alignment == 16:
        scalar = istft_run(X, None, None, B, T, n, hop, w, y_offset=1)
        for v in (0, 1, 4):
            assert same_bits(scalar(v)[0], y), ("scalar gather against the float4 form", case.name, v)


# ---- D: center=False over a strided view --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", W.UNCENTRED, ids=["%s_%d" % (f[0], f[1]) for f in W.UNCENTRED])
def test_uncentred_frames_past_the_clip_end(dev, form):
    """center=False with explicit T, clip_stride > L and L: the last frame ends past the clip and is filled with zeros.
    The floats between L and clip_stride are NaN: nothing past a clip's end may be read."""
    kernel, n, hop, L, stride, T = form
    B = 3 if n < 8192 else 2
    N = B * T
    buf = noise((B, stride), n + 5, dev)
    buf[:, L:] = NAN
    w = device_window(n, dev)
    plans = (0, W.ONE_TRIP, 1, 4, N - 1)
    spec, phase = sweep(forward_run(buf, B, L, stride, T, n, hop, 0, w), plans, form)
    want = ref_forward(cpu(buf[:, :L]), window64(n), n, hop, center=False, T=T)
    err = rel_max(c128(spec), want)
    print(form, "uncentred rel_max", err)
    assert err < TOL, err
    check_phase(spec, phase)
    X = ops.stft_forward(buf, w, n, hop, center=False, T=T, clip_stride=stride, L=L, B=B)
    assert same_bits(torch.view_as_real(X).reshape(B, T, -1), spec)


# ---- E: the shortest legal clip -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", W.SHORTEST, ids=["%s_%d" % (f[0], f[1]) for f in W.SHORTEST])
def test_shortest_clip_reflects_at_both_ends(dev, form):
    """L = n_fft // 2 + 1: the reflect padding is as long as it may be and one frame reflects at both ends of the clip.
    Forward and the inverse of the result."""
    kernel, n, hop = form
    B, L = 3, n // 2 + 1
    T = W.frames_of(n, hop, L)
    x = noise((B, L), n + 7, dev)
    w = device_window(n, dev)
    plans = (0, W.ONE_TRIP, 1, 2, B * T - 1)
    spec, phase = sweep(forward_run(x, B, L, L, T, n, hop, 1, w), plans, form)
    err = rel_max(c128(spec), ref_forward(cpu(x), window64(n), n, hop))
    print(form, "shortest clip rel_max", err)
    assert err < TOL, err
    check_phase(spec, phase)
    X = torch.view_as_complex(spec.reshape(B, T, n // 2 + 1, 2).contiguous())
    (y,) = sweep(istft_run(X, None, None, B, T, n, hop, w), plans, (form, "inverse"))
    assert rel_max(cpu(y).astype(np.float64), ref_istft(c128(spec), window64(n), n, hop)) < TOL


# ---- F: the default plan across its cap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", W.ACROSS_CAP, ids=["%s_%d" % (f[0], f[1]) for f in W.ACROSS_CAP])
def test_default_plan_walks_past_4096_frames(dev, form):
    """6003 frames: the default launch itself takes 4096 workgroups, 1907 of which walk to a second frame in another
    clip.  Forward and inverse: the bits of one workgroup per frame, and the bar against float64."""
    kernel, n, hop, B, L = form
    T = W.frames_of(n, hop, L)
    assert B * T > W.WALK_CAP
    x = noise((B, L), n + 11, dev)
    w = device_window(n, dev)
    spec, phase = sweep(forward_run(x, B, L, L, T, n, hop, 1, w), (0, W.ONE_TRIP), form)
    assert rel_max(c128(spec), ref_forward(cpu(x), window64(n), n, hop)) < TOL
    check_phase(spec, phase)
    X = torch.view_as_complex(spec.reshape(B, T, n // 2 + 1, 2).contiguous())
    (y,) = sweep(istft_run(X, None, None, B, T, n, hop, w), (0, W.ONE_TRIP), (form, "inverse"))
    assert rel_max(cpu(y).astype(np.float64), ref_istft(c128(spec), window64(n), n, hop)) < TOL
    assert same_bits(ops.istft(X, w, n, hop), y)


# ---- G: the workspace error of a fused shape with a 4-byte-aligned window ------------------------------------------------
def test_fused_shape_with_offset_window_fails_before_launching(dev):
    """at_istft_workspace_bytes is 0 at n_fft 1024 / hop 256 -- for a 16-byte aligned window.  A 4-byte-offset view
    takes at_istft off the fused kernel, which then needs the frames workspace: AT_EWORKSPACE, nothing launched, y
    untouched."""
    n, hop, B, T = 1024, 256, 2, 9
    X = spectrum(B, T, n // 2 + 1, 3, dev)
    wm = device_window(n, dev, 4)
    assert lib().at_istft_workspace_bytes(B, T, n, hop) == 0
    with pytest.raises(AcidsHipError, match="at_istft"):
        ops.istft(X, wm, n, hop)
    env = ops.istft_envelope_table(device_window(n, dev), n, hop)
    y = torch.full((B * hop * (T - 1),), SENTINEL, dtype=torch.float32, device=dev)
    rc = lib().at_istft(ptr(X), ptr(None), ptr(None), B, T, n, hop, ptr(wm), ptr(env), ptr(y), ptr(None), 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc == AT_EWORKSPACE
    assert bool((y == SENTINEL).all())
    # the same call with the workspace it asks for runs (generic frames kernel + scalar gather)
    ws = torch.empty(B * T * n, dtype=torch.float32, device=dev)
    check(lib().at_istft(ptr(X), ptr(None), ptr(None), B, T, n, hop, ptr(wm), ptr(env), ptr(y), ptr(ws), 4 * ws.numel(),
                         stream_ptr()), "at_istft")
    assert rel_max(cpu(y).reshape(B, -1).astype(np.float64), ref_istft(cpu(X), window64(n), n, hop)) < TOL

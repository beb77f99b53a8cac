"""Every row plan of the projection kernels (banded, fixed 513-bin, small dense, n_fft-512 / 2048 features-only, dense
MFMA GEMM, bf16), forced through AT_VARIANT_ROW_RUN.

Each launcher cuts its rows (frames, frame pairs, tiles) from the row count and the device; at the suite's sizes every
one takes its minimum cut, so the cuts of real batches ran on no test.  The sweeps of row_plan_cases.py (their store
coverage and geometry are checked on the CPU by test_row_plan_cases_cpu.py) hold every cut bit for bit to the default
plan and to one run over everything (README: bit-identical whatever batch a clip rides in), with one float64 check per
form.  Every output is pre-filled with NaN between guard bands: a missing store or a stray one fails, whatever the
caching allocator hands back."""
import ctypes

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import row_plan_cases as P
from acids_transforms_amd import ops
from acids_transforms_amd._lib import VARIANTS, check, lib, ptr, require_device, stream_ptr, variant
from acids_transforms_amd.utils.banded import BandedBank
from conftest import rel_max
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
GUARD = 256             # floats of guard band on either side of an output (keeps the output 1 KB aligned)
SENTINEL = -7777.0
NAN = float("nan")


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def _variants_back_to_default():
    yield
    assert all(lib().at_get_variant(w) == 0 for w in VARIANTS.values())


def launch(v, n, fn, fill=NAN, complex_out=False):
    """fn(out_view) under AT_VARIANT_ROW_RUN = v into n floats pre-filled with `fill` between guard bands: the guards
    must come back untouched and (for a NaN fill) no NaN may be left.  Returns a copy of the output."""
    dev = torch.device("cuda:0")
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + n] = fill
    out = buf[GUARD:GUARD + n]
    with variant("row_run", v):
        fn(out.view(torch.complex64) if complex_out else out)
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    assert bool((g == SENTINEL).all()), ("guard band written", v)
    res = out.clone()
    if fill != fill:
        assert not bool(torch.isnan(res).any()), ("element left unwritten", v)
    else:
        assert not bool((res == fill).any()), ("element left unwritten", v)
    return res


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def sweep_equal(n, fn, vs, what, fill=NAN, complex_out=False):
    """The default plan, one run over everything and every forced cut of `vs`: identical bits.  Returns the default."""
    ref = launch(0, n, fn, fill, complex_out)
    assert same_bits(launch(P.ROW_RUN_MAX, n, fn, fill, complex_out), ref), (what, "one run")
    for v in vs:
        assert same_bits(launch(v, n, fn, fill, complex_out), ref), (what, v)
    return ref


def mel_bank(n_freqs, n_mels, sr=44100):
    return O.melscale_fbanks(n_freqs, 0.0, float(sr // 2), n_mels, sr).float()


def spectrum(rows, K, g, dev):
    re = torch.randn(rows, K, generator=g)
    im = torch.randn(rows, K, generator=g)
    return torch.complex(re, im).to(dev)


def norm_pair(dev, on):
    if not on:
        return None, None
    return torch.tensor(0.375, device=dev), torch.tensor(1.625, device=dev)


# ---- banded -------------------------------------------------------------------------------------------------------------
def banded(x, a_kind, band, contrast, off, sc, T=0, inverse=False, ld_out=None, phase_out=None, ld_phase=0,
           ph_off=None, ph_sc=None, phase_in=None, rows=None, lda=None):
    def fn(out):
        ops._project_banded(x, a_kind, band, contrast, inverse, off, sc, 1.1920929e-07, out, band.N, T, ld_out=ld_out,
                            phase_out=phase_out(out) if phase_out else None, ld_phase=ld_phase, phase_offset=ph_off,
                            phase_scale=ph_sc, phase_in=phase_in, rows=rows, lda=lda)
    return fn


BANDED_CM = [
    # name, n_fft, n_mels (1 pass <= 64 < 2 passes <= 128; 3 passes: the scalar channel-major walk), power, contrast, norm
    ("nfft256_cmw2", 256, 100, 2, None, False),
    ("nfft512_cmw1", 512, 40, 2, "log", True),
    ("nfft1024_cmw2", 1024, 128, 1, "log1p", True),
    ("nfft2048_cmw2", 2048, 128, 2, None, False),
    ("nfft4096_cmw1", 4096, 64, 2, "log10", False),
    ("nfft400_scalar", 400, 80, 2, None, True),
    ("nfft1024_3pass_scalar", 1024, 160, 2, "log", False),
]


@pytest.mark.parametrize("form", BANDED_CM, ids=[f[0] for f in BANDED_CM])
def test_banded_channel_major_every_cut(dev, form):
    """mel_banded_kernel's channel-major output: the register-window variants (CMW 1 / 2 at 3, 5, 9, 17, 33 segments)
    and the scalar store (4 segments; a 3-pass bank).  Every cut of CM_SWEEP: runs of 1 row, of every length mod 4,
    runs across 2+ clip boundaries, every partial flush at a run end and a clip end."""
    name, n_fft, n_mels, power, contrast, norm = form
    K = n_fft // 2 + 1
    bank = mel_bank(K, n_mels)
    band = BandedBank(bank)
    assert band.eligible
    g = torch.Generator().manual_seed(n_fft + n_mels)
    Tmax = max(T for _, T, _ in P.CM_SWEEP)
    xall = spectrum(4 * Tmax, K, g, dev)
    off, sc = norm_pair(dev, norm)
    kind = 1 if power == 2 else 0
    vs = sorted({v for _, _, v in P.CM_SWEEP})
    for B, T in sorted({(B, T) for B, T, _ in P.CM_SWEEP}):
        x = xall[:B * T].contiguous()
        ref = sweep_equal(B * n_mels * T, banded(x, kind, band, contrast, off, sc, T=T), vs, (name, B, T))
        if (B, T) == (4, 17):
            Xr = x.cpu().reshape(B, T, K).to(torch.complex128)
            mag = Xr.abs() ** power @ bank.double()
            want = O.contrast(mag, contrast)
            if norm:
                want = (want - off.item()) / sc.item()
            assert rel_max(cpu(ref).reshape(B, n_mels, T), want.transpose(-2, -1).numpy()) < TOL


BANDED_ROWS = [
    # name, K, n_mels, a_kind (0 |X|, 1 |X|^2, 3 |real|), contrast, norm
    ("abs_513", 513, 128, 0, "log", True),
    ("abs2_513", 513, 128, 1, None, False),
    ("abs_751_next_kernel", 751, 96, 0, "log1p", True),
    ("abs_257_exact", 257, 64, 0, None, True),
    ("real_513", 513, 128, 3, "log1p", False),
    ("real_2049", 2049, 128, 3, None, True),
]


@pytest.mark.parametrize("form", BANDED_ROWS, ids=[f[0] for f in BANDED_ROWS])
def test_banded_row_major_every_cut(dev, form):
    """mel_banded_kernel, row-major: complex rows on the two-register-set loop (odd run lengths in the middle of the
    launch), real rows on the single-buffered loop; exact NSEG and the next larger kernel (K = 751 -> 17 segments)."""
    name, K, n_mels, kind, contrast, norm = form
    bank = mel_bank(K, n_mels)
    band = BandedBank(bank)
    assert band.eligible
    g = torch.Generator().manual_seed(K + kind)
    nmax = max(r for r, _ in P.ROW_SWEEP)
    xall = spectrum(nmax, K, g, dev) if kind < 3 else torch.randn(nmax, K, generator=g).to(dev)
    off, sc = norm_pair(dev, norm)
    vs = sorted({v for _, v in P.ROW_SWEEP})
    for rows in sorted({r for r, _ in P.ROW_SWEEP}):
        x = xall[:rows].contiguous()
        ref = sweep_equal(rows * n_mels, banded(x, kind, band, contrast, off, sc), vs, (name, rows))
        if rows == nmax:
            xd = x.cpu().to(torch.complex128 if kind < 3 else torch.float64)
            mag = (xd.abs() ** (2 if kind == 1 else 1)) @ bank.double()
            want = O.contrast(mag, contrast)
            if norm:
                want = (want - off.item()) / sc.item()
            assert rel_max(cpu(ref).reshape(rows, n_mels), want.numpy()) < TOL


@pytest.mark.parametrize("norm", [False, True])
def test_banded_inverse_every_cut(dev, norm):
    """Magnitude.invert's banded walk (real rows, inverse contrast before the walk) over every cut."""
    fwd, inv = O.magnitude_banks(mel_bank(513, 128))
    inv = inv[0].float()                                   # (128, 513)
    band = BandedBank(inv)
    assert band.eligible
    g = torch.Generator().manual_seed(3 + norm)
    nmax = max(r for r, _ in P.ROW_SWEEP)
    yall = (torch.rand(nmax, 128, generator=g) * 2).to(dev)
    off, sc = norm_pair(dev, norm)
    vs = sorted({v for _, v in P.ROW_SWEEP})
    for rows in sorted({r for r, _ in P.ROW_SWEEP}):
        y = yall[:rows].contiguous()
        ref = sweep_equal(rows * 513, banded(y, 2, band, "log1p", off, sc, inverse=True), vs, ("inverse", rows))
        if rows == nmax:
            stats = (off.item(), sc.item()) if norm else (None, None)
            want = O.magnitude_invert(y.cpu().double(), inv[None].double(), "log1p", *stats)
            assert rel_max(cpu(ref).reshape(rows, 513), want.numpy()) < TOL


def test_polar_forward_and_inverse_every_cut(dev):
    """Polar / PolarIF's stacked forward (magnitude rows and normalised angles in one pass, phase_out) and Polar.invert
    (phase_in: complex output), every cut of ROW_SWEEP."""
    F = 513
    raw = O.magnitude_default_bank(44100, 1024)
    fwd, inv = O.magnitude_banks(raw)
    fband, iband = BandedBank(fwd[0].float()), BandedBank(inv[0].float())
    assert fband.eligible and iband.eligible
    g = torch.Generator().manual_seed(29)
    nmax = max(r for r, _ in P.ROW_SWEEP)
    xall = spectrum(nmax, F, g, dev)
    off, sc = norm_pair(dev, True)
    po, ps = torch.tensor(0.5, device=dev), torch.tensor(3.25, device=dev)
    vs = sorted({v for _, v in P.ROW_SWEEP})
    for rows in sorted({r for r, _ in P.ROW_SWEEP}):
        x = xall[:rows].contiguous()
        for o, s, q, r in ((off, sc, po, ps), (None, None, None, None)):
            fn = banded(x, 0, fband, "log1p", o, s, ld_out=2 * F, ld_phase=2 * F, ph_off=q, ph_sc=r,
                        phase_out=lambda out: ctypes.c_void_p(out.data_ptr() + 4 * F))
            y = sweep_equal(rows * 2 * F, fn, vs, ("polar", rows, o is None)).view(rows, 2, F)
            inv_fn = banded(y, 2, iband, "log1p", o, s, inverse=True, ld_out=F, ld_phase=2 * F, ph_off=q, ph_sc=r,
                            phase_in=ctypes.c_void_p(y.data_ptr() + 4 * F), rows=rows, lda=2 * F)
            xi = sweep_equal(rows * 2 * F, inv_fn, vs, ("polar.invert", rows, o is None), complex_out=True)
            if rows == nmax and o is not None:
                Xr = x.cpu().to(torch.complex128)
                want = O.magnitude_forward(Xr, fwd.double(), "log1p", off.item(), sc.item())     # fwd: (1, F, F)
                assert rel_max(cpu(y[:, 0]), want.numpy()) < TOL
                ang = (cpu(y[:, 1]).astype(np.float64) * ps.item()) + po.item()
                big = np.abs(Xr.numpy()) > 1e-3 * np.abs(Xr.numpy()).max()
                d = np.angle(np.exp(1j * (ang - np.angle(Xr.numpy()))))
                assert np.abs(d[big]).max() < 1e-3
                mag = O.magnitude_invert(y[:, 0].cpu().double(), inv.double(), "log1p", off.item(), sc.item())
                want_c = mag * torch.exp(1j * torch.from_numpy(ang))
                assert rel_max(cpu(xi.view(torch.complex64)).reshape(rows, F), want_c.numpy()) < 1e-4


# ---- fixed 513-bin projection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
def test_fixed_projection_every_cut(dev, norm):
    """mel_fixed_kernel (the headline |X| @ 128-mel, log1p, row-major) on its three-register-set prefetch ring."""
    mg = A.Magnitude(n_mels=128)
    bank = mg.mel_bank.reshape(513, -1).float()
    band = BandedBank(bank)
    assert band.eligible and list(band.pass_len[:2]) == [32, 8] and band.n_passes == 2
    g = torch.Generator().manual_seed(41 + norm)
    nmax = max(r for r, _ in P.ROW_SWEEP)
    xall = spectrum(nmax, 513, g, dev)
    off, sc = norm_pair(dev, norm)
    vs = sorted({v for _, v in P.ROW_SWEEP})
    for rows in sorted({r for r, _ in P.ROW_SWEEP}):
        x = xall[:rows].contiguous()
        ref = sweep_equal(rows * 128, banded(x, 0, band, "log1p", off, sc), vs, ("fixed", rows))
        with variant("epilogue", 1):                      # the generic kernel: same formula, not the same bits
            gen = launch(0, rows * 128, banded(x, 0, band, "log1p", off, sc))
        assert rel_max(cpu(ref), cpu(gen)) < TOL
        if rows == nmax:
            want = O.magnitude_forward(x.cpu().to(torch.complex128), bank[None].double(), "log1p",
                                       *((off.item(), sc.item()) if norm else (None, None)))
            assert rel_max(cpu(ref).reshape(rows, 128), want.numpy()) < TOL


# ---- small dense projection ---------------------------------------------------------------------------------------------
def small(x, W, off, sc, T=0):
    rows, K = x.shape
    N = W.shape[1]

    def fn(out):
        check(lib().at_project_small(ptr(x), rows, K, ptr(W), N, ptr(off), ptr(sc), ptr(out), T, stream_ptr()),
              "at_project_small")
    return fn


def dct(n_mels, n_mfcc):
    return O.mfcc_dct(torch.eye(n_mels), n_mfcc).contiguous()      # (n_mels, n_mfcc): x @ dct(..) is MFCC's DCT-II


SMALL_FORMS = [(128, 40), (80, 20), (64, 64), (20, 13), (33, 7), (40, 40)]


@pytest.mark.parametrize("K,N", SMALL_FORMS, ids=["%dx%d" % kn for kn in SMALL_FORMS])
def test_small_projection_row_form_every_cut(dev, K, N):
    """small_proj_kernel (the row form; forced for K = 128 / 80 / 64): its 4-row ring past 4 rows per wave, and the
    channel-major window at every run start and end (the `first < run_t0` clamp)."""
    W = dct(K, N).to(dev)
    g = torch.Generator().manual_seed(K * N)
    Tmax = max(T for _, T, _ in P.CM_SWEEP)
    nmax = max(4 * Tmax, max(r for r, _ in P.ROW_SWEEP))
    xall = torch.randn(nmax, K, generator=g).to(dev)
    off, sc = norm_pair(dev, K % 2 == 0)
    with variant("small_projection", 1):
        vs = sorted({v for _, _, v in P.CM_SWEEP})
        for B, T in sorted({(B, T) for B, T, _ in P.CM_SWEEP}):
            x = xall[:B * T].contiguous()
            ref = sweep_equal(B * T * N, small(x, W, off, sc, T=T), vs, ("small cm", B, T))
            if (B, T) == (4, 31):
                want = x.cpu().double().reshape(B, T, K) @ W.cpu().double()
                if off is not None:
                    want = (want - off.item()) / sc.item()
                assert rel_max(cpu(ref).reshape(B, N, T), want.transpose(-2, -1).numpy()) < TOL
        vs = sorted({v for _, v in P.ROW_SWEEP})
        for rows in sorted({r for r, _ in P.ROW_SWEEP}):
            sweep_equal(rows * N, small(xall[:rows].contiguous(), W, off, sc), vs, ("small rows", rows))


@pytest.mark.parametrize("K,N", [(128, 40), (80, 20), (64, 64)], ids=["128x40", "80x20", "64x64"])
def test_small_projection_mfma_form_every_cut(dev, K, N):
    """small_proj_mfma_kernel: runs of 1, 2 and 3+ 32-row tile pairs, runs that start and end mid-clip, row-major and
    channel-major (the MFCC DCT of MFCC(n_mfcc))."""
    W = dct(K, N).to(dev)
    g = torch.Generator().manual_seed(K + N)
    nmax = max(B * T for B, T, _ in P.MFMA_SWEEP)
    xall = torch.randn(nmax, K, generator=g).to(dev)
    off, sc = norm_pair(dev, True)
    vs = sorted({v for _, _, v in P.MFMA_SWEEP})
    for B, T in sorted({(B, T) for B, T, _ in P.MFMA_SWEEP}):
        x = xall[:B * T].contiguous()
        assert x.data_ptr() % 16 == 0
        ref = sweep_equal(B * T * N, small(x, W, off, sc, T=T), vs, ("mfma cm", B, T))
        sweep_equal(B * T * N, small(x, W, None, None), vs, ("mfma rows", B, T))
        if (B, T) == (2, 100):
            want = (x.cpu().double().reshape(B, T, K) @ W.cpu().double() - off.item()) / sc.item()
            assert rel_max(cpu(ref).reshape(B, N, T), want.transpose(-2, -1).numpy()) < TOL


# ---- fused features-only forward at n_fft 512 / 2048 --------------------------------------------------------------------
def fused(x, w, band, n_fft, hop, T, cm, power, contrast, off, sc):
    B, L = x.shape
    require_device(x, w)                  # at_init: the twiddle tables of the device
    lf, ls, wt = band.on(x.device)

    def fn(out):
        check(lib().at_stft_mel_forward(ptr(x), B, L, L, T, n_fft, hop, ptr(w), ptr(lf), ptr(ls), ptr(wt), band.N,
                                        band.n_passes, band.pass_len.ctypes.data, ops.contrast_code(contrast),
                                        int(power == 2), ptr(off), ptr(sc), 1.1920929e-07, ptr(None), ptr(None), ptr(out),
                                        int(cm), stream_ptr()), "at_stft_mel_forward")
    return fn


# n_fft, n_mels, channel-major, sample rate (a one-pass bank at 2048 that the fused kernel takes: 64 mels at 16 kHz).
# At 2048 the analysis window joins the bank in LDS when 8 KB are left (launch_stft2048_mel): the bands of 60 mels at
# 4 kHz and of 128 at 44.1 kHz leave them, those of 64 at 16 kHz and of 100 at 44.1 kHz do not -- each of the register
# windows (one pass, two passes, none) with the window in LDS and without.
FUSED = [(512, 40, True, 44100), (512, 128, True, 44100), (512, 128, False, 44100), (2048, 64, True, 16000),
         (2048, 128, True, 44100), (2048, 100, False, 44100), (2048, 60, True, 4000), (2048, 100, True, 44100),
         (2048, 128, False, 44100)]


@pytest.mark.parametrize("n_fft,n_mels,cm,sr", FUSED, ids=["%d_%d_%s" % (a, b, "cm" if c else "rows") for a, b, c, _ in
                                                           FUSED])
def test_fused_features_every_cut(dev, n_fft, n_mels, cm, sr):
    """stft512_mel_kernel (runs of per-clip frame pairs; the half pair that ends an odd-T clip first, mid-run and last in a run)
    and stft2048_mel_kernel (runs of frames): MelSpectrogram's one-kernel forward, 1- and 2-pass banks, channel-major
    through the register window and row-major."""
    F = n_fft // 2 + 1
    bank = mel_bank(F, n_mels, sr)
    band = BandedBank(bank)
    assert band.fusable512 if n_fft == 512 else band.fusable2048
    assert band.n_passes == (1 if n_mels <= 64 else 2)
    w = torch.hann_window(n_fft, device=dev)
    g = torch.Generator().manual_seed(n_fft + n_mels)
    sweep = P.S512_SWEEP if n_fft == 512 else P.CM_SWEEP
    xall = (torch.randn(4, n_fft // 4 * 32 + n_fft, generator=g) * 0.1).to(dev)
    off, sc = norm_pair(dev, n_mels == 128)
    contrast = "log" if n_mels == 128 else None
    vs = sorted({v for _, _, v in sweep})
    checked = False
    for B, T in sorted({(B, T) for B, T, _ in sweep}):
        hop = n_fft // 4 if T >= 3 else n_fft
        L = hop * (T - 1) + 4 if T >= 3 else n_fft // 2 + 4
        assert 1 + L // hop == T
        x = xall[:B, :L].contiguous()
        ref = sweep_equal(B * T * n_mels, fused(x, w, band, n_fft, hop, T, cm, 2, contrast, off, sc), vs,
                          (n_fft, n_mels, B, T))
        if not checked and T >= 16:
            checked = True
            X = torch.stft(x.cpu().double(), n_fft, hop, window=torch.hann_window(n_fft, dtype=torch.float64),
                           return_complex=True)                                   # (B, F, T)
            mel = (X.abs() ** 2).transpose(-1, -2) @ bank.double()               # (B, T, n_mels)
            want = O.contrast(mel, contrast)
            if off is not None:
                want = (want - off.item()) / sc.item()
            got = cpu(ref).reshape(B, n_mels, T) if cm else cpu(ref).reshape(B, T, n_mels).transpose(0, 2, 1)
            assert rel_max(got, want.transpose(-2, -1).numpy()) < TOL
            if contrast is None and off is None:
                ms = O.melspectrogram(x.cpu(), sr, n_fft, hop, n_mels).double()      # float32 oracle
                assert rel_max(got, ms.numpy()) < TOL
    assert checked


# ---- dense MFMA GEMM ----------------------------------------------------------------------------------------------------
def gemm(x, bank, contrast, off, sc, inverse=False, T=0):
    rows, K = x.shape
    N = bank.shape[1]
    bank = bank.contiguous()
    kind = 2 if inverse else ops._a_kind(x)

    def fn(out):
        check(lib().at_mel_project(ptr(x), kind, rows, K, K, ptr(bank), N, N, ops.contrast_code(contrast), int(inverse),
                                   ptr(off), ptr(sc), 1.1920929e-07, ptr(out), N, T, stream_ptr()), "at_mel_project")
    return fn


GEMM_K = [20, 40, 100, 129, 257, 300, 450, 513, 576]       # every NL (1..5) and KSTEPS (4..128), with K tails


@pytest.mark.parametrize("K", GEMM_K)
def test_dense_gemm_every_tile_count(dev, K):
    """mel_gemm_kernel with 1, 2, 3, 4 and 7 tiles per workgroup (the next tile's prefetch, the LDS double buffer, the
    flag ring wrapping twice) and short last blocks; a dense and a banded bank, 128 and 200 columns, channel-major."""
    g = torch.Generator().manual_seed(K)
    nmax = max(r for r, _ in P.GEMM_SWEEP)
    xall = spectrum(nmax, K, g, dev)
    banks = [mel_bank(K, 128).to(dev), (torch.rand(K, 200, generator=g) + 0.1).to(dev)]
    off, sc = norm_pair(dev, K % 2 == 1)
    vs = sorted({v for _, v in P.GEMM_SWEEP})
    for rows in sorted({r for r, _ in P.GEMM_SWEEP}):
        x = xall[:rows].contiguous()
        for bank in banks:
            N = bank.shape[1]
            ref = sweep_equal(rows * N, gemm(x, bank, "log1p", off, sc), vs, ("gemm", K, rows, N))
            if rows == nmax:
                want = O.magnitude_forward(x.cpu().to(torch.complex128), bank.cpu().double()[None], "log1p",
                                           *((off.item(), sc.item()) if off is not None else (None, None)))
                assert rel_max(cpu(ref).reshape(rows, N), want.numpy()) < TOL
        if rows % 5 == 0:
            sweep_equal(rows * 128, gemm(x, banks[0], None, None, None, T=rows // 5), vs, ("gemm cm", K, rows))


def test_dense_gemm_inverse_every_tile_count(dev):
    """Magnitude.invert through the dense GEMM (inverse contrast on the staged tile), every tile count."""
    fwd, inv = O.magnitude_banks(mel_bank(513, 128))
    invb = inv[0].float().to(dev)                         # (128, 513)
    g = torch.Generator().manual_seed(7)
    nmax = max(r for r, _ in P.GEMM_SWEEP)
    yall = (torch.rand(nmax, 128, generator=g) * 2).to(dev)
    off, sc = norm_pair(dev, True)
    vs = sorted({v for _, v in P.GEMM_SWEEP})
    for rows in sorted({r for r, _ in P.GEMM_SWEEP}):
        y = yall[:rows].contiguous()
        ref = sweep_equal(rows * 513, gemm(y, invb, "log1p", off, sc, inverse=True), vs, ("gemm inverse", rows))
        if rows == nmax:
            want = O.magnitude_invert(y.cpu().double(), invb.cpu().double()[None], "log1p", off.item(), sc.item())
            assert rel_max(cpu(ref).reshape(rows, 513), want.numpy()) < TOL


@pytest.mark.parametrize("case", P.GEMM_POISON, ids=["%dt_v%d_%s" % (t, v, "-".join(map(str, b))) for t, v, b in
                                                      P.GEMM_POISON])
def test_dense_gemm_non_finite_tiles_every_position(dev, case):
    """A tile holding inf / NaN takes the dense path (0 * NaN stays NaN).  Poisoned tiles at block positions 0..3, in
    consecutive tiles, as the last tile of a short block: the flag of every one must reach its iteration of the ring.
    Poisoned rows match the float64 dense contraction's inf / NaN pattern, every other row the default plan's bits."""
    tiles, v, poisoned = case
    rows, K = 32 * tiles - 5, 513
    bank = mel_bank(K, 128)
    g = torch.Generator().manual_seed(tiles * 10 + v)
    X = spectrum(rows, K, g, torch.device("cpu"))
    bad_rows = []
    for i, t in enumerate(poisoned):
        r = min(32 * t + 3 + 7 * i, rows - 1)
        X[r, 400 - 50 * i] = complex(float("nan"), 0.0) if i % 2 == 0 else complex(float("inf"), 1.0)
        bad_rows.append(r)
    x = X.to(dev)
    fn = gemm(x, bank.to(dev), None, None, None)
    fill = -1.25e30                                    # outputs hold NaN here: an unwritten element shows as the fill
    ref = launch(0, rows * 128, fn, fill).view(rows, 128)
    got = launch(v, rows * 128, fn, fill).view(rows, 128)
    want = (X.abs().double() @ bank.double()).numpy()
    ok = np.ones(rows, bool)
    ok[bad_rows] = False
    g_np = cpu(got)
    assert np.array_equal(np.isnan(g_np[~ok]), np.isnan(want[~ok])), "NaN pattern of the poisoned rows"
    assert np.array_equal(np.isinf(g_np[~ok]), np.isinf(want[~ok])), "inf pattern of the poisoned rows"
    assert np.isnan(want[~ok]).any()
    assert same_bits(got[torch.from_numpy(ok).to(dev)], ref[torch.from_numpy(ok).to(dev)])
    assert rel_max(g_np[ok], want[ok]) < TOL


# ---- bf16 ---------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).float()


def test_bf16_projection_several_trips(dev):
    """mel_bf16_kernel's persistent loop taking 1, 2, 3+ tiles per workgroup: bits of the default plan, and the
    exact-operand check (bf16 operands: exact products, only the summation order differs from float64)."""
    K, N = 513, 128
    g = torch.Generator().manual_seed(55)
    bank = _bf16(torch.rand(K, N, generator=g) * (torch.rand(K, N, generator=g) < 0.3))
    img = ops.mel_bf16_pack_bank(bank.to(dev))
    nmax = max(r for r, _ in P.BF16_SWEEP)
    aall = _bf16(torch.rand(nmax, K, generator=g) * 3.0)
    vs = sorted({v for _, v in P.BF16_SWEEP})
    for rows in sorted({r for r, _ in P.BF16_SWEEP}):
        a = aall[:rows].to(dev).contiguous()
        ref = sweep_equal(rows * N, lambda out: ops.mel_forward_bf16(a, img, K, N, out=out.view(rows, N)), vs,
                          ("bf16", rows))
        want = aall[:rows].double() @ bank.double()
        assert rel_max(cpu(ref).reshape(rows, N), want.numpy()) < TOL


# ---- natural large shapes: the default plan above its minimum ----------------------------------------------------------
def test_large_shapes_default_plan_matches_the_minimum_cut(dev):
    """One production-sized shape per launcher, where the default plan cuts more than its minimum: bit for bit the
    launcher's minimum cut (the float64 checks above cover the arithmetic)."""
    g = torch.Generator(device=dev).manual_seed(99)
    # banded, channel-major (MelSpectrogram at n_fft 512 on 300k frames) and complex row-major
    bank = mel_bank(257, 128)
    band = BandedBank(bank)
    B, T = 1000, 300
    X = torch.complex(torch.randn(B * T, 257, device=dev, generator=g), torch.randn(B * T, 257, device=dev, generator=g))
    fn = banded(X, 1, band, "log", None, None, T=T)
    assert same_bits(launch(0, B * T * 128, fn), launch(8, B * T * 128, fn))
    bank1 = A.Magnitude(n_mels=128).mel_bank.reshape(513, -1).float()
    X = torch.complex(torch.randn(300_000, 513, device=dev, generator=g), torch.randn(300_000, 513, device=dev, generator=g))
    fn = banded(X, 0, BandedBank(bank1), "log1p", None, None)              # the fixed form
    assert same_bits(launch(0, 300_000 * 128, fn), launch(8, 300_000 * 128, fn))
    del X
    # small projection, both forms (the MFCC DCT at 1024 clips of 4 s: 706 560 rows)
    W = dct(128, 40).to(dev)
    x = torch.randn(706_560, 128, device=dev, generator=g)
    fn = small(x, W, None, None, T=690)
    assert same_bits(launch(0, 706_560 * 40, fn), launch(64, 706_560 * 40, fn))
    W = dct(40, 13).to(dev)
    x = torch.randn(40_020, 40, device=dev, generator=g)
    fn = small(x, W, None, None, T=690)
    assert same_bits(launch(0, 40_020 * 13, fn), launch(4, 40_020 * 13, fn))
    # fused features-only forwards
    for n_fft, n_mels, Bc, L in ((512, 128, 256, 44100), (2048, 128, 128, 262144)):
        F = n_fft // 2 + 1
        band = BandedBank(mel_bank(F, n_mels))
        w = torch.hann_window(n_fft, device=dev)
        hop = n_fft // 4
        T = 1 + L // hop
        x = torch.randn(Bc, L, device=dev, generator=g) * 0.1
        fn = fused(x, w, band, n_fft, hop, T, True, 2, "log", None, None)
        assert same_bits(launch(0, Bc * T * n_mels, fn), launch(4 if n_fft == 512 else 8, Bc * T * n_mels, fn))
    # dense GEMM (a dense 513 x 128 bank) and bf16
    bankd = (torch.rand(513, 128, device=dev, generator=g) + 0.1)
    X = torch.complex(torch.randn(20_000, 513, device=dev, generator=g), torch.randn(20_000, 513, device=dev, generator=g))
    fn = gemm(X, bankd, "log1p", None, None)
    assert same_bits(launch(0, 20_000 * 128, fn), launch(1, 20_000 * 128, fn))
    img = ops.mel_bf16_pack_bank(bankd)
    x = torch.complex(torch.randn(40_000, 513, device=dev, generator=g), torch.randn(40_000, 513, device=dev, generator=g))
    fn = lambda out: ops.mel_forward_bf16(x, img, 513, 128, out=out.view(40_000, 128))     # noqa: E731
    assert same_bits(launch(0, 40_000 * 128, fn), launch(1, 40_000 * 128, fn))

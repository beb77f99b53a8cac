"""The n_fft-1024 inverse kernels with mirror pairs split in one lane (csrc/inv1024_pairs.h, fft512.h: irfft_split).

Lane L loads bins L + 64 m (m < 4) and (64 - L) + 64 m (m >= 4), splits the four pairs it holds, swaps registers 4..7
with lane (64 - L) & 63, and lane 0 takes bin 256 -- its own partner -- from one extra element.  A slip in that layout
moves or drops single bins, so the spectra here name them: one-hot spectra at the bins of lanes 0 and 32, the
self-paired bin 256 and the Nyquist bin, and a spectrum whose every bin and frame has its own value.  All against the
oracle at the project's 1e-5, for complex, polar and Griffin-Lim input, and the three kernel families -- long runs,
workgroup tiles (forced at small batch through the plan variant), frames -- against each other bit for bit.
"""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
from acids_transforms_amd import ops
from acids_transforms_amd._lib import VARIANTS, lib, variant
from conftest import rel_max
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
ONE_HOT_BINS = (0, 1, 63, 64, 255, 256, 257, 320, 448, 511, 512)
TILE_V = 6          # frames per wave of the forced tiles (tests/plan_cases.py: TILE_SWEEP has (6, 67))


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def _variants_back_to_default():
    yield
    assert all(lib().at_get_variant(w) == 0 for w in VARIANTS.values())


@pytest.fixture(scope="module")
def st(dev):
    return A.STFT().to(dev)


def long_runs(st, X=None, **kw):
    with variant("istft_runs", 1):
        return ops.istft(X, st.inv_window[:1024], 1024, 256, env16=st._env16, **kw)


def tiles(st, X=None, **kw):
    with variant("istft_tile", TILE_V):
        return ops.istft(X, st.inv_window[:1024], 1024, 256, env16=st._env16, **kw)


def frames_ref(X, w):
    """irfft of every frame times the synthesis window, float64 on the CPU"""
    return np.fft.irfft(cpu(X).astype(np.complex128), n=1024, axis=-1) * cpu(w).astype(np.float64)


def distinct_spectrum(B, T, dev):
    """Every bin of every frame of every clip its own value, real and imaginary part: i -> a i mod p is one-to-one
    below the prime p.  Scattered rather than a ramp over the bins, whose frames would be a spike at sample 0, where
    the synthesis window is zero -- a result a thousand times smaller than the transform's rounding error."""
    n, p = B * T * 513, 1048573
    assert n < p
    i = torch.arange(n, dtype=torch.int64)
    re = ((i * 613651) % p).to(torch.float64) / p - 0.5
    im = ((i * 274177) % p).to(torch.float64) / p - 0.5
    assert len(torch.unique(re.float())) == n and len(torch.unique(im.float())) == n
    return torch.complex(re, im).to(torch.complex64).view(B, T, 513).to(dev)


def one_hot(T, frame_of, dev):
    """clip b: bin ONE_HOT_BINS[b] of frame frame_of(b) set, everything else zero"""
    X = torch.zeros(len(ONE_HOT_BINS), T, 513, dtype=torch.complex64)
    for b, k in enumerate(ONE_HOT_BINS):
        X[b, frame_of(b), k] = 0.7 - 0.4j
    return X.to(dev)


def assert_clips_match(y, ref, what):
    assert y.shape == ref.shape, what
    for b in range(y.shape[0]):       # clip by clip: a wrong bin in one clip is not hidden by a louder one
        assert rel_max(y[b], ref[b]) < TOL, (what, b)


@pytest.mark.parametrize("T", [5, 67])
def test_one_hot_spectra(dev, st, T):
    w = st.inv_window[:1024]
    X = one_hot(T, (lambda b: b % T) if T == 5 else (lambda b: 30 + b), dev)
    ref = O.istft(X.cpu(), w.cpu(), 1024, 256).numpy()
    y = long_runs(st, X)
    assert_clips_match(cpu(y), ref, "long runs")
    fr = ops.irfft_frames(X, w, 1024)
    assert_clips_match(cpu(fr).reshape(len(ONE_HOT_BINS), -1), frames_ref(X, w).reshape(len(ONE_HOT_BINS), -1), "frames")
    mag, ph = X.abs().contiguous(), torch.angle(X).contiguous()
    yp = long_runs(st, mag=mag, phase=ph)
    assert_clips_match(cpu(yp), ref, "polar, long runs")
    if T >= 64:
        assert torch.equal(tiles(st, X), y)
        assert torch.equal(tiles(st, mag=mag, phase=ph), yp)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 4, 5, 67])
def test_distinct_spectrum_complex_and_polar(dev, st, T, B):
    w = st.inv_window[:1024]
    X = distinct_spectrum(B, T, dev)
    mag = X.abs().contiguous()
    ph = torch.angle(X).contiguous()
    y, yp = long_runs(st, X), long_runs(st, mag=mag, phase=ph)
    fr = ops.irfft_frames(X, w, 1024)
    frp = ops.irfft_frames(None, w, 1024, mag=mag, phase=ph)
    fref = frames_ref(X, w)
    assert rel_max(cpu(fr), fref) < TOL
    assert rel_max(cpu(frp), fref) < TOL
    if T == 1:                          # one frame: torch.istft's length is 0
        assert y.shape == yp.shape == (B, 0)
        return
    ref = O.istft(X.cpu(), w.cpu(), 1024, 256).numpy()
    assert_clips_match(cpu(y), ref, "complex")
    assert_clips_match(cpu(yp), O.polar_istft(mag.cpu(), ph.cpu(), w.cpu(), 1024, 256).numpy(), "polar")
    if T >= 64:
        assert torch.equal(tiles(st, X), y)
        assert torch.equal(tiles(st, mag=mag, phase=ph), yp)


@pytest.mark.parametrize("hop", [128, 512])
@pytest.mark.parametrize("T", [5, 67])
def test_distinct_spectrum_other_hops(dev, T, hop):
    """istft1024_ola_kernel at its other two hops"""
    mod = A.STFT(hop_length=hop).to(dev)
    w = mod.inv_window[:1024]
    X = distinct_spectrum(3, T, dev)
    with variant("istft_runs", 1):
        y = ops.istft(X, w, 1024, hop, env16=mod._env16)
    assert_clips_match(cpu(y), O.istft(X.cpu(), w.cpu(), 1024, hop).numpy(), hop)


@pytest.mark.parametrize("T", [4, 5, 67])
def test_distinct_spectrum_griffin_lim(dev, st, T):
    """the Griffin-Lim form (phase update at load time) against the update as its own kernel, then the oracle's inverse"""
    w, env = st.inv_window[:1024], st._env16
    rb = distinct_spectrum(3, T, dev)
    tp = torch.flip(rb, dims=(2,)).contiguous() * (0.3 + 0.2j)
    mag = (rb.abs() * 0.5 + 0.1).contiguous()
    one_hot_mag = torch.zeros_like(mag)
    for b, k in enumerate((0, 256, 512)):
        one_hot_mag[b, T // 2, k] = 1.0
    for m, name in ((mag, "distinct"), (one_hot_mag, "one hot")):
        for tprev in (None, tp):
            X = ops.griffinlim_update(m, rb, tprev, 0.99 / 1.99)
            y = ops.istft_griffinlim(m, rb, tprev, 0.99 / 1.99, w, 1024, 256, env)
            assert_clips_match(cpu(y), O.istft(X.cpu(), w.cpu(), 1024, 256).numpy(), (name, tprev is None))


def test_three_kernel_families_bit_for_bit(dev, st):
    """Long runs against tiles directly.  The frames kernel writes round(z w) and the overlap-add kernels
    fma(z, w, acc), so they meet where one frame alone is live: there acc = round(z w) exactly, the other frames add
    zeros, and a fully overlapped hop leaves as acc * (1 / envelope), both IEEE operations."""
    T, t0 = 67, 31
    w, env = st.inv_window[:1024], st._env16
    X = torch.zeros(3, T, 513, dtype=torch.complex64, device=dev)
    X[:, t0] = distinct_spectrum(3, 1, dev)[:, 0]
    mag, ph = X.abs().contiguous(), torch.angle(X).contiguous()
    for kw in (dict(X=X), dict(mag=mag, phase=ph)):
        y = long_runs(st, **kw)
        assert torch.equal(tiles(st, **kw), y)
        fr = cpu(ops.irfft_frames(kw.get("X"), w, 1024, mag=kw.get("mag"), phase=kw.get("phase")))[:, t0]       # (3, 1024)
        assert np.count_nonzero(fr) > 3000
        rcp = np.float32(1.0) / cpu(env)[15].astype(np.float32)                   # all four frames present
        want = (fr.reshape(3, 4, 256) * rcp[None, None, :]).reshape(3, 1024)
        # frame t0 covers padded samples 256 t0 .. 256 t0 + 1023; the centre trim is 512
        got = cpu(y)[:, 256 * t0 - 512:256 * t0 + 512]
        assert np.array_equal(got, want)
        rest = np.concatenate([cpu(y)[:, :256 * t0 - 512], cpu(y)[:, 256 * t0 + 512:]], axis=1)
        assert not rest.any()

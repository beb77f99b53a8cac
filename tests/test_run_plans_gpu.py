"""Every run and tile plan of the streaming STFT / ISTFT kernels, forced through the plan variants.

The launchers cut clips into per-wave runs (and, for full batches of the n_fft-1024 inverse, workgroup tiles) from the
batch size and the device's occupancy, so a test shape alone reaches one plan per box.  AT_VARIANT_RUN_LENGTH and
AT_VARIANT_ISTFT_TILE make the cut a test input: the sweeps of plan_cases.py (their geometry coverage is checked on the CPU
by test_plan_cases_cpu.py) run each kernel at short last runs, runs in the reflect-padded tail, last tiles of 1-3 frames,
waves of 0-2 frames, and hold the result bit for bit to one run per clip (README: bit-identical whatever batch a clip
rides in), with one oracle check per form.  The fused inverses at n_fft 512 / 2048 / 4096 get the same sweep with a
float64 oracle check per geometry class, their full-batch default plans are held to the forced 8-unit cut, and the
two-pass inverse of 2048 / 4096 runs at the hops no fused kernel takes."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import plan_cases as P
from acids_transforms_amd import ops
from acids_transforms_amd._lib import VARIANTS, check, lib, ptr, stream_ptr, variant
from acids_transforms_amd.utils.banded import BandedBank
from conftest import rel_max
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
B = P.BATCH      # 3 clips: where the stream's wrap frames fall in the runs depends on it (plan_cases.stream_classes)


def cpu(t):
    return t.detach().cpu().numpy()


def planned(v, fn):
    with variant("run_length", v):
        return fn()


def check_angle(ph, X, tol=1e-3):
    """phase against the oracle's angle where the bin is well above the noise."""
    X = np.asarray(X)
    big = np.abs(X) > 1e-3 * np.abs(X).max()
    d = np.angle(np.exp(1j * (np.asarray(ph) - np.angle(X))))
    assert np.abs(d[big]).max() < tol


@pytest.fixture(autouse=True)
def _variants_back_to_default():
    yield
    assert all(lib().at_get_variant(w) == 0 for w in VARIANTS.values())


# ---- tiled inverse -----------------------------------------------------------------------------------------------------
def test_tiled_inverse_every_tile_geometry(dev):
    """istft1024_tile_kernel at exactly v frames per wave (no balancing) against the long-run kernel, bit for bit, over
    TILE_SWEEP (last tiles of 1, 2, 3, >= 4 frames; clips ending in each wave; waves of 0-2 frames; a wave closing its
    own hops before a 1-2-frame successor; single tiles, >= 3 tiles); complex and polar input, STFT and DGT windows.
    One case per geometry class against the oracle."""
    g = torch.Generator(device=dev).manual_seed(1207)
    mods = (A.STFT().to(dev), A.DGT().to(dev))
    Tmax = max(T for _, T in P.TILE_SWEEP)
    Xall = torch.randn(B, Tmax, 513, 2, device=dev, generator=g)
    seen = set()
    for v, T in P.TILE_SWEEP:
        mod = mods[T % 2]
        w, env = mod.inv_window[:1024], mod._env16
        X = torch.view_as_complex(Xall[:, :T].contiguous())
        with variant("istft_tile", v):
            y_tile = ops.istft(X, w, 1024, 256, env16=env)
        with variant("istft_runs", 1):
            y_runs = ops.istft(X, w, 1024, 256, env16=env)
        assert y_tile.shape == (B, 256 * (T - 1))
        assert torch.equal(y_tile, y_runs), (v, T)
        mag = Xall[:, :T, :, 0].abs().contiguous()
        ph = (Xall[:, :T, :, 1] * 3e4).contiguous()
        with variant("istft_tile", v):
            p_tile = ops.istft(None, w, 1024, 256, env16=env, mag=mag, phase=ph)
        with variant("istft_runs", 1):
            p_runs = ops.istft(None, w, 1024, 256, env16=env, mag=mag, phase=ph)
        assert torch.equal(p_tile, p_runs), ("polar", v, T)
        new = P.tile_classes(T, v) - seen
        if new:
            seen |= new
            yr = O.istft(X.cpu(), w.cpu(), 1024, 256)
            assert rel_max(cpu(y_tile), yr.numpy()) < TOL, (v, T, sorted(new))
    assert P.TILE_CLASSES <= seen


# ---- long-run inverse --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [128, 256, 512])
def test_long_run_inverse_every_run_length(dev, hop):
    """istft1024_ola_kernel (complex, polar at the default hop) and its Griffin-Lim-fused form: every run length of
    INV_SWEEP is bit for bit the one-run-per-clip inverse; the oracle on the shortest and longest clip."""
    g = torch.Generator(device=dev).manual_seed(hop)
    st = A.STFT(hop_length=hop).to(dev)
    w, env = st.inv_window[:1024], st._env16
    Tmax = max(T for _, T in P.INV_SWEEP)
    Xall = torch.randn(B, Tmax, 513, 2, device=dev, generator=g)
    Rall = torch.randn(B, Tmax, 513, 2, device=dev, generator=g)
    Pall = torch.randn(B, Tmax, 513, 2, device=dev, generator=g)
    with variant("istft_runs", 1):                     # the long-run kernel at the default hop, whatever the batch
        for v, T in P.INV_SWEEP:
            X = torch.view_as_complex(Xall[:, :T].contiguous())
            ref = planned(P.ONE_RUN, lambda: ops.istft(X, w, 1024, hop, env16=env))
            assert torch.equal(planned(v, lambda: ops.istft(X, w, 1024, hop, env16=env)), ref), (v, T)
            if hop == 256:
                mag, ph = Xall[:, :T, :, 0].abs().contiguous(), (Xall[:, :T, :, 1] * 3e4).contiguous()
                pol = lambda: ops.istft(None, w, 1024, hop, env16=env, mag=mag, phase=ph)     # noqa: E731
                assert torch.equal(planned(v, pol), planned(P.ONE_RUN, pol)), ("polar", v, T)
            mag = X.abs().contiguous()
            rb = torch.view_as_complex(Rall[:, :T].contiguous())
            tp = torch.view_as_complex(Pall[:, :T].contiguous())
            for tprev in (None, tp):
                gl = lambda: ops.istft_griffinlim(mag, rb, tprev, 0.99 / 1.99, w, 1024, hop, env)   # noqa: E731
                assert torch.equal(planned(v, gl), planned(P.ONE_RUN, gl)), ("gl", v, T, tprev is None)
            if T in (2, Tmax) and v == 8:
                assert rel_max(cpu(ref), O.istft(X.cpu(), w.cpu(), 1024, hop).numpy()) < TOL
                want = ops.istft(ops.griffinlim_update(mag, rb, tp, 0.99 / 1.99), w, 1024, hop, env16=env)
                assert rel_max(cpu(planned(v, gl)), cpu(want)) < TOL


# ---- n_fft 1024 forward ------------------------------------------------------------------------------------------------
def _stft_unaligned(x, w, hop, T):
    """at_stft_forward into an output 8 bytes off a 512-byte boundary: the row-store form of the plain forward."""
    L = x.shape[1]
    buf = torch.empty(B * T * 513 + 1, dtype=torch.complex64, device=x.device)
    out = buf[1:].view(B, T, 513)
    check(lib().at_stft_forward(ptr(x), B, L, L, T, 1024, hop, 1, ptr(w), ptr(out), ptr(None), stream_ptr()),
          "at_stft_forward")
    return out


@pytest.mark.parametrize("hop", [128, 256, 512])
def test_forward_1024_every_run_length(dev, hop):
    """stft1024_h256_fwd_kernel, plain (row and aligned stores) and with the phase side output: every run length of the
    sweep -- last runs of 1-7 frames, runs inside the reflect-padded tail, T < 8 -- is bit for bit one run per clip."""
    g = torch.Generator(device=dev).manual_seed(10 + hop)
    w = torch.hann_window(1024, device=dev)
    sweep = P.FWD_SWEEPS[(1024, hop)]
    xall = torch.randn(B, max(L for _, _, L in sweep), device=dev, generator=g) * 0.1
    checked = False
    for v, T, L in sweep:
        x = xall[:, :L].contiguous()

        def with_phase():
            X, ph = ops.stft_forward(x, w, 1024, hop, want_phase=True)
            return torch.cat([torch.view_as_real(X).flatten(), ph.flatten()])
        forms = {"plain": lambda: ops.stft_forward(x, w, 1024, hop), "phase": with_phase}
        if hop == 256:
            forms["rows"] = lambda: _stft_unaligned(x, w, hop, T)
        for name, fn in forms.items():
            assert torch.equal(planned(v, fn), planned(P.ONE_RUN, fn)), (name, v, T, L)
        if not checked and T >= 20:
            checked = True
            Xr = O.stft_forward(x.cpu(), w.cpu(), 1024, hop)
            X, ph = planned(v, lambda: ops.stft_forward(x, w, 1024, hop, want_phase=True))
            assert rel_max(cpu(X), Xr.numpy()) < TOL
            check_angle(cpu(ph), Xr.numpy())
            assert rel_max(cpu(planned(v, forms["plain"])), Xr.numpy()) < TOL
            if hop == 256:
                assert rel_max(cpu(planned(v, forms["rows"])), Xr.numpy()) < TOL
    assert checked


def _contrast(m, mode, eps=1.1920929e-07):
    return O.contrast(m, mode, eps)


FUSED_FORMS = [
    # name, n_mels (None: the 513-filter default bank), contrast, power, channel_major, want_spectrum, variants
    ("mel128_fixed", 128, "log1p", 1, False, True, ()),
    ("mel128_fixed_features", 128, "log1p", 1, False, False, ()),
    ("mel128_generic", 128, "log1p", 1, False, True, (("epilogue", 1),)),
    ("mfcc_channel_major", 128, None, 2, True, False, ()),
    ("config3_logmel", 128, "log", 2, False, False, ()),
    ("default_bank_features", None, "log1p", 1, False, False, ()),
]


@pytest.mark.parametrize("form", FUSED_FORMS, ids=[f[0] for f in FUSED_FORMS])
def test_fused_forward_every_run_length(dev, form):
    """The fused forward (framing + FFT + banded epilogue) in each of its kernels: spectrum and features bit for bit
    one run per clip over FUSED_SWEEP, and against the oracle once."""
    name, n_mels, contrast, power, cm, spec, variants = form
    g = torch.Generator(device=dev).manual_seed(len(name))
    mg = A.Magnitude(n_mels=n_mels) if n_mels else A.Magnitude()
    bank = mg.mel_bank.reshape(513, -1)
    band = BandedBank(bank)
    w = torch.hann_window(1024, device=dev)
    xall = torch.randn(B, max(L for _, _, L in P.FUSED_SWEEP), device=dev, generator=g) * 0.1
    ctx = [variant(*kv) for kv in variants]
    for c in ctx:
        c.__enter__()
    try:
        checked = False
        for v, T, L in P.FUSED_SWEEP:
            x = xall[:, :L].contiguous()

            def fn():
                return ops.stft_mel_forward(x, w, band, contrast, power=power, want_spectrum=spec, channel_major=cm)
            Xa, _, fa = planned(v, fn)
            Xb, _, fb = planned(P.ONE_RUN, fn)
            assert torch.equal(fa, fb), (name, v, T, L)
            if spec:
                assert torch.equal(Xa, Xb), (name, v, T, L)
            if not checked and T >= 16:
                checked = True
                Xr = O.stft_forward(x.cpu().double(), w.cpu().double(), 1024, 256)
                fr = _contrast(Xr.abs() ** power @ bank.double(), contrast)
                if cm:
                    fr = fr.transpose(-2, -1)
                assert rel_max(cpu(fa), fr.numpy()) < TOL
                if spec:
                    assert rel_max(cpu(Xa), Xr.numpy()) < TOL
        assert checked
    finally:
        for c in reversed(ctx):
            c.__exit__(None, None, None)


@pytest.mark.parametrize("hop", [128, 512])
def test_fused_forward_other_hops_every_run_length(dev, hop):
    """The fused 128-mel forward at hops 128 / 512 (its own sliding-window kernels)."""
    g = torch.Generator(device=dev).manual_seed(hop + 1)
    bank = A.Magnitude(n_mels=128).mel_bank.reshape(513, -1)
    band = BandedBank(bank)
    w = torch.hann_window(1024, device=dev)
    sweep = P.fwd_sweep(1024, hop, v_list=(8, 11), T_list=list(range(3, 21)))
    xall = torch.randn(B, max(L for _, _, L in sweep), device=dev, generator=g) * 0.1
    for v, T, L in sweep:
        x = xall[:, :L].contiguous()
        for spec in (True, False):
            fn = lambda: ops.stft_mel_forward(x, w, band, "log1p", want_spectrum=spec, hop=hop)   # noqa: E731
            Xa, _, fa = planned(v, fn)
            Xb, _, fb = planned(P.ONE_RUN, fn)
            assert torch.equal(fa, fb) and (not spec or torch.equal(Xa, Xb)), (spec, v, T, L)
    Xr = O.stft_forward(x.cpu().double(), w.cpu().double(), 1024, hop)
    assert rel_max(cpu(fa), _contrast(Xr.abs() @ bank.double(), "log1p").numpy()) < TOL


def test_polar_forward_every_run_length(dev):
    """Compose(STFT -> Polar) in one kernel: magnitude and angle halves bit for bit one run per clip."""
    g = torch.Generator(device=dev).manual_seed(5)
    bank = A.Magnitude().mel_bank.reshape(513, -1)
    band = BandedBank(bank)
    w = torch.hann_window(1024, device=dev)
    xall = torch.randn(B, max(L for _, _, L in P.FUSED_SWEEP), device=dev, generator=g) * 0.1
    for v, T, L in P.FUSED_SWEEP:
        x = xall[:, :L].contiguous()
        fn = lambda: ops.stft_polar_forward(x, w, band, "log1p")   # noqa: E731
        out = planned(v, fn)
        assert torch.equal(out, planned(P.ONE_RUN, fn)), (v, T, L)
    Xr = O.stft_forward(x.cpu().double(), w.cpu().double(), 1024, 256)
    assert rel_max(cpu(out[:, :, 0]), _contrast(Xr.abs() @ bank.double(), "log1p").numpy()) < TOL
    check_angle(cpu(out[:, :, 1]), Xr.numpy())


# ---- sliding-window forwards at n_fft 512 / 2048 / 4096 ----------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", [(512, 128), (2048, 512), (4096, 1024)])
def test_sliding_forward_every_run_length(dev, n_fft, hop):
    """stft512_run_fwd_kernel (runs of frame pairs, a half pair at odd T), stft2048_run_fwd_kernel and
    stft4096_run_fwd_kernel: every run length of the sweep bit for bit one run per clip; the oracle at 1e-5 on the
    longest clip and on a short one."""
    g = torch.Generator(device=dev).manual_seed(n_fft)
    w = torch.hann_window(n_fft, device=dev)
    sweep = P.FWD_SWEEPS[(n_fft, hop)]
    xall = torch.randn(B, max(L for _, _, L in sweep), device=dev, generator=g) * 0.1
    for v, T, L in sweep:
        x = xall[:, :L].contiguous()
        fn = lambda: ops.stft_forward(x, w, n_fft, hop)   # noqa: E731
        X = planned(v, fn)
        assert X.shape == (B, T, n_fft // 2 + 1)
        assert torch.equal(X, planned(P.ONE_RUN, fn)), (v, T, L)
        if (v, T, L) in (sweep[0], sweep[-1]) or (T % 2 == 1 and v == 8 and 9 <= T <= 10):
            assert rel_max(cpu(X), O.stft_forward(x.cpu(), w.cpu(), n_fft, hop).numpy()) < TOL, (v, T, L)


def test_512_half_pair_starting_a_run(dev):
    """Found by the sweep above: at odd T the last frame pair of stft512_run_fwd_kernel is half a pair, and the two frames
    of a pair share one complex FFT.  A run that STARTED at the half pair zeroed the missing frame where the steady state
    carries half a window into it, so the last frame's bits (not its accuracy) depended on the run cut."""
    g = torch.Generator(device=dev).manual_seed(17)
    w = torch.hann_window(512, device=dev)
    for T, L in ((17, 2052), (33, 4100), (49, 6148)):
        x = torch.randn(B, L, device=dev, generator=g) * 0.1
        fn = lambda: ops.stft_forward(x, w, 512, 128)   # noqa: E731
        X = planned(8, fn)                             # the last run is the half pair alone
        last = P.runs((T + 1) // 2, 8)[-1]
        assert last[1] - last[0] == 1 and T % 2 == 1 and T == 1 + L // 128
        assert torch.equal(X, planned(P.ONE_RUN, fn)), (T, L)
        assert rel_max(cpu(X), O.stft_forward(x.cpu(), w.cpu(), 512, 128).numpy()) < TOL


# ---- fused inverses at n_fft 512 / 2048 / 4096 --------------------------------------------------------------------------
def _inverse_windows(n_fft, hop, dev):
    """[(name, synthesis window, envelope table)] of STFT (Hann) and DGT (dual of the Gaussian)."""
    out = []
    for cls in (A.STFT, A.DGT):
        m = cls(n_fft=n_fft, hop_length=hop).to(dev)
        out.append((cls.__name__, m.inv_window[:n_fft], m._env16 if m._env16.numel() else None))
    return out


@pytest.mark.parametrize("n_fft,hop", P.INV_OTHER)
def test_fused_inverse_512_2048_4096_every_run_length(dev, n_fft, hop):
    """istft512_ola_kernel (runs of frame pairs), istft2048_ola_kernel and istft4096_ola_kernel (runs of output hops) at
    hop n/8, n/4, n/2, complex and polar input (phases of about 3e4 rad: the big-argument reduction), STFT and DGT
    windows: every cut of INV_OTHER_SWEEPS -- single runs, last runs of 1-7 units, runs that hold only the clip's partially
    overlapped trailing hops, clips of at most R frames, a run that starts at the final half pair -- is bit for bit one run
    per clip.  Two cuts can share a fault, so the first cut that reaches each geometry class is also held to torch.istft in
    float64: complex input at 1e-5, polar input (|X|, angle X) at 2e-5."""
    g = torch.Generator(device=dev).manual_seed(n_fft + hop)
    F = n_fft // 2 + 1
    sweep = P.INV_OTHER_SWEEPS[(n_fft, hop)]
    Xall = torch.randn(B, max(T for _, T in sweep), F, 2, device=dev, generator=g)
    windows = _inverse_windows(n_fft, hop, dev)
    seen = {name: set() for name, _, _ in windows}
    for T in sorted({T for _, T in sweep}):
        X = torch.view_as_complex(Xall[:, :T].contiguous())
        mag, ph = Xall[:, :T, :, 0].abs().contiguous(), (Xall[:, :T, :, 1] * 3e4).contiguous()
        amag, aph = X.abs(), X.angle()
        for name, w, env in windows:
            assert env is not None
            cplx = lambda: ops.istft(X, w, n_fft, hop, env16=env)                            # noqa: E731
            polar = lambda: ops.istft(None, w, n_fft, hop, env16=env, mag=mag, phase=ph)     # noqa: E731
            one_c, one_p = planned(P.ONE_RUN, cplx), planned(P.ONE_RUN, polar)
            assert one_c.shape == (B, hop * (T - 1))
            yr = None
            for v in [v for v, t in sweep if t == T]:
                yc = planned(v, cplx)
                assert torch.equal(yc, one_c), (name, v, T)
                assert torch.equal(planned(v, polar), one_p), (name, "polar", v, T)
                new = P.inv_classes(n_fft, hop, v, T) - seen[name]
                if new:
                    seen[name] |= new
                    if yr is None:
                        yr = O.istft(X.cpu().to(torch.complex128), w.cpu().double(), n_fft, hop).numpy()
                    e_c = rel_max(cpu(yc), yr)
                    e_p = rel_max(cpu(planned(v, lambda: ops.istft(None, w, n_fft, hop, env16=env, mag=amag, phase=aph))), yr)
                    print("inverse %d/%d %s v=%d T=%d %s: complex %.3g polar %.3g" % (n_fft, hop, name, v, T, sorted(new), e_c, e_p))
                    assert e_c < TOL, (name, v, T, sorted(new), e_c)
                    assert e_p < 2e-5, (name, "polar", v, T, sorted(new), e_p)
    assert all(P.inv_want_classes(n_fft, hop) <= s for s in seen.values())


@pytest.mark.parametrize("case", [0, 1], ids=["1024_clips", "one_run_per_clip"])
@pytest.mark.parametrize("n_fft", [512, 2048, 4096])
def test_fused_inverse_512_2048_4096_full_batch(dev, n_fft, case):
    """The plans that ship, at hop n/4: 1024 clips of 4 s (what bench.py times under other_sizes: two runs of 172 / 86
    hops per clip at 2048 / 4096, four runs of 173 frame pairs at 512) and the smallest batch that gets one run per clip.
    The whole output is bit for bit the forced 8-unit cut of the same input; clips {0, B/2 - 1, B - 1} against torch.istft in
    float64 at 1e-5, and each of them alone (a single clip is cut at the launcher's floor) bit for bit the clip inside the
    batch -- STFT and DGT windows."""
    Bf, L = P.INV_FULL_BATCH[n_fft][case]
    hop = n_fft // 4
    g = torch.Generator(device=dev).manual_seed(n_fft + case)
    x = torch.randn(Bf, L, device=dev, generator=g) * 0.1
    X = A.STFT(n_fft=n_fft, hop_length=hop).to(dev)(x)
    del x
    T = X.shape[1]
    assert T == 1 + L // hop
    units, per, nruns = P.default_inverse_plan(n_fft, hop, Bf, T)
    assert nruns == (1 if case else 4 if n_fft == 512 else 2) and (case or per > 64)
    ids = [0, Bf // 2 - 1, Bf - 1]
    Xi = X[ids].contiguous()
    for name, w, env in _inverse_windows(n_fft, hop, dev):
        y = ops.istft(X, w, n_fft, hop, env16=env)
        assert y.shape == (Bf, hop * (T - 1))
        assert torch.equal(y, planned(8, lambda: ops.istft(X, w, n_fft, hop, env16=env))), name
        err = rel_max(cpu(y[ids]), O.istft(Xi.cpu().to(torch.complex128), w.cpu().double(), n_fft, hop).numpy())
        print("inverse %d/%d B=%d %s: runs of %d x %d, oracle %.3g" % (n_fft, hop, Bf, name, nruns, per, err))
        assert err < TOL, (name, err)
        for j, k in enumerate(ids):
            assert torch.equal(ops.istft(Xi[j:j + 1], w, n_fft, hop, env16=env)[0], y[k]), (name, k)
        del y


@pytest.mark.parametrize("n_fft,hop", P.TWO_PASS_HOPS)
def test_two_pass_inverse_2048_4096(dev, n_fft, hop):
    """irfft2048_frames_kernel / irfft4096_frames_kernel + the overlap-add gather as an istft: hop n/16 (STFT and DGT)
    and hops that do not divide n_fft (STFT), complex at 1e-5 and polar at 2e-5 against torch.istft in float64.  Then a
    launch of more than 8192 frames, where a workgroup's waves take more than one frame each: three clips against the
    oracle, and every clip bit for bit what launches of three clips give."""
    g = torch.Generator(device=dev).manual_seed(n_fft + hop)
    for cls in ((A.STFT, A.DGT) if n_fft % hop == 0 else (A.STFT,)):
        m = cls(n_fft=n_fft, hop_length=hop).to(dev)
        assert m._env16.numel() == 0                       # no fused kernel for this hop
        w = m.inv_window[:n_fft].cpu().double()
        for Bs, T in ((3, 41), (24, 401)):
            x = torch.randn(Bs, hop * (T - 1) + 17, device=dev, generator=g) * 0.1
            X = m(x)
            assert X.shape == (Bs, T, n_fft // 2 + 1)
            assert (P.frames_per_block_2k_4k(Bs * T) > 4) == (Bs == 24)
            y = m.invert(X)
            assert y.shape == (Bs, hop * (T - 1))
            ids = [0, Bs // 2, Bs - 1]
            yr = O.istft(X[ids].cpu().to(torch.complex128), w, n_fft, hop).numpy()
            e_c = rel_max(cpu(y[ids]), yr)
            e_p = rel_max(cpu(m._istft(mag=X.abs(), phase=X.angle())[ids]), yr)
            print("two-pass %d/%d %s B=%d T=%d: complex %.3g polar %.3g" % (n_fft, hop, cls.__name__, Bs, T, e_c, e_p))
            assert e_c < TOL and e_p < 2e-5, (cls.__name__, Bs, T, e_c, e_p)
            if Bs == 24:
                small = torch.cat([m.invert(X[k:k + 3].contiguous()) for k in range(0, Bs, 3)])
                assert torch.equal(y, small), cls.__name__

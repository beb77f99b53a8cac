"""GPU parity: PGHI (offline and realtime) through the C ABI.

PGHI parity is defined as in SURVEY.md hard part 2: (i) identical visited mask,
(ii) identical heap pop order (bit exact: it depends only on magnitude compares
and the heap's tie-breaking), (iii) phase within 1e-3 + 8 ulp(|phase_ref|)
(+ a small relative slack for the device's logf), (iv) resynthesised audio by
SNR against the reference's own PGHI audio."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
from acids_transforms_amd import ops
from conftest import rel_max
from acids_transforms_amd._lib import variant
from oracle import oracle as O

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy

CASES = ["n12x17", "t12x17", "s12x17", "n40x65", "t40x65", "d40x65", "s40x65", "n64x257", "d64x257",
         "const6x17", "one1x17", "zero5x17"]


def cpu(t):
    return t.detach().cpu().numpy()


def phase_tol(ref, base=1e-3, ulps=8, rel=1e-5):
    ref = np.asarray(ref, np.float32)
    return base + ulps * np.spacing(np.abs(ref)) + rel * np.abs(ref)


@pytest.mark.parametrize("case", CASES)
def test_offline_golden_exact_order(golden, dev, case):
    g = golden("g4_pghi_offline")
    n_fft, hop, tol = g[case + "_params"]
    d = A.DGT(n_fft=int(n_fft), hop_length=int(hop), tolerance=float(tol)).to(dev)
    mag = T_(g[case + "_mag"]).to(dev)
    tg, fg = d.modgabphasegrad(torch.clamp(mag, float(d.eps)))
    assert np.allclose(cpu(tg), g[case + "_tgradw"], rtol=0, atol=3e-5)
    assert np.allclose(cpu(fg), g[case + "_fgradw"], rtol=1e-5, atol=3e-4)
    phase, npops, order = ops.pghi_offline(mag.unsqueeze(0), float(d.gamma), int(n_fft), int(hop),
                                           float(d.tolerance), float(d.eps), debug=True)
    ref_order = g[case + "_order"]
    F = mag.shape[1]
    assert int(npops[0]) == len(ref_order)
    got = cpu(order[0][:len(ref_order)])
    assert np.array_equal(got, ref_order[:, 0] * F + ref_order[:, 1])      # (ii) bit-exact pop order
    ref = g[case + "_phase"]
    ph = cpu(phase[0])
    assert np.array_equal(ph == 0, ref == 0)                                # (i) visited mask
    assert np.all(np.abs(ph - ref) <= phase_tol(ref))                       # (iii)
    assert np.array_equal(cpu(mag), g[case + "_mag"])                       # caller's tensor untouched
    assert np.array_equal(cpu(d.pghi(mag, d.tolerance)), ph)                             # module entry point, 2-D input
    # perform_hgi on its own, fed the REFERENCE's gradients (dgt.py:168-220): same pops, the reference's phases
    mc = torch.clamp(mag, float(d.eps))
    ph2, np2, or2 = ops.pghi_integrate(mc.unsqueeze(0), T_(g[case + "_tgradw"]).to(dev).unsqueeze(0),
                                       T_(g[case + "_fgradw"]).to(dev).unsqueeze(0), float(d.tolerance), float(d.eps), debug=True)
    assert int(np2[0]) == len(ref_order) and np.array_equal(cpu(or2[0][:len(ref_order)]), got)
    assert np.all(np.abs(cpu(ph2[0]) - ref) <= phase_tol(ref))


def test_offline_batch_matches_per_clip_oracle(dev):
    # ragged content in one launch: noise, tonal, silence, a single spike
    g = torch.Generator().manual_seed(3)
    T, F = 23, 65
    mags = torch.stack([
        (torch.randn(T, F, generator=g) ** 2 + torch.randn(T, F, generator=g) ** 2).sqrt(),
        torch.rand(T, F, generator=g) * 1e-4 + torch.eye(T, F) * 3.0,
        torch.zeros(T, F),
        torch.zeros(T, F),
    ])
    mags[3, 7, 9] = 2.0
    d = A.DGT(n_fft=128, hop_length=32).to(dev)
    ph, npops, order = ops.pghi_offline(mags.to(dev), float(d.gamma), 128, 32, float(d.tolerance), float(d.eps), debug=True)
    for b in range(4):
        r = O.pghi_offline(mags[b], 128, 32, want_order=True)
        k = len(r["order"])
        assert int(npops[b]) == k
        assert np.array_equal(cpu(order[b][:k]), r["order"][:, 0] * F + r["order"][:, 1])
        assert np.all(np.abs(cpu(ph[b]) - r["phase"]) <= phase_tol(r["phase"]))


@pytest.mark.parametrize("n,h", [(400, 100), (441, 110), (1000, 250), (254, 64)])
def test_offline_sizes_that_are_not_powers_of_two(dev, n, h):
    """DGT(n_fft not a power of two): the heap integration follows the oracle pop for pop (the phase-gradient
    constants depend on n_fft and hop only), and `invert(|X|, "pghi")` runs end to end on the mixed-radix kernels."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2, 12 * n, generator=g) * 0.1
    d = A.DGT(n_fft=n, hop_length=h).to(dev)
    mags = d(x.to(dev)).abs()
    F = n // 2 + 1
    assert mags.shape[-1] == F
    ph, npops, order = ops.pghi_offline(mags, float(d.gamma), n, h, float(d.tolerance), float(d.eps), debug=True)
    for b in range(2):
        r = O.pghi_offline(mags[b].cpu(), n, h, want_order=True)
        k = len(r["order"])
        assert int(npops[b]) == k
        assert np.array_equal(cpu(order[b][:k]), r["order"][:, 0] * F + r["order"][:, 1])
        assert np.all(np.abs(cpu(ph[b]) - r["phase"]) <= phase_tol(r["phase"]))
    y = d.invert(mags, inversion_mode="pghi")
    yr = O.polar_istft(mags.cpu(), torch.from_numpy(cpu(ph)), d.inv_window[:n].cpu(), n, h)
    assert y.shape == yr.shape and rel_max(cpu(y), yr.numpy()) < 1e-4


def test_offline_invert_end_to_end_golden(golden, dev):
    g = golden("g4_pghi_invert")
    d = A.DGT(n_fft=128, hop_length=32).to(dev)
    y = cpu(d.invert(T_(g["mag"]).to(dev), inversion_mode="pghi"))
    ref = g["y"]
    assert y.shape == ref.shape
    snr = 10 * np.log10((ref ** 2).sum() / max(((y - ref) ** 2).sum(), 1e-30))
    assert snr > 40.0, snr                                                  # (iv)


def test_offline_real_audio_golden(golden, dev):
    g = golden("g10_agogo")
    d = A.DGT().to(dev)
    x = T_(g["x"]).to(dev)
    X = d(x)
    # (iii) on the reference's own magnitudes (a round trip through the GPU DGT may flip near-ties)
    ph = cpu(d.pghi(T_(g["mag_dgt"]).to(dev), d.tolerance))
    ref = g["phase_pghi"]
    assert np.array_equal(ph == 0, ref == 0)
    assert np.all(np.abs(ph - ref) <= phase_tol(ref, base=5e-3, ulps=16))
    y = cpu(d.invert(T_(g["mag_dgt"]).to(dev), inversion_mode="pghi"))
    snr = 10 * np.log10((g["y_pghi"] ** 2).sum() / max(((y - g["y_pghi"]) ** 2).sum(), 1e-30))
    assert snr > 40.0, snr
    # and the README chain end to end on device: DGT -> |.| -> PGHI invert gives a faithful resynthesis
    y2 = d.invert(X.abs(), inversion_mode="pghi")
    assert y2.shape == (22016,)


@pytest.mark.parametrize("tag", ["k1", "k2", "k3"])
def test_realtime_kernel_golden(golden, dev, tag):
    g = golden("g5_rtpghi_kernel")
    n, h = [int(v) for v in g[tag + "_params"]]
    rt = A.RealtimeDGT(n_fft=n, hop_length=h, batch_size=[3]).to(dev)
    rt.hgi_mag_buffer = T_(g[tag + "_magbuf"]).to(dev)
    rt.hgi_phase_buffer = T_(g[tag + "_phasebuf"]).to(dev)
    mag = T_(g[tag + "_mag"]).to(dev)
    ph, tg, fg = ops.pghi_realtime(rt.hgi_mag_buffer, mag, rt.hgi_phase_buffer, T_(g[tag + "_noise"]).to(dev),
                                   float(rt.gamma), n, h, float(rt.tolerance), float(rt.eps), debug=True)
    assert np.allclose(cpu(tg), g[tag + "_tgradw"], rtol=1e-5, atol=5e-5)
    assert np.allclose(cpu(fg), g[tag + "_fgradw"], rtol=1e-5, atol=3e-3)
    ref = g[tag + "_phase"]
    assert np.all(np.abs(cpu(ph) - ref) <= phase_tol(ref, base=2e-3, ulps=16))
    # module entry point with explicit noise
    ph2 = rt.pghi(mag, rt.tolerance, noise=T_(g[tag + "_noise"]).to(dev))
    assert np.array_equal(cpu(ph2), cpu(ph))


@pytest.mark.parametrize("tag", ["a", "c"])
def test_realtime_stream_golden(golden, dev, tag):
    """chunked stream: OverlapAdd frames -> RealtimeDGT -> |.| -> RTPGHI invert; buffers carried chunk to chunk."""
    g = golden("g5_rtpghi")
    n, h, chunk, nchunks = [int(v) for v in g[tag + "_params"]]
    rt = A.RealtimeDGT(n_fft=n, hop_length=h, batch_size=[2]).to(dev)
    for c in range(nchunks):
        mag = T_(g["%s_mag_%d" % (tag, c)]).to(dev)
        noise = T_(g["%s_noise_%d" % (tag, c)]).to(dev)
        if list(mag.shape[:-2]) != list(rt.hgi_mag_buffer.shape[:-2]):
            rt.reset(mag.shape[:-2])
        ph = rt.pghi(mag, rt.tolerance, noise=noise)
        frames, rt.hgi_mag_buffer, rt.hgi_phase_buffer = ops.rt_polar_irfft_update(
            mag, ph, rt.inv_window[:n], n, rt.hgi_mag_buffer)
        ref = g["%s_yframes_%d" % (tag, c)]
        y = cpu(frames)
        snr = 10 * np.log10((ref ** 2).sum() / max(((y - ref) ** 2).sum(), 1e-30))
        assert snr > 40.0, (c, snr)
        assert np.allclose(cpu(rt.hgi_mag_buffer), g["%s_magbuf_%d" % (tag, c)], rtol=1e-5, atol=1e-6)
        dphi = np.angle(np.exp(1j * (cpu(rt.hgi_phase_buffer) - g["%s_phasebuf_%d" % (tag, c)])))
        big = g["%s_magbuf_%d" % (tag, c)][:, 1] > 1e-3 * g["%s_magbuf_%d" % (tag, c)].max()
        assert np.abs(dphi[big]).max() < 5e-2, c
        # keep the stream on the reference's trajectory for the next chunk
        rt.hgi_mag_buffer = T_(g["%s_magbuf_%d" % (tag, c)]).to(dev)
        rt.hgi_phase_buffer = T_(g["%s_phasebuf_%d" % (tag, c)]).to(dev)


def test_realtime_module_invert_runs(dev):
    torch.manual_seed(0)
    rt = A.RealtimeDGT(batch_size=4).to(dev)
    fr = torch.randn(4, 6, 1024, device=dev)
    X = rt(fr)
    y = rt.invert(X.abs(), inversion_mode="pghi")
    assert y.shape == (4, 6, 1024) and bool(torch.isfinite(y).all())
    assert rt.hgi_mag_buffer.shape == (4, 2, 513) and rt.hgi_phase_buffer.shape == (4, 513)
    y1 = rt.invert(X.abs()[:, :1], inversion_mode="pghi")      # single-frame step keeps one history frame
    assert y1.shape == (4, 1, 1024)


def test_offline_full_size_properties(dev):
    """One 4-s clip at the BASELINE size: every bin above tol*max is visited exactly once,
    below-threshold bins keep phase exactly 0, result independent of batch position."""
    torch.manual_seed(4)
    d = A.DGT().to(dev)
    x = torch.randn(2, 176400, device=dev) * 0.1
    mag = d(x).abs()
    mag = torch.cat([mag, mag[:1]])                    # clip 2 == clip 0
    ph, npops, _ = ops.pghi_offline(mag, float(d.gamma), 1024, 256, float(d.tolerance), float(d.eps), debug=True)
    live = mag > (mag.amax(dim=(1, 2), keepdim=True) * d.tolerance)
    assert torch.equal(npops.cpu(), live.flatten(1).sum(1).cpu() + 0) or bool((npops.cpu() - live.flatten(1).sum(1).cpu()).abs().max() <= 1)
    assert bool((ph[~live] == 0).all())
    assert torch.equal(ph[0], ph[2])
    # exact pop order at full size as well: here the heap outgrows its LDS share, so the global part of the
    # array and the deep bubble rounds are on the checked path (the C oracle needs ~30 ms for such a clip)
    _, npops1, order1 = ops.pghi_offline(mag[1:2], float(d.gamma), 1024, 256, float(d.tolerance), float(d.eps), debug=True)
    r = O.pghi_offline(mag[1].cpu(), 1024, 256, want_order=True)
    k = len(r["order"])
    assert int(npops1[0]) == k
    assert np.array_equal(order1[0][:k].cpu().numpy(), r["order"][:, 0] * 513 + r["order"][:, 1])


@pytest.mark.parametrize("kind", ["decaying", "bursts"])
def test_offline_many_reseeds_exact_order(dev, kind):
    """Sounds that decay (or come in separate bursts) empty the heap hundreds of times; every reseed takes the global
    maximum of what is left (dgt.py:216-219).  The kernel finds it through per-segment upper bounds instead of
    rescanning the clip -- the pop order must still be the C oracle's, pop for pop."""
    rng = np.random.RandomState(5 if kind == "decaying" else 6)
    T, F = 150, 513
    m = np.abs(rng.randn(2, T, F) + 1j * rng.randn(2, T, F)).astype(np.float32)
    if kind == "decaying":
        m *= np.exp(-np.arange(T, dtype=np.float32) / 12.0)[None, :, None]
    else:
        gate = (rng.rand(2, T, 1) < 0.25) * (rng.rand(2, 1, F) < 0.5)
        m = m * gate + 1e-7
        m[1] = np.round(m[1] * 8) / 8 + 1e-7                    # ties across bursts: first row-major index wins
    d = A.DGT().to(dev)
    mag = T_(m).to(dev)
    ph, npops, order = ops.pghi_offline(mag, float(d.gamma), 1024, 256, float(d.tolerance), float(d.eps), debug=True)
    for b in range(2):
        r = O.pghi_offline(m[b], 1024, 256, want_order=True)
        k = len(r["order"])
        assert int(npops[b]) == k and k > 1000
        assert np.array_equal(cpu(order[b][:k]), r["order"][:, 0] * F + r["order"][:, 1])
        seeds = int(((r["phase"] == 0) & (m[b] >= 1e-2 * m[b].max())).sum())
        assert seeds > 20, seeds                                   # the case does reseed many times
        assert np.all(np.abs(cpu(ph[b]) - r["phase"]) <= phase_tol(r["phase"]))


def test_realtime_seeded_draws_are_standard_normal(dev):
    """at_pghi_realtime_seeded: the phases of the bins at or below the tolerance are standard-normal draws made on the
    device (dgt.py:404-405 draws them with torch.randn_like: statistical parity) -- mean, variance, kurtosis, tails;
    a new counter every call; same state, same draws."""
    S, n, F = 64, 4, 513
    mag = torch.full((S, n, F), 1e-6, device=dev)
    mag[:, :, 100] = 1.0                                   # tolerance 1e-2: every other bin is below it
    hist = torch.full((S, 2, F), 1e-6, device=dev)
    prev = torch.zeros(S, F, device=dev)
    d = A.RealtimeDGT(batch_size=[S]).to(dev)
    args = (float(d.gamma), 1024, 256, float(d.tolerance), float(d.eps))
    st = torch.tensor([12345, -6789, 0, 0], dtype=torch.int32, device=dev)
    a = ops.pghi_realtime_seeded(hist, mag, prev, st, *args)
    assert int(st[2]) == 1
    b = ops.pghi_realtime_seeded(hist, mag, prev, st, *args)
    assert int(st[2]) == 2
    keep = torch.ones(F, dtype=torch.bool, device=dev)
    keep[100] = False
    xa, xb = a[:, :, keep].flatten().double(), b[:, :, keep].flatten().double()
    N = xa.numel()
    assert N == S * n * 512
    for x in (xa, xb):
        assert abs(float(x.mean())) < 6 / N ** 0.5
        assert abs(float(x.var()) - 1.0) < 0.02
        assert abs(float((x ** 4).mean()) - 3.0) < 0.15
        assert float(x.abs().max()) < 6.0 and float((x.abs() > 3).double().mean()) < 0.005
    assert abs(float((xa * xb).mean())) < 6 / N ** 0.5      # consecutive steps are uncorrelated
    st2 = torch.tensor([12345, -6789, 0, 0], dtype=torch.int32, device=dev)
    assert torch.equal(ops.pghi_realtime_seeded(hist, mag, prev, st2, *args), a)        # same state, same draws
    st3 = torch.tensor([1, 2, 0, 0], dtype=torch.int32, device=dev)
    assert not torch.equal(ops.pghi_realtime_seeded(hist, mag, prev, st3, *args), a)    # another seed, other draws
    # with explicit noise the two entry points agree bit for bit on everything above the tolerance
    ref = ops.pghi_realtime(hist, mag, prev, torch.zeros_like(mag), *args)
    assert torch.equal(ref[:, :, 100], a[:, :, 100])


def test_winner_bit_kernel_stays_exact(dev):
    """The opt-in winner-bit heap kernel (at_set_variant(AT_VARIANT_PGHI_KERNEL, 1); the fuzz tool sets it from
    FUZZ_PGHI_KERNEL) must keep producing the C oracle's pop order: ties, sparse spectra, batches of unequal clips."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FUZZ_PGHI_KERNEL="1", FUZZ_CASES="24", FUZZ_SEED="3")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_pghi.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "24 cases ok" in r.stdout and "identical order" in r.stdout


def test_perform_hgi_with_caller_supplied_gradients(dev):
    """DGT.perform_hgi (dgt.py:168-220) as its own entry point: fed modgabphasegrad's gradients it reproduces pghi()
    pop for pop; fed other gradients it integrates those (the pop order depends on the magnitudes alone), and the
    magnitude array passed in stays untouched."""
    g = torch.Generator().manual_seed(77)
    d = A.DGT(n_fft=128, hop_length=32).to(dev)
    mags = (torch.randn(3, 19, 65, generator=g) ** 2 + torch.randn(3, 19, 65, generator=g) ** 2).sqrt().to(dev)
    eps, tol = float(d.eps), float(d.tolerance)
    clamped = torch.clamp(mags, min=eps)
    tg, fg = d.modgabphasegrad(clamped)
    keep = clamped.clone()
    ph = d.perform_hgi(clamped, tg, fg, eps, tol)
    assert torch.equal(clamped, keep)
    assert torch.equal(ph, d.pghi(mags, d.tolerance))
    assert torch.equal(d.perform_hgi(clamped[1], tg[1], fg[1], eps, tol), ph[1])          # 2-D form
    # other gradients, same magnitudes: same pops, phases follow the new gradients (zero gradients -> zero phase)
    z = torch.zeros_like(tg)
    p0, n0, o0 = ops.pghi_integrate(clamped, z, z, tol, eps, debug=True)
    p1, n1, o1 = ops.pghi_integrate(clamped, tg, fg, tol, eps, debug=True)
    assert torch.equal(n0, n1) and torch.equal(o0, o1) and float(p0.abs().max()) == 0.0
    for b in range(3):
        r = O.pghi_offline(mags[b].cpu(), 128, 32, want_order=True)
        assert int(n1[b]) == len(r["order"])
        assert np.array_equal(cpu(o1[b][:len(r["order"])]), r["order"][:, 0] * 65 + r["order"][:, 1])


def test_overlap_add_state_helpers(dev):
    """get_input_buffer / get_output_buffer / _forward_without_update / _invert_without_update (reference
    oadd.py:33-67): the stateless pair reproduces what forward / invert do on a fresh module."""
    oa = A.OverlapAdd(1024, 256).to(dev)
    x = torch.randn(2, 4096, device=dev)
    fr = oa._forward_without_update(x)
    assert fr.shape[-1] == 1024
    full = oa._invert_without_update(fr)
    assert full.shape == (2, fr.shape[-2] * 256 + 1024)
    fresh = A.OverlapAdd(1024, 256).to(dev)
    y = fresh.invert(fr)                                   # zeros carried in: the same sums, minus the tail ...
    # ... but `invert` adds the frames as they are (oadd.py:98) where the stateless form scales each by 2 / overlap
    # (oadd.py:65; pinned against the reference's outputs by G19, tests/test_chain_gpu.py)
    assert torch.allclose(full[..., :y.shape[-1]] * 2.0, y, rtol=0, atol=1e-6)
    h0 = oa.get_input_buffer(x)
    assert h0.shape == (2, 768) and float(h0.abs().max()) == 0.0
    assert torch.equal(oa.get_input_buffer(x), x[..., -768:])
    assert oa.get_output_buffer(fr).shape == (2, 768)


def test_direct_pghi_calls_use_the_reference_defaults(dev):
    """DGT.pghi(mag) defaults to tolerance 1e-4 and RealtimeDGT.pghi(mag) to 1e-6 (dgt.py:156, 338) -- `invert` is what
    passes the module's own `tolerance` (1e-2)."""
    g = torch.Generator().manual_seed(5)
    d = A.DGT(n_fft=128, hop_length=32).to(dev)
    mag = (torch.rand(17, 65, generator=g) ** 4).to(dev)
    assert torch.equal(d.pghi(mag), d.pghi(mag, 1e-4))
    assert not torch.equal(d.pghi(mag), d.pghi(mag, d.tolerance))          # more bins integrated at the tighter tolerance
    rt = A.RealtimeDGT(n_fft=128, hop_length=32, batch_size=[1]).to(dev)
    m = mag[:4].unsqueeze(0)
    z = torch.zeros_like(m)
    assert torch.equal(rt.pghi(m, noise=z), rt.pghi(m, 1e-6, noise=z))


@pytest.mark.parametrize("n_fft,hop,S,n", [(1024, 256, 5, 3), (1024, 256, 3, 1), (512, 128, 4, 4), (400, 160, 3, 2), (256, 64, 2, 5),
                                            (2048, 512, 2, 2), (64, 16, 3, 3)])
def test_realtime_rank_fast_path_equals_the_heap_kernels(dev, n_fft, hop, S, n):
    """Round 4: where no two candidate magnitudes of a frame are equal, the realtime flood hands its entries out through a
    bitmap over their ranks (sorted by a pre-pass) instead of the heap (since round 5: variant 4; the default tries the
    queue-free scan path first and goes to the heap when that declines -- all four routes must agree).  Same pop order, same float operations: the
    phases must be the SAME BITS as the cooperative heap kernel's (variant 3) and the single-lane kernel's (variant 2), on
    noise, on sparse spectra (reseeds inside a frame, bins below the tolerance) and on input with exact ties -- quantised
    magnitudes, and a frame repeated exactly (every candidate of row f ties with row f-1) -- where the pre-pass reports
    the tie and the frame takes the heap.  n_fft 2048 (2F > 2048) and 64 (tables do not fit) never take the fast path."""
    F = n_fft // 2 + 1
    g = torch.Generator().manual_seed(n_fft + 7 * S + n)
    rt = A.RealtimeDGT(n_fft=n_fft, hop_length=hop, batch_size=[S]).to(dev)
    kinds = {}
    base = (torch.randn(S, n + 2, F, generator=g) ** 2 + torch.randn(S, n + 2, F, generator=g) ** 2).sqrt()
    kinds["noise"] = base
    kinds["sparse"] = base * (torch.rand(S, n + 2, F, generator=g) < 0.15) + 1e-6
    kinds["quantised"] = torch.round(base * 3) / 3 + 0.25
    rep = base.clone()
    rep[:, 1:] = rep[:, :1]                                          # every frame equal to the one before
    kinds["repeated"] = rep
    peaky = base * torch.exp(-((torch.arange(F) - F / 3.0) / (F / 20.0)) ** 2)      # most bins under the tolerance
    kinds["peaky"] = peaky + 1e-7
    for kind, m in kinds.items():
        hist, mag = m[:, :2].contiguous().to(dev), m[:, 2:].contiguous().to(dev)
        prev = (torch.rand(S, F, generator=g) * 6.28).to(dev)
        noise = torch.randn(S, n, F, generator=g).to(dev)
        args = (float(rt.gamma), n_fft, hop, float(rt.tolerance), float(rt.eps))
        got = ops.pghi_realtime(hist, mag, prev, noise, *args)
        with variant("pghi_kernel", 3):
            heap = ops.pghi_realtime(hist, mag, prev, noise, *args)
        with variant("pghi_kernel", 2):
            serial = ops.pghi_realtime(hist, mag, prev, noise, *args)
        with variant("pghi_kernel", 4):                     # round 5: the rank path without the scan path in front of it
            ranked = ops.pghi_realtime(hist, mag, prev, noise, *args)
        assert torch.equal(got, heap), (kind, float((got - heap).abs().max()))
        assert torch.equal(got, serial), (kind, float((got - serial).abs().max()))
        assert torch.equal(got, ranked), (kind, float((got - ranked).abs().max()))
        assert bool(torch.isfinite(got).all())
        if kind in ("noise", "sparse"):          # and the checker itself: the C restatement of dgt.py:330-466
            ref = O.pghi_realtime(hist.cpu().numpy(), mag.cpu().numpy(), prev.cpu().numpy(), noise.cpu().numpy(), n_fft, hop,
                                  tol=float(rt.tolerance), gamma=float(rt.gamma), eps=float(rt.eps))["phase"]
            assert np.all(np.abs(cpu(got) - ref) <= phase_tol(ref, base=2e-3, ulps=16)), kind


def test_realtime_rows_that_do_not_fit_lds(dev):
    """n_fft 4096 (F = 2049): a frame's rows and heap need more than 64 KB of LDS, so every variant runs
    `pghi_hgi_rt_kernel`, the single-lane flood on rows in global memory -- the product path of every row longer than about
    1088 bins.  Two streams (the per-stream base offsets) and two new frames (the step from one frame to the next), on noise
    and on a sparse spectrum (reseeds inside a frame; bins at or below the tolerance keep their draw), against the C
    restatement of dgt.py:330-466.  The default and variant 2 take the same kernel here: the same bits, so a change of the
    64 KB rule cannot move this size onto another route unnoticed."""
    n_fft, hop, S, n = 4096, 1024, 2, 2
    F = n_fft // 2 + 1
    g = torch.Generator().manual_seed(n_fft + 7 * S + n)
    rt = A.RealtimeDGT(n_fft=n_fft, hop_length=hop, batch_size=[S]).to(dev)
    base = (torch.randn(S, n + 2, F, generator=g) ** 2 + torch.randn(S, n + 2, F, generator=g) ** 2).sqrt()
    kinds = {"noise": base, "sparse": base * (torch.rand(S, n + 2, F, generator=g) < 0.15) + 1e-6}
    for kind, m in kinds.items():
        hist, mag = m[:, :2].contiguous().to(dev), m[:, 2:].contiguous().to(dev)
        prev = (torch.rand(S, F, generator=g) * 6.28).to(dev)
        noise = torch.randn(S, n, F, generator=g).to(dev)
        args = (float(rt.gamma), n_fft, hop, float(rt.tolerance), float(rt.eps))
        got = ops.pghi_realtime(hist, mag, prev, noise, *args)
        with variant("pghi_kernel", 2):
            serial = ops.pghi_realtime(hist, mag, prev, noise, *args)
        ref = O.pghi_realtime(hist.cpu().numpy(), mag.cpu().numpy(), prev.cpu().numpy(), noise.cpu().numpy(), n_fft, hop,
                              tol=float(rt.tolerance), gamma=float(rt.gamma), eps=float(rt.eps))["phase"]
        err = np.abs(cpu(got) - ref)
        print(f"{kind}: max |got - oracle| = {float(err.max()):.3e}, kept draws = {int((ref == cpu(noise)).sum())}")
        assert bool(torch.isfinite(got).all()), kind
        assert np.all(err <= phase_tol(ref, base=2e-3, ulps=16)), (kind, float(err.max()))
        assert torch.equal(got, serial), (kind, float((got - serial).abs().max()))


def test_realtime_scan_path_edge_cases(dev):
    """Round 5: by default a realtime frame is resolved WITHOUT a queue -- two directional scans of clamp functions give
    every bin the level at which it is reached and by whom, the phases follow the parent chains (`rt_scan_frame`,
    pghi_rt.hip) -- and only competing ties / islands of several unreached bins go to the heap.  The cases the derivation has
    to get right, each against the cooperative heap kernel (variant 3) bit for bit: the frame maximum (the reference's
    UNMARKED seed, dgt.py:427) at bin 0, 1, F-2, F-1, under a larger / smaller / dead source, between dead neighbours;
    bin 0 under a dead source (never reached from above, :453: a one-bin reseed); onsets (row f live where row f-1 is
    silent: islands of several bins -> declined); silence; one live bin; exact ties next to the maximum; plus random
    sparsity patterns of both rows."""
    n_fft, hop, F = 1024, 256, 513
    g = torch.Generator().manual_seed(555)
    rt = A.RealtimeDGT(n_fft=n_fft, hop_length=hop, batch_size=[1]).to(dev)
    args = (float(rt.gamma), n_fft, hop, float(rt.tolerance), float(rt.eps))

    def ray(*shape):
        return (torch.randn(*shape, generator=g) ** 2 + torch.randn(*shape, generator=g) ** 2).sqrt() + 0.05

    cases = []
    for kmax in (0, 1, 2, F - 2, F - 1, 200):
        for src in ("larger", "smaller", "dead"):
            for nb in ("live", "dead", "left_dead", "right_dead"):
                m = ray(6, F)
                m[2:] = m[2:].clamp(max=3.0)
                for f in range(2, 6):
                    m[f, kmax] = 5.0 + 0.1 * f                                  # the frame maximum of rows 2..5
                    m[f - 1, kmax] = {"larger": 9.0 + f, "smaller": 1.0, "dead": 0.0}[src] if f - 1 < 2 else m[f - 1, kmax]
                    if nb in ("dead", "left_dead") and kmax - 1 >= 0:
                        m[f, kmax - 1] = 0.0
                    if nb in ("dead", "right_dead") and kmax + 1 < F:
                        m[f, kmax + 1] = 0.0
                m[1, kmax] = {"larger": 9.0, "smaller": 1.0, "dead": 0.0}[src]
                cases.append(m)
    m = ray(6, F)
    m[0:2, 0] = 0.0
    cases.append(m)                                                             # bin 0 under a dead source
    m = ray(6, F) * (torch.rand(6, F, generator=g) < 0.5)
    cases.append(m)                                                             # half the bins dead in every row
    m = ray(6, F)
    m[:3] = 0.0
    cases.append(m)                                                             # onset: silence, then noise
    m = ray(6, F)
    m[3:] = 0.0
    cases.append(m)                                                             # offset: noise, then silence
    m = torch.zeros(6, F)
    m[:, 77] = 1.0
    cases.append(m)                                                             # one live bin
    m = ray(6, F)
    m[2:, 300] = 7.0
    m[2:, 301] = 7.0
    cases.append(m)                                                             # the maximum twice, side by side
    m = ray(6, F)
    m[2:, 300] = 7.0
    m[1:5, 302] = 7.0
    cases.append(m)                                                             # a source tied with the seed two bins away
    for _ in range(40):
        dens0, dens1 = float(torch.rand(1, generator=g)), float(torch.rand(1, generator=g))
        m = ray(6, F)
        m[0::2] = m[0::2] * (torch.rand(3, F, generator=g) < dens0)
        m[1::2] = m[1::2] * (torch.rand(3, F, generator=g) < dens1)
        cases.append(m)
    spec = torch.stack(cases)                                                   # (cases, 6, F): every case a stream
    S = spec.shape[0]
    hist, mag = spec[:, :2].contiguous().to(dev), spec[:, 2:].contiguous().to(dev)
    prev = (torch.rand(S, F, generator=g) * 6.28).to(dev)
    noise = torch.randn(S, 4, F, generator=g).to(dev)
    got = ops.pghi_realtime(hist, mag, prev, noise, *args)
    with variant("pghi_kernel", 3):
        heap = ops.pghi_realtime(hist, mag, prev, noise, *args)
    with variant("pghi_kernel", 4):
        ranked = ops.pghi_realtime(hist, mag, prev, noise, *args)
    bad = (got != heap).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, ("streams that differ from the heap kernel", bad[:10])
    assert torch.equal(ranked, heap)
    assert bool(torch.isfinite(got).all())


def test_realtime_rank_fast_path_with_injected_ties(dev):
    """tools/fuzz_rt_ties.py: magnitudes copied onto other bins (far away: the tied pops commute and the frame stays on the
    bitmap; next to each other or onto the frame maximum: the blocks collide and the frame is redone on the heap) --
    the phases are the cooperative heap kernel's bit for bit either way."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FUZZ_CASES="80", FUZZ_SEED="11")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_rt_ties.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "80 cases ok" in r.stdout and "bit for bit" in r.stdout

"""GPU parity: "sinebank" inversion (at_sinebank_offline / at_sinebank_realtime) against the reference's outputs
(tests/golden/g13_sinebank.npz, random phases recorded) and the oracle.  The oscillator phase is formed in fp32
exactly as the reference does; what differs is the summation order over bins (MFMA contraction vs torch.sum)
and sin()'s last bit -> 1e-5 of the output's largest magnitude (the output is peak-normalised to 1).

The second half runs the cases of sinebank_cases.py, which name the kernel path each one reaches
(test_sinebank_cases_cpu.py checks that they reach all of them), under the same bar, and pins who owns the stream clock."""
import copy

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import sinebank_cases as C
from acids_transforms_amd import ops
from acids_transforms_amd._lib import AcidsHipError, variant
from acids_transforms_amd.transforms.sinebank import _offline_tables
from conftest import rel_max
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
T_ = torch.from_numpy


def cpu(t):
    return t.detach().cpu()


def test_offline_golden(golden, dev):
    g = golden("g13_sinebank")
    s = A.STFT(n_fft=128, hop_length=32).to(dev)
    y = s.get_sinebank_inversion(T_(g["mag"]).to(dev), random_phase=T_(g["offline_phase"]))
    assert y.shape == g["offline"].shape
    assert rel_max(cpu(y).numpy(), g["offline"]) < TOL
    s1k = A.STFT().to(dev)
    y = s1k.get_sinebank_inversion(T_(g["mag1k"]).to(dev), random_phase=T_(g["offline1k_phase"]))
    assert rel_max(cpu(y).numpy(), g["offline1k"]) < TOL
    # through invert(): same CPU generator stream as the reference -> same phases after the same seed
    torch.manual_seed(77)
    want_phase = 2 * torch.pi * torch.rand(65, 1)
    torch.manual_seed(77)
    d = A.DGT(n_fft=128, hop_length=32).to(dev)
    y = d.invert(T_(g["mag"]).to(dev), inversion_mode="sinebank")
    want = O.sinebank_offline(T_(g["mag"]), 44100, 128, 32, want_phase)
    assert rel_max(cpu(y).numpy(), want.numpy()) < TOL
    assert "sinebank" in s.get_inversion_modes() and "sinebank" in A.DGT.get_inversion_modes()


def test_realtime_golden(golden, dev):
    g = golden("g13_sinebank")
    chunks = T_(g["chunks"]).to(dev)
    for name, cls in (("rtstft", A.RealtimeSTFT), ("rtdgt", A.RealtimeDGT)):
        r = cls(n_fft=128, hop_length=32).to(dev)
        r.random_phase = T_(g[name + "_phase"]).to(dev)        # batch-shaped already: no re-draw
        for i in range(3):
            y = r.get_sinebank_inversion(chunks[i])
            assert y.shape == (3, 4, 128)
            assert rel_max(cpu(y).numpy(), g[name][i]) < TOL, (name, i)
        assert abs(float(r.time_index) - float(g[name + "_time"])) < 1e-6
    r = A.RealtimeSTFT(n_fft=128, hop_length=32).to(dev)
    r.random_phase = T_(g["rt_unbatched_phase"]).to(dev)
    for i in range(2):
        y = r.get_sinebank_inversion(chunks[i, 0])
        assert rel_max(cpu(y).numpy(), g["rt_unbatched"][i]) < TOL
    # invert(mode="sinebank") hands OverlapAdd the frames TIMES the synthesis window (stft.py:303-304, dgt.py:321-322)
    for name, cls in (("rtstft_invert", A.RealtimeSTFT), ("rtdgt_invert", A.RealtimeDGT)):
        ri = cls(n_fft=128, hop_length=32).to(dev)
        ri.random_phase = T_(g[name + "_phase"]).to(dev)
        assert np.allclose(cpu(ri.inv_window[:128]).numpy(), g[name + "_inv_window"], rtol=1e-6, atol=1e-7)
        for i in range(2):
            y = ri.invert(chunks[i], inversion_mode="sinebank")
            assert rel_max(cpu(y).numpy(), g[name][i]) < TOL, (name, i)
    r.reset()
    y0 = r.get_sinebank_inversion(chunks[0, 0])
    assert rel_max(cpu(y0).numpy(), g["rt_unbatched"][0]) < TOL          # the clock restarts


def test_offline_against_oracle_shapes(dev):
    """Default geometry at a size the oracle still handles, ragged batch shapes, hop < 128 (more frames per block)."""
    gen = torch.Generator().manual_seed(9)
    for (shape, n_fft, hop) in [((3, 40, 513), 1024, 256), ((2, 2, 7, 513), 1024, 256), ((1, 1, 513), 1024, 256),
                                ((4, 33, 129), 256, 64), ((2, 50, 33), 64, 16)]:
        mag = torch.rand(*shape, generator=gen) ** 2
        F = shape[-1]
        phase = 2 * torch.pi * torch.rand(F, 1, generator=gen)
        s = A.STFT(n_fft=n_fft, hop_length=hop).to(dev)
        y = s.get_sinebank_inversion(mag.to(dev), random_phase=phase)
        want = O.sinebank_offline(mag.reshape((-1,) + shape[-2:]), 44100, n_fft, hop, phase)
        assert y.shape == shape[:-2] + (hop * shape[-2] + n_fft,)
        assert rel_max(cpu(y).reshape(want.shape).numpy(), want.numpy()) < TOL, (shape, n_fft, hop)
        assert abs(float(y.max()) - 1.0) < 1e-6                       # peak-normalised


def test_full_size_properties(dev):
    """BASELINE clip length (4 s -> 690 frames), 64 clips: properties that do not need the oracle at this size --
    linear in the magnitudes up to the two normalisations, and the clip of a constant single-bin spectrum is that
    bin's sinusoid with a constant envelope."""
    T, F = 690, 513
    s = A.STFT().to(dev)
    gen = torch.Generator().manual_seed(10)
    phase = 2 * torch.pi * torch.rand(F, 1, generator=gen)
    mag = torch.zeros(64, T, F)
    mag[:, :, 40] = 1.0                     # 40 * 44100 / 1024 = 1722.66 Hz
    mag[1:] += 0.0
    y = cpu(s.get_sinebank_inversion(mag.to(dev), random_phase=phase))
    L = 256 * T + 1024
    assert y.shape == (64, L)
    t = torch.linspace(0, L / 44100, L)
    arg = (2 * torch.pi * torch.linspace(0, 22050, F)[40]) * t + phase[40, 0]
    want = torch.sin(arg)
    want = want / want.max()
    assert float((y[0] - want).abs().max()) < 1e-5 and torch.equal(y[0], y[63])
    # scaling the input leaves the output unchanged (x / max|x| first)
    m2 = torch.rand(8, T, F, generator=gen)
    a = s.get_sinebank_inversion(m2.to(dev), random_phase=phase)
    b = s.get_sinebank_inversion((m2 * 3.0).to(dev), random_phase=phase)
    assert float((a - b).abs().max()) < 2e-6


# ---- every kernel path: the cases of sinebank_cases.py ----------------------------------------------------------------
def _offline(case, dev, module=None):
    """The case's clips through STFT.get_sinebank_inversion: (output on the CPU, error against the fp32 oracle)."""
    B, T, n_fft, hop = case
    mag, phase = C.offline_inputs(case)
    s = module if module is not None else A.STFT(n_fft=n_fft, hop_length=hop).to(dev)
    y = cpu(s.get_sinebank_inversion(mag.to(dev), random_phase=phase))
    assert y.shape == (B, C.out_len(T, n_fft, hop))
    return y, rel_max(y.numpy(), C.offline_oracle(case).numpy())


@pytest.mark.parametrize("case", C.OFFLINE_CASES, ids=lambda c: "B%d-T%d-n%d-h%d" % c)
def test_offline_paths(case, dev):
    y, err = _offline(case, dev)
    print("sinebank offline %-22s F %4d  n_pass %2d  rel_max %.2e" % (case, C.n_bins(case[2]), C.n_pass(*case[1:]), err))
    assert err < TOL, (case, err)
    assert abs(float(y.max()) - 1.0) < 1e-6                           # peak-normalised


@pytest.mark.parametrize("case", C.ROW_RUN_CASES, ids=lambda c: "B%d-T%d-n%d-h%d" % c)
def test_offline_row_runs(case, dev):
    """DENSE mel_gemm_kernel with 1, 2 and all of its 32-row tiles per workgroup (the double-buffered staging through the
    block offsets): same bits as the default plan; every clip differs, so a swapped row or a stale tile shows."""
    mag, _ = C.offline_inputs(case)
    assert all(not torch.equal(mag[0], mag[b]) for b in range(1, case[0]))
    y0, err0 = _offline(case, dev)
    assert err0 < TOL
    for v in sorted({1, 2, C.row_tiles(case[0])}):
        with variant("row_run", v):
            y, err = _offline(case, dev)
        print("sinebank offline %-18s row_run %d  rel_max %.2e  bit-equal %s" % (case, v, err, torch.equal(y, y0)))
        assert torch.equal(y, y0), (case, v)
        assert err < TOL, (case, v, err)


def _tables(case):
    B, T, n_fft, hop = case
    return _offline_tables(T, C.n_bins(n_fft), n_fft, hop, C.SR)


def test_offline_pass_limit(dev):
    """64 passes, the ABI's limit, pass parity; 70 are refused by the launcher's argument check, and the module goes on."""
    assert _tables(C.PASS_LIMIT_CASE)[1] == C.PASS_LIMIT
    _, err = _offline(C.PASS_LIMIT_CASE, dev)
    print("sinebank offline %-22s n_pass 64  rel_max %.2e" % (C.PASS_LIMIT_CASE, err))
    assert err < TOL
    B, T, n_fft, hop = C.OVER_PASS_LIMIT_CASE
    assert _tables(C.OVER_PASS_LIMIT_CASE)[1] == 70
    s = A.STFT(n_fft=n_fft, hop_length=hop).to(dev)
    mag, phase = C.offline_inputs(C.OVER_PASS_LIMIT_CASE)
    with pytest.raises(AcidsHipError):
        s.get_sinebank_inversion(mag.to(dev), random_phase=phase)
    follow = (2, 6, n_fft, hop)                                       # one block, six passes
    _, err = _offline(follow, dev, module=s)
    print("sinebank offline %-22s after the refusal  rel_max %.2e" % (follow, err))
    assert err < TOL


def _realtime_module(cls, case, batch, dev):
    """A fresh module with the case's phases and clock set by the caller."""
    S, T, n_fft, hop, clock = case
    mag, phase = C.realtime_inputs(case, batch)
    r = cls(n_fft=n_fft, hop_length=hop).to(dev)
    r.random_phase = phase.to(dev)
    r.time_index = torch.tensor(clock, device=dev)
    return r, mag


@pytest.mark.parametrize("cls", [A.RealtimeSTFT, A.RealtimeDGT], ids=["stft", "dgt"])
@pytest.mark.parametrize("case", C.REALTIME_CASES, ids=lambda c: "S%d-T%d-n%d-h%d-t%g" % c)
def test_realtime_paths(case, cls, dev):
    S, T, n_fft, hop, clock = case
    for batch in ((S,), (2, 3), ()):
        want, clock_after = C.realtime_oracle(case, batch)
        for windowed in (False, True):
            r, mag = _realtime_module(cls, case, batch, dev)
            if windowed:
                y = cpu(r.invert(mag.to(dev), inversion_mode="sinebank"))
                ref = want * cpu(r.inv_window[:n_fft])
            else:
                y = cpu(r.get_sinebank_inversion(mag.to(dev)))
                ref = want
            assert y.shape == tuple(batch) + (T, n_fft)
            err = rel_max(y.numpy(), ref.numpy())
            print("sinebank realtime %-4s %-28s batch %-6s %-10s rel_max %.2e" % (
                cls.__name__[8:], case, batch, "windowed" if windowed else "unwindowed", err))
            assert err < TOL, (case, batch, windowed, err)
            assert float(r.time_index) == float(clock_after)


def test_realtime_limits(dev):
    """Op level: one step past the grid and the LDS limit is refused by the launcher's argument check (nothing is
    launched); at the limits the kernel matches the float64 model."""
    for S, T, F, N in C.REALTIME_REFUSED:
        z = torch.zeros
        with pytest.raises(AcidsHipError):
            ops.sinebank_realtime(z(S, T, F, device=dev), z(F, device=dev), z(T, N, device=dev), z(S, F, device=dev))
    for lim in C.REALTIME_LIMIT_CASES:
        x, c, tau, phi = C.realtime_limit_inputs(*lim)
        y = cpu(ops.sinebank_realtime(x.to(dev), c.to(dev), tau.to(dev), phi.to(dev)))
        assert y.shape == (lim[0], lim[1], lim[3])
        err = rel_max(y.numpy(), C.realtime_model_op(x, c, tau, phi).numpy())
        print("sinebank realtime op S %d T %d F %d N %d  rel_max %.2e against the float64 model" % (lim[:4] + (err,)))
        assert err < TOL, (lim, err)


def test_realtime_long_stream(dev):
    """200 one-frame chunks at the default size: the buffer's clock stays the oracle's, bit for bit, and the frames at
    it pass parity."""
    S, n_fft, hop = C.LONG_STREAM["S"], C.LONG_STREAM["n_fft"], C.LONG_STREAM["hop"]
    n, every, F = C.LONG_STREAM["chunks"], C.LONG_STREAM["check_every"], C.n_bins(n_fft)
    gen = torch.Generator().manual_seed(12)
    mags = torch.rand(n, S, 1, F, generator=gen) ** 2
    phase = 2 * torch.pi * torch.rand(S, 1, F, generator=gen)
    r = A.RealtimeSTFT(n_fft=n_fft, hop_length=hop).to(dev)
    r.random_phase = phase.to(dev)
    mags_d = mags.to(dev)
    now = torch.tensor(0.)
    for i in range(n):
        y = r.get_sinebank_inversion(mags_d[i])
        if (i + 1) % every == 0:
            want, after = O.sinebank_realtime(mags[i], C.SR, n_fft, hop, phase, now)
            err = rel_max(cpu(y).numpy(), want.numpy())
            print("sinebank realtime chunk %3d at %.4f s  rel_max %.2e" % (i + 1, float(now), err))
            assert err < TOL, (i, err)
            assert float(r.time_index) == float(after), (i, float(r.time_index), float(after))
            now = after
        else:
            now = now + (1 * hop + n_fft) / C.SR                     # the oracle's own advance
    assert float(now) > 5.0


@pytest.mark.parametrize("cls", [A.RealtimeSTFT, A.RealtimeDGT], ids=["stft", "dgt"])
def test_realtime_clock_ownership(cls, dev):
    """The registered buffer `time_index` is the clock: a loaded state, an assigned tensor and an in-place write all
    rule over what the module remembers of its own earlier chunks (the reference reads the buffer on every call)."""
    n_fft, hop, T = 128, 32, 4
    gen = torch.Generator().manual_seed(13)
    chunks = torch.rand(4, 3, T, 65, generator=gen) ** 2
    phase = 2 * torch.pi * torch.rand(3, 1, 65, generator=gen)
    step = (T * hop + n_fft) / C.SR
    r = cls(n_fft=n_fft, hop_length=hop).to(dev)
    r.random_phase = phase.to(dev)

    def run(i):
        return cpu(r.get_sinebank_inversion(chunks[i].to(dev)))

    def want(i, t):
        return O.sinebank_realtime(chunks[i], C.SR, n_fft, hop, phase, torch.tensor(t))[0].numpy()

    y1 = run(0)
    sd = copy.deepcopy(r.state_dict())
    y2 = run(1)
    assert rel_max(y2.numpy(), want(1, step)) < TOL
    r.load_state_dict(sd)                                             # back to the state after chunk 1
    assert torch.equal(run(1), y2)
    t0 = 1234.5
    r.time_index = torch.tensor(t0, device=dev)                       # a clock set by the caller
    assert rel_max(run(2).numpy(), want(2, t0)) < TOL
    assert float(r.time_index) == float(torch.tensor(t0) + step)
    r.time_index.zero_()                                              # in place
    assert torch.equal(run(0), y1)
    assert rel_max(run(1).numpy(), want(1, step)) < TOL               # ... and the shadow follows on from there
    if cls is A.RealtimeDGT:
        t = float(r.time_index)
        r.reset([3])                                                  # the PGHI history only (reference dgt.py)
        assert float(r.time_index) == t
        assert rel_max(run(3).numpy(), want(3, t)) < TOL

"""The cases of test_sinebank_gpu.py reach every path of the sinebank kernels (sinebank_cases.py restates them), the
host tables of transforms/sinebank._offline_tables rebuild F.interpolate's envelope, the fp32 oracle lies far below the
GPU file's 1e-5 bar from a float64 model, and the host shadow of the stream clock adds as the buffer does.  CPU only."""
import collections

import numpy as np
import torch

import sinebank_cases as C
from acids_transforms_amd.transforms import sinebank as SB
from conftest import rel_max

TABLE_BAR = 2e-6      # envelope from the tables against F.interpolate, absolute (magnitudes in [0, 1]): about twice the
                      # worst value over the sweep, 8.5e-7 at (n_fft 16, hop 1, T 33), where the tables' frame below a
                      # near-integer source index is one off ATen's and the weight at stake is ~1e-6; 6e-8 everywhere else
ORACLE_BAR = 1e-6     # fp32 oracle against the float64 model: measured 1e-7 .. 2.6e-7 offline, up to 1.9e-7 realtime


def test_projection_form_restated():
    assert C.projection_form(15) == {"kernel": "simple"} and C.projection_form(577) == {"kernel": "simple"}
    assert C.projection_form(16) == {"kernel": "mfma", "k_main": 16, "tail": 0, "segments": 1}
    assert C.projection_form(576) == {"kernel": "mfma", "k_main": 512, "tail": 64, "segments": 5}
    assert C.projection_form(513) == {"kernel": "mfma", "k_main": 512, "tail": 1, "segments": 5}
    assert C.projection_form(201)["tail"] == 73 and C.projection_form(221)["tail"] == 93
    assert C.projection_form(501) == {"kernel": "mfma", "k_main": 256, "tail": 245, "segments": 4}
    assert C.n_pass(690, 1024, 256) == 3 and C.n_pass(129, 64, 4) == 30
    assert C.n_pass(*C.PASS_LIMIT_CASE[1:]) == C.PASS_LIMIT and C.n_pass(*C.OVER_PASS_LIMIT_CASE[1:]) == 70
    assert C.combine_sweeps(3, C.out_len(175000, 16, 4)) == 2 and 3 * C.out_len(175000, 16, 4) == 2_100_048
    assert C.row_tiles(40) == 2 and C.row_tiles(70) == 3
    assert C.rt_blocks(1024) == 4 and C.rt_blocks(400) == 2 and C.rt_staging_trips(513) == 3
    assert C.rt_staging_trips(2049) == 9 and C.rt_staging_trips(201) == 1


def test_offline_cases_reach_every_path():
    hit = collections.Counter()
    for case in C.OFFLINE_CASES:
        hit.update(C.offline_paths(case))
    assert dict(hit) == C.OFFLINE_PATH_COUNTS, {k: (hit.get(k), C.OFFLINE_PATH_COUNTS.get(k))
                                                 for k in set(hit) | set(C.OFFLINE_PATH_COUNTS)
                                                 if hit.get(k) != C.OFFLINE_PATH_COUNTS.get(k)}
    assert all(case in C.OFFLINE_CASES for case in C.ROW_RUN_CASES + [C.PASS_LIMIT_CASE])
    for case in C.ROW_RUN_CASES:
        assert {"partial_last_tile"} <= C.offline_paths(case) and C.row_tiles(case[0]) in (2, 3)
    assert C.n_pass(*C.OVER_PASS_LIMIT_CASE[1:]) > C.PASS_LIMIT


def test_realtime_cases_reach_every_path():
    hit = collections.Counter()
    for S, T, n_fft, hop, clock in C.REALTIME_CASES:
        assert not C.rt_refused(S, T, C.n_bins(n_fft)) and not C.rt_refused(6, T, C.n_bins(n_fft))
        hit.update(C.realtime_paths(S, T, C.n_bins(n_fft), n_fft, clock))
    for S, T, F, N, clock in C.REALTIME_LIMIT_CASES:
        assert not C.rt_refused(S, T, F)
        hit.update(C.realtime_paths(S, T, F, N, clock))
    assert dict(hit) == C.REALTIME_PATH_COUNTS, dict(hit)
    # each refusal sits one step past a limit case, on one limit only
    (S0, T0, F0, N0), (S1, T1, F1, N1) = C.REALTIME_REFUSED
    assert C.rt_refused(S0, T0, F0) and not C.rt_refused(S0, T0, F0 - 1) and S0 * T0 <= C.RT_GRID_LIMIT
    assert C.rt_refused(S1, T1, F1) and S1 * T1 == C.RT_GRID_LIMIT + 1 and 12 * F1 <= C.RT_LDS_BYTES


def _check_tables(T, n_fft, hop, seed):
    F = C.n_bins(n_fft)
    L, n_pass, c, t, frame_off, W = SB._offline_tables(T, F, n_fft, hop, C.SR)
    W = W.numpy()
    frames = frame_off.numpy() // F
    blocks = C.cdiv(L, C.COL_BLOCK)
    assert L == C.out_len(T, n_fft, hop) and n_pass == C.n_pass(T, n_fft, hop), (T, n_fft, hop, n_pass)
    assert W.shape == (n_pass, L) and frames.shape == (n_pass, blocks) and frame_off.dtype == torch.int64
    assert (frame_off.numpy() % F == 0).all() and frames.min() >= 0 and frames.max() < T
    assert W.min() >= 0.0 and W.max() <= 1.0 and int((W != 0).sum(0).max()) <= 2
    assert c.shape == (F,) and t.shape == (L,) and c.dtype == t.dtype == torch.float32
    x = torch.rand(4, T, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    want = torch.nn.functional.interpolate(x.float().unsqueeze(0), L, mode="linear")[0].double().numpy()
    got = C.envelope_from_tables(x.float().double().numpy(), frames, W)
    return float(np.abs(got - want).max())


def test_offline_tables_against_interpolate():
    worst = 0.0
    geoms = [(T, n_fft, hop) for _, T, n_fft, hop in C.OFFLINE_CASES] + [(T, n, h) for (n, h), T in C.TABLE_SWEEP]
    assert len(C.TABLE_SWEEP) == 17 * 6
    for i, (T, n_fft, hop) in enumerate(geoms):
        err = _check_tables(T, n_fft, hop, i)
        worst = max(worst, err)
        assert err < TABLE_BAR, (T, n_fft, hop, err)
    print("tables against F.interpolate: worst %.2e over %d geometries" % (worst, len(geoms)))


def test_offline_tables_survive_eviction():
    geoms = [(T, n_fft, hop) for (n_fft, hop), T in C.TABLE_SWEEP[2::11]][:10]
    assert len(set(geoms)) == 10
    first = [SB._offline_tables(T, C.n_bins(n), n, h, C.SR) for T, n, h in geoms]
    assert len(SB._TABLES) <= 8                                   # the oldest ones are gone
    for i, ((T, n, h), old) in enumerate(zip(geoms, first)):
        assert _check_tables(T, n, h, 100 + i) < TABLE_BAR
        new = SB._offline_tables(T, C.n_bins(n), n, h, C.SR)
        assert new[:2] == old[:2] and all(torch.equal(a, b) for a, b in zip(new[2:], old[2:]))


def test_oracle_sits_far_below_the_bar_offline():
    for case in C.OFFLINE_CASES:
        mag, phase = C.offline_inputs(case)
        err = rel_max(C.offline_oracle(case).numpy(), C.offline_model(mag, C.SR, case[2], case[3], phase).numpy())
        print("offline %-22s oracle against float64 model %.2e" % (case, err))
        assert err < ORACLE_BAR, (case, err)


def test_oracle_sits_far_below_the_bar_realtime():
    for case in C.REALTIME_CASES:
        mag, phase = C.realtime_inputs(case)
        y, clock = C.realtime_oracle(case)
        S, T, n_fft, hop, now = case
        err = rel_max(y.numpy(), C.realtime_model(mag, C.SR, n_fft, hop, phase, now).numpy())
        print("realtime %-28s oracle against float64 model %.2e" % (case, err))
        assert err < ORACLE_BAR, (case, err)
        assert clock.dtype == torch.float32 and float(clock) == float(np.float32(now) + np.float32((T * hop + n_fft) / C.SR))
    # the op-level model agrees with the module-level one (the limit cases of the GPU file use it alone)
    case = C.REALTIME_CASES[1]
    S, T, n_fft, hop, now = case
    mag, phase = C.realtime_inputs(case)
    c = 2 * torch.pi * torch.linspace(0, C.SR / 2, C.n_bins(n_fft))
    y = C.realtime_model_op(mag, c, C.realtime_tau(T, n_fft, hop, C.SR, now), phase.reshape(S, -1))
    assert torch.equal(y, C.realtime_model(mag, C.SR, n_fft, hop, phase, now))


def test_clock_shadow_adds_like_the_buffer():
    """sinebank_realtime advances `time_index` (an fp32 tensor) by a Python float and its host shadow by np.float32
    additions: 20 000 chunks of each, at three chunk sizes, never part."""
    for T, n_fft, hop in ((1, 1024, 256), (4, 1024, 256), (3, 400, 100)):
        step = (T * hop + n_fft) / C.SR
        buf, shadow, bad = torch.tensor(0.), np.float32(0.), 0
        for _ in range(20000):
            buf = buf + step
            shadow = np.float32(shadow + np.float32(step))
            bad += float(buf) != float(shadow)
        assert bad == 0 and float(buf) > 300          # minutes into the stream: 24-bit sums that round at every step


def test_clock_shadow_follows_the_buffer(monkeypatch):
    """The host side of sinebank_realtime with the kernel stubbed out: the chunk's time stamps start at the registered
    buffer's value whoever wrote it last, and a run of chunks reads the buffer back once (one sync), not per chunk."""
    import copy

    import acids_transforms_amd as A
    starts, reads = [], [0]

    def fake_kernel(x, c, tau, phi, window=None):
        starts.append(tau[0, 0].item())
        return torch.zeros(x.shape[0], x.shape[1], tau.shape[-1])

    to_float = torch.Tensor.__float__

    def counting_float(self):
        reads[0] += 1
        return to_float(self)

    monkeypatch.setattr(SB.ops, "sinebank_realtime", fake_kernel)
    step = np.float32((4 * 32 + 128) / C.SR)
    for cls in (A.RealtimeSTFT, A.RealtimeDGT):
        r = cls(n_fft=128, hop_length=32)
        x = torch.rand(3, 4, 65)
        del starts[:]
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "__float__", counting_float)
            reads[0] = 0
            for _ in range(5):
                r.get_sinebank_inversion(x)
            assert reads[0] == 1                                   # the first chunk only
            sd = copy.deepcopy(r.state_dict())
            r.get_sinebank_inversion(x)
            r.load_state_dict(sd)
            r.get_sinebank_inversion(x)
            r.get_sinebank_inversion(x)
            assert reads[0] == 2                                   # once more after the load
        want = [np.float32(0)]
        for _ in range(5):
            want.append(np.float32(want[-1] + step))
        assert starts[:6] == [float(w) for w in want] and starts[6] == starts[5]
        assert starts[7] == float(np.float32(want[5] + step))
        r.time_index = torch.tensor(77.25)                         # set by the caller
        r.get_sinebank_inversion(x)
        r.time_index.zero_()                                       # written in place
        r.get_sinebank_inversion(x)
        r.get_sinebank_inversion(x)
        assert starts[8:] == [77.25, 0.0, float(step)]
        assert float(r.time_index) == float(np.float32(step + step))
        if cls is A.RealtimeDGT:
            r.reset([3])                                           # the PGHI history only: the clock stays
            assert float(r.time_index) == float(np.float32(step + step))
        else:
            r.reset()
            assert float(r.time_index) == 0.0
            r.get_sinebank_inversion(x)
            assert starts[-1] == 0.0

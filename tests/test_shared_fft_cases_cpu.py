"""CPU checks of shared_fft_cases.py: the per-clip grouping, the dispatch, that the sweeps of
test_clip_isolation_gpu.py reach every geometry class, and the float32 packing model behind the choice of inputs."""
import numpy as np

import shared_fft_cases as S


def test_groups_never_leave_a_clip():
    for K in (2, 4, 8):
        for B in (1, 2, 5):
            for T in range(1, 3 * K + 2):
                g = S.groups(B, T, K)
                assert len(g) == B * S.cdiv(T, K)
                seen = [m for grp in g for m in grp if m is not None]
                assert seen == [(b, t) for b in range(B) for t in range(T)]          # every frame once, in order
                for grp in g:
                    assert len(S.clips_in_group(grp)) == 1
                    for r, m in enumerate(grp):
                        assert m is None or m[1] % K == r                              # slot = index in the clip mod K
                # a clip's groups do not depend on the batch: clip b of B clips is clip 0 of one
                one = S.groups(1, T, K)
                for b in range(B):
                    mine = [[None if m is None else (0, m[1]) for m in grp] for grp in g if S.clips_in_group(grp) == {b}]
                    assert mine == one


def test_launch_wide_grouping_is_what_the_sweeps_tell_apart():
    """Where T % K != 0 the old grouping put frames of two (T < K: three or more) clips into one transform."""
    assert S.launch_wide_groups(2, 3, 2)[1] == [(0, 2), (1, 0)]
    assert len(S.clips_in_group(S.launch_wide_groups(5, 2, 8)[0])) == 4
    for K in (2, 4, 8):
        for T in range(1, 3 * K + 2):
            straddles = any(len(S.clips_in_group(g)) > 1 for g in S.launch_wide_groups(5, T, K))
            assert straddles == (T % K != 0)
            if T % K == 0:
                assert S.launch_wide_groups(5, T, K) == S.groups(5, T, K)              # the control
    assert S.mates(S.launch_wide_groups(3, 5, 4), 1, 0) == {(0, 4), (1, 0), (1, 1), (1, 2)}
    assert S.mates(S.groups(3, 5, 4), 1, 0) == {(1, 0), (1, 1), (1, 2), (1, 3)}
    assert S.mates(S.groups(3, 5, 4), 1, 4) == {(1, 4)}


def test_plans():
    assert S.groups_per_block(1) == 4 and S.groups_per_block(8192) == 4 and S.groups_per_block(8193) == 8
    assert S.groups_per_block(S.B_LARGE * 2) > S.WS
    assert S.mel_pairs_per_wave(5, 9) == 4 and S.mel_pairs_per_wave(5, 9, v=1) == 1 and S.mel_pairs_per_wave(5, 9, v=99) == 25
    assert S.mel_pairs_per_wave(1024, 690) == 44
    assert abs(S.extra_transform_work(5513, 8) - 7 / 5513) < 1e-12 and S.extra_transform_work(5513, 8) < 1.3e-3
    assert S.extra_transform_work(1, 8) == 7.0                                      # one-frame clips: K times the work


def test_dispatch():
    for n, K in ((128, 8), (256, 4)):
        for hop in S.hops_of(n):
            for center in (True, False):
                for phase in (True, False):
                    assert S.forward_kernel(n, hop, center, phase) == "stft_small_fwd_kernel<%d>" % K
            assert S.istft_kernel(n, hop) == "irfft_small_frames_kernel<%d>" % K
        assert S.irfft_frames_kernel(n) == "irfft_small_frames_kernel<%d>" % K
    assert S.forward_kernel(512, 128) == "stft512_run_fwd_kernel"
    for kw in (dict(hop=64), dict(hop=256), dict(hop=136), dict(hop=128, center=False), dict(hop=128, phase=True),
               dict(hop=128, L=300), dict(hop=128, clip_stride_odd=True), dict(hop=128, x_aligned=False),
               dict(hop=128, out_aligned=False), dict(hop=128, frame_kernels=True)):
        assert S.forward_kernel(512, **kw) == "stft512_fwd_kernel", kw
        assert len(S.forward_reason(512, **kw)) == 1
    assert [S.istft_kernel(512, h) for h in (64, 128, 256)] == ["istft512_ola_kernel"] * 3
    assert S.istft_kernel(512, 136) == "irfft512_frames_kernel" and S.istft_kernel(512, 128, env=False) == "irfft512_frames_kernel"
    assert S.irfft_frames_kernel(512) == "irfft512_frames_kernel"
    assert S.mel_kernel(512) == "stft512_mel_kernel" and S.mel_kernel(1024) == "other"
    assert S.forward_kernel(1024, 256) == "other" and S.irfft_frames_kernel(2048) == "other"


def test_sweeps_reach_every_geometry_class():
    for n_fft, K in S.K_OF.items():
        for kind in ("forward", "inverse", "frames"):
            want = S.geometry_classes(K)
            if kind == "inverse":
                want = want - {"T_lt_K_1"}                 # at_istft: one frame of an even size has no output
                if K == 4:
                    want = want - {"wide_group_holds_3_clips"}     # ... and four slots hold three clips at T = 1 only
            hit = S.swept_geometry(n_fft, kind)
            assert want <= hit, (n_fft, kind, sorted(want - hit))
    want = S.geometry_classes(2) - {"block_takes_more_than_WS_groups"}      # the mel kernel cuts by wave, see below
    hit = S.swept_geometry(512, "mel")
    assert want <= hit, sorted(want - hit)
    # stft512_mel_kernel: more than one pair per wave under the default plan and under two forced cuts, and a wave's
    # run that starts inside a clip and crosses into the next (the pair bookkeeping that must restart at t = 0)
    crossing = False
    for B, T, _, _ in S.mel_cases():
        ppc = S.cdiv(T, 2)
        for v in S.MEL_ROW_RUNS:
            ppw = S.mel_pairs_per_wave(B, T, v)
            assert ppw > 1 or v == 1
            for p0 in range(0, B * ppc, ppw):
                p1 = min(p0 + ppw, B * ppc)
                if p0 % ppc and (p1 - 1) // ppc > p0 // ppc:
                    crossing = True
    assert crossing
    assert any(T % 2 for _, T, _, _ in S.mel_cases()) and any(T % 2 == 0 for _, T, _, _ in S.mel_cases())


def test_512_forward_cases_reach_every_dispatch_condition():
    """The swept shapes give four of the conditions; the GPU file adds the rest as named cases (DISPATCH_EXTRA there
    must stay in step with this list)."""
    hit = set()
    for B, T, hop, center, L in S.forward_cases(512):
        hit |= S.forward_reason(512, hop, center, L=L)
    assert {"hop_not_128", "center_false"} <= hit
    named = {"phase_output", "L_lt_512", "odd_clip_stride", "unaligned_input", "unaligned_output", "variant_frame_kernels"}
    assert hit | named == S.FWD512_REASONS
    assert any(S.forward_kernel(512, hop, center, L=L) == "stft512_run_fwd_kernel" for _, _, hop, center, L in
               S.forward_cases(512))                                                   # the control
    assert {S.istft_kernel(512, hop) for _, _, hop in S.inverse_cases(512)} == {"istft512_ola_kernel", "irfft512_frames_kernel"}


def test_per_clip_metric_sees_a_quiet_clip():
    ref = np.stack([np.ones(8), 1e-4 * np.ones(8)])
    got = ref.copy()
    got[1, 3] *= 1.01
    per = S.rel_max_per_clip(got, ref)
    assert per[0] == 0 and abs(per[1] - 0.01) < 1e-9
    whole = np.abs(got - ref).max() / np.abs(ref).max()
    assert whole < 2e-6                                   # what conftest.rel_max would have reported


def test_packing_model():
    """The two facts the GPU tests lean on: a frame grouped with ZEROS meets 1e-5 with a wide margin at every K (so a
    clip under the per-clip grouping can meet it), and a frame whose mates are 1e4 louder does not (so the test's
    80 dB contrast tells the groupings apart)."""
    rng = np.random.default_rng(1)
    for K in (2, 4, 8):
        fr = rng.standard_normal((K, 1024 // K)).astype(np.float32)
        got = S.packed_rfft_model(fr)
        ref = np.fft.rfft(fr.astype(np.float64), axis=1)
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-6                     # the model is the transform
        alone = S.model_error(K, 0.0, zeros=True)
        equal = S.model_error(K, 1.0)
        loud2 = S.model_error(K, 1e2)
        loud4 = S.model_error(K, 1e4)
        print("K %d: mates zero %.2e, ratio 1 %.2e, 1e2 %.2e, 1e4 %.2e" % (K, alone, equal, loud2, loud4))
        assert alone < 5e-7 and equal < 1e-6
        assert 1e-6 < loud2 < 1e-4
        assert loud4 > 1e-4 > 10 * 1e-5 * 0.99

"""The plan sweeps of test_run_plans_gpu.py reach every run and tile geometry the launchers can cut (plan_cases.py
restates the cut).  CPU only: this turns the GPU file's coverage claims into checked facts."""
import plan_cases as P


def test_forced_run_length_clamps_like_the_library():
    assert P.forced_run_length(1, 100) == 8 and P.forced_run_length(8, 100) == 8 and P.forced_run_length(9, 100) == 9
    assert P.forced_run_length(P.ONE_RUN, 100) == 100 and P.forced_run_length(3, 5) == 5
    assert P.runs(17, 8) == [(0, 8), (8, 16), (16, 17)]
    assert P.runs(5, 8) == [(0, 5)]


def test_tile_share_rule():
    # v = 6: 21-frame tiles, waves of 6, 6, 6, 3; a 22-frame clip leaves a 1-frame last tile
    n, tile, tpc = P.tile_plan(22, 6)
    assert (n, tile, tpc) == (6, 21, 2)
    assert P.tile_waves(22, 6, 0) == [(0, 6, False), (6, 12, False), (12, 18, False), (18, 21, True)]
    assert P.tile_waves(22, 6, 1) == [(21, 22, True), (22, 22, True), (22, 22, True), (22, 22, True)]
    # a last tile of n + 1 frames: wave 0 closes its own hops (its successor holds 1 frame)
    assert P.tile_waves(21 + 7, 6, 1)[:2] == [(21, 27, True), (27, 28, True)]
    assert P.tile_plan(64, 1) == (6, 21, 4)                       # v < 6 means 6
    assert "self_cool_before_short_wave" in P.tile_classes(28, 6)


def test_tile_sweep_reaches_every_tile_geometry():
    hit = set()
    for v, T in P.TILE_SWEEP:
        assert T >= 64                                             # below 64 frames the tiles are never used
        hit |= P.tile_classes(T, v)
    assert P.TILE_CLASSES <= hit, sorted(P.TILE_CLASSES - hit)


def test_run_sweeps_reach_every_run_geometry():
    for (n_fft, hop), sweep in P.FWD_SWEEPS.items():
        hit = set()
        for v, T, L in sweep:
            assert T == 1 + L // hop and L % 4 == 0
            hit |= P.fwd_case_classes(n_fft, hop, v, T, L)
        want = set(P.RUN_CLASSES)
        if n_fft in (2048, 4096):
            want.discard("T<8")      # L >= n_fft: 5 frames at least, still a single short run
            assert any(T < 8 for _, T, _ in sweep)
        if n_fft == 512:
            want.discard("T<8")      # 8 pairs = 16 frames; the short clips are the single-run class
            want.add("half_pair")
        assert want <= hit, (n_fft, hop, sorted(want - hit))
    hit = set()
    for v, T, L in P.FUSED_SWEEP:
        hit |= P.fwd_case_classes(1024, 256, v, T, L)
    assert P.RUN_CLASSES <= hit, sorted(P.RUN_CLASSES - hit)
    hit = set()
    for v, T in P.INV_SWEEP:
        hit |= P.run_classes(T - 1, v)
    assert P.RUN_CLASSES - {"run_in_padded_tail"} <= hit, sorted(P.RUN_CLASSES - {"run_in_padded_tail"} - hit)


def test_forward_sweeps_reach_every_place_of_the_stream_wrap():
    """With the BATCH clips of the GPU sweeps, every forward sweep puts a wrap frame (global index 63 mod 64) first in a
    run, inside one and last in one; at n_fft 512 on either frame of a pair."""
    assert P.stream_classes(1024, 8, 64, B=1) == {"wrap_last_in_run"}                 # frame 63 closes the run [56, 64)
    assert P.stream_classes(1024, 13, 66, B=1) == {"wrap_inside_run"}                 # the run [52, 65)
    assert P.stream_classes(1024, 9, 64, B=1) == {"wrap_first_in_run", "wrap_last_in_run"}     # the run [63, 64)
    assert P.stream_classes(512, 8, 64, B=1) == {"wrap_last_in_run", "wrap_on_pair_second"}
    assert P.stream_classes(512, 8, 21, B=4) == {"wrap_first_in_run", "wrap_on_pair_first"}     # clip 3, frame 0
    for (n_fft, hop), sweep in P.FWD_SWEEPS.items():
        hit = set()
        for v, T, L in sweep:
            hit |= P.stream_classes(n_fft, v, T)
        want = P.STREAM_CLASSES_512 if n_fft == 512 else P.STREAM_CLASSES
        assert want <= hit, (n_fft, hop, sorted(want - hit))
    # FUSED_SWEEP stops at 3 x 20 frames, before the first wrap: the fused forms' wrap is not this sweep's subject
    assert not any(P.stream_classes(1024, v, T) for v, T, L in P.FUSED_SWEEP)


# ---- fused inverses at n_fft 512 / 2048 / 4096 --------------------------------------------------------------------------
def test_inverse_units_and_default_plan():
    # n_fft 512: pairs that hold a valid block; lead = 256 / hop blocks are trimmed at the front
    assert P.inverse_units(512, 128, 1379) == 689 and P.inverse_units(512, 256, 2) == 1 and P.inverse_units(512, 64, 2) == 1
    assert P.inverse_units(512, 256, 3) == 2 and P.inverse_units(512, 128, 3) == 1 and P.inverse_units(2048, 512, 345) == 344
    for n, h in P.INV_OTHER:
        lead = (n // 2) // h
        for T in range(2, 70):
            # every valid block lies in one of the pairs, and the last pair holds one
            units = P.inverse_units(n, h, T)
            if n == 512:
                first, last = lead // 2, lead // 2 + units - 1
                assert 2 * first <= lead and 2 * last <= lead + T - 2 <= 2 * last + 1
            for v in (8, 9, 13, P.ONE_RUN):
                P.inv_classes(n, h, v, T)                  # asserts that the runs store every hop exactly once
    assert P.default_inverse_plan(2048, 512, 1024, 345) == (344, 172, 2)
    assert P.default_inverse_plan(4096, 1024, 1024, 173) == (172, 86, 2)
    assert P.default_inverse_plan(512, 128, 1024, 1379) == (689, 173, 4)
    assert P.default_inverse_plan(2048, 512, 3, 5) == (4, 4, 1) and P.default_inverse_plan(512, 128, 3, 100) == (50, 16, 4)
    assert P.inverse_grid(3, 5) == 4 and P.inverse_grid(1024, 2) == 512


def test_inverse_sweeps_reach_every_run_geometry():
    assert set(P.INV_OTHER_SWEEPS) == set(P.INV_OTHER) and len(P.INV_OTHER) == 9
    for (n, h), sweep in P.INV_OTHER_SWEEPS.items():
        hit = set()
        for v, T in sweep:
            hit |= P.inv_classes(n, h, v, T)
        want = P.inv_want_classes(n, h)
        assert want <= hit, (n, h, sorted(want - hit))
        if n // h == 2:
            # the classes left out at hop n/2 do not exist there, whatever the clip
            assert not any(P.hop_is_partial(n, h, T, q) for T in range(2, 200) for q in range(T - 1))
        # the forcing can show: one cut that is neither the B = 3 default plan nor one run per clip
        assert any(1 < P.forced_inverse_plan(n, h, v, T)[2] and
                   P.forced_inverse_plan(n, h, v, T)[1:] != P.default_inverse_plan(n, h, 3, T)[1:] for v, T in sweep), (n, h)


def test_full_batches_land_on_the_long_run_plans_and_small_shapes_on_the_floor():
    for n, cases in P.INV_FULL_BATCH.items():
        h = n // 4
        (B1, L1), (B2, L2) = cases
        assert B1 == 1024 and L1 == 176400 and B2 == (4096 if n == 512 else 2048)
        units, per, nruns = P.default_inverse_plan(n, h, B1, 1 + L1 // h)
        assert nruns == (4 if n == 512 else 2) and per > 64 and units - (nruns - 1) * per > 64    # long runs, long last run
        assert P.default_inverse_plan(n, h, B2, 1 + L2 // h)[2] == 1
        # the forced 8-unit cut those outputs are compared with is a different plan
        assert P.forced_inverse_plan(n, h, 8, 1 + L1 // h)[1] == 8 and P.forced_inverse_plan(n, h, 8, 1 + L2 // h)[2] > 1
        # the record of the gap: every inverse launch of the size tests is runs of exactly the floor, or one run
        floor = 16 if n == 512 else 8
        for B, T, hop in P.INV_SMALL_SHAPES[n]:
            assert B <= 5
            units, per, nruns = P.default_inverse_plan(n, hop, B, T)
            assert per == floor or nruns == 1, (n, B, T, hop)


def test_two_pass_frame_plan():
    assert P.frames_per_block_2k_4k(15) == 4 and P.frames_per_block_2k_4k(8192) == 4 and P.frames_per_block_2k_4k(8193) == 8
    for n, h in P.TWO_PASS_HOPS:
        assert h not in (n // 8, n // 4, n // 2)            # no fused kernel takes these hops
    assert {n % h == 0 for n, h in P.TWO_PASS_HOPS} == {True, False}

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

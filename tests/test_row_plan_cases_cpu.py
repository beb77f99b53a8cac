"""The row-plan sweeps of test_row_plans_gpu.py store every element once and reach every geometry the projection
launchers can cut (row_plan_cases.py restates the cut and the channel-major store windows).  CPU only: this turns the GPU
file's coverage claims into checked facts."""
import row_plan_cases as P


def test_forced_cut_clamps_like_the_library():
    assert P.forced(0, 100) == 0 and P.forced(1, 100) == 1 and P.forced(P.ROW_RUN_MAX, 100) == 100
    assert P.banded_rows_per_wave(200, 4096) == 8 and P.banded_rows_per_wave(200, 4096, v=3) == 3
    assert P.banded_rows_per_wave(300_000, 4096) == 19                 # above the minimum only past 32 x slots rows
    assert P.small_row_rows_per_wave(4096) == 4 and P.small_row_rows_per_wave(40_000) == 5
    assert P.small_mfma_rows_per_wave(4096) == 64 and P.small_mfma_rows_per_wave(4096, v=1) == 32
    assert P.small_mfma_rows_per_wave(4096, v=33) == 64 and P.small_mfma_rows_per_wave(706_560) == 192
    assert P.stft512_pairs_per_wave(4, 250) == 4 and P.stft512_pairs_per_wave(4, 250, v=1) == 1
    assert P.stft512_pairs_per_wave(4, 7, v=99) == 16                  # an odd-T clip has ceil(T / 2) pairs
    assert P.stft2048_frames_per_wave(1000) == 8 and P.stft2048_frames_per_wave(100_000) == 13
    assert P.gemm_tiles_per_block(200, 128) == 1 and P.gemm_tiles_per_block(20_000, 128) == 3
    assert P.gemm_tiles_per_block(200, 128, v=4) == 4 and P.gemm_tiles_per_block(200, 128, v=99) == 7
    assert P.bf16_grid(1000) == 8 and P.bf16_grid(1000, v=3) == 3 and P.bf16_grid(50_000) == 256
    assert P.frame_runs_512(1, 7, 2) == [(0, 4), (4, 7)]
    assert P.frame_runs_512(2, 3, 3) == [(0, 5), (5, 6)]              # pairs (0,1) (2,-) (3,4) | (5,-)


def test_channel_major_window_stores_every_element_once():
    """mel_banded_kernel CMW 1 / 2 and stft2048_mel_kernel (runs of rows / frames) and stft512_mel_kernel (runs of frame
    pairs): every swept cut, every residue of a lane's output row."""
    N = 40
    lanes = P.representative_filters(N)
    for B, T, v in P.CM_SWEEP + [(B, T, P.ROW_RUN_MAX) for B, T, _ in P.CM_SWEEP[::len(P.V_ROWS)]]:
        rr = P.runs(B * T, P.forced(v, B * T))
        w = []
        for f in lanes:
            w += P.cm_window(T, N, f, rr)[0]
        P.check_once(w, B, N, T, lanes)
    for B, T, v in P.S512_SWEEP:
        rr = P.frame_runs_512(B, T, P.stft512_pairs_per_wave(B, T, v))
        assert rr[0][0] == 0 and rr[-1][1] == B * T and all(a[1] == b[0] for a, b in zip(rr, rr[1:]))
        w = []
        for f in lanes:
            w += P.cm_window(T, N, f, rr)[0]
        P.check_once(w, B, N, T, lanes)


def test_small_row_window_stores_every_element_once():
    N = 13
    for B, T, v in P.CM_SWEEP:
        rr = P.runs(B * T, P.small_row_rows_per_wave(B * T, v))
        w = []
        for lane in range(N):
            w += P.small_row_window(T, N, lane, rr)[0]
        P.check_once(w, B, N, T, range(N))


def test_full_flush_is_always_the_float4_form():
    """A lane holds 8 frames only when its 8th one ends a 32-byte sector of the output row (e % 8 == 0): the scalar
    8-frame store of the window ((e & 3) != 0) is unreachable under any cut, so no sweep can (or needs to) reach it."""
    for B, T, v in P.CM_SWEEP:
        rr = P.runs(B * T, P.forced(v, B * T))
        for f in range(8):
            assert all(kind != "scalar8" for kind, _, _ in P.cm_window(T, 128, f, rr)[1])


def test_channel_major_sweeps_reach_every_geometry():
    hit = P.cm_cases_classes(P.CM_SWEEP)
    assert P.RUN_CLASSES <= hit, sorted(P.RUN_CLASSES - hit)
    assert P.CM_CLASSES <= hit, sorted(P.CM_CLASSES - hit)
    hit = P.cm_cases_classes(P.CM_SWEEP, window="small", N=40)
    assert P.SMALL_CM_CLASSES <= hit, sorted(P.SMALL_CM_CLASSES - hit)
    hit = set()
    for B, T, v in P.S512_SWEEP:
        ppw = P.stft512_pairs_per_wave(B, T, v)
        rr = P.frame_runs_512(B, T, ppw)
        hit |= P.pair_classes(B, T, ppw) | P.run_geometry(T, rr)
        for f in P.representative_filters(128):
            hit |= P.cm_window(T, 128, f, rr)[1]
    assert P.PAIR_CLASSES <= hit, sorted(P.PAIR_CLASSES - hit)
    want = P.CM_CLASSES | (P.RUN_CLASSES - {"run_1", "len_mod4_1", "len_mod4_3", "last_wave_1"})   # runs of whole pairs
    assert want <= hit, sorted(want - hit)


def test_row_major_sweep_reaches_every_run_length():
    hit = set()
    for rows, v in P.ROW_SWEEP:
        hit |= P.run_geometry(rows, P.runs(rows, P.forced(v, rows)))
    want = {"run_1", "len_mod4_0", "len_mod4_1", "len_mod4_2", "len_mod4_3", "last_wave_1"}
    assert want <= hit, sorted(want - hit)


def test_mfma_sweep_reaches_every_tile_pair_count():
    hit = set()
    for B, T, v in P.MFMA_SWEEP:
        rpw = P.small_mfma_rows_per_wave(B * T, v=v)
        assert rpw % 32 == 0
        rr = P.runs(B * T, rpw)
        hit |= {"pairs_%d" % min(-(-(b - a) // 32), 3) for a, b in rr} | P.run_geometry(T, rr)
    want = {"pairs_1", "pairs_2", "pairs_3", "start_mid", "end_mid", "spans_2_boundaries", "T1"}
    assert want <= hit, sorted(want - hit)


def test_gemm_flag_ring_marks_every_poisoned_tile():
    """The three-slot ring is right for every poison pattern of blocks up to 7 tiles; a ring that clears the slot it is
    about to read (reset offset 0) is not, and the GPU sweep's poison cases tell the two apart."""
    for n in range(1, 10):
        for mask in range(1 << n):
            bad = [(mask >> i) & 1 for i in range(n)]
            for tpb in (1, 2, 3, 4, 7):
                assert {i for i in range(n) if bad[i]} <= P.gemm_dense_tiles(bad, tpb)
    caught = False
    for tiles, v, poisoned in P.GEMM_POISON:
        bad = [int(i in poisoned) for i in range(tiles)]
        caught |= not set(poisoned) <= P.gemm_dense_tiles(bad, v, reset=0)
    assert caught


def test_gemm_sweeps_reach_every_block_geometry():
    hit = set()
    for rows, v in P.GEMM_SWEEP:
        hit |= P.gemm_classes(-(-rows // 32), P.forced(v, -(-rows // 32)))
    assert P.GEMM_CLASSES <= hit, sorted(P.GEMM_CLASSES - hit)
    hit = set()
    for tiles, v, bad in P.GEMM_POISON:
        hit |= P.gemm_classes(tiles, v, bad)
    assert P.GEMM_BAD_CLASSES <= hit, sorted(P.GEMM_BAD_CLASSES - hit)


def test_bf16_sweep_takes_several_trips():
    trips = set()
    for rows, v in P.BF16_SWEEP:
        tiles = -(-rows // 128)
        gx = P.bf16_grid(rows, v=v)
        trips |= {-(-(tiles - b) // gx) for b in range(gx)}
    assert {1, 2, 3} <= trips

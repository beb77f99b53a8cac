"""The cases of test_frame_walk_gpu.py reach every walk shape of the fallback STFT kernels, every stage kind of their
radix plans with and without a twiddle table, and both forms of the overlap-add gather (frame_walk_cases.py restates the
launch arithmetic).  CPU only: this turns the GPU file's coverage claims into checked facts."""
import frame_walk_cases as W


def test_radix_plans_follow_the_stated_rule():
    assert W.radix_plan(1) == [] and W.radix_plan(2) == [2] and W.radix_plan(3) == [3] and W.radix_plan(4) == [4]
    assert W.radix_plan(8) == [4, 2] and W.radix_plan(200) == [4, 2, 5, 5] and W.radix_plan(127) == [127]
    assert W.radix_plan(441) == [3, 3, 7, 7] and W.radix_plan(4802) == [2, 7, 7, 7, 7] and W.radix_plan(6561) == [3] * 8
    assert W.radix_plan(6000) == [4, 4, 3, 5, 5, 5] and W.radix_plan(8191) == [8191]
    for M in range(1, 3000):
        plan, prod = W.radix_plan(M), 1
        for p in plan:
            prod *= p
        odd = [p for p in plan if p & 1]
        assert prod == M and len(plan) <= 16 and odd == sorted(odd) and plan.count(2) <= 1
        assert plan == sorted(plan, key=lambda p: (p != 4, p != 2)), M       # fours, a two, then the rest
    assert W.fft_length(400) == 200 and W.fft_length(441) == 441
    assert W.stockham_stages(8) == [4] and W.stockham_stages(16) == [2, 4] and W.stockham_stages(64) == [2, 4, 4]
    assert W.stockham_stages(8192) == [4] * 6 and W.stockham_stages(16384) == [2] * 13


def test_dispatch_of_the_table_sizes():
    for c in W.CASES:
        assert W.kernel_of(c.n_fft, c.window_alignment) == c.kernel, c.name
        assert c.L > c.n_fft // 2 and W.frames_of(c.n_fft, c.hop, c.L) == c.T, c.name
        assert c.hop == 1 or c.L % c.hop, c.name
        assert c.hop <= max(c.n_fft // 2, 1), c.name                    # the asymmetric window satisfies NOLA there
        if c.window_alignment == 4:
            assert W.kernel_of(c.n_fft) == "register"                     # the aligned window is the control
    for kernel, n, hop, L, stride, T in W.UNCENTRED:
        assert W.kernel_of(n) == kernel and stride > L and (T - 1) * hop < L < (T - 1) * hop + n
    for kernel, n, hop in W.SHORTEST:
        L = n // 2 + 1
        assert W.kernel_of(n) == kernel and W.frames_of(n, hop, L) >= 3
        assert hop - n // 2 < 0 and hop - n // 2 + n > L                # frame 1 reflects at both ends of the clip
    assert {k for k, *_ in W.SHORTEST} == {"generic", "mixed"} and {n & 1 for k, n, _ in W.SHORTEST if k == "mixed"} == {0, 1}
    assert {k for k, *_ in W.UNCENTRED} == {"generic", "mixed"}


def test_only_8192_needs_the_lds_limit_raised():
    sizes = [n for n in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192) if W.generic_has_table(n)]
    over = [n for n in sizes if W.generic_lds_bytes(n) > W.LDS_DEFAULT_LIMIT]
    assert over == [8192] and W.generic_lds_bytes(8192, inverse=True) <= 160 * 1024
    assert W.generic_lds_bytes(16384) > W.LDS_DEFAULT_LIMIT and not W.generic_has_table(16384)
    assert 8192 in {c.n_fft for c in W.CASES if c.kernel == "generic"}


def test_walks_reach_every_shape():
    assert W.walkers(21) == 21 and W.walkers(6003) == 4096 and W.walkers(21, 4) == 4 and W.walkers(21, W.ONE_TRIP) == 21
    assert W.trips(21, 4, 0) == [0, 4, 8, 12, 16, 20] and W.trips(21, 4, 3) == [3, 7, 11, 15, 19]
    assert W.trips(6003, 0, 1906) == [1906, 6002] and W.trips(6003, 0, 1907) == [1907]
    want = {"trips_3", "ragged_last_trip", "v=1", "v=N-1", "v>=N", "v=65535", "walker_crosses_clips"}
    for kernel in ("generic", "mixed"):
        hit = set()
        for c in W.CASES:
            if c.kernel == kernel:
                assert W.ONE_TRIP >= c.B * c.T
                for v in W.plans(c):
                    hit |= W.walk_classes(c.B, c.T, v)
        assert want <= hit, (kernel, sorted(want - hit))
    for c in W.CASES:                                                     # every case on its own walks 3+ trips raggedly
        hit = set().union(*(W.walk_classes(c.B, c.T, v) for v in W.plans(c)))
        assert {"trips_3", "ragged_last_trip", "walker_crosses_clips", "v=N-1"} <= hit, c.name
    for kernel, n, hop, B, L in W.ACROSS_CAP:                             # the default plan itself, past its cap
        T = W.frames_of(n, hop, L)
        assert W.kernel_of(n) == kernel and B * T == 6003
        assert {"ragged_last_trip", "walker_crosses_clips", "trips_2"} <= W.walk_classes(B, T, 0)
    assert {k for k, *_ in W.ACROSS_CAP} == {"generic", "mixed"}


def test_every_stage_kind_with_and_without_the_table():
    kinds = {True: set(), False: set()}
    empty = False
    for c in W.CASES:
        if c.kernel == "mixed":
            plan = W.radix_plan(W.fft_length(c.n_fft))
            empty |= plan == []
            kinds[W.mixed_has_table(c.n_fft)] |= {W.stage_kind(p) for p in plan}
    assert empty
    assert kinds[True] == {2, 3, 4, 5, 7, "prime"}, kinds[True]
    assert kinds[False] == {2, 3, 4, 5, 7, "prime"}, kinds[False]
    assert {c.n_fft & 1 for c in W.CASES if c.kernel == "mixed" and not W.mixed_has_table(c.n_fft)} == {0, 1}
    forms = set()
    for c in W.CASES:
        if c.kernel == "generic":
            st = W.stockham_stages(c.n_fft)
            forms.add("no_table_radix2" if not W.generic_has_table(c.n_fft) else
                      "radix2_first" if st[0] == 2 else "pure_radix4")
    assert forms == {"no_table_radix2", "radix2_first", "pure_radix4"}
    assert {c.n_fft for c in W.CASES if c.window_alignment == 4} == {128, 1024, 2048}


def test_gather_cases_reach_both_forms_and_three_strides():
    assert W.gather_float4(64, 16) and not W.gather_float4(30, 7) and not W.gather_float4(254, 84)
    assert W.gather_units(3, 7, 441, 147) == 3 * (147 * 6 + 1) and W.gather_units(2, 4, 8192, 2048) == 2 * 2048 * 3 // 4
    assert W.gather_blocks(600) == 3 and W.gather_blocks(600, 1) == 1 and W.gather_strides(600, 1) == 3
    assert W.gather_blocks(1 << 30) == W.GATHER_CAP
    hit = {"float4": set(), "scalar": set()}
    for c in W.CASES:
        for v in W.plans(c):
            cl = W.gather_classes(c, v)
            hit["float4" if "float4" in cl else "scalar"] |= cl
    assert "strides_3" in hit["float4"] and "strides_3" in hit["scalar"]
    assert {"hop_does_not_divide", "odd_n_fft"} <= hit["scalar"]
    # the float4 cases are also run through the scalar kernel (an output 4 bytes off): three strides there too
    assert any(W.gather_strides(W.gather_units(c.B, c.T, c.n_fft, c.hop, float4=False), 1) >= 3
               for c in W.CASES if W.gather_float4(c.n_fft, c.hop))

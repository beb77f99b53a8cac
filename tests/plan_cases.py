"""The launchers' cut of a clip into per-wave runs and workgroup tiles, restated for the CPU, and the sweeps of
test_run_plans_gpu.py that force those cuts through the plan variants (AT_VARIANT_RUN_LENGTH, AT_VARIANT_ISTFT_TILE).

test_plan_cases_cpu.py checks that the sweeps reach every geometry class named here; the GPU file runs them.  The
arithmetic follows csrc/run_plan.h (forced_units_per_run), csrc/stft1024.hip (launch_istft1024_ola and the share() /
self_cool rule of istft1024_tile_kernel) and launch_istft512_ola / launch_istft2048_ola / launch_istft4096_ola."""

TILE_WAVES = 4          # waves per workgroup of the tile kernel
ONE_RUN = 65535         # AT_VARIANT_RUN_LENGTH value that clamps to one run per clip


def forced_run_length(v, units):
    """forced_units_per_run: v clamped to [8, units] (all of a clip shorter than 8 units is one run)."""
    if v > units:
        return units
    return v if v >= 8 else min(units, 8)


def runs(units, v):
    """[(start, stop)] of one clip's runs, in units."""
    upr = forced_run_length(v, units)
    return [(a, min(a + upr, units)) for a in range(0, units, upr)]


def tail_start(n_fft, hop, L):
    """First frame whose window reaches past the clip's end into torch.stft's reflect padding."""
    t = 0
    while t * hop + n_fft // 2 <= L:
        t += 1
    return t


def run_classes(units, v, tail_unit=None, half_pair=False):
    """Geometry classes of a forward / inverse run plan: units per clip, forced run length v, the first unit in the
    padded tail (forward only), whether the clip's last unit is half a frame pair (n_fft 512, odd T)."""
    rs = runs(units, v)
    last = rs[-1][1] - rs[-1][0]
    c = set()
    if units < 8:
        c.add("T<8")
    if len(rs) == 1:
        c.add("single_run")
    else:
        c.add("last_run_full" if last == rs[0][1] - rs[0][0] else "last_run_%d" % last if last <= 7 else "last_run_long")
    if tail_unit is not None and len(rs) > 1 and rs[-1][0] >= tail_unit:
        c.add("run_in_padded_tail")
    if half_pair:
        c.add("half_pair")
    return c


def tile_plan(T, v):
    """Forced tile plan: frames per wave n = max(v, 6), 4n - 3 frames per tile, no balancing."""
    n = max(v, 6)
    tile = TILE_WAVES * n - 3
    return n, tile, (T + tile - 1) // tile


def tile_waves(T, v, k):
    """[(ta, tb, self_cool)] of tile k's waves (istft1024_tile_kernel's share() and self_cool)."""
    n, tile, _ = tile_plan(T, v)
    tile0, tile1 = k * tile, min(k * tile + tile, T)

    def share(w):
        a = min(tile0 + w * n, tile1)
        e = tile1 if w == TILE_WAVES - 1 else min(a + n, tile1)
        return a, e
    out = []
    for w in range(TILE_WAVES):
        a, e = share(w)
        cool = True
        if w < TILE_WAVES - 1:
            a2, e2 = share(w + 1)
            cool = e2 - a2 < 3
        out.append((a, e, cool))
    return out


def tile_classes(T, v):
    n, tile, tpc = tile_plan(T, v)
    c = set()
    last = T - (tpc - 1) * tile
    c.add("last_tile_%d" % last if last <= 3 else "last_tile_ge4")
    waves = tile_waves(T, v, tpc - 1)
    end_wave = [w for w, (a, e, _) in enumerate(waves) if a <= T - 1 < e][0]
    c.add("end_in_wave_%d" % end_wave)
    for k in range(tpc):
        ws = tile_waves(T, v, k)
        for w, (a, e, cool) in enumerate(ws):
            if e - a <= 2:
                c.add("wave_holds_%d" % (e - a))
            if w < TILE_WAVES - 1 and cool and e > a and 1 <= ws[w + 1][1] - ws[w + 1][0] <= 2:
                c.add("self_cool_before_short_wave")
    if tpc == 1:
        c.add("single_tile")
    if tpc >= 3:
        c.add("three_tiles")
    return c


TILE_CLASSES = {"last_tile_1", "last_tile_2", "last_tile_3", "last_tile_ge4", "end_in_wave_0", "end_in_wave_1",
                "end_in_wave_2", "end_in_wave_3", "wave_holds_0", "wave_holds_1", "wave_holds_2",
                "self_cool_before_short_wave", "single_tile", "three_tiles"}
RUN_CLASSES = {"T<8", "single_run", "last_run_full", "run_in_padded_tail"} | {"last_run_%d" % i for i in range(1, 8)}

# ---- the sweeps -------------------------------------------------------------------------------------------------------
# tiled inverse (T >= 64): every remainder of a 21-, 25- and 33-frame tile, single tiles that end in each wave
TILE_SWEEP = ([(6, T) for T in range(64, 85)] + [(7, T) for T in range(100, 125)] + [(9, T) for T in range(66, 99)] +
              [(20, T) for T in (64, 70, 75, 77)] + [(40, T) for T in (64, 80, 81, 82, 83, 120, 121, 157)] +
              [(70, T) for T in (64, 70)] + [(8, 300)])


def fwd_sweep(n_fft, hop, v_list=(8, 9, 13), T_list=None):
    """[(v, T, L)] for a forward run plan: clips of L samples (a multiple of 4), T = 1 + L // hop frames; L just past a
    hop boundary and just short of the next one, so the padded tail holds the most and the fewest frames."""
    if T_list is None:
        T_list = list(range(3, 27)) + [40, 41]
    out = []
    for T in T_list:
        for L in (hop * (T - 1) + 4, hop * T - 4):
            if L <= n_fft // 2 or (n_fft > 1024 and L < n_fft) or (n_fft == 512 and L < 512):
                continue
            for v in v_list:
                out.append((v, T, L))
    return out


FWD_SWEEPS = {
    (1024, 128): fwd_sweep(1024, 128),
    (1024, 256): fwd_sweep(1024, 256),
    (1024, 512): fwd_sweep(1024, 512),
    (2048, 512): fwd_sweep(2048, 512),
    (4096, 1024): fwd_sweep(4096, 1024),
    (512, 128): fwd_sweep(512, 128, T_list=list(range(5, 40)) + [57, 58]),
}
# the fused forward forms (each a kernel of its own): fewer lengths, same classes
FUSED_SWEEP = fwd_sweep(1024, 256, v_list=(8, 11), T_list=list(range(3, 21)))

# long-run inverse: units are the T - 1 hop slots
INV_SWEEP = [(v, T) for T in list(range(2, 26)) + [40, 64, 65] for v in (8, 9, 13)]


def fwd_case_classes(n_fft, hop, v, T, L):
    if n_fft == 512:
        pairs = (T + 1) // 2
        return run_classes(pairs, v, tail_unit=(tail_start(n_fft, hop, L) + 1) // 2, half_pair=T % 2 == 1)
    return run_classes(T, v, tail_unit=tail_start(n_fft, hop, L))


# ---- the aligned row stream of the sliding forwards (csrc/row_stream.h) -----------------------------------------------------
# The spectrum's rows leave as one stream of 64-element blocks, rotated by the global frame index g = b T + t mod 64; the
# frame with g = 63 (mod 64) ends on a block boundary and stores one block more -- the wrap.  Where it falls in a run
# (first frame: on the masked head block; last: an empty carry at the end) depends on the clip's place in the batch, so
# the classes are taken over the BATCH clips the GPU sweeps run.  At n_fft 512 a run is frame pairs and the wrap falls on
# a pair's first or second frame (the one moved up a lane).
BATCH = 3
STREAM_CLASSES = {"wrap_first_in_run", "wrap_inside_run", "wrap_last_in_run"}
STREAM_CLASSES_512 = STREAM_CLASSES | {"wrap_on_pair_first", "wrap_on_pair_second"}


def stream_classes(n_fft, v, T, B=BATCH):
    """Where the wrap frames of B clips of T frames fall in the runs of the forced length v."""
    per = 2 if n_fft == 512 else 1                      # frames per unit
    c = set()
    for b in range(B):
        for a, e in runs((T + per - 1) // per, v):
            t0, t1 = per * a, min(per * e, T)
            for t in range(t0, t1):
                if (b * T + t) % 64 != 63:
                    continue
                if t == t0:
                    c.add("wrap_first_in_run")
                if t == t1 - 1:
                    c.add("wrap_last_in_run")
                if t0 < t < t1 - 1:
                    c.add("wrap_inside_run")
                if n_fft == 512:
                    c.add("wrap_on_pair_second" if t % 2 else "wrap_on_pair_first")
    return c


# ---- fused inverses at n_fft 512 / 2048 / 4096 (istft512_ola_kernel, istft2048_ola_kernel, istft4096_ola_kernel) ---------
# R = n_fft / hop frames overlap a hop; output hop q is block c = q + lead, summed from frames c - R + 1 .. c; the first
# lead = R / 2 blocks are torch.istft's trimmed front.  Units: output hops at 2048 / 4096, frame pairs at 512 (pair i holds
# frames 2 i, 2 i + 1 and completes blocks 2 i, 2 i + 1; the first pair of a clip is pair lead // 2).
INV_OTHER = [(n, n // d) for n in (512, 2048, 4096) for d in (8, 4, 2)]
INV_WAVES_PER_BLOCK = 4     # W5, W2K, W4K


def inverse_units(n_fft, hop, T):
    """Units per clip of the launcher: T - 1 output hops, or the frame pairs that hold a valid block at n_fft 512."""
    if n_fft == 512:
        lead = 256 // hop
        return (lead + T) // 2 - lead // 2
    return T - 1


def default_inverse_plan(n_fft, hop, B, T):
    """(units, per, runs) of the launcher's own plan: from the batch size alone, with a floor of 8 hops / 16 pairs."""
    units = inverse_units(n_fft, hop, T)
    full, floor = (4096, 16) if n_fft == 512 else (2048, 8)
    runs = 1 if B >= full else (full + B - 1) // B
    per = (units + runs - 1) // runs
    if per < floor:
        per = min(floor, units)
    per = max(per, 1)
    return units, per, (units + per - 1) // per


def forced_inverse_plan(n_fft, hop, v, T):
    units = inverse_units(n_fft, hop, T)
    per = forced_run_length(v, units)
    return units, per, (units + per - 1) // per


def inverse_grid(B, runs):
    """Workgroups of the launch: one wave per run, four waves per workgroup."""
    return (B * runs + INV_WAVES_PER_BLOCK - 1) // INV_WAVES_PER_BLOCK


def hop_is_partial(n_fft, hop, T, q):
    """Output hop q lacks one of its R frames (clip start or end): the divided-envelope store."""
    R = n_fft // hop
    c = q + R // 2
    return c - (R - 1) < 0 or c > T - 1


def run_hops(n_fft, hop, T, a, b):
    """The valid output hops that the run of units [a, b) stores."""
    if n_fft != 512:
        return list(range(a, b))
    lead = 256 // hop
    out = []
    for i in range(lead // 2 + a, lead // 2 + b):
        out += [c - lead for c in (2 * i, 2 * i + 1) if lead <= c < lead + T - 1]
    return out


def inv_classes(n_fft, hop, v, T):
    """Geometry classes of one forced cut of a fused 512 / 2048 / 4096 inverse."""
    R = n_fft // hop
    units = inverse_units(n_fft, hop, T)
    rs = runs(units, v)
    per, last = rs[0][1] - rs[0][0], rs[-1][1] - rs[-1][0]
    hops = [run_hops(n_fft, hop, T, a, b) for a, b in rs]
    assert sorted(sum(hops, [])) == list(range(T - 1))             # the runs store every hop exactly once
    c = set()
    if len(rs) == 1:
        c.add("single_run_lt8" if units < 8 else "single_run_ge8")
    else:
        c.add("last_run_full" if last == per else "last_run_%d" % last if last <= 7 else "last_run_long")
        if all(hop_is_partial(n_fft, hop, T, q) for q in hops[-1]):
            c.add("last_run_partial_hops_only")
    if all(hop_is_partial(n_fft, hop, T, q) for q in range(T - 1)):
        c.add("every_hop_partial")
    # R - 1 warm-up frames before a run's first hop: with T - 1 <= R - 1 they reach before frame 0 for every hop
    c.add("T-1<R-1" if T < R else "T-1==R-1" if T == R else "T-1>R-1")
    if n_fft == 512:
        lead = 256 // hop
        c.add("T_odd" if T % 2 else "T_even")                       # odd: frame T - 1 is half a pair
        one_block = (lead + T - 1) % 2 == 1                         # the last pair completes one valid block only
        c.add("last_pair_one_block" if one_block else "last_pair_two_blocks")
        if lead % 2:
            c.add("first_pair_opens_trimmed")                       # hop 256: block 0 of pair 0 is trimmed
        if len(rs) > 1 and last == 1:
            if T % 2:
                c.add("run_starts_at_half_frame_pair")
            if one_block:
                c.add("run_starts_at_one_block_pair")
    return c


def inv_want_classes(n_fft, hop):
    """What a sweep must reach.  At hop n/2 (R = 2) no hop is ever partial (block q + 1 is frames q, q + 1) and
    T - 1 < R - 1 would be a clip without output: those classes do not exist there."""
    R = n_fft // hop
    want = {"single_run_lt8", "single_run_ge8", "last_run_full", "last_run_long", "T-1==R-1", "T-1>R-1"}
    want |= {"last_run_%d" % i for i in range(1, 8)}
    if R > 2:
        want |= {"last_run_partial_hops_only", "every_hop_partial", "T-1<R-1"}
    if n_fft == 512:
        want |= {"T_odd", "T_even", "last_pair_one_block", "last_pair_two_blocks", "run_starts_at_half_frame_pair",
                 "run_starts_at_one_block_pair"}
        if hop == 256:
            want.add("first_pair_opens_trimmed")
    return want


def inv_other_sweep(n_fft, v_list=(8, 9, 13)):
    """[(v, T)]: every frame count up to three forced runs of the longest v, and two long clips."""
    T_list = list(range(2, 58)) + [80, 81] if n_fft == 512 else list(range(2, 29)) + [40, 41]
    return [(v, T) for T in T_list for v in v_list]


INV_OTHER_SWEEPS = {(n, h): inv_other_sweep(n) for n, h in INV_OTHER}

# The full-batch cases of test_run_plans_gpu.py (hop n/4): (B, samples per clip).  1024 clips of 4 s are what bench.py
# times under other_sizes; the second batch is the smallest that gets one run per clip (1 s clips: the plan looks at B only).
INV_FULL_BATCH = {512: [(1024, 176400), (4096, 44100)], 2048: [(1024, 176400), (2048, 44100)],
                  4096: [(1024, 176400), (2048, 44100)]}
# (B, T, hop) of the inverse launches the size tests of test_stft_gpu.py make at these sizes: the (B, L, h) list of
# test_register_core_sizes_512_and_2048 (T = 1 + L // h), test_every_power_of_two_size (2 clips of max(3 n, 2000) samples)
# and the 13-frame goldens of test_other_sizes_golden
INV_SMALL_SHAPES = {n: [(3, 1 + (9 * n + 7) // (n // 4), n // 4), (5, 1 + 4 * n // (n // 2), n // 2),
                        (2, 1 + (7 * n + 2) // (n // 8), n // 8), (1, 1 + 20 * n // (n // 4), n // 4), (2, 13, n // 4)] +
                       [(2, 1 + max(3 * n, 2000) // (n // d), n // d) for d in (8, 4, 2)]
                    for n in (512, 2048, 4096)}


# two-pass inverse at 2048 / 4096 (irfft2048_frames_kernel / irfft4096_frames_kernel + the overlap-add gather): hops that
# no fused kernel takes -- n/16, and hops that do not divide n_fft
TWO_PASS_HOPS = [(2048, 128), (2048, 300), (2048, 333), (4096, 256), (4096, 700)]


def frames_per_block_2k_4k(nframes):
    """units_per_block(nframes, 4) of run_plan.h: at most 2048 workgroups of four waves, whole rounds of the waves."""
    fpb = (nframes + 2047) // 2048
    return max((fpb + 3) // 4 * 4, 4)

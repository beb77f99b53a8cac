"""The launchers' cut of a clip into per-wave runs and workgroup tiles, restated for the CPU, and the sweeps of
test_run_plans_gpu.py that force those cuts through the plan variants (AT_VARIANT_RUN_LENGTH, AT_VARIANT_ISTFT_TILE).

test_plan_cases_cpu.py checks that the sweeps reach every geometry class named here; the GPU file runs them.  The
arithmetic follows csrc/run_plan.h (forced_units_per_run) and csrc/stft1024.hip (launch_istft1024_ola and the share() /
self_cool rule of istft1024_tile_kernel)."""

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

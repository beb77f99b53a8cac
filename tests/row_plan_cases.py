"""The projection launchers' row cut, restated for the CPU, the channel-major store windows that depend on it, and the
sweeps of test_row_plans_gpu.py that force the cut through AT_VARIANT_ROW_RUN.

Every launcher below sets its rows per wave (or tiles per workgroup) from the row count and the device; at the sizes of
the suite each one falls back to its minimum cut.  The variant replaces the plan by v (csrc/variants.h forced_row_run:
v clamped to [1, total]).  test_row_plan_cases_cpu.py checks with the models here that every element is stored exactly
once under every swept cut, and that the sweeps reach every geometry class named here; the GPU file runs them.

The arithmetic follows csrc/mel_banded.hip (launch_banded, launch_fixed_proj, at_project_small, the `held` / `e_next` /
`last_of_run` window of mel_banded_kernel and the `(t & 7) == 7` / `run_t0` window of small_proj_kernel), stft512.hip
(launch_stft512_mel, the same window over the frame pairs of each clip), stft2048.hip (launch_stft2048_mel), mel.hip (launch_mel and the
three-slot non-finite flag ring of mel_gemm_kernel) and mel_bf16.hip (at_mel_project_bf16)."""

ROW_RUN_MAX = 65535     # AT_VARIANT_ROW_RUN value that clamps to the whole launch (one run, one block)
GEMM_ROWS = 32          # rows of a dense-GEMM tile
BF16_ROWS = 128         # rows of a bf16 tile


def cdiv(a, b):
    return -(-a // b)


def forced(v, total):
    """forced_row_run: v clamped to [1, total]; 0 keeps the launcher's plan."""
    return 0 if v <= 0 else min(v, max(total, 1))


# ---- default and forced cuts ------------------------------------------------------------------------------------------
def banded_rows_per_wave(rows, slots, v=0):
    """launch_banded / launch_fixed_proj: a few whole rounds of the kernel's resident waves, at least 8 rows."""
    return forced(v, rows) or max(8, cdiv(rows, 4 * slots))


def small_row_rows_per_wave(rows, v=0):
    """at_project_small, row form (small_proj_kernel): 8192 waves, at least 4 rows."""
    return forced(v, rows) or max(4, cdiv(rows, 8192))


def small_mfma_rows_per_wave(rows, cus=256, v=0):
    """at_project_small, matrix-core form: 16 waves per CU, whole 32-row tile pairs, at least two pairs."""
    f = forced(v, rows)
    if f:
        return cdiv(f, 32) * 32
    return max(64, cdiv(cdiv(rows, 16 * cus), 32) * 32)


def stft512_pairs_per_wave(B, T, v=0):
    """launch_stft512_mel: frame pairs per wave, at least 4.  Pairs are formed per clip (frames 2 i, 2 i + 1 of one
    clip; the last frame of an odd-T clip is paired with zeros): B * ceil(T / 2) of them."""
    pairs = B * cdiv(T, 2)
    return forced(v, pairs) or max(4, cdiv(pairs, 256 * 8 * 4))


def stft2048_frames_per_wave(frames, v=0):
    """launch_stft2048_mel: frames per wave, at least 8."""
    return forced(v, frames) or max(8, cdiv(frames, 256 * 8 * 4))


def gemm_tiles_per_block(rows, N, cus=256, v=0):
    """launch_mel: one row block per CU and column block, tiles split evenly."""
    ntiles = cdiv(rows, GEMM_ROWS)
    f = forced(v, ntiles)
    if f:
        return f
    rowblocks = min(max(cus // cdiv(N, 128), 1), ntiles)
    return cdiv(ntiles, rowblocks)


def bf16_grid(rows, cus=256, v=0):
    """at_mel_project_bf16: persistent workgroups over 128-row tiles (workgroup b takes tiles b, b + gx, ..)."""
    tiles = cdiv(rows, BF16_ROWS)
    f = forced(v, tiles)
    return cdiv(tiles, f) if f else min(tiles, cus)


def runs(total, per):
    """[(start, stop)] of the waves' runs over `total` units, `per` units each."""
    return [(a, min(a + per, total)) for a in range(0, total, per)]


def frame_runs_512(B, T, ppw):
    """stft512_mel_kernel: a wave takes pairs [p0, p1) of the per-clip pair list (pair p = clip p // ppc, frames 2 i and
    2 i + 1 of it, i = p % ppc, ppc = ceil(T / 2)): flat frames from the first frame of pair p0 to the last existing
    frame of pair p1 - 1.  The frames of a run stay consecutive."""
    ppc = cdiv(T, 2)

    def first(p):
        return (p // ppc) * T + 2 * (p % ppc)
    return [(first(a), (b - 1) // ppc * T + min(2 * ((b - 1) % ppc) + 2, T)) for a, b in runs(B * ppc, ppw)]


# ---- channel-major store windows --------------------------------------------------------------------------------------
def cm_window(T, N, f, frame_runs):
    """The register window of mel_banded_kernel (CMW 1 / 2), stft512_mel_kernel and stft2048_mel_kernel for the lane that
    holds filter f, over runs of flat frame indices r = b T + t.  Returns (writes, events): writes [(element, row whose
    value lands there)], events {(kind, held, where)} of every flush."""
    writes, events = [], set()
    for r0, r1 in frame_runs:
        cm, held, e_next = [None] * 8, 0, None
        for r in range(r0, r1):
            b, t = divmod(r, T)
            cm = cm[1:] + [r]
            held += 1
            if e_next is None:
                e_next = (b * N + f) * T + t + 1
            e = e_next
            e_next = e + ((N - 1) * T + 1 if t == T - 1 else 1)
            last_of_run = t == T - 1 or r == r1 - 1
            if e % 8 == 0 or last_of_run:
                if held >= 8:
                    kind = "float4" if e % 4 == 0 else "scalar8"
                    ks = range(8)
                else:
                    kind, ks = "partial", range(8 - held, 8)
                writes += [(e - 8 + k, cm[k]) for k in ks]
                where = "clip_end" if t == T - 1 else "run_end" if r == r1 - 1 else "sector"
                events.add((kind, held, where))
                held = 0
    return writes, events


def small_row_window(T, N, lane, row_runs):
    """small_proj_kernel's channel-major store: flush at (t & 7) == 7, at a clip end and at the run's last row, frames
    [max(t & ~7, run_t0), t].  Returns (writes, events)."""
    writes, events = [], set()
    for r0, r1 in row_runs:
        cm, run_t0 = [None] * 8, r0 % T
        for r in range(r0, r1):
            b, t = divmod(r, T)
            if t == 0:
                run_t0 = 0
            cm = cm[1:] + [r]
            if (t & 7) == 7 or t == T - 1 or r == r1 - 1:
                first = t & ~7
                if first < run_t0:
                    first = run_t0
                    events.add("first_lt_run_t0")
                base = (b * N + lane) * T + t - 7
                ks = [k for k in range(8) if t - 7 + k >= first]
                writes += [(base + k, cm[k]) for k in ks]
                events.add("flush_%d" % len(ks))
    return writes, events


def check_once(writes, B, N, T, lanes):
    """Every (b, f, t) of the given filters / lanes is written exactly once, with the value of row b T + t, and nothing
    outside the (B, N, T) output is touched."""
    seen = {}
    for idx, src in writes:
        assert 0 <= idx < B * N * T, ("outside the output", idx)
        bf, t = divmod(idx, T)
        b, f = divmod(bf, N)
        assert src == b * T + t, ("wrong frame", idx, src)
        assert idx not in seen, ("stored twice", idx)
        seen[idx] = src
    want = {(b * N + f) * T + t for b in range(B) for f in lanes for t in range(T)}
    assert set(seen) == want, ("not stored", sorted(want - set(seen))[:8])


def representative_filters(N):
    """A lane's store pattern depends on its filter only through (b N + f) T mod 8: filters 0..7 give every residue."""
    return list(range(min(N, 8))) + ([N - 1] if N > 8 else [])


# ---- dense GEMM: blocks and the non-finite flag ring ------------------------------------------------------------------
def gemm_blocks(ntiles, tpb):
    return runs(ntiles, tpb)


def gemm_dense_tiles(bad, tpb, reset=2):
    """mel_gemm_kernel's three rotating 'tile holds inf/NaN' flags, sequentially: the prologue stages the first tile into
    slot 0, iteration `it` reads slot it % 3, clears slot (it + reset) % 3 and marks slot (it + 1) % 3 while staging the
    next tile.  Returns the tiles that take the dense (no zero-block skipping) path."""
    dense = set()
    for t0, t1 in gemm_blocks(len(bad), tpb):
        flags = [0, 0, 0]
        flags[0] = int(bad[t0])
        for tile in range(t0, t1):
            it = tile - t0
            flags[(it + reset) % 3] = 0
            if flags[it % 3]:
                dense.add(tile)
            if tile + 1 < t1 and bad[tile + 1]:
                flags[(it + 1) % 3] = 1
    return dense


# ---- geometry classes ---------------------------------------------------------------------------------------------------
def run_geometry(T, row_runs):
    """Classes of a cut of B clips of T frames (flat rows r = b T + t) into the waves' runs."""
    c = set()
    lens = [b - a for a, b in row_runs]
    for a, b in row_runs:
        n = b - a
        if n == 1:
            c.add("run_1")
        if n > 4:
            c.add("len_mod4_%d" % (n % 4))
        fa, fb = a, b - 1
        c.add("start_t0" if fa % T == 0 else "start_mid")
        c.add("end_clip_end" if fb % T == T - 1 else "end_mid")
        if fb // T - fa // T >= 2:
            c.add("spans_2_boundaries")
    if len(row_runs) > 1 and lens[-1] == 1:
        c.add("last_wave_1")
    if T == 1:
        c.add("T1")
    elif T < 8:
        c.add("T_lt8")
    if T % 8 == 0:
        c.add("T_mod8_0")
    return c


RUN_CLASSES = {"run_1", "len_mod4_0", "len_mod4_1", "len_mod4_2", "len_mod4_3", "last_wave_1", "start_t0", "start_mid",
               "end_clip_end", "end_mid", "spans_2_boundaries", "T1", "T_lt8", "T_mod8_0"}
CM_CLASSES = ({("float4", 8, "sector")} | {("partial", h, w) for h in range(1, 8) for w in ("run_end", "clip_end")})
SMALL_CM_CLASSES = {"first_lt_run_t0"} | {"flush_%d" % n for n in range(1, 9)}


def pair_classes(B, T, ppw):
    """n_fft 512: where the half pair of an odd-T clip (its last frame, paired with zeros; the next pair starts the next
    clip at t = 0) sits in its run."""
    c = set()
    ppc = cdiv(T, 2)
    for p0, p1 in runs(B * ppc, ppw):
        for p in range(p0, p1):
            if 2 * (p % ppc) + 1 >= T:
                c.add("half_pair_first" if p == p0 else "half_pair_last" if p == p1 - 1 else "half_pair_mid")
    return c


PAIR_CLASSES = {"half_pair_first", "half_pair_mid", "half_pair_last"}


def gemm_classes(ntiles, tpb, bad=()):
    c = set()
    blocks = gemm_blocks(ntiles, tpb)
    for t0, t1 in blocks:
        c.add("block_%d" % (t1 - t0))
    if len(blocks) > 1 and blocks[-1][1] - blocks[-1][0] < tpb:
        c.add("short_last_block")
    for t0, t1 in blocks:
        for tile in bad:
            if t0 <= tile < t1:
                c.add("bad_at_%d" % (tile - t0) if tile - t0 < 4 else "bad_at_ge4")
                if tile + 1 in bad and tile + 1 < t1:
                    c.add("bad_consecutive")
                if tile == t1 - 1 and t1 - t0 < tpb:
                    c.add("bad_last_of_short_block")
    return c


GEMM_CLASSES = {"block_1", "block_2", "block_3", "block_4", "block_7", "short_last_block"}
GEMM_BAD_CLASSES = {"bad_at_0", "bad_at_1", "bad_at_2", "bad_at_3", "bad_consecutive", "bad_last_of_short_block"}

# ---- the sweeps -------------------------------------------------------------------------------------------------------
V_ROWS = (1, 2, 3, 5, 6, 7, 8, 9, 11, 13, 17, 29)
# channel-major forms (banded CMW 1 / 2, n_fft-2048 features, small row form): B clips of T frames, v rows per wave
CM_SWEEP = [(4, T, v) for T in (1, 3, 5, 7, 8, 9, 13, 16, 17, 24, 31) for v in V_ROWS]
# n_fft-512 features: v frame pairs per wave, odd and even T
S512_SWEEP = [(4, T, v) for T in (1, 3, 5, 7, 8, 9, 13, 16, 17, 24, 31) for v in (1, 2, 3, 4, 5, 7, 9, 13)]
# row-major forms (banded, fixed, small row form, the scalar channel-major walk): rows, v rows per wave
ROW_SWEEP = [(rows, v) for rows in (1, 2, 5, 37, 203) for v in V_ROWS + (64,)]
# small projection, matrix-core form: v rounds up to whole tile pairs (1 -> 32, 33 -> 64 ..)
MFMA_SWEEP = [(B, T, v) for B, T in ((3, 41), (2, 100), (5, 37), (1, 1)) for v in (1, 32, 33, 64, 65, 96, 130)]
# dense GEMM: tiles per block (7: the flag ring wraps twice), row counts off the 32-row grid
GEMM_SWEEP = [(rows, v) for rows in (1, 31, 33, 95, 200, 450) for v in (1, 2, 3, 4, 7)]
# non-finite tiles: (tiles, v, poisoned tiles)
GEMM_POISON = [(8, 4, (0,)), (8, 4, (1,)), (8, 4, (2,)), (8, 4, (3,)), (9, 4, (5, 6)), (11, 4, (10,)), (10, 3, (9,)),
               (16, 7, (3, 4, 5)), (16, 7, (6, 13)), (9, 2, (1, 2)), (5, 1, (2,))]
# bf16: tiles per workgroup, 2+ trips of the persistent loop
BF16_SWEEP = [(rows, v) for rows in (129, 600, 1000) for v in (1, 2, 3, 8)]


def cm_cases_classes(sweep, window="cm", N=128):
    """Union of the geometry and store-window classes of a channel-major sweep."""
    hit = set()
    for B, T, v in sweep:
        rr = runs(B * T, forced(v, B * T))
        hit |= run_geometry(T, rr)
        for f in representative_filters(N):
            if window == "cm":
                hit |= cm_window(T, N, f, rr)[1]
            else:
                hit |= small_row_window(T, N, f, rr)[1]
    return hit


if __name__ == "__main__":
    # the default cuts of a few suite and production shapes on a 256-CU device (slots: occupancy x CUs, an assumption
    # here: 2 resident workgroups of 8 waves per CU)
    slots = 256 * 2 * 8
    for rows in (200, 4096, 300_000, 1024 * 690):
        print("banded / fixed  rows %8d: %5d rows per wave" % (rows, banded_rows_per_wave(rows, slots)))
        print("small row form  rows %8d: %5d rows per wave" % (rows, small_row_rows_per_wave(rows)))
        print("small MFMA form rows %8d: %5d rows per wave" % (rows, small_mfma_rows_per_wave(rows)))
        print("dense GEMM      rows %8d: %5d tiles per block" % (rows, gemm_tiles_per_block(rows, 128)))
        print("bf16            rows %8d: %5d workgroups" % (rows, bf16_grid(rows)))
        print("stft512 mel   frames %8d: %5d pairs per wave" % (rows, stft512_pairs_per_wave(1, rows)))
        print("stft2048 mel  frames %8d: %5d frames per wave" % (rows, stft2048_frames_per_wave(rows)))

"""The launch rules of the pointwise, statistics and quantisation kernels, restated for the CPU, with the cases,
inputs and float64 references of test_small_kernels_gpu.py.

csrc/pointwise.hip, csrc/quant.hip, csrc/resample.hip and the two small kernels of csrc/mel.hip and csrc/phase_repr.hip
are grid-stride loops of 256-thread blocks under a cap, multi-block reductions, or a block per stream under the grid
limit.  test_small_kernel_cases_cpu.py checks that the tables below take every one of those loops into its second and
third trip, stand on both sides of every dispatch condition and meet the conditions the tolerances rest on; the GPU file
runs them.

The arithmetic restates the rules, not the code: grid_for() of pointwise.hip and qgrid() of quant.hip (blocks of 256
threads, at most 2048: 8 per compute unit), the `* 4` of the Cartesian launchers and the 256 * 32 of
at_polar_to_complex, the dispatch comment of at_cartesian_pack (rows that are not whole 64-byte segments, F >= 64,
rows >= 64: a block owns 8 rows), the header of the statistics kernels (per-block partials of 2048 elements, at most
1024 blocks, one block of 256 threads folds them), launch_mel_project() (K > 576 or K < 16: one thread per output, at
most 8192 blocks), the block per stream of at_oadd_invert / at_oadd_push (at most 65535) and the rows on grid.y of
at_resample_sinc (at most 65535; more is AT_EUNSUPPORTED)."""
import math
from collections import namedtuple

import numpy as np

THREADS = 256
CAP = 2048                              # blocks of grid_for() / qgrid() / at_mag_pointwise
TRIP = CAP * THREADS                    # 524 288 elements per trip of those loops
WIDE_CAP = 8192                         # Cartesian flat form, at_polar_to_complex, mel_gemm_simple_kernel
WIDE_TRIP = WIDE_CAP * THREADS          # 2 097 152
STATS_PER_BLOCK = 8 * THREADS
STATS_MAX_BLOCKS = 1024
STREAM_BLOCKS = 65535                   # at_oadd_invert / at_oadd_push
GRID_Y = 65535                          # at_resample_sinc
PACK_ROWS = 8
EPS = 1.1920929e-07

f32, f64 = np.float32, np.float64


def cdiv(a, b):
    return -(-a // b)


# ---- grid-stride loops ------------------------------------------------------------------------------------------------
def blocks(n, cap=CAP):
    return max(1, min(cdiv(n, THREADS), cap))


def trips(n, cap=CAP):
    """Trips of the first thread of the launch."""
    return cdiv(n, blocks(n, cap) * THREADS)


def trip_classes(n, cap=CAP):
    T = cap * THREADS
    c = {"trips_%d" % min(trips(n, cap), 3)}
    if n == 1:
        c.add("n=1")
    if 1 < n < THREADS:
        c.add("one_partial_block")
    if THREADS < n < 2 * THREADS:
        c.add("ragged_second_block")
    if n == T - 1:
        c.add("trip-1")
    if n == T:
        c.add("trip")
    if n == T + 1:
        c.add("trip+1")
    if T + THREADS < n < 2 * T:
        c.add("second_trip_partly_filled")
    return c


LOOP_WANT = {"n=1", "one_partial_block", "ragged_second_block", "trip-1", "trip", "trip+1", "second_trip_partly_filled", "trips_3"}
# what every plain loop is run at: 1, 255 and 257 elements, one trip exactly and one element either side, a second trip
# half filled, a third trip
SIZES = (1, 255, 257, TRIP - 1, TRIP, TRIP + 1, TRIP + TRIP // 2 + 3, 2 * TRIP + 77)
LOOP_ENTRIES = ("at_angle", "at_affine", "at_griffinlim_update", "at_scale_complex", "at_mag_pointwise", "at_mulaw_encode",
                "at_mulaw_decode", "at_onehot", "at_argmax_last", "at_oadd_forward")


# ---- statistics -----------------------------------------------------------------------------------------------------------
def stats_plan(n):
    """(blocks of the partial kernel, trips of its first thread, trips of the fold's first thread)."""
    b = max(1, min(cdiv(n, STATS_PER_BLOCK), STATS_MAX_BLOCKS))
    return b, cdiv(n, b * THREADS), cdiv(b, THREADS)


def stats_classes(n):
    b, t, ft = stats_plan(n)
    c = set()
    if n < 64:
        c.add("n<64")
    if n < THREADS:
        c.add("n<256")
    if b == 1 and n >= THREADS:
        c.add("one_block")
    if 2 <= b <= THREADS:
        c.add("blocks_2_256")
    if b == THREADS:
        c.add("blocks=256")
    if ft >= 2:
        c.add("fold_second_trip")
    if cdiv(n, STATS_PER_BLOCK) > STATS_MAX_BLOCKS:
        c.add("capped")
        if n % (b * THREADS) and n % STATS_PER_BLOCK and n % THREADS and n % 64:
            c.add("capped_ragged")
    return c


STATS_WANT = {"n<64", "n<256", "one_block", "blocks_2_256", "blocks=256", "fold_second_trip", "capped", "capped_ragged"}
STATS_SIZES = (37, 200, 1500, 2048, 6 * 2048 - 35, 256 * 2048, 300 * 2048 + 1, 4300003)
CAPPED_N = 4300003                      # real input of the Normalize cases (17 MB)
CAPPED_SPECTRUM = (4093, 513)           # complex input of the Magnitude.scale_data cases (17 MB)


def stats_positions(n):
    """Where the extremes go: the first element, the last element (of the last block), an element only the second trip
    of the partial kernel reads, and one in its last trip."""
    b, t, _ = stats_plan(n)
    pos = {"first": 0, "last": n - 1}
    if t >= 2:
        pos["second_trip"] = b * THREADS + 5
    if t >= 3:
        pos["last_trip"] = (t - 1) * b * THREADS + 3
    return pos


def stats_ref(v):
    """[min, max, sum, sum of squares] of a float64 array, NaN propagating like Tensor.min() / max()."""
    v = np.asarray(v, f64)
    return np.array([v.min(), v.max(), v.sum(), (v * v).sum()])


def stats_values(x, kind, contrast):
    """float64 values whose statistics at_stats takes: kind 0 |z|, 1 |z|^2, 2 x, 3 |x|; contrast 0 none, 1 log1p, 2 log,
    3 log10 (clamped at eps)."""
    if kind <= 1:
        re, im = x.real.astype(f64), x.imag.astype(f64)
        v = re * re + im * im if kind == 1 else np.hypot(re, im)
    else:
        v = x.astype(f64) if kind == 2 else np.abs(x.astype(f64))
    return contrast_ref(v, contrast)


def contrast_ref(v, contrast):
    with np.errstate(divide="ignore", invalid="ignore"):
        if contrast == 1:
            return np.log1p(v)
        if contrast == 2:
            return np.log(np.maximum(v, f64(f32(EPS))))
        if contrast == 3:
            return np.log10(np.maximum(v, f64(f32(EPS))))
    return v


def contrast_inv_ref(v, contrast):
    if contrast == 1:
        return np.exp(v) - 1
    if contrast == 2:
        return np.exp(v) - f64(f32(EPS))
    if contrast == 3:
        return 10.0 ** v
    return v


CONTRASTS = {None: 0, "log1p": 1, "log": 2, "log10": 3}


def affine_ref64(values, mode):
    """Two-pass float64 (offset, scale) of Normalize (the reference's norm.py:25-38)."""
    v = np.asarray(values, f64)
    if mode == "unipolar":
        return v.min(), v.max() - v.min()
    if mode == "bipolar":
        off = (v.max() + v.min()) / 2
        return off, v.max() - off
    mean = v.mean()
    return mean, math.sqrt(((v - mean) ** 2).sum() / (v.size - 1))


def one_pass_condition(values):
    """1 + mean^2 / var: the factor by which the one-pass variance amplifies the rounding of its sums."""
    v = np.asarray(values, f64)
    return 1.0 + v.mean() ** 2 / v.var()


def real_data(n, seed=11):
    """mean 3, standard deviation 1: 1 + mean^2 / var = 10."""
    return (np.random.RandomState(seed).randn(n) + 3.0).astype(f32)


def spectrum_data(shape, seed=12):
    """Moduli in [1.5, 50]: every contrast of them is positive (no cancellation in the sums)."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    mod, ph = rng.uniform(1.5, 50.0, n), rng.uniform(-np.pi, np.pi, n)
    return (mod * np.exp(1j * ph)).astype(np.complex64).reshape(shape)


# ---- special values -----------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.17549435e-38, 3e38, -3e38, 1.0, -1.0, 1e-30],
                    dtype=f32)


def with_specials(a, specials=SPECIALS):
    """`a` (flat float32) with the special values at its start, in its middle and at its end (where it is long enough:
    the end of the last trip)."""
    a = a.copy()
    k = len(specials)
    if a.size >= k:
        a[:k] = specials
        a[-k:] = specials[::-1]
    if a.size >= 4 * k:
        a[a.size // 2:a.size // 2 + k] = specials
    return a


def randn32(n, seed):
    return np.random.RandomState(seed).randn(n).astype(f32)


def same_bits(a, b):
    """Equal with NaN == NaN, and zeros of the same sign."""
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a):
        return same_bits(a.real, b.real) and same_bits(a.imag, b.imag)
    return bool(a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and
                np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0])))


# ---- affine, scale_complex, griffinlim, mag_pointwise, polar_to_complex, angle ------------------------------------------
AFFINE_OFFSET, AFFINE_SCALE = f32(0.3), f32(1.7)            # a scale that is no power of two


def affine_ref(x, off, sc, inverse):
    """The same float32 expression: an IEEE division one way, an unfused multiply then add the other."""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        return (x * f32(sc) + f32(off)).astype(f32) if inverse else ((x - f32(off)) / f32(sc)).astype(f32)


def angle_data(n, seed=5):
    rng = np.random.RandomState(seed)
    re = (rng.randn(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(f32)
    im = (rng.randn(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(f32)
    return re, im


ANGLE_BAR = 5e-7                        # test_fast_atan2_accuracy_and_edge_cases


def griffinlim_data(n, seed=6):
    """mag, rebuilt, tprev; rebuilt is exactly 0 at every 7th element and rebuilt = tprev = 0 at every 11th."""
    rng = np.random.RandomState(seed)
    mag = np.abs(rng.randn(n)).astype(f32)
    reb = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
    tp = (rng.randn(n) + 1j * rng.randn(n)).astype(np.complex64)
    reb[::7] = 0
    reb[::11] = 0
    tp[::11] = 0
    return mag, reb, tp


GL_MOMENTUM = f32(0.99 / 1.99)


def griffinlim_ref(mag, reb, tp, m):
    """(reference, per-element bar, mask of the elements whose `a` is exactly 0)."""
    m = f64(f32(m))
    a = reb.astype(np.complex128) - (m * tp.astype(np.complex128) if tp is not None else 0)
    mod = np.abs(a)
    ref = mag.astype(f64) * a / (mod + 1e-16)
    big = np.abs(reb.astype(np.complex128)) + (np.abs(m * tp.astype(np.complex128)) if tp is not None else 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        bar = np.abs(mag.astype(f64)) * 8 * 2.0 ** -24 * (1 + big / mod)
    return ref, bar, mod == 0


PARITY = 1e-5                           # the project's bar: max|got - ref| / max|ref|


# ---- Cartesian ------------------------------------------------------------------------------------------------------------
def pack_form(rows, F):
    """'rows' (a block owns 8 rows) or 'flat' (grid stride over rows * F, 8192 blocks)."""
    return "rows" if (F * 4) % 64 != 0 and F >= 64 and rows >= 64 else "flat"


def pack_classes(rows, F):
    form = pack_form(rows, F)
    c = {form}
    if form == "rows":
        if rows % PACK_ROWS:
            c.add("short_last_chunk")
        c.add("row_shorter_than_256" if F < 256 else "row_longer_than_256")
    else:
        if (F * 4) % 64 == 0:
            c.add("flat:whole_segments")
        if F < 64:
            c.add("flat:F<64")
        if rows < 64:
            c.add("flat:rows<64")
        c.add("flat:trips_%d" % min(trips(rows * F, WIDE_CAP), 3))
    return c


PACK_WANT = {"rows", "flat", "short_last_chunk", "row_shorter_than_256", "row_longer_than_256", "flat:whole_segments",
             "flat:F<64", "flat:rows<64", "flat:trips_2"}
# (rows, F)
CARTESIAN = [(63, 513), (64, 513), (65, 513), (64, 63), (65, 64), (64, 65), (67, 127), (200, 513), (1, 1), (3, 257),
             (4100, 512)]
NORM_COMBOS = [(False, False), (True, False), (False, True), (True, True)]          # Normalize on the real / imaginary half
RE_AFFINE, IM_AFFINE = (f32(0.3), f32(1.7)), (f32(-0.7), f32(0.6))


def cartesian_pack_ref(x, re, im):
    out = np.empty(x.shape[:-1] + (2, x.shape[-1]), f32)
    out[..., 0, :] = affine_ref(x.real, re[0], re[1], False) if re else x.real
    out[..., 1, :] = affine_ref(x.imag, im[0], im[1], False) if im else x.imag
    return out


def cartesian_unpack_ref(y, re, im):
    r = affine_ref(y[..., 0, :], re[0], re[1], True) if re else y[..., 0, :]
    i = affine_ref(y[..., 1, :], im[0], im[1], True) if im else y[..., 1, :]
    out = np.empty(r.shape, np.complex64)
    out.real, out.imag = r, i
    return out


# ---- mu-law, one-hot, argmax ----------------------------------------------------------------------------------------------
MULAW_CHANNELS = (256, 64, 2)
MULAW_SPECIALS = np.array([-1.0, 1.0, 0.0, -0.0, 1e-8, -1e-8, 0.5, -0.5], dtype=f32)
MULAW_BAND = 1e-4
MULAW_BAND_SHARE = 1e-3


def mulaw_input(n, seed=9):
    """Uniform in [-1, 1]; the second block uniform in [-4, 4] (torchaudio does not clamp); the special values first and
    last."""
    rng = np.random.RandomState(seed + n % 1000)
    x = rng.uniform(-1, 1, n).astype(f32)
    if n >= 2 * THREADS:
        x[THREADS:2 * THREADS] = rng.uniform(-4, 4, THREADS).astype(f32)
    return with_specials(x, MULAW_SPECIALS)


def mulaw_q64(x, channels):
    """The closed form in float64, before truncation."""
    mu = channels - 1.0
    x = x.astype(f64)
    return (np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu) + 1) / 2 * mu + 0.5


def mulaw_band(q):
    return np.abs(q - np.rint(q)) < MULAW_BAND


def mulaw_decode_ref(codes, channels):
    mu = channels - 1.0
    v = codes.astype(f64) / mu * 2 - 1
    return np.sign(v) * (np.exp(np.abs(v) * np.log1p(mu)) - 1) / mu


# (shape of x, classes, channel_major): the loop runs over x.size * classes
ONEHOT = [((1,), 1, False), ((255,), 1, False), ((257,), 1, False), ((257,), 3, False), ((TRIP - 1,), 1, False), ((TRIP,), 1, False),
          ((TRIP + 1,), 1, False), ((2048,), 256, False), ((262145,), 3, False), ((4099,), 256, False),
          ((1, 1), 1, True), ((3, 43), 3, True), ((7, 37), 3, True), ((3, 174763), 1, True), ((1, 2049), 256, True), ((87383, 3), 3, True),
          ((5, 821), 256, True)]
ONEHOT_CHANNEL_WANT = {"n=1", "ragged_second_block", "trip+1", "second_trip_partly_filled", "trips_3"}

# (rows, cols): the loop runs over rows
ARGMAX = [(1, 3), (255, 2), (257, 3), (TRIP - 1, 1), (TRIP, 2), (TRIP + 1, 3), (TRIP + TRIP // 2 + 3, 2), (2 * TRIP + 77, 1),
          (2 * TRIP + 77, 3), (3000, 256)]
ARGMAX_ROW_KINDS = ("random_ties", "all_equal", "signed_zero_tie", "all_-inf", "nan_first", "nan_middle", "nan_last",
                    "nan_middle_and_last", "inf_after_nan")


def argmax_rows(rows, cols, floating, seed=10):
    """Small integers (ties everywhere); every 16th row starts a run of the special rows of ARGMAX_ROW_KINDS."""
    rng = np.random.RandomState(seed)
    a = rng.randint(-2, 3, (rows, cols))
    if not floating:
        a = a.astype(np.int64)
        a[1::16] = 4                                            # all equal
        if cols > 1:
            a[2::16, -1] = np.iinfo(np.int64).max               # beyond what a float32 compare could tell apart
            a[2::16, 0] = np.iinfo(np.int64).max - 1
            a[3::16] = np.iinfo(np.int64).min
        return a
    a = a.astype(f32)
    mid = cols // 2
    a[1::16] = 1.5
    a[2::16] = 0.0
    a[2::16, ::2] = -0.0
    a[3::16] = -np.inf
    a[4::16, 0] = np.nan
    a[5::16, mid] = np.nan
    a[6::16, -1] = np.nan
    a[7::16, mid] = np.nan
    a[7::16, -1] = np.nan
    a[8::16, mid] = np.nan
    a[8::16, -1] = np.inf
    return a


# ---- OverlapAdd -----------------------------------------------------------------------------------------------------------
# at_oadd_forward (S, C, keep, buf_len): the loop runs over S * buf_len; C < keep and a zero pad are in
OADD_FORWARD = [(1, 1, 0, 1), (1, 200, 50, 255), (1, 201, 50, 257), (1, TRIP - 8, 6, TRIP - 1), (65536, 2, 6, 8),
                (1, TRIP - 9, 6, TRIP + 1), (3, 262140, 6, 262149), (131077, 4, 3, 8), (65537, 2, 6, 9)]


def oadd_forward_ref(x, hist, keep, buf_len):
    S, C = x.shape
    h = hist if hist is not None else np.zeros((S, keep), f32)
    buf = np.zeros((S, buf_len), f32)
    buf[:, :keep] = h
    buf[:, keep:keep + C] = x
    return buf, buf[:, C:C + keep].copy()


# at_oadd_invert at n_fft 8 / hop 2 (keep 6): (S, frames)
OADD_N_FFT, OADD_HOP, OADD_KEEP = 8, 2, 6
OADD_INVERT = [(65534, 2), (65535, 1), (65536, 3), (65541, 2), (2 * 65535 + 3, 1)]
OADD_BAR = 1e-6


def stream_classes(S):
    c = {"walks_%d" % min(cdiv(S, STREAM_BLOCKS), 3)}
    if S == STREAM_BLOCKS:
        c.add("S=65535")
    if S == STREAM_BLOCKS + 1:
        c.add("S=65536")
    if S > STREAM_BLOCKS and S % STREAM_BLOCKS:
        c.add("ragged_last_walk")
    return c


STREAM_WANT = {"walks_1", "walks_2", "walks_3", "S=65535", "S=65536", "ragged_last_walk"}


def oadd_invert_ref(frames, tail, gain):
    """float64 overlap-add: (out, new tail)."""
    S, n, n_fft = frames.shape
    rec = np.zeros((S, (n - 1) * OADD_HOP + n_fft), f64)
    if tail is not None:
        rec[:, :OADD_KEEP] = tail
    for i in range(n):
        rec[:, i * OADD_HOP:i * OADD_HOP + n_fft] += frames[:, i]
    return rec[:, :rec.shape[1] - OADD_KEEP] / f64(gain), rec[:, rec.shape[1] - OADD_KEEP:]


# at_oadd_push (S, C, keep, buf_len): C < keep is the overlapping move
OADD_PUSH = [(65535, 2, 6, 8), (65536, 10, 6, 19), (65541, 2, 6, 9), (2 * 65535 + 3, 7, 6, 13), (5, 300, 700, 1003),
             (5, 700, 300, 1000)]


def oadd_push_ref(buf, x, keep):
    C = x.shape[1]
    out = buf.copy()
    out[:, :keep] = buf[:, C:C + keep]
    out[:, keep:keep + C] = x
    return out


# ---- resample -------------------------------------------------------------------------------------------------------------
RESAMPLE_ORIG, RESAMPLE_NEW = 3, 2
# (rows, L)
RESAMPLE = [(3, 382), (3, 384), (3, 385), (5, 5), (5, 1), (2, 1500), (65535, 4)]
RESAMPLE_TOO_MANY = (65536, 4)
RESAMPLE_BAR = 1e-5


def resample_out_len(L, orig=RESAMPLE_ORIG, new=RESAMPLE_NEW):
    return cdiv(new * L, orig)


def resample_ref(x, h, width, orig=RESAMPLE_ORIG, new=RESAMPLE_NEW):
    """y[i * new + j] = sum_k h[j][k] * xpad[i * orig + k] in float64 over the float32 bank h (new, 2 width + orig)."""
    rows, L = x.shape
    out_len = resample_out_len(L, orig, new)
    nb = cdiv(out_len, new)
    taps = 2 * width + orig
    xpad = np.zeros((rows, max(L + 2 * width + orig, (nb - 1) * orig + taps)), f64)
    xpad[:, width:width + L] = x
    win = np.lib.stride_tricks.sliding_window_view(xpad, taps, axis=1)[:, ::orig][:, :nb]
    y = win @ np.asarray(h, f64).T
    return y.reshape(rows, nb * new)[:, :out_len]


# ---- the one-thread-per-output projection ---------------------------------------------------------------------------------
def mel_kernel(K):
    return "simple" if K > 576 or K < 16 else "mfma"


# name, K, N, rows, T (channel-major store when > 0), complex input, contrast, Normalize, inverse
Mel = namedtuple("Mel", "name K N rows T complex contrast norm inverse")
MEL = [
    Mel("k600_over_the_cap", 600, 130, 16411, 0, False, "log1p", True, False),
    Mel("k577_channel_major_log1p", 577, 130, 3 * 77, 77, True, "log1p", True, False),
    Mel("k577_log", 577, 130, 3 * 77, 0, True, "log", False, False),
    Mel("k600_log10", 600, 70, 200, 0, True, "log10", True, False),
    Mel("k600_plain", 600, 70, 200, 0, True, None, False, False),
    Mel("k15_channel_major_over_the_cap", 15, 130, 3 * 5471, 5471, True, "log1p", True, False),
    Mel("k8_over_the_cap", 8, 129, 16411, 0, True, "log", True, False),
    Mel("k15_log10", 15, 33, 100, 0, False, "log10", False, False),
    Mel("k8_plain_channel_major", 8, 33, 2 * 51, 51, False, None, True, False),
    Mel("k600_inverse_log1p", 600, 130, 300, 0, False, "log1p", True, True),
    Mel("k577_inverse_log", 577, 70, 300, 0, False, "log", True, True),
    Mel("k15_inverse_log10", 15, 33, 16411 * 4, 0, False, "log10", True, True),
    Mel("k8_inverse_plain", 8, 33, 300, 0, False, None, False, True),
]
MEL_AFFINE = (f32(0.3), f32(1.7))


def mel_classes(c):
    k = {"K=%d" % c.K, "inverse" if c.inverse else "forward:%s" % c.contrast, "channel_major" if c.T else "row_major",
         "trips_%d" % min(trips(c.rows * c.N, WIDE_CAP), 3)}
    if trips(c.rows * c.N, WIDE_CAP) >= 2 and c.N % 128:
        k.add("over_the_cap_ragged_N")
        k.add("over_the_cap:%s" % ("channel_major" if c.T else "row_major"))
    return k


MEL_WANT = {"K=8", "K=15", "K=577", "K=600", "inverse", "forward:None", "forward:log1p", "forward:log", "forward:log10",
            "channel_major", "row_major", "over_the_cap_ragged_N", "over_the_cap:channel_major", "over_the_cap:row_major"}


def mel_inputs(c, seed=13):
    rng = np.random.RandomState(seed + c.K)
    bank = rng.uniform(0.0, 1.0, (c.K, c.N)).astype(f32)
    bank[rng.uniform(size=bank.shape) < 0.5] = 0
    if c.inverse:
        x = rng.uniform(0.0, 1.5, (c.rows, c.K)).astype(f32)
    elif c.complex:
        x = spectrum_data((c.rows, c.K), seed + 1)
    else:
        x = (rng.uniform(1.5, 50.0, (c.rows, c.K)) * rng.choice([-1.0, 1.0], (c.rows, c.K))).astype(f32)
    if c.T:
        x = x.reshape((c.rows // c.T, c.T, c.K))
    return x, bank


def mel_ref(c, x, bank):
    """float64 matmul through the same contrast / Normalize chain (Magnitude.forward / invert with a dense bank)."""
    off, sc = (f64(MEL_AFFINE[0]), f64(MEL_AFFINE[1])) if c.norm else (0.0, 1.0)
    code = CONTRASTS[c.contrast]
    if c.inverse:
        return contrast_inv_ref(x.astype(f64) * sc + off, code) @ bank.astype(f64)
    y = (contrast_ref(np.abs(x).astype(f64) @ bank.astype(f64), code) - off) / sc
    return np.swapaxes(y, -1, -2) if c.T else y


def rel_max(a, b):
    a, b = np.asarray(a), np.asarray(b)
    d = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (d if d > 0 else 1.0)

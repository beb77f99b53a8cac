"""The frame walk and the radix plans of the fallback STFT kernels, restated for the CPU, and the cases of
test_frame_walk_gpu.py that force the walk through AT_VARIANT_FRAME_WALKERS.

csrc/stft_generic.hip (powers of two from 8 that have no register-core kernel, or whose window is not aligned for it) and
csrc/stft_mixed.hip (everything else) launch min(frames, 4096) workgroups; workgroup i transforms frames i, i + g,
i + 2 g, ... with its twiddle tables filled once.  The overlap-add gather behind the unfused inverse strides a grid of
at most 65536 blocks of 256 threads over its outputs (four outputs per thread in its float4 form).  The variant replaces
both grids by min(v, frames) and min(v, blocks).  test_frame_walk_cases_cpu.py checks that the table below reaches every
walk shape, every stage kind of both kernels and both forms of the gather; the GPU file runs it.

The arithmetic restates the rules, not the code: the header comment of stft_mixed.hip (fours, then a two, then the odd
primes in ascending order; a table of M twiddles in LDS up to M = 4096), the comment of stockham() in stft_generic.hip
(one radix-2 stage first when log2 M is odd, then radix-4 stages; radix-2 throughout when there is no table, n_fft
16384) and the dispatch of at_stft_forward / at_istft in csrc/capi.hip."""
from collections import namedtuple

WALK_CAP = 4096         # workgroups of a default launch of the frame kernels
GATHER_CAP = 65536      # blocks of a default launch of the gather
GATHER_THREADS = 256
ONE_TRIP = 65535        # AT_VARIANT_FRAME_WALKERS value that clamps to a workgroup per frame at every size of the table
REGISTER_SIZES = {128: 8, 256: 8, 512: 8, 1024: 8, 2048: 16, 4096: 16}    # n_fft: window alignment its kernel needs
LDS_DEFAULT_LIMIT = 64 * 1024


def cdiv(a, b):
    return -(-a // b)


# ---- which kernel, which stages ---------------------------------------------------------------------------------------
def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def kernel_of(n_fft, window_alignment=16):
    """'register', 'generic' or 'mixed': the forward / frames kernel of a size for a window pointer of that alignment."""
    if n_fft in REGISTER_SIZES and window_alignment % REGISTER_SIZES[n_fft] == 0:
        return "register"
    return "generic" if is_pow2(n_fft) and n_fft >= 8 else "mixed"


def fft_length(n_fft):
    """Points of the complex transform: half the frame (packed real pairs) for even sizes, the whole frame for odd."""
    return n_fft if n_fft & 1 else n_fft // 2


def radix_plan(M):
    """Stage radices of the mixed kernel: fours, then a two, then the odd primes in ascending order (product M)."""
    plan = []
    while M % 4 == 0:
        plan.append(4)
        M //= 4
    if M % 2 == 0:
        plan.append(2)
        M //= 2
    p = 3
    while M > 1:
        if M % p:
            p += 2
        else:
            plan.append(p)
            M //= p
    return plan


def stage_kind(p):
    """Radix 2 / 3 / 4 / 5 / 7 butterflies in registers; any other prime is a direct p-term sum."""
    return p if p in (2, 3, 4, 5, 7) else "prime"


def mixed_has_table(n_fft):
    return fft_length(n_fft) <= 4096


def generic_has_table(n_fft):
    return n_fft <= 8192


def stockham_stages(n_fft):
    """Stage radices of the generic kernel for M = n_fft / 2 points."""
    log2m = (n_fft // 2).bit_length() - 1
    if not generic_has_table(n_fft):
        return [2] * log2m
    return [2] * (log2m & 1) + [4] * (log2m // 2)


def generic_lds_bytes(n_fft, inverse=False):
    """Two frame buffers of M complex values (the inverse stages M + 1 bins in the second: two more), then the tables:
    3 M / 4 + 1 FFT twiddles and M + 1 split twiddles."""
    M = n_fft // 2
    words = 2 * M + (2 if inverse else 0)
    if generic_has_table(n_fft):
        words += 3 * M // 4 + 1 + M + 1
    return 8 * words


# ---- the walk -----------------------------------------------------------------------------------------------------------
def walkers(frames, v=0):
    """Workgroups of a frame-kernel launch: the default plan, or AT_VARIANT_FRAME_WALKERS = v."""
    return min(v, frames) if v > 0 else min(frames, WALK_CAP)


def trips(frames, v, i):
    """The frames workgroup i transforms, in order."""
    return list(range(i, frames, walkers(frames, v)))


def walk_classes(B, T, v):
    """Shape classes of one launch over B clips of T frames."""
    N = B * T
    g = walkers(N, v)
    most = len(trips(N, v, 0))
    c = {"trips_%d" % min(most, 3)}
    if N % g:
        c.add("ragged_last_trip")
    if v == 1:
        c.add("v=1")
    if v == N - 1:
        c.add("v=N-1")
    if v >= N:
        c.add("v>=N")
    if v == ONE_TRIP:
        c.add("v=65535")
    if any(a // T != b // T for i in range(g) for a, b in zip(trips(N, v, i), trips(N, v, i)[1:])):
        c.add("walker_crosses_clips")
    return c


# ---- the gather ---------------------------------------------------------------------------------------------------------
def gather_float4(n_fft, hop):
    """Four outputs per thread when no aligned group of four can straddle a frame start (pointers 16-byte aligned)."""
    return hop % 4 == 0 and n_fft % 8 == 0


def out_len(n_fft, hop, T):
    return hop * (T - 1) + (n_fft & 1)


def gather_units(B, T, n_fft, hop, float4=None):
    f4 = gather_float4(n_fft, hop) if float4 is None else float4
    total = B * out_len(n_fft, hop, T)
    return total // 4 if f4 else total


def gather_blocks(units, v=0):
    blocks = cdiv(units, GATHER_THREADS)
    return min(v, blocks) if v > 0 else min(blocks, GATHER_CAP)


def gather_strides(units, v=0):
    """Outputs (or groups of four) the first thread of the launch visits."""
    return cdiv(units, gather_blocks(units, v) * GATHER_THREADS)


def gather_classes(case, v):
    c = {"float4" if gather_float4(case.n_fft, case.hop) else "scalar"}
    if case.n_fft % case.hop:
        c.add("hop_does_not_divide")
    if case.n_fft & 1:
        c.add("odd_n_fft")
    c.add("strides_%d" % min(gather_strides(gather_units(case.B, case.T, case.n_fft, case.hop), v), 3))
    return c


# ---- the cases ----------------------------------------------------------------------------------------------------------
# kernel: what runs the frames; window_alignment 4: the window is a view one float into its buffer, which takes the
# register-core sizes to the generic kernel.  forced: the walker counts swept besides 0 (default) and ONE_TRIP.
Case = namedtuple("Case", "name kernel n_fft hop B T L window_alignment forced")


def clip_length(n_fft, hop, T):
    """A clip of exactly T centred frames whose length is no multiple of the hop."""
    return hop * (T - 1) + (n_fft & 1) + min(hop - 1, 3)


def frames_of(n_fft, hop, L):
    """torch.stft(center=True): frames of a clip reflect-padded by n_fft // 2 on both sides."""
    return 1 + (L - (n_fft & 1)) // hop


def _case(kernel, n_fft, hop, B=3, T=7, window_alignment=16):
    N = B * T
    name = "%s_%d_h%d%s" % (kernel, n_fft, hop, "_window4" if window_alignment == 4 else "")
    return Case(name, kernel, n_fft, hop, B, T, clip_length(n_fft, hop, T), window_alignment, (1, 4, 5, N - 1, N))


# Three clips of 7 frames (21: odd, so every walker count but 1, 3, 7 leaves a ragged last trip); the sizes without a
# twiddle table take 2 clips of 4 frames (the direct 8191-term sums are slow).
CASES = [
    _case("generic", 8, 1),              # M = 4: one radix-4 stage
    _case("generic", 16, 4),             # M = 8: radix 2 first
    _case("generic", 64, 16),            # M = 32: 2, 4, 4
    _case("generic", 8192, 2048, B=2, T=4),      # tables past the default LDS limit
    _case("generic", 16384, 4096, B=2, T=4),     # no table
    _case("generic", 128, 32, window_alignment=4),
    _case("generic", 1024, 256, window_alignment=4),
    _case("generic", 2048, 512, window_alignment=4),
    _case("mixed", 2, 1),                # M = 1: the empty plan
    _case("mixed", 3, 1),
    _case("mixed", 4, 1),
    _case("mixed", 5, 1),
    _case("mixed", 7, 1),
    _case("mixed", 6, 1),
    _case("mixed", 30, 7),               # 3 x 5
    _case("mixed", 254, 84),             # 2 x 127, hop n / 3
    _case("mixed", 441, 147),            # odd: 3 x 3 x 7 x 7 at full length, hop n / 3
    _case("mixed", 400, 100),            # 4 x 2 x 5 x 5
    _case("mixed", 9604, 2401, B=2, T=4),        # M = 4802 = 2 x 7^4, no table
    _case("mixed", 12000, 3000, B=2, T=4),       # M = 6000 = 4 x 4 x 3 x 5 x 5 x 5, no table
    _case("mixed", 6561, 1640, B=2, T=4),        # 3^8, odd, no table
    _case("mixed", 8191, 2047, B=2, T=4),        # prime, no table
]

# center=False over a strided view (Test D): n_fft, hop, L, clip_stride, T -- the last frame ends past the clip
UNCENTRED = [("generic", 64, 16, 150, 157, 7), ("generic", 16384, 4096, 30001, 30005, 5),
             ("mixed", 30, 7, 61, 67, 7), ("mixed", 441, 147, 1000, 1003, 6)]

# the shortest legal clip, L = n_fft // 2 + 1 (Test E): n_fft, hop
SHORTEST = [("generic", 64, 16), ("mixed", 30, 7), ("mixed", 441, 110)]

# the default plan across its cap (Test F): n_fft, hop, clips, samples
ACROSS_CAP = [("generic", 8, 1, 3, 2000), ("mixed", 6, 1, 3, 2000)]


def plans(case):
    """Every AT_VARIANT_FRAME_WALKERS value a case is run under, the default first."""
    return [0, ONE_TRIP] + list(case.forced)

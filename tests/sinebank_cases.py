"""The "sinebank" inversion's kernel paths, restated for the CPU, the cases of test_sinebank_gpu.py that reach them, and
a float64 model of both entry points.

Offline (csrc/sinebank.hip at_sinebank_offline): sine_matrix_kernel builds S (F x L); per pass launch_mel_project
(csrc/mel.hip) contracts the frame `a_block_offset[col >> 7]` of every clip against S with K = F, dense = 1 -- through
mel_gemm_simple_kernel when `K > 576 || K < 16`, else mel_gemm_kernel<KSTEPS, NL, true> with K_main = 4 KSTEPS the largest
of {512 .. 16} <= K, a K tail on the vector ALU (4 bank columns in registers, the rest re-read) and NL = ceil(K / 128) load
segments per staged piece; sine_combine_kernel sums the passes under the weights of transforms/sinebank._offline_tables
in a grid-stride loop of 8192 x 256 threads.  Realtime (at_sinebank_realtime): one 256-thread block per 256 samples of a
frame, the frame's magnitudes, c and phi staged in LDS in trips of 256; refused above S T = 65535 (grid.y) and above 3 F
floats = 48 KB.

test_sinebank_cases_cpu.py checks with the helpers here that the tables reach every path named below, and the host tables
against F.interpolate; the GPU file runs the cases.  The fp32 oracle stays oracle.sinebank_offline / sinebank_realtime;
the float64 model here measures how far the oracle's own rounding is from the 1e-5 bar of the GPU file."""
import functools

import numpy as np
import torch

from oracle import oracle as O

SR = 44100
SIMPLE_ABOVE, SIMPLE_BELOW = 576, 16     # launch_mel_project: K > 576 || K < 16 -> one thread per output
GEMM_ROWS = 32                           # rows of a mel_gemm_kernel tile
COL_BLOCK = 128                          # output samples that share one frame offset per pass
SWEEP_OUTPUTS = 8192 * 256               # sine_combine_kernel / mel_gemm_simple_kernel: outputs per grid sweep
PASS_LIMIT = 64                          # at_sinebank_offline: n_pass > 64 is AT_EINVAL
RT_GRID_LIMIT = 65535                    # at_sinebank_realtime: S T (grid.y)
RT_LDS_BYTES = 48 * 1024                 # ... and 3 F floats of LDS


def cdiv(a, b):
    return -(-a // b)


# ---- the cases ----------------------------------------------------------------------------------------------------------
# offline: (B, T, n_fft, hop)
OFFLINE_CASES = [
    (2, 3, 4096, 1024),     # F 2049: simple kernel with block offsets (56 column blocks), two passes
    (2, 5, 2048, 512),      # F 1025: simple kernel with block offsets, three passes
    (3, 6, 16, 4),          # F 9 < 16: simple kernel, one column block, L = 40
    (2, 4, 30, 8),          # F 16: the smallest MFMA form (K_main 16), tail 0
    (2, 4, 32, 8),          # F 17: K_main 16, tail 1
    (2, 4, 36, 8),          # F 19: tail 3 -- registers only, the fourth one zero
    (2, 4, 38, 8),          # F 20: tail 4 -- the last tail that stays in registers
    (2, 4, 40, 8),          # F 21: tail 5 -- the first one that re-reads the bank
    (2, 4, 1150, 256),      # F 576: the largest MFMA form (K_main 512, tail 64, five load segments)
    (2, 4, 1152, 256),      # F 577: the first size past it, simple kernel
    (3, 9, 400, 100),       # F 201: K_main 128, tail 73, two load segments
    (3, 9, 1000, 250),      # F 501: K_main 256, tail 245, four load segments
    (2, 4, 600, 150),       # F 301: K_main 256, tail 45, three load segments
    (2, 7, 254, 64),        # F 128: tail 0, one load segment exactly full
    (2, 7, 441, 110),       # F 221: odd L (1211), tail 93
    (1, 1, 1024, 256),      # n_pass 1
    (1, 2, 1024, 256),      # n_pass 2 at T = 2
    (1, 3, 1024, 256),      # n_pass 2 at T = 3
    (2, 129, 64, 4),        # n_pass 30
    (1, 1000, 64, 2),       # n_pass 64, the limit
    (3, 175000, 16, 4),     # B L = 2 100 048: a second sweep of the combine kernel (and of the simple kernel)
    (40, 5, 64, 16),        # two row tiles, the last one partial (F 33)
    (70, 5, 128, 32),       # three row tiles, the last one partial (F 65)
]
ROW_RUN_CASES = [(40, 5, 64, 16), (70, 5, 128, 32)]
PASS_LIMIT_CASE = (1, 1000, 64, 2)
OVER_PASS_LIMIT_CASE = (1, 70, 16, 1)    # n_pass 70: refused before anything is launched

# realtime: (S, T, n_fft, hop, clock in s)
REALTIME_CASES = [
    (2, 2, 1024, 256, 0.0),       # four blocks per frame, three staging trips
    (2, 3, 400, 100, 600.0),      # a partial last block (400 = 256 + 144), one staging trip
    (1, 2, 4096, 1024, 60.0),     # F 2049: nine staging trips, sixteen blocks
    (3, 1, 16, 4, 1e4),           # small n_fft, large clock
    (2, 2, 1024, 256, 3600.0),    # large clock at the default size: c_k tau up to 5e8 rad
]
# op level, (S, T, F, N, clock)
REALTIME_LIMIT_CASES = [
    (1, 1, 4096, 8190, 1.0),      # 3 F floats = 48 KB exactly: the LDS limit
    (255, 257, 9, 16, 1.0),       # S T = 65535: the grid limit
]
REALTIME_REFUSED = [
    (1, 1, 4097, 8192),           # 3 F floats > 48 KB
    (256, 256, 9, 16),            # S T = 65536
]
LONG_STREAM = dict(S=2, n_fft=1024, hop=256, chunks=200, check_every=50)

# _offline_tables against F.interpolate: 17 (n_fft, hop) x 6 T
TABLE_SWEEP = [(g, T) for g in ((16, 1), (16, 4), (30, 8), (64, 2), (64, 4), (64, 16), (128, 32), (254, 64), (256, 64),
                                (400, 100), (441, 110), (512, 128), (1000, 250), (1024, 256), (1024, 100), (2048, 512),
                                (4096, 1024))
               for T in (1, 2, 3, 7, 33, 100)]


# ---- paths, restated from the code --------------------------------------------------------------------------------------
def n_bins(n_fft):
    return int(n_fft / 2 + 1)


def out_len(T, n_fft, hop):
    return hop * T + n_fft


def projection_form(K):
    """launch_mel_project: {'kernel': 'simple'} or the MFMA form's K_main, tail and load segments."""
    if K > SIMPLE_ABOVE or K < SIMPLE_BELOW:
        return {"kernel": "simple"}
    k_main = max(k for k in (512, 256, 128, 64, 32, 16) if k <= K)
    return {"kernel": "mfma", "k_main": k_main, "tail": K - k_main, "segments": cdiv(K, 128)}


def frame_below(T, L):
    """Frame below every output sample under align_corners=False: floor(max((n + 1/2) T / L - 1/2, 0)), in integers."""
    n = np.arange(L, dtype=np.int64)
    return np.minimum(np.maximum(((2 * n + 1) * T - L) // (2 * L), 0), T - 1)


def n_pass(T, n_fft, hop):
    """Frames that one block of 128 output samples touches, at most: from the frame below its first sample to the frame
    above its last one."""
    L = out_len(T, n_fft, hop)
    j0 = frame_below(T, L)
    j1 = np.minimum(j0 + 1, T - 1)
    b = np.arange(cdiv(L, COL_BLOCK))
    return int((j1[np.minimum(b * COL_BLOCK + COL_BLOCK - 1, L - 1)] - j0[b * COL_BLOCK]).max()) + 1


def row_tiles(B):
    return cdiv(B, GEMM_ROWS)


def combine_sweeps(B, L):
    return cdiv(B * L, SWEEP_OUTPUTS)


def offline_paths(case):
    """Names of the paths an offline case reaches."""
    B, T, n_fft, hop = case
    F, L = n_bins(n_fft), out_len(T, n_fft, hop)
    p = set()
    form = projection_form(F)
    blocks = cdiv(L, COL_BLOCK)
    if form["kernel"] == "simple":
        p.add("simple_above_576" if F > SIMPLE_ABOVE else "simple_below_16")
        p.add("simple_block_offsets" if blocks > 1 else "simple_one_block")
        if F >= 2049:
            p.add("simple_chain_2049")
        if B * L > SWEEP_OUTPUTS:
            p.add("simple_sweeps_2")
    else:
        tail = form["tail"]
        p.add("tail_0" if tail == 0 else "tail_1" if tail == 1 else "tail_2_4" if tail <= 4 else "tail_reread")
        p.add("segments_%d" % form["segments"])
        p.add("k_main_%d" % form["k_main"])
        p.add("row_tiles_%d" % min(row_tiles(B), 3))
        if row_tiles(B) > 1 and B % GEMM_ROWS:
            p.add("partial_last_tile")
    for edge in (16, 17, 576, 577):
        if F == edge:
            p.add("F_%d" % edge)
    P = n_pass(T, n_fft, hop)
    p.add("n_pass_%d" % P if P in (1, 2, 3, PASS_LIMIT) else "n_pass_many" if P >= 30 else "n_pass_4_29")
    if P == 2:
        p.add("n_pass_2_T%d" % T)
    if L % 2:
        p.add("L_odd")
    if L % 4:
        p.add("L_mod4")
    p.add("L_mod128_0" if L % COL_BLOCK == 0 else "L_mod128")
    p.add("combine_sweeps_%d" % combine_sweeps(B, L))
    return p


# path -> how many of OFFLINE_CASES reach it (test_sinebank_cases_cpu.py: deleting a case fails the count)
OFFLINE_PATH_COUNTS = {
    "simple_above_576": 3, "simple_below_16": 2, "simple_block_offsets": 4, "simple_one_block": 1, "simple_chain_2049": 1,
    "simple_sweeps_2": 1, "F_16": 1, "F_17": 1, "F_576": 1, "F_577": 1,
    "tail_0": 2, "tail_1": 8, "tail_2_4": 2, "tail_reread": 6,
    "segments_1": 10, "segments_2": 2, "segments_3": 1, "segments_4": 1, "segments_5": 4,
    "k_main_16": 5, "k_main_32": 3, "k_main_64": 1, "k_main_128": 3, "k_main_256": 2, "k_main_512": 4,
    "row_tiles_1": 16, "row_tiles_2": 1, "row_tiles_3": 1, "partial_last_tile": 2,
    "n_pass_1": 1, "n_pass_2": 3, "n_pass_2_T2": 1, "n_pass_2_T3": 2, "n_pass_3": 7, "n_pass_4_29": 9, "n_pass_many": 2, "n_pass_64": 1,
    "L_odd": 1, "L_mod4": 6, "L_mod128": 17, "L_mod128_0": 6, "combine_sweeps_1": 22, "combine_sweeps_2": 1,
}


def rt_blocks(N):
    return cdiv(N, 256)


def rt_staging_trips(F):
    return cdiv(F, 256)


def rt_refused(S, T, F):
    return S * T > RT_GRID_LIMIT or 3 * F * 4 > RT_LDS_BYTES


def realtime_paths(S, T, F, N, clock):
    p = {"blocks_%d" % rt_blocks(N) if rt_blocks(N) in (1, 4) else "blocks_many" if rt_blocks(N) > 4 else "blocks_2_3",
         "trips_1" if rt_staging_trips(F) == 1 else "trips_many"}
    if N % 256 and rt_blocks(N) > 1:
        p.add("partial_last_block")
    if F >= 2049:
        p.add("F_ge_2049")
    if clock >= 600:
        p.add("clock_minutes")
    if clock >= 3600:
        p.add("clock_hours")
    if 3 * F * 4 == RT_LDS_BYTES:
        p.add("lds_limit")
    if S * T == RT_GRID_LIMIT:
        p.add("grid_limit")
    return p


REALTIME_PATH_COUNTS = {"blocks_1": 2, "blocks_4": 2, "blocks_2_3": 1, "blocks_many": 2, "partial_last_block": 2,
                        "trips_1": 3, "trips_many": 4, "F_ge_2049": 2, "clock_minutes": 3, "clock_hours": 2,
                        "lds_limit": 1, "grid_limit": 1}


# ---- inputs, oracle and float64 model -------------------------------------------------------------------------------------
def _gen(case):
    seed = 0
    for v in case:
        seed = (seed * 1000003 + int(v * 7) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def offline_inputs(case):
    """(mag (B, T, F) = rand ** 2, different in every clip and frame; phase (F, 1))."""
    B, T, n_fft, hop = case
    g = _gen(case)
    F = n_bins(n_fft)
    return torch.rand(B, T, F, generator=g) ** 2, 2 * torch.pi * torch.rand(F, 1, generator=g)


@functools.lru_cache(maxsize=None)
def offline_oracle(case):
    mag, phase = offline_inputs(case)
    return O.sinebank_offline(mag, SR, case[2], case[3], phase)


def offline_model(mag, sr, n_fft, hop, phase):
    """float64 model of sinebank_offline: the oscillator argument in fp32 as the reference forms it, and the envelope
    interpolated in fp32 as the reference does (ATen's fp32 source index is off by up to T ulps of one frame, 1e-2 of a
    frame at T = 175000: like the argument, that is part of what the reference computes, and the kernel takes its
    weights from F.interpolate itself); then the sine, the envelope product and the sums in float64."""
    F = mag.shape[-1]
    freqs = torch.linspace(0, sr / 2, n_bins(n_fft)).view(1, -1, 1)
    L = out_len(mag.shape[-2], n_fft, hop)
    t = torch.linspace(0, L / sr, L).view(1, 1, -1)
    arg = 2 * torch.pi * freqs * t + phase.reshape(F, 1)                  # fp32
    x = mag / mag.abs().max()
    env = torch.nn.functional.interpolate(x.transpose(-2, -1), L, mode="linear").double() / (2 * np.pi)
    y = (env * torch.sin(arg.double())).sum(-2)
    return y / y.max()


@functools.lru_cache(maxsize=None)
def realtime_inputs(case, batch=None):
    """(mag batch + (T, F), phase batch + (1, F)); batch defaults to (S,)."""
    S, T, n_fft, hop, clock = case
    batch = (S,) if batch is None else tuple(batch)
    g = _gen(case + tuple(batch))
    F = n_bins(n_fft)
    return torch.rand(*batch, T, F, generator=g) ** 2, 2 * torch.pi * torch.rand(*batch, 1, F, generator=g)


@functools.lru_cache(maxsize=None)
def realtime_oracle(case, batch=None):
    """(frames, advanced clock) of the oracle for the case's chunk on a module whose clock reads `clock`."""
    mag, phase = realtime_inputs(case, batch)
    return O.sinebank_realtime(mag, SR, case[2], case[3], phase, torch.tensor(case[4]))


def realtime_tau(T, n_fft, hop, sr, clock):
    """Absolute time of every sample of the chunk's frames, fp32 as the reference forms it: (T, n_fft)."""
    tidx = torch.arange(n_fft).unsqueeze(0) + torch.arange(T).unsqueeze(1) * hop
    return tidx / sr + torch.tensor(clock, dtype=torch.float32)


def realtime_model_op(x, c, tau, phi):
    """float64 model at op level: x (S, T, F), c (F,), tau (T, N), phi (S, F) -> (S, T, N); argument in fp32."""
    out = torch.empty(x.shape[0], x.shape[1], tau.shape[-1], dtype=torch.float64)
    for s in range(x.shape[0]):                                           # per stream: bounds the (T, F, N) temporary
        arg = c.view(1, -1, 1) * tau.unsqueeze(1) + phi[s].view(1, -1, 1)   # fp32
        out[s] = (x[s].double().unsqueeze(-1) * torch.sin(arg.double())).sum(-2) / x.shape[-1]
    return out


def realtime_model(mag, sr, n_fft, hop, phase, clock):
    """float64 model of sinebank_realtime for mag batch + (T, F), phase batch + (1, F)."""
    T, F = mag.shape[-2], mag.shape[-1]
    c = 2 * torch.pi * torch.linspace(0, sr / 2, n_bins(n_fft))
    y = realtime_model_op(mag.reshape(-1, T, F), c, realtime_tau(T, n_fft, hop, sr, clock), phase.reshape(-1, F))
    return y.reshape(mag.shape[:-2] + (T, n_fft))


@functools.lru_cache(maxsize=None)
def realtime_limit_inputs(S, T, F, N, clock):
    """Op-level arguments (x, c, tau, phi) at a geometry no module has: N samples per frame, F bins."""
    g = _gen((S, T, F, N))
    x = torch.rand(S, T, F, generator=g) ** 2
    c = 2 * torch.pi * torch.linspace(0, SR / 2, F)
    tau = (torch.arange(N).unsqueeze(0) + torch.arange(T).unsqueeze(1) * (N // 4)) / SR + torch.tensor(clock)
    return x, c, tau, 2 * torch.pi * torch.rand(S, F, generator=g)


def envelope_from_tables(x, frames, W):
    """sum_p W[p, n] x[..., frames[p, n // 128]]: the envelope the three-pass contraction and the combine kernel build;
    x (..., T) float64, frames (P, blocks) frame indices, W (P, L)."""
    L = W.shape[1]
    blk = np.arange(L) // COL_BLOCK
    env = np.zeros(x.shape[:-1] + (L,))
    for p in range(W.shape[0]):
        env += W[p].astype(np.float64) * x[..., frames[p, blk]]
    return env


if __name__ == "__main__":
    for case in OFFLINE_CASES + [OVER_PASS_LIMIT_CASE]:
        B, T, n_fft, hop = case
        print(case, "F", n_bins(n_fft), "L", out_len(T, n_fft, hop), projection_form(n_bins(n_fft)), "n_pass",
              n_pass(T, n_fft, hop), sorted(offline_paths(case)))
    for S, T, n_fft, hop, clock in REALTIME_CASES:
        print((S, T, n_fft, hop, clock), sorted(realtime_paths(S, T, n_bins(n_fft), n_fft, clock)))

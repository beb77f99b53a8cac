"""The plan classes of the time-domain stages, as arithmetic on Python integers, and the cases that reach every one of them;
shared by test_sweep_cases_cpu.py and test_sweep_gpu.py.

Each stage's own case table (pqmf_cases, resample_cases, sinc_interp_cases, loudness_cases.HOPS, fft_convolve_cases) puts
its LENGTHS at the cut points of the plan that its listed parameters produce, but the parameters themselves -- (n_band, taps),
(orig, new), (a, b, Qi), hop, (K, block) -- are a handful of hand-picked points, and the index arithmetic of the kernels
changes with them.  For every stage this module has

  * a `*_plan` function that restates the plan arithmetic of the kernel source (csrc/pqmf.hip pq_plan, resample.hip rb_plan,
    sinc_interp.hip si_plan, sos_filter.hip's tile and hop walk, fft_convolve.hip's at_fft_convolve_plan and its unrolled
    partition loop) and a `*_classes` function that names the classes a case reaches.  test_sweep_cases_cpu.py holds every
    restatement against the library's own plan entry, so that it cannot drift from the code;
  * `*_UNIVERSE`, every class of the stage;
  * `*_NAMED`, the smallest parameters that reach each class the stage's table does not, and
  * `*_generated()`, 24 further parameter sets from numpy.random.default_rng(SEED) over the ranges the library accepts.  All
    randomness of the sweep lives here: the draws are described at each generator, and `chunk_lists` draws the chunkings of
    the streaming forms.

Nothing here inspects compiled code, and nothing reads a device."""
import math

import numpy as np

SEED = 20240611
GENERATED = 24


def _up4(v):
    return (v + 3) & ~3


def _coprime_pairs(rng, n, first=()):
    """n distinct coprime (orig, new), orig != new, both in 1 .. 64: `first` fixes the `new` of the leading pairs (their orig
    is drawn from 2 .. 64 until it is coprime to it), every other pair draws both sides from 1 .. 64 until the pair is
    coprime, unequal and new."""
    out = []
    while len(out) < n:
        new = first[len(out)] if len(out) < len(first) else int(rng.integers(1, 65))
        orig = int(rng.integers(2 if len(out) < len(first) else 1, 65))
        if orig != new and math.gcd(orig, new) == 1 and (orig, new) not in out:
            out.append((orig, new))
    return tuple(out)


# ---- PQMF (csrc/pqmf.hip) ------------------------------------------------------------------------------------------------
PQ_MIN_BAND, PQ_MAX_BAND, PQ_MAX_TAPS, PQ_LDS_BYTES, PQ_TILE = 2, 64, 4097, 160 * 1024, 1024
PQ_OWN_COPIES = (4, 8, 16, 32, 64)                    # band counts with a kernel compiled for them
PQ_UNROLL = 4                                         # the fold and accumulation loops walk G four groups at a time


def pqmf_plan(M, N):
    """pq_plan: dict of P, G, TB and the two LDS sizes in bytes, or None where at_pqmf_tile_blocks refuses (M, N)."""
    if M < PQ_MIN_BAND or M > PQ_MAX_BAND or N < 2 * M + 1 or N % 2 == 0 or N > PQ_MAX_TAPS:
        return None
    P, G = (N - 1) // 2, -(-N // (2 * M))
    Np = 2 * M * G
    TB = 64 * (PQ_TILE // 64 // M if M * 64 < PQ_TILE else 1)
    wlen, us = TB * M + Np - M, 2 * M + 1
    lo = 2 * G - 1 - P // M
    ys = _up4(TB + (M - 1 + P) // M + lo)
    lds_a = 4 * (_up4(Np) + 2 * M * _up4(M) + _up4(wlen) + TB * us)
    lds_s = 4 * (_up4(Np) + _up4(2 * M * M) + M * ys + ys * 2 * M)
    if lds_a > PQ_LDS_BYTES or lds_s > PQ_LDS_BYTES:
        return None
    return dict(P=P, G=G, TB=TB, lds_analysis=lds_a, lds_synthesis=lds_s)


def pqmf_classes(M, N, T):
    p = pqmf_plan(M, N)
    G, TB = p["G"], p["TB"]
    out = {"copy=own" if M in PQ_OWN_COPIES else "copy=general", "M%%4=%d" % (M % 4), "G%%4=%d" % (G % PQ_UNROLL),
           "G<4" if G < PQ_UNROLL else "G>=4", "P%M=0" if p["P"] % M == 0 else "P%M!=0", "TB=%d" % TB}
    if M >= 32 and G < PQ_UNROLL:
        out.add("M>=32,G<4")                          # the smallest filters of a wide bank
    if T < TB:
        out.add("T<TB")
    if T == TB:
        out.add("T=TB")
    if T > TB and T % TB:
        out.add("T ragged")
    if T >= 2 * TB:
        out.add("T several tiles")
    return out


PQ_UNIVERSE = ({"copy=own", "copy=general", "G<4", "G>=4", "P%M=0", "P%M!=0", "M>=32,G<4", "T<TB", "T=TB", "T ragged",
                "T several tiles"} | {"M%%4=%d" % i for i in range(4)} | {"G%%4=%d" % i for i in range(4)}
               | {"TB=%d" % t for t in (64, 128, 192, 256, 320, 512)})
# G = 4, 8, 5 (P = 4 M), 4; then G = 2 on the widest specialised copy and on the general copy next to the LDS maximum of u, v
PQ_NAMED = ((4, 31), (4, 63), (7, 57), (12, 95), (64, 129), (48, 97), (63, 127))


def pqmf_generated():
    """24 (M, N).  M: a permutation of 2 .. 8 (every tile size and every M mod 4 on both copies), then 9 draws from 9 .. 31
    and 8 from 32 .. 64.  G from 2 .. 9 (taps >= 2 M + 1 leaves no G = 1), N an odd number of the 2 M (G - 1) + 1 .. 2 M G - 1
    that have this G."""
    rng = np.random.default_rng(SEED + 1)
    Ms = ([int(m) for m in rng.permutation(np.arange(2, 9))] + [int(m) for m in rng.integers(9, 32, 9)]
          + [int(m) for m in rng.integers(32, 65, 8)])
    out = []
    for M in Ms:
        G = int(rng.integers(2, 10))
        out.append((M, 2 * M * (G - 1) + 1 + 2 * int(rng.integers(0, M))))
    return tuple(out)


def pqmf_random_pairs(n=300):
    """n (M, N) over M in 2 .. 64 and G in 2 .. 9, drawn as in pqmf_generated but with M uniform: all must be accepted."""
    rng = np.random.default_rng(SEED + 2)
    out = []
    for _ in range(n):
        M, G = int(rng.integers(2, 65)), int(rng.integers(2, 10))
        out.append((M, 2 * M * (G - 1) + 1 + 2 * int(rng.integers(0, M))))
    return tuple(out)


# ---- Resample backward (csrc/resample.hip, rb_plan) -------------------------------------------------------------------------
RB_TILE, RB_LDS_BYTES, RB_WINDOW_BYTES = 1024, 160 * 1024, 64 * 1024
RB_OWN_NEW = (1, 2, 3)
LPW, ROLLOFF = 6, 0.99                                # the converters' defaults


def resample_width(orig, new):
    """utils.audio_io.sinc_filter_bank's width (the only float arithmetic here: the library's own expression)."""
    return math.ceil(LPW * orig / (min(orig, new) * ROLLOFF))


def resample_plan(orig, new, taps=None, lead=None):
    """rb_plan: (TB, bank_in_lds, default TB), or None where it answers AT_EUNSUPPORTED."""
    width = resample_width(orig, new)
    taps = 2 * width + orig if taps is None else taps
    lead = width if lead is None else lead
    dlo, dhi = -((taps - 1 - lead) // orig), (lead + orig - 1) // orig            # Python's // is the floor
    halo = dhi - dlo
    default = 1 if orig >= RB_TILE else RB_TILE // orig
    TB = default
    while TB > 1 and (TB + halo) * new * 4 > RB_WINDOW_BYTES:
        TB //= 2
    window = _up4((TB + halo) * new) * 4
    if window > RB_LDS_BYTES or new * taps > 0x7fffffff // 4:
        return None
    return TB, window + new * taps * 4 <= RB_LDS_BYTES, default


def resample_classes(orig, new):
    TB, in_lds, default = resample_plan(orig, new)
    return {"new=%d" % new if new in RB_OWN_NEW else "new=general", "bank=lds" if in_lds else "bank=global",
            "tile=one block" if orig >= RB_TILE else "tile=default" if TB == default else "tile=shrunk"}


RB_UNIVERSE = {"new=1", "new=2", "new=3", "new=general", "bank=lds", "bank=global", "tile=default", "tile=shrunk",
               "tile=one block"}
# control rate to audio rate (the window of g shrinks the tile), its downsampling twin, and a bank of 4 MB at TB = 1
RB_NAMED = ((1, 24), (1, 64), (20, 441), (441, 20), (1025, 1024))
RB_STREAM_NAMED = RB_NAMED[:3]


def resample_generated():
    """24 coprime (orig, new) up to 64 on either side: the first six have new = 1, 2, 3, 1, 2, 3 (the specialised copies of
    the backward kernel), the rest are free (_coprime_pairs)."""
    return _coprime_pairs(np.random.default_rng(SEED + 3), GENERATED, first=(1, 2, 3, 1, 2, 3))


# ---- the bankless converter (csrc/sinc_interp.hip, si_plan) -----------------------------------------------------------------
SI_TILE, SI_LDS_BYTES, SI_WINDOW_BYTES = 1024, 160 * 1024, 64 * 1024


def sinc_qi(orig, new):
    """ops.sinc_table's Qi for reduced rates (the library's own float expression)."""
    return math.ceil(LPW * orig * new / (min(orig, new) * ROLLOFF)) - 1


def _si_window(T, a, b, Qi):
    return ((T - 1) * a + 2 * Qi) // b + 2


def sinc_plan(a, b, Qi):
    """si_plan: (T, table_in_lds), or None where it answers AT_EUNSUPPORTED."""
    T = SI_TILE
    while T > 1 and (T * a + 2 * Qi + 2 * b > 0x7fffffff or _si_window(T, a, b, Qi) * 4 > SI_WINDOW_BYTES):
        T //= 2
    if T * a + 2 * Qi + 2 * b > 0x7fffffff:
        return None
    window = _up4(_si_window(T, a, b, Qi)) * 4
    if window > SI_LDS_BYTES:
        return None
    table = (Qi + (Qi >> 5) + (Qi >> 10) + 1) * 4                              # the swizzled table
    return T, window + table <= SI_LDS_BYTES


def sinc_classes(orig, new):
    """The classes of both directions: the forward runs (a, b) = (orig, new), the backward (new, orig)."""
    Qi, out = sinc_qi(orig, new), set()
    for name, (a, b) in (("fwd", (orig, new)), ("bwd", (new, orig))):
        T, in_lds = sinc_plan(a, b, Qi)
        out |= {"%s:tile=%s" % (name, "1024" if T == SI_TILE else "shrunk"), "%s:table=%s" % (name, "lds" if in_lds else "global")}
    return out


SI_UNIVERSE = {"%s:%s" % (d, c) for d in ("fwd", "bwd") for c in ("tile=1024", "tile=shrunk", "table=lds", "table=global")}
# downsampling by more than 16 (the forward's tile shrinks) and the reverses (the backward's does); the last two are the
# converter of PitchShift(44100, n_steps=-60), 1378 -> 44100, and its reverse: a shrunk tile beside a table of 534 KB that
# stays in global memory
SI_NAMED = ((24, 1), (64, 1), (100, 3), (441, 20), (1, 24), (1, 64), (3, 100), (20, 441), (689, 22050), (22050, 689))
SI_BANK_BUILDABLE = SI_NAMED[:8]                      # the bank of the last two would hold gigabytes
PITCH_STEPS = (60, -60)                               # at sr 44100: 1411200 -> 44100 = (32, 1) and 1378 -> 44100 = (689, 22050)


def sinc_generated():
    """24 coprime (orig, new), both sides free in 1 .. 64 (_coprime_pairs)."""
    return _coprime_pairs(np.random.default_rng(SEED + 4), GENERATED)


# ---- the hop endings (csrc/sos_filter.hip) ----------------------------------------------------------------------------------
SOS_TILE, SOS_PER_LANE, SOS_WAVE = 4096, 16, 1024     # a tile, a lane's samples, a wavefront's samples
SOS_MIN_HOP = SOS_PER_LANE


def hop_plan(L, hop):
    """(tile, per_lane, nh, tiles), or None where at_sos_hop_power_plan refuses the hop."""
    if hop < SOS_MIN_HOP or hop > 0x7fffffff:
        return None
    return SOS_TILE, SOS_PER_LANE, L // hop, -(-L // SOS_TILE)


def hop_classes(L, hop):
    _, S, nh, tiles = hop_plan(L, hop)
    out = {"hop wave-aligned" if hop % SOS_WAVE == 0 else "hop lane-aligned" if hop % S == 0 else "hop unaligned",
           "hop<wave" if hop < SOS_WAVE else "wave<=hop<tile" if hop < SOS_TILE else "tile<=hop<2tile+1" if hop <= 2 * SOS_TILE
           else "hop holds a tile",                   # hop >= 2 tile + 1: some tile lies strictly inside one hop
           "tiles=1" if tiles == 1 else "tiles=2-4" if tiles <= 4 else "tiles>=5",
           "last hop ends inside a lane" if (nh * hop) % S else "last hop ends on a lane"}
    if tiles >= 5 and SOS_TILE % hop:
        out.add("tiles>=5, hop wraps")                # hop_off wraps several times; lane 0's hand-over runs in steady state
    return out


HOP_UNIVERSE = {"hop wave-aligned", "hop lane-aligned", "hop unaligned", "hop<wave", "wave<=hop<tile", "tile<=hop<2tile+1",
                "hop holds a tile", "tiles=1", "tiles=2-4", "tiles>=5", "last hop ends inside a lane", "last hop ends on a lane",
                "tiles>=5, hop wraps"}
HOP_NAMED_HOPS = (32, 1024, 2048, 9000)
HOP_LENGTHS = (SOS_TILE + 1, 3 * SOS_TILE, 5 * SOS_TILE + 3)
HOP_NAMED = tuple((L, hop) for hop in HOP_NAMED_HOPS for L in HOP_LENGTHS)
HOP_FILTERS = ("kweighting", "cascade4")


def hop_generated():
    """24 (L, hop): eight hops from 16 .. 1023, eight from 1024 .. 4095 and eight from 4096 .. 10000; every fourth draw is
    rounded down to a multiple of 16; L walks a row of one ragged tile and then HOP_LENGTHS, and a hop longer than its row
    takes the longest row instead (no row without a whole hop)."""
    rng = np.random.default_rng(SEED + 5)
    lengths = (SOS_TILE - 7,) + HOP_LENGTHS
    out = []
    for i, (lo, hi) in enumerate(((16, 1024), (1024, 4096), (4096, 10001)) * 8):
        hop = int(rng.integers(lo, hi))
        if i % 4 == 3:
            hop -= hop % 16
        L = lengths[i % 4]
        out.append((L if hop <= L else lengths[-1], hop))
    return tuple(out)


# ---- the spectral FIR of FFTConvolve (csrc/fft_convolve.hip, FirSteps / CorrSteps) -----------------------------------------------
FIR_TILE = 8                                          # output frames per lane, and the unrolled steps of the partition loop
FIR_BLOCKS = (128, 256, 512, 1024, 2048)
FIR_BLOCK = 128


def fir_plan(L, K, block):
    """at_fft_convolve_plan for a requested block: (B, T, P, frame_tile)."""
    assert block in FIR_BLOCKS
    return block, -(-(L + K - 1) // block), -(-K // block), FIR_TILE


def fir_classes(P, T):
    out = {"P%%8=%d" % (P % FIR_TILE), "P<8" if P < FIR_TILE else "P=8" if P == FIR_TILE else "P>8",
           "T<8" if T < FIR_TILE else "T=8" if T == FIR_TILE else "T>8"}
    if P > FIR_TILE:
        out.add("P>8,P%%8=%d" % (P % FIR_TILE))       # how far a later trip of the unrolled p0 loop runs
    return out


FIR_UNIVERSE = ({"P<8", "P=8", "P>8", "T<8", "T=8", "T>8"} | {"P%%8=%d" % i for i in range(8)}
                | {"P>8,P%%8=%d" % i for i in range(8)})
FIR_NAMED_P = (7, 9, 16, 17)
FIR_NAMED_T = (7, 8, 9)
# at_spectral_fir and at_spectral_fir_corr take T and P apart: every (P, T) of the two lists
FIR_NAMED = tuple((P, T) for P in FIR_NAMED_P for T in FIR_NAMED_T)


def fir_lengths(P, block=FIR_BLOCK):
    """(L, T) of the end-to-end cases at K = P block.  The full result has L + K - 1 >= P block samples, so T >= P: the T of
    FIR_NAMED_T that a convolution can have (all three at P = 7, T = 9 at P = 9), else T = P, P + 1 and P + 2."""
    K = P * block
    want = [T for T in FIR_NAMED_T if T >= P] or [P, P + 1, P + 2]
    out = []
    for T in want:
        L = 1 if T == P else (T - P) * block - 28     # (T - 1) block < L + K - 1 <= T block
        assert fir_plan(L, K, block)[1:3] == (T, P)
        out.append((L, T))
    return tuple(out)


def fir_generated():
    """24 (P, T): P a permutation of 1 .. 24 (every count of the first three trips of the unrolled loop once), T from 1 .. 17."""
    rng = np.random.default_rng(SEED + 6)
    return tuple((int(P), int(rng.integers(1, 18))) for P in rng.permutation(np.arange(1, 25)))


# ---- the chunkings of the streaming forms ---------------------------------------------------------------------------------
def chunk_lists(key, tile, lists=3, chunks=4):
    """`lists` chunk lists of `chunks` sizes each, drawn from 1 .. tile + 1, for the stream named by the integers `key`."""
    rng = np.random.default_rng([SEED, 7] + [int(k) for k in key])
    return tuple(tuple(int(c) for c in rng.integers(1, tile + 2, chunks)) for _ in range(lists))

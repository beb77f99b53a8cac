"""The MFCC backward's dispatch (at_mfcc_backward, autograd.MfccFunction), restated for the CPU, and the sweep of
test_mfcc_grad_gpu.py that drives every class of it and every path of MFCC.forward.

test_mfcc_grad_cpu.py checks that the sweep reaches every class named here; the GPU file runs it.  The arithmetic follows
csrc/mfcc_grad.hip (launch_mfcc_backward, mfcc_bwd_kernel), autograd.py (mfcc_chunk_clips) and transforms/mel.py
(MFCC._forward_plain)."""

TILE = 32                   # kMfccTile: frames of one clip per workgroup tile
LDS_BUDGET = 160 * 1024     # kBandLdsBudget (csrc/band_plan.h)
CHUNK_ELEMS = 1 << 26       # autograd.MFCC_CHUNK_ELEMS: complex64 elements of spectrum per chunk (512 MiB)


def frames(n_fft, hop, L):
    """T of the centred, reflect-padded STFT."""
    return 1 + (L - (n_fft & 1)) // hop


def chunk_clips(B, T, n_fft):
    """autograd.mfcc_chunk_clips: the most clips whose spectrum stays within CHUNK_ELEMS, at least 1."""
    per_clip = T * (n_fft // 2 + 1)
    return min(max(CHUNK_ELEMS // per_clip, 1), B)


def tiles(T):
    """(tiles per clip, frames of the last one): a tile never spans two clips, the last one of a clip may be short."""
    per_clip = -(-T // TILE)
    return per_clip, T - (per_clip - 1) * TILE


def kernel_class(K, N, C, t_nnz, f_nnz=None):
    """The kernel launch_mfcc_backward picks.  t_nnz / f_nnz: lengths of bank_columns' weight arrays of the transposed
    / forward bank (trailing zero included); f_nnz None: the mel power route (no DCT, C == N)."""
    dct = f_nnz is not None
    gs = C | 1
    g_bytes = 4 * ((TILE * gs + 3) // 4 * 4)
    k_pad, n_pad = (K + 63) // 64 * 64, (N + 63) // 64 * 64
    per_wave = 4 * (k_pad + n_pad) if dct else 0
    if g_bytes > LDS_BUDGET:
        return "unsupported"
    tab = 3 * K + t_nnz + (3 * N + f_nnz + C * N if dct else 0)
    tab = (tab + 3) // 4 * 4
    lds = 4 * tab + g_bytes + 4 * per_wave
    suffix = "_dct" if dct else "_mel"
    if lds <= LDS_BUDGET:
        if K <= 9 * 64:
            return "lds_kit9" + suffix
        return ("lds_kit0_big" if lds > 64 * 1024 else "lds_kit0") + suffix
    if dct and g_bytes + 4 * per_wave > LDS_BUDGET:
        return "unsupported"
    return "global" + suffix


KERNEL_CLASSES = {"lds_kit9_mel", "lds_kit0_mel", "lds_kit0_big_mel", "global_mel",
                  "lds_kit9_dct", "lds_kit0_dct", "lds_kit0_big_dct", "global_dct"}
# MFCC._forward_plain: the fused 1024 / 256 kernel (mel power; log mel + DCT), the single n_fft 2048 / 512 kernels (the
# same two), the generic STFT + walk (the same two)
FORWARD_PATHS = {"fused", "fused_dct", "single", "single_dct", "generic", "generic_dct"}


def forward_path(mod, L):
    """The branch of MFCC._forward_plain a float32 (B, L) input takes."""
    suffix = "_dct" if mod.n_mfcc is not None else ""
    if mod.n_fft == 1024 and mod.hop_length == 256 and mod._band.fusable and L > 512 and not (L & 1):
        return "fused" + suffix
    if ((mod.n_fft == 2048 and mod._band.fusable2048) or (mod.n_fft == 512 and mod._band.fusable512)) \
            and L > mod.n_fft // 2:
        return "single" + suffix
    return "generic" + suffix


def module_class(mod):
    """kernel_class of an MFCC, from bank_columns of its bank (as autograd._mfcc_tables builds them)."""
    from acids_transforms_amd.utils.banded import bank_columns
    K, N = mod.fbank.shape
    t = bank_columns(mod.fbank.transpose(-2, -1))
    if mod.n_mfcc is None:
        return kernel_class(K, N, N, len(t[3]))
    return kernel_class(K, N, mod.n_mfcc, len(t[3]), len(bank_columns(mod.fbank)[3]))


# ---- the parity grid -------------------------------------------------------------------------------------------------
# (name, n_fft, hop, n_mels, batch shapes).  Every case also runs a (3, 2, n_fft / 2 + 1) batch: the shortest clip the
# reflect padding takes.
SIZES = [
    # T = 36 (one full tile and a short one), then T = 64 (two full tiles): even lengths, the fused kernel
    ("1024_even", 1024, 256, 128, [(2, 9000), (1, 16128)]),
    ("1024_odd", 1024, 256, 128, [(2, 9001)]),                 # odd length: STFT + walk
    ("1024_hop100", 1024, 100, 128, [(2, 7000)]),              # T = 71
    ("2048_m128", 2048, 512, 128, [(2, 30000)]),               # the single n_fft 2048 kernel
    ("2048_m40", 2048, 512, 40, [(2, 30000)]),                 # bands of 168 bins: not fusable, STFT + walk
    ("512_m64", 512, 128, 64, [(2, 9001)]),                    # the single n_fft 512 kernel
    ("4096_m128", 4096, 1024, 128, [(2, 50000)]),
    ("256_m40", 256, 64, 40, [(2, 5000)]),
    ("400_m40", 400, 160, 40, [(2, 16000)]),
    ("8192_m128", 8192, 2048, 128, [(2, 40000)]),
    ("16384_m128", 16384, 4096, 128, [(1, 50000)]),            # K = 8193: the tables stay in global memory
]
POWERS = (1, 2)
NORMS = (None, "gaussian")


def n_mfcc_of(n_mels):
    return (None, min(40, n_mels))


def shapes_of(case):
    _, n, _, _, shapes = case
    return list(shapes) + [(3, 2, n // 2 + 1)]


def module_of(case, power=2, n_mfcc=None, norm=None):
    import acids_transforms_amd as A
    _, n, h, n_mels, _ = case
    return A.MFCC(n_fft=n, hop_length=h, n_mels=n_mels, power=power, n_mfcc=n_mfcc, norm_mode=norm)


# ---- the bench-size cases --------------------------------------------------------------------------------------------
BENCH = (1024, 256, 176400, 1024)       # n_fft, hop, samples, clips: 5 chunks of 189 clips and one of 79
# both sides of a chunk boundary at the start and at the end, and the short last chunk's ends
BENCH_CLIPS = (0, 188, 189, 944, 945, 1023)

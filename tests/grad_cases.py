"""The backward launchers' dispatch, restated for the CPU, and the sweeps of test_grad_paths_gpu.py that drive every
path of it.

test_grad_cases_cpu.py checks that the sweeps reach every class named here; the GPU file runs them.  The arithmetic
follows csrc/capi.hip (at_irfft_frames, adj_chunk_clips, at_stft_backward) and csrc/autograd.hip (launch_adj_ola_fold,
adj_ola_fold_kernel, launch_magnitude_backward)."""

CHUNK_FLOATS = 1 << 28      # adj_chunk_clips: a chunk's irFFT frames stay within 1 GiB
GRID_Y = 65535              # launch_adj_ola_fold: rows of blocks, one per clip, at most this many
LDS_BUDGET = 160 * 1024     # kBandLdsBudget (csrc/band_plan.h)


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def irfft_family(n_fft):
    """The irFFT kernel at_irfft_frames picks (the adjoint's workspace is 256-byte aligned, so every alignment test
    passes)."""
    if n_fft in (1024, 2048, 4096, 512):
        return str(n_fft)
    if n_fft in (128, 256):
        return "small"
    if not is_pow2(n_fft) or n_fft < 8:
        return "mixed"
    return "generic"


def frames(n_fft, hop, L):
    """T of at_stft_backward (torch.stft's frame count of a reflect-padded clip)."""
    return 1 + (L - (n_fft & 1)) // hop


def chunk_clips(B, T, n_fft):
    """adj_chunk_clips."""
    per_clip = T * n_fft
    c = CHUNK_FLOATS // per_clip if per_clip > 0 else B
    return min(max(c, 1), B)


def workspace_bytes(B, T, n_fft):
    """at_stft_backward_workspace_bytes: the scaled window's 256-byte slot, then one chunk of frames."""
    return (n_fft * 4 + 255) // 256 * 256 + chunk_clips(B, T, n_fft) * T * n_fft * 4


def adjoint_class(n_fft, hop, B, L):
    """The path of one at_stft_backward call, as a dict."""
    P = n_fft // 2
    T = frames(n_fft, hop, L)
    chunk = chunk_clips(B, T, n_fft)
    n_chunks = -(-B // chunk)
    vec4 = hop % 4 == 0 and n_fft % 8 == 0
    return {
        "family": irfft_family(n_fft),
        "vec4": vec4,
        # samples s0 > P with s0 + 3 < L - P - 1 take adj_dp4; the group that ends at L - P - 1 (residue 3) holds the
        # first right-fold sample, which reads the last padded sample when hop divides L
        "residue": (L - P - 1) % 4,
        "vec4_interior": vec4 and (L - P - 5) // 4 * 4 > P,
        "hop_divides_L": L % hop == 0,
        "hop_vs_n": "below" if hop < n_fft else ("equal" if hop == n_fft else "above"),
        "T": T,
        "chunk": chunk,
        "n_chunks": n_chunks,
        "last_chunk": B - (n_chunks - 1) * chunk,
        "clip_loop": chunk > GRID_Y,
    }


def magnitude_bwd_class(K, N, f_nnz, t_nnz):
    """The kernel launch_magnitude_backward picks for a (K x N) bank whose forward / transposed tables hold f_nnz /
    t_nnz weights (bank_columns' weight arrays, trailing zero included); f_nnz = None: mel=False."""
    if f_nnz is None:
        return "pointwise"
    k_pad, n_pad = (K + 63) // 64 * 64, (N + 63) // 64 * 64
    per_wave = 4 * (k_pad + n_pad)
    tab = (3 * (N + K) + f_nnz + t_nnz + 3) // 4 * 4
    if tab * 4 + 4 * per_wave <= LDS_BUDGET:
        if K <= 9 * 64:
            return "lds_kit9"
        return "lds_kit0_big" if tab * 4 + 4 * per_wave > 64 * 1024 else "lds_kit0"
    if per_wave > LDS_BUDGET:
        return "unsupported"
    return "global_w%d" % min(4, LDS_BUDGET // per_wave)


ADJ_FAMILIES = {"1024", "2048", "4096", "512", "small", "mixed", "generic"}
MAG_CLASSES = {"pointwise", "lds_kit9", "lds_kit0", "lds_kit0_big", "global_w4", "global_w2"}

# ---- the STFT / DGT adjoint sweep ----------------------------------------------------------------------------------
ADJ_SIZES = [2, 4, 6, 8, 12, 16, 32, 64, 77, 254, 256, 1000, 1536, 2401, 6000, 8191, 8192, 12000, 16384]
# hop = n and hop = n + n/3 (frames leave samples uncovered) at these sizes; hop = 1 at these
WIDE_HOP_SIZES = (6, 16, 77, 256, 1000, 8192)
HOP1_SIZES = (6, 16)


def adj_hops(n):
    hops = [max(1, n // 4)]
    odd = next(h for h in (n // 4 + 1, n // 4 + 2, n // 4 + 3) if h % 4 != 0)   # the scalar interior path
    hops.append(max(1, odd))
    if n in WIDE_HOP_SIZES:
        hops += [n, n + n // 3]
    if n in HOP1_SIZES:
        hops.append(1)
    return list(dict.fromkeys(h for h in hops if h >= 1))


def adj_lengths(n, h):
    """P + 1, P + 2, an odd length below n, a multiple of hop long enough to hold vec4 interior groups, and the three
    lengths after it (every residue of (L - P - 1) % 4)."""
    P = n // 2
    M = h * -(-(2 * n + 16) // h)
    Ls = [P + 1, P + 2]
    odd = n - 1 if (n - 1) % 2 == 1 else n - 2
    if odd > P + 2:
        Ls.append(odd)
    Ls += [M, M + 1, M + 2, M + 3]
    return list(dict.fromkeys(L for L in Ls if L > P))


ADJ_SWEEP = [(n, h) for n in ADJ_SIZES for h in adj_hops(n)]
# hop | L at the fast sizes (added to test_autograd_gpu.py's grid): 16384 at 1024/256, 8192 at 512/128
FAST_HOP_DIVIDES = [(1024, 256, 16384), (1024, 128, 8192), (1024, 512, 4096), (512, 128, 8192), (2048, 512, 16384),
                    (4096, 1024, 16384)]

# chunked and big-batch adjoints: (name, n_fft, hop, L, B, clips compared against float64)
BIG_ADJ = {
    # 378 + 378 + 44 clips: both sides of each chunk boundary, and the short last chunk
    "three_chunks": (4096, 1024, 176400, 800, (0, 377, 378, 755, 756, 799)),
    # one clip's frames exceed 2^28 floats: a chunk of 1
    "chunk_of_one": (1024, 1, 300000, 2, (0, 1)),
    # 140000 clips in one chunk: the grid's 65535 rows loop three times
    "clip_loop": (128, 32, 100, 140000, (0, 1, 65534, 65535, 65536, 131069, 131070, 131071, 139999)),
}

# ---- the Magnitude backward sweep ------------------------------------------------------------------------------------
# (name, Magnitude kwargs, rows shape); "dense" builds a random dense bank and loads it with load_state_dict
MAG_CASES = [
    ("n256", {"n_fft": 256}, (2, 5)),
    ("n512", {"n_fft": 512}, (2, 5)),
    ("n1536", {"n_fft": 1536}, (2, 5)),
    ("n2048_m80", {"n_fft": 2048, "n_mels": 80}, (2, 5)),
    ("n2048_m128", {"n_fft": 2048, "n_mels": 128}, (2, 5)),
    ("n2048", {"n_fft": 2048}, (2, 5)),
    ("n3000", {"n_fft": 3000}, (2, 5)),
    ("n4096_m128", {"n_fft": 4096, "n_mels": 128}, (2, 5)),
    ("n4096", {"n_fft": 4096}, (1, 3)),
    ("n8192", {"n_fft": 8192}, (1, 3)),
    ("n8192_m80", {"n_fft": 8192, "n_mels": 80}, (1, 3)),
    ("n16384", {"n_fft": 16384}, (1, 3)),
    ("n1024_m1", {"n_fft": 1024, "n_mels": 1}, (2, 5)),
    ("n1024_m520", {"n_fft": 1024, "n_mels": 520}, (2, 5)),
    ("n1024_dense", {"n_fft": 1024, "n_mels": 96, "dense": True}, (2, 5)),
    ("n2048_nonyq", {"n_fft": 2048, "n_mels": 128, "keep_nyquist": False}, (2, 5)),
    ("n2048_bf16", {"n_fft": 2048, "n_mels": 128, "bank_dtype": "bf16"}, (2, 5)),
    ("n1024_off", {"n_fft": 1024, "mel": False}, (2, 5)),
    ("n8192_off", {"n_fft": 8192, "mel": False}, (1, 3)),
    # rows that leave waves of a workgroup idle
    ("rows1", {"n_fft": 1024}, (1, 1)),
    ("rows3", {"n_fft": 2048}, (1, 3)),
    ("rows5", {"n_fft": 16384}, (1, 5)),
]
# (contrast, norm) per case: the two logs with the default norm, one log10 / gaussian
MAG_MODES = [("log1p", "unipolar"), ("log", "bipolar"), ("log10", "gaussian")]
# many rows: several grid-stride passes of the banded and pointwise kernels
MANY_ROWS = {"banked": ({"n_fft": 1024, "n_mels": 128}, (300, 690)), "pointwise": ({"n_fft": 1024, "mel": False}, (300, 690))}


def magnitude_module(kw, seed=0):
    """The (CPU) Magnitude a MAG_CASES entry builds; a "dense" case loads a random dense bank of the same shape."""
    import torch
    import acids_transforms_amd as A
    kw = dict(kw)
    dense = kw.pop("dense", False)
    mod = A.Magnitude(**kw)
    if dense:
        g = torch.Generator().manual_seed(seed)
        sd = mod.state_dict()
        sd["mel_bank"] = torch.rand(mod.mel_bank.shape, generator=g) / mod.mel_bank.shape[-2]
        mod.load_state_dict(sd)
    return mod


def module_class(mod):
    """magnitude_bwd_class of a Magnitude, from bank_columns of its bank (as autograd._bank_tables builds them)."""
    from acids_transforms_amd.utils.banded import bank_columns
    K = mod.n_fft // 2 + 1
    if not mod.mel:
        return magnitude_bwd_class(K, K, None, None)
    bank = mod.mel_bank
    f = bank_columns(bank)
    t = bank_columns(bank.transpose(-2, -1))
    return magnitude_bwd_class(bank.shape[-2], bank.shape[-1], len(f[3]), len(t[3]))

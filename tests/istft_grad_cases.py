"""The ISTFT adjoint's dispatch (at_istft_backward), restated for the CPU, and the sweep of test_istft_grad_gpu.py that
drives every path of it.

test_istft_grad_cpu.py checks that the sweep reaches every class named here; the GPU file runs it.  The arithmetic
follows csrc/capi.hip (istft_adj_chunk_clips, at_istft_backward_workspace_bytes, at_istft_backward, at_stft_forward)."""

CHUNK_FLOATS = 1 << 28      # istft_adj_chunk_clips: a chunk's u and polar rows stay within 1 GiB


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def family(n_fft):
    """The forward kernel that transforms the frames of u: at_stft_forward's with center = 0 on a 256-byte aligned
    workspace (the frame-at-a-time register kernels at 1024 / 2048 / 4096), the generic kernel directly at n_fft 128 /
    256 / 512."""
    if n_fft in (1024, 2048, 4096):
        return str(n_fft)
    if n_fft in (128, 256, 512):
        return "generic"
    if not is_pow2(n_fft) or n_fft < 8:
        return "mixed"
    return "generic"


def padded(n_fft, hop, T):
    return n_fft + hop * (T - 1)


def out_len(n_fft, hop, T):
    return hop * (T - 1) + (n_fft & 1)


def chunk_clips(B, T, n_fft, hop):
    """istft_adj_chunk_clips: u (P floats) and the polar form's rows (T F complex) per clip."""
    per_clip = padded(n_fft, hop, T) + 2 * T * (n_fft // 2 + 1)
    return min(max(CHUNK_FLOATS // per_clip, 1), B)


def workspace_bytes(B, T, n_fft, hop):
    """at_istft_backward_workspace_bytes: the scaled window's 256-byte slot, u rounded to 256 bytes, then the rows of
    the polar form."""
    c = chunk_clips(B, T, n_fft, hop)
    return (n_fft * 4 + 255) // 256 * 256 + (c * padded(n_fft, hop, T) * 4 + 255) // 256 * 256 + \
        c * T * (n_fft // 2 + 1) * 8


def path_class(n_fft, hop, B, T, polar=False):
    """The path of one at_istft_backward call, as a dict."""
    if T == 1 and not n_fft & 1:
        return {"family": "zeros", "polar": polar, "chunks": 0}
    return {"family": family(n_fft), "polar": polar, "chunks": -(-B // chunk_clips(B, T, n_fft, hop))}


FAMILIES = {"1024", "2048", "4096", "generic", "mixed", "zeros"}

# parity sweep of test_istft_grad_gpu.py: (n_fft, hop), frame counts T (1, 2, fewer than n / h, a few hundred), and
# one (3, 2, T, F) batch per pair
PAIRS = [(1024, 256), (1024, 128), (1024, 512), (1024, 300), (512, 128), (2048, 512), (4096, 1024), (256, 64), (128, 32),
         (400, 160), (441, 110), (9, 3), (64, 16)]


def frame_counts(n, h):
    short = max(2, n // h - 1)
    return sorted({1, 2, short, 300 if n <= 1024 else 120})


BATCH_T = 7                 # the (3, 2, T, F) batch
# hops of the misaligned-pointer test (n_fft 1024, the default module and the bench shape among them)
MISALIGNED_HOPS = (128, 256, 300, 512)
# a case cut into chunks: (n_fft, hop, T, B) with at least two chunks; clips alone, or in a batch of 7, for the rest
CHUNKED = (16, 4, 1200000, 16)
BATCH7 = [(1024, 256, 37), (1024, 300, 37), (512, 128, 21), (2048, 512, 11), (4096, 1024, 9), (256, 64, 13),
          (128, 32, 23), (441, 110, 9), (8192, 2048, 5)]
BENCH = (1024, 690, 1024, 256)   # B, T, n_fft, hop


def sweep_classes():
    """Every (case, class) the GPU sweep runs."""
    out = []
    for n, h in PAIRS:
        for T in frame_counts(n, h) + [BATCH_T]:
            B = 6 if T == BATCH_T else 1
            for polar in (False, True):
                out.append(((n, h, B, T, polar), path_class(n, h, B, T, polar)))
    n, h, T, B = CHUNKED
    out.append((CHUNKED, path_class(n, h, B, T)))
    for n, h, T in BATCH7:
        out.append(((n, h, 7, T), path_class(n, h, 7, T)))
    return out

"""Case table and float64 restatement of the streaming partitioned convolution (transforms.RealtimeImpulseResponse,
ops.fft_convolve_stream, at_spectral_fir_stream of csrc/fft_convolve.hip), shared by test_convolve_stream_cpu.py and
test_convolve_stream_gpu.py.

The ORACLE stays numpy.convolve (fft_convolve_cases.oracle).  `stream` restates the algorithm as the module runs it: the
tail of B samples, the ring of R = P - 1 + 8 spectra with its `head`, chunks walked in sub-chunks of at most 8 blocks, and
"a frame the stream has not received yet is a frame of zeros".  `chunk_gradients` is the gradient reference: float64 conv1d
autograd over one chunk with everything before the chunk a constant."""
import functools

import numpy as np
import torch

import fft_convolve_cases as C

BLOCK = C.BLOCK                                   # 128, forced
STREAM_BLOCKS = 40
LENGTH = STREAM_BLOCKS * BLOCK                    # 5120 samples
TAPS = (1, 128, 129, 300, 1000, 1100, 2200)       # P = 1, 1, 2, 3, 8, 9 (second round of the unrolled p loop), 18
CHUNKINGS = ((1,) * 40, (8,) * 5, (3, 8, 1, 9, 16, 3))       # in blocks; 9 and 16 are walked in sub-chunks
LEADS = C.LEADS
# (block, K, rows): one case per other block of the ladder, a stream of 6 blocks as chunks of (1, 3, 2)
BLOCK_CASES = ((256, 600, 3), (512, 1100, 3), (1024, 2500, 3), (2048, 4200, 2))
BLOCK_CHUNKS = (1, 3, 2)
MAX_FRAMES = 8
TOL = C.TOL


def data(K, B=BLOCK, blocks=STREAM_BLOCKS, rows=C.ROWS):
    """x (rows, blocks B) and h (K,) float32, and a cotangent g like x (fft_convolve_cases.data at L = blocks B)."""
    d = C.data(blocks * B, K, rows)
    return d["x"], d["h"], d["g_same"]


@functools.lru_cache(maxsize=None)
def reference(K, B=BLOCK, blocks=STREAM_BLOCKS, rows=C.ROWS):
    """numpy.convolve(x, h)[:L] per row, float64."""
    x, h, _ = data(K, B, blocks, rows)
    return C.oracle(x, h, "full")[:, :blocks * B]


def stream(x, h, B, chunks, R=None):
    """The streaming algorithm in float64: x (rows, L) and h (K,) float64 torch, chunks in blocks -> (rows, L)."""
    rows, L = x.shape
    P = -(-h.shape[0] // B)
    R = P - 1 + MAX_FRAMES if R is None else R
    H = C._filter_spectrum(h[None], B, P)[0]                               # (P, F)
    tail = torch.zeros(rows, B, dtype=x.dtype)
    ring = torch.zeros(rows, R, B + 1, dtype=torch.complex128)            # zeros: frames that never arrived
    head, out, a = 0, [], 0
    for n in chunks:
        for b0 in range(0, n, MAX_FRAMES):
            Tc = min(MAX_FRAMES, n - b0)
            stage = torch.cat([tail, x[:, a:a + Tc * B]], dim=-1)
            Xc = torch.fft.rfft(stage.unfold(-1, 2 * B, B), dim=-1)        # (rows, Tc, F)
            Y = torch.zeros_like(Xc)
            for t in range(Tc):
                for p in range(P):                                         # no term is skipped
                    s = t - p
                    V = Xc[:, s] if s >= 0 else ring[:, (head + s) % R]
                    Y[:, t] += H[p] * V
            for t in range(Tc):
                ring[:, (head + t) % R] = Xc[:, t]
            head = (head + Tc) % R
            out.append(torch.fft.irfft(Y, n=2 * B, dim=-1)[..., B:].reshape(rows, Tc * B))
            tail = stage[:, -B:]
            a += Tc * B
    assert a == L
    return torch.cat(out, dim=-1)


def chunk_gradients(x, h, g, B, chunks):
    """float64 conv1d autograd, chunk by chunk, the samples before the chunk a constant: x (rows, L), h (K,), g (rows, L)
    -> (gx (rows, L): every chunk's own gradient side by side, gh (K,): summed over the chunks, [gh of every chunk])."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    h = torch.as_tensor(np.asarray(h, dtype=np.float64))
    g = torch.as_tensor(np.asarray(g, dtype=np.float64))
    K = h.shape[0]
    gx, ghs, a = torch.zeros_like(x), [], 0
    for n in chunks:
        b = a + n * B
        lo = max(0, a - (K - 1))
        xc = x[:, a:b].clone().requires_grad_()
        hh = h.clone().requires_grad_()
        xin = torch.nn.functional.pad(torch.cat([x[:, lo:a], xc], dim=-1), (K - 1, 0))
        y = torch.nn.functional.conv1d(xin[:, None], hh.flip(-1)[None, None])[:, 0][:, a - lo:]
        y.backward(g[:, a:b])
        gx[:, a:b] = xc.grad
        ghs.append(hh.grad)
        a = b
    return gx.numpy(), torch.stack(ghs).sum(0).numpy(), [v.numpy() for v in ghs]

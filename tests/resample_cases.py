"""Float64 restatement of the sample-rate converter (utils.Resample / RealtimeResample, csrc/resample.hip), its adjoint
and its streaming form, and the case table shared by test_resample_grad_cpu.py and test_resample_grad_gpu.py.

Rates are reduced by their gcd to (orig, new); width and the (new, taps) float32 bank h, taps = 2 width + orig, come from
utils.audio_io.sinc_filter_bank.  The MODEL is torchaudio's conv1d construction on that float32-rounded bank taken as
float64: pad (width, width + orig), conv1d with stride orig, transpose, reshape, crop to ceil(new L / orig); torch's own
float64 autograd on the CPU differentiates it.  The ADJOINT is written from the formula the kernel is written from:
    gx[n] = sum over (i, j) with o = i new + j < out_len and 0 <= k = n - i orig + lead < taps of h[j][k] g[o]
with lead = width offline and lead = Ha in a stream.  The STREAM is a valid conv1d over [state | chunk]:
    out[t new + j] = sum_k h[j][k] v[t orig + k],   D = ceil(width / orig),   Ha = D orig + width."""
import functools

import numpy as np
import torch

from acids_transforms_amd import ops
from acids_transforms_amd.utils.audio_io import sinc_filter_bank

RATIOS = ((1, 2), (2, 1), (3, 2), (2, 3), (147, 160), (160, 147), (441, 160), (80, 441))
LEADS = ((1,), (3,), (2, 2))                       # 1 and 3 rows, and a leading shape
STREAM_RATIOS = ((3, 2), (147, 160), (441, 160))
# blocks per chunk of the mixed chunking of a stream; (3, 2) is long enough for more than one workgroup of outputs
STREAM_BLOCKS = {(3, 2): (1, 2, 7, 200, 90), (147, 160): (1, 2, 3, 5), (441, 160): (1, 2, 3, 5)}


@functools.lru_cache(maxsize=None)
def bank(orig, new):
    """(h (new, taps) float32 torch, width)."""
    return sinc_filter_bank(orig, new)


def taps_of(orig, new):
    return 2 * bank(orig, new)[1] + orig


def plan(orig, new, lead=None):
    """(tile_blocks, bank_in_lds) of the backward kernel; lead defaults to width."""
    width = bank(orig, new)[1]
    return ops.resample_backward_plan(orig, new, 2 * width + orig, width if lead is None else lead)


def out_len(L, orig, new):
    return -(-new * L // orig)


def stream_sizes(orig, new):
    """(D, Ha)."""
    width = bank(orig, new)[1]
    D = -(-width // orig)
    return D, D * orig + width


def lengths(orig, new):
    """The clip lengths of a ratio: around one block, both sides of a tile edge, several tiles with a cropped block."""
    tb = plan(orig, new)[0]
    want = (1, orig - 1, orig, orig + 1, tb * orig - 1, tb * orig, tb * orig + 1, 3 * tb * orig + 5)
    return tuple(sorted({L for L in want if L > 0}))


def audio(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1)


def model(x, orig, new):
    """x (..., L) float64 -> (..., ceil(new L / orig)) float64."""
    h, width = bank(orig, new)
    lead, L = tuple(x.shape[:-1]), x.shape[-1]
    xp = torch.nn.functional.pad(x.reshape(-1, 1, L), (width, width + orig))
    y = torch.nn.functional.conv1d(xp, h.double().unsqueeze(1), stride=orig)          # (rows, new, blocks)
    y = y.transpose(1, 2).reshape(y.shape[0], -1)[..., :out_len(L, orig, new)]
    return y.reshape(lead + (y.shape[-1],))


@functools.lru_cache(maxsize=None)
def model_case(orig, new, L, lead):
    """(x, g, gx) float64 of a case, computed once: the planted audio, the planted output gradient, and the model's
    gradient of <model(x), g> by torch autograd."""
    x = audio(lead + (L,), 1000 + 7 * L + len(lead) + lead[0]).requires_grad_()
    g = audio(lead + (out_len(L, orig, new),), 2000 + 7 * L + len(lead) + lead[0])
    (model(x, orig, new) * g).sum().backward()
    return x.detach(), g, x.grad.detach()


def adjoint(g, L, orig, new, lead=None):
    """The adjoint formula in float64 numpy: g (..., out_len) -> gx (..., L).  lead defaults to width."""
    h, width = bank(orig, new)
    lead = width if lead is None else lead
    h = h.double().numpy()
    taps = h.shape[1]
    g = np.asarray(g)
    shape, olen = g.shape[:-1], g.shape[-1]
    nblk = -(-olen // new)
    gp = np.zeros((int(np.prod(shape)), nblk * new))
    gp[:, :olen] = g.reshape(-1, olen)
    w = gp.reshape(-1, nblk, new) @ h                       # w[row, i, k] = sum_j h[j][k] g[i new + j]
    ext = np.zeros((gp.shape[0], lead + max(L, nblk * orig) + taps))          # ext[lead + n] = gx[n]
    at = orig * np.arange(nblk)
    for k in range(taps):                                   # n = i orig - lead + k: distinct places for one k
        ext[:, at + k] += w[:, :, k]
    return ext[:, lead:lead + L].reshape(shape + (L,))


def stream_chunk(x, state, orig, new):
    """x (..., C) and state (..., Ha) float64 -> (y (..., C new / orig), new state (..., Ha))."""
    h, width = bank(orig, new)
    Ha = stream_sizes(orig, new)[1]
    assert state.shape[-1] == Ha and x.shape[-1] % orig == 0
    lead, c = tuple(x.shape[:-1]), x.shape[-1] // orig
    v = torch.cat([state, x], -1)
    y = torch.nn.functional.conv1d(v.reshape(-1, 1, v.shape[-1]), h.double().unsqueeze(1), stride=orig)      # valid
    assert y.shape[-1] >= c, "Ha is too short for the chunk's blocks"
    y = y[..., :c].transpose(1, 2).reshape(y.shape[0], -1)
    return y.reshape(lead + (c * new,)), v[..., -Ha:]


def stream(x, orig, new, blocks):
    """The concatenated outputs of stream_chunk over x (..., L) cut into `blocks`, from a zero state."""
    state = x.new_zeros(tuple(x.shape[:-1]) + (stream_sizes(orig, new)[1],))
    outs, pos = [], 0
    for b in blocks:
        y, state = stream_chunk(x[..., pos:pos + b * orig], state, orig, new)
        outs.append(y)
        pos += b * orig
    assert pos == x.shape[-1]
    return torch.cat(outs, -1)


def delayed(x, orig, new):
    """The offline model of x delayed by D blocks, cut to x's blocks."""
    D = stream_sizes(orig, new)[0]
    y = model(torch.cat([x.new_zeros(tuple(x.shape[:-1]) + (D * orig,)), x], -1), orig, new)
    return y[..., :x.shape[-1] // orig * new]


def rel_max(a, b):
    a, b = np.asarray(a), np.asarray(b)
    denom = float(np.abs(b).max()) if b.size else 0.0
    return float(np.abs(a - b).max()) / (denom if denom > 0 else 1.0) if b.size else 0.0

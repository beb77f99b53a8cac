"""Float64 restatement of the streaming PQMF (transforms.RealtimePQMF, csrc/pqmf.hip's *_stream entries), written from
its definition on top of pqmf_cases.py and shared by test_pqmf_stream_cpu.py and test_pqmf_stream_gpu.py, and the case
table of both.

M = n_band, N = taps (odd), P = (N - 1) / 2, D = ceil(P / M).  The streaming bank is the offline one delayed by D blocks:
    analysis    block t of the stream is sum_n h_k[n] x[(t - D) M + n - P], x zero before the stream's start; it reads
                samples (t - D) M - P ... (t - D) M + P, so a call needs the Ha = D M + P samples before its chunk and
                nothing after it: a VALID conv1d of [state | chunk] with stride M, cut to the chunk's blocks
    synthesis   sample m of the stream is M sum_k sum_t h_k[m - D M + P - tM] y[k, t]; it reads blocks
                ceil((m - D M - P) / M) ... floor((m - D M + P) / M), so a call needs the Hs = D + floor(P / M) blocks
                before its chunk and nothing after it: the synthesis of [state | chunk] alone, read (Hs - D) M samples in
The new state is the tail of [state | chunk].  Everything is float64 torch, so torch autograd differentiates it with the
state a constant."""
import torch

import pqmf_cases as C

# (n_band, taps): the smallest filter; a non-power-of-two M with a partial last fold group; an odd M with two fold groups;
# a band count with a kernel of its own; the defaults
CASES = ((2, 5), (3, 51), (5, 11), (4, 65), (16, 513))
# further (n_band, taps) at which the sufficiency of Ha and Hs is checked in float64 only
CPU_ONLY = ((16, 257),)
# (n_band, taps, blocks of the differentiated chunk).  At (3, 51) a one-block chunk is not read by its own output block
# (that block ends at sample D M - P = 2 before the chunk): the gradient of forward is exactly zero there, in both
# implementations, and the case checks that the kernel writes those zeros
GRAD = ((3, 51, "1"), (3, 51, "tile+1"), (16, 513, "tile+1"))


def sizes(n_band, taps):
    """(P, D, Ha, Hs)."""
    P = (taps - 1) // 2
    D = -(-P // n_band)
    return P, D, D * n_band + P, D + P // n_band


def chunk_blocks(Hs, tile):
    """The chunk list of a stream, in blocks: single blocks, a chunk shorter than the state, both sides of a tile edge."""
    return [1, 1, 2, max(Hs - 1, 1), tile - 1, tile, tile + 1]


def analysis_chunk(x, state, hk):
    """x (..., C) and state (..., Ha) float64 -> (y (..., M, C / M), new state (..., Ha))."""
    M, N = hk.shape
    _, _, Ha, _ = sizes(M, N)
    assert state.shape[-1] == Ha and x.shape[-1] % M == 0
    s = torch.cat([state, x], -1)
    lead, c = x.shape[:-1], x.shape[-1] // M
    w = torch.from_numpy(hk).unsqueeze(1)
    y = torch.nn.functional.conv1d(s.reshape(-1, 1, s.shape[-1]), w, stride=M)       # valid: no sample but [state | chunk]
    assert y.shape[-1] >= c, "Ha is too short for the chunk's blocks"
    return y[..., :c].reshape(tuple(lead) + (M, c)), s[..., -Ha:]


def synthesis_chunk(y, state, hk):
    """y (..., M, c) and state (..., M, Hs) float64 -> (x (..., c M), new state (..., M, Hs))."""
    M, N = hk.shape
    _, D, _, Hs = sizes(M, N)
    assert state.shape[-1] == Hs and y.shape[-2] == M
    s = torch.cat([state, y], -1)
    c = y.shape[-1]
    full = C.synthesis(s, hk)                           # of the Hs + c blocks alone, zeros before and after them
    lo = (Hs - D) * M
    return full[..., lo:lo + c * M], s[..., -Hs:]


def stream_analysis(x, hk, blocks):
    """The concatenated outputs of analysis_chunk over x (..., L) cut into `blocks`, from a zero state."""
    M, N = hk.shape
    state = x.new_zeros(tuple(x.shape[:-1]) + (sizes(M, N)[2],))
    outs, pos = [], 0
    for b in blocks:
        y, state = analysis_chunk(x[..., pos:pos + b * M], state, hk)
        outs.append(y)
        pos += b * M
    assert pos == x.shape[-1]
    return torch.cat(outs, -1)


def stream_synthesis(y, hk, blocks):
    M, N = hk.shape
    state = y.new_zeros(tuple(y.shape[:-1]) + (sizes(M, N)[3],))
    outs, pos = [], 0
    for b in blocks:
        x, state = synthesis_chunk(y[..., pos:pos + b], state, hk)
        outs.append(x)
        pos += b
    assert pos == y.shape[-1]
    return torch.cat(outs, -1)


def delayed_analysis(x, hk):
    """The offline analysis of x delayed by D blocks, cut to x's blocks."""
    M, N = hk.shape
    D = sizes(M, N)[1]
    return C.analysis(torch.cat([x.new_zeros(tuple(x.shape[:-1]) + (D * M,)), x], -1), hk)[..., :x.shape[-1] // M]


def delayed_synthesis(y, hk):
    M, N = hk.shape
    D = sizes(M, N)[1]
    return C.synthesis(torch.cat([y.new_zeros(tuple(y.shape[:-1]) + (D,)), y], -1), hk)[..., :y.shape[-1] * M]

"""Float64 restatement of the bankless sample-rate converter (ops.resample_direct, csrc/sinc_interp.hip) and the case
table shared by test_sinc_interp_cpu.py, test_sinc_interp_gpu.py and test_pitch_shift_gpu.py.

With the rates reduced by their gcd to (orig, new), rho = rolloff / max(orig, new) and Qi the largest integer below
lpw / rho, the MODEL is a gather over the input samples, with no bank anywhere:
    y[o] = sum over 0 <= n < L with |n new - o orig| <= Qi of table[|n new - o orig|] x[n]
on the float32-rounded half-table (ops.sinc_table) taken as float64.  Its ADJOINT is the same gather with the two signals
and the two rates exchanged.  At the ratios where a bank can be built the model agrees with resample_cases.model to 1e-12
(test_sinc_interp_cpu.py), which is what makes it the oracle at (18521, 14700), where none can."""
import functools
import math

import numpy as np
import torch

import resample_cases as RC
from acids_transforms_amd import ops

RATIOS = RC.RATIOS
BIG = (18521, 14700)                # 55563 -> 44100, a third of an octave: the bank would hold 1 GB, the table 450 KB
MID = (1852, 1470)                  # the largest rates whose bank the CPU tests still build; they reduce to (926, 735)
LEADS = RC.LEADS
BIG_LENGTHS = (20000, 40001)

out_len = RC.out_len
rel_max = RC.rel_max
audio = RC.audio


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


@functools.lru_cache(maxsize=None)
def table(orig, new):
    """(table float32 torch (Qi + 1,), Qi)."""
    return ops.sinc_table(orig, new)


def gather(x, a, b, n_out, tab, Qi):
    """out[..., o] = sum_n tab[|n b - o a|] x[..., n] over 0 <= n < x.shape[-1], |n b - o a| <= Qi; float64 numpy."""
    x = np.asarray(x, dtype=np.float64)
    tab = np.asarray(tab, dtype=np.float64)
    n_in = x.shape[-1]
    o = np.arange(n_out, dtype=np.int64)[:, None]
    first = -((Qi - o * a) // b)                                   # ceil((o a - Qi) / b)
    n = first + np.arange(2 * Qi // b + 2, dtype=np.int64)[None, :]
    q = np.abs(n * b - o * a)
    live = (q <= Qi) & (n >= 0) & (n < n_in)
    coeff = np.where(live, tab[np.minimum(q, Qi)], 0.0)
    if n_in == 0:
        return np.zeros(x.shape[:-1] + (n_out,))
    return (x[..., np.clip(n, 0, n_in - 1)] * coeff).sum(-1)


def model(x, orig, new):
    """x (..., L) float64 -> (..., ceil(new L / orig)) float64 numpy."""
    tab, Qi = table(orig, new)
    return gather(x, orig, new, out_len(np.asarray(x).shape[-1], orig, new), tab.numpy(), Qi)


def adjoint(g, L, orig, new):
    """g (..., ceil(new L / orig)) float64 -> gx (..., L): the model with the roles exchanged."""
    tab, Qi = table(orig, new)
    assert np.asarray(g).shape[-1] == out_len(L, orig, new)
    return gather(g, new, orig, L, tab.numpy(), Qi)


def plan(a, b, Qi):
    """(tile_outputs, table_in_lds) of at_sinc_interp."""
    return ops.sinc_interp_plan(a, b, Qi)


def lengths(orig, new):
    """The clip lengths of a ratio: 1, 2, around one block, and both sides of one and of two tiles of the forward (a tile
    is `tile_outputs` outputs) and of the backward (whose outputs are the clip's own samples)."""
    Qi = table(orig, new)[1]
    tf, tb = plan(orig, new, Qi)[0], plan(new, orig, Qi)[0]
    want = {1, 2, orig - 1, orig, orig + 1}
    for t in (tf, 2 * tf):
        L0 = t * orig // new                                       # out_len(L0) <= t < out_len(L0 + 2)
        want |= {L0 - 1, L0, L0 + 1, L0 + 2}
    for t in (tb, 2 * tb):
        want |= {t - 1, t, t + 1}
    return tuple(sorted(L for L in want if L > 0))


@functools.lru_cache(maxsize=None)
def case(orig, new, L, lead):
    """(x, g, y, gx) float64 of a case, computed once: planted audio and output gradient, the model and its adjoint."""
    x = audio(lead + (L,), 3000 + 7 * L + len(lead) + lead[0])
    g = audio(lead + (out_len(L, orig, new),), 4000 + 7 * L + len(lead) + lead[0])
    return x, g, torch.from_numpy(model(x.numpy(), orig, new)), torch.from_numpy(adjoint(g.numpy(), L, orig, new))


def pitch_rates(sr, n_steps, bins_per_octave=12):
    """(rate, orig_freq) as torchaudio.functional.pitch_shift derives them, in host float64."""
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    return rate, int(sr / rate)

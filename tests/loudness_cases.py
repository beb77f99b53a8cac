"""Float64 restatement of gated loudness (ITU-R BS.1770-4 / EBU R128: ops.loudness, ops.loudness_blocks, ops.sos_hop_power,
transforms.Loudness; csrc/sos_filter.hip and csrc/loudness.hip) and the case table shared by test_loudness_cpu.py and
test_loudness_gpu.py.

The ORACLE is scipy.signal.sosfilt in float64 on the K-weighting sections, then numpy:
    H = round(sr / 10),  nh = L // H,  nb = nh - hb + 1,
    s[c][h] = sum over hop h of y_c[n]^2,   p_j = sum_c G_c (s[c][j] + ... + s[c][j + hb - 1]) / (hb H),
    l_j = -0.691 + 10 log10 p_j,
    J1 = {j: p_j > 10^((-70 + 0.691) / 10)},  Pabs = mean_J1 p,  J2 = {j in J1: p_j > Pabs / 10},  P = mean_J2 p,
    loudness = -0.691 + 10 log10 P   (-inf when J1 is empty).
`p > t` is evaluated as not (p <= t): a NaN block passes, so a clip with a NaN reads NaN.  The ANALYTIC GRADIENT treats the
gates as constants: with m[h] the number of J2 blocks that cover hop h and N2 = |J2|,
    d loudness / d y_c[n] = (10 / ln 10) / (P N2) G_c (2 / (4 H)) m[n // H] y_c[n]     (0 for n >= nh H),
and the gradient with respect to x is the reverse K-weighting filter of that (flip -> sosfilt -> flip, the adjoint of
sosfilt from zero state).  For block loudness: d l_j / d y_c[n] = (10 / ln 10) / p_j G_c (2 / (hb H)) y_c[n] on the block's
samples, nothing where p_j == 0.

Planted clips, all at SR = 8000 (H = 800) so that a GPU test takes seconds.  EVERY case used for parity keeps every block
at least MARGIN_DB = 1 dB away from both gates in the oracle -- no rounding of a kernel can flip a gate -- and
`assert_margins` checks that for the whole table (test_loudness_cpu.py runs it; no case is left out)."""
import functools
import math

import numpy as np
from scipy.signal import sosfilt

from acids_transforms_amd.utils import filter_design as fd

SR = 8000
H = 800
TILE = 4096                        # sos_filter.hip's tile (test_loudness_cpu.py checks it against the plan)
ABS_THRESHOLD = 10.0 ** ((-70.0 + 0.691) / 10.0)
REL_RATIO = 0.1
DEFAULT_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)
MARGIN_DB = 1.0
TOL = 1e-5                         # the project's standing normwise bound, max|a - b| / max|b|
TOL_LU = 1e-4                      # 1e-5 on y: 10 log10(1 + 2e-5) = 8.7e-5
LEADS = ((), (3,), (2, 3), (70,))
HOPS = (16, 17, 255, 800, 4096, 4097, 4410)
PARITY_LENGTHS = (TILE - 1, TILE, TILE + 1, 2 * TILE + 5)             # the rows every hop of HOPS runs at: around the tile cuts


def hop_of(sr):
    return int(round(float(sr) / 10.0))


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    denom = float(np.abs(b).max()) if b.size else 0.0
    return float(np.abs(a - b).max()) / (denom if denom > 0 else 1.0) if a.size else 0.0


def weights_for(C, weights=None):
    return np.asarray(DEFAULT_WEIGHTS[:C] if weights is None else weights, dtype=np.float64)


def above(p, t):
    return ~(p <= t)


def hop_power(sos, x, hop):
    """sum over each whole hop of sosfilt(sos, x)^2: x (..., L) -> (..., L // hop), float64."""
    x = np.asarray(x, dtype=np.float64)
    y = sosfilt(np.array(sos, dtype=np.float64), x, axis=-1)           # a copy: scipy wants a writable buffer
    nh = x.shape[-1] // hop
    return (y[..., :nh * hop].reshape(x.shape[:-1] + (nh, hop)) ** 2).sum(-1)


def kweighted(x, sr):
    return sosfilt(fd.k_weighting(sr), np.asarray(x, dtype=np.float64), axis=-1)


def block_power(x, sr, hb=4, weights=None):
    """x (..., C, L) -> p (..., nb) float64."""
    x = np.asarray(x, dtype=np.float64)
    hop, G = hop_of(sr), weights_for(x.shape[-2], weights)
    s = hop_power(fd.k_weighting(sr), x, hop)                           # (..., C, nh)
    nb = s.shape[-1] - hb + 1
    assert nb >= 1
    blocks = sum(s[..., k:k + nb] for k in range(hb))                   # (..., C, nb)
    return np.einsum("c,...cj->...j", G, blocks) / (hb * hop)


def lufs_of(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def block_loudness(x, sr, hb=4, weights=None):
    return lufs_of(block_power(x, sr, hb, weights))


def gating(p):
    """One clip's block powers p (nb,) -> dict(J1, J2 boolean masks, Pabs, P, N2, lufs, margin_db).  margin_db is the
    distance in dB of the nearest block to either gate (inf for a clip with no power at all)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        J1 = above(p, ABS_THRESHOLD)
        Pabs = float(p[J1].mean()) if J1.any() else 0.0
        J2 = J1 & above(p, REL_RATIO * Pabs)
        P = float(p[J2].mean()) if J2.any() else 0.0
        lufs = float(lufs_of(np.float64(P))) if J2.any() else -math.inf
        dist = np.abs(10.0 * np.log10(p / ABS_THRESHOLD))
        if J1.any():
            dist = np.minimum(dist, np.where(J1, np.abs(10.0 * np.log10(p / (REL_RATIO * Pabs))), np.inf))
        finite = dist[np.isfinite(dist)]
    return dict(J1=J1, J2=J2, Pabs=Pabs, P=P, N2=int(J2.sum()), lufs=lufs,
                margin_db=float(finite.min()) if finite.size else math.inf)


def loudness(x, sr, weights=None):
    """x (..., C, L) -> integrated loudness (...,) float64."""
    p = block_power(x, sr, 4, weights)
    flat = p.reshape(-1, p.shape[-1])
    return np.array([gating(row)["lufs"] for row in flat]).reshape(p.shape[:-1])


def _reverse_k(u, sr):
    return sosfilt(fd.k_weighting(sr), u[..., ::-1], axis=-1)[..., ::-1]


def _spread(per_block, hb, nh):
    """(..., nb) block terms -> (..., nh): for every hop the sum over the blocks that cover it."""
    out = np.zeros(per_block.shape[:-1] + (nh,))
    nb = per_block.shape[-1]
    for k in range(hb):
        out[..., k:k + nb] += per_block
    return out


def loudness_gradient(x, sr, weights=None, g=None):
    """d (sum over clips of g loudness) / dx, the gates constant: x (..., C, L) -> (..., C, L) float64.  A clip that reads
    -inf has gradient 0."""
    x = np.asarray(x, dtype=np.float64)
    hop, G = hop_of(sr), weights_for(x.shape[-2], weights)
    lead, C, L = x.shape[:-2], x.shape[-2], x.shape[-1]
    nh = L // hop
    y = kweighted(x, sr)
    p = block_power(x, sr, 4, weights).reshape(-1, nh - 3)
    g = np.ones(len(p)) if g is None else np.asarray(g, dtype=np.float64).reshape(-1)
    u = np.zeros((len(p), C, L))
    yf = y.reshape(-1, C, L)
    for i, row in enumerate(p):
        gate = gating(row)
        if gate["N2"] == 0:
            continue
        m = _spread(gate["J2"].astype(np.float64), 4, nh)
        per_hop = g[i] * (10.0 / math.log(10.0)) / (gate["P"] * gate["N2"]) * (2.0 / (4 * hop)) * m
        u[i, :, :nh * hop] = G[:, None] * np.repeat(per_hop, hop)[None, :] * yf[i, :, :nh * hop]
    return _reverse_k(u, sr).reshape(x.shape)


def blocks_gradient(x, sr, hb, g, weights=None):
    """d (sum of g * block loudness) / dx: x (..., C, L), g (..., nb) -> (..., C, L) float64; silent blocks pass nothing."""
    x = np.asarray(x, dtype=np.float64)
    hop, G = hop_of(sr), weights_for(x.shape[-2], weights)
    L = x.shape[-1]
    nh = L // hop
    y = kweighted(x, sr)
    p = block_power(x, sr, hb, weights)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(p == 0.0, 0.0, np.asarray(g, dtype=np.float64) * (10.0 / math.log(10.0)) / p)
    per_hop = _spread(term, hb, nh) * (2.0 / (hb * hop))                # (..., nh)
    u = np.zeros_like(x)
    u[..., :nh * hop] = G[:, None] * np.repeat(per_hop, hop, axis=-1)[..., None, :] * y[..., :nh * hop]
    return _reverse_k(u, sr)


# ---- planted clips -----------------------------------------------------------------------------------------------------

def _noise(seed, shape, sigma=0.1):
    return (sigma * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _gated():
    """Two channels of 0.1-sigma noise, 3 s + 123 samples; the second second 30 dB down, the third at 1e-5: 27 blocks, 20
    pass the absolute gate, 10 the relative one."""
    x = _noise(1, (2, 3 * SR + 123))
    x[:, SR:2 * SR] *= np.float32(10.0 ** (-30.0 / 20.0))
    x[:, 2 * SR:] *= np.float32(1e-5)
    return x


def _tech3341_3(sr, seconds=(1, 4, 1), levels=(-36.0, -23.0, -36.0)):
    """EBU Tech 3341 case 3 in its shape: a stereo 1 kHz sine at -36, -23 and -36 dBFS (full length: 10, 60 and 10 s)."""
    t = np.arange(int(sum(seconds) * sr)) / sr
    amp = np.concatenate([np.full(int(s * sr), 10.0 ** (l / 20.0)) for s, l in zip(seconds, levels)])
    x = amp * np.sin(2 * np.pi * 1000.0 * t)
    return np.stack([x, x]).astype(np.float32)


def _five():
    x = _noise(5, (5, 6 * H + 11))
    x *= np.array([1.0, 0.5, 0.25, 0.8, 0.3], dtype=np.float32)[:, None]
    return x


def _nan_clip():
    x = _gated().copy()
    x[1, 10000] = np.nan
    return x


def _batch():
    """70 stereo clips over two tiles, each at its own level, every other one with a second half 20 dB down."""
    x = _noise(70, (70, 2, 8 * H - 1))
    x *= (10.0 ** (-np.arange(70) / 40.0)).astype(np.float32)[:, None, None]
    x[::2, :, 4 * H:] *= np.float32(0.1)
    return x


LENGTHS = (4 * H, 4 * H + 1, 8 * H - 1, TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1)


@functools.lru_cache(maxsize=None)
def clips():
    """name -> x (..., C, L) float32, read-only.  `PARITY` names the ones compared with the oracle to TOL_LU."""
    out = {"gated": _gated(), "tech3341-3 short": _tech3341_3(SR), "silent": np.zeros((2, 4 * H), dtype=np.float32),
           "below gate": _noise(3, (1, 5 * H + 3), 1e-5), "five": _five(), "nan": _nan_clip(), "batch": _batch()}
    for L in LENGTHS:
        out["L%d" % L] = _noise(1000 + L, (2 if L % 2 else 1, L))
    for v in out.values():
        v.setflags(write=False)
    return out


PARITY = ("gated", "tech3341-3 short", "silent", "below gate", "five", "batch") + tuple("L%d" % L for L in LENGTHS)


@functools.lru_cache(maxsize=None)
def reference(name, hb=4):
    """The oracle on a planted clip, computed once: dict(p (..., nb), blocks (..., nb) LUFS, lufs (...,), margin_db)."""
    x = clips()[name]
    with np.errstate(invalid="ignore"):
        p = block_power(x, SR, hb)
    flat = p.reshape(-1, p.shape[-1])
    gates = [gating(row) for row in flat]
    out = dict(p=p, blocks=lufs_of(p), lufs=np.array([g["lufs"] for g in gates]).reshape(p.shape[:-1]),
               margin_db=min(g["margin_db"] for g in gates), N1=[int(g["J1"].sum()) for g in gates],
               N2=[g["N2"] for g in gates])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def assert_margins():
    """Every parity case keeps every block at least MARGIN_DB from both gates; returns the margins."""
    margins = {name: reference(name)["margin_db"] for name in PARITY}
    bad = {k: v for k, v in margins.items() if not v >= MARGIN_DB}
    assert not bad, bad
    return margins


def take(a, lead):
    """The first clips of a (70, ...) array that make up the leading shape `lead`."""
    rows = int(np.prod(lead)) if lead else 1
    return np.ascontiguousarray(a[:rows]).reshape(tuple(lead) + a.shape[1:])

"""Float64 restatement of recursive filtering by second-order sections (ops.sos_filter, csrc/sos_filter.hip) and the case
table shared by test_sos_filter_cpu.py and test_sos_filter_gpu.py.

The ORACLE is the sequential recurrence of scipy.signal.sosfilt in numpy float64, in scipy's order of operations,
    y = b0 v + z1,   z1' = (b1 v - a1 y) + z2,   z2' = b2 v - a2 y,
vectorised over the rows and -- as a skewed walk, section k working on sample t - k while section 0 works on sample t --
over the sections, so that a 16-section cascade costs as many Python steps as one section.  The arithmetic of a
(row, section, sample) is exactly the sequential one.  Its ADJOINT (zero state) is the same filter run backwards in time.

Filters: the 20 Hz high-pass and the resonator are the cases on which an fp32 state or fp32 coefficients miss the 1e-5
bound by 10 x or more.  Lengths come from ops.sos_filter_plan, so they follow the kernel's tile.  One batch of 70 rows per
(filter, length) serves every leading shape: (L,) is its row 0, (3, L) rows 0..2, (2, 3, L) rows 0..5."""
import functools
import math

import numpy as np

from acids_transforms_amd import ops
from acids_transforms_amd.utils import filter_design as fd

SR = 44100
ROWS = 70
LEADS = ((), (3,), (2, 3), (ROWS,))
TOL = 1e-5                     # the project's standing normwise bound, max|a - b| / max|b|
# The carried state is held to the same bound as the audio.  It is double, but on the 20 Hz high-pass it is NOT double-accurate:
# the scan applies explicit powers of A = [[-a1, 1], [-a2, 0]], whose entries grow like n r^n (up to 180 at pole radius
# r = 0.998) while what they do to a decaying state is of order r^n, so the rounding of a squared power, eps |A^n|^2, is
# 1e-12 absolute against an action of 1e-2.  Measured: 7.6e-8 normwise on that filter (a numpy restatement of the scan gives
# 1.4e-9 on three rows), 1.1e-8 on the 4-section cascade, < 2e-10 elsewhere, where the sequential float64 recurrence is
# itself 6e-12 off an 80-bit run.  The float32 output does not see it (5e-8 is its own rounding).
STATE_TOL = TOL


def _resonator(r=0.9995, w=0.05):
    return np.array([[1.0 - r, 0.0, 0.0, 1.0, -2.0 * r * math.cos(w), r * r]])


def _cascade16():
    """Sixteen peaks and dips between 100 Hz and 15 kHz: unit gain away from the peaks, so the signal stays of order 1."""
    return np.concatenate([fd.equalizer(SR, 100.0 * 1.4 ** i, 3.0 if i % 2 else -3.0, 2.0) for i in range(16)])


FILTERS = {
    "highpass20": fd.highpass(SR, 20.0, 0.707),
    "peak1k": fd.equalizer(SR, 1000.0, 6.0, 4.0),
    "resonator": _resonator(),
    "cascade4": np.concatenate([fd.highpass(SR, 20.0, 0.707), fd.equalizer(SR, 1000.0, 6.0, 4.0), _resonator(),
                                fd.highpass(SR, 20.0, 0.707)]),
    "kweighting": fd.k_weighting(48000),
    "cascade16": _cascade16(),
}
NAMES = tuple(FILTERS)


def plan(n_sections, rows=ROWS, L=1):
    return ops.sos_filter_plan(rows, L, n_sections)


def lengths(n_sections):
    tile, per_lane, _ = plan(n_sections)
    return (1, 2, 3, per_lane - 1, per_lane, per_lane + 1, tile - 1, tile, tile + 1, 2 * tile + 5)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    denom = float(np.abs(b).max()) if b.size else 0.0
    return float(np.abs(a - b).max()) / (denom if denom > 0 else 1.0) if a.size else 0.0


def sosfilt(sos, x, zi=None):
    """(y, zf): x (..., L) and zi (..., n, 2) in float64 -> y (..., L), zf (..., n, 2).  a0 must be 1."""
    sos = np.asarray(sos, dtype=np.float64)
    assert sos.ndim == 2 and sos.shape[1] == 6 and np.all(sos[:, 3] == 1.0)
    x = np.asarray(x, dtype=np.float64)
    lead, L, n = x.shape[:-1], x.shape[-1], sos.shape[0]
    xr = x.reshape(-1, L)
    R = xr.shape[0]
    b0, b1, b2, a1, a2 = sos[:, 0], sos[:, 1], sos[:, 2], sos[:, 4], sos[:, 5]
    z = np.zeros((R, n, 2)) if zi is None else np.array(zi, dtype=np.float64).reshape(R, n, 2)
    z1, z2 = z[:, :, 0].copy(), z[:, :, 1].copy()
    y = np.empty((R, L))
    out = np.zeros((R, n))                       # what each section put out at the step before
    k = np.arange(n)
    for t in range(L + n - 1):                   # section k works on sample t - k
        u = np.empty((R, n))
        u[:, 0] = xr[:, t] if t < L else 0.0
        u[:, 1:] = out[:, :-1]
        live = (t - k >= 0) & (t - k < L)
        w = b0 * u + z1
        n1 = (b1 * u - a1 * w) + z2
        n2 = b2 * u - a2 * w
        z1 = np.where(live, n1, z1)
        z2 = np.where(live, n2, z2)
        out = w
        if t >= n - 1:
            y[:, t - (n - 1)] = w[:, n - 1]
    return y.reshape(lead + (L,)), np.stack([z1, z2], -1).reshape(lead + (n, 2))


def sosfilt_reverse(sos, x):
    """The anti-causal filter with zero state: flip -> sosfilt -> flip.  The adjoint of sosfilt(., zi=None)."""
    return sosfilt(sos, np.asarray(x, dtype=np.float64)[..., ::-1])[0][..., ::-1]


def steady_state(sos):
    """scipy.signal.sosfilt_zi restated: the (n, 2) state of the cascade in the steady state of a unit step."""
    sos = np.asarray(sos, dtype=np.float64)
    zi, scale = np.zeros((sos.shape[0], 2)), 1.0
    for k, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        A = np.array([[-a1, 1.0], [-a2, 0.0]])
        zi[k] = scale * np.linalg.solve(np.eye(2) - A, np.array([b1 - a1 * b0, b2 - a2 * b0]))
        scale *= (b0 + b1 + b2) / (1.0 + a1 + a2)
    return zi


def zero_phase(sos, x, primed=False):
    """Forward, then backward.  primed=False: both passes from zero state (what SOSFilter(zero_phase=True) computes, and its
    own adjoint).  primed=True: both passes start in the steady state of a step as high as their first sample, which is
    scipy.signal.sosfiltfilt(padtype=None)."""
    x = np.asarray(x, dtype=np.float64)
    if not primed:
        return sosfilt_reverse(sos, sosfilt(sos, x)[0])
    zi = steady_state(sos)
    y = sosfilt(sos, x, zi * x[..., 0][..., None, None])[0][..., ::-1]
    return sosfilt(sos, y, zi * y[..., 0][..., None, None])[0][..., ::-1]


def _seed(name, L):
    return NAMES.index(name) * 100003 + L


@functools.lru_cache(maxsize=None)
def case(name, L):
    """One batch per (filter, length), computed once: dict of x (ROWS, L) float32, zi (ROWS, n, 2) float64 and the oracle's
    fwd / rev / zp (zero-state forward, reverse and zero-phase), yzi / zf (forward from zi and the state after it)."""
    sos = FILTERS[name]
    n = sos.shape[0]
    rng = np.random.default_rng(_seed(name, L))
    x = rng.standard_normal((ROWS, L)).astype(np.float32)
    zi = 0.5 * rng.standard_normal((ROWS, n, 2))
    x64 = x.astype(np.float64)
    stacked = np.concatenate([x64, x64[:, ::-1], x64])
    y, zf = sosfilt(sos, stacked, np.concatenate([np.zeros_like(zi), np.zeros_like(zi), zi]))
    fwd = y[:ROWS]
    # sos: a copy, so that freezing the case leaves FILTERS writable (scipy.signal.sosfilt refuses a read-only table, and
    # test_sos_filter_cpu.py hands it FILTERS' own arrays after the GPU tests have been through here)
    out = dict(sos=sos.copy(), x=x, zi=zi, fwd=fwd, rev=y[ROWS:2 * ROWS, ::-1].copy(), yzi=y[2 * ROWS:], zf=zf[2 * ROWS:],
               zp=sosfilt_reverse(sos, fwd))
    for v in out.values():
        v.setflags(write=False)
    return out


def take(a, lead):
    """The rows of a (ROWS, ...) array that make up the leading shape `lead`."""
    rows = int(np.prod(lead)) if lead else 1
    return np.ascontiguousarray(a[:rows]).reshape(tuple(lead) + a.shape[1:])

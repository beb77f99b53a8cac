"""Float64 restatement of the true-peak measure (ops.true_peak, transforms.TruePeak, RealtimeTruePeak; csrc/true_peak.hip),
shared by test_true_peak_cpu.py and test_true_peak_gpu.py.

A filter is a table h (P, K): P phases, K taps per phase.  For a row x of L samples, with x[n] = 0 for n < 0 (or the K - 1
samples of a carried state),
    y[P n + p] = sum over k of h[p][k] x[n - k],   peak = max |y|,   index = the smallest m that attains it.
The ORACLE evaluates that in float64 on the table ROUNDED TO FLOAT32 (the module's buffer), one multiply-add per tap over
whole rows.  Every input that is compared by index is PLANTED: low noise plus one dominant sample, and the CPU tests check
that its largest |y| stands at least MARGIN = 1e-3 relative above the runner-up, so float32 rounding (1e-5 normwise) cannot
move the index."""
import functools

import numpy as np

from acids_transforms_amd.utils import filter_design as fd

TILE, PER_LANE = 2048, 8                       # at_true_peak_plan's answer, held by test_true_peak_cpu.py
TOL, TOL_DB, MARGIN = 1e-5, 1e-4, 1e-3
BS1770_INTEGERS = ((14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68),
                   (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155))


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (P, K) float32 table, read-only."""
    out = {"bs1770": fd.true_peak_filter(4, 12, "bs1770"), "kaiser 2x16": fd.true_peak_filter(2, 16, "kaiser"),
           "kaiser 8x7": fd.true_peak_filter(8, 7, "kaiser"), "identity": np.ones((1, 1)),
           "random 3x5": np.random.default_rng(35).standard_normal((3, 5))}
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


TABLES = ("bs1770", "kaiser 2x16", "kaiser 8x7", "identity", "random 3x5")


# ---- the oracle --------------------------------------------------------------------------------------------------------

def oversampled(x, h, state=None):
    """x (..., L), h (P, K), state (..., K - 1) or None -> y (..., P L) float64."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    P, K = h.shape
    lead, L = x.shape[:-1], x.shape[-1]
    before = np.zeros(lead + (K - 1,)) if state is None else np.asarray(state, dtype=np.float64)
    xp = np.concatenate([before, x], axis=-1)
    y = np.zeros(lead + (L, P))
    for p in range(P):
        for k in range(K):
            y[..., p] += h[p, k] * xp[..., K - 1 - k:K - 1 - k + L]
    return y.reshape(lead + (L * P,))


def measure(x, h, state=None):
    """dict(peak, index, sign, margin, y): the linear peak, the smallest index that attains it, the sign of y there and the
    relative distance of the runner-up, each (...,)."""
    y = oversampled(x, h, state)
    a = np.abs(y)
    index = a.argmax(-1)
    peak = np.take_along_axis(a, index[..., None], -1)[..., 0]
    sign = np.sign(np.take_along_axis(y, index[..., None], -1)[..., 0])
    if a.shape[-1] > 1:
        second = np.partition(a, -2, axis=-1)[..., -2]
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(peak > 0, (peak - second) / peak, 0.0)
    else:
        margin = np.ones_like(peak)
    return dict(peak=peak, index=index, sign=sign, margin=margin, y=y)


def dbtp(peak):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.asarray(peak, dtype=np.float64))


def next_state(x, K, state=None):
    """The last K - 1 samples of [state | x]."""
    x = np.asarray(x)
    before = np.zeros(x.shape[:-1] + (K - 1,), x.dtype) if state is None else state
    return np.concatenate([before, x], axis=-1)[..., x.shape[-1]:]


# ---- planted signals ---------------------------------------------------------------------------------------------------

def main_delay(h):
    """The samples between the planted pair (1, 0.5) and the sample whose outputs hold the maximum of |y|.  (A lone
    sample will not do: a symmetric table answers it with two equal maxima, one in each mirrored phase.)"""
    K = h.shape[1]
    pair = np.zeros(K + 1)
    pair[:2] = 1.0, 0.5
    return int(measure(pair, h)["index"]) // h.shape[0]


def planted(h, rows, L, at, seed, negative=False):
    """(rows, L) float32: 0.01-sigma noise and per row the pair (1, 0.5) times +-1, placed so that the maximum of |y| falls
    among the outputs of sample `at` (an int, or one per row); rows alternate in sign, or are all negative."""
    rng = np.random.default_rng(seed)
    x = (0.01 * rng.standard_normal((rows, L))).astype(np.float32)
    at = np.broadcast_to(np.asarray(at), (rows,))
    where = np.clip(at - main_delay(h), 0, L - 1)
    sign = (-np.ones(rows) if negative else np.where(np.arange(rows) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    x[np.arange(rows), where] = sign
    follows = where + 1 < L
    x[np.arange(rows)[follows], where[follows] + 1] = np.float32(0.5) * sign[follows]
    return x


def lengths(K):
    return sorted({n for n in (1, K - 2, K - 1, K, TILE - 1, TILE, TILE + 1, 2 * TILE + K - 2) if n >= 1})


LONG = 2 * TILE + 37
# name -> (table, rows, L, the sample whose outputs hold the maximum, all negative)
SPOTS = {"early": ("bs1770", 3, LONG, 8, False),                 # inside the first K - 1 samples
         "last sample": ("bs1770", 3, LONG, LONG - 1, False),
         "tile edge": ("bs1770", 3, LONG, TILE + 2, False),        # its window straddles samples TILE - 1 | TILE
         "second tile edge": ("kaiser 2x16", 3, LONG, 2 * TILE + 4, False),
         "wave end": ("bs1770", 3, LONG, 64 * PER_LANE - 1, False),  # the last sample of lane 63
         "negative": ("bs1770", 3, LONG, 1000, True),
         "negative 8x7": ("kaiser 8x7", 3, LONG, TILE + 3, True)}
ROW_COUNTS = (1, 3, 70)
MANY_ROWS, MANY_L = 70000, 40                                     # past 65535 rows


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (table name, x (rows, L) float32 read-only).  Names: '<table>/L=<n>', 'spot/<spot>', 'rows/<n>', 'many'."""
    kind, _, arg = name.partition("/")
    if kind == "spot":
        table, rows, L, at, negative = SPOTS[arg]
        x = planted(tables()[table], rows, L, at, 100 + sorted(SPOTS).index(arg), negative)
    elif kind == "rows":
        table, rows = "bs1770", int(arg)
        x = planted(tables()[table], 70, TILE + 1, 7 + 29 * np.arange(70), 7)[:rows]       # row r is the same in every batch
    elif kind == "many":
        table = "bs1770"
        x = planted(tables()[table], MANY_ROWS, MANY_L, 6 + np.arange(MANY_ROWS) % (MANY_L - 6), 9)
    else:
        table, L = kind, int(arg[2:])
        h = tables()[table]
        x = planted(h, 3, L, np.array([0, L // 2, L - 1]) + main_delay(h), 1000 + L)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return table, x


def all_cases():
    names = ["%s/L=%d" % (t, n) for t in TABLES for n in lengths(tables()[t].shape[1])]
    return names + ["spot/" + s for s in SPOTS] + ["rows/%d" % r for r in ROW_COUNTS] + ["many"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle on a case, computed once and shared: measure()'s dict without y."""
    table, x = case(name)
    ref = measure(x, tables()[table])
    ref.pop("y")
    return ref


def chunk_list(seed, total, longest=TILE + 1):
    """A seeded list of chunks of 1 .. longest samples that add up to `total`."""
    rng, out = np.random.default_rng(seed), []
    while total > 0:
        n = int(min(total, rng.integers(1, longest + 1)))
        out.append(n)
        total -= n
    return out


CHUNK_LISTS = {"seed 1": chunk_list(1, 3 * TILE + 5), "seed 2": chunk_list(2, 3 * TILE + 5), "seed 3": chunk_list(3, 3 * TILE + 5),
               "fifty ones": [1] * 50, "short then long": [3, 1, 7, 10, 11, 12, TILE + 1, 2, 2 * TILE + 9]}


def stream_signal(total, seed=77):
    """(2, 2, total) float32: noise with a planted sample per row, two leading axes as a module sees them."""
    h = tables()["bs1770"]
    x = planted(h, 4, total, np.array([total // 3, total // 2, total - 2, 9]) , seed)
    return np.ascontiguousarray(x.reshape(2, 2, total))


# ---- EBU Tech 3341, cases 15 to 19 ---------------------------------------------------------------------------------------
# case -> (fs / f, phase in degrees, amplitude, expected dBTP); read inside +0.2 / -0.4 dB
TECH3341 = {15: (4, 0.0, 0.5, -6.02), 16: (4, 45.0, 0.5, -6.02), 17: (6, 60.0, 0.5, -6.02), 18: (8, 67.5, 0.5, -6.02),
            19: (4, 45.0, 1.41, 2.98)}
TECH3341_READINGS = {15: -6.218, 16: -5.976, 17: -6.316, 18: -6.028, 19: 3.029}     # this table's, to 1e-3 dB


def tech3341(number, fade=480, seconds=0.25, sr=48000):
    """One channel of the case's sine, float64, with a raised-cosine fade-in of `fade` samples (0: the abrupt onset, whose
    step overshoots -- case 18 then reads -5.32 dBTP: a property of the signal, not of the meter)."""
    div, phase, amp, _ = TECH3341[number]
    n = np.arange(int(seconds * sr))
    x = amp * np.sin(2.0 * np.pi * n / div + np.deg2rad(phase))
    if fade:
        x[:fade] *= 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    return x


def passband_ripple(h, upto=0.4, points=2001):
    """(lowest, highest) gain in dB of the interpolator below `upto` x the input rate: |G(f)| / P of the prototype g[P k + p] =
    h[p][k] at the oversampled rate."""
    P, K = h.shape
    g = np.asarray(h, dtype=np.float64).T.reshape(-1)
    w = 2.0 * np.pi * np.linspace(0.0, upto, points) / P
    G = np.abs(np.exp(-1j * np.outer(w, np.arange(P * K))) @ g) / P
    return float(20.0 * np.log10(G.min())), float(20.0 * np.log10(G.max()))

"""Second-order sections for transforms.SOSFilter, designed on the host in float64.

Every function returns an (n, 6) float64 numpy array in scipy's `sos` layout -- b0 b1 b2 a0 a1 a2 per row, a0 == 1 -- that
goes as it is into SOSFilter / ops.sos_filter (or scipy.signal.sosfilt).  The one-section designs are the biquads of
R. Bristow-Johnson's Audio EQ Cookbook, restated: with w0 = 2 pi f / sr and alpha = sin(w0) / (2 Q),

    lowpass      b = ((1 - cos) / 2, 1 - cos, (1 - cos) / 2)           a = (1 + alpha, -2 cos, 1 - alpha)
    highpass     b = ((1 + cos) / 2, -(1 + cos), (1 + cos) / 2)        a as above
    bandpass     b = (alpha, 0, -alpha)   (peak gain 1)    or   (sin / 2, 0, -sin / 2)   (const_skirt_gain: peak gain Q)
    bandreject   b = (1, -2 cos, 1)
    allpass      b = (1 - alpha, -2 cos, 1 + alpha)
    equalizer    b = (1 + alpha A, -2 cos, 1 - alpha A)                a = (1 + alpha / A, -2 cos, 1 - alpha / A)
    low_shelf, high_shelf: the cookbook's shelves with A = 10^(gain_db / 40) and the same alpha (Q = 1 / sqrt(2): the
                 steepest slope without overshoot)

`k_weighting(sr)` is the two-section pre-filter of ITU-R BS.1770 (a high shelf, then a high-pass), from the analogue
prototypes behind the standard's 48 kHz table by the bilinear transform with K = tan(pi fc / sr); at 48 kHz it reproduces
the printed coefficients.  transforms.Loudness is the gated loudness measure on top of it.

`true_peak_filter(oversample, taps_per_phase, design)` is not a section cascade but the (P, K) polyphase FIR table of
transforms.TruePeak: the standard's own 48 taps, or a Kaiser-windowed sinc.

ValueError: f outside (0, sr / 2), Q <= 0, a non-finite argument.
"""
import math

import numpy as np

__all__ = ["lowpass", "highpass", "bandpass", "bandreject", "allpass", "equalizer", "low_shelf", "high_shelf",
           "k_weighting", "true_peak_filter"]

_SQRT_HALF = 1.0 / math.sqrt(2.0)


def _section(b, a):
    return np.array([[b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]]], dtype=np.float64)


def _angles(sr, f, Q):
    sr, f, Q = float(sr), float(f), float(Q)
    if not (math.isfinite(sr) and sr > 0.0):
        raise ValueError("sr must be finite and > 0, got %r" % (sr,))
    if not (math.isfinite(f) and 0.0 < f < sr / 2):
        raise ValueError("f must lie inside (0, sr / 2) = (0, %g), got %r" % (sr / 2, f))
    if not (math.isfinite(Q) and Q > 0.0):
        raise ValueError("Q must be finite and > 0, got %r" % (Q,))
    w0 = 2.0 * math.pi * f / sr
    return math.cos(w0), math.sin(w0), math.sin(w0) / (2.0 * Q)


def _amplitude(gain_db):
    gain_db = float(gain_db)
    if not math.isfinite(gain_db):
        raise ValueError("gain_db must be finite, got %r" % (gain_db,))
    return 10.0 ** (gain_db / 40.0)


def lowpass(sr, f, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    return _section(((1 - c) / 2, 1 - c, (1 - c) / 2), (1 + al, -2 * c, 1 - al))


def highpass(sr, f, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    return _section(((1 + c) / 2, -(1 + c), (1 + c) / 2), (1 + al, -2 * c, 1 - al))


def bandpass(sr, f, Q=_SQRT_HALF, const_skirt_gain=False):
    c, s, al = _angles(sr, f, Q)
    b = (s / 2, 0.0, -s / 2) if const_skirt_gain else (al, 0.0, -al)
    return _section(b, (1 + al, -2 * c, 1 - al))


def bandreject(sr, f, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    return _section((1.0, -2 * c, 1.0), (1 + al, -2 * c, 1 - al))


def allpass(sr, f, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    return _section((1 - al, -2 * c, 1 + al), (1 + al, -2 * c, 1 - al))


def equalizer(sr, f, gain_db, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    A = _amplitude(gain_db)
    return _section((1 + al * A, -2 * c, 1 - al * A), (1 + al / A, -2 * c, 1 - al / A))


def low_shelf(sr, f, gain_db, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    A = _amplitude(gain_db)
    r = 2 * math.sqrt(A) * al
    return _section((A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r)),
                    ((A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r))


def high_shelf(sr, f, gain_db, Q=_SQRT_HALF):
    c, _, al = _angles(sr, f, Q)
    A = _amplitude(gain_db)
    r = 2 * math.sqrt(A) * al
    return _section((A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)),
                    ((A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r))


# the analogue prototypes of BS.1770's pre-filter
_K_SHELF_FC, _K_SHELF_GAIN_DB, _K_SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
_K_SHELF_VB_EXPONENT = 0.4996667741545416
_K_HP_FC, _K_HP_Q = 38.13547087602444, 0.5003270373238773


def k_weighting(sr=48000):
    """The K-weighting pre-filter of ITU-R BS.1770 at sample rate sr: (2, 6), the high shelf first."""
    sr = float(sr)
    if not (math.isfinite(sr) and sr > 2 * _K_SHELF_FC):
        raise ValueError("k_weighting needs sr > %g Hz, got %r" % (2 * _K_SHELF_FC, sr))
    K = math.tan(math.pi * _K_SHELF_FC / sr)
    Vh = 10.0 ** (_K_SHELF_GAIN_DB / 20.0)
    Vb = Vh ** _K_SHELF_VB_EXPONENT
    shelf = _section((Vh + Vb * K / _K_SHELF_Q + K * K, 2 * (K * K - Vh), Vh - Vb * K / _K_SHELF_Q + K * K),
                     (1 + K / _K_SHELF_Q + K * K, 2 * (K * K - 1), 1 - K / _K_SHELF_Q + K * K))
    K = math.tan(math.pi * _K_HP_FC / sr)
    a0 = 1 + K / _K_HP_Q + K * K
    hp = np.array([[1.0, -2.0, 1.0, 1.0, 2 * (K * K - 1) / a0, (1 - K / _K_HP_Q + K * K) / a0]], dtype=np.float64)
    return np.concatenate([shelf, hp], axis=0)


# the interpolation filter of ITU-R BS.1770-4 Annex 2 in units of 1 / 8192: phases 0 and 1; phases 2 and 3 are their reversals
_TRUE_PEAK_BS1770 = ((14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68),
                     (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155))
TRUE_PEAK_KAISER_BETA = 5.0


def true_peak_filter(oversample=4, taps_per_phase=12, design="bs1770"):
    """The polyphase interpolation filter of a true-peak meter: a float64 (P, K) table, P = oversample phases of K =
    taps_per_phase taps, phase p giving the oversampled value y[P n + p] = sum_k h[p][k] x[n - k].

    design="bs1770": the 48-tap table of ITU-R BS.1770-4 Annex 2, every entry a multiple of 1 / 8192; only (4, 12).
    design="kaiser": a Kaiser-windowed sinc (beta = 5) of P K taps with its cutoff at the input's Nyquist frequency, each
    phase scaled to unity DC gain; P in {2, 4, 8}, K in 4 .. 64.  ValueError for anything else."""
    P, K = int(oversample), int(taps_per_phase)
    if P != oversample or K != taps_per_phase:
        raise ValueError("oversample and taps_per_phase must be integers, got %r and %r" % (oversample, taps_per_phase))
    if design == "bs1770":
        if (P, K) != (4, 12):
            raise ValueError("the BS.1770 table is 4 phases of 12 taps, got (%d, %d): use design='kaiser'" % (P, K))
        a, b = (np.array(r, dtype=np.float64) / 8192.0 for r in _TRUE_PEAK_BS1770)
        return np.stack([a, b, b[::-1], a[::-1]])
    if design == "kaiser":
        if P not in (2, 4, 8) or not 4 <= K <= 64:
            raise ValueError("the Kaiser design takes oversample in {2, 4, 8} and 4 <= taps_per_phase <= 64, got (%d, %d)" % (P, K))
        i = np.arange(P * K, dtype=np.float64)
        g = np.sinc((i - (P * K - 1) / 2.0) / P) * np.kaiser(P * K, TRUE_PEAK_KAISER_BETA)
        h = g.reshape(K, P).T.copy()                         # g[P k + p] = h[p][k]
        return h / h.sum(axis=1, keepdims=True)
    raise ValueError("design must be 'bs1770' or 'kaiser', got %r" % (design,))

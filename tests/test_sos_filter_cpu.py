"""CPU side of the recursive filters (ops.sos_filter, transforms.SOSFilter / RealtimeSOSFilter / Preemphasis,
utils.filter_design, at_sos_filter of csrc/sos_filter.hip): the oracle of sos_filter_cases.py against scipy, the adjoint
identity the backward rests on, every design by its defining property on the unit circle, the answers of the C entries
that need no device, and the host-side errors.  No test here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import sos_filter_cases as C
from acids_transforms_amd import _lib, autograd, ops
from acids_transforms_amd.utils import filter_design as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def H(sos, w):
    """The cascade's frequency response at w rad / sample, in float64."""
    z = np.exp(-1j * np.asarray(w, dtype=np.float64))
    out = np.ones_like(z)
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos, dtype=np.float64):
        out = out * (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
    return out


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_is_scipy_sosfilt_with_and_without_state(name):
    sg = pytest.importorskip("scipy.signal")
    sos = C.FILTERS[name]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 700))
    zi = rng.standard_normal((2, 3, sos.shape[0], 2))
    y, zf = C.sosfilt(sos, x)
    assert C.rel_max(y, sg.sosfilt(sos, x, axis=-1)) < 1e-13
    ry, rzf = sg.sosfilt(sos, x, axis=-1, zi=np.moveaxis(zi, -2, 0))
    y, zf = C.sosfilt(sos, x, zi)
    assert C.rel_max(y, ry) < 1e-13 and C.rel_max(zf, np.moveaxis(rzf, 0, -2)) < 1e-13


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_zero_phase_against_scipy(name):
    """primed: scipy.signal.sosfiltfilt(padtype=None), which starts both passes in the steady state of a step as high as
    the edge sample.  Zero state (what the kernel computes): sosfilt, flipped, twice; the two differ, and only the second
    is its own adjoint."""
    sg = pytest.importorskip("scipy.signal")
    sos = C.FILTERS[name]
    x = np.random.default_rng(4).standard_normal((3, 500)) + 0.5
    assert C.rel_max(C.steady_state(sos), sg.sosfilt_zi(sos)) < 1e-9
    assert C.rel_max(C.zero_phase(sos, x, primed=True), sg.sosfiltfilt(sos, x, axis=-1, padtype=None)) < 1e-9
    twice = sg.sosfilt(sos, sg.sosfilt(sos, x, axis=-1)[:, ::-1], axis=-1)[:, ::-1]
    assert C.rel_max(C.zero_phase(sos, x), twice) < 1e-13
    g = np.random.default_rng(5).standard_normal((3, 500))
    assert abs(np.sum(C.zero_phase(sos, x) * g) - np.sum(x * C.zero_phase(sos, g))) < 1e-10 * np.sum(np.abs(x) * np.abs(g)) * 500


@pytest.mark.parametrize("name", C.NAMES)
def test_the_adjoint_is_the_filter_run_backwards(name):
    """L = 300: H as a lower-triangular Toeplitz matrix of the impulse response, its transpose by float64 torch autograd."""
    sos, L = C.FILTERS[name], 300
    h = C.sosfilt(sos, np.eye(1, L)[0])[0]
    idx = np.arange(L)[:, None] - np.arange(L)[None, :]
    T = torch.from_numpy(np.where(idx >= 0, h[np.clip(idx, 0, L - 1)], 0.0))
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal(L)).requires_grad_()
    g = rng.standard_normal(L)
    y = T @ x
    assert C.rel_max(y.detach().numpy(), C.sosfilt(sos, x.detach().numpy())[0]) < 1e-9
    (y * torch.from_numpy(g)).sum().backward()
    gx = C.sosfilt_reverse(sos, g)
    assert C.rel_max(gx, x.grad.numpy()) < 1e-9
    xn = x.detach().numpy()
    lhs, rhs = np.sum(C.sosfilt(sos, xn)[0] * g), np.sum(xn * gx)
    assert abs(lhs - rhs) < 1e-13 * np.sum(np.abs(C.sosfilt(sos, xn)[0]) * np.abs(g)) * L


def test_case_table_follows_the_plan():
    tile, per_lane, dispatch = C.plan(1)
    assert tile == 256 * per_lane and dispatch == 0
    for n in (1, 2, 4, 16):
        for rows, L in ((1, 1), (1, 2 ** 24), (70, tile + 1), (100000, 7)):
            assert ops.sos_filter_plan(rows, L, n) == (tile, per_lane, 0)      # one dispatch: nothing depends on the shape
        assert C.lengths(n) == (1, 2, 3, per_lane - 1, per_lane, per_lane + 1, tile - 1, tile, tile + 1, 2 * tile + 5)
    assert [C.FILTERS[k].shape[0] for k in C.NAMES] == [1, 1, 1, 4, 2, 16]
    for sos in C.FILTERS.values():                                   # every case is stable
        for s in sos:
            assert np.abs(np.roots(s[3:])).max() < 1.0


# ---- the designs -----------------------------------------------------------------------------------------------------------
SR, F0 = 44100.0, 1234.5
W0 = 2 * np.pi * F0 / SR


@pytest.mark.parametrize("Q", [0.5, 0.7071, 3.0])
def test_lowpass_and_highpass(Q):
    lo, hi = fd.lowpass(SR, F0, Q), fd.highpass(SR, F0, Q)
    assert lo.shape == hi.shape == (1, 6) and lo.dtype == np.float64 and lo[0, 3] == hi[0, 3] == 1.0
    assert abs(abs(H(lo, 0.0)) - 1) < 1e-12 and abs(abs(H(lo, W0)) - Q) < 1e-12 * Q and abs(H(lo, np.pi)) < 1e-12
    assert abs(abs(H(hi, np.pi)) - 1) < 1e-12 and abs(abs(H(hi, W0)) - Q) < 1e-12 * Q and abs(H(hi, 0.0)) < 1e-12


@pytest.mark.parametrize("gain", [-12.0, 3.0, 6.0])
def test_equalizer_and_shelves(gain):
    lin = 10 ** (gain / 20)
    eq = fd.equalizer(SR, F0, gain, 4.0)
    assert abs(abs(H(eq, W0)) - lin) < 1e-12 * lin and abs(abs(H(eq, 0.0)) - 1) < 1e-12 and abs(abs(H(eq, np.pi)) - 1) < 1e-12
    lo, hi = fd.low_shelf(SR, F0, gain), fd.high_shelf(SR, F0, gain)
    assert abs(abs(H(lo, 0.0)) - lin) < 1e-12 * lin and abs(abs(H(lo, np.pi)) - 1) < 1e-12
    assert abs(abs(H(hi, np.pi)) - lin) < 1e-12 * lin and abs(abs(H(hi, 0.0)) - 1) < 1e-12
    for sos in (eq, lo, hi):
        assert np.abs(np.roots(sos[0, 3:])).max() < 1.0


def test_bandpass_bandreject_allpass():
    w = np.linspace(0.01, np.pi - 0.01, 97)
    Q = 2.5
    assert abs(H(fd.bandreject(SR, F0, Q), W0)) < 1e-12
    assert abs(abs(H(fd.bandreject(SR, F0, Q), 0.0)) - 1) < 1e-12 and abs(abs(H(fd.bandreject(SR, F0, Q), np.pi)) - 1) < 1e-12
    assert np.abs(np.abs(H(fd.allpass(SR, F0, Q), w)) - 1).max() < 1e-12
    bp, skirt = fd.bandpass(SR, F0, Q), fd.bandpass(SR, F0, Q, const_skirt_gain=True)
    assert abs(abs(H(bp, W0)) - 1) < 1e-12 and abs(abs(H(skirt, W0)) - Q) < 1e-12 * Q
    for sos in (bp, skirt):
        assert abs(H(sos, 0.0)) < 1e-12 and abs(H(sos, np.pi)) < 1e-12


def test_k_weighting_is_the_table_of_bs1770_at_48_khz():
    table = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                      [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
    k = fd.k_weighting(48000)
    assert k.shape == (2, 6) and k.dtype == np.float64
    assert np.abs(k - table).max() < 1e-14
    k44 = fd.k_weighting(44100)                   # another rate: the same analogue filter, so the same gain far above the shelf
    assert abs(abs(H(k44, 2 * np.pi * 10000 / 44100)) - abs(H(k, 2 * np.pi * 10000 / 48000))) < 2e-2
    assert abs(H(k44, 0.0)) < 1e-12


def test_design_errors():
    for f in (0.0, -1.0, SR / 2, SR, float("nan")):
        for make in (fd.lowpass, fd.highpass, fd.bandpass, fd.bandreject, fd.allpass):
            with pytest.raises(ValueError):
                make(SR, f, 1.0)
        for make in (fd.equalizer, fd.low_shelf, fd.high_shelf):
            with pytest.raises(ValueError):
                make(SR, f, 3.0, 1.0)
    for Q in (0.0, -2.0, float("inf")):
        with pytest.raises(ValueError):
            fd.lowpass(SR, F0, Q)
        with pytest.raises(ValueError):
            fd.equalizer(SR, F0, 3.0, Q)
    with pytest.raises(ValueError):
        fd.k_weighting(3000)


# ---- the C entries, without a device ---------------------------------------------------------------------------------------
def _call(sos, rows=0, L=0, n=None, reverse=0, zi=0, zf=0, x=64, y=128):
    sos = None if sos is None else np.ascontiguousarray(sos, dtype=np.float64)
    n = (0 if sos is None else sos.shape[0]) if n is None else n
    p = ctypes.c_void_p
    return _lib.lib().at_sos_filter(p(x), rows, L, p(sos.ctypes.data) if sos is not None else p(0), n, reverse, p(zi), p(zf),
                                    p(y), p(0))


def test_c_entry_answers_that_need_no_device():
    ok = C.FILTERS["kweighting"]
    assert _call(ok) == _lib.AT_OK and _call(ok, rows=0, L=100) == _lib.AT_OK           # nothing to do
    assert _call(ok, rows=-1) == _lib.AT_EINVAL and _call(ok, L=-1) == _lib.AT_EINVAL
    assert _call(ok, n=0) == _lib.AT_EINVAL and _call(None, n=1) == _lib.AT_EINVAL
    assert _call(np.tile(ok, (9, 1))[:17]) == _lib.AT_EUNSUPPORTED and _call(np.tile(ok, (8, 1))) == _lib.AT_OK
    for bad in (np.nan, np.inf):
        for j in range(6):
            s = ok.copy()
            s[1, j] = bad
            assert _call(s) == _lib.AT_EINVAL
    s = ok.copy()
    s[0, 3] = 2.0
    assert _call(s) == _lib.AT_EINVAL                                                     # a0 != 1: the host divides
    assert _call(ok, reverse=1) == _lib.AT_OK
    assert _call(ok, reverse=1, zi=64) == _lib.AT_EINVAL and _call(ok, reverse=1, zf=64) == _lib.AT_EINVAL
    assert _call(ok, reverse=2) == _lib.AT_EINVAL
    assert _call(ok, zi=64, zf=64) == _lib.AT_EINVAL and _call(ok, zi=68) == _lib.AT_EINVAL   # aliased, misaligned state
    assert _call(ok, rows=2, L=5, x=0) == _lib.AT_EINVAL and _call(ok, rows=2, L=5, y=0) == _lib.AT_EINVAL
    assert _call(ok, rows=2, L=5, x=66) == _lib.AT_EINVAL
    t, s_, d = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(7)
    plan = _lib.lib().at_sos_filter_plan
    assert plan(3, 100, 2, ctypes.byref(t), ctypes.byref(s_), ctypes.byref(d)) == _lib.AT_OK
    assert (t.value, s_.value, d.value) == ops.sos_filter_plan(3, 100, 2) and t.value == 256 * s_.value
    assert plan(-1, 100, 2, ctypes.byref(t), ctypes.byref(s_), ctypes.byref(d)) == _lib.AT_EINVAL
    assert plan(3, 100, 0, ctypes.byref(t), ctypes.byref(s_), ctypes.byref(d)) == _lib.AT_EINVAL
    assert plan(3, 100, 17, ctypes.byref(t), ctypes.byref(s_), ctypes.byref(d)) == _lib.AT_EUNSUPPORTED
    assert plan(3, 100, 2, None, ctypes.byref(s_), ctypes.byref(d)) == _lib.AT_EINVAL


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ("at_sos_filter", "at_sos_filter_plan"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 4
    for name in ("SosFilterFunction", "SosFilterStreamFunction"):
        assert name in autograd.__all__ and issubclass(getattr(autograd, name), torch.autograd.Function)
    for name in ("SOSFilter", "RealtimeSOSFilter", "Preemphasis"):
        assert name in A.transforms.__all__ and getattr(A, name) is getattr(A.transforms, name)
    assert A.filters is A.transforms.filters and A.filter_design is fd
    mk = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "Makefile")).read()
    assert re.search(r"sos_filter\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk)


# ---- host-side behaviour ---------------------------------------------------------------------------------------------------
def test_coefficients_are_checked_and_normalised_on_the_host():
    co = ops.sos_coefficients([[2.0, 1.0, 0.5, 2.0, -1.0, 0.25]])
    assert co.array.dtype == np.float64 and co.array.tolist() == [[1.0, 0.5, 0.25, 1.0, -0.5, 0.125]]
    assert ops.sos_coefficients(co) is co
    assert ops.sos_coefficients(torch.tensor([[1.0, 0, 0, 1, 0, 0]])).n == 1
    for bad in ([1.0, 0, 0, 1, 0, 0], [[1.0, 0, 0, 1, 0]], np.zeros((0, 6)), np.zeros((2, 3, 6)),
                [[1.0, 0, 0, 0.0, 0, 0]], [[np.nan, 0, 0, 1, 0, 0]], [[1.0, 0, 0, 1, np.inf, 0]]):
        with pytest.raises(ValueError):
            ops.sos_coefficients(bad)
        with pytest.raises(ValueError):
            A.SOSFilter(bad)


def test_cpu_tensors_and_float64_audio_are_refused():
    sos = C.FILTERS["peak1k"]
    with pytest.raises(A.AcidsHipError):
        ops.sos_filter(torch.zeros(2, 10), sos)
    with pytest.raises(A.AcidsHipError):
        A.SOSFilter(sos)(torch.zeros(2, 10))
    with pytest.raises(A.AcidsHipError):
        A.RealtimeSOSFilter(sos)(torch.zeros(2, 10))
    with pytest.raises(ValueError):
        ops.sos_filter(torch.zeros(2, 10), sos, reverse=True, return_state=True)
    with pytest.raises(ValueError):
        ops.sos_filter(torch.zeros(2, 10), sos, reverse=True, zi=torch.zeros(2, 1, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sos_filter(torch.tensor(1.0), sos)


def test_modules_on_the_host():
    hp = C.FILTERS["highpass20"]
    x = torch.zeros(3, 5)
    assert A.SOSFilter()(x) is x and A.RealtimeSOSFilter()(x) is x and A.SOSFilter().n_sections == 0
    m = A.SOSFilter(hp)
    assert m.sos.dtype == torch.float64 and not m.invertible and m.n_sections == 1
    with pytest.raises(A.NotInvertibleError):
        m.invert(x)
    for cast in (lambda t: t.half(), lambda t: t.float(), lambda t: t.to(torch.bfloat16)):
        sd = cast(A.SOSFilter(hp)).state_dict()
        assert sd["sos"].dtype == torch.float64 and np.array_equal(sd["sos"].numpy(), hp)
        back = A.SOSFilter()
        back.load_state_dict(sd)
        assert np.array_equal(back.coefficients, hp) and np.array_equal(cast(back).coefficients, hp)
    rt = m.streaming()
    assert isinstance(rt, A.RealtimeSOSFilter) and rt._co is m._co and rt.latency == 0 and rt.streaming() is rt
    assert rt.state.dtype == torch.float64 and tuple(rt.state.shape) == (1, 2) and isinstance(m.realtime(), A.RealtimeSOSFilter)
    rt.state = torch.ones(4, 2, 1, 2, dtype=torch.float64)
    other = A.RealtimeSOSFilter(C.FILTERS["peak1k"])
    other.load_state_dict(rt.state_dict())
    assert torch.equal(other.state, rt.state) and np.array_equal(other.coefficients, hp)
    other.reset()
    assert tuple(other.state.shape) == (4, 2, 1, 2) and not other.state.any()
    zp = A.SOSFilter(hp, zero_phase=True)
    with pytest.raises(ValueError):
        zp.streaming()
    with pytest.warns(UserWarning):
        assert zp.realtime() is zp
    with pytest.raises(ValueError):
        A.RealtimeSOSFilter(hp, zero_phase=True)
    pre = A.Preemphasis()
    assert pre.invertible and pre.coeff == 0.97 and pre.coefficients.tolist() == [[1.0, -0.97, 0.0, 1.0, 0.0, 0.0]]
    assert pre._inverse.array.tolist() == [[1.0, 0.0, 0.0, 1.0, -0.97, 0.0]]
    for c in (1.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            A.Preemphasis(c)
    for cls in (A.SOSFilter, A.RealtimeSOSFilter, A.Preemphasis):
        assert callable(cls().test_forward) and callable(cls.test_scripted_transform)

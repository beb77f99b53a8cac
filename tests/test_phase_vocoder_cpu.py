"""TimeStretch without a device (transforms.TimeStretch, ops.phase_vocoder*, autograd.PhaseVocoderFunction,
at_phase_vocoder / at_phase_vocoder_backward of csrc/phase_vocoder.hip): the step table against cases written out by
hand, the identity the kernel rests on -- the phasor product equals the textbook angle / wrap / advance / cumsum algorithm
whatever the hop -- and the backward's gather against float64 autograd of the textbook, both in float64 on the CPU; then
the surface and the argument checks that answer before any launch."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import acids_transforms_amd as A
import phase_vocoder_cases as C
from acids_transforms_amd import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_phase_vocoder", "at_phase_vocoder_backward")


def _table(T, rate):
    idx, alpha = ops.phase_vocoder_steps(T, rate)
    assert idx.dtype == torch.int32 and alpha.dtype == torch.float32 and idx.shape == alpha.shape and idx.ndim == 1
    assert idx.device.type == "cpu" and alpha.device.type == "cpu"
    return idx.tolist(), alpha.tolist()


def _f32(values):
    return torch.tensor(values, dtype=torch.float64).to(torch.float32).tolist()


@pytest.mark.parametrize("rate,idx,alpha", [
    (0.5, [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8], [0.0, 0.5] * 9),
    (0.8, [0, 0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 8], [0.0, 0.8, 0.6, 0.4, 0.2, 0.0, 0.8, 0.6, 0.4, 0.2, 0.0, 0.8]),
    (1 / 1.1, [0, 0, 1, 2, 3, 4, 5, 6, 7, 8], [0.0] + [k / 11 for k in (10, 9, 8, 7, 6, 5, 4, 3, 2)]),     # frac(10 j / 11)
    (1.3, [0, 1, 2, 3, 5, 6, 7], [0.0, 0.3, 0.6, 0.9, 0.2, 0.5, 0.8]),
    (2.0, [0, 2, 4, 6, 8], [0.0] * 5),
    (3.0, [0, 3, 6], [0.0] * 3),
    (100.0, [0], [0.0]),
])
def test_step_table_of_nine_frames(rate, idx, alpha):
    got_idx, got_alpha = _table(9, rate)
    assert got_idx == idx
    assert got_alpha == _f32(alpha)
    assert (got_idx, _f32(C.steps(9, rate)[1])) == (idx, got_alpha)          # the rule written out as a loop agrees


def test_step_table_edges_and_errors():
    assert _table(1, 0.5) == ([0, 0], [0.0, 0.5]) and _table(1, 1.0) == ([0], [0.0]) and _table(1, 7.0) == ([0], [0.0])
    assert _table(0, 0.8) == ([], [])
    # an exact multiple at the edge: 4 * 2.25 = 9.0 is not < 9, 4 * 2.2 = 8.8 is; 0.75 * 12 = 9.0 is not, row 11 = 8.25 is
    assert _table(9, 2.25) == ([0, 2, 4, 6], [0.0, 0.25, 0.5, 0.75])
    assert _table(9, 2.2)[0] == [0, 2, 4, 6, 8]
    assert _table(9, 0.75)[0] == [0, 0, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8] and _table(9, 0.75)[1][-1] == 0.25
    assert _table(9, 1.0) == (list(range(9)), [0.0] * 9)
    # ceil(T / rate) except for rounding at the edge: 0.1 * 30 rounds to 3.0000000000000004 in float64
    assert len(_table(3, 0.1)[0]) == 30 and len(_table(690, 0.8)[0]) == 863
    idx, alpha = _table(690, 1 / 1.1)
    assert all(b - a in (0, 1) for a, b in zip(idx, idx[1:])) and idx[0] == 0 and idx[-1] + 1 <= 690
    assert all(0.0 <= a <= 1.0 for a in alpha)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            ops.phase_vocoder_steps(9, bad)
    with pytest.raises(ValueError):
        ops.phase_vocoder_steps(-1, 1.0)
    with pytest.raises(ValueError):
        ops.phase_vocoder_steps(690, 1e-7)                    # 6.9e9 rows: past the kernel's int row index
    assert ops.PV_MAX_ROWS < 2 ** 31 - 1


def _planted(T, F, seed):
    X = C.spectrum((3, T, F), seed).to(torch.complex128)
    X[0, 0] = 0                                               # an all-zero first frame
    X[1, T // 2, ::3] = 0                                     # zero bins inside
    X[2, T - 1, 1::2] = 0                                     # ... and in the last frame
    X[2, :, F - 1] = 0                                        # a bin that is silent throughout
    return X


@pytest.mark.parametrize("T", (1, 2, 9, 33))
@pytest.mark.parametrize("rate", C.RATES)
def test_phasor_product_is_the_textbook_algorithm_whatever_the_hop(T, rate):
    X = _planted(T, 17, 100 + T)
    idx, alpha = C.steps(T, rate)
    Z, fin = C.phasor_product(X, idx, alpha)
    assert Z.shape == (3, len(idx), 17) and bool(torch.isfinite(torch.view_as_real(Z)).all())
    worst = max(C.normwise(Z, C.textbook(X, rate, hop)) for hop in (128, 256))
    assert worst < 1e-9, worst
    assert abs(float(fin.abs().max()) - 1.0) < 1e-12 and not Z[2, :, 16].any()


@pytest.mark.parametrize("T", (1, 2, 9, 33))
@pytest.mark.parametrize("rate", C.RATES)
def test_gather_backward_is_autograd_of_the_textbook(T, rate):
    """At hop 1: the textbook's accumulated phase grows by up to pi * hop a step, 5e4 rad over 66 steps at hop 256, where one
    float64 ulp is 7e-12 -- the reference itself is then no better than 4e-12 (measured: 3.8e-12 at T = 33, rate 0.5),
    above the 1e-12 asked of the formula.  The hop has no effect on what is differentiated (the identity above)."""
    X = _planted(T, 17, 200 + T)
    idx, alpha = C.steps(T, rate)
    g = C.spectrum((3, len(idx), 17), 300 + T).to(torch.complex128)
    Xr = X.clone().requires_grad_()
    (want,) = torch.autograd.grad(C.textbook(Xr, rate, 1), Xr, grad_outputs=g)
    fin = C.phasor_product(X, idx, alpha)[1]
    got = C.gather_backward(X, g, idx, alpha, fin)
    assert not torch.isnan(torch.view_as_real(got)).any()     # every frame was written, the skipped ones with zeros
    assert C.normwise(got, want) < 1e-12, C.normwise(got, want)
    assert not got[X == 0].any()                              # zero bins: exactly zero


def test_surface():
    assert A.TimeStretch is A.transforms.TimeStretch is A.transforms.stretch.TimeStretch and A.stretch is A.transforms.stretch
    assert "TimeStretch" in A.transforms.__all__ and "PhaseVocoderFunction" in autograd.__all__
    assert issubclass(A.TimeStretch, A.AudioTransform)
    t = A.TimeStretch()
    assert (t.rate, t.n_freq, t.hop_length, t.sr) == (1.0, None, None, 44100)
    assert not t.invertible and not t.scriptable and not t.needs_scaling and t.ratio == 1.0
    assert A.TimeStretch(0.8).ratio == 1 / 0.8 and A.TimeStretch(rate=2.0, n_freq=513, hop_length=256, sr=16000).sr == 16000
    with pytest.raises(A.NotInvertibleError):
        t.invert(torch.zeros(2, 3, 5, dtype=torch.complex64))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert t.realtime() is t
    assert len(w) == 1 and "streaming" in str(w[0].message)
    x = torch.zeros(2, 3, 5, dtype=torch.complex64)
    time = torch.zeros(2)
    assert t(x) is x and t(x, overriding_rate=1.0) is x       # rate 1: the argument itself, on any device
    y, tm = t.forward_with_time(x, time)
    assert y is x and tm is time
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            A.TimeStretch(bad)
        with pytest.raises(ValueError):
            t(x, overriding_rate=bad)
    with pytest.raises(ValueError):
        A.TimeStretch(0.8)(torch.zeros(2, 3, 5))               # a real input
    with pytest.raises(ValueError):
        ops.phase_vocoder(torch.zeros(2, 3, 5), 0.8)
    with pytest.raises(ValueError):
        A.TimeStretch(0.8, n_freq=513)(x)                      # n_freq is checked against the input
    with pytest.raises(A.AcidsHipError):
        A.TimeStretch(0.8)(x)                                  # no CPU route
    with pytest.raises(A.AcidsHipError):
        A.TimeStretch(0.8)(x.clone().requires_grad_())         # the grad route raises what the plain one does
    with pytest.raises(A.AcidsHipError):
        A.TimeStretch(0.8)(x.to(torch.complex128))
    with pytest.raises(A.AcidsHipError):
        ops.phase_vocoder_backward(x, x, 0.8, x[:, 0])
    doc = A.transforms.stretch.__doc__ + ops.phase_vocoder.__doc__
    assert "hop_length" in doc and "no effect" in doc and "-0 + 0i" in doc


def test_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    src = open(os.path.join(ROOT, "acids_transforms_amd", "_lib.py")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert re.search(r"\bint %s\s*\(" % name, hdr) and '"%s"' % name in src
    assert lib.at_abi_version() == 4                              # additive: the ABI version stays
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in ENTRIES)


def test_argument_checks_answer_before_any_launch():
    lib = _lib.lib()
    E, U, OK = _lib.AT_EINVAL, _lib.AT_EUNSUPPORTED, _lib.AT_OK
    null = ctypes.c_void_p(0)
    a, b, c, d = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))   # never dereferenced: every call answers before a launch

    def fwd(B, T, F, N, X=null, idx=null, alpha=null, out=null, fin=null):
        return lib.at_phase_vocoder(X, B, T, F, idx, alpha, N, out, fin, null)

    def bwd(B, T, F, N, X=null, g=null, idx=null, alpha=null, fin=null, gX=null):
        return lib.at_phase_vocoder_backward(X, g, idx, alpha, fin, B, T, F, N, gX, null)

    for call in (fwd, bwd):
        assert call(0, 9, 5, 12) == OK and call(2, 9, 0, 12) == OK and call(2, 0, 5, 0) == OK     # empty work
        assert call(2, 9, 5, 12) == E                              # a legal shape with null pointers
        assert call(-1, 9, 5, 12) == E and call(2, -9, 5, 12) == E and call(2, 9, -5, 12) == E and call(2, 9, 5, -1) == E
        assert call(2, 9, 5, 0) == E and call(2, 0, 5, 3) == E     # rows without frames, frames without rows
        assert call(2, 2 ** 31, 5, 12) == U and call(2, 9, 5, 2 ** 31 - 8) == U
        assert call(2 ** 31, 9, 5, 12) == U and call(2 ** 20, 9, 2 ** 40, 12) == U
    assert fwd(2, 9, 5, 12, a, b, c, a) == E                       # out == X
    assert fwd(2, 9, 5, 12, ctypes.c_void_p(260), b, c, d) == E    # a complex tensor off its 8-byte boundary
    assert fwd(2, 9, 5, 12, a, ctypes.c_void_p(514), c, d) == E
    assert fwd(2, 9, 5, 12, a, b, c, d, ctypes.c_void_p(1028)) == E
    assert bwd(2, 9, 5, 12, a, b, c, d, null, a) == E              # the final phasor is required
    assert bwd(2, 9, 5, 12, a, b, c, d, a, a) == E and bwd(2, 9, 5, 12, a, b, c, d, a, b) == E     # gX is X, gX is g
    assert bwd(2, 9, 5, 12, a, ctypes.c_void_p(516), c, d, a, ctypes.c_void_p(2048)) == E

"""Host side of the long-filter convolution (ops.fft_convolve_plan, at_fft_convolve_plan / at_spectral_fir /
at_spectral_fir_corr of csrc/fft_convolve.hip, transforms.FFTConvolve / Convolve / ImpulseResponse): the plan's block rule at
every edge of the ladder, the partitioned algorithm and its four gradient formulas restated in float64 against
numpy.convolve and conv1d's autograd, the mode cuts, the C entries' answers that need no device, bindings, exports and the
errors a caller can make.  No device needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import fft_convolve_cases as C
from acids_transforms_amd import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = (128, 256, 512, 1024, 2048)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_block_rule_at_every_edge_of_the_ladder():
    """The rule that ships: the smallest block of 512, 1024, 2048 with at most 4 partitions, else 2048; 128 and 256 by
    block= only.  (The probe measured 2 B ahead of the rule as first counted -- 16 partitions from 128 up -- and again of its
    first revision -- 8 partitions from 256 up -- at 513 and at 4096 taps: DESIGN 7i.)"""
    assert ops.FFT_CONVOLVE_BLOCKS == LADDER
    rule = LADDER[2:]
    for K in (1, 2, 513, 4 * 512):
        assert ops.fft_convolve_plan(1, K)[0] == 512
    for i, B in enumerate(rule):
        assert ops.fft_convolve_plan(1000, 4 * B)[0] == B                         # 4 partitions still fit
        assert ops.fft_convolve_plan(1000, 4 * B + 1)[0] == rule[min(i + 1, 2)]   # one tap more: the next block
    for K, B in ((513, 512), (4096, 1024), (22050, 2048), (66150, 2048)):         # the probe's taps
        assert ops.fft_convolve_plan(176400, K)[0] == B
    for K in (4 * 2048 + 1, 66150, 88200, 10 ** 6):                               # past the ladder: 2048, more partitions
        B, T, P, _, _ = ops.fft_convolve_plan(44100, K)
        assert B == 2048 and P == -(-K // 2048) and P > 4
    assert ops.fft_convolve_plan(1000, 300, 128)[0] == 128 and ops.fft_convolve_plan(1000, 300, 256)[0] == 256


@pytest.mark.parametrize("block", (None,) + LADDER)
def test_frames_partitions_and_chunks_follow_the_formulas(block):
    for L, K in ((1, 1), (37, 20), (127, 129), (1000, 300), (5000, 40000), (176400, 513), (44100, 66150)):
        B, T, P, tile, chunk = ops.fft_convolve_plan(L, K, block)
        if block is not None:
            assert B == block
        M = L + K - 1
        assert T == -(-M // B) and P == -(-K // B) and tile == C.FRAME_TILE >= 2
        assert chunk == max(1, 2 ** 26 // (T * (B + 1)))
    assert ops.fft_convolve_plan(2 ** 27, 1, 128)[4] == 1                         # one row is already past 2^26: one row


def test_plan_rejects_what_it_must():
    for block in (0, 64, 100, 129, 4096, -128, 128.5, True):
        with pytest.raises(ValueError):
            ops.fft_convolve_plan(100, 10, block)
    for L, K in ((0, 1), (1, 0), (-3, 4)):
        with pytest.raises(ValueError):
            ops.fft_convolve_plan(L, K)
    plan = _lib.lib().at_fft_convolve_plan
    out = [ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)]
    refs = [ctypes.byref(o) for o in out]
    assert plan(100, 10, 0, *refs) == _lib.AT_OK and out[0].value == 512
    assert plan(100, 10, 512, *refs) == _lib.AT_OK and out[0].value == 512
    assert plan(0, 10, 0, *refs) == _lib.AT_EINVAL and plan(100, 0, 0, *refs) == _lib.AT_EINVAL
    assert plan(100, 10, 100, *refs) == _lib.AT_EINVAL and plan(100, 10, -1, *refs) == _lib.AT_EINVAL
    for i in range(5):
        assert plan(100, 10, 0, *[None if j == i else r for j, r in enumerate(refs)]) == _lib.AT_EINVAL


# ---- the algorithm, in float64 -----------------------------------------------------------------------------------------------
ALGO_CASES = ((37, 1, 8), (37, 20, 8), (100, 45, 8), (16, 40, 8), (8, 8, 8), (1, 5, 4), (65, 64, 16))


@pytest.mark.parametrize("per_row", (False, True), ids=("shared", "per_row"))
@pytest.mark.parametrize("L,K,B", ALGO_CASES)
def test_partitioned_forward_and_backward_formulas_in_float64(L, K, B, per_row):
    g = np.random.default_rng(L * 100 + K)
    rows = 3
    x = g.standard_normal((rows, L))
    h = g.standard_normal((rows, K) if per_row else K)
    ct = g.standard_normal((rows, L + K - 1))
    want = C.oracle(x, h)
    got = C.partitioned(torch.as_tensor(x), torch.as_tensor(h), B).numpy()
    assert got.shape == want.shape and C.rel_max(got, want) < 1e-10
    y, gx, gh = C.conv1d_autograd(x, h, ct)
    assert C.rel_max(y, want) < 1e-10                                           # the two references agree
    px, ph = C.partitioned_backward(torch.as_tensor(x), torch.as_tensor(h), torch.as_tensor(ct), B)
    assert px.shape == gx.shape and ph.shape == gh.shape
    assert C.rel_max(px.numpy(), gx) < 1e-10 and C.rel_max(ph.numpy(), gh) < 1e-10


def test_spectral_fir_reference_directions():
    """The anticausal conjugate FIR is the adjoint of the causal one, and the correlation the adjoint in H: <H * X, G> etc."""
    g = np.random.default_rng(5)
    cplx = lambda *s: g.standard_normal(s) + 1j * g.standard_normal(s)
    X, H, G = cplx(2, 9, 3), cplx(2, 4, 3), cplx(2, 9, 3)
    Y = C.spectral_fir_reference(X, H)
    gX = C.spectral_fir_reference(G, H, anticausal=True, conj=True)
    gH = C.spectral_fir_corr_reference(X, G, 4, shared=False)
    dot = lambda a, b: float((a.conj() * b).real.sum())
    assert abs(dot(Y, G) - dot(X, gX)) < 1e-10 and abs(dot(Y, G) - dot(H, gH)) < 1e-10
    assert np.allclose(C.spectral_fir_corr_reference(X, G, 4, shared=True), gH.sum(0))


@pytest.mark.parametrize("K", (1, 2, 5, 6, 40, 41))
def test_mode_cuts_at_even_and_odd_taps(K):
    for L in (1, 7, 40, 41):
        g = np.random.default_rng(K * 50 + L)
        x, h = g.standard_normal((2, L)), g.standard_normal(K)
        full = C.oracle(x, h, "full")
        assert full.shape == (2, L + K - 1)
        same, valid = C.oracle(x, h, "same"), C.oracle(x, h, "valid")
        assert same.shape == (2, L) and np.array_equal(same, full[:, (K - 1) // 2:(K - 1) // 2 + L])
        lo, n = min(L, K) - 1, max(L, K) - min(L, K) + 1
        assert valid.shape == (2, n) and np.array_equal(valid, full[:, lo:lo + n])
        for mode in C.MODES:
            assert ops.fft_convolve_cut(L, K, mode) == C.cut(L, K, mode)
            if L >= K:                                                           # numpy's own modes agree where it centres alike
                assert np.allclose(C.oracle(x, h, mode)[0], np.convolve(x[0], h, mode))
    with pytest.raises(ValueError):
        ops.fft_convolve_cut(5, 3, "circular")


def test_case_table_covers_what_it_says():
    tile = C.FRAME_TILE
    frames = sorted({ops.fft_convolve_plan(L, K, C.BLOCK)[1] for L, K in C.TILE_CASES})
    assert frames == [tile - 1, tile, tile + 1, tile + 2]
    assert any(K > L for L in C.LENGTHS for K in C.TAPS) and 1 in C.LENGTHS and 1 in C.TAPS
    blocks = sorted(ops.fft_convolve_plan(L, K, b)[0] for L, K, _, b in C.BLOCK_CASES)
    assert blocks == [256, 512, 1024, 2048]
    L, K, _ = C.LONG_CASE
    assert ops.fft_convolve_plan(L, K)[0] == 2048 and ops.fft_convolve_plan(L, K)[2] > 4
    parts = {ops.fft_convolve_plan(L, K, C.BLOCK)[2] for L in C.LENGTHS for K in C.TAPS}
    assert {1, 2, 3, 8} <= parts


# ---- the C entries, without a device -----------------------------------------------------------------------------------------
def _fir(rows=0, T=0, P=1, F=129, X=64, H=128, Y=256, xs=None, hs=0, anti=0, conj=0):
    p = ctypes.c_void_p
    xs = T * F if xs is None else xs
    return _lib.lib().at_spectral_fir(p(X), xs, p(H), hs, rows, T, P, F, anti, conj, p(Y), p(0))


def _corr(rows=0, T=0, P=1, F=129, X=64, G=128, gH=256, ws=512, wsb=0, shared=1, xs=None):
    p = ctypes.c_void_p
    xs = T * F if xs is None else xs
    return _lib.lib().at_spectral_fir_corr(p(X), xs, p(G), rows, T, P, F, shared, p(gH), p(ws), wsb, p(0))


def test_c_entry_answers_that_need_no_device():
    assert _fir() == _lib.AT_OK and _fir(rows=0, T=5) == _lib.AT_OK and _fir(rows=3, T=0) == _lib.AT_OK   # nothing to do
    assert _fir(rows=-1) == _lib.AT_EINVAL and _fir(T=-1) == _lib.AT_EINVAL and _fir(P=-1) == _lib.AT_EINVAL
    assert _fir(F=0) == _lib.AT_EINVAL and _fir(anti=2) == _lib.AT_EINVAL and _fir(conj=-1) == _lib.AT_EINVAL
    assert _fir(xs=-1) == _lib.AT_EINVAL and _fir(hs=-1) == _lib.AT_EINVAL
    assert _fir(rows=2, T=5, X=0) == _lib.AT_EINVAL and _fir(rows=2, T=5, Y=0) == _lib.AT_EINVAL
    assert _fir(rows=2, T=5, H=0) == _lib.AT_EINVAL
    assert _fir(rows=2, T=5, xs=5 * 129 - 1) == _lib.AT_EINVAL and _fir(rows=2, T=5, P=3, hs=129) == _lib.AT_EINVAL
    assert _fir(rows=2, T=5, X=68) == _lib.AT_EINVAL                                 # complex64 is 8-byte aligned
    assert _corr() == _lib.AT_OK and _corr(rows=0, T=5) == _lib.AT_OK and _corr(rows=3, T=5, P=0) == _lib.AT_OK
    assert _corr(rows=-1) == _lib.AT_EINVAL and _corr(T=-1) == _lib.AT_EINVAL and _corr(shared=2) == _lib.AT_EINVAL
    assert _corr(rows=2, T=5, X=0) == _lib.AT_EINVAL and _corr(rows=2, T=5, G=0) == _lib.AT_EINVAL
    assert _corr(rows=2, T=5, gH=0) == _lib.AT_EINVAL
    need = _lib.lib().at_spectral_fir_corr_workspace_bytes
    for shared in (0, 1):
        n = need(2, 5, 3, 129, shared)
        assert n > 0 and n % 16 == 0
        assert _corr(rows=2, T=5, P=3, shared=shared, ws=0, wsb=n) == _lib.AT_EWORKSPACE
        assert _corr(rows=2, T=5, P=3, shared=shared, wsb=n - 1) == _lib.AT_EWORKSPACE
    assert need(0, 5, 3, 129, 1) == 0 and need(2, 5, 0, 129, 1) == 0
    assert need(2, 0, 3, 129, 1) == 0 and need(2, 0, 3, 129, 0) == 0                 # no frames: zeros by a memset, nothing to plan
    assert need(1, 1, 1, 1, 1) == 16 and need(10 ** 6, 1, 1, 1, 1) <= 256 * 16       # the smallest plans there are
    # per row: one group of P F complex doubles per row; shared: at most 256 groups, whatever the batch
    assert need(70, 10, 3, 129, 0) == 70 * 3 * 129 * 16
    assert need(10 ** 6, 1383, 5, 129, 1) <= 256 * 5 * 129 * 16
    assert need(1, 5, 3, 129, 1) == need(1, 5, 3, 129, 0)                            # one slice, one group


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ("at_fft_convolve_plan", "at_spectral_fir", "at_spectral_fir_corr"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _lib.exported_symbols()
    assert re.search(r"\bsize_t at_spectral_fir_corr_workspace_bytes\s*\(", hdr)
    assert "at_spectral_fir_corr_workspace_bytes" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 4
    assert "FFTConvolveFunction" in autograd.__all__ and issubclass(autograd.FFTConvolveFunction, torch.autograd.Function)
    for name in ("FFTConvolve", "Convolve", "ImpulseResponse"):
        assert name in A.transforms.__all__ and getattr(A, name) is getattr(A.transforms, name)
    assert A.convolve is A.transforms.convolve
    mk = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "Makefile")).read()
    assert re.search(r"fft_convolve\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk)


# ---- what a caller can get wrong -----------------------------------------------------------------------------------------------
def test_shape_and_mode_errors_come_before_any_device():
    x, h = torch.zeros(3, 10), torch.zeros(4)
    for bad_mode in ("circular", "", None, "FULL"):
        with pytest.raises(ValueError):
            ops.fft_convolve(x, h, bad_mode)
        with pytest.raises(ValueError):
            A.FFTConvolve(bad_mode)
        with pytest.raises(ValueError):
            A.Convolve(bad_mode)
    for bx, bh in ((torch.zeros(3, 0), h), (x, torch.zeros(0)), (torch.tensor(1.0), h), (x, torch.tensor(1.0)),
                   (x, torch.zeros(2, 4)), (torch.zeros(2, 3, 10), torch.zeros(3, 2, 4))):
        with pytest.raises(ValueError):
            ops.fft_convolve(bx, bh)
        with pytest.raises(ValueError):
            A.FFTConvolve()(bx, bh)
    with pytest.raises(ValueError):
        ops.fft_convolve(x, h, block=100)
    for bad_ir in (torch.zeros(0), torch.zeros(2, 3), 1.0):
        with pytest.raises(ValueError):
            A.ImpulseResponse(bad_ir)
    with pytest.raises(ValueError):
        A.ImpulseResponse(None, learnable=True)                                   # the pass-through has nothing to learn


def test_cpu_tensors_are_refused():
    x, h = torch.zeros(3, 10), torch.ones(4)
    with pytest.raises(A.AcidsHipError):
        ops.fft_convolve(x, h)
    with pytest.raises(A.AcidsHipError):
        ops.fft_convolve(x, torch.ones(3, 4), "same")
    for m in (A.FFTConvolve(), A.Convolve("valid")):
        with pytest.raises(A.AcidsHipError):
            m(x, h)
    with pytest.raises(A.AcidsHipError):
        A.ImpulseResponse(h)(x)
    with pytest.raises(A.AcidsHipError):
        A.ImpulseResponse(h, learnable=True)(x)
    with pytest.raises(A.AcidsHipError):
        ops.spectral_fir(torch.zeros(1, 2, 3, dtype=torch.complex64), torch.zeros(1, 3, dtype=torch.complex64))


def test_modules_on_the_host():
    ir = torch.tensor([1.0, 0.5, 0.25])
    m = A.ImpulseResponse(ir)
    assert isinstance(m, A.AudioTransform) and not m.invertible and m.taps == 3 and not m.tail and not m.learnable
    assert "ir" in dict(m.named_buffers()) and not list(m.parameters()) and torch.equal(m.ir, ir) and m.ir is not ir
    learn = A.ImpulseResponse(ir, tail=True, learnable=True, sr=48000)
    assert isinstance(learn.ir, torch.nn.Parameter) and learn.ir.requires_grad and learn.tail and learn.sr == 48000
    assert [n for n, _ in learn.named_parameters()] == ["ir"] and "ir" in learn.state_dict()
    x = torch.zeros(3, 5)
    assert A.ImpulseResponse()(x) is x                                            # no response: the pass-through
    y, time = A.ImpulseResponse().forward_with_time(x, torch.ones(3))
    assert y is x and torch.equal(time, torch.ones(3))
    with pytest.raises(A.NotInvertibleError):
        m.invert(x)
    with pytest.warns(UserWarning):
        assert m.realtime() is m
    chain = A.ImpulseResponse(ir) + A.ImpulseResponse()
    assert isinstance(chain, A.ComposeAudioTransform) and len(chain.transforms) == 2
    assert callable(m.test_forward) and callable(A.ImpulseResponse.test_scripted_transform)
    for cls in (A.FFTConvolve, A.Convolve):
        mod = cls("same")
        assert isinstance(mod, torch.nn.Module) and not isinstance(mod, A.AudioTransform) and mod.mode == "same"
        assert cls().mode == "full" and not list(mod.parameters())
    assert issubclass(A.Convolve, A.FFTConvolve)

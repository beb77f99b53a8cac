"""CPU side of SpectralDistance (csrc/spectral_distance.hip, autograd.SpectralDistanceFunction, losses.py): the float64
model of the two kernels against float64 torch autograd of the stated expression; the chunk rule; the C ABI entries
and their argument checks; and what the module does without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import spectral_distance_cases as C
from distance_driver_stub import stub_ops
from acids_transforms_amd import _lib, autograd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_spectral_distance_workspace_bytes", "at_spectral_distance_sums", "at_spectral_distance_backward")


def _hard_spectra(seed):
    """(2, 6, 65) complex128 spectra with exact-zero bins in X, in Y and in both, and a frame scaled by 1e-6 (bins of
    the size of eps, where 1 / (A + eps) is steep)."""
    X, Y = (v.astype(np.complex128) for v in C.spectra((2, 6, 65), seed))
    X[0, 2] *= 1e-6
    Y[1, 3] *= 1e-6
    return X, Y


@pytest.mark.parametrize("need_x,need_y", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.3, 2.5), (1.0, 0.0), (0.0, 1.0)])
def test_float64_model_matches_torch_autograd(need_x, need_y, weights):
    X, Y = _hard_spectra(11)
    assert (np.abs(X) == 0).any() and (np.abs(Y) == 0).any() and ((np.abs(X) == 0) & (np.abs(Y) == 0)).any()
    g = np.array([0.7, -1.3])
    sums = C.model_sums(X, Y)
    want_loss = C.torch_loss(torch.from_numpy(X), torch.from_numpy(Y), *weights).numpy()
    got_loss = C.model_loss(sums, X[0].size, *weights)
    assert np.abs(got_loss - want_loss).max() <= 1e-12 * np.abs(want_loss).max()
    GX, GY = C.model_backward(X, Y, g, *weights, need_x=need_x, need_y=need_y)
    wantX, wantY = C.autograd_backward(X, Y, g, *weights)
    assert (GX is None) == (not need_x) and (GY is None) == (not need_y)
    for got, want, src in ((GX, wantX, X), (GY, wantY, Y)):
        if got is None:
            continue
        assert np.isfinite(got).all() and np.isfinite(want).all()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.all(got[np.abs(src) == 0] == 0)


def test_chunk_rule():
    assert autograd.SPECDIST_CHUNK_ELEMS == C.CHUNK_ELEMS == 1 << 26
    assert autograd.specdist_chunk_clips(1024, 690, 1024) == 189 == C.chunk_clips(1024, 690, 1024)
    assert autograd.specdist_chunk_clips(4, 1 << 20, 1024) == 1 == C.chunk_clips(4, 1 << 20, 1024)   # one clip over budget
    assert autograd.specdist_chunk_clips(3, 690, 1024) == 3                                           # fewer clips than fit
    assert C.chunks(1024, 690, 1024) == [189] * 5 + [79]                                              # a ragged tail
    assert autograd._specdist_chunks(1024, 176400, 1024, 256)[-2:] == [(756, 945), (945, 1024)]
    for Bk, Tk, nk in [(1024, 690, 1024), (7, 345, 2048), (800, 173, 4096), (50, 1765, 400), (2, 13, 16384)]:
        assert C.chunk_clips(Bk, Tk, nk) == autograd.specdist_chunk_clips(Bk, Tk, nk)
    # two spectra of a chunk peak at 1 GiB whatever B is
    for n, hop in C.DEFAULT_SCALES:
        T = C.frames(n, hop, 176400)
        for B in (1, 100, 1024, 5000):
            assert 2 * 8 * autograd.specdist_chunk_clips(B, T, n) * T * (n // 2 + 1) <= 1 << 30
    # the 2 + 2 + 1 cut of the GPU chunk test holds at every default scale
    for n, hop in C.DEFAULT_SCALES:
        assert C.chunks(5, C.frames(n, hop, C.MODULE_L), n, elems=20000) == [2, 2, 1]
    src = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "distance_core.h")).read()
    assert re.search(r"kDistThreads = 256;", src) and re.search(r"kDistPerLane = 16;", src) and C.SLICE == 256 * 16
    assert re.search(r"kDistSlice = kDistThreads \* kDistPerLane;", src)
    assert [C.slices(T * F) for _, T, F in C.OP_SHAPES] == [1, 1, 3, 87]


def test_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert re.search(r"\b(int|size_t) %s\s*\(" % name, hdr)
    assert lib.at_abi_version() == 4                            # additive: the ABI version stays
    assert "spectral_distance_sums" in dir(A.ops) and "spectral_distance_backward" in dir(A.ops)


def test_argument_checks_answer_before_any_launch():
    lib = _lib.lib()
    E, OK = _lib.AT_EINVAL, _lib.AT_OK
    wsb = lib.at_spectral_distance_workspace_bytes
    assert wsb(2, 65) == 2 * 3 * 4 and wsb(3, 4096) == 3 * 3 * 4 and wsb(3, 4097) == 3 * 2 * 3 * 4
    assert wsb(0, 65) == 0 and wsb(2, 0) == 0
    sums = lib.at_spectral_distance_sums
    assert sums(None, 8, 2, 65, C.EPS, 8, 8, 64, None) == E          # null X
    assert sums(8, None, 2, 65, C.EPS, 8, 8, 64, None) == E          # null Y
    assert sums(8, 8, 2, 65, C.EPS, None, 8, 64, None) == E          # null sums
    assert sums(8, 8, -1, 65, C.EPS, 8, 8, 64, None) == E            # B < 0
    assert sums(8, 8, 2, 0, C.EPS, 8, 8, 64, None) == E              # n < 1
    assert sums(8, 8, 2, 65, -1.0, 8, 8, 64, None) == E              # eps < 0
    assert sums(12, 8, 2, 65, C.EPS, 8, 8, 64, None) == E            # a spectrum off its 8-byte grid
    assert sums(8, 8, 2, 65, C.EPS, 8, 8, 23, None) == _lib.AT_EWORKSPACE
    assert sums(8, 8, 2, 65, C.EPS, 8, None, 64, None) == _lib.AT_EWORKSPACE
    assert sums(None, None, 0, 65, C.EPS, None, None, 0, None) == OK
    bwd = lib.at_spectral_distance_backward
    assert bwd(None, 8, 2, 65, 8, 8, 1.0, 1.0, C.EPS, 1, 0, None) == E
    assert bwd(8, None, 2, 65, 8, 8, 1.0, 1.0, C.EPS, 1, 0, None) == E
    assert bwd(8, 8, 2, 65, None, 8, 1.0, 1.0, C.EPS, 1, 0, None) == E
    assert bwd(8, 8, 2, 65, 8, None, 1.0, 1.0, C.EPS, 1, 0, None) == E
    assert bwd(8, 8, -1, 65, 8, 8, 1.0, 1.0, C.EPS, 1, 0, None) == E
    assert bwd(8, 8, 2, 0, 8, 8, 1.0, 1.0, C.EPS, 1, 0, None) == E
    assert bwd(8, 8, 2, 65, 8, 8, 1.0, 1.0, -1.0, 1, 0, None) == E
    assert bwd(8, 8, 2, 65, 8, 8, 1.0, 1.0, C.EPS, 0, 0, None) == E   # nothing asked for
    assert bwd(None, None, 0, 65, None, None, 1.0, 1.0, C.EPS, 1, 1, None) == OK


def test_module_on_the_cpu():
    crit = A.SpectralDistance()
    assert A.losses.SpectralDistance is A.SpectralDistance and isinstance(crit, torch.nn.Module)
    assert not isinstance(crit, A.base.AudioTransform)
    assert crit.scales == C.DEFAULT_SCALES and crit.reduction == "mean" and crit.eps == C.EPS
    bufs = dict(crit.named_buffers())
    assert len(bufs) == 5                                        # one window per scale
    for i, (n, _) in enumerate(crit.scales):
        assert torch.equal(bufs["window_%d" % i], torch.hann_window(n))     # periodic, as STFT's
    crit = A.SpectralDistance(scales=C.SCALES, lin_weight=0.5, log_weight=2.0, reduction="none")
    assert len(list(crit.buffers())) == 7 and crit.window_5.shape == (400,)
    for x in (torch.zeros(2, 4096), torch.zeros(2, 4096, requires_grad=True)):      # no CPU route, graph or not
        with pytest.raises(A.AcidsHipError):
            crit(x, torch.zeros(2, 4096))
    with pytest.raises(A.AcidsHipError):
        crit(torch.zeros(2, 4096, dtype=torch.float64), torch.zeros(2, 4096, dtype=torch.float64))
    with pytest.raises(A.AcidsHipError):
        A.ops.spectral_distance_sums(torch.zeros(2, 3, 65, dtype=torch.complex64), torch.zeros(2, 3, 65, dtype=torch.complex64))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4096), torch.zeros(3, 4096))         # mismatched shapes
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4096), torch.zeros(2, 4095))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1024), torch.zeros(2, 1024))         # L <= max n_fft // 2: no reflect padding
    with pytest.raises(ValueError):
        A.SpectralDistance(reduction="median")
    with pytest.raises(ValueError):
        A.SpectralDistance(window="nope")


def test_autograd_surface():
    assert "SpectralDistanceFunction" in autograd.__all__ and "specdist_chunk_clips" in autograd.__all__
    assert issubclass(autograd.SpectralDistanceFunction, torch.autograd.Function)


def test_module_surface_is_unchanged():
    """state_dict keys, repr and every constructor and call message, as literals."""
    crit = A.SpectralDistance()
    assert list(crit.state_dict().keys()) == ["window_0", "window_1", "window_2", "window_3", "window_4"]
    assert repr(crit) == ("SpectralDistance(scales=((2048, 512), (1024, 256), (512, 128), (256, 64), (128, 32)), "
                          "lin_weight=1, log_weight=1, reduction=mean)")
    for kw, msg in ((dict(window="nope"), "Window nope is not known"),
                    (dict(reduction="median"), "reduction median not known (none, sum, mean)"),
                    (dict(scales=()), "at least one (n_fft, hop) scale is needed"),
                    (dict(scales=((1, 1),)), "scale (1, 1): n_fft must lie in 2 .. 16384 and hop be positive"),
                    (dict(scales=((1024, 0),)), "scale (1024, 0): n_fft must lie in 2 .. 16384 and hop be positive"),
                    (dict(eps=-1.0), "eps must not be negative"),
                    (dict(window="nope", reduction="median", scales=()), "Window nope is not known"),     # the order
                    (dict(reduction="median", scales=()), "reduction median not known (none, sum, mean)")):
        with pytest.raises(ValueError) as e:
            A.SpectralDistance(**kw)
        assert str(e.value) == msg
    with pytest.raises(ValueError):
        A.SpectralDistance(scales=((1024, 256, 80),))           # a scale is a pair: the unpacking's own error
    for a, b, msg in ((torch.zeros(2, 4096), torch.zeros(3, 4096), "x and y must have one shape, got (2, 4096) and (3, 4096)"),
                      (torch.zeros(2, 1024), torch.zeros(2, 1024),
                       "clips of 1024 samples are too short for n_fft 2048 (reflect padding needs more than n_fft // 2)"),
                      (torch.zeros(()), torch.zeros(()),
                       "clips of 0 samples are too short for n_fft 2048 (reflect padding needs more than n_fft // 2)")):
        with pytest.raises(ValueError) as e:
            crit(a, b)
        assert str(e.value) == msg


def test_chunk_constants_are_read_at_the_call(monkeypatch):
    assert autograd.mfcc_chunk_clips(5, 33, 128) == 5 == autograd.specdist_chunk_clips(5, 33, 128)
    monkeypatch.setattr(autograd, "SPECDIST_CHUNK_ELEMS", 2 * 33 * 65)
    assert autograd.specdist_chunk_clips(5, 33, 128) == 2 and autograd.mfcc_chunk_clips(5, 33, 128) == 5
    assert autograd._specdist_chunks(5, 1024, 128, 32) == [(0, 2), (2, 4), (4, 5)]
    monkeypatch.setattr(autograd, "MFCC_CHUNK_ELEMS", 3 * 33 * 65 + 1)
    assert autograd.specdist_chunk_clips(5, 33, 128) == 2 and autograd.mfcc_chunk_clips(5, 33, 128) == 3
    assert autograd._chunk_clips(33 * 65 - 1, 5, 33, 128) == 1          # one clip over the budget: a chunk of one


@pytest.mark.parametrize("need", [(True, False), (False, True), (True, True)])
def test_function_goes_through_the_shared_driver(monkeypatch, need):
    """With ops stubbed: the sums driver and the backward helper are the shared ones, the chunks follow the patched
    constant, and the first scale writes into the result while later scales go through the scratch and are added."""
    log = stub_ops(monkeypatch, autograd)
    scales = ((128, 32), (64, 32), (64, 64))
    B, L = 5, 1024
    monkeypatch.setattr(autograd, "SPECDIST_CHUNK_ELEMS", 2 * C.bins(128, 32, L))       # 2, 3 and 5 clips per chunk
    cuts = [C.chunks(B, C.frames(n, h, L), n, elems=2 * C.bins(128, 32, L)) for n, h in scales]
    assert cuts == [[2, 2, 1], [3, 2], [5]]
    x, y = (torch.zeros(B, L, requires_grad=nd) for nd in need)
    windows = tuple(torch.hann_window(n) for n, _ in scales)
    loss = autograd.SpectralDistanceFunction.apply(x, y, windows, scales, 0.5, 2.0, C.EPS)
    want = 0.5 * 3 * (1.0 / 2.0) + 2.0 * sum(3.0 / C.bins(n, h, L) for n, h in scales)
    assert loss.shape == (B,) and loss.dtype == torch.float32 and torch.allclose(loss, torch.full((B,), want))
    assert [e[0] for e in log].count("_dist_sums") == 1 and ("_DistBackward", None) not in log
    assert [e[1] for e in log if e[0] == "spectral_distance_sums"] == [(c, C.frames(n, h, L), n // 2 + 1)
                                                                      for (n, h), cut in zip(scales, cuts) for c in cut]
    del log[:]
    loss.sum().backward()
    assert [e[0] for e in log].count("_DistBackward") == 1
    assert [e[1] for e in log if e[0] == "stft_forward"] == [(c, n, h) for (n, h), cut in zip(scales, cuts) for c in cut
                                                            for _ in (0, 1)]
    assert [e[1] for e in log if e[0] == "spectral_distance_backward"] == [(c, need[1]) for cut in cuts for c in cut]
    for t, nd in zip((x, y), need):
        assert (t.grad is None) == (not nd)
        if nd:
            assert torch.equal(t.grad, torch.full((B, L), 128.0 + 64.0 + 64.0))        # written once, added twice
    outs = [e[1] for e in log if e[0] == "stft_backward"]
    first, later = [o for o in outs if o[1] == 128], [o for o in outs if o[1] != 128]
    assert len(first) == 3 * sum(need) and len(later) == 3 * sum(need)
    assert len({o[2] for o in later}) == 1 and not {o[2] for o in later} & {o[2] for o in first}      # one scratch

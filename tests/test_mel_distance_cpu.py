"""CPU side of MelSpectralDistance (csrc/mel_distance.hip, autograd.MelSpectralDistanceFunction, losses.py): the float64
model of the three kernels against float64 torch autograd of the stated expression; the case tables and the plan rule;
the C ABI entries and their argument checks; and what the module does without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import mel_distance_cases as C
from distance_driver_stub import stub_ops
from acids_transforms_amd import _lib, autograd
from acids_transforms_amd.utils.banded import bank_columns
from acids_transforms_amd.utils.melbank import melscale_fbanks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_mel_rows", "at_mel_distance_workspace_bytes", "at_mel_distance_sums", "at_mel_distance_backward")


def _hard_spectra(seed):
    """(2, 6, 65) complex128 spectra with exact-zero bins in X, in Y and in both, a frame that X and Y share, and a
    frame scaled by 1e-6 in each (mel cells of the size of eps, where 1 / (M + eps) is steep)."""
    X, Y = (v.astype(np.complex128) for v in C.spectra((2, 6, 65), seed))
    X[0, 2] *= 1e-6
    Y[1, 4] *= 1e-6
    return X, Y


@pytest.mark.parametrize("need_x,need_y", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.3, 2.5), (1.0, 0.0), (0.0, 1.0)])
def test_float64_model_matches_torch_autograd(need_x, need_y, weights):
    X, Y = _hard_spectra(11)
    W = C.bank(65, 20)
    assert C.empty_filters(W) == 1
    assert (np.abs(X) == 0).any() and (np.abs(Y) == 0).any() and ((np.abs(X) == 0) & (np.abs(Y) == 0)).any()
    assert np.array_equal(X[-1, 3], Y[-1, 3])                         # the shared frame
    g = np.array([0.7, -1.3])
    M, Q = C.model_mel_rows(X, W), C.model_mel_rows(Y, W)
    sums = C.model_sums(M, Q)
    want_loss = C.torch_loss(torch.from_numpy(X), torch.from_numpy(Y), W, *weights).numpy()
    got_loss = C.model_loss(sums, M[0].size, *weights)
    assert np.abs(got_loss - want_loss).max() <= 1e-12 * np.abs(want_loss).max()
    GX, GY = C.model_gradients(X, Y, W, g, *weights, need_x=need_x, need_y=need_y)
    wantX, wantY = C.autograd_backward(X, Y, W, g, *weights)
    assert (GX is None) == (not need_x) and (GY is None) == (not need_y)
    for got, want, src in ((GX, wantX, X), (GY, wantY, Y)):
        if got is None:
            continue
        assert np.isfinite(got).all() and np.isfinite(want).all()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.all(got[np.abs(src) == 0] == 0)
        assert np.all(got[..., 0] == 0) and np.all(got[..., -1] == 0)     # DC and Nyquist: empty bank rows


def test_case_tables_and_plan_rule():
    csrc = os.path.join(ROOT, "acids_transforms_amd", "csrc")
    src = open(os.path.join(csrc, "mel_distance.hip")).read()
    sd = open(os.path.join(csrc, "spectral_distance.hip")).read()
    core = open(os.path.join(csrc, "distance_core.h")).read()
    assert re.search(r"kDistThreads = 256;", core) and re.search(r"kDistPerLane = 16;", core) and C.SLICE == 256 * 16
    assert '#include "distance_core.h"' in src and '#include "band_cols.h"' in src and '#include "distance_core.h"' in sd
    # stated once, in the shared header; both files go through its launcher and its constants
    for name in ("sd_block_fold", "sd_clip_sums_kernel", "dist_slice_sums_kernel", "dist_consts", "dist_d_generated",
                 "dist_d_target"):
        assert re.search(r"(void|float) %s\(" % name, core)
        assert not re.search(r"(void|float) %s\(" % name, sd) and not re.search(r"(void|float) %s\(" % name, src)
    for name in ("dist_sums(", "dist_workspace_bytes(", "dist_consts(", "dist_d_generated(", "dist_d_target(", "dist_bin_grad("):
        assert name in sd and name in src
    assert not re.search(r"k(Sd|Md)(Threads|PerLane|Slice)", sd + src)       # no slice geometry of their own
    # the default ladder's empty filters, and DC / Nyquist rows empty at every scale of the sweep
    assert tuple(C.empty_filters(C.bank(n // 2 + 1, m)) for n, _, m in C.DEFAULT_SCALES) == C.DEFAULT_EMPTY
    for n, _, m in C.SCALES:
        W = C.bank(n // 2 + 1, m)
        assert not W[0].any() and not W[-1].any()
    # the op-level shapes reach every plan
    got = []
    for (B, T, F, N), empty in zip(C.OP_SHAPES, C.OP_EMPTY):
        W = C.bank(F, N)
        assert C.empty_filters(W) == empty and not W[0].any() and not W[-1].any()
        rows_plan, bwd_plan = C.bank_plans(W)
        assert rows_plan[0] == bwd_plan[0] and rows_plan[3] == bwd_plan[3] == (F <= 576)
        got.append((bwd_plan[0], bwd_plan[3]))
    assert set(got) == {("lds", True), ("lds", False), ("global_w4", False)}
    W = C.bank(8193, 320)
    f_nnz, t_nnz = bank_columns(W)[3].size, bank_columns(W.t())[3].size
    assert 3 * (8193 + 320) + f_nnz + t_nnz == C.OP_TABLE_FLOATS_8193 and 4 * C.OP_TABLE_FLOATS_8193 > C.LDS_BUDGET
    assert C.bank_plans(W)[1] == ("global_w4", 4, 4 * 4 * (8256 + 320), False)
    # the many-rows case: three trips of the row loop, the last with only some workgroups, on 256 CUs and on fewer
    for cus in (256, 304, 64):
        B, T, F, N = C.many_rows_shape(cus)
        for p in C.bank_plans(C.bank(F, N)):
            n_trips, last = C.trips(B * T, p, cus)
            assert n_trips == 3 and 0 < last < 8 * cus
    # slices: one, and two with a short last one
    assert [C.slices(T * N) for _, T, _, N in C.OP_SHAPES] == [1, 1, 1, 1, 1, 1, 2] and 130 * 40 % C.SLICE == 1104
    # every chunk of the module's sweep under the 2 + 2 + 1 cut of the GPU chunk test
    for n, hop, _ in C.DEFAULT_SCALES:
        assert C.SD.chunks(5, C.frames(n, hop, C.MODULE_L), n, elems=20000) == [2, 2, 1]


def test_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert re.search(r"\b(int|size_t) %s\s*\(" % name, hdr)
    assert lib.at_abi_version() == 4                            # additive: the ABI version stays
    for op in ("mel_rows", "mel_distance_sums", "mel_distance_backward"):
        assert op in dir(A.ops)


def test_argument_checks_answer_before_any_launch():
    lib = _lib.lib()
    E, OK, WS = _lib.AT_EINVAL, _lib.AT_OK, _lib.AT_EWORKSPACE
    rows = lib.at_mel_rows
    assert rows(None, 2, 65, 20, 8, 8, 8, 8, 5, 8, None) == E          # null X
    assert rows(8, 2, 65, 20, 8, 8, 8, 8, 5, None, None) == E          # null out
    for k in range(4):                                                  # a null table
        cols = [8, 8, 8, 8]
        cols[k] = None
        assert rows(8, 2, 65, 20, *cols, 5, 8, None) == E
    assert rows(8, 2, 65, 20, 8, 8, 8, 8, 0, 8, None) == E             # no weights
    assert rows(8, -1, 65, 20, 8, 8, 8, 8, 5, 8, None) == E            # rows < 0
    assert rows(8, 2, 0, 20, 8, 8, 8, 8, 5, 8, None) == E              # K < 1
    assert rows(8, 2, 65, 0, 8, 8, 8, 8, 5, 8, None) == E              # N < 1
    assert rows(12, 2, 65, 20, 8, 8, 8, 8, 5, 8, None) == E            # a spectrum off its 8-byte grid
    assert rows(8, 2, 1 << 20, 20, 8, 8, 8, 8, 5, 8, None) == _lib.AT_EUNSUPPORTED     # one row over the LDS budget
    assert rows(None, 0, 65, 20, None, None, None, None, 0, None, None) == OK

    wsb = lib.at_mel_distance_workspace_bytes
    assert wsb(2, 20) == 2 * 3 * 4 and wsb(3, 4096) == 3 * 3 * 4 and wsb(3, 4097) == 3 * 2 * 3 * 4
    assert wsb(0, 20) == 0 and wsb(2, 0) == 0
    sums = lib.at_mel_distance_sums
    assert sums(None, 8, 2, 20, C.EPS, 8, 8, 64, None) == E          # null M
    assert sums(8, None, 2, 20, C.EPS, 8, 8, 64, None) == E          # null Q
    assert sums(8, 8, 2, 20, C.EPS, None, 8, 64, None) == E          # null sums
    assert sums(8, 8, -1, 20, C.EPS, 8, 8, 64, None) == E            # B < 0
    assert sums(8, 8, 2, 0, C.EPS, 8, 8, 64, None) == E              # n < 1
    assert sums(8, 8, 2, 20, -1.0, 8, 8, 64, None) == E              # eps < 0
    assert sums(8, 8, 2, 20, float("nan"), 8, 8, 64, None) == E
    assert sums(8, 8, 2, 20, C.EPS, 8, 8, 23, None) == WS            # a short workspace
    assert sums(8, 8, 2, 20, C.EPS, 8, None, 64, None) == WS         # none
    assert sums(8, 8, 2, 20, C.EPS, 8, 6, 64, None) == WS            # off its 4-byte grid
    assert sums(None, None, 0, 20, C.EPS, None, None, 0, None) == OK

    bwd = lib.at_mel_distance_backward
    good = dict(S=8, O=8, B=2, T=3, K=65, N=20, f=[8, 8, 8, 8, 5], t=[8, 8, 8, 8, 5], sums=8, g=8, lin=1.0, log=1.0,
                eps=C.EPS, side=0)

    def call(**kw):
        a = dict(good, **kw)
        return bwd(a["S"], a["O"], a["B"], a["T"], a["K"], a["N"], *a["f"], *a["t"], a["sums"], a["g"], a["lin"], a["log"],
                   a["eps"], a["side"], None)
    for name in ("S", "O", "sums", "g"):
        assert call(**{name: None}) == E
    for which in ("f", "t"):
        for k in range(4):
            cols = [8, 8, 8, 8, 5]
            cols[k] = None
            assert call(**{which: cols}) == E
        assert call(**{which: [8, 8, 8, 8, 0]}) == E
    assert call(B=-1) == E and call(T=0) == E and call(K=0) == E and call(N=0) == E
    assert call(eps=-1.0) == E
    assert call(S=12) == E                                              # a spectrum off its 8-byte grid
    assert call(side=2) == E and call(side=-1) == E
    assert call(K=1 << 20) == _lib.AT_EUNSUPPORTED
    assert call(B=0, S=None, O=None, sums=None, g=None) == OK


def test_module_on_the_cpu():
    crit = A.MelSpectralDistance()
    assert A.losses.MelSpectralDistance is A.MelSpectralDistance and isinstance(crit, torch.nn.Module)
    assert not isinstance(crit, A.base.AudioTransform)
    assert crit.scales == C.DEFAULT_SCALES and crit.reduction == "mean" and crit.eps == C.EPS
    assert crit.sr == 44100 and crit.f_min == 0.0 and crit.f_max == 22050.0
    assert crit.lin_weight == 1.0 and crit.log_weight == 1.0
    bufs = dict(crit.named_buffers())
    assert len(bufs) == 10                                       # one window and one bank per scale
    for i, (n, _, m) in enumerate(crit.scales):
        assert torch.equal(bufs["window_%d" % i], torch.hann_window(n))     # periodic, as STFT's
        W = bufs["mel_bank_%d" % i]
        assert W.shape == (n // 2 + 1, m) and W.dtype == torch.float32
        assert torch.equal(W, melscale_fbanks(n // 2 + 1, 0.0, 22050.0, m, 44100))
        assert C.empty_filters(W) == C.DEFAULT_EMPTY[i]
    crit = A.MelSpectralDistance(scales=C.SCALES, sr=16000, f_min=50.0, f_max=7000.0, lin_weight=0.5, log_weight=2.0,
                                 reduction="none")
    assert len(list(crit.buffers())) == 14 and crit.window_5.shape == (400,) and crit.mel_bank_6.shape == (513, 128)
    assert torch.equal(crit.mel_bank_5, melscale_fbanks(201, 50.0, 7000.0, 40, 16000))
    for x in (torch.zeros(2, 4096), torch.zeros(2, 4096, requires_grad=True)):      # no CPU route, graph or not
        with pytest.raises(A.AcidsHipError):
            crit(x, torch.zeros(2, 4096))
    with pytest.raises(A.AcidsHipError):
        crit(torch.zeros(2, 4096, dtype=torch.float64), torch.zeros(2, 4096, dtype=torch.float64))
    with pytest.raises(A.AcidsHipError):
        A.ops.mel_rows(torch.zeros(2, 3, 65, dtype=torch.complex64),
                       tuple(torch.from_numpy(a) for a in bank_columns(C.bank(65, 20))))
    with pytest.raises(A.AcidsHipError):
        A.ops.mel_distance_sums(torch.zeros(2, 3, 20), torch.zeros(2, 3, 20))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4096), torch.zeros(3, 4096))         # mismatched shapes
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 4096), torch.zeros(2, 4095))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1024), torch.zeros(2, 1024))         # L <= max n_fft // 2: no reflect padding
    with pytest.raises(ValueError):
        A.MelSpectralDistance(reduction="median")
    with pytest.raises(ValueError):
        A.MelSpectralDistance(window="nope")
    with pytest.raises(ValueError):
        A.MelSpectralDistance(scales=((1024, 256, 0),))          # n_mels < 1
    with pytest.raises(ValueError):
        A.MelSpectralDistance(scales=())


def test_autograd_surface():
    for name in ("MelSpectralDistanceFunction", "meldist_sums", "meldist_loss"):
        assert name in autograd.__all__ and hasattr(autograd, name)
    assert issubclass(autograd.MelSpectralDistanceFunction, torch.autograd.Function)
    sums = torch.tensor([[[2.0, 4.0, 6.0], [1.0, 2.0, 3.0]]], dtype=torch.float64)
    scales = ((128, 32, 20), (256, 64, 40))
    want = 0.5 * (2.0 / 4.0 + 1.0 / 2.0) + 2.0 * (6.0 / (129 * 20) + 3.0 / (65 * 40))
    got = autograd.meldist_loss(sums, 4096, scales, 0.5, 2.0)
    assert got.dtype == torch.float32 and abs(float(got[0]) - want) < 1e-6 * want


def test_module_surface_is_unchanged():
    """state_dict keys, repr and every constructor and call message, as literals."""
    crit = A.MelSpectralDistance()
    assert list(crit.state_dict().keys()) == ["window_0", "mel_bank_0", "window_1", "mel_bank_1", "window_2", "mel_bank_2",
                                              "window_3", "mel_bank_3", "window_4", "mel_bank_4"]
    assert repr(crit) == ("MelSpectralDistance(scales=((2048, 512, 320), (1024, 256, 160), (512, 128, 80), (256, 64, 40), "
                          "(128, 32, 20)), sr=44100, lin_weight=1, log_weight=1, reduction=mean)")
    for kw, msg in ((dict(window="nope"), "Window nope is not known"),
                    (dict(reduction="median"), "reduction median not known (none, sum, mean)"),
                    (dict(scales=()), "at least one (n_fft, hop, n_mels) scale is needed"),
                    (dict(scales=((1, 1, 4),)), "scale (1, 1, 4): n_fft must lie in 2 .. 16384 and hop be positive"),
                    (dict(scales=((1024, 0, 4),)), "scale (1024, 0, 4): n_fft must lie in 2 .. 16384 and hop be positive"),
                    (dict(scales=((1024, 256, 0),)), "scale (1024, 256, 0): n_mels must be at least 1"),
                    (dict(scales=((1024, 256, 4), (1, 1, 0))), "scale (1, 1, 0): n_fft must lie in 2 .. 16384 and hop be positive"),
                    (dict(eps=-1.0), "eps must not be negative"),
                    (dict(window="nope", reduction="median", scales=()), "Window nope is not known"),     # the order
                    (dict(scales=((1024, 256, 0),), eps=-1.0), "scale (1024, 256, 0): n_mels must be at least 1")):
        with pytest.raises(ValueError) as e:
            A.MelSpectralDistance(**kw)
        assert str(e.value) == msg
    with pytest.raises(ValueError):
        A.MelSpectralDistance(scales=((1024, 256),))             # a scale is a triple: the unpacking's own error
    for a, b, msg in ((torch.zeros(2, 4096), torch.zeros(3, 4096), "x and y must have one shape, got (2, 4096) and (3, 4096)"),
                      (torch.zeros(2, 1024), torch.zeros(2, 1024),
                       "clips of 1024 samples are too short for n_fft 2048 (reflect padding needs more than n_fft // 2)"),
                      (torch.zeros(()), torch.zeros(()),
                       "clips of 0 samples are too short for n_fft 2048 (reflect padding needs more than n_fft // 2)")):
        with pytest.raises(ValueError) as e:
            crit(a, b)
        assert str(e.value) == msg


@pytest.mark.parametrize("need", [(True, False), (False, True), (True, True)])
def test_function_goes_through_the_shared_driver(monkeypatch, need):
    """With ops stubbed: the sums driver and the backward helper are SpectralDistanceFunction's, the chunks follow the
    patched constant, one spectrum is built per mel_rows call, and only the sides that need a gradient run."""
    log = stub_ops(monkeypatch, autograd)
    scales = ((128, 32, 20), (64, 32, 8), (64, 64, 40))
    B, L = 5, 1024
    elems = 2 * C.SD.bins(128, 32, L)
    monkeypatch.setattr(autograd, "SPECDIST_CHUNK_ELEMS", elems)                        # 2, 3 and 5 clips per chunk
    monkeypatch.setattr(autograd, "MFCC_CHUNK_ELEMS", 1)                                # not this one
    cuts = [C.SD.chunks(B, C.frames(n, h, L), n, elems=elems) for n, h, _ in scales]
    assert cuts == [[2, 2, 1], [3, 2], [5]]
    x, y = (torch.zeros(B, L, requires_grad=nd) for nd in need)
    windows = tuple(torch.hann_window(n) for n, _, _ in scales)
    tables = tuple(((torch.zeros(m, dtype=torch.int32),) * 4,) * 2 for _, _, m in scales)
    loss = autograd.MelSpectralDistanceFunction.apply(x, y, windows, scales, tables, 0.5, 2.0, C.EPS)
    want = 0.5 * 3 * (1.0 / 2.0) + 2.0 * sum(3.0 / (C.frames(n, h, L) * m) for n, h, m in scales)
    assert loss.shape == (B,) and loss.dtype == torch.float32 and torch.allclose(loss, torch.full((B,), want))
    assert [e[0] for e in log].count("_dist_sums") == 1 and ("_DistBackward", None) not in log
    assert [e[1] for e in log if e[0] == "mel_distance_sums"] == [(c, C.frames(n, h, L), m)
                                                                 for (n, h, m), cut in zip(scales, cuts) for c in cut]
    names = [e[0] for e in log if e[0] in ("stft_forward", "mel_rows", "mel_distance_sums")]
    assert names == ["stft_forward", "mel_rows", "stft_forward", "mel_rows", "mel_distance_sums"] * 6
    del log[:]
    loss.sum().backward()
    assert [e[0] for e in log].count("_DistBackward") == 1
    sides = [s for s in (0, 1) if need[s]]
    assert [e[1] for e in log if e[0] == "mel_distance_backward"] == [(c, s) for cut in cuts for c in cut for s in sides]
    per_side = ["stft_forward", "mel_rows", "stft_forward", "mel_distance_backward", "stft_backward"]
    assert [e[0] for e in log if e[0] != "_DistBackward"] == per_side * (6 * len(sides))
    for t, nd in zip((x, y), need):
        assert (t.grad is None) == (not nd)
        if nd:
            assert torch.equal(t.grad, torch.full((B, L), 128.0 + 64.0 + 64.0))        # written once, added twice
    outs = [e[1] for e in log if e[0] == "stft_backward"]
    later = {o[2] for o in outs if o[1] != 128}
    assert len(later) == 1 and not later & {o[2] for o in outs if o[1] == 128}          # one scratch

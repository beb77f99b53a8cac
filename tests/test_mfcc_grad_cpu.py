"""CPU side of the MFCC backward (at_mfcc_backward, autograd.MfccFunction): the two formulas the kernel implements,
restated in float64 and checked against torch autograd; the dispatch, tile and chunk restatements of
mfcc_grad_cases.py; the coverage of the GPU sweep; and the C ABI entry."""
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import mfcc_grad_cases as C
from acids_transforms_amd import _lib, autograd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_backward(X, dF, fbank, power, dct=None, scale=None):
    """What at_mfcc_backward computes, in float64.  X (T, K) complex, dF (C, T), fbank (K, N), dct (N, C)."""
    a = np.abs(X) ** power                                       # (T, K)
    g = dF.T / (scale if scale is not None else 1.0)             # (T, C)
    if dct is None:
        dM = g
    else:
        M = a @ fbank
        dlnM = g @ dct.T                                         # (T, N)
        dM = np.where(M >= 1e-10, dlnM / np.where(M >= 1e-10, M, 1.0), 0.0)
    dA = dM @ fbank.T                                            # (T, K)
    if power == 2:
        return 2.0 * dA[..., None] * np.stack([X.real, X.imag], -1)
    mag = np.abs(X)
    r = np.where(mag > 0, dA / np.where(mag > 0, mag, 1.0), 0.0)
    return r[..., None] * np.stack([X.real, X.imag], -1)


def autograd_backward(X, dF, fbank, power, dct=None, offset=0.0, scale=None):
    """torch autograd of the forward's expression from the spectrum on, in float64."""
    Xt = torch.from_numpy(X).requires_grad_()
    M = torch.matmul(Xt.abs() ** power, torch.from_numpy(fbank)).transpose(-1, -2)           # (N, T)
    if dct is not None:
        db = 10.0 * torch.log10(torch.clamp(M, min=1e-10)).transpose(-1, -2)
        M = torch.matmul(db, torch.from_numpy(dct) * (np.log(10.0) / 10.0)).transpose(-1, -2)  # dct carries 10 / ln 10
    if scale is not None:
        M = (M - offset) / scale
    M.backward(torch.from_numpy(dF))
    return torch.view_as_real(Xt.grad).numpy()


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("with_dct", [False, True])
@pytest.mark.parametrize("scale", [None, 0.37])
def test_float64_model_matches_torch_autograd(power, with_dct, scale):
    rng = np.random.default_rng(power * 7 + with_dct * 3 + (scale is not None))
    T, n_mels = 6, 128
    mod = A.MFCC(n_mels=n_mels, power=power, n_mfcc=40 if with_dct else None)
    fbank = mod.fbank.double().numpy()
    assert int((fbank.sum(0) == 0).sum()) == 1                   # the empty filter of the 128-mel bank at 1024
    dct = mod.dct.double().numpy() if with_dct else None
    X = rng.standard_normal((T, 513)) + 1j * rng.standard_normal((T, 513))
    X[0, :40] = 0.0                                              # exact-zero bins
    X[2] = 0.0                                                   # a silent frame: every M below the clamp
    X[3] *= 1e-7                                                 # power 2: M ~ 1e-14 .. 1e-12, on both sides of the clamp
    C_out = 40 if with_dct else n_mels
    dF = rng.standard_normal((C_out, T))
    got = model_backward(X, dF, fbank, power, dct, scale)
    want = autograd_backward(X, dF, fbank, power, dct, 0.11, scale)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(got[0, :40] == 0) and np.all(got[2] == 0)


def test_chunk_and_tile_restatement():
    assert C.chunk_clips(1024, 690, 1024) == 189 == autograd.mfcc_chunk_clips(1024, 690, 1024)
    n, h, L, B = C.BENCH
    T = C.frames(n, h, L)
    assert T == 690
    chunk = C.chunk_clips(B, T, n)
    assert (B // chunk, B % chunk) == (5, 79)                    # 5 x 189 + 79
    assert chunk * T * (n // 2 + 1) <= C.CHUNK_ELEMS < (chunk + 1) * T * (n // 2 + 1)
    for k in (1, 5):                                             # both sides of the first and the last chunk boundary
        assert k * chunk - 1 in C.BENCH_CLIPS and k * chunk in C.BENCH_CLIPS
    assert 0 in C.BENCH_CLIPS and B - 1 in C.BENCH_CLIPS
    # one clip's spectrum beyond the chunk: a chunk of one; fewer clips than a chunk: all of them
    assert C.chunk_clips(4, 1 << 20, 1024) == 1 == autograd.mfcc_chunk_clips(4, 1 << 20, 1024)
    assert C.chunk_clips(3, 690, 1024) == 3 == autograd.mfcc_chunk_clips(3, 690, 1024)
    for Bk, Tk, nk in [(1024, 690, 1024), (7, 345, 2048), (800, 173, 4096), (50, 1765, 400), (2, 13, 16384)]:
        assert C.chunk_clips(Bk, Tk, nk) == autograd.mfcc_chunk_clips(Bk, Tk, nk)
    assert autograd.MFCC_CHUNK_ELEMS == C.CHUNK_ELEMS
    assert C.tiles(690) == (22, 18) and C.tiles(64) == (2, 32) and C.tiles(1) == (1, 1) and C.tiles(33) == (2, 1)
    csrc = os.path.join(ROOT, "acids_transforms_amd", "csrc")
    assert re.search(r"kMfccTile = %d;" % C.TILE, open(os.path.join(csrc, "mfcc_grad.hip")).read())
    assert re.search(r"kBandLdsBudget = 160 \* 1024;", open(os.path.join(csrc, "band_plan.h")).read())


def _sweep():
    out = []
    for case in C.SIZES:
        for n_mfcc in C.n_mfcc_of(case[3]):
            mod = C.module_of(case, n_mfcc=n_mfcc)
            for shape in C.shapes_of(case):
                out.append((case[0], n_mfcc, shape, C.module_class(mod), C.forward_path(mod, shape[-1]),
                            C.frames(case[1], case[2], shape[-1])))
    return out


def test_sweep_reaches_every_kernel_class_and_forward_path():
    sweep = _sweep()
    classes = {s[3] for s in sweep}
    assert C.KERNEL_CLASSES <= classes, sorted(C.KERNEL_CLASSES - classes)
    assert "unsupported" not in classes
    paths = {s[4] for s in sweep}
    assert C.FORWARD_PATHS <= paths, sorted(C.FORWARD_PATHS - paths)
    # frame counts: below a tile, a multiple of the tile, several tiles with a short last one
    Ts = {s[5] for s in sweep}
    assert any(T < C.TILE for T in Ts) and any(T % C.TILE == 0 for T in Ts)
    assert any(T > C.TILE and T % C.TILE != 0 for T in Ts)
    # the issue's sizes
    sizes = {(c[1], c[2], c[3]) for c in C.SIZES}
    assert {(1024, 256, 128), (1024, 100, 128), (2048, 512, 128), (2048, 512, 40), (512, 128, 64), (4096, 1024, 128),
            (256, 64, 40), (400, 160, 40)} <= sizes and any(n >= 8192 for n, _, _ in sizes)
    assert any(n == 1024 and h == 256 and s[-1] % 2 == 1 for _, n, h, _, shapes in C.SIZES for s in shapes)
    for case in C.SIZES:
        assert (3, 2, case[1] // 2 + 1) in C.shapes_of(case)


@pytest.mark.parametrize("name,n_mfcc,want", [
    ("1024_even", None, "lds_kit9_mel"), ("1024_even", 40, "lds_kit9_dct"), ("256_m40", 40, "lds_kit9_dct"),
    ("2048_m128", None, "lds_kit0_mel"), ("2048_m40", 40, "lds_kit0_dct"), ("4096_m128", None, "lds_kit0_mel"),
    ("4096_m128", 40, "lds_kit0_big_dct"), ("8192_m128", None, "lds_kit0_big_mel"), ("8192_m128", 40, "global_dct"),
    ("16384_m128", None, "global_mel"), ("16384_m128", 40, "global_dct")])
def test_case_class(name, n_mfcc, want):
    case = next(c for c in C.SIZES if c[0] == name)
    assert C.module_class(C.module_of(case, n_mfcc=n_mfcc)) == want


def test_forward_paths_of_the_named_cases():
    def path(name, n_mfcc, L):
        case = next(c for c in C.SIZES if c[0] == name)
        return C.forward_path(C.module_of(case, n_mfcc=n_mfcc), L)
    assert path("1024_even", None, 9000) == "fused" and path("1024_even", 40, 9000) == "fused_dct"
    assert path("1024_odd", None, 9001) == "generic" and path("1024_even", None, 513) == "generic"
    assert path("1024_hop100", None, 7000) == "generic"
    assert path("2048_m128", None, 30000) == "single" and path("2048_m128", 40, 30000) == "single_dct"
    assert path("2048_m40", None, 30000) == "generic" and path("2048_m40", 40, 30000) == "generic_dct"
    assert path("512_m64", None, 9001) == "single"


def test_mfcc_backward_entry_is_exported_declared_and_bound():
    lib = _lib.lib()
    assert hasattr(lib, "at_mfcc_backward") and "at_mfcc_backward" in _lib.exported_symbols()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    assert re.search(r"\bint at_mfcc_backward\s*\(", hdr)
    assert lib.at_abi_version() == 4
    nil4 = (None, None, None, None)
    # null arguments, a bad power, a channel count that does not match without a DCT: refused before any device call
    assert lib.at_mfcc_backward(None, 1, 3, 513, None, 128, 128, 2, *nil4, 0, *nil4, 0, None, None, None, None) == _lib.AT_EINVAL
    assert lib.at_mfcc_backward(8, 1, 3, 513, 8, 128, 128, 3, *nil4, 0, 8, 8, 8, 8, 4, None, None, 8, None) == _lib.AT_EINVAL
    assert lib.at_mfcc_backward(8, 1, 3, 513, 8, 40, 128, 2, *nil4, 0, 8, 8, 8, 8, 4, None, None, 8, None) == _lib.AT_EINVAL
    assert lib.at_mfcc_backward(8, 1, 0, 513, 8, 128, 128, 2, *nil4, 0, 8, 8, 8, 8, 4, None, None, 8, None) == _lib.AT_EINVAL
    assert lib.at_mfcc_backward(8, 1, 3, 513, 8, 128, 128, 2, *nil4, 0, *nil4, 0, None, None, 8, None) == _lib.AT_EINVAL
    # a DCT without the forward bank's tables; a misaligned spectrum
    assert lib.at_mfcc_backward(8, 1, 3, 513, 8, 40, 128, 2, *nil4, 0, 8, 8, 8, 8, 4, 8, None, 8, None) == _lib.AT_EINVAL
    assert lib.at_mfcc_backward(12, 1, 3, 513, 8, 128, 128, 2, *nil4, 0, 8, 8, 8, 8, 4, None, None, 8, None) == _lib.AT_EINVAL
    assert lib.at_mfcc_backward(None, 0, 3, 513, None, 128, 128, 2, *nil4, 0, *nil4, 0, None, None, None, None) == _lib.AT_OK


def test_autograd_surface_and_unchanged_refusals():
    assert "MfccFunction" in autograd.__all__ and issubclass(autograd.MfccFunction, torch.autograd.Function)
    m = A.MFCC()
    # a CPU tensor is refused with or without requires_grad; so is float64 (no silent narrowing)
    for x in (torch.zeros(2, 4096), torch.zeros(2, 4096, requires_grad=True)):
        with pytest.raises(A.AcidsHipError):
            m(x)
    with pytest.raises(A.AcidsHipError):
        m(torch.zeros(2, 4096, dtype=torch.float64, requires_grad=True))

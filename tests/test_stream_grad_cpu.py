"""CPU side of the streaming-path backward passes (stream_grad.hip; at_rfft_frames_backward, at_irfft_frames_backward,
at_oadd_forward_backward, at_oadd_invert_backward): the four adjoint formulas restated in numpy against float64 torch
autograd of the reference's statements, the sweep's coverage, the argument checks of the four entry points (no device
is touched) and the new autograd.Functions."""
import itertools

import numpy as np
import pytest
import torch

import stream_grad_cases as C
from acids_transforms_amd import _lib, autograd

TOL = 1e-12


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


@pytest.mark.parametrize("case", C.SWEEP, ids=C.sweep_id)
def test_frame_analysis_adjoint_formula(case):
    (N, h), n, S = case["size"], case["n"], case["S"]
    g = _gen(N, h, n, S)
    w = C.hann(N)
    frames = torch.randn(S, n, N, dtype=torch.float64, generator=g)
    G = torch.randn(S, n, N // 2 + 1, dtype=torch.complex128, generator=g)
    want = C.autograd_of(lambda f: C.ref_analysis(f, w), frames, G)
    assert C.rel_err(C.np_rfft_frames_backward(G, w, N), want) < TOL


@pytest.mark.parametrize("case", C.SYNTH_SWEEP, ids=C.sweep_id)
def test_frame_synthesis_adjoint_formula(case):
    (N, h), n, S = case["size"], case["n"], case["S"]
    g = _gen(N, h, n, S, 3)
    wd = C.rand_window(N)
    F = N // 2 + 1
    gf = torch.randn(S, n, N, dtype=torch.float64, generator=g)
    if case["form"] == "complex":
        X = torch.randn(S, n, F, dtype=torch.complex128, generator=g)
        want = C.autograd_of(lambda X_: C.ref_synthesis(X_, wd, N), X, gf)
        got = C.np_irfft_frames_backward(gf, wd, N)
    else:
        mag = torch.rand(S, n, F, dtype=torch.float64, generator=g)
        phase = 6.283 * torch.rand(S, n, F, dtype=torch.float64, generator=g)
        want = C.autograd_of(lambda m: C.ref_synthesis(m * torch.exp(1j * phase), wd, N), mag, gf)
        got = C.np_irfft_frames_backward(gf, wd, N, phase=phase)
    assert C.rel_err(got, want) < TOL


@pytest.mark.parametrize("N,h", C.SIZES)
def test_overlap_add_adjoint_formulas(N, h):
    keep = C.keep_of(N, h)
    for Cn, S in itertools.product(C.chunk_lengths(N, h), C.STREAMS):
        g = _gen(N, h, Cn, S)
        x = torch.randn(S, Cn, dtype=torch.float64, generator=g)
        hist = torch.randn(S, keep, dtype=torch.float64, generator=g)
        n = C.n_frames(keep + Cn, N, h)
        gf = torch.randn(S, n, N, dtype=torch.float64, generator=g)
        want = C.autograd_of(lambda x_: C.ref_frames(x_, hist, N, h), x, gf)
        got = C.np_oadd_forward_backward(gf, N, h, keep, Cn)
        assert C.rel_err(got, want) < TOL, (N, h, Cn, S)
        covered = (n - 1) * h + N - keep
        if covered < Cn:
            assert np.all(got[:, covered:] == 0), (N, h, Cn)
        # invert: the same frames on a carried tail
        frames = torch.randn(S, n, N, dtype=torch.float64, generator=g)
        tail = torch.randn(S, keep, dtype=torch.float64, generator=g)
        gain = 1.5
        out_len = (n - 1) * h + N - keep
        gy = torch.randn(S, out_len, dtype=torch.float64, generator=g)
        want = C.autograd_of(lambda f: C.ref_oadd_invert(f, tail, N, h, gain)[0], frames, gy)
        got = C.np_oadd_invert_backward(gy, n, N, h, keep, gain)
        assert C.rel_err(got, want) < TOL, (N, h, Cn, S)
        # what only reaches the new tail gets exactly 0
        assert np.all(got[:, -1, max(0, out_len - (n - 1) * h):] == 0)


def test_c1000_leaves_232_samples_uncovered():
    N, h, keep = 1024, 256, 768
    assert C.n_frames(keep + 1000, N, h) == 3
    gx = C.np_oadd_forward_backward(np.ones((1, 3, N)), N, h, keep, 1000)
    assert np.all(gx[:, 768:] == 0) and np.all(gx[:, :768] > 0) and gx[:, 768:].shape[-1] == 232


def test_sweep_covers_every_pair_of_factors():
    for cases, names in ((C.SWEEP, ("size", "n", "S")), (C.SYNTH_SWEEP, ("size", "n", "S", "form"))):
        for a, b in itertools.combinations(names, 2):
            seen = {(repr(c[a]), repr(c[b])) for c in cases}
            want = {(repr(x), repr(y)) for x in C.FACTORS[a] for y in C.FACTORS[b]}
            assert seen == want, (a, b, sorted(want - seen))
    assert (1024, 256) in C.SIZES and 1000 in C.chunk_lengths(1024, 256)
    # a frame count that ends a shared register FFT inside a stream, at each of the shared sizes
    for N, per in ((128, 8), (512, 2)):
        assert any(c["size"][0] == N and c["n"] % per and c["S"] > 1 for c in C.SWEEP)


def test_entry_points_are_exported_bound_and_check_their_arguments():
    lib = _lib.lib()
    names = ("at_rfft_frames_backward", "at_rfft_frames_backward_workspace_bytes", "at_irfft_frames_backward",
             "at_irfft_frames_backward_workspace_bytes", "at_oadd_forward_backward", "at_oadd_invert_backward")
    for name in names:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
    assert lib.at_abi_version() == _lib.ABI_VERSION == 4
    OK, EINVAL = _lib.AT_OK, _lib.AT_EINVAL
    # frame analysis: (G, nframes, frames_per_stream, n_fft, window, gframes, workspace, bytes, stream)
    f = lib.at_rfft_frames_backward
    assert f(None, 0, 3, 1024, None, None, None, 0, None) == OK
    assert f(None, 6, 3, 1024, None, None, None, 0, None) == EINVAL          # null pointers
    assert f(8, -1, 3, 1024, 8, 8, 256, 4096, None) == EINVAL
    assert f(8, 6, 0, 1024, 8, 8, 256, 4096, None) == EINVAL                 # no stream length
    assert f(8, 7, 3, 1024, 8, 8, 256, 4096, None) == EINVAL                 # not a whole number of streams
    assert f(8, 6, 3, 0, 8, 8, 256, 4096, None) == EINVAL
    assert f(12, 6, 3, 1024, 8, 8, 256, 4096, None) == EINVAL                # complex rows 8-byte aligned
    assert f(8, 6, 3, 16386, 8, 8, 256, 1 << 20, None) == _lib.AT_EUNSUPPORTED
    assert f(8, 6, 3, 1024, 8, 8, 256, 16, None) == _lib.AT_EWORKSPACE
    assert lib.at_rfft_frames_backward_workspace_bytes(6, 1024) == 4096
    assert lib.at_rfft_frames_backward_workspace_bytes(0, 1024) == 0
    # frame synthesis: (gframes, phase, nframes, frames_per_stream, n_fft, inv_window, out, workspace, bytes, stream)
    f = lib.at_irfft_frames_backward
    assert f(None, None, 0, 3, 1024, None, None, None, 0, None) == OK
    assert f(None, None, 6, 3, 1024, None, None, None, 0, None) == EINVAL
    assert f(8, None, 7, 3, 1024, 8, 8, 256, 4096, None) == EINVAL
    assert f(8, None, 6, 3, 1024, 8, 12, 256, 4096, None) == EINVAL          # complex out 8-byte aligned
    assert f(8, 8, 6, 3, 1024, 8, 12, 256, 4096, None) == _lib.AT_EWORKSPACE  # polar: float out, but rows in the workspace
    assert f(8, None, 6, 3, 1024, 8, 8, 128, 4096, None) == _lib.AT_EWORKSPACE
    assert lib.at_irfft_frames_backward_workspace_bytes(6, 3, 1024, 0) == 4096
    assert lib.at_irfft_frames_backward_workspace_bytes(6, 3, 1024, 1) == 4096 + 6 * 513 * 8
    assert lib.at_irfft_frames_backward_workspace_bytes(7, 3, 1024, 1) == 0
    # the polar form is cut into chunks of whole streams within 1 GiB of rows
    per_stream = 9 * 513 * 8
    big = lib.at_irfft_frames_backward_workspace_bytes(9 * 100000, 9, 1024, 1) - 4096
    assert big % per_stream == 0 and big <= 1 << 30 < big + per_stream
    # overlap-add: (gframes, S, n, n_fft, hop, keep, C, gx, stream) / (gy, S, n, n_fft, hop, keep, gain, gframes, stream)
    f = lib.at_oadd_forward_backward
    assert f(None, 0, 3, 1024, 256, 768, 1000, None, None) == OK
    assert f(None, 1, 3, 1024, 256, 768, 1000, None, None) == EINVAL
    assert f(8, 1, 0, 1024, 256, 768, 1000, 8, None) == EINVAL
    assert f(8, 1, 3, 1024, 0, 768, 1000, 8, None) == EINVAL
    assert f(8, 1, 3, 1024, 256, 768, 0, 8, None) == EINVAL
    f = lib.at_oadd_invert_backward
    assert f(None, 0, 3, 1024, 256, 768, None, None, None) == OK
    assert f(None, 1, 3, 1024, 256, 768, None, None, None) == EINVAL
    assert f(8, 1, 3, 1024, 256, 768, None, 8, None) == EINVAL               # the gain is read on the device
    assert f(8, 1, 1, 128, 32, 4096, 8, 8, None) == EINVAL                   # keep longer than the frames reach
    assert f(8, 1, 3, 1024, -1, 768, 8, 8, None) == EINVAL


def test_new_functions_are_public():
    for name in ("RtStftFunction", "RtIstftFunction", "RtIstftPolarFunction", "OaddFramesFunction",
                 "OaddInvertFunction"):
        assert name in autograd.__all__ and issubclass(getattr(autograd, name), torch.autograd.Function)

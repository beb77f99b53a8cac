"""CPU side of the ISTFT adjoint (at_istft_backward): the formula the kernels implement, restated in float64 and
checked against torch autograd of torch.istft; the GPU sweep's coverage of the launcher's dispatch (istft_grad_cases.py);
the new ABI entries."""
import pytest
import torch

import istft_grad_cases as C
from acids_transforms_amd import _lib


def envelope(w, N, h, T):
    """sum of w^2 over the frames that cover each padded sample, oldest first."""
    env = torch.zeros(N + h * (T - 1), dtype=w.dtype)
    for t in range(T):
        env[t * h:t * h + N] += w * w
    return env


def istft_adjoint_model(gy, w, N, h, T, phase=None):
    """What at_istft_backward computes: u = gy / env in the kept samples (0 in the padding), the rfft of w u per frame
    scaled by c_k / N.  With a phase: Re(gX e^{-i phase})."""
    B = gy.shape[0]
    env = envelope(w, N, h, T)
    u = torch.zeros(B, N + h * (T - 1), dtype=gy.dtype)
    lo, Ly = N // 2, gy.shape[-1]
    u[:, lo:lo + Ly] = gy / env[lo:lo + Ly]
    frames = torch.stack([u[:, t * h:t * h + N] for t in range(T)], 1)
    gX = torch.fft.rfft(frames * w, dim=-1) * (2.0 / N)
    gX[..., 0] *= 0.5
    if N % 2 == 0:
        gX[..., N // 2] *= 0.5
    if phase is None:
        return gX
    return gX.real * torch.cos(phase) + gX.imag * torch.sin(phase)


def torch_grads(X, w, N, h, gy, mag=None, phase=None):
    """(X.grad, mag.grad) of torch.istft fed gy, in float64."""
    if mag is not None:
        mag = mag.clone().requires_grad_()
        Xc = mag * torch.exp(1j * phase)
    else:
        X = X.clone().requires_grad_()
        Xc = X
    y = torch.istft(Xc.transpose(-2, -1), N, h, window=w, center=True, onesided=True)
    y.backward(gy)
    return (X.grad if mag is None else None), (mag.grad if mag is not None else None)


CASES = [(16, 4, T) for T in (1, 2, 3, 5, 20)] + [(9, 3, T) for T in (1, 2, 4, 11)] + \
    [(9, 9, 1), (9, 9, 3), (8, 1, 20), (7, 1, 13), (16, 16, 4), (16, 6, 7), (400, 160, 7), (441, 110, 6),
     (1024, 256, 10), (1024, 300, 5), (15, 4, 17)]


@pytest.mark.parametrize("N,h,T", CASES)
def test_istft_adjoint_formula_matches_torch_autograd(N, h, T):
    g = torch.Generator().manual_seed(N * 131 + h * 7 + T)
    # a window with no zero: the NOLA condition then holds at h = N too, the Hann window where it holds anyway
    w = torch.hann_window(N, dtype=torch.float64) if h < N else 0.5 + torch.rand(N, generator=g, dtype=torch.float64)
    F = N // 2 + 1
    X = torch.randn(2, T, F, dtype=torch.complex128, generator=g)
    Ly = h * (T - 1) + (N & 1)
    gy = torch.randn(2, Ly, dtype=torch.float64, generator=g)
    if Ly == 0:
        assert istft_adjoint_model(gy, w, N, h, T).abs().max() == 0
        return
    gX, _ = torch_grads(X, w, N, h, gy)
    assert torch.allclose(istft_adjoint_model(gy, w, N, h, T), gX, rtol=0, atol=1e-12 * float(gX.abs().max())), (N, h, T)
    mag = torch.rand(2, T, F, dtype=torch.float64, generator=g)
    phase = 6.283 * torch.rand(2, T, F, dtype=torch.float64, generator=g)
    _, gmag = torch_grads(None, w, N, h, gy, mag=mag, phase=phase)
    model = istft_adjoint_model(gy, w, N, h, T, phase=phase)
    assert torch.allclose(model, gmag, rtol=0, atol=1e-12 * float(gmag.abs().max())), (N, h, T)


def test_restated_dispatch():
    assert [C.family(n) for n in [1024, 2048, 4096, 512, 128, 256, 8192, 400, 441, 4, 64]] == \
        ["1024", "2048", "4096", "generic", "generic", "generic", "generic", "mixed", "mixed", "mixed", "generic"]
    # the library's own numbers (no device needed)
    lib = _lib.lib()
    for B, T, n, h in [(4, 10, 1024, 300), (1024, 690, 1024, 300), (3, 5, 441, 110), (16, 1200000, 16, 4), (2, 7, 8192, 2048),
                       (1024, 690, 1024, 256)]:
        assert lib.at_istft_backward_workspace_bytes(B, T, n, h) == C.workspace_bytes(B, T, n, h), (B, T, n, h)
    assert C.path_class(*C.CHUNKED[:2], C.CHUNKED[3], C.CHUNKED[2])["chunks"] >= 2


def test_gpu_sweep_reaches_every_dispatch_class():
    classes = C.sweep_classes()
    assert C.FAMILIES <= {c["family"] for _, c in classes}, sorted(C.FAMILIES - {c["family"] for _, c in classes})
    for fam in C.FAMILIES - {"zeros"}:
        for polar in (False, True):
            assert any(c["family"] == fam and c["polar"] == polar for _, c in classes), (fam, polar)
    assert any(c["chunks"] >= 2 for _, c in classes)
    # T = 1 at odd n_fft keeps one sample; T = 1 at even n_fft keeps none
    assert any(k[0] % 2 and k[3] == 1 for k, _ in classes if len(k) == 5)


def test_istft_backward_entries_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("at_istft_backward", "at_istft_backward_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
    assert lib.at_istft_backward_workspace_bytes(0, 10, 1024, 300) == 0
    # argument checks that need no device
    assert lib.at_istft_backward(None, 1, 3, 1024, 0, None, None, None, None, None, 0, None) == _lib.AT_EINVAL
    assert lib.at_istft_backward(None, 1, 3, 1024, 256, None, None, None, None, None, 0, None) == _lib.AT_EINVAL
    assert lib.at_istft_backward(None, 0, 3, 1024, 256, None, None, None, None, None, 0, None) == _lib.AT_OK
    # complex output rows must be 8-byte aligned (checked before any device work); every shape states its workspace
    assert lib.at_istft_backward(8, 1, 3, 1024, 256, 8, None, None, 4, None, 0, None) == _lib.AT_EINVAL
    for h in (128, 256, 512):
        assert lib.at_istft_backward_workspace_bytes(7, 90, 1024, h) == C.workspace_bytes(7, 90, 1024, h) > 0

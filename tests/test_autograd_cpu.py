"""CPU side of the backward passes (autograd.hip): the adjoint formula the STFT kernel implements, restated in float64
and checked against torch autograd of torch.stft; the band tables of the Magnitude backward; the new ABI entries."""
import numpy as np
import pytest
import torch

from acids_transforms_amd import _lib
from acids_transforms_amd.utils.banded import bank_columns
from acids_transforms_amd.utils.melbank import melscale_fbanks


def adjoint_model(G, w, N, h, L):
    """What at_stft_backward computes: (N/2) w irfft(G) plus the halves of DC / Nyquist, overlap-added in frame order
    without an envelope, then the reflect fold at both ends."""
    B, T, _ = G.shape
    m = torch.arange(N)
    edge = 0.5 * G[..., :1].real
    if N % 2 == 0:
        edge = edge + 0.5 * G[..., N // 2:N // 2 + 1].real * (1 - 2 * (m % 2))
    q = torch.fft.irfft(G, n=N) * (w * (N / 2)) + w * edge
    P = N // 2
    dp = torch.zeros(B, L + 2 * P, dtype=q.dtype)
    for t in range(T):
        dp[:, t * h:t * h + N] += q[:, t]
    dx = dp[:, P:P + L].clone()
    for i in range(1, P + 1):
        dx[:, i] += dp[:, P - i]
    for i in range(L - P - 1, L - 1):
        dx[:, i] += dp[:, 2 * L + P - 2 - i]
    return dx


@pytest.mark.parametrize("N,h,L", [(16, 4, 9), (16, 4, 40), (15, 4, 8), (15, 5, 33), (441, 110, 221), (400, 160, 1000),
                                   (1024, 256, 513), (128, 32, 65)])
def test_adjoint_formula_matches_torch_autograd(N, h, L):
    g = torch.Generator().manual_seed(N + L)
    x = torch.randn(2, L, dtype=torch.float64, generator=g).requires_grad_()
    w = torch.hann_window(N, dtype=torch.float64)
    X = torch.stft(x, N, h, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(-2, -1)
    assert X.shape[1] == 1 + (L - (N & 1)) // h          # the frame count at_stft_backward checks
    G = torch.randn(X.shape, dtype=torch.complex128, generator=g)
    X.backward(G)
    d = adjoint_model(G, w, N, h, L)
    assert float((d - x.grad).abs().max() / x.grad.abs().max()) < 1e-13


@pytest.mark.parametrize("n_mels", [128, 513])
def test_bank_columns_rebuild_the_bank_and_its_transpose(n_mels):
    bank = melscale_fbanks(513, 0.0, 22050.0, n_mels, 44100)
    for b in (bank, bank.t().contiguous()):
        start, length, offset, w = bank_columns(b)
        K, N = b.shape
        assert start.shape == length.shape == offset.shape == (N,)
        dense = np.zeros((K, N), np.float32)
        for j in range(N):
            dense[start[j]:start[j] + length[j], j] = w[offset[j]:offset[j] + length[j]]
        assert np.array_equal(dense, b.numpy())
        assert w.size >= 1 and int(offset[-1] + length[-1]) <= w.size


def test_backward_entries_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("at_stft_backward", "at_stft_backward_workspace_bytes", "at_magnitude_backward"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    # one window slot + the irFFT frames of a chunk of clips (capped at 1 GiB of frames)
    assert lib.at_stft_backward_workspace_bytes(4, 10, 1024, 256) == 4096 + 4 * 10 * 1024 * 4
    assert lib.at_stft_backward_workspace_bytes(1024, 690, 1024, 256) == 4096 + 379 * 690 * 1024 * 4
    # argument checks that need no device: L at most n_fft/2, a frame count that is not the forward's
    assert lib.at_stft_backward(None, 1, 3, 512, 1024, 256, None, None, None, 0, None) == _lib.AT_EINVAL
    assert lib.at_stft_backward(None, 1, 5, 1000, 1024, 256, None, None, None, 0, None) == _lib.AT_EINVAL
    assert lib.at_magnitude_backward(None, 1, 1, 513, None, 513, 0, None, None, None, None, 0, None, None, None, None, 0,
                                     0, None, 0.0, None, None, None) == _lib.AT_EINVAL

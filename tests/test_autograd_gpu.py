"""Gradients through STFT / DGT / Magnitude (autograd.py, autograd.hip) against torch autograd of the reference's own
expressions (torch.stft(center=True, pad_mode="reflect"), abs, matmul with the bank, the contrast, (x - o) / s), run on
the CPU in float64 from the same fp32 inputs.  Tolerance: normwise rel_max <= 1e-5, as for the forward."""
import zlib

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5


def cpu(t):
    return t.detach().cpu().numpy()


def ref_stft_grad(x, window, n_fft, hop, G):
    """x.grad of torch.stft(x) fed the upstream gradient G, in float64 on the CPU."""
    x64 = x.detach().cpu().double().requires_grad_()
    w64 = window.detach().cpu().double()
    X = torch.stft(x64.reshape(-1, x64.shape[-1]), n_fft, hop, window=w64, center=True, pad_mode="reflect",
                   return_complex=True).transpose(-2, -1)
    X.backward(G.detach().cpu().to(torch.complex128).reshape(X.shape))
    return x64.grad


@pytest.mark.parametrize("cls", ["stft", "dgt"])
@pytest.mark.parametrize("n,h", [(1024, 256), (1024, 128), (1024, 512), (512, 128), (2048, 512), (4096, 1024), (128, 32),
                                 (400, 160), (441, 110)])
def test_stft_grad_matches_torch_autograd(dev, cls, n, h):
    m = (A.STFT if cls == "stft" else A.DGT)(n_fft=n, hop_length=h).to(dev)
    g = torch.Generator().manual_seed(n * 7 + h)
    # L just above n_fft/2 (both folds overlap one frame), a few frames, a longer odd length; and a (3, 2, L) batch
    for shape in [(1, n // 2 + 1), (2, n // 2 + 3), (2, 3 * n + 5), (3, 2, 2 * n + h + 1)]:
        x = torch.randn(shape, generator=g).to(dev).requires_grad_()
        X = m(x)
        assert X.requires_grad and X.grad_fn is not None
        G = torch.randn(X.shape, dtype=torch.complex64, generator=g).to(dev)
        X.backward(G)
        ref = ref_stft_grad(x, m.window[:n], n, h, G)
        assert x.grad.shape == x.shape and x.grad.dtype == torch.float32
        assert rel_max(cpu(x.grad).reshape(ref.shape), ref.numpy()) < TOL, (cls, n, h, shape)


def test_stft_grad_without_grad_is_the_plain_forward(dev):
    m = A.STFT().to(dev)
    x = torch.randn(2, 9000, device=dev)
    X0 = m(x)
    X1 = m(x.clone().requires_grad_())
    assert X0.grad_fn is None and X1.grad_fn is not None
    assert torch.equal(X0, X1.detach())
    # the lazy phase buffer holds a detached spectrum: reading it does not touch the graph
    assert not m.phase_buffer.requires_grad
    with torch.no_grad():
        assert m(x.clone().requires_grad_()).grad_fn is None
    with pytest.raises(RuntimeError):
        xx = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad(m(xx).abs().sum(), xx, create_graph=True)
        gx.sum().backward()


@pytest.fixture(scope="module")
def bench_grad(dev):
    """1024 clips x 4 s at 1024/256: the bench size.  x, G, <STFT(x), G> and x.grad of STFT fed G."""
    m = A.STFT().to(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(1024, 176400, device=dev, generator=g)
    xr = x.clone().requires_grad_()
    X = m(xr)
    G = torch.randn(X.shape, dtype=torch.complex64, device=dev, generator=g)
    lhs = 0.0
    for i in range(0, 1024, 64):
        Xi, Gi = X[i:i + 64].detach(), G[i:i + 64]
        lhs += float((Xi.real.double() * Gi.real.double()).sum() + (Xi.imag.double() * Gi.imag.double()).sum())
    del X
    torch.autograd.backward(m(xr), G)
    return m, x, G, lhs, xr.grad


def test_adjoint_identity_at_bench_size(bench_grad):
    _, x, _, lhs, dx = bench_grad
    rhs = 0.0
    for i in range(0, 1024, 64):
        rhs += float((x[i:i + 64].double() * dx[i:i + 64].double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_grad_bits_do_not_depend_on_the_batch(bench_grad):
    m, x, G, _, dx = bench_grad
    for k in (0, 511, 1023):
        xk = x[k:k + 1].clone().requires_grad_()
        m(xk).backward(G[k:k + 1])
        assert torch.equal(xk.grad[0], dx[k]), k


def _ref_magnitude(x64, mod):
    """The reference's Magnitude.forward (spectral_repr.py:215-226) in float64."""
    a = x64.abs()
    if mod.mel:
        a = torch.matmul(a, mod.mel_bank[0].detach().cpu().double())
    eps = float(mod.eps)
    c = mod.contrast_mode
    if c == "log1p":
        a = torch.log(1 + a)
    elif c == "log":
        a = torch.log(torch.clamp(a, eps, None))
    elif c == "log10":
        a = torch.log10(torch.clamp(a, eps, None))
    if isinstance(mod.norm, A.transforms.norm.Normalize):
        a = (a - mod.norm.offset.detach().cpu().double()) / mod.norm.scale.detach().cpu().double()
    if not mod.keep_nyquist:
        a = a[..., 1:]
    return a


def _mag_input(complex_in, g):
    shape = (2, 5, 513)
    mag = torch.rand(shape, generator=g) * 4
    eps = torch.finfo(torch.float32).eps
    mag[0, 0, :40] = 0.0                                      # exact zeros
    mag[0, 1, :60] = eps * torch.tensor([0.3, 3.0]).repeat(30)   # straddling eps
    mag[1, 2, 100:200] = 0.0
    if not complex_in:
        return mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    ph = torch.rand(shape, generator=g) * 6.283
    return torch.polar(mag, ph)


@pytest.mark.parametrize("complex_in", [True, False])
@pytest.mark.parametrize("keep_nyquist", [True, False])
@pytest.mark.parametrize("norm", ["unipolar", "bipolar", "gaussian", None])
@pytest.mark.parametrize("mel", ["n128", "n513", "off"])
@pytest.mark.parametrize("contrast", [None, "log1p", "log", "log10"])
def test_magnitude_grad(dev, contrast, mel, norm, keep_nyquist, complex_in):
    kw = {"n_mels": 128} if mel == "n128" else ({"mel": False} if mel == "off" else {})
    mod = A.Magnitude(mode=norm, contrast=contrast, keep_nyquist=keep_nyquist, **kw).to(dev)
    g = torch.Generator().manual_seed(zlib.crc32(repr((contrast, mel, norm, keep_nyquist, complex_in)).encode()))
    x = _mag_input(complex_in, g)
    mod.scale_data(x.to(dev))
    xd = x.to(dev).requires_grad_()
    f = mod(xd)
    assert f.grad_fn is not None
    plain = mod(x.to(dev))
    assert torch.equal(plain, f.detach())
    dF = torch.randn(f.shape, generator=g)
    f.backward(dF.to(dev))
    x64 = x.to(torch.complex128 if complex_in else torch.float64).requires_grad_()
    ref = _ref_magnitude(x64, mod)
    assert ref.shape == f.shape
    ref.backward(dF.double())
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    got, want = cpu(xd.grad), x64.grad.numpy()
    assert rel_max(got, want) < TOL
    assert np.all(got[x.numpy() == 0] == 0)                  # torch's sgn(0) = 0


def test_magnitude_bf16_backward_is_the_fp32_one(dev):
    mod = A.Magnitude(n_mels=128, bank_dtype="bf16").to(dev)
    g = torch.Generator().manual_seed(11)
    x = _mag_input(True, g)
    mod.scale_data(x.to(dev))
    xd = x.to(dev).requires_grad_()
    f = mod(xd)
    dF = torch.randn(f.shape, generator=g)
    f.backward(dF.to(dev))
    x64 = x.to(torch.complex128).requires_grad_()
    _ref_magnitude(x64, mod).backward(dF.double())
    assert rel_max(cpu(xd.grad), x64.grad.numpy()) < TOL


def _ref_chain(x, stft, mag):
    x64 = x.detach().cpu().double().requires_grad_()
    X = torch.stft(x64, 1024, stft._hop, window=stft.window[:1024].cpu().double(), center=True, pad_mode="reflect",
                   return_complex=True).transpose(-2, -1)
    return x64, X, _ref_magnitude(X, mag)


@pytest.mark.parametrize("fused", [True, False])
def test_stft_magnitude_chain(dev, fused):
    stft = A.STFT().to(dev)
    mag = A.Magnitude(n_mels=128).to(dev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 20000, generator=g) * 0.1
    xd = x.to(dev)
    mag.scale_data(stft(xd))
    assert mag.can_fuse_with(stft, xd)
    run = (lambda v: mag.forward_fused(stft, v)) if fused else (lambda v: mag(stft(v)))
    plain = run(xd)
    xr = xd.clone().requires_grad_()
    feat = run(xr)
    assert feat.grad_fn is not None and torch.equal(plain, feat.detach())
    dF = torch.randn(feat.shape, generator=g)
    feat.backward(dF.to(dev))
    x64, _, ref = _ref_chain(x, stft, mag)
    ref.backward(dF.double())
    assert rel_max(cpu(xr.grad), x64.grad.numpy()) < TOL
    # the composed transform (fused when it can be) gives the same gradient
    xc = xd.clone().requires_grad_()
    (stft + mag)(xc).backward(dF.to(dev))
    assert rel_max(cpu(xc.grad), x64.grad.numpy()) < TOL


def test_fused_chain_with_the_spectrum_in_the_loss(dev):
    stft = A.STFT().to(dev)
    mag = A.Magnitude(n_mels=128).to(dev)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 12000, generator=g) * 0.1
    mag.scale_data(stft(x.to(dev)))
    xr = x.to(dev).requires_grad_()
    X, feat = mag.forward_fused(stft, xr, return_spectrum=True)
    dF = torch.randn(feat.shape, generator=g)
    G = torch.randn(X.shape, dtype=torch.complex64, generator=g)
    torch.autograd.backward([feat, X], [dF.to(dev), G.to(dev)])
    x64, X64, ref = _ref_chain(x, stft, mag)
    torch.autograd.backward([ref, X64], [dF.double(), G.to(torch.complex128)])
    assert rel_max(cpu(xr.grad), x64.grad.numpy()) < TOL


def test_training_an_upstream_conv_on_a_mel_loss(dev):
    torch.manual_seed(0)
    T = A.STFT() + A.Magnitude(n_mels=128)
    T = T.to(dev)
    x = torch.randn(4, 1, 16384, device=dev) * 0.1
    target_conv = torch.nn.Conv1d(1, 1, 31, padding=15, bias=False).to(dev)
    with torch.no_grad():
        y = target_conv(x).squeeze(1)
    T.scale_data(y)
    target = T(y)
    model = torch.nn.Conv1d(1, 1, 31, padding=15, bias=False).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(T(model(x).squeeze(1)), target)
        loss.backward()
        assert model.weight.grad is not None and bool(torch.isfinite(model.weight.grad).all())
        assert float(model.weight.grad.abs().max()) > 0
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.8 * losses[0], losses

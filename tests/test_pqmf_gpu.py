"""GPU side of PQMF (csrc/pqmf.hip, transforms/pqmf.py, autograd.PqmfFunction / PqmfInvertFunction): parity of forward,
invert and their gradients with the float64 restatement of pqmf_cases.py within the library's normwise bound 1e-5,
batch and shift independence to the bit, routing, composition and the errors on the device."""
import math

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import pqmf_cases as C
from acids_transforms_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-5

_MODULES = {}


def _module(n_band, taps, dev):
    key = (n_band, taps)
    if key not in _MODULES:
        _MODULES[key] = A.PQMF(n_band=n_band, taps=taps).to(dev)
    return _MODULES[key]


def _bank(pq):
    """The float64 bank of the module's own fp32 prototype: the kernels and the restatement filter with the same taps."""
    return C.bank(pq.prototype.cpu().numpy(), pq.n_band)


def _tile(pq):
    return ops.pqmf_tile_blocks(pq.n_band, pq.taps)


@pytest.mark.parametrize("n_band,taps", C.PARITY)
def test_forward_and_invert_match_float64(dev, n_band, taps):
    pq = _module(n_band, taps, dev)
    hk, tile = _bank(pq), _tile(pq)
    for i, T in enumerate(C.block_counts(tile)):
        x = C.audio((2, n_band * T), 10 + i)
        y = pq(x.float().to(dev))
        assert y.shape == (2, n_band, T) and y.dtype == torch.float32
        err_f = C.rel_max(y.cpu().numpy(), C.analysis(x.float().double(), hk).numpy())
        # invert on planted band signals, not on forward's output
        z = C.audio((2, n_band, T), 20 + i)
        xh = pq.invert(z.float().to(dev))
        assert xh.shape == (2, n_band * T) and xh.dtype == torch.float32
        err_i = C.rel_max(xh.cpu().numpy(), C.synthesis(z.float().double(), hk).numpy())
        print("n_band %d taps %d T %d: forward %.2e invert %.2e" % (n_band, taps, T, err_f, err_i))
        assert err_f < TOL and err_i < TOL


@pytest.mark.parametrize("n_band,taps", C.SPECIALISED)
def test_every_band_count_with_a_kernel_of_its_own(dev, n_band, taps):
    """4, 8, 16, 32 and 64 bands run kernels compiled for that count; the sweep above reaches 16 and 64."""
    pq = _module(n_band, taps, dev)
    hk, T = _bank(pq), _tile(pq) + 3
    x, z = C.audio((2, n_band * T), 25), C.audio((2, n_band, T), 26)
    err_f = C.rel_max(pq(x.float().to(dev)).cpu().numpy(), C.analysis(x.float().double(), hk).numpy())
    err_i = C.rel_max(pq.invert(z.float().to(dev)).cpu().numpy(), C.synthesis(z.float().double(), hk).numpy())
    print("n_band %d taps %d T %d: forward %.2e invert %.2e" % (n_band, taps, T, err_f, err_i))
    assert err_f < TOL and err_i < TOL


def test_leading_dims_noncontiguous_and_many_rows(dev):
    pq = _module(3, 51, dev)
    hk = _bank(pq)
    x = C.audio((2, 3, 99), 30).float()
    y = pq(x.to(dev))
    assert y.shape == (2, 3, 3, 33)
    assert C.rel_max(y.cpu().numpy(), C.analysis(x.double(), hk).numpy()) < TOL
    xh = pq.invert(y)
    assert xh.shape == (2, 3, 99)
    assert C.rel_max(xh.cpu().numpy(), C.synthesis(y.cpu().double(), hk).numpy()) < TOL
    # non-contiguous: every second sample of a longer signal, and a transposed band axis
    wide = C.audio((2, 198), 31).float().to(dev)
    xs = wide[:, ::2]
    assert not xs.is_contiguous() and torch.equal(pq(xs), pq(xs.contiguous()))
    yt = y.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not yt.is_contiguous() and torch.equal(pq.invert(yt), xh)
    # more rows than a 16-bit grid dimension holds
    rows, M, N, L = C.MANY_ROWS
    small = _module(M, N, dev)
    hs = _bank(small)
    x = C.audio((rows, L), 32).float()
    y = small(x.to(dev))
    assert y.shape == (rows, M, L // M)
    assert C.rel_max(y.cpu().numpy(), C.analysis(x.double(), hs).numpy()) < TOL
    xh = small.invert(y)
    assert C.rel_max(xh.cpu().numpy(), C.synthesis(y.cpu().double(), hs).numpy()) < TOL


def test_a_clip_does_not_depend_on_its_batch(dev):
    pq = _module(16, 513, dev)
    T = _tile(pq) + 9
    x = C.audio((5, 16 * T), 40).float().to(dev)
    y = pq(x)
    z = C.audio((5, 16, T), 41).float().to(dev)
    xh = pq.invert(z)
    for b in (0, 3, 4):
        assert torch.equal(pq(x[b:b + 1]), y[b:b + 1])
        assert torch.equal(pq.invert(z[b:b + 1]), xh[b:b + 1])
    # a NaN stays in its clip
    x[2, 777] = float("nan")
    z[2, 5, 11] = float("nan")
    yn, xn = pq(x), pq.invert(z)
    keep = [0, 1, 3, 4]
    assert torch.equal(yn[keep], y[keep]) and torch.equal(xn[keep], xh[keep])
    assert bool(torch.isnan(yn[2]).any()) and bool(torch.isnan(xn[2]).any())


def test_a_shift_by_one_block_is_a_shift_to_the_bit(dev):
    M, N = 16, 513
    pq = _module(M, N, dev)
    T = 2 * _tile(pq) + 40
    edge = -(-N // M) + 1
    x = C.audio((1, M * T), 50).float()
    shifted = torch.cat([C.audio((1, M), 51).float(), x[:, :-M]], -1)
    y, ys = pq(x.to(dev)), pq(shifted.to(dev))
    assert torch.equal(ys[..., edge + 1:T - edge], y[..., edge:T - edge - 1])
    z = C.audio((1, M, T), 52).float()
    zs = torch.cat([C.audio((1, M, 1), 53).float(), z[..., :-1]], -1)
    xh, xs = pq.invert(z.to(dev)), pq.invert(zs.to(dev))
    assert torch.equal(xs[..., M * (edge + 1):M * (T - edge)], xh[..., M * edge:M * (T - edge - 1)])


def test_round_trip(dev):
    for n_band, taps in ((4, 65), (16, 513)):
        pq = _module(n_band, taps, dev)
        hk = _bank(pq)
        L = n_band * ((4 * taps) // n_band + 8)
        x = C.audio((2, L), 60).float()
        xh = pq.invert(pq(x.to(dev))).cpu().numpy()
        want = C.synthesis(C.analysis(x.double(), hk), hk).numpy()
        print("n_band %d taps %d: round trip against float64 %.2e, interior relative rms against x %.3e"
              % (n_band, taps, C.rel_max(xh, want), C.interior_rel_rms(xh, x.numpy(), taps)))
        assert C.rel_max(xh, want) < TOL


def test_routing(dev):
    pq = _module(4, 65, dev)
    x = C.audio((2, 400), 70).float().to(dev)
    z = C.audio((2, 4, 100), 71).float().to(dev)
    xr, zr = x.clone().requires_grad_(), z.clone().requires_grad_()
    y, xh = pq(xr), pq.invert(zr)
    assert y.grad_fn is not None and xh.grad_fn is not None
    assert torch.equal(y.detach(), pq(x)) and torch.equal(xh.detach(), pq.invert(z))     # the plain route's bits
    assert pq(x).grad_fn is None and pq.invert(z).grad_fn is None
    with torch.no_grad():
        assert pq(xr).grad_fn is None and pq.invert(zr).grad_fn is None
    # the graph keeps no tensor: the two buffers are attributes of the node, not saved tensors
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        pq(xr), pq.invert(zr)
    assert saved == []
    # first order only
    for fn, leaf in ((pq, xr), (pq.invert, zr)):
        with pytest.raises(RuntimeError):
            (g,) = torch.autograd.grad(fn(leaf).square().sum(), leaf, create_graph=True)
            g.sum().backward()


@pytest.mark.parametrize("n_band,taps,blocks", C.GRAD)
def test_gradients_match_float64_autograd(dev, n_band, taps, blocks):
    pq = _module(n_band, taps, dev)
    hk, tile = _bank(pq), _tile(pq)
    T = {"tile+1": tile + 1, "2tile+1": 2 * tile + 1}[blocks]
    x, gy = C.audio((2, n_band * T), 80).float(), C.audio((2, n_band, T), 81).float()
    z, gx = C.audio((2, n_band, T), 82).float(), C.audio((2, n_band * T), 83).float()
    # forward
    xr = x.to(dev).requires_grad_()
    (pq(xr) * gy.to(dev)).sum().backward()
    xd = x.double().requires_grad_()
    (C.analysis(xd, hk) * gy.double()).sum().backward()
    err_f = C.rel_max(xr.grad.cpu().numpy(), xd.grad.numpy())
    # invert
    zr = z.to(dev).requires_grad_()
    (pq.invert(zr) * gx.to(dev)).sum().backward()
    zd = z.double().requires_grad_()
    (C.synthesis(zd, hk) * gx.double()).sum().backward()
    err_i = C.rel_max(zr.grad.cpu().numpy(), zd.grad.numpy())
    print("n_band %d taps %d T %d: d forward %.2e d invert %.2e" % (n_band, taps, T, err_f, err_i))
    assert xr.grad.shape == x.shape and zr.grad.shape == z.shape
    assert err_f < TOL and err_i < TOL
    # the transpose identity in fp32: <forward(x), g> = <x, forward-backward(g)>
    lhs = float((pq(x.to(dev)).double() * gy.to(dev).double()).sum())
    rhs = float((x.to(dev).double() * xr.grad.double()).sum())
    scale = float(pq(x.to(dev)).double().norm() * gy.double().norm())
    assert abs(lhs - rhs) <= 1e-5 * scale
    # a gradient reaches the caller's own, non-contiguous tensor
    wide = torch.zeros(2, 2 * n_band * T, device=dev).requires_grad_()
    pq(wide[:, ::2]).sum().backward()
    assert wide.grad is not None and bool((wide.grad[:, 1::2] == 0).all()) and bool((wide.grad[:, ::2] != 0).any())


def test_composition(dev):
    pq = A.PQMF(4, 65).to(dev)
    chain = A.ComposeAudioTransform([pq])
    x = C.audio((2, 4096), 90).float().to(dev)
    y = chain(x)
    assert y.shape == (2, 4, 1024)
    assert chain.invert(y, inversion_mode=None).shape == (2, 4096) and chain.ratio == 4
    # a band-domain signal trained with the spectral distance: the gradient reaches the bands
    z = y.clone().requires_grad_()
    loss = A.SpectralDistance().to(dev)(pq.invert(z), x)
    loss.sum().backward()
    assert z.grad is not None and z.grad.shape == z.shape
    assert bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0


def test_errors_on_the_device(dev):
    pq = _module(4, 65, dev)
    with pytest.raises(ValueError):
        pq(torch.zeros(2, 1001, device=dev))
    with pytest.raises(ValueError):
        pq.invert(torch.zeros(2, 5, 100, device=dev))
    with pytest.raises(A.AcidsHipError):
        pq(torch.zeros(2, 1000, device=dev, dtype=torch.float64))
    with pytest.raises(A.AcidsHipError):
        pq.invert(torch.zeros(2, 4, 250, device=dev, dtype=torch.float64))
    with A.allow_fp64_narrowing():
        assert pq(torch.zeros(2, 1000, device=dev, dtype=torch.float64)).dtype == torch.float32
    with pytest.raises(A.AcidsHipError):
        pq(torch.zeros(2, 1000))
    assert pq.prototype.is_cuda                       # a refused CPU tensor does not move the module
    # an empty batch and an empty clip are answered without a launch
    assert pq(torch.zeros(0, 1000, device=dev)).shape == (0, 4, 250)
    assert pq(torch.zeros(2, 0, device=dev)).shape == (2, 4, 0)
    assert pq.invert(torch.zeros(2, 4, 0, device=dev)).shape == (2, 0)

"""GPU side of the streaming PQMF (transforms.RealtimePQMF, autograd.PqmfStreamFunction / PqmfStreamInvertFunction, the
*_stream entries of csrc/pqmf.hip): the chunking does not matter to the bit (finite input), the state handling, parity
with the float64 restatement of pqmf_stream_cases.py within the library's normwise bound 1e-5, the gradients with the
state a constant, routing, errors and composition."""
import math

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import pqmf_cases as C
import pqmf_stream_cases as SC
from acids_transforms_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _bank(pq):
    return C.bank(pq.prototype.cpu().numpy(), pq.n_band)


def _tile(pq):
    return ops.pqmf_tile_blocks(pq.n_band, pq.taps)


def _forward_chunks(rt, x, blocks):
    outs, pos, M = [], 0, rt.n_band
    for b in blocks:
        outs.append(rt(x[..., pos:pos + b * M]))
        pos += b * M
    assert pos == x.shape[-1]
    return torch.cat(outs, -1)


def _invert_chunks(rt, y, blocks):
    outs, pos = [], 0
    for b in blocks:
        outs.append(rt.invert(y[..., pos:pos + b]))
        pos += b
    assert pos == y.shape[-1]
    return torch.cat(outs, -1)


@pytest.mark.parametrize("n_band,taps", SC.CASES)
def test_chunking_does_not_matter_to_the_bit(dev, n_band, taps):
    rt = A.RealtimePQMF(n_band=n_band, taps=taps).to(dev)
    pq = A.PQMF(n_band=n_band, taps=taps).to(dev)
    assert torch.equal(rt.prototype, pq.prototype)
    hk = _bank(rt)
    _, D, Ha, Hs = SC.sizes(n_band, taps)
    blocks = SC.chunk_blocks(Hs, _tile(rt))
    T = sum(blocks)
    x = C.audio((2, n_band * T), 100).float()
    xd = x.to(dev)
    chunked = _forward_chunks(rt, xd, blocks)
    assert rt.input_buffer.shape == (2, Ha) and torch.equal(rt.input_buffer, xd[:, -Ha:])
    rt.reset()
    whole = rt(xd)
    offline = pq(torch.cat([xd.new_zeros(2, D * n_band), xd], -1))[..., :T]
    assert chunked.shape == (2, n_band, T) and chunked.dtype == torch.float32
    assert torch.equal(chunked, whole) and torch.equal(chunked, offline)
    err_f = C.rel_max(chunked.cpu().numpy(), SC.stream_analysis(x.double(), hk, blocks).numpy())
    # invert, on planted band signals
    y = C.audio((2, n_band, T), 101).float()
    yd = y.to(dev)
    chunked = _invert_chunks(rt, yd, blocks)
    assert rt.band_buffer.shape == (2, n_band, Hs) and torch.equal(rt.band_buffer, yd[..., -Hs:])
    rt.reset()
    whole = rt.invert(yd)
    offline = pq.invert(torch.cat([yd.new_zeros(2, n_band, D), yd], -1))[..., :T * n_band]
    assert chunked.shape == (2, n_band * T) and chunked.dtype == torch.float32
    assert torch.equal(chunked, whole) and torch.equal(chunked, offline)
    err_i = C.rel_max(chunked.cpu().numpy(), SC.stream_synthesis(y.double(), hk, blocks).numpy())
    print("n_band %d taps %d blocks %s: forward %.2e invert %.2e" % (n_band, taps, blocks, err_f, err_i))
    assert err_f < TOL and err_i < TOL


def test_state_starts_from_zeros_and_streams_do_not_interact(dev):
    M, N = 3, 51
    a, b = A.RealtimePQMF(M, N).to(dev), A.RealtimePQMF(M, N).to(dev)
    x = C.audio((2, M * 40), 110).float().to(dev)
    z = C.audio((2, M * 40), 111).float().to(dev)
    first = a(x)
    # a new leading shape starts a new stream from zeros, and so does reset()
    assert torch.equal(a(x.reshape(2, 1, -1)), first.reshape(2, 1, M, 40))
    assert a.input_buffer.shape == (2, 1, a.input_buffer.shape[-1])
    assert not torch.equal(a(x.reshape(2, 1, -1)), first.reshape(2, 1, M, 40))        # the second chunk of that stream
    a.reset()
    assert torch.equal(a(x), first)
    fi = a.invert(first)
    assert torch.equal(a.invert(first.reshape(2, 1, M, 40)), fi.reshape(2, 1, -1))
    a.reset()
    assert torch.equal(a.invert(first), fi)
    # two modules interleaved on different streams are two streams
    a.reset()
    want_a = torch.cat([a(x[:, :M * 7]), a(x[:, M * 7:])], -1)
    want_b = torch.cat([b(z[:, :M * 30]), b(z[:, M * 30:])], -1)
    a.reset(), b.reset()
    a1, b1, a2, b2 = a(x[:, :M * 7]), b(z[:, :M * 30]), a(x[:, M * 7:]), b(z[:, M * 30:])
    assert torch.equal(torch.cat([a1, a2], -1), want_a) and torch.equal(torch.cat([b1, b2], -1), want_b)
    ya, yb = a.invert(a1), b.invert(b1)
    ya2, yb2 = a.invert(a2), b.invert(b2)
    a.reset(), b.reset()
    assert torch.equal(torch.cat([ya, ya2], -1), a.invert(want_a)) and torch.equal(torch.cat([yb, yb2], -1), b.invert(want_b))


def test_a_stream_does_not_depend_on_its_batch_and_a_nan_stays_in_its_row(dev):
    M, N = 16, 513
    _, D, Ha, Hs = SC.sizes(M, N)
    rt, solo = A.RealtimePQMF(M, N).to(dev), A.RealtimePQMF(M, N).to(dev)
    blocks = [3, Hs + 40, 5, 70]
    T = sum(blocks)
    x = C.audio((5, M * T), 120).float().to(dev)
    z = C.audio((5, M, T), 121).float().to(dev)
    y, xh = _forward_chunks(rt, x, blocks), _invert_chunks(rt, z, blocks)
    for row in (0, 3, 4):
        solo.reset()
        assert torch.equal(_forward_chunks(solo, x[row:row + 1], blocks), y[row:row + 1])
        assert torch.equal(_invert_chunks(solo, z[row:row + 1], blocks), xh[row:row + 1])
    # a NaN in row 2, in the second chunk: the other rows keep their bits, the row itself is finite again once the NaN
    # has left the window -- Ha + 2M samples (analysis), Hs + 2 blocks (synthesis) later
    s_nan, b_nan = M * 3 + 37, 3 + 4
    x[2, s_nan] = float("nan")
    z[2, 5, b_nan] = float("nan")
    rt.reset()
    yn, xn = _forward_chunks(rt, x, blocks), _invert_chunks(rt, z, blocks)
    keep = [0, 1, 3, 4]
    assert torch.equal(yn[keep], y[keep]) and torch.equal(xn[keep], xh[keep])
    assert bool(torch.isnan(yn[2]).any()) and bool(torch.isnan(xn[2]).any())
    t_clean = -(-(s_nan + Ha + 2 * M) // M)
    assert t_clean < T and torch.equal(yn[2, :, t_clean:], y[2, :, t_clean:])
    m_clean = M * (b_nan + Hs + 2)
    assert m_clean < M * T and torch.equal(xn[2, m_clean:], xh[2, m_clean:])
    assert bool(torch.isfinite(rt.input_buffer).all()) and bool(torch.isfinite(rt.band_buffer).all())


def test_round_trip(dev):
    for n_band, taps in ((4, 65), (16, 513)):
        rt = A.RealtimePQMF(n_band, taps).to(dev)
        hk = _bank(rt)
        T = (4 * taps) // n_band + 8 + rt.latency // n_band
        blocks = [1, 2, T - 3 - 50, 50]
        x = C.audio((2, n_band * T), 130).float()
        xh = _invert_chunks(rt, _forward_chunks(rt, x.to(dev), blocks), blocks).cpu().numpy()
        want = SC.stream_synthesis(SC.stream_analysis(x.double(), hk, blocks), hk, blocks).numpy()
        lat = rt.latency
        print("n_band %d taps %d: round trip against float64 %.2e, interior relative rms against x delayed by %d: %.3e"
              % (n_band, taps, C.rel_max(xh, want), lat, C.interior_rel_rms(xh[..., lat:], x.numpy()[..., :-lat], taps)))
        assert C.rel_max(xh, want) < TOL


@pytest.mark.parametrize("n_band,taps,blocks", SC.GRAD)
def test_gradients_on_the_second_chunk_match_float64_autograd(dev, n_band, taps, blocks):
    rt = A.RealtimePQMF(n_band, taps).to(dev)
    hk, tile = _bank(rt), _tile(rt)
    _, D, Ha, Hs = SC.sizes(n_band, taps)
    c = {"1": 1, "tile+1": tile + 1}[blocks]
    c0 = Hs + 3                                                                   # the first chunk fills both states
    x0, x, gy = C.audio((2, n_band * c0), 140).float(), C.audio((2, n_band * c), 141).float(), C.audio((2, n_band, c), 142).float()
    z0, z, gx = C.audio((2, n_band, c0), 143).float(), C.audio((2, n_band, c), 144).float(), C.audio((2, n_band * c), 145).float()
    # forward
    rt(x0.to(dev))
    state = rt.input_buffer.clone()
    assert bool(state.any())
    xr = x.to(dev).requires_grad_()
    y = rt(xr)
    assert not rt.input_buffer.requires_grad and rt.input_buffer.grad_fn is None
    (y * gy.to(dev)).sum().backward()
    xd = x.double().requires_grad_()
    yd, _ = SC.analysis_chunk(xd, state.cpu().double(), hk)
    (yd * gy.double()).sum().backward()
    err_y, err_f = C.rel_max(y.detach().cpu().numpy(), yd.detach().numpy()), C.rel_max(xr.grad.cpu().numpy(), xd.grad.numpy())
    # the transpose identity in fp32, <f(x), g> = <x, f*(g)>, with the state's share f(0) taken off f(x): the difference
    # of two fp32 outputs is rounded at the size of f(x), so the bound is 1e-5 of |f(x)| |g| (at c = 1 the chunk's own
    # share of the output is the filter's outermost taps, orders of magnitude below the state's)
    rt.input_buffer = state.clone()
    y_zero = rt(torch.zeros_like(xr))
    lin = (y.detach() - y_zero).double()
    lhs, rhs = float((lin * gy.to(dev).double()).sum()), float((x.to(dev).double() * xr.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(y.detach().double().norm() * gy.double().norm())
    # invert
    rt.invert(z0.to(dev))
    bstate = rt.band_buffer.clone()
    assert bool(bstate.any())
    zr = z.to(dev).requires_grad_()
    xh = rt.invert(zr)
    assert not rt.band_buffer.requires_grad and rt.band_buffer.grad_fn is None
    (xh * gx.to(dev)).sum().backward()
    zd = z.double().requires_grad_()
    xhd, _ = SC.synthesis_chunk(zd, bstate.cpu().double(), hk)
    (xhd * gx.double()).sum().backward()
    err_x, err_i = C.rel_max(xh.detach().cpu().numpy(), xhd.detach().numpy()), C.rel_max(zr.grad.cpu().numpy(), zd.grad.numpy())
    rt.band_buffer = bstate.clone()
    x_zero = rt.invert(torch.zeros_like(zr))
    lin = (xh.detach() - x_zero).double()
    lhs, rhs = float((lin * gx.to(dev).double()).sum()), float((z.to(dev).double() * zr.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(xh.detach().double().norm() * gx.double().norm())
    print("n_band %d taps %d c %d: forward %.2e d forward %.2e invert %.2e d invert %.2e"
          % (n_band, taps, c, err_y, err_f, err_x, err_i))
    assert xr.grad.shape == x.shape and zr.grad.shape == z.shape
    assert max(err_y, err_f, err_x, err_i) < TOL
    # a second backward, on a later chunk of the same streams, does not raise: the state carries no graph
    xr2, zr2 = x.to(dev).requires_grad_(), z.to(dev).requires_grad_()
    (rt(xr2).sum() + rt.invert(zr2).sum()).backward()
    assert xr2.grad is not None and zr2.grad is not None
    # a gradient reaches the caller's own, non-contiguous tensors (a chunk's first samples are read D blocks later: the
    # chunk is long enough to hold blocks that read it)
    wide = torch.zeros(2, 2 * n_band * (c + D + 1), device=dev).requires_grad_()
    rt(wide[:, ::2]).sum().backward()
    assert wide.grad is not None and bool((wide.grad[:, 1::2] == 0).all()) and bool((wide.grad[:, ::2] != 0).any())
    bands = torch.zeros(2, c, n_band, device=dev).requires_grad_()
    rt.invert(bands.transpose(-1, -2)).sum().backward()
    assert bands.grad is not None and bands.grad.shape == bands.shape and bool((bands.grad != 0).any())


def test_routing(dev):
    rt, plain = A.RealtimePQMF(4, 65).to(dev), A.RealtimePQMF(4, 65).to(dev)
    x0, x = C.audio((2, 200), 150).float().to(dev), C.audio((2, 400), 151).float().to(dev)
    z0, z = C.audio((2, 4, 50), 152).float().to(dev), C.audio((2, 4, 100), 153).float().to(dev)
    for m in (rt, plain):
        m(x0), m.invert(z0)
    xr, zr = x.clone().requires_grad_(), z.clone().requires_grad_()
    y, xh = rt(xr), rt.invert(zr)
    assert y.grad_fn is not None and xh.grad_fn is not None
    # the plain route's bits, of the outputs and of the new state
    assert torch.equal(y.detach(), plain(x)) and torch.equal(xh.detach(), plain.invert(z))
    assert torch.equal(rt.input_buffer, plain.input_buffer) and torch.equal(rt.band_buffer, plain.band_buffer)
    assert plain(x).grad_fn is None and plain.invert(z).grad_fn is None
    with torch.no_grad():
        assert rt(xr).grad_fn is None and rt.invert(zr).grad_fn is None
    # the graph keeps no tensor
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        rt(xr), rt.invert(zr)
    assert saved == []
    # first order only
    for fn, leaf in ((rt, xr), (rt.invert, zr)):
        with pytest.raises(RuntimeError):
            (g,) = torch.autograd.grad(fn(leaf).square().sum(), leaf, create_graph=True)
            g.sum().backward()
    # forward_with_time moves the time stamps back by the analysis delay
    _, tm = rt.forward_with_time(x, torch.ones(2, device=dev))
    assert torch.allclose(tm.cpu(), torch.full((2,), 1.0 - rt.analysis_delay / rt.sr))


def test_errors_on_the_device(dev):
    rt = A.RealtimePQMF(4, 65).to(dev)
    rt(C.audio((2, 1000), 160).float().to(dev)), rt.invert(C.audio((2, 4, 250), 161).float().to(dev))
    state, bstate = rt.input_buffer.clone(), rt.band_buffer.clone()
    with pytest.raises(ValueError):
        rt(torch.zeros(2, 1001, device=dev))
    with pytest.raises(ValueError):
        rt.invert(torch.zeros(2, 5, 100, device=dev))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 1000, device=dev, dtype=torch.float64))
    with pytest.raises(A.AcidsHipError):
        rt.invert(torch.zeros(2, 4, 250, device=dev, dtype=torch.float64))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 1000))
    assert rt.prototype.is_cuda                       # a refused CPU tensor does not move the module
    # an empty batch and an empty chunk are answered without a launch and leave the state alone
    assert rt(torch.zeros(0, 1000, device=dev)).shape == (0, 4, 250)
    assert rt(torch.zeros(2, 0, device=dev)).shape == (2, 4, 0)
    assert rt.invert(torch.zeros(2, 4, 0, device=dev)).shape == (2, 0)
    assert rt.invert(torch.zeros(0, 4, 9, device=dev)).shape == (0, 36)
    assert torch.equal(rt.input_buffer, state) and torch.equal(rt.band_buffer, bstate)
    with A.allow_fp64_narrowing():
        assert rt(torch.zeros(2, 1000, device=dev, dtype=torch.float64)).dtype == torch.float32
        assert rt.invert(torch.zeros(2, 4, 250, device=dev, dtype=torch.float64)).dtype == torch.float32
    # the ops refuse a state of another stream's shape
    with pytest.raises(AssertionError):
        ops.pqmf_analysis_stream(torch.zeros(2, 8, device=dev), torch.zeros(3, rt.input_buffer.shape[-1], device=dev),
                                 rt.prototype, rt.modulation)


def test_composition(dev):
    chain = A.RealtimePQMF(4, 65).to(dev) + A.RealtimePQMF(2, 9).to(dev)
    assert isinstance(chain, A.ComposeAudioTransform) and chain.ratio == 8
    rt_chain = chain.realtime()
    assert rt_chain[0] is chain[0] and rt_chain[1] is chain[1]
    assert chain(torch.zeros(2, 64, device=dev)).shape == (2, 4, 2, 8)
    alone = A.ComposeAudioTransform([A.RealtimePQMF(4, 65).to(dev)])
    x = C.audio((2, 4096), 170).float().to(dev)
    y = torch.cat([alone(x[:, :1024]), alone(x[:, 1024:])], -1)
    assert y.shape == (2, 4, 1024)
    xh = torch.cat([alone.invert(y[..., :100], inversion_mode=None), alone.invert(y[..., 100:], inversion_mode=None)], -1)
    assert xh.shape == (2, 4096)
    ref = A.RealtimePQMF(4, 65).to(dev)
    assert torch.equal(y, ref(x)) and torch.equal(xh, ref.invert(y))

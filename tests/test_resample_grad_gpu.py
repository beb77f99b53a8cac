"""GPU side of the differentiable and the streaming Resample (utils.Resample / RealtimeResample, autograd.ResampleFunction /
ResampleStreamFunction, at_resample_sinc_backward / at_resample_sinc_stream of csrc/resample.hip): parity of the adjoint
with float64 autograd of the conv1d model of resample_cases.py within the library's normwise bound 1e-5 on every plan the
kernel takes, the bit-level properties that follow from one ordered fmaf chain per input sample, the stream against the
delayed offline call to the bit, its state handling and its gradient with the state a constant, routing and errors."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import resample_cases as C
from acids_transforms_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _bank(orig, new, dev):
    h, width = C.bank(orig, new)
    return h.to(dev), width


def _chunks(rt, x, blocks):
    outs, pos = [], 0
    for b in blocks:
        outs.append(rt(x[..., pos:pos + b * rt.orig]))
        pos += b * rt.orig
    assert pos == x.shape[-1]
    return torch.cat(outs, -1)


def test_resample_carries_a_gradient(dev):
    x = C.audio((2, 50), 1).float().to(dev).requires_grad_()
    y = A.Resample(3, 2)(x)
    assert y.grad_fn is not None and "ResampleFunction" in type(y.grad_fn).__name__
    y.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool((x.grad != 0).any())


@pytest.mark.parametrize("orig,new", C.RATIOS)
def test_the_adjoint_matches_float64_autograd_of_the_model(dev, orig, new):
    hd, width = _bank(orig, new, dev)
    rs = A.Resample(orig, new).to(dev)
    tb, in_lds = C.plan(orig, new)
    worst_op = worst_mod = worst_fwd = 0.0
    for L in C.lengths(orig, new):
        for lead in C.LEADS:
            x, g, want = C.model_case(orig, new, L, lead)
            rows = int(np.prod(lead))
            got = ops.resample_sinc_backward(g.float().to(dev).reshape(rows, -1), L, orig, new, 2 * width + orig, width, hd)
            assert got.shape == (rows, L) and got.dtype == torch.float32
            worst_op = max(worst_op, C.rel_max(got.cpu().numpy().reshape(lead + (L,)), want.numpy()))
            xr = x.float().to(dev).requires_grad_()
            y = rs(xr)
            assert y.shape == lead + (C.out_len(L, orig, new),)
            (y * g.float().to(dev)).sum().backward()
            assert xr.grad.shape == lead + (L,)
            worst_mod = max(worst_mod, C.rel_max(xr.grad.cpu().numpy(), want.numpy()))
            worst_fwd = max(worst_fwd, C.rel_max(y.detach().cpu().numpy(), C.model(x, orig, new).numpy()))
    print("(%d, %d) tile %d blocks, bank in LDS %s: ops %.2e module %.2e forward %.2e"
          % (orig, new, tb, in_lds, worst_op, worst_mod, worst_fwd))
    assert worst_op < TOL and worst_mod < TOL and worst_fwd < TOL


@pytest.mark.parametrize("orig,new", ((3, 2), (147, 160), (441, 160)))
def test_bits(dev, orig, new):
    hd, width = _bank(orig, new, dev)
    taps = 2 * width + orig
    rs = A.Resample(orig, new).to(dev)
    tb = C.plan(orig, new)[0]
    L = 3 * tb * orig + 5
    olen = C.out_len(L, orig, new)
    x = C.audio((3, L), 40).float().to(dev)
    g = C.audio((3, olen), 41).float().to(dev)
    # forward values under autograd are the no-grad call's
    plain = rs(x)
    assert plain.grad_fn is None
    xr = x.clone().requires_grad_()
    routed = rs(xr)
    assert routed.grad_fn is not None and torch.equal(routed.detach(), plain)
    assert torch.equal(plain, ops.resample_sinc(x, orig, new, width, hd))
    # a row alone is the same row in a batch of 3
    gx = ops.resample_sinc_backward(g, L, orig, new, taps, width, hd)
    for row in range(3):
        assert torch.equal(ops.resample_sinc_backward(g[row:row + 1], L, orig, new, taps, width, hd), gx[row:row + 1])
    # g == 0 gives exactly 0
    assert not ops.resample_sinc_backward(torch.zeros_like(g), L, orig, new, taps, width, hd).any()
    # a NaN in one row of g stays in its row
    gn = g.clone()
    gn[1, olen // 2] = float("nan")
    gxn = ops.resample_sinc_backward(gn, L, orig, new, taps, width, hd)
    assert torch.equal(gxn[[0, 2]], gx[[0, 2]]) and bool(torch.isnan(gxn[1]).any())
    if (orig, new) == (441, 160):
        return
    # away from both ends, g shifted by new is gx shifted by orig, to the bit: across block, tile and workgroup places
    s = 1
    shifted = torch.zeros_like(g)
    shifted[:, s * new:] = g[:, :olen - s * new]
    gxs = ops.resample_sinc_backward(shifted, L, orig, new, taps, width, hd)
    reach = -(-taps // orig) + 1                        # blocks over which an end is felt
    lo, hi = (s + reach) * orig, L - (s + reach) * orig
    assert hi - lo > tb * orig
    assert torch.equal(gxs[:, lo:hi], gx[:, lo - s * orig:hi - s * orig])


def test_routing_and_errors(dev):
    rs = A.Resample(3, 2).to(dev)
    xr = C.audio((2, 2, 40), 50).float().to(dev).requires_grad_()
    with torch.no_grad():
        assert rs(xr).grad_fn is None
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = rs(xr)
    assert saved == []                                  # the graph keeps no tensor
    with pytest.raises(RuntimeError):                   # first order only
        (gr,) = torch.autograd.grad(rs(xr).square().sum(), xr, create_graph=True)
        gr.sum().backward()
    # a gradient reaches the caller's own, non-contiguous tensor
    wide = torch.zeros(2, 80, device=dev).requires_grad_()
    rs(wide[:, ::2]).sum().backward()
    assert bool((wide.grad[:, 1::2] == 0).all()) and bool((wide.grad[:, ::2] != 0).any())
    # equal rates: the identity, and torch carries the gradient
    leaf = torch.ones(2, 8, device=dev, requires_grad=True)
    A.Resample(5, 5)(leaf).sum().backward()
    assert torch.equal(leaf.grad, torch.ones_like(leaf))
    # what the forward raises, the grad route raises
    with pytest.raises(A.AcidsHipError):
        rs(torch.zeros(2, 40, requires_grad=True))
    with pytest.raises(A.AcidsHipError):
        rs(torch.zeros(2, 40, device=dev, dtype=torch.float64, requires_grad=True))
    with A.allow_fp64_narrowing():
        x64 = torch.ones(2, 40, device=dev, dtype=torch.float64, requires_grad=True)
        y = rs(x64)
        y.sum().backward()
        assert y.dtype == torch.float32 and x64.grad.dtype == torch.float64
    with pytest.raises(A.AcidsHipError):
        ops.resample_sinc_backward(torch.zeros(2, 27), 40, 3, 2, 23, 10, rs.kernel)
    rt = rs.streaming()
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 9))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 9, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        rt(torch.zeros(2, 10, device=dev))
    assert rt(torch.zeros(2, 0, device=dev)).shape == (2, 0) and rt(torch.zeros(0, 9, device=dev)).shape == (0, 6)
    assert rt.input_buffer.shape == (22,)               # refused and empty calls leave the state


@pytest.mark.parametrize("orig,new", C.STREAM_RATIOS)
def test_the_chunking_of_a_stream_does_not_matter_to_the_bit(dev, orig, new):
    rs = A.Resample(orig, new).to(dev)
    rt = rs.streaming()
    assert rt.kernel is rs.kernel and rt.input_buffer.device.type == "cuda"
    D, Ha = C.stream_sizes(orig, new)
    blocks = C.STREAM_BLOCKS[(orig, new)]
    T = sum(blocks)
    x = C.audio((3, T * orig), 60).float()
    xd = x.to(dev)
    offline = rs(torch.cat([xd.new_zeros(3, D * orig), xd], -1))[..., :T * new]
    outs = {}
    for name, cut in (("mixed", blocks), ("single blocks", (1,) * T), ("one call", (T,))):
        rt.reset()
        outs[name] = _chunks(rt, xd, cut)
        assert outs[name].shape == (3, T * new) and outs[name].dtype == torch.float32
        assert torch.equal(outs[name], offline), name
        assert rt.input_buffer.shape == (3, Ha)
        assert torch.equal(rt.input_buffer, torch.cat([xd.new_zeros(3, Ha), xd], -1)[:, -Ha:])
    err = C.rel_max(offline.cpu().numpy(), C.delayed(x.double(), orig, new).numpy())
    print("(%d, %d) blocks %s: stream against the float64 model %.2e" % (orig, new, blocks, err))
    assert err < TOL
    # a stream's bits do not depend on its batch; a new leading shape starts a new stream
    solo = A.RealtimeResample(orig, new).to(dev)
    for row in (0, 2):
        solo.reset()
        assert torch.equal(_chunks(solo, xd[row:row + 1], blocks), offline[row:row + 1])
    first = solo(xd[:, :orig])
    assert torch.equal(solo(xd[:, :orig].reshape(3, 1, orig)), first.reshape(3, 1, new))
    assert solo.input_buffer.shape == (3, 1, Ha)


def test_reset_and_a_state_dict_round_trip(dev):
    a, b = A.RealtimeResample(3, 2).to(dev), A.RealtimeResample(3, 2).to(dev)
    x = C.audio((2, 2, 90), 70).float().to(dev)
    first = a(x[..., :30])
    b.load_state_dict(a.state_dict())
    assert b.input_buffer.shape == (2, 2, 22) and torch.equal(b.input_buffer, a.input_buffer)
    assert torch.equal(a(x[..., 30:]), b(x[..., 30:]))
    a.reset()
    assert not a.input_buffer.any() and torch.equal(a(x[..., :30]), first)


@pytest.mark.parametrize("orig,new", C.STREAM_RATIOS)
def test_the_gradient_of_a_chunk_with_the_state_a_constant(dev, orig, new):
    rt = A.RealtimeResample(orig, new).to(dev)
    D, Ha = C.stream_sizes(orig, new)
    tb = C.plan(orig, new, Ha)[0]
    x0 = C.audio((2, (D + 2) * orig), 80).float().to(dev).requires_grad_()
    rt(x0)                                                         # the first chunk fills the state
    state = rt.input_buffer.clone()
    assert bool(state.any()) and not rt.input_buffer.requires_grad and rt.input_buffer.grad_fn is None
    for c in (1, tb + 1):
        x, g = C.audio((2, c * orig), 81 + c), C.audio((2, c * new), 82 + c)
        rt.input_buffer = state.clone()
        xr = x.float().to(dev).requires_grad_()
        y = rt(xr)
        assert "ResampleStreamFunction" in type(y.grad_fn).__name__
        (y * g.float().to(dev)).sum().backward()
        xd = x.float().double().requires_grad_()
        yd, sd = C.stream_chunk(xd, state.cpu().double(), orig, new)
        (yd * g.float().double()).sum().backward()
        err_y, err_g = C.rel_max(y.detach().cpu().numpy(), yd.detach().numpy()), C.rel_max(xr.grad.cpu().numpy(), xd.grad.numpy())
        print("(%d, %d) c %d: forward %.2e gradient %.2e" % (orig, new, c, err_y, err_g))
        assert err_y < TOL and err_g < TOL
        assert torch.equal(rt.input_buffer.cpu(), sd.float())
        # the state's share of the gradient is exactly zero: from a zero state the same bits
        rt.reset()
        xz = x.float().to(dev).requires_grad_()
        (rt(xz) * g.float().to(dev)).sum().backward()
        assert torch.equal(xz.grad, xr.grad)
    assert x0.grad is None                                         # nothing reached the previous chunk's tensor
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        rt(xr)
    assert saved == []
    with pytest.raises(RuntimeError):
        (gr,) = torch.autograd.grad(rt(xr).square().sum(), xr, create_graph=True)
        gr.sum().backward()

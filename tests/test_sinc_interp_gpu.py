"""GPU side of the bankless sample-rate converter (ops.resample_direct / resample_direct_backward, Resample(direct=True),
autograd.ResampleDirectFunction, at_sinc_interp of csrc/sinc_interp.hip): parity of both directions with the float64 gather
of sinc_interp_cases.py within the library's normwise bound 1e-5 on every tile cut and both table placements, the bits of
the bank route where a bank exists, and the properties that follow from one ordered fmaf chain per output."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import sinc_interp_cases as C
from acids_transforms_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _lengths(orig, new):
    if (orig, new) == C.BIG:
        return (1, 2, orig - 1, orig, orig + 1) + C.BIG_LENGTHS
    return C.lengths(orig, new)


@pytest.mark.parametrize("orig,new", C.RATIOS + (C.BIG,))
def test_both_directions_match_the_float64_model(dev, orig, new):
    rs = A.Resample(orig, new, direct=True).to(dev)
    assert not hasattr(rs, "kernel") and rs.table.device.type == "cuda"
    Qi = C.table(orig, new)[1]
    (tf, lds_f), (tb, lds_b) = C.plan(orig, new, Qi), C.plan(new, orig, Qi)
    worst = dict(fwd=0.0, bwd=0.0, mod=0.0, grad=0.0)
    for L in _lengths(orig, new):
        for lead in (C.LEADS if L < 30000 else C.LEADS[:1]):
            x, g, y, gx = C.case(orig, new, L, lead)
            olen = C.out_len(L, orig, new)
            xd, gd = x.float().to(dev), g.float().to(dev)
            got = ops.resample_direct(xd, orig, new)
            assert got.shape == lead + (olen,) and got.dtype == torch.float32
            worst["fwd"] = max(worst["fwd"], C.rel_max(got.cpu().numpy(), y.numpy()))
            back = ops.resample_direct_backward(gd, L, orig, new)
            assert back.shape == lead + (L,) and back.dtype == torch.float32
            worst["bwd"] = max(worst["bwd"], C.rel_max(back.cpu().numpy(), gx.numpy()))
            plain = rs(xd)
            assert plain.grad_fn is None and torch.equal(plain, got)
            xr = xd.clone().requires_grad_()
            routed = rs(xr)
            assert routed.shape == lead + (olen,) and torch.equal(routed.detach(), got)
            (routed * gd).sum().backward()
            assert xr.grad.shape == lead + (L,) and torch.equal(xr.grad, back)
            worst["mod"] = max(worst["mod"], C.rel_max(routed.detach().cpu().numpy(), y.numpy()))
            worst["grad"] = max(worst["grad"], C.rel_max(xr.grad.cpu().numpy(), gx.numpy()))
    print("(%d, %d) forward tile %d, table in LDS %s; backward tile %d, table in LDS %s: %s"
          % (orig, new, tf, lds_f, tb, lds_b, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


@pytest.mark.parametrize("orig,new", C.RATIOS)
def test_the_bits_of_the_bank_route(dev, orig, new):
    bank, direct = A.Resample(orig, new).to(dev), A.Resample(orig, new, direct=True).to(dev)
    for L in C.lengths(orig, new):
        for lead in C.LEADS:
            x, g, _, _ = C.case(orig, new, L, lead)
            xd, gd = x.float().to(dev), g.float().to(dev)
            want = bank(xd)
            assert torch.equal(ops.resample_direct(xd, orig, new), want), (L, lead)
            assert torch.equal(direct(xd), want), (L, lead)
            xa, xb = xd.clone().requires_grad_(), xd.clone().requires_grad_()
            (bank(xa) * gd).sum().backward()
            (direct(xb) * gd).sum().backward()
            assert torch.equal(xa.grad, xb.grad), (L, lead)
            assert torch.equal(ops.resample_direct_backward(gd, L, orig, new), xa.grad), (L, lead)


@pytest.mark.parametrize("orig,new", C.RATIOS + (C.BIG,))
def test_the_backward_is_the_adjoint_to_the_bit_of_the_coefficients(dev, orig, new):
    """<A x, g> and <x, A^T g>, accumulated in float64 from the float32 results, use the same products table[|q|] x[n] g[o];
    they differ by the rounding of the float32 chains alone, a few 2^-24 of sum |A x| |g|: 1e-6 of it bounds that."""
    worst = 0.0
    for L in _lengths(orig, new):
        x, g, _, _ = C.case(orig, new, L, (3,))
        xd, gd = x.float().to(dev), g.float().to(dev)
        y = ops.resample_direct(xd, orig, new).double()
        gx = ops.resample_direct_backward(gd, L, orig, new).double()
        lhs, rhs = float((y * gd.double()).sum()), float((xd.double() * gx).sum())
        scale = float((y.abs() * gd.double().abs()).sum()) or 1.0
        worst = max(worst, abs(lhs - rhs) / scale)
    print("(%d, %d): <A x, g> against <x, A^T g>, worst %.2e" % (orig, new, worst))
    assert worst < 1e-6


def test_a_row_does_not_depend_on_its_batch(dev):
    orig, new, L = 3, 2, 8
    olen = C.out_len(L, orig, new)
    x = C.audio((1, L), 70).float().to(dev)
    g = C.audio((1, olen), 71).float().to(dev)
    y1, gx1 = ops.resample_direct(x, orig, new), ops.resample_direct_backward(g, L, orig, new)
    for rows in (3, 70000):                                        # past the 65535 rows of a grid's second axis
        noise = C.audio((rows, L), 72).float().to(dev)
        noise[rows - 1] = x[0]
        yb = ops.resample_direct(noise, orig, new)
        assert yb.shape == (rows, olen) and torch.equal(yb[rows - 1], y1[0])
        noise = C.audio((rows, olen), 73).float().to(dev)
        noise[rows // 2] = g[0]
        gb = ops.resample_direct_backward(noise, L, orig, new)
        assert gb.shape == (rows, L) and torch.equal(gb[rows // 2], gx1[0])
    # nor on the tile it falls into: the same clip as the head of a longer one, away from the longer one's extra samples
    orig, new = 147, 160
    Qi = C.table(orig, new)[1]
    tile = C.plan(orig, new, Qi)[0]
    long = C.audio((1, 4 * tile), 74).float().to(dev)
    head = long[:, :2 * tile].contiguous()
    ya, yb = ops.resample_direct(long, orig, new), ops.resample_direct(head, orig, new)
    clean = (2 * tile * new - Qi) // orig - 1                      # outputs below it reach no sample past the head
    assert clean > tile and torch.equal(ya[:, :clean], yb[:, :clean])


@pytest.mark.parametrize("orig,new", ((3, 2), (147, 160), (441, 160), C.BIG))
def test_bad_values_stay_where_they_are(dev, orig, new):
    Qi = C.table(orig, new)[1]
    L = 2 * orig + 7 if (orig, new) != C.BIG else C.BIG_LENGTHS[0]
    olen = C.out_len(L, orig, new)
    zeros = torch.zeros(3, L, device=dev)
    out = ops.resample_direct(zeros, orig, new)
    assert out.shape == (3, olen) and not out.any() and not torch.signbit(out).any()          # exactly +0
    back = ops.resample_direct_backward(torch.zeros(3, olen, device=dev), L, orig, new)
    assert not back.any() and not torch.signbit(back).any()
    x = C.audio((3, L), 80).float().to(dev)
    clean = ops.resample_direct(x, orig, new)
    for n in (0, L // 2, L - 1):
        bad = x.clone()
        bad[1, n] = float("nan")
        got = ops.resample_direct(bad, orig, new)
        o = torch.arange(olen, device=dev, dtype=torch.int64)
        reach = (n * new - o * orig).abs() <= Qi
        assert bool(reach.any())
        assert torch.equal(torch.isnan(got[1]), reach)                                  # there, and only there
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[1] = ~reach
        assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32))  # everything else to the bit
    g = C.audio((3, olen), 81).float().to(dev)
    clean = ops.resample_direct_backward(g, L, orig, new)
    bad = g.clone()
    bad[2, olen // 2] = float("nan")
    got = ops.resample_direct_backward(bad, L, orig, new)
    n = torch.arange(L, device=dev, dtype=torch.int64)
    reach = (n * new - (olen // 2) * orig).abs() <= Qi
    assert torch.equal(torch.isnan(got[2]), reach)
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[2] = ~reach
    assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32))


def test_routing_and_errors(dev):
    rs = A.Resample(147, 160, direct=True).to(dev)
    x = C.audio((2, 300), 90).float().to(dev).requires_grad_()
    y = rs(x)
    assert y.grad_fn is not None and "ResampleDirectFunction" in type(y.grad_fn).__name__
    assert not getattr(y.grad_fn, "saved_tensors", ())                                  # the graph keeps no tensor
    with torch.no_grad():
        assert rs(x).grad_fn is None
    w = torch.ones_like(y, requires_grad=True)
    (gx,) = torch.autograd.grad((y * w).sum(), x, create_graph=True)                    # first order only
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    with pytest.raises(A.AcidsHipError):
        rs(x.detach().double())
    with pytest.raises(A.AcidsHipError):
        ops.resample_direct(x.detach().double(), 147, 160)
    with A.allow_fp64_narrowing():
        assert torch.equal(rs(x.detach().double()), y.detach())
    assert ops.resample_direct(x, 48000, 48000) is x
    # gcd reduction, and one upload per converter and device
    assert torch.equal(ops.resample_direct(x.detach(), 44100, 48000), y.detach())
    assert ops._sinc_table_on(x.device, 147, 160)[0] is ops._sinc_table_on(x.device, 147, 160)[0]
    # empty work launches nothing
    assert ops.resample_direct(torch.zeros(0, 300, device=dev), 147, 160).shape == (0, 327)
    assert ops.resample_direct(torch.zeros(2, 0, device=dev), 147, 160).shape == (2, 0)
    # a module moved to the device keeps its table with it, and a half input widens
    assert torch.equal(rs(x.detach().half()), ops.resample_direct(x.detach().half().float(), 147, 160))

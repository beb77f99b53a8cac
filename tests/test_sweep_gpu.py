"""GPU side of the plan-class sweep (sweep_cases.py): PQMF, Resample, the bankless sinc converter, the hop endings of the SOS
scan and the spectral FIR of FFTConvolve at the parameters whose plan classes the stages' own tables never reach -- the named
cases and 24 seeded parameter sets per stage -- parametrised by stage and case id.

Every case: parity of the forward and of the adjoint (or gradient) with the float64 model of the stage's `*_cases.py` within
that module's own bound (TOL = 1e-5 normwise, STATE_TOL for a carried SOS state); then the bit rules the project states, with
torch.equal: a row alone is the row in a batch of 3, a stream cut by a seeded chunk list is the one call (RealtimeSOSFilter:
within 1e-6 of it; RealtimePQMF also by pqmf_stream_cases.chunk_blocks; the gradient of a chunk of the two differentiable streams
with the carried state a constant), a NaN in one row leaves the bits of the others, zeros give +0; and for the hop endings and the two
converters the C entry on a buffer with a guard band on both sides: a shrunk tile must not write past a row.

T >= P in a full convolution, so the (P, T) of sweep_cases.FIR_NAMED with T < P run on at_spectral_fir / at_spectral_fir_corr
alone, which take T and P apart; end to end K = 128 P runs at the T the convolution can have (sweep_cases.fir_lengths).

Measured on an MI355X (smallest ... largest of the worst figures the tests print case by case; bound 1e-5; also in the README,
"Plan-class sweep" under each stage):
    PQMF, 31 (n_band, taps)        forward 1.0e-7 ... 6.1e-7, invert 1.1e-7 ... 4.1e-7, gradients 8.8e-8 ... 6.6e-7
    RealtimePQMF                   forward 9.9e-8 ... 5.4e-7, invert 1.0e-7 ... 3.5e-7, chunk gradients 7.4e-8 ... 4.4e-7
    Resample, 29 ratios            forward 1.6e-7 ... 9.6e-7, backward 1.5e-7 ... 1.0e-6
    RealtimeResample, 3 ratios     the stream 1.8e-7 ... 2.1e-7, chunk gradients (the backward plan at lead = Ha) 5.7e-7 ... 1.3e-6
    sinc converter, 34 ratios      forward 1.8e-7 ... 1.5e-6, backward 1.7e-7 ... 1.2e-6
    PitchShift +60 / -60 steps     converter forward 5.9e-7 / 1.6e-7, backward 1.9e-7 / 8.0e-7
    hop endings, 36 (L, hop) x 2   power at most 1.7e-10, scaled at most 5.3e-8
    RealtimeSOSFilter              4.9e-8 of the oracle, 5.0e-8 of the one call (bound 1e-6), state 8.8e-11
    spectral FIR, 36 (P, T)        2.9e-8 ... 2.7e-7 over the causal, the anticausal-conjugate and the correlation kernels
    FFTConvolve, P = 7, 9, 16, 17  forward 1.8e-7 ... 2.3e-7, gx 2.6e-7 ... 5.2e-7, gh 1.8e-7 ... 2.5e-7
    RealtimeImpulseResponse        2.3e-7 ... 3.0e-7
All 376 cases pass; the sweep exposed no bug."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import fft_convolve_cases as FC
import loudness_cases as LC
import pqmf_cases as PC
import pqmf_stream_cases as PS
import resample_cases as RC
import sinc_interp_cases as SI
import sos_filter_cases as SC
import sweep_cases as W
import test_pitch_shift_gpu as PT                  # the chain PitchShift is defined by lives there
from acids_transforms_amd import _lib, ops
from acids_transforms_amd.autograd import FFTConvolveFunction

pytestmark = pytest.mark.gpu
SR = 44100
GUARD = 4096
SENTINEL = 7.0
# the project's standing normwise bound, max|a - b| / max|b|: sos_filter_cases, loudness_cases and fft_convolve_cases name it,
# the GPU tests of PQMF, Resample and the sinc converter state the same figure
TOL = SC.TOL
assert TOL == LC.TOL == FC.TOL == 1e-5

PQ_CASES = W.PQ_NAMED + W.pqmf_generated()
RB_CASES = W.RB_NAMED + W.resample_generated()
SI_CASES = W.SI_NAMED + W.sinc_generated()
HOP_CASES = W.HOP_NAMED + W.hop_generated()
FIR_CASES = W.FIR_NAMED + W.fir_generated()


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _plus_zero(t):
    """Every element is +0: no bit set, the sign bit included."""
    return not bool(t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).any())


def _guarded(n, dtype, dev, fn):
    """fn(out) on n elements between two guard bands of a sentinel -> out; the bands must come back untouched."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    out = whole[GUARD:GUARD + n]
    fn(out)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all()), "guard band written"
    return out


# ---- PQMF ----------------------------------------------------------------------------------------------------------------------
def _pq_bank(pq):
    return PC.bank(_np(pq.prototype), pq.n_band)


@pytest.mark.parametrize("n_band,taps", PQ_CASES, ids=_ids(PQ_CASES))
def test_pqmf_forward_invert_and_gradients_match_float64(dev, n_band, taps):
    pq = A.PQMF(n_band=n_band, taps=taps).to(dev)
    hk, tile = _pq_bank(pq), ops.pqmf_tile_blocks(n_band, taps)
    worst = dict(forward=0.0, invert=0.0, d_forward=0.0, d_invert=0.0)
    for i, T in enumerate(PC.block_counts(tile)):
        x, gy = PC.audio((2, n_band * T), 500 + i).float(), PC.audio((2, n_band, T), 510 + i).float()
        z, gx = PC.audio((2, n_band, T), 520 + i).float(), PC.audio((2, n_band * T), 530 + i).float()
        xr, zr = x.to(dev).requires_grad_(), z.to(dev).requires_grad_()
        y, xh = pq(xr), pq.invert(zr)
        assert y.shape == (2, n_band, T) and xh.shape == (2, n_band * T)
        ((y * gy.to(dev)).sum() + (xh * gx.to(dev)).sum()).backward()
        xd, zd = x.double().requires_grad_(), z.double().requires_grad_()
        yd, xhd = PC.analysis(xd, hk), PC.synthesis(zd, hk)
        ((yd * gy.double()).sum() + (xhd * gx.double()).sum()).backward()
        for key, got, want in (("forward", y, yd), ("invert", xh, xhd), ("d_forward", xr.grad, xd.grad), ("d_invert", zr.grad, zd.grad)):
            worst[key] = max(worst[key], PC.rel_max(_np(got), _np(want)))
    print("pqmf (%d, %d) tile %d: %s" % (n_band, taps, tile, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


@pytest.mark.parametrize("n_band,taps", PQ_CASES, ids=_ids(PQ_CASES))
def test_pqmf_bit_rules(dev, n_band, taps):
    pq = A.PQMF(n_band=n_band, taps=taps).to(dev)
    T = ops.pqmf_tile_blocks(n_band, taps) + 1
    x, z = PC.audio((3, n_band * T), 540).float().to(dev), PC.audio((3, n_band, T), 541).float().to(dev)
    y, xh = pq(x), pq.invert(z)
    for r in range(3):
        assert torch.equal(pq(x[r:r + 1]), y[r:r + 1]) and torch.equal(pq.invert(z[r:r + 1]), xh[r:r + 1]), r
    bad_x, bad_z = x.clone(), z.clone()
    bad_x[1, n_band * T // 2] = float("nan")
    bad_z[1, n_band - 1, T // 2] = float("nan")
    yn, xn = pq(bad_x), pq.invert(bad_z)
    assert torch.equal(yn[[0, 2]], y[[0, 2]]) and torch.equal(xn[[0, 2]], xh[[0, 2]])
    assert bool(torch.isnan(yn[1]).any()) and bool(torch.isnan(xn[1]).any())
    assert _plus_zero(pq(torch.zeros_like(x))) and _plus_zero(pq.invert(torch.zeros_like(z)))


@pytest.mark.parametrize("n_band,taps", PQ_CASES, ids=_ids(PQ_CASES))
def test_pqmf_stream_is_the_one_call_to_the_bit(dev, n_band, taps):
    rt, pq = A.RealtimePQMF(n_band=n_band, taps=taps).to(dev), A.PQMF(n_band=n_band, taps=taps).to(dev)
    hk, tile = _pq_bank(rt), ops.pqmf_tile_blocks(n_band, taps)
    _, D, Ha, Hs = PS.sizes(n_band, taps)
    worst = dict(forward=0.0, invert=0.0)
    # three seeded lists, and the stage's own list: single blocks, a chunk shorter than the state, both sides of a tile edge
    for i, blocks in enumerate(W.chunk_lists((n_band, taps), tile) + (tuple(PS.chunk_blocks(Hs, tile)),)):
        T = sum(blocks)
        x, z = PC.audio((2, n_band * T), 550 + i).float(), PC.audio((2, n_band, T), 560 + i).float()
        xd, zd = x.to(dev), z.to(dev)
        rt.reset()
        pos, outs = 0, []
        for b in blocks:
            outs.append(rt(xd[:, pos:pos + b * n_band]))
            pos += b * n_band
        chunked = torch.cat(outs, -1)
        assert torch.equal(rt.input_buffer, torch.cat([xd.new_zeros(2, Ha), xd], -1)[:, -Ha:])
        rt.reset()
        assert torch.equal(chunked, rt(xd)), blocks
        assert torch.equal(chunked, pq(torch.cat([xd.new_zeros(2, D * n_band), xd], -1))[..., :T]), blocks
        worst["forward"] = max(worst["forward"], PC.rel_max(_np(chunked), PS.stream_analysis(x.double(), hk, blocks).numpy()))
        rt.reset()
        pos, outs = 0, []
        for b in blocks:
            outs.append(rt.invert(zd[..., pos:pos + b]))
            pos += b
        chunked = torch.cat(outs, -1)
        assert torch.equal(rt.band_buffer, torch.cat([zd.new_zeros(2, n_band, Hs), zd], -1)[..., -Hs:])
        rt.reset()
        assert torch.equal(chunked, rt.invert(zd)), blocks
        assert torch.equal(chunked, pq.invert(torch.cat([zd.new_zeros(2, n_band, D), zd], -1))[..., :T * n_band]), blocks
        worst["invert"] = max(worst["invert"], PC.rel_max(_np(chunked), PS.stream_synthesis(z.double(), hk, blocks).numpy()))
    print("pqmf stream (%d, %d): %s" % (n_band, taps, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


@pytest.mark.parametrize("n_band,taps", PQ_CASES, ids=_ids(PQ_CASES))
def test_pqmf_stream_gradients_of_a_chunk_match_float64(dev, n_band, taps):
    """The backward of a chunk is the stream kernel again (the other bank, shift = D, no state out), the carried state a
    constant: chunks of 1 block and on both sides of a tile edge behind a first chunk that fills both states."""
    rt = A.RealtimePQMF(n_band=n_band, taps=taps).to(dev)
    hk, tile = _pq_bank(rt), ops.pqmf_tile_blocks(n_band, taps)
    _, D, Ha, Hs = PS.sizes(n_band, taps)
    c0 = Hs + 3
    rt(PC.audio((2, n_band * c0), 570).float().to(dev))
    rt.invert(PC.audio((2, n_band, c0), 571).float().to(dev))
    state, bstate = rt.input_buffer.clone(), rt.band_buffer.clone()
    assert bool(state.any()) and bool(bstate.any())
    worst = dict(forward=0.0, d_forward=0.0, invert=0.0, d_invert=0.0)
    for c in (1, tile - 1, tile, tile + 1):
        x, gy = PC.audio((2, n_band * c), 572 + c).float(), PC.audio((2, n_band, c), 573 + c).float()
        z, gx = PC.audio((2, n_band, c), 574 + c).float(), PC.audio((2, n_band * c), 575 + c).float()
        rt.input_buffer, rt.band_buffer = state.clone(), bstate.clone()
        xr, zr = x.to(dev).requires_grad_(), z.to(dev).requires_grad_()
        y, xh = rt(xr), rt.invert(zr)
        assert not rt.input_buffer.requires_grad and not rt.band_buffer.requires_grad
        ((y * gy.to(dev)).sum() + (xh * gx.to(dev)).sum()).backward()
        xd, zd = x.double().requires_grad_(), z.double().requires_grad_()
        yd, _ = PS.analysis_chunk(xd, state.cpu().double(), hk)
        xhd, _ = PS.synthesis_chunk(zd, bstate.cpu().double(), hk)
        ((yd * gy.double()).sum() + (xhd * gx.double()).sum()).backward()
        assert xr.grad.shape == x.shape and zr.grad.shape == z.shape
        for key, got, want in (("forward", y, yd), ("d_forward", xr.grad, xd.grad), ("invert", xh, xhd), ("d_invert", zr.grad, zd.grad)):
            worst[key] = max(worst[key], PC.rel_max(_np(got), _np(want)))
        # a row alone has the gradient bits it has in the batch
        rt.input_buffer, rt.band_buffer = state[1:2].clone(), bstate[1:2].clone()
        x1, z1 = x[1:2].to(dev).requires_grad_(), z[1:2].to(dev).requires_grad_()
        ((rt(x1) * gy[1:2].to(dev)).sum() + (rt.invert(z1) * gx[1:2].to(dev)).sum()).backward()
        assert torch.equal(x1.grad, xr.grad[1:2]) and torch.equal(z1.grad, zr.grad[1:2]), c
    print("pqmf stream gradients (%d, %d): %s" % (n_band, taps, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


# ---- Resample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", RB_CASES, ids=_ids(RB_CASES))
def test_resample_forward_and_backward_match_float64(dev, orig, new):
    rs = A.Resample(orig, new).to(dev)
    tb, in_lds = RC.plan(orig, new)
    worst = dict(forward=0.0, backward=0.0)
    for L in RC.lengths(orig, new):
        x = RC.audio((3, L), 600 + L).float()
        g = RC.audio((3, RC.out_len(L, orig, new)), 610 + L).float()
        xr = x.to(dev).requires_grad_()
        y = rs(xr)
        assert y.shape == g.shape and y.dtype == torch.float32
        (y * g.to(dev)).sum().backward()
        xd = x.double().requires_grad_()
        yd = RC.model(xd, orig, new)
        (yd * g.double()).sum().backward()
        worst["forward"] = max(worst["forward"], RC.rel_max(_np(y), _np(yd)))
        worst["backward"] = max(worst["backward"], RC.rel_max(_np(xr.grad), _np(xd.grad)))
    print("resample (%d, %d) backward tile %d blocks, bank in LDS %s: %s"
          % (orig, new, tb, in_lds, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


@pytest.mark.parametrize("orig,new", RB_CASES, ids=_ids(RB_CASES))
def test_resample_bit_rules_and_guard_bands(dev, orig, new):
    h, width = RC.bank(orig, new)
    hd, taps = h.to(dev), 2 * width + orig
    tb = RC.plan(orig, new)[0]
    L = tb * orig + 1                                          # a whole tile and a one-sample tile
    olen = RC.out_len(L, orig, new)
    x, g = RC.audio((3, L), 620).float().to(dev), RC.audio((3, olen), 621).float().to(dev)
    y, gx = ops.resample_sinc(x, orig, new, width, hd), ops.resample_sinc_backward(g, L, orig, new, taps, width, hd)
    for r in range(3):
        assert torch.equal(ops.resample_sinc(x[r:r + 1].contiguous(), orig, new, width, hd), y[r:r + 1]), r
        assert torch.equal(ops.resample_sinc_backward(g[r:r + 1].contiguous(), L, orig, new, taps, width, hd), gx[r:r + 1]), r
    bad_x, bad_g = x.clone(), g.clone()
    bad_x[1, L // 2] = float("nan")
    bad_g[1, olen // 2] = float("nan")
    yn, gn = ops.resample_sinc(bad_x, orig, new, width, hd), ops.resample_sinc_backward(bad_g, L, orig, new, taps, width, hd)
    assert torch.equal(yn[[0, 2]], y[[0, 2]]) and torch.equal(gn[[0, 2]], gx[[0, 2]])
    assert bool(torch.isnan(yn[1]).any()) and bool(torch.isnan(gn[1]).any())
    assert _plus_zero(ops.resample_sinc(torch.zeros_like(x), orig, new, width, hd))
    assert _plus_zero(ops.resample_sinc_backward(torch.zeros_like(g), L, orig, new, taps, width, hd))
    lib = _lib.lib()
    out = _guarded(3 * olen, torch.float32, dev, lambda o: _lib.check(lib.at_resample_sinc(
        _lib.ptr(x), 3, L, orig, new, width, _lib.ptr(hd), olen, _lib.ptr(o), _lib.stream_ptr()), "at_resample_sinc"))
    assert torch.equal(out.view(3, olen), y)
    out = _guarded(3 * L, torch.float32, dev, lambda o: _lib.check(lib.at_resample_sinc_backward(
        _lib.ptr(g), 3, L, orig, new, taps, width, _lib.ptr(hd), olen, _lib.ptr(o), _lib.stream_ptr()), "at_resample_sinc_backward"))
    assert torch.equal(out.view(3, L), gx)


@pytest.mark.parametrize("orig,new", W.RB_STREAM_NAMED, ids=_ids(W.RB_STREAM_NAMED))
def test_resample_stream_is_the_one_call_to_the_bit(dev, orig, new):
    rt, rs = A.RealtimeResample(orig, new).to(dev), A.Resample(orig, new).to(dev)
    D, Ha = RC.stream_sizes(orig, new)
    worst = 0.0
    for i, blocks in enumerate(W.chunk_lists((orig, new), RC.plan(orig, new)[0])):
        n = sum(blocks)
        x = RC.audio((2, n * orig), 630 + i).float()
        xd = x.to(dev)
        rt.reset()
        pos, outs = 0, []
        for b in blocks:
            outs.append(rt(xd[:, pos:pos + b * orig]))
            pos += b * orig
        chunked = torch.cat(outs, -1)
        assert chunked.shape == (2, n * new)
        assert torch.equal(rt.input_buffer, torch.cat([xd.new_zeros(2, Ha), xd], -1)[:, -Ha:])
        rt.reset()
        assert torch.equal(chunked, rt(xd)), blocks
        assert torch.equal(chunked, rs(torch.cat([xd.new_zeros(2, D * orig), xd], -1))[..., :n * new]), blocks
        worst = max(worst, RC.rel_max(_np(chunked), RC.stream(x.double(), orig, new, blocks).numpy()))
    print("resample stream (%d, %d): %.2e" % (orig, new, worst))
    assert worst < TOL


@pytest.mark.parametrize("orig,new", W.RB_STREAM_NAMED, ids=_ids(W.RB_STREAM_NAMED))
def test_resample_stream_gradient_of_a_chunk_matches_float64(dev, orig, new):
    """The only place a stream reaches the backward plan: at_resample_sinc_backward with lead = Ha over the chunk's own
    blocks, whose halo and tile differ from the offline backward's.  Chunks of 1 block, on both sides of that tile and past
    two tiles, behind a first chunk that fills the state; the state is a constant of the graph."""
    rt = A.RealtimeResample(orig, new).to(dev)
    D, Ha = RC.stream_sizes(orig, new)
    tb, in_lds = RC.plan(orig, new, Ha)
    assert (tb, in_lds) == W.resample_plan(orig, new, lead=Ha)[:2] and tb < W.resample_plan(orig, new, lead=Ha)[2]
    rt(RC.audio((2, (D + 2) * orig), 640).float().to(dev))
    state = rt.input_buffer.clone()
    assert bool(state.any())
    worst = dict(forward=0.0, gradient=0.0)
    for c in (1, tb - 1, tb, tb + 1, 2 * tb + 1):
        x, g = RC.audio((2, c * orig), 641 + c).float(), RC.audio((2, c * new), 642 + c).float()
        rt.input_buffer = state.clone()
        xr = x.to(dev).requires_grad_()
        y = rt(xr)
        assert "ResampleStreamFunction" in type(y.grad_fn).__name__ and not rt.input_buffer.requires_grad
        (y * g.to(dev)).sum().backward()
        xd = x.double().requires_grad_()
        yd, sd = RC.stream_chunk(xd, state.cpu().double(), orig, new)
        (yd * g.double()).sum().backward()
        assert xr.grad.shape == x.shape and torch.equal(rt.input_buffer.cpu(), sd.float())
        worst["forward"] = max(worst["forward"], RC.rel_max(_np(y), _np(yd)))
        worst["gradient"] = max(worst["gradient"], RC.rel_max(_np(xr.grad), _np(xd.grad)))
        # the bits of the C entry at lead = Ha, a row alone, a NaN in one row of g, zeros
        h, width = RC.bank(orig, new)
        hd, taps, gd = h.to(dev), 2 * width + orig, g.to(dev)
        assert torch.equal(ops.resample_sinc_backward(gd, c * orig, orig, new, taps, Ha, hd), xr.grad), c
        assert torch.equal(ops.resample_sinc_backward(gd[1:2].contiguous(), c * orig, orig, new, taps, Ha, hd), xr.grad[1:2]), c
        bad = gd.clone()
        bad[0, c * new // 2] = float("nan")
        gn = ops.resample_sinc_backward(bad, c * orig, orig, new, taps, Ha, hd)
        assert torch.equal(gn[1], xr.grad[1]) and bool(torch.isnan(gn[0]).any())
        assert _plus_zero(ops.resample_sinc_backward(torch.zeros_like(gd), c * orig, orig, new, taps, Ha, hd))
        out = _guarded(2 * c * orig, torch.float32, dev, lambda o: _lib.check(_lib.lib().at_resample_sinc_backward(
            _lib.ptr(gd), 2, c * orig, orig, new, taps, Ha, _lib.ptr(hd), c * new, _lib.ptr(o), _lib.stream_ptr()),
            "at_resample_sinc_backward"))
        assert torch.equal(out.view(2, c * orig), xr.grad)
    print("resample stream gradient (%d, %d) tile %d blocks at lead %d: %s"
          % (orig, new, tb, Ha, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


# ---- the bankless converter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", SI_CASES, ids=_ids(SI_CASES))
def test_sinc_converter_both_directions_match_float64(dev, orig, new):
    Qi = SI.table(orig, new)[1]
    (tf, lds_f), (tb, lds_b) = SI.plan(orig, new, Qi), SI.plan(new, orig, Qi)
    rs = A.Resample(orig, new, direct=True).to(dev)
    worst = dict(forward=0.0, backward=0.0)
    for L in SI.lengths(orig, new):
        x, g, y, gx = SI.case(orig, new, L, (3,))
        xd, gd = x.float().to(dev), g.float().to(dev)
        got = ops.resample_direct(xd, orig, new)
        back = ops.resample_direct_backward(gd, L, orig, new)
        assert got.shape == (3, SI.out_len(L, orig, new)) and back.shape == (3, L)
        worst["forward"] = max(worst["forward"], SI.rel_max(_np(got), y.numpy()))
        worst["backward"] = max(worst["backward"], SI.rel_max(_np(back), gx.numpy()))
        xr = xd.clone().requires_grad_()
        routed = rs(xr)
        (routed * gd).sum().backward()
        assert torch.equal(routed.detach(), got) and torch.equal(xr.grad, back), L
    print("sinc (%d, %d) forward tile %d, table in LDS %s; backward tile %d, table in LDS %s: %s"
          % (orig, new, tf, lds_f, tb, lds_b, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL


@pytest.mark.parametrize("orig,new", SI_CASES, ids=_ids(SI_CASES))
def test_sinc_converter_bit_rules_and_guard_bands(dev, orig, new):
    table, Qi = ops._sinc_table_on(dev, orig, new)
    lengths = SI.lengths(orig, new)
    for L in (lengths[-1], lengths[len(lengths) // 2]):       # past two tiles of a direction, and a cut in between
        olen = SI.out_len(L, orig, new)
        x, g = SI.audio((3, L), 700 + L).float().to(dev), SI.audio((3, olen), 710 + L).float().to(dev)
        y, gx = ops.resample_direct(x, orig, new), ops.resample_direct_backward(g, L, orig, new)
        for r in range(3):
            assert torch.equal(ops.resample_direct(x[r:r + 1].contiguous(), orig, new), y[r:r + 1]), (L, r)
            assert torch.equal(ops.resample_direct_backward(g[r:r + 1].contiguous(), L, orig, new), gx[r:r + 1]), (L, r)
        bad_x, bad_g = x.clone(), g.clone()
        bad_x[1, L // 2] = float("nan")
        bad_g[1, olen // 2] = float("nan")
        yn, gn = ops.resample_direct(bad_x, orig, new), ops.resample_direct_backward(bad_g, L, orig, new)
        assert torch.equal(yn[[0, 2]], y[[0, 2]]) and torch.equal(gn[[0, 2]], gx[[0, 2]]), L
        assert bool(torch.isnan(yn[1]).any()) and bool(torch.isnan(gn[1]).any())
        assert _plus_zero(ops.resample_direct(torch.zeros_like(x), orig, new))
        assert _plus_zero(ops.resample_direct_backward(torch.zeros_like(g), L, orig, new))
        lib = _lib.lib()
        out = _guarded(3 * olen, torch.float32, dev, lambda o: _lib.check(lib.at_sinc_interp(
            _lib.ptr(x), 3, L, orig, new, _lib.ptr(table), Qi, olen, _lib.ptr(o), _lib.stream_ptr()), "at_sinc_interp"))
        assert torch.equal(out.view(3, olen), y)
        out = _guarded(3 * L, torch.float32, dev, lambda o: _lib.check(lib.at_sinc_interp(
            _lib.ptr(g), 3, olen, new, orig, _lib.ptr(table), Qi, L, _lib.ptr(o), _lib.stream_ptr()), "at_sinc_interp"))
        assert torch.equal(out.view(3, L), gx)


@pytest.mark.parametrize("n_steps,L", tuple(zip(W.PITCH_STEPS, (2048, 9600))), ids=("up5oct", "down5oct"))
def test_pitch_shift_by_five_octaves_runs_the_shrunk_tiles(dev, n_steps, L):
    """+60 steps convert 1411200 -> 44100 = (32, 1): the forward's tile shrinks.  -60 steps convert 1378 -> 44100 = (689,
    22050): the backward's tile shrinks and the table stays in global memory.  The module against its definition to the bit,
    forward and gradient, and its converter stage against the float64 gather on the module's own intermediate signal."""
    rate, orig_freq = SI.pitch_rates(SR, n_steps)
    orig, new = SI.reduced(orig_freq, SR)
    assert (orig, new) in ((32, 1), (689, 22050))
    Qi = SI.table(orig, new)[1]
    assert SI.plan(orig, new, Qi)[0] < W.SI_TILE or SI.plan(new, orig, Qi)[0] < W.SI_TILE
    ps = A.PitchShift(SR, n_steps).to(dev)
    n = int(round(L / rate))
    x, g = SI.audio((2, L), 720).float().to(dev), SI.audio((2, L), 721).float().to(dev)
    y = ps(x)
    pre, want = PT._stretched(x, n_steps), PT._chain(x, n_steps)
    assert pre.shape == (2, n)
    assert y.shape == x.shape and bool(torch.isfinite(y).all()) and bool(y.any()) and torch.equal(y, want)
    olen = SI.out_len(n, orig, new)
    model = SI.model(_np(pre).astype(np.float64), orig, new)
    err_f = SI.rel_max(_np(y)[..., :min(L, olen)], model[..., :min(L, olen)])
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    (ps(xa) * g).sum().backward()
    (PT._chain(xb, n_steps) * g).sum().backward()
    assert bool(xa.grad.any()) and torch.equal(xa.grad, xb.grad)
    gfull = PT._fit(g, olen)                                      # the cotangent as it reaches the converter
    back = ops.resample_direct_backward(gfull, n, orig_freq, SR)
    err_b = SI.rel_max(_np(back), SI.adjoint(_np(gfull).astype(np.float64), n, orig, new))
    print("pitch shift %+d steps, converter (%d, %d) on %d samples: forward %.2e backward %.2e" % (n_steps, orig, new, n, err_f, err_b))
    assert err_f < TOL and err_b < TOL


# ---- the hop endings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.HOP_FILTERS)
@pytest.mark.parametrize("L,hop", HOP_CASES, ids=_ids(HOP_CASES))
def test_hop_endings_match_float64_keep_their_rows_and_stay_inside_them(dev, L, hop, name):
    sos = SC.FILTERS[name]
    co = ops.sos_coefficients(sos)
    nh = L // hop
    rng = np.random.default_rng([800, L, hop])
    x = rng.standard_normal((3, L)).astype(np.float32)
    w = rng.standard_normal((3, nh)) + 2.0
    xd, wd = _dev(x, dev), _dev(w, dev)
    power, u = ops.sos_hop_power(xd, sos, hop), ops.sos_filter_hop_scaled(xd, sos, hop, wd)
    assert power.shape == (3, nh) and power.dtype == torch.float64 and u.shape == (3, L) and u.dtype == torch.float32
    y = LC.sosfilt(np.array(sos, dtype=np.float64), x.astype(np.float64), axis=-1)
    want_u = np.zeros((3, L))
    want_u[:, :nh * hop] = np.repeat(w, hop, axis=-1) * y[:, :nh * hop]
    err_p, err_u = LC.rel_max(_np(power), LC.hop_power(sos, x, hop)), LC.rel_max(_np(u), want_u)
    print("hop endings %s L %d hop %d: power %.2e scaled %.2e" % (name, L, hop, err_p, err_u))
    assert err_p < LC.TOL and err_u < SC.TOL
    assert _plus_zero(u[:, nh * hop:])                         # +0 past the last whole hop
    for r in range(3):
        assert torch.equal(ops.sos_hop_power(xd[r].clone(), sos, hop), power[r]), r
        assert torch.equal(ops.sos_filter_hop_scaled(xd[r].clone(), sos, hop, wd[r].clone()), u[r]), r
    at = min(L - 1, L // 2 + 1000)
    bad = xd.clone()
    bad[1, at] = float("nan")
    pn, un = ops.sos_hop_power(bad, sos, hop), ops.sos_filter_hop_scaled(bad, sos, hop, wd)
    assert torch.equal(pn[[0, 2]], power[[0, 2]]) and torch.equal(un[[0, 2]], u[[0, 2]])
    assert torch.equal(pn[1, :at // hop], power[1, :at // hop]) and bool(torch.isnan(pn[1, at // hop:]).all())
    assert torch.equal(un[1, :at], u[1, :at]) and bool(torch.isnan(un[1, at:nh * hop]).all())
    zeros = torch.zeros_like(xd)
    assert _plus_zero(ops.sos_hop_power(zeros, sos, hop)) and _plus_zero(ops.sos_filter_hop_scaled(zeros, sos, hop, wd))
    lib = _lib.lib()
    if nh:
        out = _guarded(3 * nh, torch.float64, dev, lambda o: _lib.check(lib.at_sos_hop_power(
            _lib.ptr(xd), 3, L, co.ptr, co.n, hop, _lib.ptr(o), _lib.stream_ptr()), "at_sos_hop_power"))
        assert torch.equal(out.view(3, nh), power)
    out = _guarded(3 * L, torch.float32, dev, lambda o: _lib.check(lib.at_sos_filter_hop_scaled(
        _lib.ptr(xd), 3, L, co.ptr, co.n, hop, _lib.ptr(wd), _lib.ptr(o), _lib.stream_ptr()), "at_sos_filter_hop_scaled"))
    assert torch.equal(out.view(3, L), u)


@pytest.mark.parametrize("name", W.HOP_FILTERS)
def test_sos_stream_cut_by_seeded_chunks_is_the_one_call(dev, name):
    sos = SC.FILTERS[name]
    n = sos.shape[0]
    worst = dict(oracle=0.0, one_call=0.0, state=0.0)
    for i, cuts in enumerate(W.chunk_lists((n,), SC.plan(n)[0])):
        L = sum(cuts)
        x = np.random.default_rng([810, n, i]).standard_normal((2, L)).astype(np.float32)
        want, want_zf = SC.sosfilt(sos, x.astype(np.float64))
        xd = _dev(x, dev)
        one_call = _np(ops.sos_filter(xd, sos))
        rt = A.SOSFilter(sos).to(dev).streaming()
        at, outs = 0, []
        for c in cuts:
            outs.append(rt(xd[..., at:at + c]))
            at += c
        got = _np(torch.cat(outs, -1))
        worst["oracle"] = max(worst["oracle"], SC.rel_max(got, want))
        worst["one_call"] = max(worst["one_call"], SC.rel_max(got, one_call))
        worst["state"] = max(worst["state"], SC.rel_max(_np(rt.state), want_zf))
    print("sos stream %s: %s" % (name, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["oracle"] < SC.TOL and worst["one_call"] < 1e-6 and worst["state"] < SC.STATE_TOL, worst


# ---- the spectral FIR and FFTConvolve ------------------------------------------------------------------------------------------------
def _planted(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _crel(got, want):
    """max |a - b| / max |b| over complex arrays."""
    got, want = _np(got).astype(np.complex128), np.asarray(want)
    return float(np.abs(got - want).max() / np.abs(want).max())


def _cbits(a, b):
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b))


@pytest.mark.parametrize("P,T", FIR_CASES, ids=_ids(FIR_CASES))
def test_spectral_fir_kernels_match_the_float64_loop(dev, P, T):
    """at_spectral_fir causal and anticausal-conjugate, and at_spectral_fir_corr, with shared and per-row filters, 3 rows of
    F = 129 bins (block 128); a row alone has the bits it has in the batch."""
    rng = np.random.default_rng([900, P, T])
    F = W.FIR_BLOCK + 1
    X, G, H, Hr = _planted(rng, 3, T, F), _planted(rng, 3, T, F), _planted(rng, P, F), _planted(rng, 3, P, F)
    Xd, Gd = _dev(X, dev), _dev(G, dev)
    worst = {}
    for key, Hh in (("shared", H), ("per_row", Hr)):
        Hd = _dev(Hh, dev)
        Y, Ya = ops.spectral_fir(Xd, Hd), ops.spectral_fir(Gd, Hd, anticausal=True, conj=True)
        gH = ops.spectral_fir_corr(Xd, Gd, P, key == "shared")
        worst[key + " fir"] = _crel(Y, FC.spectral_fir_reference(X, Hh))
        worst[key + " adjoint"] = _crel(Ya, FC.spectral_fir_reference(G, Hh, anticausal=True, conj=True))
        worst[key + " corr"] = _crel(gH, FC.spectral_fir_corr_reference(X, G, P, key == "shared"))
        for r in range(3):
            Hone = Hd if key == "shared" else Hd[r:r + 1].contiguous()
            assert _cbits(ops.spectral_fir(Xd[r:r + 1].contiguous(), Hone), Y[r:r + 1]), (key, r)
            assert _cbits(ops.spectral_fir(Gd[r:r + 1].contiguous(), Hone, anticausal=True, conj=True), Ya[r:r + 1]), (key, r)
            if key == "per_row":
                assert _cbits(ops.spectral_fir_corr(Xd[r:r + 1].contiguous(), Gd[r:r + 1].contiguous(), P, False), gH[r:r + 1]), r
    print("spectral fir P %d T %d: %s" % (P, T, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < FC.TOL


@pytest.mark.parametrize("P", W.FIR_NAMED_P)
def test_fft_convolve_forward_and_both_gradients_at_the_named_partition_counts(dev, P):
    B, K = W.FIR_BLOCK, P * W.FIR_BLOCK
    worst = dict(forward=0.0, gx=0.0, gh=0.0)
    for L, T in W.fir_lengths(P):
        assert ops.fft_convolve_plan(L, K, B)[:3] == (B, T, P)
        d = FC.data(L, K, 3)
        for per_row in (False, True):
            hh = d["hr"] if per_row else d["h"]
            want, gx, gh = FC.conv1d_autograd(d["x"], hh, d["g_full"])
            x, h = _dev(d["x"], dev).requires_grad_(), _dev(hh, dev).requires_grad_()
            y = FFTConvolveFunction.apply(x, h, "full", B)
            y.backward(_dev(d["g_full"], dev))
            worst["forward"] = max(worst["forward"], FC.rel_max(_np(y), FC.oracle(d["x"], hh)), FC.rel_max(_np(y), want))
            worst["gx"] = max(worst["gx"], FC.rel_max(_np(x.grad), gx))
            worst["gh"] = max(worst["gh"], FC.rel_max(_np(h.grad), gh))
            # the bit rules: the plain route, a row alone, a NaN in one row, zeros
            xp, hp, y = x.detach(), h.detach(), y.detach()
            assert torch.equal(ops.fft_convolve(xp, hp, "full", block=B), y)
            for r in range(3):
                assert torch.equal(ops.fft_convolve(xp[r:r + 1], hp[r:r + 1] if per_row else hp, "full", block=B), y[r:r + 1]), r
            bad = xp.clone()
            bad[1, L // 2] = float("nan")
            yn = ops.fft_convolve(bad, hp, "full", block=B)
            assert torch.equal(yn[[0, 2]], y[[0, 2]]) and bool(torch.isnan(yn[1]).any())
            assert _plus_zero(ops.fft_convolve(torch.zeros_like(xp), hp, "full", block=B))
    print("fft convolve block %d P %d: %s" % (B, P, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < FC.TOL


@pytest.mark.parametrize("P", W.FIR_NAMED_P)
def test_convolution_stream_cut_by_seeded_chunks_is_the_offline_call_to_the_bit(dev, P):
    B, K = W.FIR_BLOCK, P * W.FIR_BLOCK
    worst = 0.0
    for i, blocks in enumerate(W.chunk_lists((P,), W.FIR_TILE)):
        n = sum(blocks)
        d = FC.data(n * B, K, 3, seed=i)
        xd = _dev(d["x"], dev)
        m = A.RealtimeImpulseResponse(torch.from_numpy(d["h"]), block=B).to(dev)
        assert (m.block, m.partitions) == (B, P)
        at, outs = 0, []
        for b in blocks:
            outs.append(m(xd[..., at:at + b * B]))
            at += b * B
        y = torch.cat(outs, -1)
        assert torch.equal(y, A.fftconvolve(xd, m.ir, "full", block=B)[..., :n * B]), blocks
        m.reset()
        assert torch.equal(y, m(xd)), blocks
        worst = max(worst, FC.rel_max(_np(y), FC.oracle(d["x"], d["h"])[:, :n * B]))
    print("convolution stream block %d P %d: %.2e" % (B, P, worst))
    assert worst < FC.TOL

"""GPU side of TimeStretch (transforms.TimeStretch, ops.phase_vocoder / phase_vocoder_backward,
autograd.PhaseVocoderFunction, csrc/phase_vocoder.hip): parity of the forward and of the gradient with the float64
textbook algorithm of phase_vocoder_cases.py -- angles, wrap, expected advance, cumsum, and torch autograd of it -- run on
the same complex64 input, within the library's normwise bound 1e-5 (the fp32 phasor product restated on the CPU is 3.4e-7
... 3.1e-6 off the textbook between 9 and 690 frames, the bound is not taken from the kernel); then the bit-level properties
that follow from one chain per (clip, bin) column, routing, and the chain STFT -> TimeStretch -> STFT.invert."""
import pytest
import torch

import acids_transforms_amd as A
import phase_vocoder_cases as C
from acids_transforms_amd import _lib, ops

pytestmark = pytest.mark.gpu
BMAX = max(C.BATCHES)


def _case(T, F, rate, seed, B=BMAX):
    """(X, g) complex64 on the CPU and the float64 reference (Z, gX) of the whole batch: clips do not mix, so a smaller
    batch is a slice of all four."""
    X = C.spectrum((B, T, F), seed)
    g = C.spectrum((B, len(C.steps(T, rate)[0]), F), seed + 1)
    Z, gX = C.textbook_with_grad(X, g, rate)
    return X, g, Z, gX


def _check(dev, X, g, Z, gX, rate, B, worst):
    """op, module, module under autograd and both gradients for the first B clips; the worst errors into `worst`"""
    Xd, gd = X[:B].to(dev), g[:B].to(dev)
    N, F = Z.shape[-2], Z.shape[-1]
    out, fin = ops.phase_vocoder(Xd, rate, want_phasor=True)
    assert out.shape == (B, N, F) and out.dtype == torch.complex64 and fin.shape == (B, F)
    worst["op"] = max(worst["op"], C.normwise(out.cpu(), Z[:B]))
    mod = A.TimeStretch(rate).to(dev)
    worst["module"] = max(worst["module"], C.normwise(mod(Xd).cpu(), Z[:B]))
    worst["op grad"] = max(worst["op grad"], C.normwise(ops.phase_vocoder_backward(Xd, gd, rate, fin).cpu(), gX[:B]))
    Xr = Xd.clone().requires_grad_()
    y = mod(Xr)
    assert y.grad_fn is not None and y.shape == (B, N, F)
    worst["autograd forward"] = max(worst["autograd forward"], C.normwise(y.detach().cpu(), Z[:B]))
    y.backward(gd)
    assert Xr.grad.shape == Xr.shape and Xr.grad.dtype == torch.complex64
    worst["module grad"] = max(worst["module grad"], C.normwise(Xr.grad.cpu(), gX[:B]))


@pytest.mark.parametrize("F", C.BINS)
def test_parity_with_the_float64_textbook(dev, F):
    worst = dict.fromkeys(("op", "module", "autograd forward", "op grad", "module grad"), 0.0)
    for T in C.FRAMES:
        for rate in C.RATES:
            X, g, Z, gX = _case(T, F, rate, 1000 * F + 10 * T)
            for B in C.BATCHES:
                _check(dev, X, g, Z, gX, rate, B, worst)
    print("F = %d: " % F + ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert all(v < C.TOL for v in worst.values()), worst


def test_parity_over_690_frames_at_half_speed(dev):
    worst = dict.fromkeys(("op", "module", "autograd forward", "op grad", "module grad"), 0.0)
    X, g, Z, gX = _case(690, 513, 0.5, 77, B=2)
    assert Z.shape == (2, 1380, 513)
    _check(dev, X, g, Z, gX, 0.5, 2, worst)
    print("(2, 690, 513) at rate 0.5: " + ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert all(v < C.TOL for v in worst.values()), worst


@pytest.mark.parametrize("rate", (0.8, 1.3, 3.0))
def test_a_clip_alone_has_its_batch_s_bits_in_either_layout(dev, rate):
    X = C.spectrum((BMAX, 33, 513), 5).to(dev)
    N = len(C.steps(33, rate)[0])
    g = C.spectrum((BMAX, N, 513), 6).to(dev)
    out, fin = ops.phase_vocoder(X, rate, want_phasor=True)            # 65 clips: one block per clip
    gX = ops.phase_vocoder_backward(X, g, rate, fin)
    for B in (1, 2, 63, 64):                                           # below and on the threshold of that layout
        o, f = ops.phase_vocoder(X[:B], rate, want_phasor=True)
        assert torch.equal(torch.view_as_real(o), torch.view_as_real(out[:B])), B
        assert torch.equal(torch.view_as_real(f), torch.view_as_real(fin[:B])), B
        assert torch.equal(torch.view_as_real(ops.phase_vocoder_backward(X[:B], g[:B], rate, f)), torch.view_as_real(gX[:B])), B
    o1 = ops.phase_vocoder(X[40:41], rate)                             # a clip from the middle, alone
    assert torch.equal(torch.view_as_real(o1), torch.view_as_real(out[40:41]))
    with _lib.variant("scan_layout", 1):                               # the whole batch on flat columns
        o, f = ops.phase_vocoder(X, rate, want_phasor=True)
        gf = ops.phase_vocoder_backward(X, g, rate, fin)
    assert torch.equal(torch.view_as_real(o), torch.view_as_real(out)) and torch.equal(torch.view_as_real(f), torch.view_as_real(fin))
    assert torch.equal(torch.view_as_real(gf), torch.view_as_real(gX))
    # four columns per thread (rows past 2048 bins)
    Xw = C.spectrum((64, 5, 2049), 7).to(dev)
    ow, fw = ops.phase_vocoder(Xw, rate, want_phasor=True)
    assert torch.equal(torch.view_as_real(ops.phase_vocoder(Xw[:3], rate)), torch.view_as_real(ow[:3]))
    gw = C.spectrum(tuple(ow.shape), 8).to(dev)
    assert torch.equal(torch.view_as_real(ops.phase_vocoder_backward(Xw[:3], gw[:3], rate, fw[:3])),
                       torch.view_as_real(ops.phase_vocoder_backward(Xw, gw, rate, fw)[:3]))


def test_routing(dev):
    X = C.spectrum((2, 3, 9, 257), 11).to(dev)                         # two batch dimensions
    ts = A.TimeStretch(0.8).to(dev)
    plain = ts(X)
    assert plain.grad_fn is None and plain.shape == (2, 3, 12, 257) and plain.dtype == torch.complex64
    Xr = X.clone().requires_grad_()
    routed = ts(Xr)
    assert routed.grad_fn is not None and "PhaseVocoderFunction" in type(routed.grad_fn).__name__
    assert torch.equal(torch.view_as_real(routed.detach()), torch.view_as_real(plain))     # the grad route's forward bits
    with torch.no_grad():
        assert ts(Xr).grad_fn is None
    assert A.TimeStretch(1.0)(X) is X and ts(X, overriding_rate=1.0) is X and A.TimeStretch(1.0)(Xr) is Xr
    assert torch.equal(torch.view_as_real(ts(X, overriding_rate=1.3)), torch.view_as_real(ops.phase_vocoder(X, 1.3)))
    # hop_length has no effect
    a = A.TimeStretch(0.8, hop_length=128, n_freq=257)(X)
    b = A.TimeStretch(0.8, hop_length=256)(X)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)) and torch.equal(torch.view_as_real(a), torch.view_as_real(plain))
    # the graph keeps the spectrum and the (..., F) phasor
    saved = [t for t in routed.grad_fn.saved_tensors]
    assert sorted(tuple(t.shape) for t in saved) == [(2, 3, 9, 257), (2, 3, 257)]
    # time is kept
    time = torch.zeros(2, 3, device=dev)
    y, tm = ts.forward_with_time(X, time)
    assert tm is time and torch.equal(torch.view_as_real(y), torch.view_as_real(plain))
    # first order only
    with pytest.raises(RuntimeError):
        xx = X.clone().requires_grad_()
        (gx,) = torch.autograd.grad(ts(xx).abs().square().sum(), xx, create_graph=True)
        gx.abs().sum().backward()
    # errors
    with pytest.raises(ValueError):
        ts(X.real)
    with pytest.raises(A.AcidsHipError):
        ts(X.to(torch.complex128))
    with A.allow_fp64_narrowing():
        assert torch.equal(torch.view_as_real(ts(X.to(torch.complex128))), torch.view_as_real(plain))
    with pytest.raises(ValueError):
        A.TimeStretch(0.8, n_freq=513)(X)
    # empty work
    assert ts(X[:0]).shape == (0, 3, 12, 257) and ts(X[..., :0]).shape == (2, 3, 12, 0) and ts(X[..., :0, :]).shape == (2, 3, 0, 257)


@pytest.mark.parametrize("rate", (0.5, 1.3, 3.0))
def test_a_nan_stays_in_its_column(dev, rate):
    B, T, F = 3, 33, 513
    X = C.spectrum((B, T, F), 21).to(dev)
    N = len(C.steps(T, rate)[0])
    g = C.spectrum((B, N, F), 22).to(dev)
    out, fin = ops.phase_vocoder(X, rate, want_phasor=True)
    gX = ops.phase_vocoder_backward(X, g, rate, fin)
    Xn = X.clone()
    Xn[1, 9, 100] = complex(float("nan"), 0.0)                          # frame 9 is read at all three rates
    outn, finn = ops.phase_vocoder(Xn, rate, want_phasor=True)
    gXn = ops.phase_vocoder_backward(Xn, g, rate, finn)
    gn = g.clone()
    gn[2, N // 2, 7] = complex(0.0, float("nan"))
    gXg = ops.phase_vocoder_backward(X, gn, rate, fin)
    for got, ref, (b, f) in ((outn, out, (1, 100)), (gXn, gX, (1, 100)), (gXg, gX, (2, 7))):
        got, ref = torch.view_as_real(got).clone(), torch.view_as_real(ref).clone()
        assert bool(torch.isnan(got[b, :, f]).any())
        got[b, :, f] = 0
        ref[b, :, f] = 0
        assert torch.equal(got, ref)


def test_zero_bins(dev):
    B, T, F, rate = 3, 9, 257, 0.8
    X = C.spectrum((B, T, F), 31)
    X[0, 0] = 0                                                         # an all-zero first frame
    X[1, 4, ::3] = 0
    X[2, :, 5] = 0                                                      # a silent bin
    X[2, 8, 1::2] = 0
    X[1, 2, 1] = complex(-0.0, 0.0)                                     # counts as zero (torch.angle: pi)
    N = len(C.steps(T, rate)[0])
    g = C.spectrum((B, N, F), 32)
    Z, gX = C.textbook_with_grad(X, g, rate)
    Xd = X.to(dev)
    out, fin = ops.phase_vocoder(Xd, rate, want_phasor=True)
    got = ops.phase_vocoder_backward(Xd, g.to(dev), rate, fin)
    assert bool(torch.isfinite(torch.view_as_real(out)).all()) and bool(torch.isfinite(torch.view_as_real(got)).all())
    assert not out[2, :, 5].any() and not got[Xd == 0].any()            # exactly zero where the spectrum is
    keep = torch.ones(B, 1, F, dtype=torch.bool)
    keep[1, 0, 1] = False                                               # the -0 bin's column: the documented divergence
    e_fwd = C.normwise(out.cpu() * keep, Z * keep)
    e_bwd = C.normwise(got.cpu() * keep, gX * keep)
    print("planted zeros: forward %.2e, gradient %.2e" % (e_fwd, e_bwd))
    assert e_fwd < C.TOL and e_bwd < C.TOL
    # the -0 + 0i bin (frame 2): zero phase here, pi in the textbook.  The step that enters the frame adds it and the step
    # that leaves it takes it away again, so only the rows in between -- idx == 2: row 3 -- have the opposite sign
    rows = [j for j, i in enumerate(C.steps(T, rate)[0]) if i == 2]
    sign = torch.ones(N, dtype=torch.complex128)
    sign[rows] = -1
    assert rows == [3] and C.normwise(out[1, :, 1].cpu() * sign, Z[1, :, 1]) < C.TOL


def test_strided_input_and_offset_gradient(dev):
    rate = 1.3
    big = C.spectrum((2, 9, 2 * 513), 41).to(dev)
    X = big[..., ::2]                                                   # not contiguous
    assert not X.is_contiguous()
    Xc = X.contiguous()
    N = len(C.steps(9, rate)[0])
    out, fin = ops.phase_vocoder(Xc, rate, want_phasor=True)
    assert torch.equal(torch.view_as_real(ops.phase_vocoder(X, rate)), torch.view_as_real(out))
    g = C.spectrum((2, N, 513), 42).to(dev)
    buf = torch.zeros(g.numel() + 1, dtype=torch.complex64, device=dev)
    assert buf.data_ptr() % 16 == 0
    g1 = buf[1:].view(g.shape)                                          # starts one element past the aligned buffer
    g1.copy_(g)
    assert g1.data_ptr() % 16 == 8 and g1.is_contiguous()
    want = ops.phase_vocoder_backward(Xc, g, rate, fin)
    assert torch.equal(torch.view_as_real(ops.phase_vocoder_backward(Xc, g1, rate, fin)), torch.view_as_real(want))
    gt = g.transpose(-1, -2).contiguous().transpose(-1, -2)             # a gradient that is not contiguous
    assert torch.equal(torch.view_as_real(ops.phase_vocoder_backward(X, gt, rate, fin)), torch.view_as_real(want))
    # through the module: the gradient arrives at the strided leaf's base
    leaf = big.clone().requires_grad_()
    A.TimeStretch(rate)(leaf[..., ::2]).backward(g)
    assert torch.equal(torch.view_as_real(leaf.grad[..., ::2]), torch.view_as_real(want)) and not leaf.grad[..., 1::2].any()


def test_chain_stft_stretch_invert(dev):
    sr, n_fft, hop, freq = 44100, 1024, 256, 1000.0
    L = 32 * hop                                                        # 33 frames
    x = (0.5 * torch.sin(2 * torch.pi * freq * torch.arange(L) / sr)).unsqueeze(0).to(dev).requires_grad_()
    stft = A.STFT(n_fft=n_fft, hop_length=hop).to(dev)
    ts = A.TimeStretch(0.8, hop_length=hop, n_freq=n_fft // 2 + 1).to(dev)
    X = stft(x)
    assert X.shape[-2:] == (33, 513)
    Y = ts(X)
    N = len(C.steps(33, 0.8)[0])
    assert Y.shape[-2:] == (N, 513) and N == 42
    y = stft.invert(Y)
    assert y.shape[-1] == (N - 1) * hop                                 # the length follows N
    peak_in = int(X.detach().abs().mean(-2).argmax())
    peak_out = int(stft(y.detach()).abs().mean(-2).argmax())
    assert peak_in == round(freq * n_fft / sr) == peak_out
    y.square().sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and bool((x.grad != 0).any())
    assert ts.ratio == 1.25 and (stft + ts).ratio == hop * 1.25

"""Gradients through STFT / DGT invert (the ISTFT adjoint, at_istft_backward) against torch autograd of the reference's
own expressions: torch.istft of the complex spectrum, and of mag * exp(i phase) for the keep_input and random modes, in
float64 on the CPU from the same fp32 inputs.  Tolerance: normwise rel_max <= 1e-5, as for the forward.  The sweep and
the dispatch classes it reaches are in istft_grad_cases.py (checked by test_istft_grad_cpu.py)."""
import math

import pytest
import torch

import acids_transforms_amd as A
import istft_grad_cases as C
from acids_transforms_amd import ops
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5


def cpu(t):
    return t.detach().cpu().numpy()


def module(cls, n, h, dev):
    return (A.STFT if cls == "stft" else A.DGT)(n_fft=n, hop_length=h).to(dev)


def ref_grad(w, n, h, gy, X=None, mag=None, phase=None):
    """X.grad (complex) or mag.grad of torch.istft fed gy, in float64 on the CPU."""
    w64 = w.detach().cpu().double()
    if X is not None:
        leaf = X.detach().cpu().to(torch.complex128).requires_grad_()
        Xc = leaf
    else:
        leaf = mag.detach().cpu().double().requires_grad_()
        Xc = leaf * torch.exp(1j * phase.detach().cpu().double().reshape(leaf.shape))
    F = n // 2 + 1
    Xf = Xc.reshape(-1, Xc.shape[-2], F)
    y = torch.istft(Xf.transpose(-2, -1), n, h, window=w64, center=True, onesided=True)
    y.backward(gy.detach().cpu().double().reshape(y.shape))
    return leaf.grad


def audio_for(n, h, T, g):
    """Audio whose forward has T frames, or None when no clip longer than n/2 has that many."""
    L = h * (T - 1) + (n & 1) + h - 1
    if L <= n // 2:
        return None
    return torch.randn(L, generator=g)


def run_case(m, n, h, shape, mode, g, dev):
    """invert() of a random input of `shape` (..., T, F) in `mode` ('complex', 'keep_input', 'random') fed a random
    gradient; returns (input.grad, reference grad, Ly)."""
    T, F = shape[-2], n // 2 + 1
    w = m.inv_window[:n]
    if mode == "complex":
        X = torch.randn(shape, dtype=torch.complex64, generator=g).to(dev).requires_grad_()
        y = m.invert(X)
        phase = None
    else:
        mag = torch.rand(shape, generator=g).to(dev).requires_grad_()
        if mode == "keep_input":
            x = audio_for(n, h, T, g)
            if x is not None:
                m(x.expand(shape[:-2] + x.shape).contiguous().to(dev))
            else:
                m._replace_phase_buffer(None, (6.283 * torch.rand(shape, generator=g)).to(dev))
            phase = m.phase_buffer.detach().clone()
            y = m.invert(mag, inversion_mode="keep_input")
        else:
            torch.manual_seed(T * 31 + n)
            y = m.invert(mag, inversion_mode="random")
            torch.manual_seed(T * 31 + n)
            phase = torch.pi * 2 * torch.rand_like(mag)
        X = mag
    Ly = h * (T - 1) + (n & 1)
    assert y.shape == shape[:-2] + (Ly,)
    assert y.grad_fn is not None
    gy = torch.randn(y.shape, generator=g).to(dev)
    y.backward(gy)
    assert X.grad.shape == X.shape and X.grad.dtype == X.dtype
    if Ly == 0:
        return X.grad, None, Ly
    ref = ref_grad(w, n, h, gy, X=X if mode == "complex" else None, mag=X if mode != "complex" else None, phase=phase)
    return X.grad, ref, Ly


@pytest.mark.parametrize("cls", ["stft", "dgt"])
@pytest.mark.parametrize("n,h", C.PAIRS)
def test_invert_grad_matches_torch_autograd(dev, cls, n, h):
    m = module(cls, n, h, dev)
    g = torch.Generator().manual_seed(n * 7 + h)
    F = n // 2 + 1
    shapes = [(1, T, F) for T in C.frame_counts(n, h)] + [(3, 2, C.BATCH_T, F)]
    for shape in shapes:
        for mode in ("complex", "keep_input", "random"):
            got, ref, Ly = run_case(m, n, h, shape, mode, g, dev)
            if Ly == 0:
                assert float(got.abs().max()) == 0.0
                continue
            assert rel_max(cpu(got).reshape(ref.shape), ref.numpy()) < TOL, (cls, n, h, shape, mode)


@pytest.mark.parametrize("cls,n,h", [("stft", 1024, 256), ("stft", 441, 110), ("dgt", 1024, 256), ("dgt", 512, 128)])
def test_plain_invert_is_unchanged(dev, cls, n, h):
    m = module(cls, n, h, dev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 20 * h, generator=g).to(dev)
    X = m(x)
    mag = X.abs()
    Xg = X.detach().clone().requires_grad_()
    y0, y1 = m.invert(X), m.invert(Xg)
    assert y0.grad_fn is None and y1.grad_fn is not None and torch.equal(y0, y1.detach())
    modes = ["keep_input", "random", "griffin_lim", "sinebank"] + (["pghi"] if cls == "dgt" else [])
    for mode in modes:
        outs = []
        for req in (False, True):
            torch.manual_seed(11)
            outs.append(m.invert(mag.clone().requires_grad_(req), inversion_mode=mode))
        assert torch.equal(outs[0], outs[1].detach()), mode
        differentiable = mode in ("keep_input", "random")
        assert (outs[1].grad_fn is not None) == differentiable, mode
    with torch.no_grad():
        assert m.invert(Xg).grad_fn is None
        assert m.invert(mag.clone().requires_grad_(), inversion_mode="keep_input").grad_fn is None
    with pytest.raises(RuntimeError):
        (gX,) = torch.autograd.grad(m.invert(Xg).square().sum(), Xg, create_graph=True)
        gX.abs().sum().backward()


def _misaligned(t):
    """A contiguous copy of t whose data pointer is 4 bytes past an 8-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape).copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 8 == 4
    return out


@pytest.mark.parametrize("h", C.MISALIGNED_HOPS)
def test_misaligned_gradient_and_window_give_the_aligned_bits(dev, h):
    """gy and the window at odd float offsets (autograd can hand over such a gradient): the same bits as the aligned
    call, complex and polar."""
    m = A.STFT(n_fft=1024, hop_length=h).to(dev)
    g = torch.Generator().manual_seed(h + 1)
    T = 33
    w = m.inv_window[:1024]
    gy = torch.randn(3, h * (T - 1), generator=g).to(dev)
    phase = (6.283 * torch.rand(3, T, 513, generator=g)).to(dev)
    for ph in (None, phase):
        ref = ops.istft_backward(gy, w, 1024, h, T, phase=ph)
        got = ops.istft_backward(_misaligned(gy), _misaligned(w), 1024, h, T, phase=None if ph is None else _misaligned(ph))
        assert torch.equal(got, ref), (h, ph is None)


@pytest.mark.parametrize("batched", [False, True])
def test_invert_output_inside_cat_after_an_odd_segment(dev, batched):
    """autograd hands invert's backward a slice of the cat's gradient at an odd offset (4-byte aligned)."""
    m = A.STFT().to(dev)
    g = torch.Generator().manual_seed(8)
    T = 30
    shape = (1, T, 513) if batched else (T, 513)
    X = torch.randn(shape, dtype=torch.complex64, generator=g).to(dev)
    mag = torch.rand(shape, generator=g).to(dev)
    gy = torch.randn(1 + 256 * (T - 1), generator=g).to(dev)
    if batched:
        gy = gy.reshape(1, -1)
    ctx = torch.zeros(gy.shape[:-1] + (1,), device=dev)
    for mode in ("complex", "random"):
        grads = []
        for wrap in (True, False):
            src = (X if mode == "complex" else mag).clone().requires_grad_()
            torch.manual_seed(3)
            y = m.invert(src) if mode == "complex" else m.invert(src, inversion_mode="random")
            if wrap:
                torch.cat([ctx, y], -1).backward(gy)
            else:
                y.backward(gy[..., 1:].contiguous())
            grads.append(src.grad)
        assert torch.equal(grads[0], grads[1]), (mode, batched)


def _clip_alone_equals_batch(m, n, h, T, B, clips, dev, seed):
    g = torch.Generator().manual_seed(seed)
    w = m.inv_window[:n]
    env = m._env16 if m._env16.numel() else None
    gy = torch.randn(B, h * (T - 1) + (n & 1), generator=g).to(dev)
    phase = (6.283 * torch.rand(B, T, n // 2 + 1, generator=g)).to(dev)
    for ph in (None, phase):
        full = ops.istft_backward(gy, w, n, h, T, env16=env, phase=ph)
        for b in clips:
            alone = ops.istft_backward(gy[b:b + 1].contiguous(), w, n, h, T, env16=env,
                                       phase=None if ph is None else ph[b:b + 1].contiguous())
            assert torch.equal(full[b:b + 1], alone), (n, h, T, B, b, ph is None)
        del full


@pytest.mark.parametrize("n,h,T", C.BATCH7)
def test_clip_bits_do_not_depend_on_the_batch(dev, n, h, T):
    _clip_alone_equals_batch(module("stft", n, h, dev), n, h, T, 7, range(7), dev, n + h + T)


def test_clip_bits_do_not_depend_on_the_chunking(dev):
    n, h, T, B = C.CHUNKED
    assert C.path_class(n, h, B, T)["chunks"] >= 2
    m = module("stft", n, h, dev)
    c = C.chunk_clips(B, T, n, h)
    _clip_alone_equals_batch(m, n, h, T, B, [0, c - 1, c, B - 1], dev, 99)
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def bench_inv(dev):
    B, T, n, h = C.BENCH
    m = A.STFT(n_fft=n, hop_length=h).to(dev)
    g = torch.Generator(device=dev).manual_seed(4)
    X = torch.randn(B, T, n // 2 + 1, dtype=torch.complex64, device=dev, generator=g)
    gy = torch.randn(B, h * (T - 1), device=dev, generator=g)
    yield m, X, gy
    torch.cuda.empty_cache()


def test_bench_size_adjoint_identity(bench_inv):
    m, X, gy = bench_inv
    Xg = X.clone().requires_grad_()
    y = m.invert(Xg)
    y.backward(gy)
    lhs = float((y.detach().double() * gy.double()).sum())
    gX = Xg.grad
    rhs = float((gX.real.double() * X.real.double() + gX.imag.double() * X.imag.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_bench_size_round_trip_gradient(bench_inv):
    """x.grad of invert(forward(x)) fed g is g: the two adjoints together (the forward keeps every sample here)."""
    m, _, gy = bench_inv
    B, T, n, h = C.BENCH
    g = torch.Generator(device=gy.device).manual_seed(6)
    x = torch.randn(B, h * (T - 1), device=gy.device, generator=g).requires_grad_()
    y = m.invert(m(x))
    assert y.shape == x.shape
    y.backward(gy)
    assert rel_max(cpu(x.grad), cpu(gy)) < TOL


def test_training_fits_a_waveform_through_invert(dev):
    n, h, T = 1024, 256, 40
    m = A.STFT(n_fft=n, hop_length=h).to(dev)
    t = torch.arange(h * (T - 1), device=dev) / 44100.0
    target = 0.5 * torch.sin(2 * math.pi * 440 * t) + 0.3 * torch.sin(2 * math.pi * 1250 * t)
    X = torch.zeros(1, T, n // 2 + 1, dtype=torch.complex64, device=dev, requires_grad=True)
    opt = torch.optim.Adam([X], lr=2.0)
    losses = []
    for _ in range(100):
        loss = (m.invert(X)[0] - target).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] * 100 <= losses[0], (losses[0], losses[-1])

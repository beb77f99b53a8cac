"""Every path of the STFT / DGT adjoint and of the Magnitude backward (grad_cases.py names them; test_grad_cases_cpu.py
checks that these sweeps reach each one) against torch autograd of the reference's own expressions in float64, as in
test_autograd_gpu.py.  Tolerance: normwise rel_max <= 1e-5, the forward's at every size.

The big cases (several chunks of the adjoint, a chunk of one clip, more clips than grid rows, a few hundred thousand
Magnitude rows) compare a handful of clips or rows against float64, require the bits of each to be those it gets
alone, and check the float64 adjoint identity <STFT(x), G> = <x, dx> over the whole batch."""
import zlib

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import grad_cases as C
from conftest import rel_max
from test_autograd_gpu import _ref_chain, _ref_magnitude, cpu, ref_stft_grad

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---- STFT / DGT adjoint ---------------------------------------------------------------------------------------------

def _check_adjoint(m, n, h, x, g):
    xr = x.to(m.window.device).requires_grad_()
    X = m(xr)
    G = torch.randn(X.shape, dtype=torch.complex64, generator=g)
    X.backward(G.to(X.device))
    ref = ref_stft_grad(xr, m.window[:n], n, h, G)
    assert xr.grad.shape == x.shape and xr.grad.dtype == torch.float32
    return rel_max(cpu(xr.grad).reshape(ref.shape), ref.numpy())


def _check_batch_bits(m, x, g):
    """Each clip's gradient bits from a batched call are the bits it gets alone (the frames of neighbouring clips
    share no transform)."""
    xr = x.to(m.window.device).requires_grad_()
    X = m(xr)
    G = torch.randn(X.shape, dtype=torch.complex64, generator=g).to(X.device)
    X.backward(G)
    for k in range(x.shape[0]):
        xk = x[k:k + 1].to(xr.device).requires_grad_()
        m(xk).backward(G[k:k + 1])
        assert torch.equal(xk.grad[0], xr.grad[k]), k


@pytest.mark.parametrize("cls", ["stft", "dgt"])
@pytest.mark.parametrize("n,h", C.ADJ_SWEEP)
def test_adjoint_sweep(dev, cls, n, h):
    """Every irFFT family, hops below / at / above n_fft, the scalar and vec4 interiors at every residue of L - P - 1,
    hop | L, both folds in one frame (L = P + 1)."""
    m = (A.STFT if cls == "stft" else A.DGT)(n_fft=n, hop_length=h).to(dev)
    g = torch.Generator().manual_seed(_seed(cls, n, h))
    for L in C.adj_lengths(n, h):
        err = _check_adjoint(m, n, h, torch.randn(2, L, generator=g), g)
        assert err < TOL, (cls, n, h, L, C.adjoint_class(n, h, 2, L), err)
    # an odd frame count: a clip's frames start at every parity of the batch's frame index
    Ls = C.adj_lengths(n, h)
    L = next((v for v in Ls if C.frames(n, h, v) % 2 == 1), Ls[-1])
    _check_batch_bits(m, torch.randn(3, L, generator=g), g)


@pytest.mark.parametrize("cls", ["stft", "dgt"])
@pytest.mark.parametrize("n,h,L", C.FAST_HOP_DIVIDES)
def test_adjoint_when_hop_divides_the_length(dev, cls, n, h, L):
    """Training crops: the last frame covers the last padded sample, whose right-fold term lands on sample L - P - 1
    (the last lane of a vec4 group)."""
    m = (A.STFT if cls == "stft" else A.DGT)(n_fft=n, hop_length=h).to(dev)
    g = torch.Generator().manual_seed(_seed(cls, n, h, L))
    for shape in [(3, L), (2, 2, L + h)]:
        err = _check_adjoint(m, n, h, torch.randn(shape, generator=g), g)
        assert err < TOL, (cls, n, h, shape, err)
    _check_batch_bits(m, torch.randn(3, L, generator=g), g)


def _inner(a, b, step):
    """<a, b> summed in float64 on the device, `step` clips at a time (real, or complex as re/im pairs)."""
    s = 0.0
    for i in range(0, a.shape[0], step):
        ai, bi = a[i:i + step], b[i:i + step]
        if torch.is_complex(ai):
            s += float((ai.real.double() * bi.real.double()).sum() + (ai.imag.double() * bi.imag.double()).sum())
        else:
            s += float((ai.double() * bi.double()).sum())
    return s


@pytest.mark.parametrize("case", list(C.BIG_ADJ))
def test_big_adjoint(dev, case):
    """Several chunks with a short last one, a chunk of one clip, more clips than the grid has rows."""
    n, h, L, B, clips = C.BIG_ADJ[case]
    m = A.STFT(n_fft=n, hop_length=h).to(dev)
    g = torch.Generator(device=dev).manual_seed(_seed(case))
    x = torch.randn(B, L, device=dev, generator=g)
    xr = x.clone().requires_grad_()
    X = m(xr)
    G = torch.randn(X.shape, dtype=torch.complex64, device=dev, generator=g)
    step = max(1, B // 16)
    lhs = _inner(X.detach(), G, step)
    X.backward(G)
    del X
    dx = xr.grad
    rhs = _inner(x, dx, step)
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (case, lhs, rhs)
    w = m.window[:n]
    for k in clips:
        if case == "chunk_of_one":
            # a float64 CPU reference of 300000 frames is heavy: torch's float64 autograd on the device instead
            x64 = x[k:k + 1].double().requires_grad_()
            Xk = torch.stft(x64, n, h, window=w.double(), center=True, pad_mode="reflect",
                            return_complex=True).transpose(-2, -1)
            Xk.backward(G[k:k + 1].to(torch.complex128))
            ref = x64.grad
            del Xk
        else:
            ref = ref_stft_grad(x[k:k + 1], w, n, h, G[k:k + 1])
        err = rel_max(cpu(dx[k:k + 1]), cpu(ref))
        assert err < TOL, (case, k, err)
        # a clip's bits do not depend on the batch it rides in or on the chunk it falls into
        xk = x[k:k + 1].clone().requires_grad_()
        m(xk).backward(G[k:k + 1])
        assert torch.equal(xk.grad[0], dx[k]), (case, k)


# ---- Magnitude backward ---------------------------------------------------------------------------------------------

def _mag_input(complex_in, g, rows, K):
    """test_autograd_gpu._mag_input for any row shape and K: exact zeros and values straddling eps."""
    shape = tuple(rows) + (K,)
    mag = torch.rand(shape, generator=g) * 4
    flat = mag.view(-1, K)
    eps = torch.finfo(torch.float32).eps
    R = flat.shape[0]
    z = min(40, K // 4)
    flat[0, :z] = 0.0
    a = K // 4
    n = min(60, K - a) // 2 * 2
    flat[min(1, R - 1), a:a + n] = eps * torch.tensor([0.3, 3.0]).repeat(n // 2)
    flat[R - 1, K // 2:K // 2 + 100] = 0.0
    if not complex_in:
        return mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    ph = torch.rand(shape, generator=g) * 6.283
    return torch.polar(mag, ph)


def _mag_grad(mod, x, dF):
    xd = x.to(mod.eps.device).requires_grad_()
    f = mod(xd)
    assert f.grad_fn is not None
    f.backward(dF.to(xd.device))
    return xd.grad


def _mag_ref(mod, x, dF):
    x64 = x.detach().cpu().to(torch.complex128 if torch.is_complex(x) else torch.float64).requires_grad_()
    ref = _ref_magnitude(x64, mod)
    ref.backward(dF.detach().cpu().double())
    return x64.grad


@pytest.mark.parametrize("complex_in", [True, False])
@pytest.mark.parametrize("contrast,norm", C.MAG_MODES)
@pytest.mark.parametrize("name", [c[0] for c in C.MAG_CASES])
def test_magnitude_paths(dev, name, contrast, norm, complex_in):
    """One case per backward kernel (tables in LDS with and without the row in registers, LDS past 64 KB, tables in
    global memory at 4 and 2 waves per workgroup, pointwise), bank edges, keep_nyquist=False, bf16 forward, row counts
    that leave waves idle."""
    _, kw, rows = next(c for c in C.MAG_CASES if c[0] == name)
    mod = C.magnitude_module(dict(kw, mode=norm, contrast=contrast), seed=_seed(name)).to(dev)
    K = mod.n_fft // 2 + 1
    g = torch.Generator().manual_seed(_seed(name, contrast, norm, complex_in))
    x = _mag_input(complex_in, g, rows, K)
    mod.scale_data(x.to(dev))
    f = mod(x.to(dev))
    dF = torch.randn(f.shape, generator=g)
    got = _mag_grad(mod, x, dF)
    assert got.dtype == x.dtype and got.shape == x.shape
    want = _mag_ref(mod, x, dF)
    got = cpu(got)
    err = rel_max(got, want.numpy())
    assert err < TOL, (name, contrast, norm, complex_in, C.module_class(mod), err)
    assert np.all(got[x.numpy() == 0] == 0)                  # torch's sgn(0) = 0


def _spread_rows(R):
    """About 20 rows: the ends, and both sides of multiples of 4 x CUs (a grid-stride pass covers 4 rows per
    workgroup, and the grid is a multiple of the CU count)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = {0, 1, R - 2, R - 1}
    k = 1
    while len(rows) < 20 and 4 * cus * k < R:
        rows |= {4 * cus * k - 1, 4 * cus * k}
        k = k * 2 + 1
    return sorted(r for r in rows if 0 <= r < R)


@pytest.mark.parametrize("which", list(C.MANY_ROWS))
def test_magnitude_many_rows(dev, which):
    kw, rows = C.MANY_ROWS[which]
    mod = C.magnitude_module(kw).to(dev)
    K = mod.n_fft // 2 + 1
    g = torch.Generator(device=dev).manual_seed(_seed(which))
    shape = tuple(rows) + (K,)
    x = torch.polar(torch.rand(shape, device=dev, generator=g) * 4, torch.rand(shape, device=dev, generator=g) * 6.283)
    x.view(-1, K)[::7, :64] = 0.0
    mod.scale_data(x)
    xr = x.requires_grad_()
    f = mod(xr)
    dF = torch.randn(f.shape, device=dev, generator=g)
    f.backward(dF)
    dx = xr.grad.view(-1, K)
    xf, dFf = x.detach().view(-1, K), dF.view(-1, dF.shape[-1])
    R = xf.shape[0]
    pick = _spread_rows(R)
    assert len(pick) >= 16
    idx = torch.tensor(pick, device=dev)
    want = _mag_ref(mod, xf[idx], dFf[idx])
    err = rel_max(cpu(dx[idx]), want.numpy())
    assert err < TOL, (which, err)
    # a sub-block of rows alone: the same bits
    a = pick[len(pick) // 2] - 5
    sub = _mag_grad(mod, xf[a:a + 37].clone(), dFf[a:a + 37].clone())
    assert torch.equal(sub, dx[a:a + 37]), which


# ---- module level ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hop", [128, 512])
@pytest.mark.parametrize("fused", [True, False])
def test_stft_magnitude_chain_at_other_hops(dev, hop, fused):
    """test_autograd_gpu.test_stft_magnitude_chain at the other hops the fused forward takes."""
    stft = A.STFT(hop_length=hop).to(dev)
    mag = A.Magnitude(n_mels=128).to(dev)
    g = torch.Generator().manual_seed(_seed("chain", hop, fused))
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


@pytest.mark.parametrize("hop", [128, 512])
def test_fused_chain_with_the_spectrum_in_the_loss_at_other_hops(dev, hop):
    stft = A.STFT(hop_length=hop).to(dev)
    mag = A.Magnitude(n_mels=128).to(dev)
    g = torch.Generator().manual_seed(_seed("chain_spectrum", hop))
    x = torch.randn(2, 12000, generator=g) * 0.1
    mag.scale_data(stft(x.to(dev)))
    assert mag.can_fuse_with(stft, x.to(dev))
    xr = x.to(dev).requires_grad_()
    X, feat = mag.forward_fused(stft, xr, return_spectrum=True)
    dF = torch.randn(feat.shape, generator=g)
    G = torch.randn(X.shape, dtype=torch.complex64, generator=g)
    torch.autograd.backward([feat, X], [dF.to(dev), G.to(dev)])
    x64, X64, ref = _ref_chain(x, stft, mag)
    torch.autograd.backward([ref, X64], [dF.double(), G.to(torch.complex128)])
    assert rel_max(cpu(xr.grad), x64.grad.numpy()) < TOL


@pytest.mark.parametrize("how", ["load_state_dict", "in_place"])
def test_bank_tables_follow_the_bank(dev, how):
    """The backward's band tables are cached per bank version: a bank replaced by load_state_dict, or edited in place,
    gives the gradient of the new bank."""
    mod = A.Magnitude(n_mels=128).to(dev)
    g = torch.Generator().manual_seed(_seed("cache", how))
    x = _mag_input(True, g, (2, 5), 513)
    mod.scale_data(x.to(dev))
    dF = torch.randn(2, 5, 128, generator=g)
    first = _mag_grad(mod, x, dF)
    assert rel_max(cpu(first), _mag_ref(mod, x, dF).numpy()) < TOL
    if how == "load_state_dict":
        sd = mod.state_dict()
        sd["mel_bank"] = sd["mel_bank"] * (0.5 + torch.rand(1, 513, 1, generator=g)).to(dev)
        mod.load_state_dict(sd)
    else:
        with torch.no_grad():
            mod.mel_bank.mul_(2.5)
    again = _mag_grad(mod, x, dF)
    want = _mag_ref(mod, x, dF)
    assert rel_max(cpu(again), want.numpy()) < TOL
    assert rel_max(cpu(first), want.numpy()) > 1e-3             # the new bank's gradient is another one


def test_grads_on_a_side_stream_are_the_default_streams(dev):
    stft = A.STFT().to(dev)
    mag = A.Magnitude(n_fft=1024, n_mels=128).to(dev)
    g = torch.Generator(device=dev).manual_seed(_seed("stream"))
    x = torch.randn(4, 30000, device=dev, generator=g) * 0.1
    mag.scale_data(stft(x))
    T = 1 + 30000 // 256
    dF = torch.randn(4, T, 128, device=dev, generator=g)
    G = torch.randn(4, T, 513, dtype=torch.complex64, device=dev, generator=g)

    def run():
        xr = x.clone().requires_grad_()
        X = stft(xr)
        torch.autograd.backward([mag(X), X], [dF, G])
        xs = x.clone().requires_grad_()
        mag.forward_fused(stft, xs).backward(dF)
        return xr.grad, xs.grad

    base = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run()
    s.synchronize()
    for a, b in zip(base, side):
        assert torch.equal(a, b)

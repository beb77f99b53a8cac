"""Gradients through MFCC (autograd.MfccFunction: the STFT recomputed per chunk of clips, at_mfcc_backward in place on
it, the STFT adjoint) against torch autograd, in float64 on the CPU, of the reference's expression from the same fp32
inputs: torch.stft(center, reflect) with the module's window, abs() ** power, matmul with the module's fbank, the
transpose, the optional clamp / log10 / DCT, (y - offset) / scale.  Metric: conftest.rel_max.

Tolerances.  Mel power route (n_mfcc None): 1e-5, the project's.  n_mfcc route: it divides by mel sums that come close to
zero, and plain fp32 torch autograd of the same expression is itself up to 2e-5 from float64 on some of these inputs; so
each case computes e32 = rel_max(fp32 CPU torch autograd, float64) from the same inputs and asserts the kernel within
max(1e-5, 4 e32) -- the factor 4 because the kernel's FFT and band-walk summation orders differ from torch's and 1 / M
amplifies whichever error lands on the smallest sums.  Every case prints its figures (run with -s);
profiles/mfcc_grad_probe.md records them."""
import math
import zlib

import pytest
import torch

import acids_transforms_amd as A
import mfcc_grad_cases as C
from acids_transforms_amd import ops
from acids_transforms_amd.autograd import _mfcc_tables
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
MIB = 1 << 20


def cpu(t):
    return t.detach().cpu().numpy()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def ref_grad(x, mod, dF, dtype=torch.float64):
    """x.grad of the reference's expression fed dF, on the CPU in `dtype`, from the module's own buffers."""
    xr = x.detach().cpu().to(dtype).requires_grad_()
    xb = xr.reshape(-1, xr.shape[-1])
    X = torch.stft(xb, mod.n_fft, mod.hop_length, window=mod.window.detach().cpu().to(dtype), center=True,
                   pad_mode="reflect", return_complex=True)                                  # (B, F, T)
    a = X.abs() ** int(mod.power)
    y = torch.matmul(a.transpose(-1, -2), mod.fbank.detach().cpu().to(dtype)).transpose(-1, -2)   # (B, n_mels, T)
    if mod.n_mfcc is not None:
        db = 10.0 * torch.log10(torch.clamp(y, min=1e-10)).transpose(-1, -2)
        dct = mod.dct.detach().cpu().to(dtype) * (math.log(10.0) / 10.0)      # the buffer carries the 10 / ln 10
        y = torch.matmul(db, dct).transpose(-1, -2)
    if mod.norm is not None:
        y = (y - mod.norm.offset.detach().cpu().to(dtype)) / mod.norm.scale.detach().cpu().to(dtype)
    y.backward(dF.detach().cpu().to(dtype).reshape(y.shape))
    return xr.grad


def run_case(dev, mod, x, g):
    """(kernel's rel_max against float64, fp32 torch's rel_max against float64) of one module on one batch."""
    if mod.norm is not None:
        mod.scale_data(x.to(dev))
    xd = x.to(dev).requires_grad_()
    y = mod(xd)
    assert y.grad_fn is not None
    dF = torch.randn(y.shape, generator=g)
    y.backward(dF.to(dev))
    assert xd.grad.shape == x.shape and xd.grad.dtype == torch.float32
    assert bool(torch.isfinite(xd.grad).all())
    want = ref_grad(x, mod, dF).numpy()
    e32 = rel_max(ref_grad(x, mod, dF, torch.float32).numpy(), want)
    return rel_max(cpu(xd.grad), want), e32


def test_mfcc_no_longer_cuts_the_graph(dev):
    m = A.MFCC().to(dev)
    x = (torch.randn(2, 9000, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev).requires_grad_()
    y = m(x)
    assert y.requires_grad and y.grad_fn is not None
    y.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    assert float(x.grad.abs().max()) > 0


@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("power", C.POWERS)
@pytest.mark.parametrize("case", C.SIZES, ids=[c[0] for c in C.SIZES])
def test_parity_grid(dev, case, power, norm):
    name, n, h, n_mels, _ = case
    for n_mfcc in C.n_mfcc_of(n_mels):
        mod = C.module_of(case, power=power, n_mfcc=n_mfcc, norm=norm).to(dev)
        g = torch.Generator().manual_seed(_seed(name, power, norm, n_mfcc))
        for shape in C.shapes_of(case):
            x = torch.randn(shape, generator=g) * 0.1
            err, e32 = run_case(dev, mod, x, g)
            tol = TOL if n_mfcc is None else max(TOL, 4 * e32)
            print("MFCCGRAD %s power=%d norm=%s n_mfcc=%s shape=%s class=%s path=%s e32=%.3e kernel=%.3e tol=%.3e"
                  % (name, power, norm, n_mfcc, tuple(shape), C.module_class(mod), C.forward_path(mod, shape[-1]), e32,
                     err, tol))
            assert err <= tol, (name, power, norm, n_mfcc, shape, err, e32)


FORWARD_CASES = [("1024_even", None, 9000, "fused"), ("1024_even", 40, 9000, "fused_dct"),
                 ("2048_m128", None, 30000, "single"), ("512_m64", 40, 9001, "single_dct"),
                 ("1024_odd", None, 9001, "generic"), ("400_m40", 40, 16000, "generic_dct")]


@pytest.mark.parametrize("name,n_mfcc,L,path", FORWARD_CASES)
def test_forward_is_bit_identical_and_builds_no_stray_graph(dev, name, n_mfcc, L, path):
    case = next(c for c in C.SIZES if c[0] == name)
    mod = C.module_of(case, n_mfcc=n_mfcc, norm="gaussian").to(dev)
    assert C.forward_path(mod, L) == path
    x = (torch.randn(3, L, generator=torch.Generator().manual_seed(_seed(name, n_mfcc))) * 0.1).to(dev)
    mod.scale_data(x)
    plain = mod(x)
    assert plain.grad_fn is None and not plain.requires_grad
    y = mod(x.clone().requires_grad_())
    assert y.grad_fn is not None and torch.equal(plain, y.detach())
    with torch.no_grad():
        assert mod(x.clone().requires_grad_()).grad_fn is None
    with pytest.raises(RuntimeError):
        xx = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad(mod(xx).sum(), xx, create_graph=True)
        gx.sum().backward()


def test_other_gradient_inputs(dev):
    """A gradient that is not contiguous, a half-precision input (widened, as by the forward), and the norm statistics,
    which are constants of the graph."""
    mod = A.MFCC(norm_mode="gaussian").to(dev)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 9000, generator=g) * 0.1
    mod.scale_data(x.to(dev))
    xd = x.to(dev).requires_grad_()
    y = mod(xd)
    dF = torch.randn(y.shape, generator=g)
    strided = torch.empty(y.shape[0], y.shape[2], y.shape[1], device=dev).transpose(1, 2)    # (B, C, T), T-major
    strided.copy_(dF.to(dev))
    assert not strided.is_contiguous()
    y.backward(strided)
    assert rel_max(cpu(xd.grad), ref_grad(x, mod, dF).numpy()) < TOL
    assert mod.norm.offset.grad is None and mod.norm.scale.grad is None
    xh = x.half().to(dev).requires_grad_()
    mod(xh).sum().backward()
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == x.shape


# ---- zeros -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,L", [("1024_even", 9000), ("1024_odd", 9001), ("2048_m128", 30000), ("400_m40", 16000),
                                    ("16384_m128", 50000)])
def test_a_silent_clip_gets_zero_gradient(dev, name, L):
    case = next(c for c in C.SIZES if c[0] == name)
    g = torch.Generator().manual_seed(_seed("silent", name))
    x = torch.randn(3, L, generator=g) * 0.1
    x[1] = 0.0
    for power in C.POWERS:
        for n_mfcc in C.n_mfcc_of(case[3]):
            mod = C.module_of(case, power=power, n_mfcc=n_mfcc).to(dev)
            xd = x.to(dev).requires_grad_()
            y = mod(xd)
            y.backward(torch.randn(y.shape, generator=g).to(dev))
            assert bool(torch.isfinite(xd.grad).all()), (name, power, n_mfcc)
            assert bool((xd.grad[1] == 0).all()), (name, power, n_mfcc)
            assert float(xd.grad[0].abs().max()) > 0 and float(xd.grad[2].abs().max()) > 0


def _kernel_case(dev, mod, g, T=37):
    """A spectrum with exact-zero bins and a silent frame, a gradient, and the kernel's operands."""
    K = mod.n_fft // 2 + 1
    X = torch.randn(2, T, K, dtype=torch.complex64, generator=g)
    X[0, 0, :40] = 0.0
    X[1, 3, 100:200] = 0.0
    X[1, 5] = 0.0
    C_out = mod.n_mfcc if mod.n_mfcc is not None else mod.n_mels
    dF = torch.randn(2, C_out, T, generator=g)
    fwd, inv, dct_t = _mfcc_tables(mod, dev)
    return X, dF, fwd, inv, dct_t


def _ref_from_spectrum(X, dF, mod, ctype=torch.complex128):
    rtype = torch.float64 if ctype == torch.complex128 else torch.float32
    Xr = X.to(ctype).requires_grad_()
    y = torch.matmul(Xr.abs() ** int(mod.power), mod.fbank.detach().cpu().to(rtype)).transpose(-1, -2)
    if mod.n_mfcc is not None:
        y = torch.matmul(torch.log(torch.clamp(y, min=1e-10)).transpose(-1, -2),
                         mod.dct.detach().cpu().to(rtype)).transpose(-1, -2)
    y.backward(dF.to(rtype))
    return Xr.grad


@pytest.mark.parametrize("n_mfcc", [None, 40])
@pytest.mark.parametrize("power", [1, 2])
def test_kernel_on_a_spectrum_with_exact_zeros_in_place_and_out_of_place(dev, power, n_mfcc):
    """The kernel alone: exact-zero bins get exactly zero (torch's sgn for power 1), a silent frame too; writing over
    X gives the bits of writing elsewhere; T = 37 leaves a short second tile."""
    mod = A.MFCC(power=power, n_mfcc=n_mfcc).to(dev)
    g = torch.Generator().manual_seed(_seed("zeros", power, n_mfcc))
    X, dF, fwd, inv, dct_t = _kernel_case(dev, mod, g)
    Xd = X.to(dev)
    out = ops.mfcc_backward(Xd, dF.to(dev), inv, power, fwd, dct_t)
    assert torch.equal(Xd, X.to(dev))                                     # out of place: X untouched
    want = torch.view_as_real(_ref_from_spectrum(X, dF, mod)).numpy()
    e32 = rel_max(torch.view_as_real(_ref_from_spectrum(X, dF, mod, torch.complex64)).numpy(), want)
    tol = TOL if n_mfcc is None else max(TOL, 4 * e32)          # as in the parity grid
    assert rel_max(cpu(torch.view_as_real(out)), want) <= tol, e32
    zero = (X == 0)
    assert bool((out.cpu()[zero] == 0).all()) and bool(torch.isfinite(torch.view_as_real(out)).all())
    inplace = ops.mfcc_backward(Xd, dF.to(dev), inv, power, fwd, dct_t, inplace=True)
    assert inplace.data_ptr() == Xd.data_ptr() and torch.equal(torch.view_as_real(inplace), torch.view_as_real(out))


def test_the_empty_filter_gets_zero_gradient(dev):
    """The 128-mel bank at n_fft 1024 has one all-zero column: its mel sum is 0, below the clamp, so whatever reaches it
    through the DCT flows no further (and divides nothing by zero)."""
    mod = A.MFCC(n_mfcc=40).to(dev)
    empty = torch.nonzero(mod.fbank.sum(0) == 0).flatten().tolist()
    assert len(empty) == 1
    g = torch.Generator().manual_seed(4)
    X, dF, fwd, inv, dct_t = _kernel_case(dev, mod, g)
    only = torch.zeros_like(dct_t)
    only[:, empty[0]] = 1.0                     # a "DCT" that reads the empty filter alone
    out = ops.mfcc_backward(X.to(dev), dF.to(dev), inv, 2, fwd, only)
    assert bool((torch.view_as_real(out) == 0).all())
    # and through the module, against float64
    x = torch.randn(2, 9000, generator=g) * 0.1
    err, e32 = run_case(dev, mod, x, g)
    assert err <= max(TOL, 4 * e32), (err, e32)


# ---- the bench size: 1024 clips x 4 s ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bench_audio(dev):
    n, h, L, B = C.BENCH
    g = torch.Generator(device=dev).manual_seed(3)
    return torch.randn(B, L, device=dev, generator=g) * 0.1


@pytest.mark.parametrize("n_mfcc", [None, 40])
def test_grad_bits_do_not_depend_on_the_batch_or_the_chunk(dev, bench_audio, n_mfcc):
    x = bench_audio
    m = A.MFCC(n_mfcc=n_mfcc).to(dev)
    xr = x.clone().requires_grad_()
    y = m(xr)
    G = torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    y.backward(G)
    del y
    dx = xr.grad
    assert bool(torch.isfinite(dx).all())
    for k in C.BENCH_CLIPS:
        xk = x[k:k + 1].clone().requires_grad_()
        m(xk).backward(G[k:k + 1])
        assert torch.equal(xk.grad[0], dx[k]), k
    # a NaN planted in clip 5 stays there
    xn = x.clone()
    xn[5, 1000] = float("nan")
    xn.requires_grad_()
    m(xn).backward(G)
    keep = torch.arange(x.shape[0], device=dev) != 5
    assert torch.equal(xn.grad[keep], dx[keep])
    assert bool(torch.isnan(xn.grad[5]).any())


@pytest.mark.parametrize("n_mfcc", [None, 40])
def test_the_graph_holds_the_audio_only(dev, bench_audio, n_mfcc):
    """After the forward the graph holds nothing but the feature tensor (the saved audio is the caller's); the backward
    peaks at dx plus one chunk: 0.5 GiB of spectrum, turned into its gradient in place, 0.5 GiB of adjoint workspace
    and the allocator's rounding.  (A saved spectrum alone would be 2.9 GB.)"""
    m = A.MFCC(n_mfcc=n_mfcc).to(dev)
    m(bench_audio[:2])                                  # tables and lazy state
    xr = bench_audio.detach().requires_grad_()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    y = m(xr)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated(dev) - before
    assert grown <= y.numel() * 4 + 16 * MIB, (grown, y.numel() * 4)
    G = torch.ones_like(y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    level = torch.cuda.memory_allocated(dev)
    y.backward(G)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - level
    dx_bytes = xr.numel() * 4
    print("MFCCGRAD memory n_mfcc=%s forward_growth=%.1f MiB features=%.1f MiB backward_rise=%.1f MiB dx=%.1f MiB"
          % (n_mfcc, grown / MIB, y.numel() * 4 / MIB, rise / MIB, dx_bytes / MIB))
    assert rise <= dx_bytes + 1536 * MIB, (rise, dx_bytes)
    assert xr.grad.shape == xr.shape


def test_adjoint_identity_at_bench_size(dev, bench_audio):
    """MFCC(power=1) is homogeneous of degree 1 in the audio, so <x, dx> = <y, G> (Euler); G is positive so that
    neither inner product cancels.  Accumulated in float64 in slices."""
    x = bench_audio
    m = A.MFCC(power=1).to(dev)
    xr = x.detach().requires_grad_()
    y = m(xr)
    G = torch.rand(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) + 0.5
    rhs = 0.0
    for i in range(0, x.shape[0], 64):
        rhs += float((y[i:i + 64].detach().double() * G[i:i + 64].double()).sum())
    y.backward(G)
    lhs = 0.0
    for i in range(0, x.shape[0], 64):
        lhs += float((x[i:i + 64].double() * xr.grad[i:i + 64].double()).sum())
    print("MFCCGRAD adjoint_identity <x,dx>=%.9e <y,G>=%.9e rel=%.3e" % (lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)

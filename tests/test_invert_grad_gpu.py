"""Gradients through the invert of Magnitude, Polar, Cartesian, Real / Imaginary / Phase (at_magnitude_invert_backward,
at_polar_to_complex_backward, at_cartesian_unpack_backward; autograd.MagnitudeInvertFunction and its neighbours) against
torch autograd of the reference's own expressions, built from the modules' buffers, in float64 on the CPU.  Tolerance:
normwise rel_max < 1e-5, as for every other gradient.  The sweep and the dispatch classes it reaches are in
invert_grad_cases.py (checked by test_invert_grad_cases_cpu.py).

Inputs: the forward features of a random complex spectrum the module was scaled on, plus 0.05 randn; phases uniform in
+-pi (normalised as the module would)."""
import math
import zlib

import pytest
import torch

import acids_transforms_amd as A
import grad_cases as G
import invert_grad_cases as C
from acids_transforms_amd import autograd as AG
from acids_transforms_amd import ops
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
NOISE = 0.05


def cpu(t):
    return t.detach().cpu().numpy()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _spectrum(g, shape):
    return torch.randn(shape, dtype=torch.complex64, generator=g)


def _features(mod, X, g):
    """mod scaled on X, then mod(X) + 0.05 randn (on mod's device)."""
    dev = mod.eps.device if hasattr(mod, "eps") else X.device
    Xd = X.to(dev)
    mod.scale_data(Xd)
    f = mod(Xd)
    return (f + NOISE * torch.randn(f.shape, generator=g).to(f.device)).contiguous()


def _phase_features(rep, g, shape, dev):
    """Phases uniform in +-pi as `rep` (a Phase) would emit them, keep_nyquist applied."""
    phi = (torch.rand(shape, generator=g) * 2 - 1) * math.pi
    off, sc = C.affine_params(rep)
    y = (phi - off) / sc if off is not None else phi
    return (y if rep.keep_nyquist else y[..., 1:]).contiguous().to(dev)


def _grad_of(fn, y, gout):
    yr = y.detach().clone().requires_grad_()
    out = fn(yr)
    assert out.grad_fn is not None
    out.backward(gout)
    assert yr.grad.shape == y.shape and yr.grad.dtype == y.dtype
    return out.detach(), yr.grad


def _ref(fn, y, gout):
    return C.autograd_of(fn, y.detach().cpu(), gout.detach().cpu().to(torch.complex128 if gout.is_complex() else torch.float64))


def _randn_like_out(out, g):
    return torch.randn(out.shape, dtype=out.dtype, generator=g).to(out.device)


# ---- Magnitude.invert: every case x mode of the sweep -------------------------------------------------------------------

@pytest.mark.parametrize("contrast,norm", C.MAG_MODES)
@pytest.mark.parametrize("name", [c[0] for c in C.MAG_CASES])
def test_magnitude_invert_paths(dev, name, contrast, norm):
    _, kw, rows = next(c for c in C.MAG_CASES if c[0] == name)
    mod = G.magnitude_module(dict(kw, mode=norm, contrast=contrast), seed=_seed(name)).to(dev)
    g = torch.Generator().manual_seed(_seed(name, contrast, norm))
    F = mod.n_fft // 2 + 1
    y = _features(mod, _spectrum(g, tuple(rows) + (F,)), g)
    with torch.no_grad():
        gout = _randn_like_out(mod.invert(y), g)
    out, got = _grad_of(mod.invert, y, gout)
    assert out.shape[-1] == F
    p = C.magnitude_params(mod)
    want = _ref(lambda t: C.ref_magnitude_invert(t, p), y, gout)
    err = rel_max(cpu(got), want.numpy())
    print(name, contrast, norm, C.module_plan(mod)[0], "max|y| %.2f" % float(y.abs().max()), "err %.3g" % err)
    assert err < TOL, (name, contrast, norm, C.module_plan(mod), err)


def _polar_op(mod, y, gX, po, ps):
    """The polar form of the kernel, called as autograd.PolarInvertFunction calls it."""
    dev = y.device
    off, sc = mod._affine()
    return ops.magnitude_invert_backward(y, gX, AG._inverse_bank_tables(mod, dev), mod.contrast_mode, off, sc, mod._eps,
                                         bank_cols=AG._inverse_bank_tables(mod, dev, forward=True), phase_offset=po,
                                         phase_scale=ps)


@pytest.mark.parametrize("contrast,norm", C.MAG_MODES)
@pytest.mark.parametrize("name", [c[0] for c in C.POLAR_CASES])
def test_polar_form_paths(dev, name, contrast, norm):
    """The polar form at every bank size of the sweep (the module's one-pass route stops where the banded forward
    projection does; the kernel does not), with a phase Normalize."""
    _, kw, rows = next(c for c in C.POLAR_CASES if c[0] == name)
    mod = G.magnitude_module(dict(kw, mode=norm, contrast=contrast)).to(dev)
    g = torch.Generator().manual_seed(_seed("polar", name, contrast, norm))
    F = mod.n_fft // 2 + 1
    ymag = _features(mod, _spectrum(g, tuple(rows) + (F,)), g)
    po, ps = 0.25, math.pi
    yph = (((torch.rand(ymag.shape, generator=g) * 2 - 1) * math.pi - po) / ps).to(dev)
    y = torch.stack([ymag, yph], -2).contiguous()
    gX = torch.randn(ymag.shape, dtype=torch.complex64, generator=g).to(dev)
    got = _polar_op(mod, y, gX, torch.tensor(po, device=dev), torch.tensor(ps, device=dev))
    assert got.shape == y.shape
    p = C.magnitude_params(mod)
    want = _ref(lambda t: C.ref_polar_invert(t, p, po, ps), y, gX).numpy()
    got = cpu(got)
    e_mag, e_ph = rel_max(got[..., 0, :], want[..., 0, :]), rel_max(got[..., 1, :], want[..., 1, :])
    print(name, contrast, norm, C.module_plan(mod, True)[0], "err mag %.3g phase %.3g" % (e_mag, e_ph))
    assert e_mag < TOL and e_ph < TOL, (name, contrast, norm, C.module_plan(mod, True), e_mag, e_ph)


# ---- Polar, Cartesian, Real / Imaginary / Phase at F = 513 and 1025 ------------------------------------------------------

def _polar_setup(dev, n_fft, g, shape=(2, 5), **kw):
    rep = A.Polar(magnitude_args={"mode": "bipolar", "n_fft": n_fft}, **kw).to(dev)
    F = n_fft // 2 + 1
    X = _spectrum(g, tuple(shape) + (F,)).to(dev)
    rep.scale_data(X)
    ymag = rep.magnitude(X)
    ymag = ymag + NOISE * torch.randn(ymag.shape, generator=g).to(dev)
    yph = _phase_features(rep.phase, g, tuple(shape) + (F,), dev)
    return rep, ymag.contiguous(), yph


def _polar_ref(rep):
    p = C.magnitude_params(rep.magnitude)
    po, ps = C.affine_params(rep.phase)
    return lambda t: C.ref_polar_invert(t, p, po, ps)


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_polar_invert_fused(dev, n_fft):
    g = torch.Generator().manual_seed(n_fft)
    rep, ymag, yph = _polar_setup(dev, n_fft, g)
    y = torch.stack([ymag, yph], -2)
    with torch.no_grad():
        assert rep._one_pass_invert(y) is not None            # the one-pass route takes this module and shape
    gX = torch.randn(ymag.shape, dtype=torch.complex64, generator=g).to(dev)
    _, got = _grad_of(rep.invert, y, gX)
    want = _ref(_polar_ref(rep), y, gX).numpy()
    got = cpu(got)
    assert rel_max(got[..., 0, :], want[..., 0, :]) < TOL and rel_max(got[..., 1, :], want[..., 1, :]) < TOL


@pytest.mark.parametrize("how", ["stack_none", "mel_off", "nonyq"])
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_polar_invert_unfused(dev, n_fft, how):
    """SpectralRepresentation.invert's composition: Magnitude.invert, Phase.invert and polar_to_complex, each with its own
    backward; a tuple input (stack=None) is routed per part."""
    g = torch.Generator().manual_seed(n_fft + 1)
    F = n_fft // 2 + 1
    margs = {"mode": "bipolar", "n_fft": n_fft}
    if how == "stack_none":
        rep = A.Polar(magnitude_args=margs, stack=None)
    elif how == "mel_off":
        rep = A.Polar(magnitude_args=dict(margs, mel=False))
    else:
        rep = A.Polar(magnitude_args=margs, keep_nyquist=False)
    rep = rep.to(dev)
    X = _spectrum(g, (2, 5, F)).to(dev)
    rep.scale_data(X)
    ymag = rep.magnitude(X)
    ymag = (ymag + NOISE * torch.randn(ymag.shape, generator=g).to(dev)).contiguous()
    yph = _phase_features(rep.phase, g, (2, 5, F), dev)
    gX = torch.randn(2, 5, F, dtype=torch.complex64, generator=g).to(dev)
    p = C.magnitude_params(rep.magnitude)
    po, ps = C.affine_params(rep.phase)
    kn = rep.keep_nyquist

    def ref(mag, ph):
        return C.ref_magnitude_invert(mag, p) * torch.exp(1j * C.ref_affine_invert(ph, po, ps, kn))

    m64 = ymag.detach().cpu().double().requires_grad_()
    p64 = yph.detach().cpu().double().requires_grad_()
    ref(m64, p64).backward(gX.cpu().to(torch.complex128))
    if how == "stack_none":
        a, b = ymag.clone().requires_grad_(), yph.clone().requires_grad_()
        out = rep.invert((a, b))
        assert out.grad_fn is not None
        out.backward(gX)
        gm, gp = a.grad, b.grad
        # one part alone: the other gets no gradient and the values stay the same bits
        a2 = ymag.clone().requires_grad_()
        out2 = rep.invert((a2, yph))
        out2.backward(gX)
        assert torch.equal(out2.detach(), out.detach()) and torch.equal(a2.grad, gm)
    else:
        y = torch.stack([ymag, yph], -2)
        with torch.no_grad():
            assert rep._one_pass_invert(y) is None
        _, gy = _grad_of(rep.invert, y, gX)
        gm, gp = gy[..., 0, :], gy[..., 1, :]
    assert rel_max(cpu(gm), m64.grad.numpy()) < TOL and rel_max(cpu(gp), p64.grad.numpy()) < TOL


def test_fused_polar_gradient_equals_the_unfused_composition(dev):
    g = torch.Generator().manual_seed(77)
    rep, ymag, yph = _polar_setup(dev, 1024, g)
    y = torch.stack([ymag, yph], -2)
    gX = torch.randn(ymag.shape, dtype=torch.complex64, generator=g).to(dev)
    out_f, fused = _grad_of(rep.invert, y, gX)

    def unfused(t):
        return AG.PolarToComplexFunction.apply(rep.magnitude.invert(t[..., 0, :]), rep.phase.invert(t[..., 1, :]))

    out_u, parts = _grad_of(unfused, y, gX)
    assert rel_max(cpu(torch.view_as_real(out_f)), cpu(torch.view_as_real(out_u))) < TOL
    assert rel_max(cpu(fused[..., 0, :]), cpu(parts[..., 0, :])) < TOL
    assert rel_max(cpu(fused[..., 1, :]), cpu(parts[..., 1, :])) < TOL


def _cartesian_setup(dev, F, g, **kw):
    rep = A.Cartesian(**kw).to(dev)
    X = _spectrum(g, (2, 5, F)).to(dev)
    rep.scale_data(X)
    y = rep(X)
    if isinstance(y, tuple):
        return rep, tuple((t + NOISE * torch.randn(t.shape, generator=g).to(dev)).contiguous() for t in y)
    return rep, (y + NOISE * torch.randn(y.shape, generator=g).to(dev)).contiguous()


@pytest.mark.parametrize("norms", [("gaussian", "gaussian"), (None, "unipolar")])
@pytest.mark.parametrize("F", [513, 1025])
def test_cartesian_invert_fused(dev, F, norms):
    g = torch.Generator().manual_seed(F + 2)
    rep, y = _cartesian_setup(dev, F, g, real_args={"mode": norms[0]}, imag_args={"mode": norms[1]})
    assert rep._one_pass_ok(y, True)
    gX = torch.randn(2, 5, F, dtype=torch.complex64, generator=g).to(dev)
    _, got = _grad_of(rep.invert, y, gX)
    ra, ia = C.affine_params(rep.magnitude), C.affine_params(rep.phase)
    want = _ref(lambda t: C.ref_cartesian_invert(t, ra, ia), y, gX)
    assert rel_max(cpu(got), want.numpy()) < TOL


@pytest.mark.parametrize("F", [513, 1025])
def test_cartesian_invert_stack_none(dev, F):
    g = torch.Generator().manual_seed(F + 3)
    rep, (yr, yi) = _cartesian_setup(dev, F, g, stack=None)
    gX = torch.randn(2, 5, F, dtype=torch.complex64, generator=g).to(dev)
    a, b = yr.clone().requires_grad_(), yi.clone().requires_grad_()
    out = rep.invert((a, b))
    assert out.grad_fn is not None
    out.backward(gX)
    ra, ia = C.affine_params(rep.magnitude), C.affine_params(rep.phase)
    r64, i64 = yr.cpu().double().requires_grad_(), yi.cpu().double().requires_grad_()
    (C.ref_affine_invert(r64, *ra) + 1j * C.ref_affine_invert(i64, *ia)).backward(gX.cpu().to(torch.complex128))
    assert rel_max(cpu(a.grad), r64.grad.numpy()) < TOL and rel_max(cpu(b.grad), i64.grad.numpy()) < TOL


@pytest.mark.parametrize("keep_nyquist", [True, False])
@pytest.mark.parametrize("cls", ["Real", "Imaginary", "Phase"])
@pytest.mark.parametrize("F", [513, 1025])
def test_part_inverts(dev, F, cls, keep_nyquist):
    g = torch.Generator().manual_seed(_seed(F, cls, keep_nyquist))
    rep = getattr(A, cls)(mode="gaussian", keep_nyquist=keep_nyquist).to(dev)
    X = _spectrum(g, (2, 5, F)).to(dev)
    rep.scale_data(X)
    if cls == "Phase":
        y = _phase_features(rep, g, (2, 5, F), dev)
    else:
        y = rep(X)
        y = (y + NOISE * torch.randn(y.shape, generator=g).to(dev)).contiguous()
    assert y.shape[-1] == F - (0 if keep_nyquist else 1)
    gout = torch.randn(2, 5, F, generator=g).to(dev)
    out, got = _grad_of(rep.invert, y, gout)
    assert out.shape[-1] == F
    off, sc = C.affine_params(rep)
    want = _ref(lambda t: C.ref_affine_invert(t, off, sc, keep_nyquist), y, gout)
    assert rel_max(cpu(got), want.numpy()) < TOL
    # Normalize.invert on its own
    _, gn = _grad_of(rep.norm.invert, y, gout[..., :y.shape[-1]].contiguous())
    assert rel_max(cpu(gn), (gout[..., :y.shape[-1]].cpu().double() * sc).numpy()) < TOL


# ---- the whole chain: representation invert, then the ISTFT adjoint ------------------------------------------------------

def _ref_istft(X64, stage):
    n, h = stage._n_fft, stage._hop
    w = stage.inv_window[:n].detach().cpu().double()
    Xf = X64.reshape(-1, X64.shape[-2], n // 2 + 1)
    return torch.istft(Xf.transpose(-2, -1), n, h, window=w, center=True, onesided=True)


def _chain_audio(g, dev, frames=9, hop=256):
    return (0.1 * torch.randn(2, hop * (frames - 1), generator=g)).to(dev)


def _chain_check(comp, y, ref_spectrum, g, mode=None, seed=None):
    yr = y.detach().clone().requires_grad_()
    if seed is not None:
        torch.manual_seed(seed)
    out = comp.invert(yr, inversion_mode=mode) if mode else comp.invert(yr)
    assert out.grad_fn is not None and out.shape == (2, 256 * 8)
    gy = torch.randn(out.shape, generator=g).to(out.device)
    out.backward(gy)
    y64 = y.detach().cpu().double().requires_grad_()
    ref = _ref_istft(ref_spectrum(y64), comp[0])
    ref.backward(gy.cpu().double().reshape(ref.shape))
    return yr.grad, y64.grad


@pytest.mark.parametrize("cls", ["stft", "dgt"])
def test_chain_polar(dev, cls):
    g = torch.Generator().manual_seed(31)
    stage = (A.STFT if cls == "stft" else A.DGT)(n_fft=1024, hop_length=256)
    comp = (stage + A.Polar()).to(dev)
    x = _chain_audio(g, dev)
    comp.scale_data(x)
    y = comp(x)
    assert y.shape == (2, 9, 2, 513)
    y = (y + NOISE * torch.randn(y.shape, generator=g).to(dev)).contiguous()
    got, want = _chain_check(comp, y, _polar_ref(comp[1]), g)
    got, want = cpu(got), want.numpy()
    assert rel_max(got[..., 0, :], want[..., 0, :]) < TOL and rel_max(got[..., 1, :], want[..., 1, :]) < TOL


@pytest.mark.parametrize("cls", ["stft", "dgt"])
def test_chain_cartesian(dev, cls):
    g = torch.Generator().manual_seed(32)
    comp = ((A.STFT if cls == "stft" else A.DGT)() + A.Cartesian()).to(dev)
    x = _chain_audio(g, dev)
    comp.scale_data(x)
    y = comp(x)
    y = (y + NOISE * torch.randn(y.shape, generator=g).to(dev)).contiguous()
    ra, ia = C.affine_params(comp[1].magnitude), C.affine_params(comp[1].phase)
    got, want = _chain_check(comp, y, lambda t: C.ref_cartesian_invert(t, ra, ia), g)
    assert rel_max(cpu(got), want.numpy()) < TOL


@pytest.mark.parametrize("mode", ["keep_input", "random"])
@pytest.mark.parametrize("cls", ["dgt", "stft"])
def test_chain_magnitude(dev, cls, mode):
    g = torch.Generator().manual_seed(33)
    comp = ((A.STFT if cls == "stft" else A.DGT)() + A.Magnitude(n_mels=128)).to(dev)
    x = _chain_audio(g, dev)
    comp.scale_data(x)
    y = comp(x)                                    # leaves the stage's phase buffer behind (keep_input)
    assert y.shape == (2, 9, 128)
    y = (y + NOISE * torch.randn(y.shape, generator=g).to(dev)).contiguous()
    seed = 9 * 31 + 1024
    if mode == "keep_input":
        phase = comp[0].phase_buffer.detach().clone()
    else:
        torch.manual_seed(seed)
        phase = torch.pi * 2 * torch.rand_like(torch.empty(2, 9, 513, device=dev))
    p = C.magnitude_params(comp[1])
    ph64 = phase.cpu().double().reshape(2, 9, 513)
    got, want = _chain_check(comp, y, lambda t: C.ref_magnitude_invert(t, p) * torch.exp(1j * ph64), g, mode, seed)
    assert rel_max(cpu(got), want.numpy()) < TOL


# ---- unchanged behaviour --------------------------------------------------------------------------------------------------

def _real_loss(out):
    return (torch.view_as_real(out) if out.is_complex() else out).square().sum()


def _unchanged(invert, y):
    """The grad route's values are the plain route's bits; the plain route and everything under no_grad has no graph;
    the backward is first-order only."""
    parts = y if isinstance(y, tuple) else (y,)
    plain = invert(y)
    assert plain.grad_fn is None
    req = tuple(t.detach().clone().requires_grad_() for t in parts)
    routed = invert(req if isinstance(y, tuple) else req[0])
    assert routed.grad_fn is not None and torch.equal(routed.detach(), plain)
    with torch.no_grad():
        quiet = invert(req if isinstance(y, tuple) else req[0])
    assert quiet.grad_fn is None and torch.equal(quiet, plain)
    with pytest.raises(RuntimeError):
        grads = torch.autograd.grad(_real_loss(invert(req if isinstance(y, tuple) else req[0])), req, create_graph=True)
        sum(t.abs().sum() for t in grads).backward()


@pytest.mark.parametrize("kw", [{}, {"n_mels": 128}, {"mel": False}, {"n_mels": 128, "keep_nyquist": False},
                                {"mel": False, "keep_nyquist": False, "mode": None}],
                         ids=["default", "m128", "mel_off", "nonyq", "off_nonyq_nonorm"])
def test_magnitude_invert_unchanged(dev, kw):
    g = torch.Generator().manual_seed(41)
    mod = A.Magnitude(**kw).to(dev)
    _unchanged(mod.invert, _features(mod, _spectrum(g, (2, 5, 513)), g))


@pytest.mark.parametrize("how", ["fused", "stack_none", "mel_off"])
def test_polar_invert_unchanged(dev, how):
    g = torch.Generator().manual_seed(42)
    kw = {"fused": {}, "stack_none": {"stack": None}, "mel_off": {"magnitude_args": {"mode": "bipolar", "mel": False}}}[how]
    rep = A.Polar(**kw).to(dev)
    X = _spectrum(g, (2, 5, 513)).to(dev)
    rep.scale_data(X)
    y = rep(X)
    _unchanged(rep.invert, y)


@pytest.mark.parametrize("stack", [-2, None])
def test_cartesian_invert_unchanged(dev, stack):
    g = torch.Generator().manual_seed(43)
    rep, y = _cartesian_setup(dev, 513, g, stack=stack)
    _unchanged(rep.invert, y)


@pytest.mark.parametrize("keep_nyquist", [True, False])
@pytest.mark.parametrize("cls", ["Real", "Imaginary", "Phase"])
def test_part_inverts_unchanged(dev, cls, keep_nyquist):
    g = torch.Generator().manual_seed(44)
    rep = getattr(A, cls)(mode="gaussian", keep_nyquist=keep_nyquist).to(dev)
    X = _spectrum(g, (2, 5, 513)).to(dev)
    rep.scale_data(X)
    y = rep(X).contiguous()
    _unchanged(rep.invert, y)
    _unchanged(rep.norm.invert, y)


@pytest.mark.parametrize("mode", ["pghi", "griffin_lim", "sinebank"])
def test_magnitude_dependent_phase_modes_keep_no_graph(dev, mode):
    g = torch.Generator().manual_seed(45)
    comp = (A.DGT() + A.Magnitude()).to(dev)
    x = (0.1 * torch.randn(2, 256 * 19, generator=g)).to(dev)
    comp.scale_data(x)
    y = comp(x)
    outs = []
    for req in (False, True):
        torch.manual_seed(11)
        outs.append(comp.invert(y.detach().clone().requires_grad_(req), inversion_mode=mode))
    assert outs[0].grad_fn is None and outs[1].grad_fn is None
    assert torch.equal(outs[0], outs[1])


# ---- robustness -------------------------------------------------------------------------------------------------------------

def _misaligned(t):
    """A contiguous copy of t that starts one element past an aligned buffer: 4 bytes past an 8-byte boundary for
    float32, 8 past a 16-byte boundary for complex64."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape).copy_(t)
    size = t.element_size()
    assert out.is_contiguous() and out.data_ptr() % (2 * size) == size
    return out


def _mag_op(mod, y, gout):
    off, sc = mod._affine()
    return ops.magnitude_invert_backward(y, gout, AG._inverse_bank_tables(mod, y.device), mod.contrast_mode, off, sc,
                                         mod._eps, pad_last=not mod.keep_nyquist)


def test_misaligned_gradients_give_the_aligned_bits(dev):
    g = torch.Generator().manual_seed(51)
    for kw in ({"n_mels": 128}, {"mel": False}, {"n_mels": 128, "keep_nyquist": False}):
        mod = A.Magnitude(**kw).to(dev)
        y = _features(mod, _spectrum(g, (7, 513)), g)
        gout = torch.randn(7, 513, generator=g).to(dev)
        assert torch.equal(_mag_op(mod, _misaligned(y), _misaligned(gout)), _mag_op(mod, y, gout)), kw
    rep, ymag, yph = _polar_setup(dev, 1024, g, shape=(7,))
    y = torch.stack([ymag, yph], -2).contiguous()
    gX = torch.randn(7, 513, dtype=torch.complex64, generator=g).to(dev)
    po, ps = rep.phase._affine(y)
    assert torch.equal(_polar_op(rep.magnitude, _misaligned(y), _misaligned(gX), po, ps),
                       _polar_op(rep.magnitude, y, gX, po, ps))
    mag, ph = torch.rand(7, 513, generator=g).to(dev), (6.283 * torch.rand(7, 513, generator=g)).to(dev)
    a = ops.polar_to_complex_backward(gX, mag, ph)
    b = ops.polar_to_complex_backward(_misaligned(gX), _misaligned(mag), _misaligned(ph))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    only_mag = ops.polar_to_complex_backward(gX, mag, ph, need_phase=False)
    assert only_mag[1] is None and torch.equal(only_mag[0], a[0])
    sc = torch.tensor(1.7, device=dev)
    assert torch.equal(ops.cartesian_inverse_backward(_misaligned(gX), sc, None), ops.cartesian_inverse_backward(gX, sc, None))


@pytest.mark.parametrize("which", ["magnitude", "polar", "cartesian"])
def test_invert_output_inside_cat_after_an_odd_segment(dev, which):
    """autograd hands the backward a slice of the cat's gradient one element past its start."""
    g = torch.Generator().manual_seed(52)
    if which == "magnitude":
        mod = A.Magnitude(n_mels=128).to(dev)
        y = _features(mod, _spectrum(g, (6, 513)), g)
        invert = mod.invert
    elif which == "polar":
        rep, ymag, yph = _polar_setup(dev, 1024, g, shape=(6,))
        y = torch.stack([ymag, yph], -2).unsqueeze(0).contiguous()
        invert = rep.invert
    else:
        rep, y = _cartesian_setup(dev, 513, g)
        invert = rep.invert
    with torch.no_grad():
        out0 = invert(y)
    gflat = torch.randn(out0.numel() + 1, dtype=out0.dtype, generator=g).to(dev)
    glast = torch.randn(out0.shape[:-1] + (out0.shape[-1] + 1,), dtype=out0.dtype, generator=g).to(dev)
    grads = []
    for wrap in ("flat", "plain_flat", "last", "plain_last"):
        yr = y.detach().clone().requires_grad_()
        out = invert(yr)
        if wrap == "flat":
            torch.cat([torch.zeros(1, dtype=out.dtype, device=dev), out.reshape(-1)]).backward(gflat)
        elif wrap == "plain_flat":
            out.backward(gflat[1:].reshape(out.shape).contiguous())
        elif wrap == "last":
            torch.cat([torch.zeros(out.shape[:-1] + (1,), dtype=out.dtype, device=dev), out], -1).backward(glast)
        else:
            out.backward(glast[..., 1:].contiguous())
        grads.append(yr.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[2], grads[3]), which


@pytest.fixture(scope="module")
def many_rows(dev):
    """form -> (module, y, gradient, the batch's result); computed once and left unchanged."""
    made = {}
    g = torch.Generator(device=dev).manual_seed(53)
    for form, (kw, rows) in C.MANY_ROWS.items():
        mod = A.Magnitude(**kw).to(dev)
        F = mod.n_fft // 2 + 1
        X = torch.randn(tuple(rows) + (F,), dtype=torch.complex64, device=dev, generator=g)
        mod.scale_data(X)
        ymag = mod(X)
        ymag = ymag + NOISE * torch.randn(ymag.shape, device=dev, generator=g)
        if form == "real":
            y = ymag.reshape(-1, ymag.shape[-1]).contiguous()
            gout = torch.randn(y.shape[0], F, device=dev, generator=g)
            full = _mag_op(mod, y, gout)
        else:
            yph = (torch.rand(ymag.shape, device=dev, generator=g) * 2 - 1)
            y = torch.stack([ymag, yph], -2).reshape(-1, 2, F).contiguous()
            gout = torch.randn(y.shape[0], F, dtype=torch.complex64, device=dev, generator=g)
            full = _polar_op(mod, y, gout, torch.tensor(0.0, device=dev), torch.tensor(math.pi, device=dev))
        made[form] = (mod, y, gout, full)
    yield made
    made.clear()
    torch.cuda.empty_cache()


def _many_op(form, mod, y, gout):
    if form == "real":
        return _mag_op(mod, y, gout)
    return _polar_op(mod, y, gout, torch.tensor(0.0, device=y.device), torch.tensor(math.pi, device=y.device))


@pytest.mark.parametrize("form", list(C.MANY_ROWS))
def test_many_rows_match_float64_and_a_row_alone_has_the_batch_bits(dev, many_rows, form):
    mod, y, gout, full = many_rows[form]
    R = y.shape[0]
    cls, wpb, lds = C.module_plan(mod, form == "polar")
    trips, _ = C.row_loop_trips(R, wpb, lds, torch.cuda.get_device_properties(0).multi_processor_count)
    assert trips >= 3
    for r in (0, R // 2, R - 1):
        alone = _many_op(form, mod, y[r:r + 1].clone(), gout[r:r + 1].clone())
        assert torch.equal(alone, full[r:r + 1]), (form, r)
    pick = torch.tensor(sorted({0, 1, 2, 3, 4, R // 3, R // 2, R // 2 + 1, R - 5, R - 4, R - 3, R - 2, R - 1}), device=dev)
    p = C.magnitude_params(mod)
    if form == "real":
        want = _ref(lambda t: C.ref_magnitude_invert(t, p), y[pick], gout[pick])
    else:
        want = _ref(lambda t: C.ref_polar_invert(t, p, 0.0, math.pi), y[pick], gout[pick])
    assert rel_max(cpu(full[pick]), want.numpy()) < TOL


@pytest.mark.parametrize("form", list(C.MANY_ROWS))
def test_nan_in_one_row_stays_in_that_row(dev, many_rows, form):
    mod, y, gout, full = many_rows[form]
    R = y.shape[0]
    bad = R // 2 + 3
    y2 = y.clone()
    y2[bad].view(-1)[17] = float("nan")
    got = _many_op(form, mod, y2, gout)
    assert torch.isnan(got[bad]).any()
    keep = torch.ones(R, dtype=torch.bool, device=dev)
    keep[bad] = False
    assert torch.equal(got[keep], full[keep])


def test_nan_through_the_modules_stays_in_its_row(dev):
    g = torch.Generator().manual_seed(54)
    rep, y = _cartesian_setup(dev, 513, g)
    gX = torch.randn(2, 5, 513, dtype=torch.complex64, generator=g).to(dev)
    _, clean = _grad_of(rep.invert, y, gX)
    gX2 = gX.clone()
    gX2[1, 2, 100] = complex(float("nan"), 0.0)
    _, got = _grad_of(rep.invert, y, gX2)
    assert torch.isnan(got[1, 2]).any()
    got[1, 2], clean[1, 2] = 0, 0
    assert torch.equal(got, clean)


@pytest.mark.parametrize("how", ["fused", "stack_none", "mel_off", "nonyq"])
def test_polarif_invert_stays_without_a_graph(dev, how):
    """PolarIF.invert is not differentiable: on its one-pass route and on every part-by-part route it falls back to, an
    input that requires grad gives a tensor without grad_fn, the bits of the no-grad call -- never a gradient for the
    magnitude half alone.  IF.invert on its own likewise."""
    g = torch.Generator().manual_seed(46)
    kw = {"fused": {}, "stack_none": {"stack": None}, "nonyq": {"keep_nyquist": False},
          "mel_off": {"magnitude_args": {"mode": "bipolar", "mel": False}}}[how]
    rep = A.PolarIF(**kw).to(dev)
    X = _spectrum(g, (2, 7, 513)).to(dev)
    rep.scale_data(X)
    y = rep(X)
    parts = y if isinstance(y, tuple) else (y,)
    with torch.no_grad():
        quiet = rep.invert(y)
    plain = rep.invert(y)
    req = tuple(t.detach().clone().requires_grad_() for t in parts)
    routed = rep.invert(req if isinstance(y, tuple) else req[0])
    assert quiet.grad_fn is None and plain.grad_fn is None and routed.grad_fn is None
    assert not routed.requires_grad
    assert torch.equal(routed, quiet) and torch.equal(plain, quiet)
    assert torch.is_grad_enabled()
    yif = (y[1] if isinstance(y, tuple) else y[..., 1, :]).contiguous()
    alone = rep.phase.invert(yif.clone().requires_grad_())
    with torch.no_grad():
        assert alone.grad_fn is None and torch.equal(alone, rep.phase.invert(yif))

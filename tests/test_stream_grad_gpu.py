"""Autograd through the streaming path on the GPU: OverlapAdd, RealtimeSTFT and RealtimeDGT, forward and invert
(stream_grad.hip, autograd.Rt*Function / Oadd*Function).  The reference for every gradient is float64 torch autograd on
the CPU of the reference's own statements (stream_grad_cases.py), built from the modules' buffers with history, tail and
phase as constants; the bound is the project's bound for every other gradient, conftest.rel_max < 1e-5."""
import numpy as np
import pytest
import torch

import stream_grad_cases as C
from conftest import rel_max

import acids_transforms_amd as A
from acids_transforms_amd import ops
from acids_transforms_amd.transforms.channels import MidSide, Mono, Window
from acids_transforms_amd.utils.misc import frame

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _randn(g, *shape, complex_=False):
    return torch.randn(*shape, generator=g, dtype=torch.complex64 if complex_ else torch.float32)


def _off_by_four_bytes(t):
    """A copy of float32 t whose storage starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _close(got, want):
    err = rel_max(got.detach().cpu().numpy(), want.numpy() if isinstance(want, torch.Tensor) else want)
    assert err < TOL, err


# ---- the kernel sweep, through ops -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.SWEEP, ids=C.sweep_id)
def test_frame_analysis_adjoint_sweep(dev, case):
    (N, h), n, S = case["size"], case["n"], case["S"]
    g = _gen(N, h, n, S)
    w = C.hann(N, torch.float32)
    G = _randn(g, S, n, N // 2 + 1, complex_=True)
    got = ops.rfft_frames_backward(G.to(dev), w.to(dev), N)
    assert got.shape == (S, n, N) and got.dtype == torch.float32
    want = C.autograd_of(lambda f: C.ref_analysis(f, w.double()), torch.zeros(S, n, N, dtype=torch.float64),
                         G.to(torch.complex128))
    _close(got, want)
    _close(got, C.np_rfft_frames_backward(G.numpy().astype(np.complex128), w.double().numpy(), N))


@pytest.mark.parametrize("case", C.SYNTH_SWEEP, ids=C.sweep_id)
def test_frame_synthesis_adjoint_sweep(dev, case):
    (N, h), n, S = case["size"], case["n"], case["S"]
    g = _gen(N, h, n, S, 3)
    wd = C.rand_window(N, dtype=torch.float32)
    F = N // 2 + 1
    gf = _randn(g, S, n, N)
    if case["form"] == "complex":
        phase = None
        want = C.autograd_of(lambda X: C.ref_synthesis(X, wd.double(), N), torch.zeros(S, n, F, dtype=torch.complex128),
                             gf.double())
    else:
        phase = 6.283 * torch.rand(S, n, F, generator=g)
        want = C.autograd_of(lambda m: C.ref_synthesis(m * torch.exp(1j * phase.double()), wd.double(), N),
                             torch.ones(S, n, F, dtype=torch.float64), gf.double())
    ph = phase.to(dev) if phase is not None else None
    got = ops.irfft_frames_backward(gf.to(dev), wd.to(dev), N, phase=ph)
    assert got.shape == (S, n, F) and got.dtype == (torch.complex64 if phase is None else torch.float32)
    _close(got, want)
    # a gradient buffer that starts 4 bytes off gives the aligned bits
    assert torch.equal(ops.irfft_frames_backward(_off_by_four_bytes(gf.to(dev)), wd.to(dev), N, phase=ph), got)


@pytest.mark.parametrize("case", C.SWEEP, ids=C.sweep_id)
def test_overlap_add_adjoints_sweep(dev, case):
    (N, h), n, S = case["size"], case["n"], case["S"]
    keep = C.keep_of(N, h)
    g = _gen(N, h, n, S, 5)
    out_len = (n - 1) * h + N - keep
    gain = torch.tensor(1.5)
    for Cn in (out_len, out_len + 3 * h // 4):       # exactly covered; a tail no frame covers
        gf = _randn(g, S, n, N)
        got = ops.oadd_forward_backward(gf.to(dev), N, h, keep, Cn)
        _close(got, C.np_oadd_forward_backward(gf.double().numpy(), N, h, keep, Cn))
        assert torch.equal(got[:, out_len:], torch.zeros_like(got[:, out_len:]))
        assert torch.equal(ops.oadd_forward_backward(_off_by_four_bytes(gf.to(dev)), N, h, keep, Cn), got)
    gy = _randn(g, S, out_len)
    got = ops.oadd_invert_backward(gy.to(dev), n, N, h, keep, gain.to(dev))
    want = C.np_oadd_invert_backward(gy.double().numpy(), n, N, h, keep, 1.5)
    _close(got, want)
    assert torch.equal(got.cpu() == 0, torch.from_numpy(want == 0))       # exactly 0 past out_len, nowhere else
    assert torch.equal(ops.oadd_invert_backward(_off_by_four_bytes(gy.to(dev)), n, N, h, keep, gain.to(dev)), got)


def test_ops_refuse_float64(dev):
    w = C.hann(128, torch.float32).to(dev)
    with pytest.raises(ops.AcidsHipError):
        ops.rfft_frames_backward(torch.zeros(2, 65, dtype=torch.complex128, device=dev), w, 128)
    with pytest.raises(ops.AcidsHipError):
        ops.irfft_frames_backward(torch.zeros(2, 128, dtype=torch.float64, device=dev), w, 128)
    with pytest.raises(ops.AcidsHipError):
        ops.oadd_forward_backward(torch.zeros(1, 2, 128, dtype=torch.float64, device=dev), 128, 32, 96, 64)
    with pytest.raises(ops.AcidsHipError):
        ops.oadd_invert_backward(torch.zeros(1, 64, dtype=torch.float64, device=dev), 2, 128, 32, 96, w[:1])
    # a strided gradient is made contiguous
    gf = torch.randn(3, 128, 2, device=dev).transpose(-1, -2)
    assert torch.equal(ops.oadd_forward_backward(gf, 128, 32, 96, 64), ops.oadd_forward_backward(gf.contiguous(), 128, 32, 96, 64))


# ---- OverlapAdd ---------------------------------------------------------------------------------------------------------------

def _twin(N, h, like, dev):
    """An OverlapAdd with the state of `like`."""
    m = A.OverlapAdd(N, h).to(dev)
    m.input_buffer, m.output_buffer = like.input_buffer.clone(), like.output_buffer.clone()
    return m


def _state64(buf, lead, keep):
    return buf.detach().double().cpu() if buf.shape[:-1] == lead else torch.zeros(lead + (keep,), dtype=torch.float64)


@pytest.mark.parametrize("N,h", C.SIZES)
def test_overlap_add_forward_gradient(dev, N, h):
    keep, lead = C.keep_of(N, h), torch.Size((2, 3))
    for Cn in C.chunk_lengths(N, h):
        g = _gen(N, h, Cn)
        oadd = A.OverlapAdd(N, h).to(dev)
        for call in range(2):              # zero history, then carried history
            hist = _state64(oadd.input_buffer, lead, keep)
            plain = _twin(N, h, oadd, dev)(_randn(_gen(N, h, Cn, call), 2, 3, Cn).to(dev))
            x = _randn(_gen(N, h, Cn, call), 2, 3, Cn)
            xg = x.to(dev).requires_grad_()
            frames = oadd(xg)
            assert plain.grad_fn is None and frames.grad_fn is not None and torch.equal(frames.detach(), plain)
            assert frames.stride() == plain.stride()                       # the same zero-copy view
            assert not oadd.input_buffer.requires_grad and oadd.input_buffer.grad_fn is None
            gf = _randn(g, *frames.shape)
            frames.backward(gf.to(dev))
            want = C.autograd_of(lambda x_: C.ref_frames(x_, hist, N, h), x.double(), gf.double())
            _close(xg.grad, want)
            if (N, h, Cn) == (1024, 256, 1000):
                assert frames.shape[-2] == 3 and torch.equal(xg.grad[..., 768:], torch.zeros(2, 3, 232, device=dev))
        assert call == 1 and hist.abs().max() > 0                          # the second call did carry a history


@pytest.mark.parametrize("N,h", C.SIZES)
def test_overlap_add_invert_gradient(dev, N, h):
    keep, lead = C.keep_of(N, h), torch.Size((2, 3))
    for n in (1, 3, N // h + 2):
        g = _gen(N, h, n, 9)
        oadd = A.OverlapAdd(N, h).to(dev)
        gain = float(oadd.gain_compensation)
        out_len = (n - 1) * h + N - keep
        for call in range(2):              # zero tail, then carried tail
            tail = _state64(oadd.output_buffer, lead, keep)
            f = _randn(g, 2, 3, n, N)
            plain = _twin(N, h, oadd, dev).invert(f.to(dev))
            fg = f.to(dev).requires_grad_()
            out = oadd.invert(fg)
            assert plain.grad_fn is None and out.grad_fn is not None and torch.equal(out.detach(), plain)
            assert not oadd.output_buffer.requires_grad and oadd.output_buffer.grad_fn is None
            gy = _randn(g, *out.shape)
            out.backward(gy.to(dev))
            want = C.autograd_of(lambda f_: C.ref_oadd_invert(f_, tail, N, h, gain)[0], f.double(), gy.double())
            _close(fg.grad, want)
            # what only reaches the new tail gets exactly 0
            pos = torch.arange(n).unsqueeze(1) * h + torch.arange(N).unsqueeze(0)
            dead = (pos >= out_len).to(dev)
            assert dead.any() and torch.equal(fg.grad[..., dead], torch.zeros_like(fg.grad[..., dead]))
        assert tail.abs().max() > 0


def test_overlap_add_policy(dev):
    N, h = 128, 32
    oadd = A.OverlapAdd(N, h).to(dev)
    x = torch.randn(2, 256, device=dev)
    with torch.no_grad():
        assert oadd(x.clone().requires_grad_()).grad_fn is None
        assert oadd.invert(torch.randn(2, 3, N, device=dev).requires_grad_()).grad_fn is None
    with pytest.raises(RuntimeError):
        xx = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad(oadd(xx).square().sum(), xx, create_graph=True)
        gx.sum().backward()
    with pytest.raises(RuntimeError):
        ff = torch.randn(2, 3, N, device=dev).requires_grad_()
        (gf,) = torch.autograd.grad(oadd.invert(ff).square().sum(), ff, create_graph=True)
        gf.sum().backward()
    # _invert_without_update stays without a graph
    assert oadd._invert_without_update(torch.randn(2, 3, N, device=dev).requires_grad_()).grad_fn is None
    # a change of batch shape resets the state, as on the plain route
    oadd(torch.randn(2, 256, device=dev).requires_grad_())
    a = oadd(torch.zeros(5, 256, device=dev).requires_grad_())
    assert torch.equal(a[:, 0, :C.keep_of(N, h)], torch.zeros(5, C.keep_of(N, h), device=dev))


# ---- RealtimeSTFT / RealtimeDGT ----------------------------------------------------------------------------------------------

MODULES = [("stft", 1024, 256), ("dgt", 1024, 256), ("stft", 512, 128), ("dgt", 128, 32), ("stft", 405, 135)]


def _make(kind, N, h, dev, mode=None, seed=0):
    torch.manual_seed(seed)
    if kind == "stft":
        m = A.RealtimeSTFT(n_fft=N, hop_length=h, inversion_mode=mode or "random")
    else:
        m = A.RealtimeDGT(n_fft=N, hop_length=h, inversion_mode=mode or "pghi")
    return m.to(dev)


def _second_order_raises(fn, x):
    with pytest.raises(RuntimeError):
        xx = x.detach().clone().requires_grad_()
        (gx,) = torch.autograd.grad(fn(xx).abs().square().sum(), xx, create_graph=True)
        gx.abs().sum().backward()


@pytest.mark.parametrize("kind,N,h", MODULES)
def test_realtime_forward_gradient(dev, kind, N, h):
    g = _gen(N, h, 1)
    m = _make(kind, N, h, dev)
    w = m.window[:N].double().cpu()
    x = _randn(g, 2, 3, N)
    plain = m(x.to(dev))
    xg = x.to(dev).requires_grad_()
    X = m(xg)
    assert plain.grad_fn is None and X.grad_fn is not None and torch.equal(X.detach(), plain)
    assert not m.phase_buffer.requires_grad
    with torch.no_grad():
        assert m(x.to(dev).requires_grad_()).grad_fn is None
    G = _randn(g, *X.shape, complex_=True)
    X.backward(G.to(dev))
    want = C.autograd_of(lambda f: C.ref_analysis(f, w), x.double(), G.to(torch.complex128))
    _close(xg.grad, want)
    _second_order_raises(m, x.to(dev))
    # a single frame (..., n_fft)
    x1 = x[0, 0].clone().to(dev).requires_grad_()
    X1 = m(x1)
    X1.backward(G[0, 0].to(dev))
    assert torch.equal(X1.detach(), m(x[0, 0].to(dev)))
    _close(x1.grad, want[0, 0])


@pytest.mark.parametrize("kind,N,h", MODULES)
def test_realtime_invert_gradient(dev, kind, N, h):
    g = _gen(N, h, 2)
    m = _make(kind, N, h, dev)
    wd = m.inv_window[:N].double().cpu()
    F = N // 2 + 1
    X = _randn(g, 2, 3, F, complex_=True)
    plain = m.invert(X.to(dev))
    Xg = X.to(dev).requires_grad_()
    f = m.invert(Xg)
    assert plain.grad_fn is None and f.grad_fn is not None and torch.equal(f.detach(), plain)
    with torch.no_grad():
        assert m.invert(X.to(dev).requires_grad_()).grad_fn is None
    gf = _randn(g, *f.shape)
    f.backward(gf.to(dev))
    want = C.autograd_of(lambda X_: C.ref_synthesis(X_, wd, N), X.to(torch.complex128), gf.double())
    _close(Xg.grad, want)
    _second_order_raises(m.invert, X.to(dev))


@pytest.mark.parametrize("mode", ["keep_input", "random"])
@pytest.mark.parametrize("kind,N,h", MODULES)
def test_realtime_invert_of_a_magnitude_gradient(dev, kind, N, h, mode):
    g = _gen(N, h, 3)
    F = N // 2 + 1
    x = _randn(g, 2, 3, N)
    mag = torch.rand(2, 3, F, generator=g) + 0.1

    def run(requires_grad):
        m = _make(kind, N, h, dev, mode)
        m(x.to(dev))                                   # fills the phase buffer (keep_input)
        torch.manual_seed(11)
        inp = mag.to(dev).requires_grad_(requires_grad)
        return m, inp, m.invert(inp)

    m_plain, _, plain = run(False)
    m, mg, f = run(True)
    assert plain.grad_fn is None and f.grad_fn is not None and torch.equal(f.detach(), plain)
    for name in ("phase_buffer", "random_phase") + (("hgi_mag_buffer", "hgi_phase_buffer") if kind == "dgt" else ()):
        assert not getattr(m, name).requires_grad and getattr(m, name).grad_fn is None, name
    if kind == "dgt":       # the fused op refreshed the PGHI history as on the plain route
        assert torch.equal(m.hgi_mag_buffer, m_plain.hgi_mag_buffer) and m.hgi_mag_buffer.abs().max() > 0
        assert torch.equal(m.hgi_phase_buffer, m_plain.hgi_phase_buffer)
    if mode == "keep_input":
        phase = m.phase_buffer.double().cpu()
    else:
        torch.manual_seed(11)
        phase = (torch.pi * 2 * torch.rand_like(mag.to(dev))).double().cpu()
    wd = m.inv_window[:N].double().cpu()
    gf = _randn(g, *f.shape)
    f.backward(gf.to(dev))
    want = C.autograd_of(lambda a: C.ref_synthesis(a * torch.exp(1j * phase), wd, N), mag.double(), gf.double())
    _close(mg.grad, want)
    with torch.no_grad():
        assert run(True)[2].grad_fn is None
    _second_order_raises(lambda a: m.invert(a, inversion_mode=mode), mag.to(dev))


@pytest.mark.parametrize("kind,mode", [("stft", "sinebank"), ("dgt", "sinebank"), ("dgt", "pghi")])
def test_magnitude_dependent_modes_stay_without_a_graph(dev, kind, mode):
    N, h = 128, 32
    mag = torch.rand(2, 3, N // 2 + 1, generator=_gen(4)) + 0.1
    outs = []
    for requires_grad in (False, True):
        m = _make(kind, N, h, dev, mode, seed=5)
        torch.manual_seed(7)
        outs.append(m.invert(mag.to(dev).requires_grad_(requires_grad)))
    assert outs[0].grad_fn is None and outs[1].grad_fn is None and torch.equal(outs[0], outs[1])


# ---- chains --------------------------------------------------------------------------------------------------------------------

def test_chain_overlap_add_into_realtime_dgt(dev):
    N, h, keep = 1024, 256, 768
    g = _gen(21)
    oadd, dgt = A.OverlapAdd(N, h).to(dev), _make("dgt", N, h, dev)
    w = dgt.window[:N].double().cpu()
    oadd(_randn(g, 2, 1024).to(dev))                     # a carried history
    hist = oadd.input_buffer.double().cpu()
    x = _randn(g, 2, 1280)
    xg = x.to(dev).requires_grad_()
    X = dgt(oadd(xg))
    G = _randn(g, *X.shape, complex_=True)
    X.backward(G.to(dev))
    want = C.autograd_of(lambda x_: C.ref_analysis(C.ref_frames(x_, hist, N, h), w), x.double(), G.to(torch.complex128))
    _close(xg.grad, want)


@pytest.mark.parametrize("source", ["complex", "keep_input"])
def test_chain_realtime_dgt_invert_into_overlap_add(dev, source):
    N, h, keep, F = 1024, 256, 768, 513
    g = _gen(22)
    oadd, dgt = A.OverlapAdd(N, h).to(dev), _make("dgt", N, h, dev, "keep_input")
    wd = dgt.inv_window[:N].double().cpu()
    gain = float(oadd.gain_compensation)
    oadd.invert(_randn(g, 2, 4, N).to(dev))              # a carried tail
    tail = oadd.output_buffer.double().cpu()
    if source == "complex":
        inp = _randn(g, 2, 5, F, complex_=True)
        synth = lambda v: C.ref_synthesis(v, wd, N)       # noqa: E731
    else:
        dgt(_randn(g, 2, 5, N).to(dev))
        phase = dgt.phase_buffer.double().cpu()
        inp = torch.rand(2, 5, F, generator=g) + 0.1
        synth = lambda v: C.ref_synthesis(v * torch.exp(1j * phase), wd, N)       # noqa: E731
    ig = inp.to(dev).requires_grad_()
    y = oadd.invert(dgt.invert(ig))
    gy = _randn(g, *y.shape)
    y.backward(gy.to(dev))
    want = C.autograd_of(lambda v: C.ref_oadd_invert(synth(v), tail, N, h, gain)[0],
                         inp.double() if source != "complex" else inp.to(torch.complex128), gy.double())
    _close(ig.grad, want)


def test_round_trip_over_two_chunks(dev):
    """x -> frames -> X -> frames -> y, chunk by chunk.  Each chunk's gradient is the reference's with that chunk's carried
    state as constants; the second chunk's backward does not touch the first chunk's graph (which is freed by then)."""
    N, h, keep = 512, 128, 384
    g = _gen(23)
    oin, oout, dgt = A.OverlapAdd(N, h).to(dev), A.OverlapAdd(N, h).to(dev), _make("dgt", N, h, dev)
    w, wd = dgt.window[:N].double().cpu(), dgt.inv_window[:N].double().cpu()
    gain = float(oout.gain_compensation)
    for chunk in range(2):
        hist = _state64(oin.input_buffer, torch.Size((2,)), keep)
        tail = _state64(oout.output_buffer, torch.Size((2,)), keep)
        x = _randn(g, 2, 1024)
        xg = x.to(dev).requires_grad_()
        y = oout.invert(dgt.invert(dgt(oin(xg))))
        gy = _randn(g, *y.shape)
        y.backward(gy.to(dev))               # raises on the second chunk if the state were graph-attached
        want = C.autograd_of(lambda x_: C.ref_oadd_invert(C.ref_synthesis(C.ref_analysis(
            C.ref_frames(x_, hist, N, h), w), wd, N), tail, N, h, gain)[0], x.double(), gy.double())
        _close(xg.grad, want)
    assert hist.abs().max() > 0 and tail.abs().max() > 0


def test_frames_built_by_frame_of_a_tensor_that_requires_grad(dev):
    N, h = 512, 128
    g = _gen(24)
    dgt = _make("dgt", N, h, dev)
    w = dgt.window[:N].double().cpu()
    x = _randn(g, 2, 2048)
    plain = dgt(frame(x.to(dev), N, h, -1))
    xg = x.to(dev).requires_grad_()
    X = dgt(frame(xg, N, h, -1))             # an overlapping view: torch's as_strided backward folds our dense gradient
    assert torch.equal(X.detach(), plain)
    G = _randn(g, *X.shape, complex_=True)
    X.backward(G.to(dev))
    nw = X.shape[-2]
    want = C.autograd_of(lambda x_: C.ref_analysis(torch.nn.functional.pad(x_, (0, nw * h + N - 2048)).unfold(-1, N, h)[
        ..., :nw, :], w), x.double(), G.to(torch.complex128))
    _close(xg.grad, want)


# ---- isolation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [128, 512, 1024])
def test_a_stream_alone_gives_the_batch_bits(dev, N):
    g = _gen(N, 31)
    n, S, F = 3, 3, N // 2 + 1              # 3 frames: the shared transforms end inside a stream
    w = C.hann(N, torch.float32).to(dev)
    G = _randn(g, S, n, F, complex_=True).to(dev)
    gf = _randn(g, S, n, N).to(dev)
    phase = (6.283 * torch.rand(S, n, F, generator=g)).to(dev)
    batch = [ops.rfft_frames_backward(G, w, N), ops.irfft_frames_backward(gf, w, N),
             ops.irfft_frames_backward(gf, w, N, phase=phase)]
    for s in range(S):
        alone = [ops.rfft_frames_backward(G[s:s + 1], w, N), ops.irfft_frames_backward(gf[s:s + 1], w, N),
                 ops.irfft_frames_backward(gf[s:s + 1], w, N, phase=phase[s:s + 1])]
        for a, b in zip(alone, batch):
            assert torch.equal(a, b[s:s + 1]), (N, s)


@pytest.mark.parametrize("N", [128, 512, 1024])
def test_a_nan_stays_in_its_stream(dev, N):
    g = _gen(N, 32)
    n, S, F, h = 3, 3, N // 2 + 1, N // 4
    keep = C.keep_of(N, h)
    w = C.hann(N, torch.float32).to(dev)
    G = _randn(g, S, n, F, complex_=True)
    G[1, 1, 5] = float("nan")
    gf = _randn(g, S, n, N)
    gf[1, 0, keep + 7] = float("nan")             # a position that reaches the chunk, not only the history
    gy = _randn(g, S, (n - 1) * h + N - keep)
    gy[1, 3] = float("nan")
    outs = [ops.rfft_frames_backward(G.to(dev), w, N), ops.irfft_frames_backward(gf.to(dev), w, N),
            ops.irfft_frames_backward(gf.to(dev), w, N, phase=torch.zeros(S, n, F, device=dev)),
            ops.oadd_forward_backward(gf.to(dev), N, h, keep, n * h),
            ops.oadd_invert_backward(gy.to(dev), n, N, h, keep, w[N // 2:N // 2 + 1])]
    for o in outs:
        bad = torch.isnan(torch.view_as_real(o) if o.is_complex() else o).reshape(S, -1).any(-1)
        assert bad.tolist() == [False, True, False]


# ---- the channel stages are torch expressions: a small pin ----------------------------------------------------------------

def test_channel_stages_carry_a_gradient(dev):
    g = _gen(41)
    x = _randn(g, 3, 2, 64)
    stages = [(Mono("mix"), lambda v: (v.sum(-2) / 2)),
              (MidSide(), lambda v: torch.stack([(v[..., 0, :] + v[..., 1, :]) / 2 / 2 ** 0.5,
                                                 (v[..., 0, :] - v[..., 1, :]) / 2], -2)),
              (Window(window_size=32, hop_size=8), lambda v: v.unfold(-1, 32, 8))]
    for stage, expr in stages:
        xg = x.to(dev).requires_grad_()
        y = stage(xg)
        ref = expr(x.double())
        assert y.grad_fn is not None and y.shape == ref.shape, stage
        gy = torch.randn(*y.shape, generator=g)
        y.backward(gy.to(dev))
        _close(xg.grad, C.autograd_of(expr, x.double(), gy.double()))

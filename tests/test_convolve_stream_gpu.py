"""GPU side of the streaming partitioned convolution (ops.spectral_fir_stream / fft_convolve_stream,
autograd.ImpulseResponseStreamFunction, transforms.RealtimeImpulseResponse, at_spectral_fir_stream of
csrc/fft_convolve.hip): the new kernel against the offline kernel on the linearised history, to the bit; the stream against
numpy.convolve within the library's normwise bound 1e-5; chunkings, batches, resets and reloaded states against each other,
to the bit; what a NaN and zeros must and must not do; the gradients of a chunk against float64 conv1d autograd with the
carried history a constant.

Measured on an MI355X (worst figures, printed by the tests): see README, "RealtimeImpulseResponse"."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import convolve_stream_cases as S
import fft_convolve_cases as C
from acids_transforms_amd import ops

pytestmark = pytest.mark.gpu
TOL = S.TOL


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b)


def _run(m, x, B, chunks):
    """The chunks of x (..., L), in blocks of B, through module m -> the concatenated outputs."""
    out, a = [], 0
    for n in chunks:
        out.append(m(x[..., a:a + n * B]))
        a += n * B
    assert a == x.shape[-1]
    return torch.cat(out, dim=-1)


def _module(h, B, dev, **kw):
    return A.RealtimeImpulseResponse(torch.from_numpy(np.asarray(h)), block=B, **kw).to(dev)


# ---- 1. the kernel against the offline kernel, to the bit ---------------------------------------------------------------------
@pytest.mark.parametrize("F", (129, 257))
@pytest.mark.parametrize("rows", (1, 3, 9000))
def test_stream_kernel_has_the_bits_of_the_offline_kernel(dev, rows, F):
    """P x Tc x head on planted finite spectra: Y equals at_spectral_fir on [the ring in order | Xc] past its first P - 1
    frames, and the ring afterwards equals the expected ring, untouched slots included.  F = 257: a second bin chunk with one
    live lane; 9000 rows: more items than the 8192 persistent workgroups."""
    g = torch.Generator(device=dev).manual_seed(rows * 1000 + F)
    planted = lambda *s: torch.view_as_complex(torch.randn(*s, 2, generator=g, device=dev))
    ring_pool, x_pool, h_pool = planted(rows, 24, F), planted(rows, 8, F), planted(17, F)
    for P in (1, 2, 8, 9, 12, 17):
        B_, P_, R, n = ops.fft_convolve_stream_plan(P * 128, 128)
        assert (P_, R, n) == (P, P + 7, 8)
        H = h_pool[:P].contiguous()
        for Tc in (1, 3, 8):
            Xc = x_pool[:, :Tc].contiguous()
            for head in (0, R - Tc, R - 1):                                      # R - 1: a wrap inside the chunk's own writes
                ring = ring_pool[:, :R].clone()
                order = [(head - (P - 1) + i) % R for i in range(P - 1)]
                hist = ring[:, order]
                want = ops.spectral_fir(torch.cat([hist, Xc], dim=1), H)[:, P - 1:]
                after = ring.clone()
                for t in range(Tc):
                    after[:, (head + t) % R] = Xc[:, t]
                Y = ops.spectral_fir_stream(Xc, ring, head, H)
                assert Y.shape == (rows, Tc, F) and Y.dtype == torch.complex64
                assert _bits(Y, want), (P, Tc, head)
                assert _bits(ring, after), (P, Tc, head)


def test_stream_kernel_strided_frames_nothing_to_do_and_errors(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    planted = lambda *s: torch.view_as_complex(torch.randn(*s, 2, generator=g, device=dev))
    rows, P, R, F = 3, 3, 10, 129
    ring0, wide, H = planted(rows, R, F), planted(rows, 6, F), planted(P, F)
    ring_a, ring_b = ring0.clone(), ring0.clone()
    ya = ops.spectral_fir_stream(wide[:, :5], ring_a, 4, H)                      # frames of a longer buffer: the row stride is not Tc F
    yb = ops.spectral_fir_stream(wide[:, :5].contiguous(), ring_b, 4, H)
    assert _bits(ya, yb) and _bits(ring_a, ring_b) and not _bits(ring_a, ring0)
    ring = ring0.clone()                                                         # Tc = 0 and rows = 0: the ring stays
    assert ops.spectral_fir_stream(wide[:, :0], ring, 4, H).shape == (rows, 0, F) and _bits(ring, ring0)
    assert ops.spectral_fir_stream(wide[:0, :5], ring[:0], 4, H).shape == (0, 5, F) and _bits(ring, ring0)
    for Xc, rg, head, Hh in ((planted(rows, 9, F), planted(rows, 16, F), 0, H),           # Tc > 8
                             (wide[:, :5], ring0[:, :6].contiguous(), 0, H),              # R < P - 1 + Tc
                             (wide[:, :5], ring, -1, H), (wide[:, :5], ring, R, H),       # head outside [0, R)
                             (wide[:, :5], ring, 0, H[:0])):                              # P < 1
        with pytest.raises(A.AcidsHipError):
            ops.spectral_fir_stream(Xc, rg, head, Hh)
    assert _bits(ring, ring0)


# ---- 2. - 4. parity, chunkings, the offline module, rows ----------------------------------------------------------------------
@pytest.mark.parametrize("K", S.TAPS)
def test_stream_matches_numpy_convolve_every_chunking_and_the_offline_module_to_the_bit(dev, K):
    """Block 128, a stream of 40 blocks.  Every chunking and every leading shape: within 1e-5 of numpy.convolve(x, h)[:L];
    the three chunkings give the same bits, and those of fftconvolve(x, ir, "full", block=128)[..., :L]; row 0 alone has the
    bits it has in the batches of 3, 6 and 70."""
    B, L = S.BLOCK, S.LENGTH
    x, h, _ = S.data(K)
    ref = S.reference(K)
    m = _module(h, B, dev)
    worst, alone = 0.0, None
    for lead in S.LEADS:
        xd = _dev(C.take(x, lead), dev)
        offline = A.fftconvolve(xd, m.ir, "full", block=B)[..., :L]
        for chunks in S.CHUNKINGS:
            y = _run(m, xd, B, chunks)                                           # a new leading shape starts from zeros
            m.reset()
            assert y.shape == tuple(lead) + (L,) and y.dtype == torch.float32
            worst = max(worst, C.rel_max(_np(y), C.take(ref, lead)))
            assert torch.equal(y, offline), (K, lead, chunks[:6])
            first = y.reshape(-1, L)[0]
            alone = first if alone is None else alone
            assert torch.equal(first, alone), (K, lead)
    print("stream block %d K %d: %.2e" % (B, K, worst))
    assert worst < TOL


@pytest.mark.parametrize("B,K,rows", S.BLOCK_CASES)
def test_the_other_blocks_of_the_ladder(dev, B, K, rows):
    """Blocks 256 .. 2048, a stream of 6 blocks as chunks of (1, 3, 2), then as 6 x 1 and as one chunk: parity, and the bits of
    each other and of the offline module."""
    n = sum(S.BLOCK_CHUNKS)
    x, h, _ = S.data(K, B, n, rows)
    xd = _dev(x, dev)
    m = _module(h, B, dev)
    assert m.block == B
    offline = A.fftconvolve(xd, m.ir, "full", block=B)[..., :n * B]
    runs = []
    for chunks in (S.BLOCK_CHUNKS, (1,) * n, (n,)):
        runs.append(_run(m, xd, B, chunks))
        m.reset()
    err = max(C.rel_max(_np(y), S.reference(K, B, n, rows)) for y in runs)
    between = max(C.rel_max(_np(y), _np(offline)) for y in runs)
    print("stream block %d K %d: %.2e against numpy.convolve, %.2e against the offline module, bit-equal %s"
          % (B, K, err, between, [bool(torch.equal(y, offline)) for y in runs]))
    assert err < TOL
    for y in runs:
        assert torch.equal(y, offline)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def test_reset_state_dict_and_a_new_leading_shape(dev):
    B, K = S.BLOCK, 1000
    x, h, _ = S.data(K)
    xd = _dev(x[:6], dev)
    chunks = S.CHUNKINGS[2]
    m = _module(h, B, dev)
    first = _run(m, xd, B, chunks)
    assert m.head == S.STREAM_BLOCKS % m.ring_slots and m.input_buffer.shape == (6, B)
    assert torch.equal(m.input_buffer, xd[:, -B:]) and not m.input_buffer.requires_grad
    m.reset()
    assert m.head == 0 and not m.input_buffer.any()
    assert torch.equal(_run(m, xd, B, chunks), first)                            # reset, the same chunks: the same bits
    # a state_dict saved mid-stream, loaded into a fresh module, continues to the bit
    m.reset()
    cut = sum(chunks[:3]) * B
    head_of = _run(m, xd[:, :cut], B, chunks[:3])
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else dict(v)) for k, v in m.state_dict().items()}
    assert sd["_extra_state"] == {"head": sum(chunks[:3]) % m.ring_slots}
    fresh = _module(np.zeros(K, dtype=np.float32), B, dev)
    fresh.load_state_dict(sd)
    rest = _run(fresh, xd[:, cut:], B, chunks[3:])
    assert torch.equal(torch.cat([head_of, rest], dim=-1), first)
    # a new leading shape starts from zeros: the stream of rows 0 .. 2 from its beginning
    y3 = _run(fresh, xd[:3], B, chunks)
    assert fresh.input_buffer.shape == (3, B) and fresh.spectrum_ring.shape == (3, fresh.ring_slots, B + 1)
    assert torch.equal(y3, first[:3])
    y23 = fresh(xd.reshape(2, 3, -1)[..., :B])
    assert fresh.input_buffer.shape == (2, 3, B) and fresh.head == 1 and torch.equal(y23.reshape(6, B), first[:, :B])


# ---- 6. NaN and zeros -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 130, 1000))
def test_a_nan_stays_in_its_row_and_leaves_with_its_frames(dev, n):
    """Block 128, K = 300 (P = 3), a NaN at sample n of row 1 of 3.  The frames n // B and n // B + 1 hold it, so blocks n // B ..
    n // B + P may; every block before and from n // B + P + 1 on has the clean bits, though ring slots may still hold the
    NaN -- a read of a stale slot would show here."""
    B, K, P = S.BLOCK, 300, 3
    x, h, _ = S.data(K)
    xd = _dev(x[:3], dev)
    bad = xd.clone()
    bad[1, n] = float("nan")
    t0 = n // B
    for chunks in S.CHUNKINGS:
        m = _module(h, B, dev)
        clean = _run(m, xd, B, chunks)
        m.reset()
        y = _run(m, bad, B, chunks)
        assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2])
        assert bool(torch.isnan(y[1, n:n + K]).all())                            # never lost where it belongs
        assert torch.equal(y[1, :t0 * B], clean[1, :t0 * B])
        assert torch.equal(y[1, (t0 + P + 1) * B:], clean[1, (t0 + P + 1) * B:])


def test_zeros_give_plus_zero(dev):
    B = S.BLOCK
    x, h, _ = S.data(1000)
    m = _module(h, B, dev)
    y = _run(m, torch.zeros(3, S.LENGTH, device=dev), B, S.CHUNKINGS[2])
    assert not y.any() and not torch.signbit(y).any()
    z = _module(np.zeros(1000, dtype=np.float32), B, dev)
    y = _run(z, _dev(x[:3], dev), B, S.CHUNKINGS[2])
    assert not y.any() and not torch.signbit(y).any()


# ---- 7. gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (129, 1000, 1100))
def test_chunk_gradients_match_float64_conv1d_autograd(dev, K):
    """gx of every chunk and gh summed over the chunks of one stream, at every chunking, against conv1d autograd in float64
    with the samples before the chunk a constant; every chunk has a graph of its own (no retain_graph); the forward of the
    grad route has the bits of the plain route."""
    B, rows = S.BLOCK, 3
    x, h, g = S.data(K)
    x, g = x[:rows], g[:rows]
    plain_m = _module(h, B, dev)
    worst = dict(gx=0.0, gh=0.0, gh_chunk=0.0)
    for chunks in S.CHUNKINGS:
        rx, rh, rhs = S.chunk_gradients(x, h, g, B, chunks)
        m = _module(h, B, dev, learnable=True)
        plain = _run(plain_m, _dev(x, dev), B, chunks)
        plain_m.reset()
        a, gxs, ys = 0, [], []
        for i, n in enumerate(chunks):
            xc = _dev(x[:, a:a + n * B], dev).requires_grad_()
            y = m(xc)
            assert y.grad_fn is not None and not m.input_buffer.requires_grad and not m.spectrum_ring.requires_grad
            before = None if m.ir.grad is None else m.ir.grad.clone()
            y.backward(_dev(g[:, a:a + n * B], dev))
            gxs.append(xc.grad)
            ys.append(y.detach())
            step = m.ir.grad if before is None else m.ir.grad - before
            if i in (0, 1, len(chunks) - 1):
                worst["gh_chunk"] = max(worst["gh_chunk"], C.rel_max(_np(step), rhs[i]))
            a += n * B
        assert torch.equal(torch.cat(ys, dim=-1), plain)
        worst["gx"] = max(worst["gx"], C.rel_max(_np(torch.cat(gxs, dim=-1)), rx))
        worst["gh"] = max(worst["gh"], C.rel_max(_np(m.ir.grad), rh))
    print("stream gradients K %d: %s" % (K, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL, worst


def test_only_the_gradients_that_are_needed_and_first_order_only(dev):
    B, K = S.BLOCK, 300
    x, h, g = S.data(K)
    xd, gd = _dev(x[:3, :4 * B], dev), _dev(g[:3, :4 * B], dev)
    frozen, learn = _module(h, B, dev), _module(h, B, dev, learnable=True)
    plain = frozen(xd)
    assert plain.grad_fn is None
    frozen.reset()
    xr = xd.clone().requires_grad_()
    y = frozen(xr)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    y.backward(gd)
    assert xr.grad is not None and frozen.ir.grad is None
    y = learn(xd)                                                                # the response alone requires grad
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    y.backward(gd)
    assert learn.ir.grad is not None and learn.ir.grad.shape == (K,) and bool(learn.ir.grad.abs().sum() > 0)
    with torch.no_grad():
        assert learn(xr).grad_fn is None
    y = learn(xr)
    (gx,) = torch.autograd.grad(y, xr, gd, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


@pytest.mark.parametrize("K", (129, 1000, 1100))
def test_adjoint_identity_per_chunk(dev, K):
    """<A x, g> = <x, A^T g> for every chunk, A the chunk's map with the carried state set to zero (the state's part of the
    output is a constant and has no gradient), accumulated in float64 from the fp32 results: within 1e-6 of sum |A x| |g|."""
    B = S.BLOCK
    x, h, g = S.data(K)
    for n in (1, 3, 8, 16):
        xd, gd = _dev(x[:3, :n * B], dev).requires_grad_(), _dev(g[:3, :n * B], dev)
        m = _module(h, B, dev)
        y = m(xd)
        y.backward(gd)
        lhs = float((y.detach().double() * gd.double()).sum())
        rhs = float((xd.detach().double() * xd.grad.double()).sum())
        bound = 1e-6 * float((y.detach().double().abs() * gd.double().abs()).sum())
        print("adjoint K %d, %d blocks: |<Ax,g> - <x,ATg>| %.2e, bound %.2e" % (K, n, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound


# ---- 8. the module's surface on the device ------------------------------------------------------------------------------------
def test_module_surface_on_the_device(dev):
    K = 300
    x, h, _ = S.data(K, 512, 6, 6)
    xd = _dev(x, dev).reshape(2, 3, -1)
    off = A.ImpulseResponse(torch.from_numpy(h)).to(dev)
    rt = off.streaming()
    assert rt.ir is off.ir and rt.block == 512 and rt.ir.device.type == "cuda"
    want = off(xd)
    y = _run(rt, xd, 512, (1, 3, 2))
    print("streaming() against the offline module at the plan's block: %.2e, bit-equal %s"
          % (C.rel_max(_np(y), _np(want)), bool(torch.equal(y, want))))
    assert C.rel_max(_np(y), _np(want)) < TOL and C.rel_max(_np(y), S.reference(K, 512, 6, 6).reshape(2, 3, -1)) < TOL
    y, time = rt.forward_with_time(xd, torch.ones(2, 3, device=dev))
    assert y.shape == xd.shape and torch.equal(time, torch.ones(2, 3, device=dev))
    with pytest.warns(UserWarning):
        chain = (A.ImpulseResponse(torch.from_numpy(h)) + A.Mono()).realtime()    # still returns, with the warning
    assert isinstance(chain, A.ComposeAudioTransform)
    assert A.RealtimeImpulseResponse().to(dev)(xd) is xd                         # the pass-through returns x itself
    assert A.RealtimeImpulseResponse().to(dev)(xd[..., :5]).shape == (2, 3, 5)
    hooks = A.RealtimeImpulseResponse().to(dev)                                  # the hooks cut to whole blocks and never raise
    out = hooks.test_forward(xd[..., :3000])
    assert out.shape == (2, 3, 2560) and bool(out.any()) and bool(torch.isfinite(out).all())
    A.RealtimeImpulseResponse.test_scripted_transform(hooks)
    A.RealtimeImpulseResponse.test_scripted_transform(rt)
    empty = rt(xd[:0])
    assert empty.shape == (0, 3, xd.shape[-1])


def test_float64_is_refused_without_the_opt_in(dev):
    B, K = S.BLOCK, 300
    x, h, _ = S.data(K)
    xd = _dev(x[:3, :4 * B], dev)
    m = _module(h, B, dev)
    want = m(xd)
    m.reset()
    with pytest.raises(A.AcidsHipError):
        m(xd.double())
    with pytest.raises(A.AcidsHipError):
        _module(h.astype(np.float64), B, dev)(xd)
    with pytest.raises(A.AcidsHipError):
        m(xd.double().requires_grad_())
    assert m.head == 0 and not m.input_buffer.any()
    with A.allow_fp64_narrowing():
        y = m(xd.double())
        y64 = _module(h.astype(np.float64), B, dev)(xd)
    assert y.dtype == torch.float32 and torch.equal(y, want) and torch.equal(y64, want)

"""GPU side of the long-filter convolution (ops.fft_convolve / fft_convolve_backward / spectral_fir / spectral_fir_corr,
autograd.FFTConvolveFunction, transforms.FFTConvolve / Convolve / ImpulseResponse, csrc/fft_convolve.hip): parity of the
forward in all three modes and of both gradients with numpy.convolve and float64 conv1d autograd within the library's
normwise bound 1e-5, the adjoint identities, the bit rules that follow from one fixed chain per output element, what zeros
and a NaN must and must not do, and the spectral kernels on planted spectra against a float64 loop.

The NaN rule.  A NaN at x[r][n] sits in frames t0 = n // B and t0 + 1, whose spectra are NaN in every bin, so overlap-save
fills blocks t0 .. t0 + P of row r (P partitions) and nothing else.  The samples n .. n + K - 1 that the convolution itself
reaches lie in blocks t0 .. (n + K - 1) // B; the two sets are the same when n % B + K - 1 >= P B, and the positions marked
`exact` below are chosen so; at the others the last block of the first set lies one block past the second, which is as far as
any implementation of this algorithm can hold it, and the test pins that set.

Measured on an MI355X (worst figures, printed by the tests): see README, "FFTConvolve"."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import fft_convolve_cases as C
from acids_transforms_amd import ops
from acids_transforms_amd.autograd import FFTConvolveFunction

pytestmark = pytest.mark.gpu
TOL = C.TOL
SMALL = tuple((L, K) for L in C.LENGTHS for K in C.TAPS) + C.TILE_CASES
GRAD_CASES = ((1, 1), (1, 300), (127, 2), (128, 128), (129, 129), (129, 1000), (1000, 1), (1000, 300), (1000, 1000)) + C.TILE_CASES[1:3]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _filter(d, per_row, lead):
    return C.take(d["hr"], lead) if per_row else d["h"]


@pytest.mark.parametrize("per_row", (False, True), ids=("shared", "per_row"))
def test_forward_matches_numpy_convolve_in_every_mode_and_leading_shape(dev, per_row):
    """Every (L, K) of the case table at block 128; in the same loop: a row alone is the row in batches of 3, 6 and 70."""
    worst = dict(full=0.0, same=0.0, valid=0.0)
    for L, K in SMALL:
        d, ref = C.data(L, K), C.forward_reference(L, K, per_row)
        alone = None
        for lead in C.LEADS:
            x, h = _dev(C.take(d["x"], lead), dev), _dev(_filter(d, per_row, lead), dev)
            for mode in C.MODES if lead in ((), (C.ROWS,)) else ("full",):
                off, n = C.cut(L, K, mode)
                y = ops.fft_convolve(x, h, mode, block=C.BLOCK)
                assert y.shape == tuple(lead) + (n,) and y.dtype == torch.float32
                worst[mode] = max(worst[mode], C.rel_max(_np(y), C.take(ref[:, off:off + n], lead)))
                if mode == "full":
                    first = y.reshape(-1, n)[0]
                    alone = first if alone is None else alone
                    assert torch.equal(first, alone), (L, K, lead)
    print("forward %s: %s" % ("per row" if per_row else "shared", ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL, worst


@pytest.mark.parametrize("L,K,rows,block", C.BLOCK_CASES)
def test_the_other_blocks_of_the_ladder(dev, L, K, rows, block):
    """Forward and both gradients at blocks 256, 512, 1024 and 2048, by block=."""
    assert ops.fft_convolve_plan(L, K, block)[0] == block
    d = C.data(L, K, rows)
    for per_row in (False, True):
        hh = d["hr"] if per_row else d["h"]
        want, gx, gh = C.conv1d_autograd(d["x"], hh, d["g_full"])
        x, h = _dev(d["x"], dev).requires_grad_(), _dev(hh, dev).requires_grad_()
        y = FFTConvolveFunction.apply(x, h, "full", block)
        y.backward(_dev(d["g_full"], dev))
        figures = (C.rel_max(_np(y), C.oracle(d["x"], hh)), C.rel_max(_np(y), want), C.rel_max(_np(x.grad), gx),
                   C.rel_max(_np(h.grad), gh))
        print("block %d %s: forward %.2e (conv1d %.2e) gx %.2e gh %.2e" % ((block, "per row" if per_row else "shared") + figures))
        assert max(figures) < TOL, figures
        assert torch.equal(y.detach(), ops.fft_convolve(x.detach(), h.detach(), "full", block))


def _adjoint_identities(x, h, g, block, what):
    """<A x, g> = <x, A^T g> for fixed h and <conv(x, h), g> = <h, gh>, accumulated in float64 from the fp32 results, within
    1e-6 of sum |A x| |g|."""
    y = ops.fft_convolve(x, h, block=block)
    gx, gh = ops.fft_convolve_backward(x, h, g, block=block)
    lhs = float((y.double() * g.double()).sum())
    bound = 1e-6 * float((y.double().abs() * g.double().abs()).sum())
    in_x, in_h = float((x.double() * gx.double()).sum()), float((h.double() * gh.double()).sum())
    print("adjoint %s: |<Ax,g> - <x,ATg>| %.2e, |<Ax,g> - <h,gh>| %.2e, bound %.2e" % (what, abs(lhs - in_x), abs(lhs - in_h), bound))
    assert abs(lhs - in_x) <= bound and abs(lhs - in_h) <= bound


def test_the_rule_past_the_end_of_the_ladder(dev):
    """40 000 taps: the rule's 2048 with 20 partitions.  Forward against numpy.convolve in every mode, gradients by the adjoint
    identities."""
    L, K, rows = C.LONG_CASE
    d = C.data(L, K, rows)
    for per_row in (False, True):
        hh = d["hr"] if per_row else d["h"]
        x, h = _dev(d["x"], dev), _dev(hh, dev)
        worst = max(C.rel_max(_np(ops.fft_convolve(x, h, mode)), C.oracle(d["x"], hh, mode)) for mode in C.MODES)
        print("40 000 taps %s: forward %.2e" % ("per row" if per_row else "shared", worst))
        assert worst < TOL
        _adjoint_identities(x, h, _dev(d["g_full"], dev), None, "L %d K %d %s" % (L, K, "per row" if per_row else "shared"))


@pytest.mark.parametrize("per_row", (False, True), ids=("shared", "per_row"))
def test_gradients_match_float64_conv1d_autograd(dev, per_row):
    """gx and gh on 70 rows in every mode; the plain route and the autograd route give the same forward bits; the same call
    twice gives the same gradient bits; a row alone has the gradients it has in the batch (per-row filters: gh too)."""
    worst = dict(gx=0.0, gh=0.0)
    for L, K in GRAD_CASES:
        d = C.data(L, K)
        hh = d["hr"] if per_row else d["h"]
        for mode in C.MODES:
            _, gx, gh = C.gradient_reference(L, K, per_row, mode)
            x, h, g = _dev(d["x"], dev).requires_grad_(), _dev(hh, dev).requires_grad_(), _dev(d["g_" + mode], dev)
            y = FFTConvolveFunction.apply(x, h, mode, C.BLOCK)
            assert torch.equal(y.detach(), ops.fft_convolve(x.detach(), h.detach(), mode, block=C.BLOCK))
            y.backward(g)
            assert x.grad.shape == x.shape and h.grad.shape == h.shape
            worst["gx"] = max(worst["gx"], C.rel_max(_np(x.grad), gx))
            worst["gh"] = max(worst["gh"], C.rel_max(_np(h.grad), gh))
            if mode != "full":
                continue
            ax, ah = ops.fft_convolve_backward(x.detach(), h.detach(), g, mode, C.BLOCK)
            assert torch.equal(ax, x.grad) and torch.equal(ah, h.grad)                  # the same call, the same bits
            ox, oh = ops.fft_convolve_backward(x.detach(), h.detach(), g, mode, C.BLOCK, need_h=False)
            assert oh is None and torch.equal(ox, x.grad)
            ox, oh = ops.fft_convolve_backward(x.detach(), h.detach(), g, mode, C.BLOCK, need_x=False)
            assert ox is None and torch.equal(oh, h.grad)
            h1 = h.detach()[:1] if per_row else h.detach()
            for n_rows in (1, 3):
                bx, bh = ops.fft_convolve_backward(x.detach()[:n_rows], h.detach()[:n_rows] if per_row else h1, g[:n_rows],
                                                   mode, C.BLOCK)
                assert torch.equal(bx[0], x.grad[0])
                if per_row:
                    assert torch.equal(bh[0], h.grad[0])
    print("gradients %s: %s" % ("per row" if per_row else "shared", ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < TOL, worst


def test_only_the_gradients_that_are_needed_and_first_order_only(dev):
    d = C.data(1000, 300)
    x, h, g = _dev(d["x"][:3], dev), _dev(d["h"], dev), _dev(d["g_full"][:3], dev)
    plain = A.fftconvolve(x, h)
    assert plain.grad_fn is None
    xr = x.clone().requires_grad_()
    y = A.fftconvolve(xr, h)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    y.backward(g)
    assert xr.grad is not None and h.grad is None
    hr = h.clone().requires_grad_()
    y = A.fftconvolve(x, hr, "same")
    y.backward(g[:, :1000])
    assert hr.grad is not None and hr.grad.shape == h.shape
    with torch.no_grad():
        assert A.fftconvolve(xr, hr).grad_fn is None
    y = A.fftconvolve(xr, hr)
    (gx,) = torch.autograd.grad(y, xr, g, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # a filter that broadcasts along a leading axis: its gradient is summed back to its own shape
    x6, h2 = _dev(C.take(d["x"], (2, 3)), dev), _dev(d["hr"][:2, None], dev).requires_grad_()
    y = A.fftconvolve(x6, h2)
    assert y.shape == (2, 3, 1299)
    y.backward(_dev(C.take(d["g_full"], (2, 3)), dev))
    _, _, gh = C.conv1d_autograd(d["x"][:6], np.repeat(d["hr"][:2], 3, axis=0), d["g_full"][:6])
    assert h2.grad.shape == (2, 1, 300) and C.rel_max(_np(h2.grad)[:, 0], gh.reshape(2, 3, 300).sum(1)) < TOL


def test_float64_is_refused_without_the_opt_in(dev):
    """On the device, so that the check for a CPU tensor does not answer first: float64 audio or a float64 filter raise; with
    the opt-in they are narrowed and the result is the float32 one."""
    d = C.data(1000, 300)
    x, h = _dev(d["x"][:3], dev), _dev(d["h"], dev)
    want = ops.fft_convolve(x, h)
    for xx, hh in ((x.double(), h), (x, h.double()), (x.double(), h.double())):
        with pytest.raises(A.AcidsHipError):
            ops.fft_convolve(xx, hh)
        with pytest.raises(A.AcidsHipError):
            A.FFTConvolve()(xx, hh)
        with pytest.raises(A.AcidsHipError):
            ops.fft_convolve_backward(xx, hh, torch.zeros_like(want))
    with pytest.raises(A.AcidsHipError):
        A.ImpulseResponse(d["h"]).to(dev)(x.double())
    with pytest.raises(A.AcidsHipError):
        A.ImpulseResponse(d["h"].astype(np.float64)).to(dev)(x)
    with A.allow_fp64_narrowing():
        y = ops.fft_convolve(x.double(), h.double())
    assert y.dtype == torch.float32 and torch.equal(y, want)


def test_modules_agree_with_the_op_and_the_oracle(dev):
    worst = 0.0
    for L, K in ((1000, 300), (129, 1000), (127, 2)):
        d = C.data(L, K)
        for per_row in (False, True):
            lead = (2, 3)
            x, h = _dev(C.take(d["x"], lead), dev), _dev(_filter(d, per_row, lead), dev)
            ref = C.forward_reference(L, K, per_row)
            for mode in C.MODES:
                off, n = C.cut(L, K, mode)
                want = ops.fft_convolve(x, h, mode)
                for cls in (A.FFTConvolve, A.Convolve):
                    y = cls(mode).to(dev)(x, h)
                    assert torch.equal(y, want)
                worst = max(worst, C.rel_max(_np(want), C.take(ref[:, off:off + n], lead)))
        ir = _dev(d["h"], dev)
        x = _dev(C.take(d["x"], (2, 3)), dev)
        full = ops.fft_convolve(x, ir)
        body, tail = A.ImpulseResponse(d["h"]).to(dev), A.ImpulseResponse(torch.from_numpy(d["h"]), tail=True).to(dev)
        assert torch.equal(body(x), full[..., :L]) and torch.equal(tail(x), full)
        y, time = body.forward_with_time(x, torch.ones(2, 3, device=dev))
        assert torch.equal(y, full[..., :L]) and torch.equal(time, torch.ones(2, 3, device=dev))
        chain = body + A.ImpulseResponse(d["h"]).to(dev)
        assert torch.equal(chain(x), body(body(x)))
        worst = max(worst, C.rel_max(_np(tail(x)), C.take(C.forward_reference(L, K, False), (2, 3))))
    print("modules: forward %.2e" % worst)
    assert worst < TOL


def test_learnable_impulse_response(dev):
    L, K = 1000, 300
    d = C.data(L, K)
    rows = 6
    _, gx, gh = C.conv1d_autograd(d["x"][:rows], d["h"], np.pad(d["g_same"][:rows], ((0, 0), (0, K - 1))))
    m = A.ImpulseResponse(d["h"], learnable=True).to(dev)
    x = _dev(C.take(d["x"], (2, 3)), dev).requires_grad_()
    y = m(x)
    assert y.shape == (2, 3, L) and y.grad_fn is not None
    y.backward(_dev(C.take(d["g_same"], (2, 3)), dev))                           # the first L samples: the rest gets no gradient
    figures = (C.rel_max(_np(m.ir.grad), gh), C.rel_max(_np(x.grad).reshape(rows, L), gx))
    print("ImpulseResponse(learnable=True): gh %.2e gx %.2e" % figures)
    assert m.ir.grad.shape == (K,) and max(figures) < TOL
    frozen = A.ImpulseResponse(d["h"], learnable=True).to(dev)
    frozen(x.detach()).sum().backward()                                          # the response alone requires grad
    assert frozen.ir.grad is not None and bool(frozen.ir.grad.abs().sum() > 0)


@pytest.mark.parametrize("L,K", ((1000, 300), (129, 1000), (1, 129)))
def test_adjoint_identities(dev, L, K):
    d = C.data(L, K)
    for per_row in (False, True):
        _adjoint_identities(_dev(d["x"], dev), _dev(d["hr"] if per_row else d["h"], dev), _dev(d["g_full"], dev), C.BLOCK,
                            "L %d K %d %s" % (L, K, "per row" if per_row else "shared"))


def test_zeros_give_plus_zero_and_zero_gradients(dev):
    d = C.data(1000, 300)
    x, h, g = _dev(d["x"][:3], dev), _dev(d["h"], dev), _dev(d["g_full"][:3], dev)
    hr = _dev(d["hr"][:3], dev)
    for xx, hh in ((torch.zeros_like(x), h), (x, torch.zeros_like(h)), (torch.zeros_like(x), hr), (x, torch.zeros_like(hr))):
        y = ops.fft_convolve(xx, hh, block=C.BLOCK)
        assert not y.any() and not torch.signbit(y).any()
        gx, gh = ops.fft_convolve_backward(xx, hh, g, block=C.BLOCK)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gh).all())
        if not hh.any():
            assert not gx.any()
        if not xx.any():
            assert not gh.any()
    gx, gh = ops.fft_convolve_backward(x, h, torch.zeros_like(g), block=C.BLOCK)
    assert not gx.any() and not gh.any()


@pytest.mark.parametrize("n,exact", ((255, True), (999, True), (90, True), (0, False), (130, False)))
def test_a_nan_stays_in_its_row_and_its_blocks(dev, n, exact):
    L, K, r = 1000, 300, 1
    B, T, P, _, _ = ops.fft_convolve_plan(L, K, C.BLOCK)
    d = C.data(L, K)
    for per_row in (False, True):
        x, h = _dev(d["x"][:3], dev), _dev(d["hr"][:3] if per_row else d["h"], dev)
        clean = ops.fft_convolve(x, h, block=C.BLOCK)
        bad = x.clone()
        bad[r, n] = float("nan")
        y = ops.fft_convolve(bad, h, block=C.BLOCK)
        assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2])
        assert bool(torch.isnan(y[r, n:n + K]).all())                             # never lost where it belongs
        reach = set(range(n // B, min(n // B + P, T - 1) + 1))
        if exact:
            assert reach == set(C.nan_blocks(n, K, B, T))
        keep = torch.ones(T * B, dtype=torch.bool)
        for t in reach:
            keep[t * B:(t + 1) * B] = False
        keep = keep[:L + K - 1].to(dev)
        assert bool(torch.isfinite(y[r][keep]).all())
        assert C.rel_max(_np(y[r][keep]), _np(clean[r][keep])) < TOL


def test_chunks_of_rows_give_the_bits_of_one_chunk(dev, monkeypatch):
    """The row chunking, forced small: the forward and the per-row gradients are bit-identical to the run in one chunk, a
    shared filter's gradient -- chunk sums added in double -- agrees within the bound."""
    d = C.data(1000, 300)
    x, g = _dev(d["x"][:23], dev), _dev(d["g_full"][:23], dev)
    plan = ops.fft_convolve_plan
    for per_row in (False, True):
        h = _dev(d["hr"][:23] if per_row else d["h"], dev)
        one = ops.fft_convolve(x, h), ops.fft_convolve_backward(x, h, g)
        monkeypatch.setattr(ops, "fft_convolve_plan", lambda L, K, block=None: plan(L, K, block)[:4] + (5,))
        cut = ops.fft_convolve(x, h), ops.fft_convolve_backward(x, h, g)
        monkeypatch.setattr(ops, "fft_convolve_plan", plan)
        assert torch.equal(cut[0], one[0]) and torch.equal(cut[1][0], one[1][0])
        if per_row:
            assert torch.equal(cut[1][1], one[1][1])
        else:
            assert C.rel_max(_np(cut[1][1]), _np(one[1][1])) < 1e-6


# ---- the spectral kernels on planted spectra -------------------------------------------------------------------------------
def _planted(shape, seed, dev):
    g = np.random.default_rng(seed)
    a = (g.standard_normal(shape) + 1j * g.standard_normal(shape)).astype(np.complex64)
    return a, torch.from_numpy(a).to(dev)


@pytest.mark.parametrize("F", (129, 257))
def test_spectral_fir_on_planted_spectra(dev, F):
    """T = tile - 1, tile, tile + 1 and P in {1, 2, T, T + 3}, both directions and both conjugations, a shared filter and one
    per row, against the float64 loop; F = 257 has a second chunk of bins with one live lane."""
    tile, rows, worst = C.FRAME_TILE, 3, 0.0
    for T in (tile - 1, tile, tile + 1):
        Xn, X = _planted((rows, T, F), T, dev)
        for P in (1, 2, T, T + 3):
            for shared in (True, False):
                Hn, H = _planted((P, F) if shared else (rows, P, F), 100 + P, dev)
                for anti in (False, True):
                    for conj in (False, True):
                        Y = ops.spectral_fir(X, H, anticausal=anti, conj=conj)
                        assert Y.shape == (rows, T, F) and Y.dtype == torch.complex64
                        ref = C.spectral_fir_reference(Xn, Hn, anti, conj)
                        worst = max(worst, float(np.abs(_np(Y) - ref).max() / np.abs(ref).max()))
                        assert torch.equal(Y[:1], ops.spectral_fir(X[:1].contiguous(), H if shared else H[:1], anti, conj))
                # frames of a longer buffer: the row stride is not T F
                wide = torch.cat([X, X.flip(1)], dim=1)
                assert torch.equal(ops.spectral_fir(wide[:, :T], H), ops.spectral_fir(X, H))
    print("spectral_fir F %d: %.2e" % (F, worst))
    assert worst < TOL


def test_spectral_fir_nan_zero_and_persistent_grid(dev):
    tile, rows, T, P, F = C.FRAME_TILE, 3, 11, 4, 129
    Xn, X = _planted((rows, T, F), 1, dev)
    Hn, H = _planted((P, F), 2, dev)
    clean = ops.spectral_fir(X, H)
    bad = X.clone()
    bad[1, 5, 7] = complex(float("nan"), 0.0)
    y = ops.spectral_fir(bad, H)
    hit = torch.isnan(torch.view_as_real(y)).any(-1)
    assert bool(hit[1, 5:5 + P, 7].all()) and int(hit.sum()) == P                 # column (1, 7), frames 5 .. 5 + P - 1
    same = ~hit
    assert torch.equal(torch.view_as_real(y)[same], torch.view_as_real(clean)[same])
    z = ops.spectral_fir(torch.zeros_like(X), H)
    assert not torch.view_as_real(z).any() and not torch.signbit(torch.view_as_real(z)).any()
    z = ops.spectral_fir(X, torch.zeros_like(H), conj=True)
    assert not torch.view_as_real(z).any() and not torch.signbit(torch.view_as_real(z)).any()
    # more work items than the grid of persistent workgroups (8192): rows x 2 tiles x 1 chunk
    many, Tm, Fm = 4200, tile + 1, 3
    Xm_n, Xm = _planted((many, Tm, Fm), 3, dev)
    Hm_n, Hm = _planted((2, Fm), 4, dev)
    ym = ops.spectral_fir(Xm, Hm)
    ref = C.spectral_fir_reference(Xm_n, Hm_n)
    assert float(np.abs(_np(ym) - ref).max() / np.abs(ref).max()) < TOL
    for r in (0, 4095, 4096, 4199):
        assert torch.equal(ym[r:r + 1], ops.spectral_fir(Xm[r:r + 1].contiguous(), Hm))


@pytest.mark.parametrize("T,P", ((7, 1), (9, 9), (9, 12), (64, 3), (65, 8), (150, 17)))
def test_spectral_fir_corr_on_planted_spectra(dev, T, P):
    """Against the float64 loop on both sides of the slice of 64 frames and of the tile of partitions; per-row results do not
    depend on the batch; the same call twice gives the same bits."""
    rows, F = 5, 129
    Xn, X = _planted((rows, T, F), T, dev)
    Gn, G = _planted((rows, T, F), T + 1000, dev)
    for shared in (True, False):
        gH = ops.spectral_fir_corr(X, G, P, shared)
        ref = C.spectral_fir_corr_reference(Xn, Gn, P, shared)
        assert gH.shape == ref.shape
        err = float(np.abs(_np(gH) - ref).max() / np.abs(ref).max())
        print("spectral_fir_corr T %d P %d %s: %.2e" % (T, P, "shared" if shared else "per row", err))
        assert err < TOL
        assert torch.equal(gH, ops.spectral_fir_corr(X, G, P, shared))
        if not shared:
            assert torch.equal(gH[2:3], ops.spectral_fir_corr(X[2:3].contiguous(), G[2:3].contiguous(), P, False))
    for shared in (True, False):                                                  # no frames: zeros, no plan, no workspace
        none = ops.spectral_fir_corr(X[:, :0], G[:, :0], P, shared)
        assert none.shape == ((P, F) if shared else (rows, P, F)) and not torch.view_as_real(none).any()
    many = 300                                                                    # a shared filter over many rows: several groups
    Xn, X = _planted((many, T, 3), 7, dev)
    Gn, G = _planted((many, T, 3), 8, dev)
    ref = C.spectral_fir_corr_reference(Xn, Gn, P, True)
    assert float(np.abs(_np(ops.spectral_fir_corr(X, G, P, True)) - ref).max() / np.abs(ref).max()) < TOL

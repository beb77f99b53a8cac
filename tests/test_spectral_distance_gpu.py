"""SpectralDistance on the GPU: the two kernels of csrc/spectral_distance.hip against float64, the module against the
float64 torch.stft chain, the routing, and the three independence properties (chunks, batch, isolation).  Tolerance:
normwise rel_max < 1e-5 against float64, as for every other value and gradient of the package.

The gradient from audio is linearised at the spectrum the library computed, as test_repr_grad_gpu.py does for the phase
chains: the float64 formula gradient at ops.stft_forward's output is pushed through the float64 adjoint of torch.stft.
End-to-end fp32 torch autograd of this chain is itself 4.5e-3 off float64 on this input (1 / (A + eps) amplifies the
STFT's rounding in near-empty bins), while its linearised comparison is at 2e-7 on every one of the seven scales."""
import functools

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import spectral_distance_cases as C
from acids_transforms_amd import autograd, ops
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5


def cpu(t):
    return t.detach().cpu().numpy()


def bits(t):
    return cpu(t).view(np.int32 if t.dtype == torch.float32 else np.int64)


# ---- op level --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _op_case(shape):
    """(X, Y, g, float64 sums, float64 autograd G_X, G_Y) of one op-level shape; computed once, never written."""
    X, Y = C.spectra(shape, seed=shape[1] * 7 + shape[2])
    g = np.random.default_rng(5).standard_normal(shape[0]).astype(np.float32)
    GX, GY = C.autograd_backward(X, Y, g, 0.7, 1.9)
    return X, Y, g, C.model_sums(X, Y), GX, GY


@pytest.mark.parametrize("shape", C.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_against_float64(dev, shape):
    X, Y, _, want, _, _ = _op_case(shape)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    got = ops.spectral_distance_sums(Xd, Yd, C.EPS)
    assert got.shape == (shape[0], 3) and got.dtype == torch.float64
    for k, name in enumerate(("S_D", "S_B", "S_L")):
        err = rel_max(cpu(got)[:, k], want[:, k])
        print(shape, name, "err %.3g" % err)
        assert err < TOL, (name, err)
    assert np.array_equal(cpu(Xd), X) and np.array_equal(cpu(Yd), Y)           # read only
    # (B, n) and (B, T, F) are one layout; `out=` a slice of a larger tensor
    out = torch.zeros((shape[0] + 1, 3), dtype=torch.float64, device=dev)
    ops.spectral_distance_sums(Xd.reshape(shape[0], -1), Yd.reshape(shape[0], -1), C.EPS, out=out[1:])
    assert np.array_equal(bits(out[1:]), bits(got)) and not out[0].any()


@pytest.mark.parametrize("need", [(True, False), (False, True), (True, True)], ids=["x", "y", "xy"])
@pytest.mark.parametrize("shape", C.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_against_float64_autograd_of_the_same_spectra(dev, shape, need):
    X, Y, g, _, wantX, wantY = _op_case(shape)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    sums = ops.spectral_distance_sums(Xd, Yd, C.EPS)
    rX, rY = ops.spectral_distance_backward(Xd, Yd, sums, torch.from_numpy(g).to(dev), 0.7, 1.9, C.EPS, *need)
    assert rX is Xd and rY is Yd                                               # in place
    for got, want, src, needed in ((Xd, wantX, X, need[0]), (Yd, wantY, Y, need[1])):
        if not needed:
            assert np.array_equal(cpu(got).view(np.int32), src.view(np.int32))   # bit-unchanged
            continue
        err = rel_max(cpu(got), want)
        print(shape, need, "err %.3g" % err)
        assert err < TOL, err
        assert np.all(cpu(got)[np.abs(src) == 0] == 0)                         # exact zeros where the magnitude vanishes


# ---- module level ------------------------------------------------------------------------------------------------------------

def _audio(dev, B=C.MODULE_B, L=C.MODULE_L, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(B, L, generator=gen)).to(dev), (0.1 * torch.randn(B, L, generator=gen)).to(dev)


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """Per-clip float64 loss of the torch.stft chain on _audio's clips, per weights (1, 1)."""
    x, y = _audio("cpu")
    return C.chain_loss(x.double(), y.double(), C.SCALES).numpy()


def _linearised(crit, x, y, g, need_x, need_y):
    """The expected gradients: the float64 formula gradient at the spectra the library computed, through the float64
    adjoint of torch.stft, summed over scales.  g (B,) float64: the gradient of the per-clip loss."""
    wx, wy = torch.zeros(x.shape, dtype=torch.float64), torch.zeros(y.shape, dtype=torch.float64)
    for (n, hop), w in zip(crit.scales, crit._windows()):
        X, Y = (cpu(ops.stft_forward(t, w, n, hop, center=True)) for t in (x, y))
        GX, GY = C.model_backward(X, Y, g, crit.lin_weight, crit.log_weight, crit.eps, need_x, need_y)
        if need_x:
            wx += C.stft_adjoint64(x.cpu().double(), n, hop, GX)
        if need_y:
            wy += C.stft_adjoint64(y.cpu().double(), n, hop, GY)
    return wx.numpy(), wy.numpy()


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_forward_value_against_the_float64_chain(dev, reduction):
    x, y = _audio(dev)
    crit = A.SpectralDistance(scales=C.SCALES, reduction=reduction).to(dev)
    got = crit(x, y)
    per = _chain_reference()
    want = {"none": per, "sum": per.sum(), "mean": per.mean()}[reduction]
    assert got.dtype == torch.float32 and got.shape == np.shape(want) and got.grad_fn is None
    err = rel_max(cpu(got), want)
    print(reduction, "err %.3g" % err)
    assert err < TOL


@pytest.mark.parametrize("need", [(True, False), (False, True), (True, True)], ids=["x", "y", "xy"])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_gradient_linearised_at_the_library_spectrum(dev, reduction, need):
    x, y = _audio(dev)
    crit = A.SpectralDistance(scales=C.SCALES, lin_weight=0.8, log_weight=1.5, reduction=reduction).to(dev)
    xr, yr = x.clone().requires_grad_(need[0]), y.clone().requires_grad_(need[1])
    loss = crit(xr, yr)
    assert loss.grad_fn is not None
    B = x.shape[0]
    if reduction == "none":
        g = torch.tensor([0.6, -1.1, 2.0])
        loss.backward(g.to(dev))
    else:
        g = torch.full((B,), 1.0 if reduction == "sum" else 1.0 / B)
        loss.backward()
    wantx, wanty = _linearised(crit, x, y, g.double().numpy(), *need)
    for t, want, needed in ((xr, wantx, need[0]), (yr, wanty, need[1])):
        if not needed:
            assert t.grad is None
            continue
        assert t.grad.shape == t.shape and t.grad.dtype == torch.float32
        err = rel_max(cpu(t.grad), want)
        print(reduction, need, "err %.3g" % err)
        assert err < TOL, err


def test_leading_batch_dims(dev):
    x, y = _audio(dev, B=6)
    crit = A.SpectralDistance(reduction="none").to(dev)
    xr = x.clone().requires_grad_()
    flat = crit(xr, y)
    (gflat,) = torch.autograd.grad(flat.sum(), xr)
    x3 = x.reshape(2, 3, -1).clone().requires_grad_()
    out = crit(x3, y.reshape(2, 3, -1))
    assert out.shape == (2, 3) and np.array_equal(bits(out.reshape(6)), bits(flat))
    (g3,) = torch.autograd.grad(out.sum(), x3)
    assert g3.shape == (2, 3, C.MODULE_L) and np.array_equal(bits(g3.reshape(6, -1)), bits(gflat))
    one = crit(x[0], y[0])                                                     # a bare clip (L,)
    assert one.shape == () and np.array_equal(bits(one.reshape(1)), bits(flat[:1]))


# ---- routing -----------------------------------------------------------------------------------------------------------------

def test_routing_and_saved_tensors(dev):
    x, y = _audio(dev)
    crit = A.SpectralDistance(reduction="none").to(dev)
    plain = crit(x, y)
    assert plain.grad_fn is None
    xr = x.clone().requires_grad_()
    routed = crit(xr, y)
    assert np.array_equal(bits(routed), bits(plain))                           # the same kernels, the same bits
    with torch.no_grad():
        quiet = crit(xr, y)
    assert quiet.grad_fn is None and np.array_equal(bits(quiet), bits(plain))
    # the node of the Function: the two audios and the (B, n_scales, 3) float64 sums, and nothing else
    node = routed.grad_fn
    while node is not None and "SpectralDistanceFunction" not in type(node).__name__:
        node = node.next_functions[0][0] if node.next_functions else None
    assert node is not None
    saved = node.saved_tensors
    assert len(saved) == 3
    assert saved[0].shape == x.shape and saved[1].shape == y.shape and saved[0].dtype == torch.float32
    assert saved[0].data_ptr() == xr.data_ptr() and saved[1].data_ptr() == y.data_ptr()    # the caller's own storage
    assert saved[2].shape == (C.MODULE_B, 5, 3) and saved[2].dtype == torch.float64
    # first order only
    with pytest.raises(RuntimeError):
        (gx,) = torch.autograd.grad(crit(xr, y).sum(), xr, create_graph=True)
        gx.sum().backward()
    # float64 needs the explicit opt-in
    with pytest.raises(A.AcidsHipError):
        crit(x.double(), y.double())
    with A.allow_fp64_narrowing():
        narrowed = crit(x.double(), y.double())
    assert narrowed.dtype == torch.float32 and np.array_equal(bits(narrowed), bits(plain))
    # the module follows its input's device, as STFT does
    fresh = A.SpectralDistance(reduction="none")
    assert np.array_equal(bits(fresh(x, y)), bits(plain)) and fresh.window_0.device == x.device


# ---- chunks, batch independence, isolation ---------------------------------------------------------------------------------

def _loss_and_grads(crit, x, y):
    xr, yr = x.clone().requires_grad_(), y.clone().requires_grad_()
    loss = crit(xr, yr)
    gx, gy = torch.autograd.grad(loss.sum(), (xr, yr))
    return loss.detach(), gx, gy


def test_chunked_run_has_the_bits_of_the_one_chunk_run(dev, monkeypatch):
    x, y = _audio(dev, B=5, seed=3)
    crit = A.SpectralDistance(reduction="none").to(dev)
    whole = _loss_and_grads(crit, x, y)
    monkeypatch.setattr(autograd, "SPECDIST_CHUNK_ELEMS", 20000)
    for n, hop in crit.scales:                                                 # 2 + 2 + 1 clips at every scale
        assert [b1 - b0 for b0, b1 in autograd._specdist_chunks(5, C.MODULE_L, n, hop)] == [2, 2, 1]
    cut = _loss_and_grads(crit, x, y)
    for a, b in zip(whole, cut):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(crit(x, y)), bits(whole[0]))                    # the plain route, chunked


def test_a_clip_does_not_depend_on_its_batch(dev):
    x, y = _audio(dev, B=7, seed=4)
    crit = A.SpectralDistance(reduction="none").to(dev)
    alone = _loss_and_grads(crit, x[3:4], y[3:4])
    for pos in (0, 3, 6):                                                      # first, in the middle, last of 7
        order = list(range(7))
        order[pos], order[3] = order[3], order[pos]
        got = _loss_and_grads(crit, x[order], y[order])
        for a, b in zip(alone, got):
            assert np.array_equal(bits(a[0]), bits(b[pos])), pos


def test_isolation(dev):
    x, y = _audio(dev, B=4, seed=6)
    crit = A.SpectralDistance(reduction="none").to(dev)
    clean = _loss_and_grads(crit, x, y)
    others = [0, 1, 3]
    # a NaN sample in clip 2 of x: that clip's loss and gradient rows are non-finite (x's where a frame that holds the
    # sample reaches, y's everywhere: S_D is in every bin of it), every other clip keeps its bits
    xn = x.clone()
    xn[2, 1000] = float("nan")
    loss, gx, gy = _loss_and_grads(crit, xn, y)
    assert not torch.isfinite(loss[2]) and not torch.isfinite(gx[2]).all() and not torch.isfinite(gy[2]).any()
    for a, b in zip(clean, (loss, gx, gy)):
        assert np.array_equal(bits(a[others]), bits(b[others]))
    # an all-zero target clip: S_B == 0 gives inf or nan there, and only there
    y0 = y.clone()
    y0[2] = 0
    loss, gx, gy = _loss_and_grads(crit, x, y0)
    assert not torch.isfinite(loss[2]) and not torch.isfinite(gx[2]).all()
    for a, b in zip(clean, (loss, gx, gy)):
        assert np.array_equal(bits(a[others]), bits(b[others]))
    # an all-zero generated clip against a live target: a finite loss and an exactly zero gradient row
    x0 = x.clone()
    x0[2] = 0
    loss, gx, _ = _loss_and_grads(crit, x0, y)
    assert torch.isfinite(loss).all() and not gx[2].any() and torch.isfinite(gx).all()
    assert np.array_equal(bits(clean[0][others]), bits(loss[others])) and np.array_equal(bits(clean[1][others]), bits(gx[others]))

"""MelSpectralDistance on the GPU: the three kernels of csrc/mel_distance.hip against float64 on every plan they take,
the module against the float64 torch.stft chain, the routing, the bit rules (the recomputed mel row has the bits of the
stored one; chunks, batch, isolation).  Tolerance: normwise rel_max < 1e-5 against float64, as for every other value
and gradient of the package.

The gradient from audio is linearised at the spectrum the library computed, as test_spectral_distance_gpu.py does and
for its reason: the float64 formula gradient at ops.stft_forward's output is pushed through the float64 adjoint of
torch.stft.  End-to-end fp32 torch autograd of this chain is itself 2.7e-5 (x) and 1.9e-5 (y) off float64 on this
input (1 / (M + eps) amplifies the STFT's rounding in near-empty cells), while the linearised comparison is at
1.5e-7 ... 3.1e-7 on the seven scales (profiles/mel_distance_probe.md)."""
import functools

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import mel_distance_cases as C
from acids_transforms_amd import autograd, ops
from acids_transforms_amd.utils.banded import BandedBank, bank_columns
from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
LIN, LOG = 0.7, 1.9


def cpu(t):
    return t.detach().cpu().numpy()


def bits(t):
    return cpu(t).view(np.int32 if t.dtype == torch.float32 else np.int64)


def sid(s):
    return "x".join(map(str, s))


# ---- op level --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _op_case(shape):
    """Of one op-level shape (B, T, F, n_mels): the spectra, the bank, g, and in float64 the mel rows and the autograd
    gradients of both spectra; computed once, never written."""
    X, Y = C.spectra(shape, seed=shape[1] * 7 + shape[2])
    W = C.bank(shape[2], shape[3])
    g = np.random.default_rng(5).standard_normal(shape[0]).astype(np.float32)
    GX, GY = C.autograd_backward(X, Y, W, g, LIN, LOG)
    return dict(X=X, Y=Y, W=W, g=g, M=C.model_mel_rows(X, W), Q=C.model_mel_rows(Y, W), GX=GX, GY=GY)


def _tables(W, dev):
    return (tuple(torch.from_numpy(a).to(dev) for a in bank_columns(W)),
            tuple(torch.from_numpy(a).to(dev) for a in bank_columns(W.t())))


def _all_shapes(dev):
    return C.OP_SHAPES + (C.many_rows_shape(torch.cuda.get_device_properties(dev).multi_processor_count),)


def _shape(dev, i):
    shapes = _all_shapes(dev)
    shape = shapes[i]
    if i == len(C.OP_SHAPES):                 # the many-rows case: at least three trips, a partial last one
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        for p in C.bank_plans(C.bank(shape[2], shape[3])):
            n_trips, last = C.trips(shape[0] * shape[1], p, cus)
            assert n_trips >= 3 and last > 0
    return shape


CASES = list(range(len(C.OP_SHAPES) + 1))
CASE_IDS = [sid(s) for s in C.OP_SHAPES] + ["many_rows"]


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_mel_rows_against_float64_and_the_banded_projection(dev, i):
    shape = _shape(dev, i)
    c = _op_case(shape)
    Xd = torch.from_numpy(c["X"]).to(dev)
    cols, _ = _tables(c["W"], dev)
    got = ops.mel_rows(Xd, cols)
    assert got.shape == shape[:2] + (shape[3],) and got.dtype == torch.float32
    err = rel_max(cpu(got), c["M"])
    # at_mel_project_banded with no contrast where the bank is eligible for it (the dense projection otherwise)
    band = BandedBank(c["W"])
    proj = ops.mel_forward(Xd, c["W"].to(dev), contrast=None, band=band)
    err_proj = rel_max(cpu(got), cpu(proj).astype(np.float64))
    print(shape, "err %.3g" % err, "against the %s projection %.3g" % ("banded" if band.eligible else "dense", err_proj))
    assert err < TOL and err_proj < TOL
    assert band.eligible == (shape[2] != 8193)
    empty = ~(c["W"] != 0).any(0).numpy()
    assert empty.sum() == C.empty_filters(c["W"]) and not cpu(got)[..., empty].any()     # empty filters: exactly 0
    assert np.array_equal(cpu(Xd), c["X"])                                                 # read only
    out = torch.zeros((shape[0] + 1,) + got.shape[1:], dtype=torch.float32, device=dev)   # `out=` a slice
    ops.mel_rows(Xd, cols, out=out[1:])
    assert np.array_equal(bits(out[1:]), bits(got)) and not out[0].any()


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_sums_against_float64(dev, i):
    shape = _shape(dev, i)
    c = _op_case(shape)
    M32, Q32 = c["M"].astype(np.float32), c["Q"].astype(np.float32)
    want = C.model_sums(M32, Q32)
    Md, Qd = torch.from_numpy(M32).to(dev), torch.from_numpy(Q32).to(dev)
    got = ops.mel_distance_sums(Md, Qd, C.EPS)
    assert got.shape == (shape[0], 3) and got.dtype == torch.float64
    for k, name in enumerate(("S_D", "S_B", "S_L")):
        err = rel_max(cpu(got)[:, k], want[:, k])
        print(shape, name, "err %.3g" % err)
        assert err < TOL, (name, err)
    assert np.array_equal(cpu(Md), M32) and np.array_equal(cpu(Qd), Q32)       # read only
    out = torch.zeros((shape[0] + 1, 3), dtype=torch.float64, device=dev)
    ops.mel_distance_sums(Md.reshape(shape[0], -1), Qd.reshape(shape[0], -1), C.EPS, out=out[1:])
    assert np.array_equal(bits(out[1:]), bits(got)) and not out[0].any()
    # a clip's sums are those it has alone, wherever it sits in the batch
    last = ops.mel_distance_sums(Md[-1:].contiguous(), Qd[-1:].contiguous(), C.EPS)
    assert np.array_equal(bits(last), bits(got[-1:]))


@pytest.mark.parametrize("side", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_backward_against_float64_autograd_of_the_same_spectra(dev, i, side):
    shape = _shape(dev, i)
    c = _op_case(shape)
    Xd, Yd = torch.from_numpy(c["X"]).to(dev), torch.from_numpy(c["Y"]).to(dev)
    cols, cols_t = _tables(c["W"], dev)
    M, Q = ops.mel_rows(Xd, cols), ops.mel_rows(Yd, cols)
    sums = ops.mel_distance_sums(M, Q, C.EPS)
    S, O, other = (Xd, Q, Yd) if side == 0 else (Yd, M, Xd)
    src, src_other, want = (c["X"], c["Y"], c["GX"]) if side == 0 else (c["Y"], c["X"], c["GY"])
    keep = O.clone()
    r = ops.mel_distance_backward(S, O, sums, torch.from_numpy(c["g"]).to(dev), cols, cols_t, LIN, LOG, C.EPS, side)
    assert r is S                                                              # in place
    got = cpu(S)
    err = rel_max(got, want)
    print(shape, "side", side, "err %.3g" % err)
    assert err < TOL, err
    assert np.all(got[np.abs(src) == 0] == 0)                                  # exact zeros where the magnitude vanishes
    assert np.all(got[..., 0] == 0) and np.all(got[..., -1] == 0)              # DC and Nyquist: empty bank rows
    assert np.array_equal(bits(O), bits(keep))                                 # what is not differentiated is not written
    assert np.array_equal(cpu(other).view(np.int32), src_other.view(np.int32))
    # the last clip alone has the bits it has in the batch
    S1 = torch.from_numpy(src[-1:]).to(dev)
    ops.mel_distance_backward(S1, O[-1:].contiguous(), sums[-1:].contiguous(), torch.from_numpy(c["g"][-1:]).to(dev), cols,
                              cols_t, LIN, LOG, C.EPS, side)
    assert np.array_equal(cpu(S1).view(np.int32), got[-1:].view(np.int32))


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_recomputed_mel_row_has_the_bits_of_the_stored_one(dev, i):
    """Fed its own mel rows as the other signal's, every d is exactly 0: the gradient is exactly zero on both sides (on
    side 1 through S_D = 0).  One differing bit in a recomputed cell would leave sgn(d) / (M + eps) there."""
    shape = _shape(dev, i)
    c = _op_case(shape)
    cols, cols_t = _tables(c["W"], dev)
    Xd = torch.from_numpy(c["X"]).to(dev)
    M = ops.mel_rows(Xd, cols)
    sums = ops.mel_distance_sums(M, M, C.EPS)
    assert not cpu(sums)[:, 0].any() and not cpu(sums)[:, 2].any() and cpu(sums)[:, 1].all()
    g = torch.from_numpy(c["g"]).to(dev)
    for side in (0, 1):
        S = Xd.clone()
        ops.mel_distance_backward(S, M, sums, g, cols, cols_t, LIN, LOG, C.EPS, side)
        assert not cpu(S).view(np.float32).any(), side


# ---- module level ------------------------------------------------------------------------------------------------------------

def _audio(dev, B=C.MODULE_B, L=C.MODULE_L, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(B, L, generator=gen)).to(dev), (0.1 * torch.randn(B, L, generator=gen)).to(dev)


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """Per-clip float64 loss of the torch.stft chain on _audio's clips, weights (1, 1)."""
    x, y = _audio("cpu")
    return C.chain_loss(x.double(), y.double(), C.SCALES).numpy()


def _linearised(crit, x, y, g, need_x, need_y):
    """The expected gradients: the float64 formula gradient at the spectra the library computed, through the float64
    adjoint of torch.stft, summed over scales.  g (B,) float64: the gradient of the per-clip loss."""
    wx, wy = torch.zeros(x.shape, dtype=torch.float64), torch.zeros(y.shape, dtype=torch.float64)
    for i, ((n, hop, _), w) in enumerate(zip(crit.scales, crit._windows())):
        X, Y = (cpu(ops.stft_forward(t, w, n, hop, center=True)) for t in (x, y))
        W = getattr(crit, "mel_bank_%d" % i).cpu()
        GX, GY = C.model_gradients(X, Y, W, g, crit.lin_weight, crit.log_weight, crit.eps, need_x, need_y)
        if need_x:
            wx += C.stft_adjoint64(x.cpu().double(), n, hop, GX)
        if need_y:
            wy += C.stft_adjoint64(y.cpu().double(), n, hop, GY)
    return wx.numpy(), wy.numpy()


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_forward_value_against_the_float64_chain(dev, reduction):
    x, y = _audio(dev)
    crit = A.MelSpectralDistance(scales=C.SCALES, reduction=reduction).to(dev)
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
    crit = A.MelSpectralDistance(scales=C.SCALES, lin_weight=0.8, log_weight=1.5, reduction=reduction).to(dev)
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


def test_routing_and_saved_tensors(dev):
    x, y = _audio(dev)
    crit = A.MelSpectralDistance(reduction="none").to(dev)
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
    while node is not None and "MelSpectralDistanceFunction" not in type(node).__name__:
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
    # the module follows its input's device, as STFT does; leading batch dims and a bare clip
    fresh = A.MelSpectralDistance(reduction="none")
    assert np.array_equal(bits(fresh(x, y)), bits(plain)) and fresh.mel_bank_0.device == x.device
    one = crit(x[0], y[0])
    assert one.shape == () and np.array_equal(bits(one.reshape(1)), bits(plain[:1]))
    out = crit(x.reshape(3, 1, -1), y.reshape(3, 1, -1))
    assert out.shape == (3, 1) and np.array_equal(bits(out.reshape(3)), bits(plain))


def _loss_and_grads(crit, x, y):
    xr, yr = x.clone().requires_grad_(), y.clone().requires_grad_()
    loss = crit(xr, yr)
    gx, gy = torch.autograd.grad(loss.sum(), (xr, yr))
    return loss.detach(), gx, gy


def test_equal_signals_give_an_exactly_zero_loss_and_gradient(dev):
    x, _ = _audio(dev)
    crit = A.MelSpectralDistance(scales=C.SCALES, reduction="none").to(dev)
    loss, gx, gy = _loss_and_grads(crit, x, x.clone())
    assert not loss.any() and not gx.any() and not gy.any()
    assert not crit(x, x.clone()).any()
    # one shared stretch of samples: the frames it covers alone get an exactly zero log term, so the log-only loss
    # is smaller than with no shared frame, and still equals the float64 chain
    y = _audio(dev, seed=1)[0]
    y[:, 1024:3072] = x[:, 1024:3072]
    logonly = A.MelSpectralDistance(scales=((128, 32, 20),), lin_weight=0.0, reduction="none").to(dev)
    M, Q = (ops.mel_rows(ops.stft_forward(t, logonly.window_0, 128, 32), _tables(logonly.mel_bank_0.cpu(), dev)[0]) for t in (x, y))
    shared = slice(40, 88)          # frames wholly inside the stretch (34 .. 94), with every frame that shares an FFT with them
    assert np.array_equal(bits(M[:, shared]), bits(Q[:, shared])) and not np.array_equal(bits(M), bits(Q))
    want = C.chain_loss(x.cpu().double(), y.cpu().double(), logonly.scales, 0.0, 1.0).numpy()
    err = rel_max(cpu(logonly(x, y)), want)
    print("shared frames err %.3g" % err)
    assert err < TOL


def test_chunked_run_has_the_bits_of_the_one_chunk_run(dev, monkeypatch):
    x, y = _audio(dev, B=5, seed=3)
    crit = A.MelSpectralDistance(reduction="none").to(dev)
    whole = _loss_and_grads(crit, x, y)
    monkeypatch.setattr(autograd, "SPECDIST_CHUNK_ELEMS", 20000)
    for n, hop, _ in crit.scales:                                              # 2 + 2 + 1 clips at every scale
        assert [b1 - b0 for b0, b1 in autograd._specdist_chunks(5, C.MODULE_L, n, hop)] == [2, 2, 1]
    cut = _loss_and_grads(crit, x, y)
    for a, b in zip(whole, cut):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(crit(x, y)), bits(whole[0]))                    # the plain route, chunked


def test_a_clip_does_not_depend_on_its_batch(dev):
    x, y = _audio(dev, B=7, seed=4)
    crit = A.MelSpectralDistance(reduction="none").to(dev)
    alone = _loss_and_grads(crit, x[3:4], y[3:4])
    for pos in (0, 3, 6):                                                      # first, in the middle, last of 7
        order = list(range(7))
        order[pos], order[3] = order[3], order[pos]
        got = _loss_and_grads(crit, x[order], y[order])
        for a, b in zip(alone, got):
            assert np.array_equal(bits(a[0]), bits(b[pos])), pos


def test_isolation(dev):
    x, y = _audio(dev, B=4, seed=6)
    crit = A.MelSpectralDistance(reduction="none").to(dev)
    clean = _loss_and_grads(crit, x, y)
    others = [0, 1, 3]
    # a NaN sample in clip 2 of x: that clip's loss and gradient rows are non-finite (x's where a frame that holds the
    # sample reaches, y's everywhere: S_D is in every cell of it), every other clip keeps its bits
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

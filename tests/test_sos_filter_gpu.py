"""GPU side of the recursive filters (ops.sos_filter, autograd.SosFilterFunction / SosFilterStreamFunction,
transforms.SOSFilter / RealtimeSOSFilter / Preemphasis, at_sos_filter of csrc/sos_filter.hip): parity of forward, reverse,
zero-phase and carried state with the float64 recurrence of sos_filter_cases.py within the library's normwise bound 1e-5
at every length around the kernel's lane and tile cuts, the bit rules that follow from one fixed order per row, gradients
against the oracle's adjoint, streaming, and what a NaN and a row of zeros must and must not do."""

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import sos_filter_cases as C
from acids_transforms_amd import _lib, ops
from acids_transforms_amd.autograd import SosFilterFunction

pytestmark = pytest.mark.gpu
TOL = C.TOL


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_reverse_zero_phase_and_state_match_the_float64_recurrence(dev, name):
    """Every length of the case table at every leading shape; the same loop holds the bit rules: reverse is flip -> forward
    -> flip, and a row alone is the row inside batches of 3, 6 and 70."""
    sos = C.FILTERS[name]
    zp_module = A.SOSFilter(sos, zero_phase=True).to(dev)
    worst = dict(fwd=0.0, rev=0.0, zp=0.0, yzi=0.0, zf=0.0)
    for L in C.lengths(sos.shape[0]):
        ref = C.case(name, L)
        alone = {}
        for lead in C.LEADS:
            x = _dev(C.take(ref["x"], lead), dev)
            zi = _dev(C.take(ref["zi"], lead), dev)
            fwd = ops.sos_filter(x, sos)
            rev = ops.sos_filter(x, sos, reverse=True)
            yzi, zf = ops.sos_filter(x, sos, zi=zi, return_state=True)
            zp = zp_module(x)
            assert fwd.shape == rev.shape == yzi.shape == zp.shape == x.shape and fwd.dtype == torch.float32
            assert zf.shape == zi.shape and zf.dtype == torch.float64
            assert torch.equal(rev, ops.sos_filter(x.flip(-1), sos).flip(-1))
            assert torch.equal(zp, ops.sos_filter(fwd, sos, reverse=True))
            for key, got in (("fwd", fwd), ("rev", rev), ("zp", zp), ("yzi", yzi)):
                worst[key] = max(worst[key], C.rel_max(got.cpu().numpy(), C.take(ref[key], lead)))
            worst["zf"] = max(worst["zf"], C.rel_max(zf.cpu().numpy(), C.take(ref["zf"], lead)))
            first = dict(fwd=fwd.reshape(-1, L)[0], rev=rev.reshape(-1, L)[0], yzi=yzi.reshape(-1, L)[0],
                         zf=zf.reshape(-1, sos.shape[0], 2)[0])
            if not alone:
                alone = first
            for key in alone:
                assert torch.equal(first[key], alone[key]), (key, L, lead)
    print("%s: %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))
    for key in ("fwd", "rev", "zp", "yzi"):
        assert worst[key] < TOL, (key, worst)
    assert worst["zf"] < C.STATE_TOL, worst


def test_one_dispatch_so_no_threshold_to_straddle(dev):
    """The plan reports one dispatch at every shape, so `both sides of every dispatch threshold` is every shape: a row of
    2 tiles + 5 alone, in a batch of 3 and as the last of 2100 rows (past the grid of persistent workgroups)."""
    sos = C.FILTERS["cascade4"]
    tile, _, _ = C.plan(4)
    for rows, L in ((1, 1), (1, 2 * tile + 5), (3, 2 * tile + 5), (2100, 33), (2100, tile + 1)):
        assert ops.sos_filter_plan(rows, L, 4)[2] == 0
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2100, 33, generator=g).to(dev)
    y = ops.sos_filter(x, sos)
    for r in (0, 2047, 2048, 2099):
        assert torch.equal(y[r], ops.sos_filter(x[r].clone(), sos))
    assert C.rel_max(y.cpu().numpy(), C.sosfilt(sos, x.cpu().numpy())[0]) < TOL


def test_module_and_op_give_the_same_bits(dev):
    sos = C.FILTERS["cascade4"]
    tile = C.plan(4)[0]
    x = _dev(C.take(C.case("cascade4", tile + 1)["x"], (2, 3)), dev)
    want = ops.sos_filter(x, sos)
    for zero_phase in (False, True):
        m = A.SOSFilter(sos, zero_phase=zero_phase).to(dev)
        target = ops.sos_filter(want, sos, reverse=True) if zero_phase else want
        with torch.no_grad():
            assert torch.equal(m(x), target)
        plain = m(x)
        assert plain.grad_fn is None and torch.equal(plain, target)
        routed = m(x.clone().requires_grad_())
        assert routed.grad_fn is not None and torch.equal(routed.detach(), target)
        y, time = m.forward_with_time(x, torch.ones(2, 3, device=dev))
        assert torch.equal(y, target) and torch.equal(time, torch.ones(2, 3, device=dev))
    assert torch.equal(SosFilterFunction.apply(x.clone().requires_grad_(), sos, False).detach(), want)
    # module casts touch no coefficient: the kernel reads the float64 host copy
    cast = A.SOSFilter(sos).half().float().to(dev)
    assert torch.equal(cast(x), want)
    assert torch.equal(A.SOSFilter(sos).to(dev).half()(x), want)
    loaded = A.SOSFilter()
    loaded.load_state_dict(A.SOSFilter(sos).half().state_dict())
    assert torch.equal(loaded.to(dev)(x), want)
    # float64 audio is refused without the opt-in; the state must be float64
    with pytest.raises(A.AcidsHipError):
        ops.sos_filter(x.double(), sos)
    with pytest.raises(A.AcidsHipError):
        ops.sos_filter(x, sos, zi=torch.zeros(2, 3, 4, 2, device=dev))
    with pytest.raises(ValueError):
        ops.sos_filter(x, sos, zi=torch.zeros(2, 3, 3, 2, device=dev, dtype=torch.float64))
    with pytest.raises(A.AcidsHipError):
        ops.sos_filter(x, np.tile(sos, (5, 1))[:17])                     # more than 16 sections


@pytest.mark.parametrize("name", ["highpass20", "resonator", "cascade4", "cascade16"])
def test_gradients_match_the_oracle_adjoint(dev, name):
    sos = C.FILTERS[name]
    tile = C.plan(sos.shape[0])[0]
    L, lead = tile + 1, (2, 3)
    ref = C.case(name, L)
    x = C.take(ref["x"], lead)
    g = np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)
    g64 = g.astype(np.float64)
    xd, gd = _dev(x, dev), _dev(g, dev)
    worst = {}

    def grad_of(fn):
        xr = xd.clone().requires_grad_()
        y = fn(xr)
        (y * gd).sum().backward()
        assert xr.grad.shape == xd.shape and xr.grad.dtype == torch.float32
        return y.detach(), xr.grad

    y, gx = grad_of(lambda t: SosFilterFunction.apply(t, sos, False))
    want = C.sosfilt_reverse(sos, g64)
    worst["op"] = C.rel_max(gx.cpu().numpy(), want)
    assert torch.equal(gx, ops.sos_filter(gd, sos, reverse=True))
    # <Hx, g> = <x, H^T g>, accumulated in float64 from the float32 results
    y64, gx64 = y.cpu().numpy().astype(np.float64), gx.cpu().numpy().astype(np.float64)
    worst["dot"] = abs(np.sum(y64 * g64) - np.sum(x.astype(np.float64) * gx64)) / np.sum(np.abs(y64) * np.abs(g64))
    _, gx = grad_of(lambda t: SosFilterFunction.apply(t, sos, True))
    worst["op_rev"] = C.rel_max(gx.cpu().numpy(), C.sosfilt(sos, g64)[0])
    _, gx = grad_of(A.SOSFilter(sos).to(dev))
    worst["module"] = C.rel_max(gx.cpu().numpy(), want)
    _, gx = grad_of(A.SOSFilter(sos, zero_phase=True).to(dev))
    worst["zero_phase"] = C.rel_max(gx.cpu().numpy(), C.zero_phase(sos, g64))
    print("%s: %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst.pop("dot") < 1e-6
    assert max(worst.values()) < TOL, worst
    with pytest.raises(RuntimeError):                    # first order only
        xr = xd.clone().requires_grad_()
        (gy,) = torch.autograd.grad(A.SOSFilter(sos).to(dev)(xr).sum(), xr, create_graph=True)
        gy.sum().backward()


def test_preemphasis_forward_invert_and_their_gradients(dev):
    L = C.plan(1)[0] + 1
    ref = C.case("peak1k", L)
    x = C.take(ref["x"], (2, 3))
    x64 = x.astype(np.float64)
    xd = _dev(x, dev)
    pre = A.Preemphasis(0.97).to(dev)
    want = x64.copy()
    want[..., 1:] -= 0.97 * x64[..., :-1]
    y = pre(xd)
    assert C.rel_max(y.cpu().numpy(), want) < TOL
    de = C.sosfilt([[1.0, 0.0, 0.0, 1.0, -0.97, 0.0]], x64)[0]
    assert C.rel_max(pre.invert(xd).cpu().numpy(), de) < TOL
    assert C.rel_max(pre.invert(y).cpu().numpy(), x64) < TOL
    out = pre.test_inversion(xd)
    assert isinstance(out, dict) and C.rel_max(out["inverted"].cpu().numpy(), x64) < TOL
    g = np.random.default_rng(8).standard_normal(x.shape).astype(np.float32)
    gd, g64 = _dev(g, dev), g.astype(np.float64)
    for fn, sos in ((pre, pre.coefficients), (pre.invert, [[1.0, 0.0, 0.0, 1.0, -0.97, 0.0]])):
        xr = xd.clone().requires_grad_()
        (fn(xr) * gd).sum().backward()
        assert C.rel_max(xr.grad.cpu().numpy(), C.sosfilt_reverse(sos, g64)) < TOL
    rt = pre.realtime()
    assert isinstance(rt, A.RealtimeSOSFilter)
    chunks = torch.cat([rt(xd[..., :100]), rt(xd[..., 100:])], -1)
    assert C.rel_max(chunks.cpu().numpy(), want) < TOL


@pytest.mark.parametrize("name", ["highpass20", "resonator", "cascade4", "kweighting"])
def test_streaming_chunks_concatenate_to_the_one_call_result(dev, name):
    sos = C.FILTERS[name]
    n = sos.shape[0]
    tile = C.plan(n)[0]
    cuts = (1, 16, tile - 1, tile + 1, 300)
    L, lead = sum(cuts), (2, 3)
    x = np.random.default_rng(9).standard_normal(lead + (L,)).astype(np.float32)
    want, want_zf = C.sosfilt(sos, x.astype(np.float64))
    xd = _dev(x, dev)
    one_call = ops.sos_filter(xd, sos).cpu().numpy()
    scale = np.abs(one_call).max()
    rt = A.SOSFilter(sos).to(dev).streaming()
    assert isinstance(rt, A.RealtimeSOSFilter) and rt.latency == 0
    worst, at = dict(oracle=0.0, one_call=0.0), 0
    for c in cuts:
        y = rt(xd[..., at:at + c])
        assert y.shape == lead + (c,) and y.dtype == torch.float32 and rt.state.shape == lead + (n, 2)
        assert rt.state.dtype == torch.float64 and not rt.state.requires_grad
        got = y.cpu().numpy()
        worst["oracle"] = max(worst["oracle"], np.abs(got - want[..., at:at + c]).max() / np.abs(want).max())
        worst["one_call"] = max(worst["one_call"], np.abs(got - one_call[..., at:at + c]).max() / scale)
        at += c
    worst["state"] = C.rel_max(rt.state.cpu().numpy(), want_zf)
    print("%s: %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["oracle"] < TOL and worst["one_call"] < 1e-6 and worst["state"] < C.STATE_TOL, worst
    # an empty chunk launches nothing and keeps the state
    before = rt.state.clone()
    assert rt(xd[..., :0]).shape == lead + (0,) and torch.equal(rt.state, before)
    # a state_dict round trip carries the stream on; a module cast of the state is undone
    other = A.RealtimeSOSFilter(C.FILTERS["peak1k"])
    other.load_state_dict(rt.state_dict())
    other = other.to(dev)
    tail = xd[..., :50]
    a = rt(tail)
    assert torch.equal(other(tail), a)
    # reset(), and a new batch shape, start from zeros
    rt.reset()
    assert not rt.state.any() and torch.equal(rt(tail), ops.sos_filter(tail, sos))
    assert torch.equal(rt(xd[0, :, :40]), ops.sos_filter(xd[0, :, :40].contiguous(), sos)) and rt.state.shape == (3, n, 2)
    half = rt.half()
    assert half.state.dtype == torch.float16
    rounded = half.state.double()                        # the cast cost the state its digits, and nothing else
    y = half(xd[0, :, 40:80])
    assert half.state.dtype == torch.float64 and y.dtype == torch.float32
    assert torch.equal(y, ops.sos_filter(xd[0, :, 40:80].contiguous(), sos, zi=rounded))


def test_streaming_gradient_is_the_zero_state_adjoint_of_the_chunk(dev):
    sos = C.FILTERS["cascade4"]
    tile = C.plan(4)[0]
    x = np.random.default_rng(10).standard_normal((2, 3, tile + 40)).astype(np.float32)
    g = np.random.default_rng(12).standard_normal((2, 3, tile + 1)).astype(np.float32)
    xd, gd = _dev(x, dev), _dev(g, dev)
    rt = A.RealtimeSOSFilter(sos).to(dev)
    rt(xd[..., :39])                                     # the stream has a history
    state = rt.state.clone()
    plain = ops.sos_filter(xd[..., 39:].contiguous(), sos, zi=state)
    chunk = xd[..., 39:].clone().requires_grad_()
    y = rt(chunk)
    assert y.grad_fn is not None and torch.equal(y.detach(), plain) and not rt.state.requires_grad
    (y * gd).sum().backward()
    assert torch.equal(chunk.grad, ops.sos_filter(gd, sos, reverse=True))
    assert C.rel_max(chunk.grad.cpu().numpy(), C.sosfilt_reverse(sos, g.astype(np.float64))) < TOL


@pytest.mark.parametrize("reverse", [False, True])
def test_a_nan_stays_behind_its_sample_and_inside_its_row(dev, reverse):
    sos = C.FILTERS["cascade4"]
    tile, per_lane, _ = C.plan(4)
    L = 2 * tile + 5
    x = _dev(C.take(C.case("cascade4", L)["x"], (3,)), dev)
    clean = ops.sos_filter(x, sos, reverse=reverse)
    for n in (0, 5, per_lane, per_lane + 1, 64 * per_lane - 1, 64 * per_lane, 100 * per_lane + 3, tile - 1, tile, tile + 70,
              2 * tile + 4):
        bad = x.clone()
        at = L - 1 - n if reverse else n                 # the n-th sample the filter meets
        bad[1, at] = float("nan")
        y = ops.sos_filter(bad, sos, reverse=reverse)
        assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2]), n
        before = (y[1, at + 1:], clean[1, at + 1:]) if reverse else (y[1, :at], clean[1, :at])
        after = y[1, :at + 1] if reverse else y[1, at:]
        assert torch.equal(*before), n
        assert bool(torch.isnan(after).all()), n


def test_zeros_give_positive_zero_and_nothing_is_written_past_a_row(dev):
    tile = C.plan(4)[0]
    for name in ("highpass20", "cascade4", "cascade16"):
        sos = C.FILTERS[name]
        for L in (1, 17, tile + 1):
            x = torch.zeros(3, L, device=dev)
            for reverse in (False, True):
                y = ops.sos_filter(x, sos, reverse=reverse)
                assert not y.view(torch.int32).any(), (name, L, reverse)           # +0: no sign bit either
            y, zf = ops.sos_filter(-x, sos, return_state=True)                     # -0 in
            assert not y.view(torch.int32).any() and not zf.any()
    # the C entry on a buffer with a guard behind the last row
    sos = ops.sos_coefficients(C.FILTERS["cascade4"])
    rows, L = 3, tile + 7
    x = _dev(C.take(C.case("cascade4", tile + 1)["x"], (3,)), dev)
    x = torch.cat([x, x[:, :6]], -1).contiguous()
    for reverse in (0, 1):
        buf = torch.full((rows * L + 4096,), 7.0, device=dev)
        head = torch.full((4096,), 7.0, device=dev)
        whole = torch.cat([head, buf])
        y = whole[4096:]
        _lib.check(_lib.lib().at_sos_filter(_lib.ptr(x), rows, L, sos.ptr, sos.n, reverse, None, None, _lib.ptr(y),
                                            _lib.stream_ptr()), "at_sos_filter")
        torch.cuda.synchronize()
        assert bool((whole[:4096] == 7.0).all()) and bool((y[rows * L:] == 7.0).all())
        assert torch.equal(y[:rows * L].reshape(rows, L), ops.sos_filter(x, sos, reverse=bool(reverse)))


def test_empty_inputs_and_the_state_of_an_empty_row(dev):
    sos = ops.sos_coefficients(C.FILTERS["kweighting"])
    assert ops.sos_filter(torch.zeros(0, 9, device=dev), sos).shape == (0, 9)
    zi = torch.randn(4, 2, 2, device=dev, dtype=torch.float64)
    y, zf = ops.sos_filter(torch.zeros(4, 0, device=dev), sos, zi=zi, return_state=True)
    assert y.shape == (4, 0) and torch.equal(zf, zi) and zf.data_ptr() != zi.data_ptr()
    y, zf = ops.sos_filter(torch.zeros(4, 0, device=dev), sos, return_state=True)
    assert zf.shape == (4, 2, 2) and not zf.any()

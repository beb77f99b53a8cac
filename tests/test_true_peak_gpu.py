"""GPU side of the true-peak measure (ops.true_peak, ops.true_peak_stream, ops.true_peak_backward, transforms.TruePeak,
RealtimeTruePeak, LoudnessNormalize(peak_limit=...); csrc/true_peak.hip) against the float64 oracle of true_peak_cases.py.

Parity: the library's normwise bound 1e-5 on the linear peak (8.7e-5 dB, so 1e-4 dB on dBTP) and the index EQUAL, on the five
tables, at every length around the filter's and the tile's ends, at 1, 3, 70 and 70 000 rows, and with the maximum planted
inside the first K - 1 samples, at the last sample, across a tile edge, in the last lane of a wave, and negative.  Bits: a row
alone against its batches, a long row against its pieces, zeros, NaN, +-inf, guard bands.  Stream: RealtimeTruePeak under
five chunkings EQUAL to the one-call TruePeak.  Gradient: against the analytic subgradient and float64 torch autograd of
conv1d -> abs -> amax, normwise < 1e-5.  The inputs' margins are checked in test_true_peak_cpu.py.

Measured on an MI355X (worst figures, printed by the tests): the linear peak 2.8e-7 normwise and 2.5e-6 dB from the oracle
(70 000 rows of 40), every index equal; every chunk's own peak within the same bound; the gradients at most 1.2e-7 normwise
(0 for the linear peak: the subgradient is a tap times +-1), through LoudnessNormalize(peak_limit=-1) 6.8e-8; the limited
clips land at -1.0000014 and -0.9999998 dBTP (11.7 and 18.2 dBTP without the limit)."""
import ctypes

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import true_peak_cases as C
from acids_transforms_amd import _lib, ops

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _taps(name, dev):
    return _dev(C.tables()[name], dev)


def _assert_parity(peak, index, sign, ref, what):
    """Normwise 1e-5 on the linear peak, 1e-4 dB per row, index and sign equal."""
    assert float(ref["margin"].min()) >= C.MARGIN, what                      # the condition on the input
    got = peak.double().cpu().numpy()
    err = float(np.abs(got - ref["peak"]).max() / np.abs(ref["peak"]).max())
    db = float(np.abs(C.dbtp(got) - C.dbtp(ref["peak"])).max())
    print("%s: normwise %.2e, %.2e dB, margin %.1e" % (what, err, db, float(ref["margin"].min())))
    assert err <= C.TOL and db <= C.TOL_DB, (what, err, db)
    assert np.array_equal(index.cpu().numpy(), ref["index"]), what
    if sign is not None:
        assert np.array_equal(sign.cpu().numpy(), ref["sign"]), what


def _measure(name, dev):
    table, x = C.case(name)
    return ops.true_peak(_dev(x, dev), _taps(table, dev), return_state=True)


# ---- parity against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", C.TABLES)
def test_parity_at_every_length(dev, table):
    K = C.tables()[table].shape[1]
    for L in C.lengths(K):
        name = "%s/L=%d" % (table, L)
        peak, index, sign = _measure(name, dev)
        _assert_parity(peak, index, sign, C.reference(name), name)


@pytest.mark.parametrize("spot", sorted(C.SPOTS))
def test_parity_with_the_maximum_planted(dev, spot):
    peak, index, sign = _measure("spot/" + spot, dev)
    _assert_parity(peak, index, sign, C.reference("spot/" + spot), spot)


@pytest.mark.parametrize("rows", C.ROW_COUNTS)
def test_parity_at_row_counts(dev, rows):
    peak, index, sign = _measure("rows/%d" % rows, dev)
    _assert_parity(peak, index, sign, C.reference("rows/%d" % rows), "rows %d" % rows)


def test_parity_past_65535_rows(dev):
    peak, index, sign = _measure("many", dev)
    assert peak.shape == (C.MANY_ROWS,) and C.MANY_ROWS > 65535
    _assert_parity(peak, index, sign, C.reference("many"), "70 000 rows of 40")


def test_module_reads_the_oracles_dbtp(dev):
    """The five Tech 3341 signals through the module, and every reading of the module on one planted clip."""
    m = A.TruePeak(sr=48000).to(dev)
    for number, (_, _, _, expected) in C.TECH3341.items():
        x = C.tech3341(number).astype(np.float32)
        ref = float(C.dbtp(C.measure(x, C.tables()["bs1770"])["peak"]))
        got = m(_dev(np.stack([x, 0.5 * x])[None], dev))                     # (1, 2, L): stereo, the right channel 6 dB down
        assert got.shape == (1, 2) and abs(got[0, 0].item() - ref) <= C.TOL_DB
        assert expected - 0.4 <= got[0, 0].item() <= expected + 0.2
        assert abs(got[0, 1].item() - (ref + 20.0 * np.log10(0.5))) <= C.TOL_DB
        assert m.programme(_dev(np.stack([0.5 * x, x])[None], dev)).shape == (1,)
        assert abs(m.programme(_dev(np.stack([0.5 * x, x])[None], dev)).item() - ref) <= C.TOL_DB
    table, x = C.case("spot/negative")
    ref, xd = C.reference("spot/negative"), _dev(x, dev)
    assert torch.equal(m.linear(xd), ops.true_peak(xd, m.taps)) and np.array_equal(m.index(xd).cpu().numpy(), ref["index"])
    assert torch.equal(m(xd), 20.0 * torch.log10(m.linear(xd)))
    assert m(xd[0]).shape == () and torch.equal(m(xd[0]), m(xd)[0]) and torch.equal(m.programme(xd[0]), m(xd)[0])
    assert torch.equal(m.programme(xd), m(xd).amax(-1))
    sample = m.sample_peak(xd)
    assert torch.equal(sample, 20.0 * torch.log10(xd.abs().amax(-1)))         # the identity table: bits of the largest sample
    y, time = m.forward_with_time(xd, torch.ones(3, device=dev))
    assert torch.equal(y, m(xd)) and torch.equal(time, torch.ones(3, device=dev))
    assert m(xd[:, :0]).shape == (3,) and bool(torch.isneginf(m(xd[:, :0])).all())       # no sample: silence
    assert torch.equal(m(xd.half()), m(xd.half().float()))                    # widening only


# ---- bits ------------------------------------------------------------------------------------------------------------------

def test_a_rows_bits_do_not_depend_on_its_batch(dev):
    _, x = C.case("rows/70")
    taps, xd = _taps("bs1770", dev), _dev(x, dev)
    whole = ops.true_peak(xd, taps, return_state=True)
    three = ops.true_peak(xd[:3].contiguous(), taps, return_state=True)
    for r in range(3):
        alone = ops.true_peak(xd[r:r + 1].contiguous(), taps, return_state=True)
        for a, b, c in zip(alone, three, whole):
            assert torch.equal(a[0], b[r]) and torch.equal(a[0], c[r])
    for name in ("kaiser 8x7", "random 3x5"):                                 # the generic copy
        taps = _taps(name, dev)
        whole = ops.true_peak(xd, taps, return_state=True)
        alone = ops.true_peak(xd[69:70].contiguous(), taps, return_state=True)
        assert all(torch.equal(a[0], w[69]) for a, w in zip(alone, whole))


@pytest.mark.parametrize("table", ["bs1770", "kaiser 2x16"])
def test_a_long_row_is_the_maximum_over_its_pieces(dev, table):
    h = C.tables()[table]
    P, K = h.shape
    L = 4 * C.TILE + 3
    x = C.planted(h, 2, L, np.array([3 * C.TILE + 1, 500]), 4)
    taps, xd = _taps(table, dev), _dev(x, dev)
    peak, index, _ = ops.true_peak(xd, taps, return_state=True)
    _assert_parity(peak, index, None, C.measure(x, h), "4 tile + 3")
    cuts = [0, 1000, C.TILE + 7, C.TILE + 9, 3 * C.TILE, L]
    pieces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        state = _dev(C.next_state(x[:, :a], K), dev)
        pieces.append(ops.true_peak_stream(xd[:, a:b].contiguous(), taps, state, torch.empty_like(state),
                                           torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int64, device=dev), P * a))
    assert torch.equal(torch.stack(pieces).amax(0), peak)


def test_zeros_nan_and_infinities(dev):
    m = A.TruePeak().to(dev)
    z = torch.zeros(3, 2 * C.TILE + 5, device=dev)
    peak, index, sign = ops.true_peak(z, m.taps, return_state=True)
    assert torch.equal(peak, torch.zeros(3, device=dev)) and not bool(torch.signbit(peak).any())      # +0
    assert not bool(index.any()) and not bool(sign.any()) and bool(torch.isneginf(m(z)).all())
    assert not bool(m.index(-z).any()) and not bool(torch.signbit(m.linear(-z)).any())                # -0 in, +0 out
    _, x = C.case("spot/tile edge")
    clean = ops.true_peak(_dev(x, dev), m.taps, return_state=True)
    for n in (0, 700, C.TILE - 1, C.TILE + 900, x.shape[1] - 1):                                      # one tile and two
        for width in (x.shape[1], min(x.shape[1], C.TILE)):
            if n >= width:
                continue
            bad = x[:, :width].copy()
            bad[1, n] = np.nan
            ref = ops.true_peak(_dev(x[:, :width], dev), m.taps, return_state=True)
            peak, index, sign = ops.true_peak(_dev(bad, dev), m.taps, return_state=True)
            assert bool(torch.isnan(peak[1])) and index[1].item() == 4 * n and sign[1].item() == 0.0
            for r in (0, 2):                                                                          # no other row
                assert all(torch.equal(a[r], b[r]) for a, b in zip((peak, index, sign), ref))
            assert bool(torch.isnan(m(_dev(bad, dev))[1]))
    assert all(torch.equal(a, b) for a, b in zip(clean, ops.true_peak(_dev(x, dev), m.taps, return_state=True)))
    for table in ("bs1770", "kaiser 8x7", "identity"):
        taps = _taps(table, dev)
        inf = x.copy()
        inf[0, 33], inf[1, C.TILE + 40], inf[2, 5] = np.inf, -np.inf, np.inf
        inf[2, 900] = np.nan                                                                          # a NaN beats an infinity
        peak, index, sign = ops.true_peak(_dev(inf, dev), taps, return_state=True)
        assert peak[0].item() == float("inf") == peak[1].item() and bool(torch.isnan(peak[2]))
        P = taps.shape[0]
        assert index[0].item() == P * 33 and index[1].item() == P * (C.TILE + 40) and index[2].item() == P * 900


def test_guard_bands_stay_intact(dev):
    """Every output of one call sits inside a larger buffer of sentinels: nothing outside it is written."""
    lib = _lib.lib()
    _, x = C.case("spot/tile edge")
    rows, L = x.shape
    xd = _dev(x, dev)
    for table in ("bs1770", "random 3x5"):
        taps = _taps(table, dev)
        P, K = taps.shape
        for n in (5, L):                                                       # one launch, and two
            state = _dev(C.next_state(x[:, :100], K), dev)
            chunk = xd[:, 100:100 + n].contiguous() if n < L else xd
            f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)       # noqa: E731
            peak, sign, running, nxt = f(rows + 8), f(rows + 8), f(rows + 8), f(rows * (K - 1) + 8)
            index = torch.full((rows + 8,), -7, dtype=torch.int64, device=dev)
            rindex = torch.full((rows + 8,), -7, dtype=torch.int64, device=dev)
            running[4:4 + rows] = 0.0
            nbytes = lib.at_true_peak_workspace_bytes(rows, chunk.shape[1], P, K)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            at = lambda t, skip: ctypes.c_void_p(t.data_ptr() + skip * t.element_size())           # noqa: E731
            with torch.cuda.device(dev):
                _lib.check(lib.at_true_peak(_lib.ptr(chunk), rows, chunk.shape[1], _lib.ptr(taps), P, K, _lib.ptr(state),
                                            at(nxt, 4), at(peak, 4), at(index, 4), at(sign, 4), at(running, 4), at(rindex, 4), 1000,
                                            _lib.ptr(ws), nbytes, _lib.stream_ptr()), "at_true_peak")
            torch.cuda.synchronize()
            ref = ops.true_peak_stream(chunk, taps, state, torch.empty_like(state), torch.zeros(rows, device=dev),
                                       torch.zeros(rows, dtype=torch.int64, device=dev), 1000)
            for t in (peak, sign, running, index, rindex):
                assert bool((t[:4] == -7).all()) and bool((t[4 + rows:] == -7).all())
            assert bool((nxt[:4] == SENTINEL).all()) and bool((nxt[4 + rows * (K - 1):] == SENTINEL).all())
            assert torch.equal(peak[4:4 + rows], ref) and torch.equal(running[4:4 + rows], ref)
            assert torch.equal(index[4:4 + rows], rindex[4:4 + rows]) and bool((index[4:4 + rows] >= 1000).all())
            want = C.next_state(chunk.cpu().numpy(), K, state.cpu().numpy())
            assert np.array_equal(nxt[4:4 + rows * (K - 1)].cpu().numpy().reshape(rows, K - 1), want)


# ---- the stream ------------------------------------------------------------------------------------------------------------

def _run(rt, xd, chunks, at=0):
    outs = []
    for n in chunks:
        outs.append(rt(xd[..., at:at + n]))
        at += n
    return outs


@pytest.mark.parametrize("name", sorted(C.CHUNK_LISTS))
def test_stream_equals_the_one_call_measurement_to_the_bit(dev, name):
    chunks = C.CHUNK_LISTS[name]
    total = sum(chunks)
    x = C.stream_signal(total)
    xd, h = _dev(x, dev), C.tables()["bs1770"]
    P, K = h.shape
    off, rt = A.TruePeak(sr=48000).to(dev), A.RealtimeTruePeak(sr=48000).to(dev)
    outs = _run(rt, xd, chunks)
    # every forward: the chunk's own outputs, by the kernel on [the K - 1 samples before | chunk] and by the oracle
    at = 0
    for n, out in zip(chunks, outs):
        before = C.next_state(x[..., :at], K)
        state = _dev(before, dev)
        own = ops.true_peak_stream(xd[..., at:at + n].contiguous(), off.taps, state, torch.empty_like(state),
                                   torch.zeros(2, 2, device=dev), torch.zeros(2, 2, dtype=torch.int64, device=dev), 0)
        assert out.shape == (2, 2) and torch.equal(out, 20.0 * torch.log10(own))
        ref = C.measure(x[..., at:at + n], h, before)["peak"]
        assert float(np.abs(own.double().cpu().numpy() - ref).max() / ref.max()) <= C.TOL
        at += n
    # the running maximum, its index and the carried samples: the one-call TruePeak on the concatenation
    assert torch.equal(rt.peak(), off(xd)) and torch.equal(rt.linear(), off.linear(xd))
    assert torch.equal(rt.index(), off.index(xd)) and torch.equal(rt.programme(), off.programme(xd))
    assert torch.equal(rt.input_buffer, _dev(C.next_state(x, K), dev)) and rt.samples_seen == total
    assert np.array_equal(rt.index().cpu().numpy(), C.measure(x, h)["index"])
    assert rt.peak().requires_grad is False and outs[0].requires_grad is False
    # the same list again gives the same bits; so does a stream resumed from a state taken mid-stream
    again = A.RealtimeTruePeak(sr=48000).to(dev)
    half = len(chunks) // 2
    first = _run(again, xd, chunks[:half])
    resumed = A.RealtimeTruePeak(sr=48000).to(dev)
    resumed.load_state_dict(again.state_dict())
    assert resumed.samples_seen == sum(chunks[:half])
    rest = _run(resumed, xd, chunks[half:], at=sum(chunks[:half]))
    assert all(torch.equal(a, b) for a, b in zip(first + rest, outs))
    for a, b in ((resumed.peak(), rt.peak()), (resumed.index(), rt.index()), (resumed.input_buffer, rt.input_buffer)):
        assert torch.equal(a, b)


def test_stream_state_reset_and_new_leading_shape(dev):
    chunks = C.CHUNK_LISTS["short then long"]
    x = C.stream_signal(sum(chunks))
    xd = _dev(x, dev)
    rt = A.RealtimeTruePeak(sr=48000).to(dev)
    first = _run(rt, xd, chunks)
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else dict(v)) for k, v in rt.state_dict().items()}
    assert tuple(sd["input_buffer"].shape) == (2, 2, 11) and sd["_extra_state"] == {"samples_seen": sum(chunks)}
    rt.reset()
    assert rt.samples_seen == 0 and not bool(rt.input_buffer.any()) and not bool(rt.max_peak.any()) and not bool(rt.max_index.any())
    assert all(torch.equal(a, b) for a, b in zip(_run(rt, xd, chunks), first))                       # a stream from zeros again
    # a new leading shape starts a new stream from zeros; a 1-D chunk is one mono stream
    mono = xd[0, 0]
    out = rt(mono[:300])
    fresh = A.RealtimeTruePeak(sr=48000).to(dev)
    assert out.shape == () and torch.equal(out, fresh(mono[:300])) and rt.samples_seen == 300
    assert tuple(rt.input_buffer.shape) == (11,) and tuple(rt.max_peak.shape) == ()
    assert torch.equal(rt.peak(), A.TruePeak(sr=48000).to(dev)(mono[:300]))
    # strided and half chunks are copied and widened, never narrowed
    wide = A.RealtimeTruePeak(sr=48000).to(dev)
    assert torch.equal(wide(xd.transpose(0, 1)[..., :500]), A.TruePeak(sr=48000).to(dev)(xd.transpose(0, 1)[..., :500].contiguous()))
    with pytest.raises(A.AcidsHipError):
        wide(xd.double()[..., :10])
    # the other tables stream too: the generic copy, and the sample peak, which carries no samples
    for kw in (dict(oversample=8), dict(sr=96000), dict(oversample=1)):
        off, srt = A.TruePeak(**kw).to(dev), A.RealtimeTruePeak(**kw).to(dev)
        _run(srt, xd, chunks)
        assert torch.equal(srt.peak(), off(xd)) and torch.equal(srt.index(), off.index(xd)), kw
        assert srt.input_buffer.shape[-1] == off.taps.shape[1] - 1


# ---- gradients -------------------------------------------------------------------------------------------------------------

def _autograd_reference(x, h, db, programme=False):
    """float64 torch autograd of conv1d -> abs -> amax on the same table: x (rows, L) -> (value (rows,), gradient of its sum)."""
    P, K = h.shape
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_()
    w = torch.from_numpy(np.asarray(h, dtype=np.float64)).flip(-1)[:, None, :]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(xt, (K - 1, 0))[:, None, :], w)            # (rows, P, L)
    peak = y.abs().amax(dim=(1, 2))
    value = 20.0 * torch.log10(peak) if db else peak
    if programme:
        value = value.amax()
    (g,) = torch.autograd.grad(value.sum(), xt)
    return value.detach().numpy(), g.numpy()


def _analytic(x, h, db):
    """The subgradient written out: g sign(y[index]) h[p*][n* - n]."""
    P, K = h.shape
    ref = C.measure(x, h)
    g = np.zeros(np.shape(x))
    for r in range(g.shape[0]):
        n, p = divmod(int(ref["index"][r]), P)
        scale = ref["sign"][r] * (20.0 / (np.log(10.0) * ref["peak"][r]) if db else 1.0)
        for k in range(K):
            if 0 <= n - k:
                g[r, n - k] = scale * h[p, k]
    return g


def _normwise(got, ref):
    return float(np.abs(got.double().cpu().numpy() - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", ["spot/tile edge", "spot/negative 8x7", "spot/early", "random 3x5/L=2049", "identity/L=2047"])
def test_gradient_against_autograd_and_the_analytic_form(dev, name):
    table, x = C.case(name)
    h = C.tables()[table]
    m = A.TruePeak(taps=torch.from_numpy(h.copy())).to(dev)
    for db, call in ((True, m), (False, m.linear)):
        value, want = _autograd_reference(x, h, db)
        assert np.abs(want - _analytic(x, h, db)).max() <= 1e-12 * np.abs(want).max()
        xd = _dev(x, dev).requires_grad_()
        y = call(xd)
        assert y.requires_grad and torch.equal(y.detach(), call(xd.detach()))                        # the plain route's bits
        (g,) = torch.autograd.grad(y.sum(), xd)
        err = _normwise(g, want)
        print("%s db=%s: gradient normwise %.2e" % (name, db, err))
        assert g.shape == xd.shape and err < C.TOL
        assert int((g != 0).sum()) <= x.shape[0] * h.shape[1]                                          # +0 elsewhere
        # the op, with weights from above
        wts = torch.tensor([0.5, -2.0, 3.0], device=dev)
        peak = A.autograd.TruePeakFunction.apply(xd, m.taps, db)
        (g2,) = torch.autograd.grad((peak * wts).sum(), xd)
        assert _normwise(g2, want * wts.cpu().numpy()[:, None]) < C.TOL


def test_gradient_through_programme_and_loudness_normalize(dev):
    table, x = C.case("spot/tile edge")
    h = C.tables()[table]
    m = A.TruePeak().to(dev)
    value, want = _autograd_reference(x, h, True, programme=True)
    xd = _dev(x, dev)[None].requires_grad_()                                 # (1, 3, L): three channels
    (g,) = torch.autograd.grad(m.programme(xd).sum(), xd)
    assert _normwise(g[0], want) < C.TOL
    # LoudnessNormalize with a binding limit: y = x 10^((limit - programme(x)) / 20), against float64 autograd of the same
    sr = 8000
    rng = np.random.default_rng(5)
    clip = (1e-3 * rng.standard_normal((2, 2, sr))).astype(np.float32)
    clip[0, 0, 3000:3002], clip[0, 1, 5000], clip[1, 1, 100:102], clip[1, 0, 7000] = (0.5, 0.25), -0.3, (-0.4, -0.2), 0.2
    cref = C.measure(clip, h)                                                # the louder channel of each clip, and its margin
    assert cref["margin"][0, 0] >= C.MARGIN and cref["margin"][1, 1] >= C.MARGIN
    assert cref["peak"][0, 0] > 1.1 * cref["peak"][0, 1] and cref["peak"][1, 1] > 1.1 * cref["peak"][1, 0]
    norm = A.LoudnessNormalize(target=-23.0, sr=sr, peak_limit=-1.0).to(dev)
    cd = _dev(clip, dev).requires_grad_()
    out = norm(cd)
    assert bool((norm.gain(cd.detach()) < A.LoudnessNormalize(target=-23.0, sr=sr).to(dev).gain(cd.detach())).all())   # it binds
    wts = _dev(rng.standard_normal(clip.shape).astype(np.float32), dev)
    (g,) = torch.autograd.grad((out * wts).sum(), cd)
    xt = torch.from_numpy(clip.astype(np.float64)).requires_grad_()
    w = torch.from_numpy(h.astype(np.float64)).flip(-1)[:, None, :]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(xt.reshape(4, 1, sr), (11, 0)), w).abs().amax(dim=(1, 2)).reshape(2, 2)
    gain = torch.pow(10.0, (-1.0 - 20.0 * torch.log10(y.amax(-1))) / 20.0)
    (want,) = torch.autograd.grad((xt * gain[:, None, None] * wts.double().cpu()).sum(), xt)
    err = _normwise(g, want.numpy())
    print("LoudnessNormalize(peak_limit=-1) gradient normwise %.2e" % err)
    assert err < C.TOL
    detached = A.LoudnessNormalize(target=-23.0, sr=sr, peak_limit=-1.0, detach_gain=True).to(dev)
    (gd,) = torch.autograd.grad((detached(cd) * wts).sum(), cd)
    assert torch.allclose(gd, wts * detached.gain(cd.detach())[:, None, None], rtol=1e-6, atol=0.0)  # both factors constants


def test_silent_rows_get_exactly_zero_and_second_order_raises(dev):
    m = A.TruePeak().to(dev)
    _, x = C.case("spot/early")
    x = x.copy()
    x[1] = 0.0
    for call in (m, m.linear, m.programme):
        xd = _dev(x, dev).requires_grad_()
        y = call(xd) if call is not m.programme else call(xd[:, None, :])
        (g,) = torch.autograd.grad(torch.where(torch.isinf(y), torch.zeros_like(y), y).sum(), xd)
        assert not bool(g[1].any()) and not bool(torch.signbit(g[1]).any()) and bool(g[0].any())
        assert bool(torch.isfinite(g).all())
    xd = _dev(x, dev).requires_grad_()
    y = m(xd)
    y.backward(torch.full_like(y, float("inf")))                             # +0 by selection, whatever arrives from above
    assert not bool(xd.grad[1].any()) and not bool(torch.isnan(xd.grad[1]).any())
    nan = _dev(x, dev)
    nan[2, 50] = float("nan")
    nan.requires_grad_()
    m.linear(nan).sum().backward()
    assert not bool(nan.grad[2].any()) and bool(nan.grad[0].any())           # a NaN row: +0 as well
    for call in (m, m.linear, A.LoudnessNormalize(sr=8000, peak_limit=-1.0).to(dev)):
        with pytest.raises(RuntimeError):                                    # first order only
            xr = _dev(np.tile(x, (1, 2)), dev).requires_grad_()
            (g,) = torch.autograd.grad(call(xr).sum(), xr, create_graph=True)
            g.sum().backward()


# ---- LoudnessNormalize(peak_limit=...) -----------------------------------------------------------------------------------------

def test_loudness_normalize_peak_limit(dev):
    sr = 8000
    rng = np.random.default_rng(6)
    peaky = (1e-3 * rng.standard_normal((2, 2, 2 * sr))).astype(np.float32)                          # quiet, with a few spikes
    peaky[0, 0, 3000:3002], peaky[0, 1, 9000], peaky[1, 1, 100:102], peaky[1, 0, 7000] = (0.5, 0.25), -0.3, (-0.4, -0.2), 0.2
    xd = _dev(peaky, dev)
    plain, lim = A.LoudnessNormalize(target=-23.0, sr=sr).to(dev), A.LoudnessNormalize(target=-23.0, sr=sr, peak_limit=-1.0).to(dev)
    meter = A.TruePeak(sr=sr).to(dev)
    over = meter.programme(plain(xd))
    assert bool((over > 0.0).all())                                          # without the limit: over full scale
    got = meter.programme(lim(xd))
    print("programme true peak after LoudnessNormalize(peak_limit=-1):", got.tolist(), "without:", over.tolist())
    assert bool((got <= -1.0 + 1e-3).all()) and bool((got >= -1.0 - 1e-3).all())
    # a clip whose limit does not bind: the bits of the module without the argument
    steady = (0.05 * rng.standard_normal((2, 2, 2 * sr))).astype(np.float32)
    sd = _dev(steady, dev)
    assert bool((meter.programme(plain(sd)) < -1.0).all())
    assert torch.equal(lim(sd), plain(sd)) and torch.equal(lim.gain(sd), plain.gain(sd))
    # silence keeps gain 1 under a limit too
    assert torch.equal(lim(torch.zeros(1, 2, sr, device=dev)), torch.zeros(1, 2, sr, device=dev))


# ---- error paths -----------------------------------------------------------------------------------------------------------

def test_error_paths(dev):
    m, rt = A.TruePeak().to(dev), A.RealtimeTruePeak().to(dev)
    x = torch.zeros(2, 2, 100, device=dev)
    for call in (m, m.linear, m.programme, m.sample_peak, m.index, rt):
        with pytest.raises(A.AcidsHipError):                                 # float64 without the opt-in
            call(x.double())
        with pytest.raises(A.AcidsHipError):                                 # a CPU tensor
            call(x.cpu())
        with pytest.raises(ValueError):                                      # a scalar
            call(torch.tensor(1.0, device=dev))
    assert rt.samples_seen == 0                                              # nothing was touched
    with A.allow_fp64_narrowing():
        assert torch.equal(m(x.double() + 0.25), m(x + 0.25)) and torch.equal(rt(x.double() + 0.25), m(x + 0.25))
    taps = m.taps
    state = torch.zeros(2, 2, 11, device=dev)
    peak, index = torch.zeros(2, 2, device=dev), torch.zeros(2, 2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.true_peak_stream(x, taps, state, state, peak, index, 0)          # the next state needs its own buffer
    with pytest.raises(ValueError):
        ops.true_peak_stream(x[..., :0], taps, state, state.clone(), peak, index, 0)
    with pytest.raises(ValueError):
        ops.true_peak_stream(x, taps, state[..., :10], state.clone(), peak, index, 0)
    with pytest.raises(ValueError):
        ops.true_peak_stream(x, taps, state, state.clone(), peak.double(), index, 0)
    with pytest.raises(ValueError):
        ops.true_peak(x, torch.zeros(9, 4, device=dev))
    with pytest.raises(ValueError):
        ops.true_peak(x, torch.zeros(12, device=dev))
    with pytest.raises(A.AcidsHipError):
        ops.true_peak(x, taps.cpu())
    with pytest.raises(ValueError):
        ops.true_peak_backward(peak, peak, index[0], taps, 100)

"""GPU side of gated loudness (ops.sos_hop_power / ops.loudness / ops.loudness_blocks, autograd.LoudnessFunction /
LoudnessBlocksFunction, transforms.Loudness / LoudnessNormalize; csrc/sos_filter.hip's hop endings and csrc/loudness.hip)
against the float64 oracle of loudness_cases.py: hop powers within the library's normwise bound 1e-5 for the six filters of
sos_filter_cases.py at every hop and length around the tile cuts, loudness and block loudness within 1e-4 LU on the planted
clips (every one at least 1 dB from both gates), gradients normwise below 1e-5 against the analytic gradient, the adjoint
identity of the scaled filter and its reverse, and the fixed points: bits that do not depend on the batch, -inf and an
exactly zero gradient for silence, a NaN that stays in its clip.

Measured on an MI355X (worst figures, printed by the tests): see README, "Loudness"."""
import math

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import loudness_cases as C
import sos_filter_cases as S
from acids_transforms_amd import ops
from acids_transforms_amd.autograd import LoudnessFunction
from acids_transforms_amd.utils import filter_design as fd

pytestmark = pytest.mark.gpu
IDENTITY = [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _lu_error(got, ref_lufs, ref_p):
    """The worst distance in LU between block loudnesses; blocks below -100 LUFS in the reference are compared in power,
    against the power of -100 LUFS, on the same scale (1e-4 LU is a relative 2.3e-5)."""
    got, ref_lufs, ref_p = np.asarray(got, np.float64), np.asarray(ref_lufs), np.asarray(ref_p)
    silent = ref_p == 0.0
    assert np.array_equal(np.isneginf(got), silent)
    loud = ~silent & (ref_lufs >= -100.0)
    quiet = ~silent & ~loud
    worst = float(np.abs(got[loud] - ref_lufs[loud]).max()) if loud.any() else 0.0
    if quiet.any():
        floor = 10.0 ** ((-100.0 + 0.691) / 10.0)
        rel = np.abs(10.0 ** ((got[quiet] + 0.691) / 10.0) - ref_p[quiet]) / floor
        worst = max(worst, float(10.0 * np.log10(1.0 + rel.max())))
    return worst


# ---- the hop powers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
def test_hop_power_matches_the_float64_filter(dev, name):
    """Every hop of the table at lengths around the tile cuts, 70 rows; in the same loop a row alone has the bits it has in
    batches of 3 and 70, and a hop longer than the row gives an empty result."""
    sos = S.FILTERS[name]
    tile, per_lane, _ = ops.sos_hop_power_plan(S.ROWS, 1, sos.shape[0], 16)
    assert (tile, per_lane) == (C.TILE, 16)
    worst = 0.0
    for L in C.PARITY_LENGTHS:
        x = S.case(name, L)["x"]
        xd = _dev(x, dev)
        for hop in C.HOPS:
            got = ops.sos_hop_power(xd, sos, hop)
            assert got.shape == (S.ROWS, L // hop) and got.dtype == torch.float64
            if L // hop == 0:
                continue
            worst = max(worst, C.rel_max(got.cpu().numpy(), C.hop_power(sos, x, hop)))
            assert torch.equal(ops.sos_hop_power(xd[0].clone(), sos, hop), got[0])
            assert torch.equal(ops.sos_hop_power(xd[:3].clone(), sos, hop), got[:3])
    print("%s: hop power %.2e" % (name, worst))
    assert worst < C.TOL


def test_hop_power_lane_cuts_and_rows_past_the_grid(dev):
    """Short rows (one hop, the lane cuts), and 2100 rows of 4100 samples: the rows that persistent workgroups take in a
    second turn have the bits of a row alone."""
    sos = S.FILTERS["kweighting"]
    worst = 0.0
    for L in (16, 17, 31, 32, 33, 255, 256, 257):
        x = np.random.default_rng(L).standard_normal((5, L)).astype(np.float32)
        for hop in (16, 17):
            worst = max(worst, C.rel_max(ops.sos_hop_power(_dev(x, dev), sos, hop).cpu().numpy(), C.hop_power(sos, x, hop)))
    x = np.random.default_rng(2100).standard_normal((2100, 4100)).astype(np.float32)
    xd = _dev(x, dev)
    for hop in (17, 800, 4097):
        got = ops.sos_hop_power(xd, sos, hop)
        worst = max(worst, C.rel_max(got.cpu().numpy(), C.hop_power(sos, x, hop)))
        for r in (0, 2047, 2048, 2099):
            assert torch.equal(got[r], ops.sos_hop_power(xd[r].clone(), sos, hop)), (hop, r)
    print("lane cuts and 2100 rows: hop power %.2e" % worst)
    assert worst < C.TOL


def test_hop_power_fixed_points(dev):
    sos = S.FILTERS["cascade4"]
    L, hop = 2 * C.TILE + 5, 255
    x = _dev(S.case("cascade4", L)["x"][:3], dev)
    clean = ops.sos_hop_power(x, sos, hop)
    zeros = ops.sos_hop_power(torch.zeros(3, L, device=dev), sos, hop)
    assert bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any())             # +0
    n = C.TILE + 1000
    bad = x.clone()
    bad[1, n] = float("nan")
    got = ops.sos_hop_power(bad, sos, hop)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    assert torch.equal(got[1, :n // hop], clean[1, :n // hop]) and bool(torch.isnan(got[1, n // hop:]).all())
    # one pass-through section: the plain energy envelope
    plain = ops.sos_hop_power(x, IDENTITY, hop).cpu().numpy()
    x64 = x.cpu().numpy().astype(np.float64)
    want = (x64[:, :(L // hop) * hop].reshape(3, -1, hop) ** 2).sum(-1)
    assert C.rel_max(plain, want) < 1e-12
    # the scaled filter: w y, +0 past the last whole hop; with unit weights it is the filter itself up to that point
    w = torch.ones(3, L // hop, dtype=torch.float64, device=dev)
    u = ops.sos_filter_hop_scaled(x, sos, hop, w)
    y = ops.sos_filter(x, sos)
    cut = (L // hop) * hop
    assert torch.equal(u[:, :cut], y[:, :cut]) and bool((u[:, cut:] == 0).all()) and not bool(torch.signbit(u[:, cut:]).any())
    with pytest.raises(A.AcidsHipError):
        ops.sos_hop_power(x, sos, 15)
    with pytest.raises(A.AcidsHipError):
        ops.sos_filter_hop_scaled(x, sos, hop, w.float())
    with pytest.raises(ValueError):
        ops.sos_filter_hop_scaled(x, sos, hop, w[:, 1:])


# ---- loudness ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.PARITY)
def test_loudness_and_block_loudness_match_the_oracle(dev, name):
    x, ref = C.clips()[name], C.reference(name)
    assert ref["margin_db"] >= C.MARGIN_DB
    xd = _dev(x, dev)
    m = A.Loudness(sr=C.SR).to(dev)
    lufs = m(xd)
    assert lufs.shape == x.shape[:-2] and lufs.dtype == torch.float32
    got, want = lufs.cpu().numpy().astype(np.float64), ref["lufs"]
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    live = ~np.isneginf(want)
    worst = float(np.abs(got[live] - want[live]).max()) if live.any() else 0.0
    mom = m.momentary(xd)
    assert mom.shape == ref["p"].shape
    worst_mom = _lu_error(mom.cpu().numpy(), ref["blocks"], ref["p"])
    worst_st = 0.0
    if x.shape[-1] >= 30 * C.H:
        ref30 = C.reference(name, 30)
        st = m.short_term(xd)
        assert st.shape == ref30["p"].shape
        worst_st = _lu_error(st.cpu().numpy(), ref30["blocks"], ref30["p"])
    print("%s: integrated %.2e LU, momentary %.2e LU, short-term %.2e LU (margin %.2f dB)"
          % (name, worst, worst_mom, worst_st, ref["margin_db"]))
    assert max(worst, worst_mom, worst_st) < C.TOL_LU
    assert torch.equal(ops.loudness(xd, C.SR), lufs) and torch.equal(ops.loudness_blocks(xd, C.SR), mom)


def test_weights_mono_and_the_stats(dev):
    x = C.clips()["five"]
    xd = _dev(x, dev)
    G = (0.5, 1.0, 2.0, 0.0, 1.41)
    got = float(A.Loudness(sr=C.SR, channel_weights=G).to(dev)(xd))
    assert abs(got - float(C.loudness(x, C.SR, G))) < C.TOL_LU
    mono = C.clips()["L%d" % (4 * C.H)]                                  # (1, L)
    one = A.Loudness(sr=C.SR).to(dev)(_dev(mono[0], dev))
    assert one.shape == () and torch.equal(one, A.Loudness(sr=C.SR).to(dev)(_dev(mono, dev)))
    lufs, power, stats = ops.loudness(_dev(C.clips()["gated"], dev), C.SR, return_state=True)
    gate = C.gating(C.reference("gated")["p"])
    assert power.shape == (2, 30) and stats.shape == (3,) and float(stats[2]) == gate["N2"] == 10
    assert abs(float(stats[0]) / gate["Pabs"] - 1) < 3e-5 and abs(float(stats[1]) / gate["P"] - 1) < 3e-5


def test_bits_do_not_depend_on_the_batch(dev):
    """A clip alone against the clip in batches of 3, 6, 70 clips and 1050 clips (2100 rows: past the grid of both
    kernels), through every leading shape."""
    batch = C.clips()["batch"]
    m = A.Loudness(sr=C.SR).to(dev)
    full = _dev(batch, dev)
    alone, alone_mom = m(full[0].clone()), m.momentary(full[0].clone())
    ref = C.reference("batch")
    for lead in C.LEADS:
        x = _dev(C.take(batch, lead), dev)
        lufs, mom = m(x), m.momentary(x)
        assert lufs.shape == tuple(lead) and mom.shape == tuple(lead) + (4,)
        assert torch.equal(lufs.reshape(-1)[0], alone) and torch.equal(mom.reshape(-1, 4)[0], alone_mom)
        assert float(np.abs(lufs.cpu().numpy().astype(np.float64) - C.take(ref["lufs"], lead)).max()) < C.TOL_LU
    many = full[:, :, :4 * C.H + 1].repeat(15, 1, 1)                      # 1050 clips, 2100 rows
    lufs = m(many)
    each = m(full[:, :, :4 * C.H + 1].contiguous())
    assert lufs.shape == (1050,) and torch.equal(lufs, each.repeat(15))
    assert torch.equal(m.momentary(many)[1049], m.momentary(many[1049].clone()))


def test_silence_reads_minus_infinity_and_passes_exactly_nothing_back(dev):
    x = torch.zeros(2, 2, 5 * C.H, device=dev)
    x[1] = _dev(C.clips()["gated"][:, :5 * C.H], dev)
    xr = x.clone().requires_grad_()
    m = A.Loudness(sr=C.SR).to(dev)
    lufs = m(xr)
    assert float(lufs[0].detach()) == -math.inf and math.isfinite(float(lufs[1].detach()))
    # whatever arrives from above: a NaN for the silent clip is what 10 ** (-lufs / 20) hands back
    lufs.backward(torch.tensor([float("nan"), 1.0], device=dev))
    assert bool((xr.grad[0] == 0).all()) and not bool(torch.signbit(xr.grad[0]).any())
    assert bool(torch.isfinite(xr.grad[1]).all()) and float(xr.grad[1].abs().max()) > 0
    # momentary: silent blocks are -inf and pass nothing; the clip below the absolute gate has blocks and a gradient
    mom = m.momentary(xr)
    assert bool(torch.isneginf(mom[0]).all())
    (g,) = torch.autograd.grad(mom[1].sum(), xr)
    assert bool((g[0] == 0).all()) and bool(torch.isfinite(g).all())
    quiet = _dev(C.clips()["below gate"], dev).requires_grad_()
    lq = m(quiet)
    lq.backward()
    assert float(lq.detach()) == -math.inf and bool((quiet.grad == 0).all())
    # LoudnessNormalize keeps gain 1 on such clips, and its gradient stays finite
    n = A.LoudnessNormalize(-23.0, sr=C.SR).to(dev)
    xr2 = x.clone().requires_grad_()
    out = n(xr2)
    assert torch.equal(out[0], x[0])
    out.sum().backward()
    assert bool(torch.isfinite(xr2.grad).all()) and bool((xr2.grad[0] == 1).all())


def test_a_nan_stays_in_its_clip(dev):
    clean = np.stack([C.clips()["gated"]] * 3)
    bad = clean.copy()
    bad[1] = C.clips()["nan"]
    m = A.Loudness(sr=C.SR).to(dev)
    want, got = m(_dev(clean, dev)), m(_dev(bad, dev))
    assert math.isnan(float(got[1])) and torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    mom_want, mom_got = m.momentary(_dev(clean, dev)), m.momentary(_dev(bad, dev))
    assert torch.equal(mom_got[0], mom_want[0]) and torch.equal(mom_got[2], mom_want[2])
    first = 10000 // C.H                                                   # the NaN sits in hop 12
    assert torch.equal(mom_got[1, :first - 3], mom_want[1, :first - 3]) and bool(torch.isnan(mom_got[1, first:]).all())


def test_normalize_reaches_its_target(dev):
    m = A.Loudness(sr=C.SR).to(dev)
    for name, target in (("gated", -23.0), ("tech3341-3 short", -14.0), ("five", -30.0)):
        x = _dev(C.clips()[name], dev)
        y = A.LoudnessNormalize(target, sr=C.SR).to(dev)(x)
        assert y.shape == x.shape and abs(float(m(y)) - target) < 1e-3, name
    batch = _dev(C.take(C.clips()["batch"], (2, 3)), dev)
    y = A.LoudnessNormalize(-20.0, sr=C.SR).to(dev)(batch)
    assert float((m(y) + 20.0).abs().max()) < 1e-3
    y1 = A.LoudnessNormalize(-20.0, sr=C.SR).to(dev)(batch[0, 0, 0])       # one mono clip
    assert y1.shape == batch[0, 0, 0].shape and abs(float(m(y1)) + 20.0) < 1e-3
    y, time = A.LoudnessNormalize(-20.0, sr=C.SR).to(dev).forward_with_time(batch, torch.ones(2, 3, device=dev))
    assert torch.equal(time, torch.ones(2, 3, device=dev))


def test_both_routes_give_the_same_bits_and_first_order_only(dev):
    x = _dev(C.clips()["gated"], dev)
    m = A.Loudness(sr=C.SR).to(dev)
    plain = m(x)
    routed = m(x.clone().requires_grad_())
    assert plain.grad_fn is None and routed.grad_fn is not None and torch.equal(plain, routed.detach())
    with torch.no_grad():
        assert torch.equal(m(x.clone().requires_grad_()), plain)
    assert torch.equal(m.momentary(x), m.momentary(x.clone().requires_grad_()).detach())
    assert torch.equal(m.short_term(x), m.short_term(x.clone().requires_grad_()).detach())
    assert torch.equal(LoudnessFunction.apply(x.clone().requires_grad_(), C.SR, None).detach(), plain)
    y, time = m.forward_with_time(x, torch.ones(3, device=dev))
    assert torch.equal(y, plain) and torch.equal(time, torch.ones(3, device=dev))
    for call in (m, m.momentary, A.LoudnessNormalize(sr=C.SR).to(dev)):
        with pytest.raises(RuntimeError):                                  # first order only
            xr = x.clone().requires_grad_()
            (g,) = torch.autograd.grad(call(xr).sum(), xr, create_graph=True)
            g.sum().backward()
    with pytest.raises(A.AcidsHipError):
        m(x.double())
    with A.allow_fp64_narrowing():
        assert torch.equal(m(x.double()), plain)


# ---- gradients -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["gated", "tech3341-3 short", "five", "batch3"])
def test_gradients_match_the_analytic_gradient(dev, name):
    x = C.take(C.clips()["batch"], (3,)) if name == "batch3" else C.clips()[name]
    lead = x.shape[:-2]
    rng = np.random.default_rng(17)
    g = rng.standard_normal(lead)
    xd = _dev(x, dev)
    m = A.Loudness(sr=C.SR).to(dev)
    worst = {}

    def grad_of(fn, upstream):
        xr = xd.clone().requires_grad_()
        out = fn(xr)
        (gx,) = torch.autograd.grad(out, xr, _dev(np.asarray(upstream, dtype=np.float32), dev).reshape(out.shape))
        assert gx.shape == xr.shape and gx.dtype == torch.float32
        return gx.cpu().numpy()

    g32 = g.astype(np.float32).astype(np.float64)
    worst["module"] = C.rel_max(grad_of(m, g32), C.loudness_gradient(x, C.SR, g=g32))
    worst["op"] = C.rel_max(grad_of(lambda t: LoudnessFunction.apply(t, C.SR, None), g32), C.loudness_gradient(x, C.SR, g=g32))
    for key, fn, hb in (("momentary", m.momentary, 4), ("short_term", m.short_term, 30)):
        if x.shape[-1] < hb * C.H:
            continue
        p = C.block_power(x, C.SR, hb)
        gl = rng.standard_normal(p.shape).astype(np.float32).astype(np.float64)
        gl = np.where(C.lufs_of(p) < -100.0, 0.0, gl)         # 1 / p of a block at -115 LUFS would set the scale alone
        worst[key] = C.rel_max(grad_of(fn, gl), C.blocks_gradient(x, C.SR, hb, gl))
    # LoudnessNormalize: y = x gain(x), gain = 10^((target - l) / 20): dL/dx = r gain - <r, x> gain ln10 / 20 dl/dx
    target = -20.0
    r = rng.standard_normal(x.shape).astype(np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    gain = 10.0 ** ((target - C.loudness(x, C.SR)) / 20.0)
    through = -(r * x64).sum((-2, -1)) * gain * math.log(10.0) / 20.0
    fixed = r * gain[..., None, None]
    full = fixed + C.loudness_gradient(x, C.SR, g=through)
    worst["normalize"] = C.rel_max(grad_of(A.LoudnessNormalize(target, sr=C.SR).to(dev), r), full)
    worst["normalize detached"] = C.rel_max(grad_of(A.LoudnessNormalize(target, sr=C.SR, detach_gain=True).to(dev), r), fixed)
    print("%s: %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) < C.TOL, worst


def test_scaled_filter_and_reverse_filter_are_adjoint(dev):
    """<J v, g> against <v, J^T g> for the linear part of the backward, J = W K (the K-weighting filter, then the hop
    weights) and J^T = K^T W, within 1e-6 of sum |.||.|."""
    sos = fd.k_weighting(C.SR)
    rng = np.random.default_rng(23)
    worst = 0.0
    for L, hop in ((2 * C.TILE + 5, 800), (C.TILE + 1, 17), (3 * C.TILE, 4097)):
        v = _dev(rng.standard_normal((3, L)).astype(np.float32), dev)
        g = _dev(rng.standard_normal((3, L)).astype(np.float32), dev)
        w = _dev(rng.standard_normal((3, L // hop)), dev)
        Jv = ops.sos_filter_hop_scaled(v, sos, hop, w)
        JTg = ops.sos_filter(ops.sos_filter_hop_scaled(g, IDENTITY, hop, w), sos, reverse=True)
        a, b = (Jv.double() * g.double()).sum(), (v.double() * JTg.double()).sum()
        scale = (Jv.double().abs() * g.double().abs()).sum()
        worst = max(worst, float((a - b).abs() / scale))
    print("adjoint identity: %.2e" % worst)
    assert worst < 1e-6

"""CPU side of the streaming R128 meter and of loudness range (ops.sos_hop_power_stream, ops.loudness_stream_plan,
ops.loudness_range, transforms.RealtimeLoudness; at_sos_hop_power_stream of csrc/sos_filter.hip, at_loudness_gate_ld and
at_loudness_range of csrc/loudness.hip): the oracle's own facts -- chunked sosfilt is the whole-signal call, the range
oracle reads EBU Tech 3342's cases, every parity clip keeps its margin -- the host plan against a brute-force count, the
ABI's argument checks, the names in the header, the binding and the documents, the module's surface and its state_dict
round trip, and the errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy.signal import sosfilt

import acids_transforms_amd as A
import loudness_cases as C
import loudness_stream_cases as S
from acids_transforms_amd import _lib, ops
from acids_transforms_amd.utils import filter_design as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle ----------------------------------------------------------------------------------------------------------

def test_chunked_sosfilt_is_the_whole_signal_call():
    sos = fd.k_weighting(S.SR)
    chunks = [1, 799, 800, 4095, 4097, 3, 20000]
    x = C._noise(3, (2, sum(chunks))).astype(np.float64)
    y, zi, at = sosfilt(sos, x, axis=-1), np.zeros((2, 2, 2)), 0
    for n in chunks:
        got, zi = sosfilt(sos, x[:, at:at + n], axis=-1, zi=zi)
        assert np.array_equal(got, y[:, at:at + n])
        at += n
    out = S.stream(sos, x, chunks, S.H)
    nh = sum(chunks) // S.H
    assert out["power"].shape == (2, nh) and out["seen"] == sum(chunks)
    assert C.rel_max(out["power"], C.hop_power(sos, x, S.H)) < 1e-14
    assert C.rel_max(out["open"], (y[:, nh * S.H:] ** 2).sum(-1)) < 1e-14
    # nothing completes: the open sum grows; a chunk that closes a hop exactly leaves +0
    p, o, _ = S.stream_step(sos, x[:, :10], 16, 3, None, np.array([1.0, 2.0]))
    assert p.shape == (2, 0) and np.all(o > np.array([1.0, 2.0]))
    p, o, _ = S.stream_step(sos, x[:, :13], 16, 3)
    assert p.shape == (2, 1) and np.array_equal(o, np.zeros(2))


@pytest.mark.parametrize("case", sorted(S.TECH3342))
def test_range_oracle_reads_tech_3342(case):
    levels, expected = S.TECH3342[case]
    x = S.tech3342(levels, (20,) * len(levels))
    got = float(S.loudness_range(x, S.SR))
    print("Tech 3342 case %d: %.4f LU (expected %.0f)" % (case, got, expected))
    assert abs(got - expected) < (1.0 if case == 4 else 1e-3)           # the standard's own tolerance is +-1 LU


def test_margins_and_planted_figures():
    margins = S.assert_margins()
    print({k: round(v, 2) for k, v in margins.items()})
    gated = S.range_reference("range gated")[0]
    assert C.block_power(S.clip("range gated"), S.SR, 30).shape == (111,)
    assert (gated["N1"], gated["n"]) == (100, 79) and abs(gated["lra"] - 15.124) < 1e-3
    assert abs(S.range_reference("case1 8+8")[0]["lra"] - 10.0) < 1e-4
    assert abs(S.range_reference("case3 8+8")[0]["lra"] - 20.0) < 1e-4
    # case 4 cannot keep the margin (its transition blocks sweep through the relative gate): oracle only
    x = S.tech3342(S.TECH3342[4][0], (20,) * 5)
    assert S.range_of(C.block_power(x, S.SR, 30))["margin_db"] < S.MARGIN_DB
    # the index rule
    assert [S.rnd(0.10 * (n - 1)) for n in (1, 2, 6, 7, 79)] == [0, 0, 1, 1, 8]
    assert [S.rnd(0.95 * (n - 1)) for n in (1, 2, 6, 7, 79)] == [0, 1, 5, 6, 74]
    assert S.range_of(np.zeros(5))["lra"] == 0.0 and np.isnan(S.range_of(np.array([1.0, np.nan, 2.0]))["lra"])


# ---- the host plan -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", (0, 1, 2))
def test_stream_plan_against_a_count(seed):
    rng = np.random.default_rng(seed)
    sr = (8000, 8004, 11025)[seed]
    seen = 0
    for n in [int(v) for v in rng.integers(0, 3 * C.hop_of(sr), 40)] + [0, 1, 35 * C.hop_of(sr)]:
        for hb in (4, 30):
            assert ops.loudness_stream_plan(sr, seen, n, hb) == S.plan(sr, seen, n, hb), (sr, seen, n, hb)
        seen += n
    for bad in (lambda: ops.loudness_stream_plan(8000, -1, 5), lambda: ops.loudness_stream_plan(8000, 0, -5),
                lambda: ops.loudness_stream_plan(8000, 0, 5, 0), lambda: ops.loudness_stream_plan(3000, 0, 5)):
        with pytest.raises(ValueError):
            bad()


# ---- the ABI -------------------------------------------------------------------------------------------------------------

def test_abi_argument_checks():
    lib = _lib.lib()
    sos = ops.sos_coefficients(fd.k_weighting(48000))
    buf = np.zeros(64)
    one = ctypes.c_void_p(buf.ctypes.data)
    w = np.ones(2)
    wp = ctypes.c_void_p(w.ctypes.data)
    thr = ops.LOUDNESS_ABS_THRESHOLD

    def stream(x=one, rows=1, n=100, sosp=sos.ptr, ns=2, hop=16, filled=0, zi=None, zf=one, oi=None, oo=one, power=one, ld=8,
               first=0):
        return lib.at_sos_hop_power_stream(x, rows, n, sosp, ns, hop, filled, zi, zf, oi, oo, power, ld, first, None)
    assert stream(rows=0) == 0                                           # no launch
    for kw in (dict(x=None), dict(sosp=None), dict(zf=None), dict(oo=None), dict(power=None), dict(rows=-1), dict(n=-1),
               dict(n=0), dict(hop=0), dict(filled=-1), dict(filled=16), dict(ld=6, first=1), dict(ld=5), dict(first=-1),
               dict(ld=-1), dict(ns=0), dict(zi=ctypes.c_void_p(buf.ctypes.data + 4))):
        assert stream(**{"rows": 0, **kw}) == -1, kw
    assert stream(rows=0, n=100, ld=6) == 0                              # done = 6 fits ld = 6
    assert stream(rows=0, hop=15) == _lib.AT_EUNSUPPORTED
    assert stream(rows=0, ns=17) == _lib.AT_EUNSUPPORTED

    def gate(power=one, clips=0, C_=2, nh=30, ld=30, hop=800, hb=4, weights=wp, lufs=one, stats=one, blocks=None):
        return lib.at_loudness_gate_ld(power, clips, C_, nh, ld, hop, hb, weights, thr, 0.1, lufs, stats, blocks, None)
    assert gate() == 0 and gate(ld=1024) == 0
    for kw in (dict(ld=29), dict(weights=None), dict(C_=0), dict(hb=0), dict(hop=0), dict(lufs=None, stats=None),
               dict(stats=None), dict(nh=-1, ld=0)):
        assert gate(**kw) == -1, kw
    assert gate(C_=33) == _lib.AT_EUNSUPPORTED and gate(hb=4097) == _lib.AT_EUNSUPPORTED
    assert gate(power=None, clips=1) == -1

    def rng(power=one, clips=0, C_=2, nh=40, ld=40, hop=800, hb=30, weights=wp, ratio=0.01, lra=one, stats=one, work=one):
        return lib.at_loudness_range(power, clips, C_, nh, ld, hop, hb, weights, thr, ratio, lra, stats, work, None)
    assert rng() == 0 and rng(ld=1024) == 0
    for kw in (dict(ld=39), dict(weights=None), dict(C_=0), dict(hb=0), dict(hop=0), dict(lra=None), dict(stats=None),
               dict(ratio=float("nan")), dict(ratio=-1.0), dict(power=None, clips=1), dict(work=None, clips=1)):
        assert rng(**kw) == -1, kw
    assert rng(C_=33) == _lib.AT_EUNSUPPORTED
    assert lib.at_abi_version() == _lib.ABI_VERSION


def test_names_in_header_binding_and_documents():
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ("at_sos_hop_power_stream", "at_loudness_gate_ld", "at_loudness_range"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols()
    for op in ("sos_hop_power_stream", "loudness_stream_plan", "loudness_range", "loudness_range_from_power"):
        assert op in dir(ops)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("RealtimeLoudness", "at_sos_hop_power_stream", "at_loudness_gate_ld", "at_loudness_range", "loudness_range"):
        assert name in integration, name
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "RealtimeLoudness" in text and "at_loudness_range" in text, doc
    assert "RealtimeLoudness" in A.transforms.__all__ and "RealtimeLoudness" in A.loudness.__all__
    assert A.RealtimeLoudness is A.transforms.RealtimeLoudness is A.loudness.RealtimeLoudness


# ---- the module ----------------------------------------------------------------------------------------------------------

def test_module_surface():
    m = A.RealtimeLoudness(sr=48000, channel_weights=(1.0, 0.5))
    assert isinstance(m, A.Loudness) and issubclass(A.RealtimeLoudness, A.AudioTransform)
    assert repr(m) == "RealtimeLoudness(sr=48000, channel_weights=(1.0, 0.5))"
    assert not m.invertible and not m.scriptable and m.latency == 0 and m.samples_seen == 0 and m.hops == 0
    assert m.realtime() is m and m.streaming() is m
    sd = m.state_dict()
    assert set(sd) == {"filter_state", "open_power", "hop_power", "_extra_state"}
    assert sd["_extra_state"] == {"samples_seen": 0}
    for name, tail in (("filter_state", (2, 2)), ("open_power", ()), ("hop_power", (1024,))):
        assert sd[name].dtype == torch.float64 and tuple(sd[name].shape) == tail == m._carried_tail(name)
        assert not bool(sd[name].any())
    assert m.hop_power.shape[-1] == 1024                                 # cap
    # before the first chunk: -inf, nothing, 0
    assert m.momentary().item() == float("-inf") == m.short_term().item() == m.integrated().item()
    assert m.block_loudness().shape == (0,) and m.loudness_range().item() == 0.0
    # Loudness: streaming() is the meter, realtime() still warns and returns the offline module
    off = A.Loudness(sr=48000, channel_weights=(1.0, 0.5))
    rt = off.streaming()
    assert isinstance(rt, A.RealtimeLoudness) and rt.sr == 48000 and rt.channel_weights == (1.0, 0.5)
    with pytest.warns(UserWarning, match="streaming"):
        assert off.realtime() is off
    assert off.state_dict() == {}
    y, time = m.forward_with_time(torch.zeros(2, 0), torch.ones(3))
    assert y.shape == (0,) and torch.equal(time, torch.ones(3)) and m.samples_seen == 0       # an empty chunk: no launch
    assert callable(m.test_forward) and callable(A.RealtimeLoudness.test_scripted_transform)
    with pytest.raises(A.NotInvertibleError):
        m.invert(torch.zeros(3))
    with pytest.raises(ValueError):
        A.RealtimeLoudness(sr=3000)


def test_state_dict_round_trip_on_another_batch_shape():
    m = A.RealtimeLoudness(sr=8000)
    g = torch.Generator().manual_seed(0)
    state = {"filter_state": torch.randn(3, 2, 2, 2, generator=g, dtype=torch.float64),
             "open_power": torch.rand(3, 2, generator=g, dtype=torch.float64),
             "hop_power": torch.rand(3, 2, 2048, generator=g, dtype=torch.float64),
             "_extra_state": {"samples_seen": 1234567}}
    m.load_state_dict(state, strict=True)
    assert m.samples_seen == 1234567 and m.hops == 1543 and m._carried_tail("hop_power") == (2048,)
    for k in ("filter_state", "open_power", "hop_power"):
        assert torch.equal(getattr(m, k), state[k]) and getattr(m, k).dtype == torch.float64
    again = A.RealtimeLoudness(sr=8000)
    again.load_state_dict(m.state_dict(), strict=True)
    assert again.get_extra_state() == {"samples_seen": 1234567} and torch.equal(again.hop_power, state["hop_power"])
    # a float32 entry comes back float64; reset() zeroes in place of the current shape and forgets the count
    half = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in state.items()}
    again.load_state_dict(half)
    assert again.hop_power.dtype == torch.float64 and torch.equal(again.hop_power, state["hop_power"].float().double())
    again.reset()
    assert again.samples_seen == 0 and again.hop_power.shape == (3, 2, 2048) and not bool(again.hop_power.any())
    assert not bool(again.filter_state.any()) and not bool(again.open_power.any())


def test_errors_that_need_no_device():
    m, x = A.RealtimeLoudness(sr=8000), torch.zeros(2, 4 * S.H)
    off = A.Loudness(sr=8000)
    zi, op, hist = torch.zeros(2, 2, 2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.float64)
    sos = fd.k_weighting(8000)
    for call in (lambda: m(x), lambda: off.loudness_range(torch.zeros(2, 30 * S.H)), lambda: ops.loudness_range(torch.zeros(2, 30 * S.H), 8000),
                 lambda: ops.sos_hop_power_stream(x, sos, 800, 0, zi, op, hist, 0),
                 lambda: ops.loudness_range_from_power(torch.zeros(2, 40, dtype=torch.float64), 40, 8000),
                 lambda: ops.sos_hop_power_stream(x, sos, 800, 0, zi.float(), op, hist, 0)):       # a float32 state
        with pytest.raises(A.AcidsHipError):
            call()
    assert m.samples_seen == 0 and m.hop_power.shape == (1024,)         # a refused chunk leaves the state alone
    with pytest.raises(A.AcidsHipError, match="float64"):
        m(x.double())
    with pytest.raises(A.AcidsHipError, match="float64"):
        ops.loudness_range(torch.zeros(2, 30 * S.H, dtype=torch.float64), 8000)
    with pytest.raises(ValueError):
        off.loudness_range(torch.zeros(2, 30 * S.H - 1))                 # below one 3 s block
    with pytest.raises(ValueError):
        ops.loudness_range(torch.zeros(8, 30 * S.H), 8000)               # (batch, L) read as 8 channels
    with pytest.raises(ValueError):
        m(torch.zeros(()))
    for bad in (lambda: ops.sos_hop_power_stream(x, sos, 800, 800, zi, op, hist, 0),        # filled outside [0, hop)
                lambda: ops.sos_hop_power_stream(x, sos, 800, 0, zi, op, hist, 5),          # 5 + 4 hops past cap = 8
                lambda: ops.sos_hop_power_stream(x[:, :0], sos, 800, 0, zi, op, hist, 0),
                lambda: ops.sos_hop_power_stream(x, sos, 800, 0, zi[:1], op, hist, 0),
                lambda: ops.sos_hop_power_stream(x, sos, 800, 0, zi, op, hist.t().contiguous().t(), 0),
                lambda: ops.loudness_range_from_power(torch.zeros(2, 40, dtype=torch.float64), 41, 8000),
                lambda: ops.loudness_range_from_power(torch.zeros(2, 40), 40, 8000)):
        with pytest.raises(ValueError):
            bad()


"""Host side of gated loudness (no device): the float64 oracle of loudness_cases.py against the figures of ITU-R BS.1770 and
EBU Tech 3341, its analytic gradient against central differences, the gate counts and margins of the planted clips, the
plan routines, the ABI's argument checks, and every error of ops / transforms.Loudness that needs no GPU.

Measured with the oracle: a 0 dBFS 997 Hz sine at 48 kHz reads -3.0103 LKFS in one channel and +0.00003 in both of a stereo
clip; Tech 3341 cases 3 and 4 at full length read -23.014 LUFS both; the gradient agrees with central differences to 2e-8."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import loudness_cases as C
from acids_transforms_amd import _lib, ops
from acids_transforms_amd.utils import filter_design as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_reads_the_standards_sines():
    sr = 48000
    s = np.sin(2 * np.pi * 997.0 * np.arange(5 * sr) / sr)
    mono, stereo = float(C.loudness(s[None], sr)), float(C.loudness(np.stack([s, s]), sr))
    print("997 Hz 0 dBFS: one channel %.4f LKFS, both %.4f" % (mono, stereo))
    assert abs(mono - (-3.01)) <= 0.01
    assert abs(stereo) <= 0.01


def test_oracle_reads_tech_3341_cases_3_and_4():
    case3 = float(C.loudness(C._tech3341_3(48000, (10, 60, 10)), 48000))
    case4 = float(C.loudness(C._tech3341_3(48000, (10, 10, 10, 60, 10), (-72.0, -36.0, -54.0, -23.0, -36.0)), 48000))
    print("Tech 3341 case 3 %.4f LUFS, case 4 %.4f" % (case3, case4))
    assert abs(case3 - (-23.0)) <= 0.1 and abs(case4 - (-23.0)) <= 0.1


def test_analytic_gradient_matches_central_differences():
    sr, L = 4000, 4000 + 37
    rng = np.random.default_rng(0)
    x = 0.1 * rng.standard_normal((2, L))
    x[:, 2000:] *= 0.01                                   # the second half is gated out: the masks matter
    assert C.gating(C.block_power(x, sr))["N2"] < L // C.hop_of(sr) - 3
    grad, eps, worst = C.loudness_gradient(x, sr), 1e-6, 0.0
    for _ in range(4):
        v = rng.standard_normal(x.shape)
        numeric = float(C.loudness(x + eps * v, sr) - C.loudness(x - eps * v, sr)) / (2 * eps)
        worst = max(worst, abs(numeric - float((grad * v).sum())) / abs(numeric))
    # block loudness, on the loud half alone (a block at -75 LUFS has a 1 / p that central differences resolve badly)
    xb = x[:, :2000]
    g = rng.standard_normal(2000 // C.hop_of(sr) - 3)
    gb, v = C.blocks_gradient(xb, sr, 4, g), rng.standard_normal(xb.shape)
    numeric = float(((C.block_loudness(xb + eps * v, sr) - C.block_loudness(xb - eps * v, sr)) * g).sum()) / (2 * eps)
    worst_blocks = abs(numeric - float((gb * v).sum())) / abs(numeric)
    print("gradient against central differences: integrated %.2e, blocks %.2e" % (worst, worst_blocks))
    assert worst < 1e-6 and worst_blocks < 1e-6


def test_planted_clips_gate_as_planted_and_keep_their_margins():
    margins = C.assert_margins()
    assert set(margins) == set(C.PARITY) and set(C.PARITY) | {"nan"} == set(C.clips())         # no case is left out
    gated, tech = C.reference("gated"), C.reference("tech3341-3 short")
    assert gated["p"].shape == (27,) and gated["N1"] == [20] and gated["N2"] == [10]
    assert abs(float(gated["lufs"]) - (-15.47)) < 0.2                       # -15.5299 with this seed
    assert margins["gated"] > 7.0
    assert tech["p"].shape == (57,) and tech["N1"] == [57] and tech["N2"] == [43] and 1.0 < margins["tech3341-3 short"] < 2.0
    for name in ("silent", "below gate"):
        assert C.reference(name)["N1"] == [0] and C.reference(name)["lufs"] == -math.inf
    assert C.reference("silent")["blocks"][0] == -math.inf
    assert C.reference("five")["p"].shape == (3,) and math.isnan(float(C.reference("nan")["lufs"]))
    assert C.reference("batch")["lufs"].shape == (70,)
    assert C.reference("tech3341-3 short", 30)["p"].shape == (31,) and C.reference("gated", 30)["p"].shape == (1,)
    print("margins (dB):", {k: round(v, 2) for k, v in margins.items()})


def test_plans_answer_without_a_device():
    assert ops.sos_hop_power_plan(70, 5000, 2, 800) == ops.sos_filter_plan(70, 5000, 2) == (C.TILE, 16, 0)
    assert ops.SOS_MIN_HOP == 16 == ops.sos_hop_power_plan(1, 1, 1, 16)[1]
    for rows, L, hop in ((1, 1, 16), (3, 2 * C.TILE + 5, 4410), (2100, 4100, 17), (0, 0, 1 << 40)):
        assert ops.sos_hop_power_plan(rows, L, 16, hop)[2] == 0
    lib = _lib.lib()
    out = [ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)]
    refs = [ctypes.byref(v) for v in out]
    assert lib.at_sos_hop_power_plan(1, 100, 2, 15, *refs) == _lib.AT_EUNSUPPORTED
    assert lib.at_sos_hop_power_plan(1, 100, 17, 16, *refs) == _lib.AT_EUNSUPPORTED
    assert lib.at_sos_hop_power_plan(1, 100, 2, 0, *refs) == -1 == lib.at_sos_hop_power_plan(-1, 100, 2, 16, *refs)
    assert lib.at_sos_hop_power_plan(1, 100, 2, 16, None, refs[1], refs[2]) == -1
    plan = ops.loudness_plan((2, 3, 2, 3 * C.SR + 123), C.SR)
    assert (plan.hop, plan.hb, plan.nh, plan.nb, plan.clips, plan.C) == (800, 4, 30, 27, 6, 2)
    assert ops.loudness_plan((44100,), 44100).mono and ops.loudness_plan((44100,), 44100).hop == 4410
    assert abs(ops.LOUDNESS_ABS_THRESHOLD - C.ABS_THRESHOLD) == 0 and ops.LOUDNESS_REL_RATIO == C.REL_RATIO
    assert ops.LOUDNESS_CHANNEL_WEIGHTS == C.DEFAULT_WEIGHTS


def test_abi_argument_checks_touch_no_device():
    lib = _lib.lib()
    sos = np.ascontiguousarray(fd.k_weighting(48000))
    sp, one = ctypes.c_void_p(sos.ctypes.data), ctypes.c_void_p(8)        # `one`: a non-null, aligned stand-in, never read
    bad = sos.copy()
    bad[1, 3] = 2.0
    nonfinite = sos.copy()
    nonfinite[0, 0] = np.inf
    assert lib.at_sos_hop_power(one, 1, 100, sp, 2, 15, one, None) == _lib.AT_EUNSUPPORTED
    assert lib.at_sos_hop_power(one, 1, 100, sp, 17, 16, one, None) == _lib.AT_EUNSUPPORTED
    assert lib.at_sos_hop_power(one, 1, 100, None, 2, 16, one, None) == -1
    assert lib.at_sos_hop_power(one, -1, 100, sp, 2, 16, one, None) == -1
    assert lib.at_sos_hop_power(one, 1, 100, ctypes.c_void_p(bad.ctypes.data), 2, 16, one, None) == -1
    assert lib.at_sos_hop_power(one, 1, 100, ctypes.c_void_p(nonfinite.ctypes.data), 2, 16, one, None) == -1
    assert lib.at_sos_hop_power(None, 1, 100, sp, 2, 16, one, None) == -1 == lib.at_sos_hop_power(one, 1, 100, sp, 2, 16, None, None)
    assert lib.at_sos_hop_power(None, 0, 100, sp, 2, 16, None, None) == 0           # empty work
    assert lib.at_sos_hop_power(None, 5, 15, sp, 2, 16, None, None) == 0            # no whole hop
    assert lib.at_sos_filter_hop_scaled(one, 1, 100, sp, 2, 8, one, one, None) == _lib.AT_EUNSUPPORTED
    assert lib.at_sos_filter_hop_scaled(one, 1, 100, sp, 2, 16, None, one, None) == -1
    assert lib.at_sos_filter_hop_scaled(one, 1, 100, sp, 2, 16, one, None, None) == -1
    assert lib.at_sos_filter_hop_scaled(None, 0, 100, sp, 2, 16, None, None, None) == 0
    w = np.array([1.0, 1.0])
    wp = ctypes.c_void_p(w.ctypes.data)
    many = np.ones(33)
    infw = np.array([1.0, np.nan])
    thr, ratio = ops.LOUDNESS_ABS_THRESHOLD, ops.LOUDNESS_REL_RATIO
    assert lib.at_loudness_gate(None, 0, 2, 30, 800, 4, wp, thr, ratio, one, one, None, None) == 0
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 4, None, thr, ratio, one, one, None, None) == -1
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 4, ctypes.c_void_p(infw.ctypes.data), thr, ratio, one, one, None, None) == -1
    assert lib.at_loudness_gate(one, 1, 33, 30, 800, 4, ctypes.c_void_p(many.ctypes.data), thr, ratio, one, one, None, None) \
        == _lib.AT_EUNSUPPORTED
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 4097, wp, thr, ratio, one, one, None, None) == _lib.AT_EUNSUPPORTED
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 0, wp, thr, ratio, one, one, None, None) == -1
    assert lib.at_loudness_gate(one, 1, 2, 30, 0, 4, wp, thr, ratio, one, one, None, None) == -1
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 4, wp, thr, ratio, None, None, None, None) == -1     # nothing to write
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 4, wp, thr, ratio, one, None, None, None) == -1      # lufs without stats
    assert lib.at_loudness_gate(one, 1, 2, 30, 800, 4, wp, float("nan"), ratio, one, one, None, None) == -1
    assert lib.at_loudness_gate(None, 1, 2, 30, 800, 4, wp, thr, ratio, one, one, None, None) == -1
    assert lib.at_loudness_gate_backward(one, one, one, 0, 2, 30, 800, 4, wp, thr, ratio, one, None) == 0
    assert lib.at_loudness_gate_backward(one, None, one, 1, 2, 30, 800, 4, wp, thr, ratio, one, None) == -1
    assert lib.at_loudness_gate_backward(one, one, one, 1, 2, 30, 800, 4, wp, thr, ratio, None, None) == -1
    assert lib.at_loudness_blocks_backward(one, one, 0, 2, 30, 800, 4, wp, one, None) == 0
    assert lib.at_loudness_blocks_backward(one, None, 1, 2, 30, 800, 4, wp, one, None) == -1
    assert lib.at_loudness_blocks_backward(one, one, 1, 0, 30, 800, 4, wp, one, None) == -1
    assert lib.at_abi_version() == 4


def test_errors_that_need_no_device():
    x = torch.zeros(2, 4 * 4410)
    with pytest.raises(ValueError):
        A.Loudness(sr=3000)                                              # k_weighting's limit
    with pytest.raises(ValueError):
        A.LoudnessNormalize(sr=3000)
    with pytest.raises(ValueError):
        A.LoudnessNormalize(target=float("nan"))
    m = A.Loudness()
    with pytest.raises(ValueError):
        m(torch.zeros(8, 4 * 4410))                                      # (batch, L) read as 8 channels
    with pytest.raises(ValueError):
        m(torch.zeros(6, 2 * 4410))
    with pytest.raises(ValueError):
        A.Loudness(channel_weights=[1.0, 1.0, 1.0])(x)                   # three weights, two channels
    with pytest.raises(ValueError):
        ops.loudness(x, 44100, [1.0, float("inf")])
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4 * 4410 - 1))                                  # no block
    with pytest.raises(ValueError):
        m.short_term(x)                                                  # no 3 s block
    with pytest.raises(ValueError):
        ops.loudness_blocks(x, 44100, 0)
    with pytest.raises(ValueError):
        ops.loudness(torch.zeros(()), 44100)
    with pytest.raises(ValueError):
        ops.sos_hop_power(torch.zeros(()), fd.k_weighting(48000), 800)
    with pytest.raises(ValueError):
        ops.sos_hop_power(x, fd.k_weighting(48000), 0)
    with pytest.raises(A.AcidsHipError):
        ops.sos_hop_power_plan(1, 100, 2, 15)
    # the project's rules: no CPU route, no silent narrowing
    for call in (lambda: m(x), lambda: m.momentary(x), lambda: A.LoudnessNormalize()(x), lambda: ops.loudness(x, 44100),
                 lambda: ops.loudness_blocks(x, 44100), lambda: ops.sos_hop_power(x, fd.k_weighting(48000), 800),
                 lambda: ops.sos_filter_hop_scaled(x, fd.k_weighting(48000), 4410, torch.zeros(2, 4, dtype=torch.float64)),
                 lambda: m(x.clone().requires_grad_())):
        with pytest.raises(A.AcidsHipError):
            call()
    with pytest.raises(A.AcidsHipError, match="float64"):
        m(x.double())
    with pytest.raises(A.NotInvertibleError):
        m.invert(torch.zeros(3))
    with pytest.raises(A.NotInvertibleError):
        A.LoudnessNormalize().invert(x)
    assert A.Loudness(channel_weights=[1, 1, 1, 1, 1, 1]).channel_weights == (1.0,) * 6       # six channels, by request


def test_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_SO", os.path.join(ROOT, "no_such_dir", "libacids_hip.so"))
    with pytest.raises(A.AcidsHipError, match="missing"):
        ops.sos_hop_power_plan(1, 100, 2, 16)


def test_modules_surface_and_state_dict_round_trip():
    m, n = A.Loudness(sr=48000, channel_weights=(1.0, 0.5)), A.LoudnessNormalize(target=-16.0, sr=48000, detach_gain=True)
    assert not m.invertible and not n.invertible and not m.scriptable and not m.needs_scaling and m.ratio == 1
    assert repr(m) == "Loudness(sr=48000, channel_weights=(1.0, 0.5))"
    assert repr(n) == "LoudnessNormalize(target=-16.0, sr=48000, channel_weights=None, detach_gain=True)"
    assert isinstance(n, A.Loudness) and issubclass(A.Loudness, A.AudioTransform)
    # nothing learned, nothing carried: the state is empty, loads strictly, and survives a chain
    assert m.state_dict() == {} == n.state_dict()
    assert A.Loudness().load_state_dict(m.state_dict(), strict=True).missing_keys == []
    chain = A.SOSFilter(fd.highpass(48000, 20.0), sr=48000) + n
    loaded = A.SOSFilter(sr=48000) + A.LoudnessNormalize(sr=48000)
    loaded.load_state_dict(chain.state_dict())
    assert torch.equal(loaded[0].sos, chain[0].sos) and not chain.invertible
    with pytest.warns(UserWarning, match="streaming"):
        assert m.realtime() is m
    assert A.transforms.Loudness is A.Loudness and A.transforms.loudness.Loudness is A.Loudness and A.loudness is A.transforms.loudness
    assert "Loudness" in A.transforms.__all__ and "LoudnessNormalize" in A.transforms.__all__


def test_build_and_docs_name_the_new_kernels():
    mk = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "Makefile")).read()
    assert re.search(r"loudness\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk)
    assert re.search(r"sos_filter\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk)
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ("at_sos_hop_power_plan", "at_sos_hop_power", "at_sos_filter_hop_scaled", "at_loudness_gate",
                 "at_loudness_gate_backward", "at_loudness_blocks_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Loudness" in integration and "LoudnessNormalize" in integration

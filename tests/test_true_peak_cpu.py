"""Host side of the true-peak measure (no GPU): the BS.1770-4 table and the Kaiser designs of
utils.filter_design.true_peak_filter, the float64 oracle of true_peak_cases.py on the five true-peak signals of EBU Tech
3341, the plan of at_true_peak held on the host (so that the GPU cases really sit at tile - 1, tile, tile + 1 ...), the
margins of every planted input, the AT_EINVAL / AT_OK answers that touch no device, and the Python surface.

Measured passband of the Kaiser designs (beta = 5, gain below 0.4 x the input rate relative to DC, lowest .. highest, dB):
(2, 12) -0.391 .. +0.018, (2, 16) -0.035 .. +0.019, (4, 12) -0.351 .. +0.020, (8, 7) -1.615 .. +0.005, (8, 12) -0.332 ..
+0.021; the standard's own (4, 12) table -0.111 .. +0.101.  The droop is the price of K taps per phase: (8, 7) is a short
filter and reads up to 1.6 dB low near 0.4 fs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import true_peak_cases as C
from acids_transforms_amd import _lib, autograd, ops
from acids_transforms_amd.utils import filter_design as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables ----------------------------------------------------------------------------------------------------------

def test_default_table_is_the_standards_integers_over_8192():
    h = fd.true_peak_filter()
    assert h.dtype == np.float64 and h.shape == (4, 12)
    a, b = (np.array(r, dtype=np.float64) for r in C.BS1770_INTEGERS)
    assert np.array_equal(h * 8192.0, np.stack([a, b, b[::-1], a[::-1]]))
    assert np.array_equal(h.astype(np.float32).astype(np.float64), h)            # every entry is exact in float32
    g = h.T.reshape(-1)                                                          # the 48-tap prototype g[4 k + p] = h[p][k]
    assert np.array_equal(g, g[::-1])
    assert np.array_equal(h.sum(axis=1) * 8192.0, [8205.0, 7971.0, 7971.0, 8205.0])
    assert np.array_equal(fd.true_peak_filter(4, 12, "bs1770"), h)


@pytest.mark.parametrize("P,K", [(2, 4), (2, 12), (2, 16), (4, 12), (8, 7), (8, 12), (4, 64)])
def test_kaiser_designs(P, K):
    h = fd.true_peak_filter(P, K, "kaiser")
    assert h.dtype == np.float64 and h.shape == (P, K)
    assert np.abs(h.sum(axis=1) - 1.0).max() < 1e-12                             # unity DC gain per phase
    g = h.T.reshape(-1)
    if P * K % 2 == 0:
        assert np.abs(h[0] - h[P - 1][::-1]).max() < 1e-12                       # mirrored phases: a symmetric prototype
    assert int(np.abs(g).argmax()) in (P * K // 2 - 1, P * K // 2)


def test_kaiser_passband_ripple_is_what_the_docstring_says():
    quoted = {(2, 12): (-0.391, 0.018), (2, 16): (-0.035, 0.019), (4, 12): (-0.351, 0.020), (8, 7): (-1.615, 0.005),
              (8, 12): (-0.332, 0.021)}
    for (P, K), (lo, hi) in quoted.items():
        got = C.passband_ripple(fd.true_peak_filter(P, K, "kaiser"))
        print("kaiser (%d, %d): %.4f .. %+.4f dB below 0.4 fs" % (P, K, got[0], got[1]))
        assert abs(got[0] - lo) < 1e-3 and abs(got[1] - hi) < 1e-3, (P, K, got)
    got = C.passband_ripple(fd.true_peak_filter())
    assert abs(got[0] + 0.111) < 1e-3 and abs(got[1] - 0.101) < 1e-3, got


def test_filter_design_errors():
    for args in ((4, 11, "bs1770"), (2, 12, "bs1770"), (3, 12, "kaiser"), (1, 12, "kaiser"), (4, 3, "kaiser"), (4, 65, "kaiser"),
                 (4, 12, "remez"), (4.5, 12, "kaiser")):
        with pytest.raises(ValueError):
            fd.true_peak_filter(*args)
    assert "true_peak_filter" in fd.__all__


# ---- the oracle ----------------------------------------------------------------------------------------------------------

def test_oracle_is_numpy_convolve_per_phase():
    rng = np.random.default_rng(0)
    for name in C.TABLES:
        h = C.tables()[name].astype(np.float64)
        P, K = h.shape
        x = rng.standard_normal(200)
        ref = np.stack([np.convolve(x, h[p])[:200] for p in range(P)], axis=1).reshape(-1)
        assert np.abs(C.oversampled(x, h) - ref).max() < 1e-13
        # a stream: the state is the samples before the chunk
        cut = 77
        tail = C.oversampled(x[cut:], h, C.next_state(x[:cut], K))
        assert np.abs(tail - ref[P * cut:]).max() < 1e-13


@pytest.mark.parametrize("number", sorted(C.TECH3341))
def test_oracle_reads_tech3341_inside_its_tolerance(number):
    h = C.tables()["bs1770"]
    got = float(C.dbtp(C.measure(C.tech3341(number), h)["peak"]))
    expected = C.TECH3341[number][3]
    print("Tech 3341 case %d: %.3f dBTP (expected %.2f +0.2 / -0.4)" % (number, got, expected))
    assert expected - 0.4 <= got <= expected + 0.2
    assert abs(got - C.TECH3341_READINGS[number]) < 1e-3


def test_abrupt_onset_of_case_18_overshoots():
    """Without the fade the step at the onset of case 18 reads -5.32 dBTP: a property of the signal, not of the meter."""
    got = float(C.dbtp(C.measure(C.tech3341(18, fade=0), C.tables()["bs1770"])["peak"]))
    assert abs(got + 5.32) < 5e-3, got


# ---- the plan, and the inputs of the GPU tests -----------------------------------------------------------------------------

def test_plan_is_held_on_the_host():
    for name in C.TABLES:
        P, K = C.tables()[name].shape
        for L in C.lengths(K):
            tile, per_lane, launches, dispatch = ops.true_peak_plan(3, L, P, K)
            assert (tile, per_lane) == (C.TILE, C.PER_LANE) == (2048, 8)
            assert launches == (1 if L <= C.TILE else 2), (name, L)
            assert dispatch == (0 if (P, K) == (4, 12) else 1)
        assert sorted({1, K - 2, K - 1, K, C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + K - 2} - {0, -1}) == C.lengths(K)
    assert ops.true_peak_plan(0, 100, 4, 12)[2] == 0 and ops.true_peak_plan(5, 0, 4, 12)[2] == 0
    assert ops.true_peak_plan(C.MANY_ROWS, C.MANY_L, 4, 12)[2] == 1 and C.MANY_ROWS > 65535
    assert ops.true_peak_plan(1, 4 * C.TILE + 3, 4, 12)[2] == 2
    lib = _lib.lib()
    assert lib.at_true_peak_workspace_bytes(3, C.TILE, 4, 12) == 0
    assert lib.at_true_peak_workspace_bytes(3, C.TILE + 1, 4, 12) == 3 * 2 * 16
    assert lib.at_true_peak_workspace_bytes(1, 1 << 24, 4, 12) == (1 << 24) // C.TILE * 16
    for chunks in C.CHUNK_LISTS.values():
        assert all(1 <= n <= 2 * C.TILE + 9 for n in chunks)
    assert min(min(c) for c in C.CHUNK_LISTS.values()) == 1 and max(max(C.CHUNK_LISTS[k]) for k in ("seed 1", "seed 2", "seed 3")) <= C.TILE + 1
    assert any(n < 11 for n in C.CHUNK_LISTS["short then long"])                 # chunks shorter than K - 1


@pytest.mark.parametrize("name", C.all_cases())
def test_every_planted_case_keeps_its_margin(name):
    """The condition on the inputs that makes the index comparable: the top |y| at least 1e-3 relative above the runner-up."""
    ref = C.reference(name)
    assert float(ref["margin"].min()) >= C.MARGIN, (name, float(ref["margin"].min()))
    assert bool((ref["peak"] > 0).all())


def test_spots_are_where_they_claim():
    for spot, (table, rows, L, at, negative) in C.SPOTS.items():
        P, K = C.tables()[table].shape
        ref = C.reference("spot/" + spot)
        assert np.array_equal(ref["index"] // P, np.full(rows, at)), spot
        if negative:
            assert bool((ref["sign"] < 0).all())
    assert (C.reference("spot/negative")["sign"] < 0).all() and {-1.0, 1.0} == set(C.reference("spot/early")["sign"])
    assert C.SPOTS["early"][3] < 11 and C.SPOTS["last sample"][3] == C.LONG - 1
    assert C.SPOTS["wave end"][3] % (64 * C.PER_LANE) == 64 * C.PER_LANE - 1
    at = C.SPOTS["tile edge"][3]
    assert at - 11 < C.TILE <= at                                                  # the window straddles the edge
    for name, chunks in C.CHUNK_LISTS.items():                                     # what the stream tests compare by index
        x = C.stream_signal(sum(chunks))
        for table in ("bs1770", "kaiser 2x16"):
            ref = C.measure(x, C.tables()[table])
            assert x.shape == (2, 2, sum(chunks)) and float(ref["margin"].min()) >= C.MARGIN, (name, table)
    # the long row of the piece test
    for table in ("bs1770", "kaiser 2x16"):
        h = C.tables()[table]
        x = C.planted(h, 2, 4 * C.TILE + 3, np.array([3 * C.TILE + 1, 500]), 4)
        assert float(C.measure(x, h)["margin"].min()) >= C.MARGIN


def test_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_SO", os.path.join(ROOT, "no_such_dir", "libacids_hip.so"))
    with pytest.raises(A.AcidsHipError, match="missing"):
        ops.true_peak_plan(1, 100, 4, 12)


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------

def test_entries_answer_without_a_device():
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    one, two = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data + 64)

    def peak(x=one, rows=0, L=100, taps=one, P=4, K=12, si=None, so=None, pk=one, idx=None, sg=None, mp=None, mi=None, ws=None,
             nb=0):
        return lib.at_true_peak(x, rows, L, taps, P, K, si, so, pk, idx, sg, mp, mi, 0, ws, nb, None)
    assert peak() == 0 and peak(rows=5, L=0) == 0                            # empty work: no launch
    for kw in (dict(rows=-1), dict(L=-1), dict(P=0), dict(P=9), dict(K=0), dict(K=65)):
        assert peak(**kw) == _lib.AT_EINVAL, kw
    for kw in (dict(x=None), dict(taps=None), dict(pk=None), dict(pk=None, mi=one), dict(si=one, so=one), dict(K=1, P=1, si=one),
               dict(K=1, P=1, so=two), dict(x=ctypes.c_void_p(buf.ctypes.data + 2)), dict(idx=ctypes.c_void_p(buf.ctypes.data + 4))):
        assert peak(**{"rows": 1, **kw}) == _lib.AT_EINVAL, kw
    assert peak(rows=1, L=C.TILE + 1) == _lib.AT_EWORKSPACE                  # two tiles need the partials

    def back(g=one, sg=one, idx=one, taps=one, P=4, K=12, rows=0, L=100, gx=one):
        return lib.at_true_peak_backward(g, sg, idx, taps, P, K, rows, L, gx, None)
    assert back() == 0 and back(rows=3, L=0) == 0
    for kw in (dict(rows=-1), dict(L=-1), dict(P=0), dict(K=65)):
        assert back(**kw) == _lib.AT_EINVAL, kw
    for kw in (dict(g=None), dict(sg=None), dict(idx=None), dict(taps=None), dict(gx=None),
               dict(idx=ctypes.c_void_p(buf.ctypes.data + 4))):
        assert back(**{"rows": 1, **kw}) == _lib.AT_EINVAL, kw
    t = ctypes.c_int64(0)
    i = ctypes.c_int(0)
    assert lib.at_true_peak_plan(1, 1, 4, 12, None, ctypes.byref(t), ctypes.byref(i), ctypes.byref(i)) == _lib.AT_EINVAL
    assert lib.at_true_peak_plan(1, 1, 9, 12, ctypes.byref(t), ctypes.byref(t), ctypes.byref(i), ctypes.byref(i)) == _lib.AT_EINVAL
    assert lib.at_abi_version() == _lib.ABI_VERSION


def test_names_in_header_binding_makefile_and_documents():
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ("at_true_peak", "at_true_peak_plan", "at_true_peak_workspace_bytes", "at_true_peak_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
    mk = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "Makefile")).read()
    assert re.search(r"true_peak\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", mk)
    src = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "true_peak.hip")).read()
    assert "fmaxf" not in src and "atomic" not in src.replace("no atomics", "").replace("No float maximum, no atomics", "")
    for op in ("true_peak", "true_peak_plan", "true_peak_stream", "true_peak_backward"):
        assert op in dir(ops)
    assert "TruePeakFunction" in autograd.__all__ and issubclass(autograd.TruePeakFunction, torch.autograd.Function)
    for name in ("TruePeak", "RealtimeTruePeak"):
        assert name in A.transforms.__all__ and name in A.loudness.__all__
        assert getattr(A, name) is getattr(A.transforms, name) is getattr(A.loudness, name)
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "TruePeak" in text and "RealtimeTruePeak" in text and "at_true_peak" in text, doc
    for text in (open(os.path.join(ROOT, "README.md")).read(), A.loudness.__doc__):
        for m in re.finditer(r"Not built:([^.]*)\.", text):
            assert not re.match(r"\s*true peak,", m.group(1)), m.group(0)[:80]


# ---- the modules ---------------------------------------------------------------------------------------------------------------

def test_module_surface():
    m = A.TruePeak()
    assert isinstance(m, A.AudioTransform) and not m.invertible and not m.scriptable
    assert repr(m) == "TruePeak(sr=44100, oversample=4, taps_per_phase=12)"
    assert m.taps.dtype == torch.float32 and tuple(m.taps.shape) == (4, 12) and m.oversample == 4
    assert np.array_equal(m.taps.numpy().astype(np.float64), fd.true_peak_filter())
    assert set(m.state_dict()) == {"taps"}
    for sr, shape in ((48000, (4, 12)), (95999, (4, 12)), (96000, (2, 12)), (176400, (2, 12)), (192000, (1, 1)), (384000, (1, 1))):
        assert tuple(A.TruePeak(sr=sr).taps.shape) == shape, sr
    assert np.array_equal(A.TruePeak(sr=96000).taps.numpy(), fd.true_peak_filter(2, 12, "kaiser").astype(np.float32))
    assert tuple(A.TruePeak(oversample=8).taps.shape) == (8, 12) and A.TruePeak(oversample=1).taps.item() == 1.0
    custom = A.TruePeak(taps=torch.from_numpy(C.tables()["random 3x5"].copy()).double())
    assert custom.taps.dtype == torch.float32 and np.array_equal(custom.taps.numpy(), C.tables()["random 3x5"])
    for kw in (dict(oversample=3), dict(oversample=16), dict(taps=torch.zeros(5)), dict(taps=torch.zeros(9, 4)),
               dict(taps=torch.zeros(2, 65)), dict(taps=torch.full((2, 3), float("nan")))):
        with pytest.raises(ValueError):
            A.TruePeak(**kw)
    with pytest.raises(A.NotInvertibleError):
        m.invert(torch.zeros(2))
    time = torch.zeros(2, 2)
    with pytest.raises(A.AcidsHipError):                                     # a CPU tensor: no fall-back
        m(torch.zeros(2, 2, 100))
    with pytest.raises(A.AcidsHipError):
        m.forward_with_time(torch.zeros(2, 2, 100), time)
    for call in (m.forward, m.linear, m.programme, m.sample_peak, m.index):
        with pytest.raises(ValueError):
            call(torch.tensor(1.0))

    rt = m.realtime()
    assert isinstance(rt, A.RealtimeTruePeak) and isinstance(rt, A.TruePeak) and rt.realtime() is rt and rt.streaming() is rt
    assert isinstance(m.streaming(), A.RealtimeTruePeak) and torch.equal(rt.taps, m.taps) and rt.sr == m.sr
    assert repr(rt) == "RealtimeTruePeak(sr=44100, oversample=4, taps_per_phase=12)"
    assert rt.latency == 0 and rt.samples_seen == 0 and not rt.invertible
    sd = rt.state_dict()
    assert set(sd) == {"taps", "input_buffer", "max_peak", "max_index", "_extra_state"}
    assert sd["_extra_state"] == {"samples_seen": 0}
    assert tuple(sd["input_buffer"].shape) == (11,) and sd["input_buffer"].dtype == torch.float32
    assert tuple(sd["max_peak"].shape) == () and sd["max_peak"].dtype == torch.float32
    assert sd["max_index"].dtype == torch.int64
    assert rt.peak().item() == float("-inf") == rt.programme().item() and rt.index().item() == 0 and rt.linear().item() == 0.0
    out = rt(torch.zeros(3, 2, 0))                                           # nothing arrived: no launch, no device needed
    assert tuple(out.shape) == (3, 2) and bool(torch.isneginf(out).all()) and rt.samples_seen == 0
    with pytest.raises(ValueError):
        rt(torch.tensor(1.0))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 2, 100))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 2, 100, dtype=torch.float64))
    # any batch shape from a state_dict, the host count with it
    donor = A.RealtimeTruePeak()
    donor.input_buffer, donor.max_peak = torch.ones(3, 2, 11), torch.full((3, 2), 0.5)
    donor.max_index, donor.samples_seen = torch.full((3, 2), 7, dtype=torch.int64), 1234
    rt.load_state_dict(donor.state_dict())
    assert tuple(rt.input_buffer.shape) == (3, 2, 11) and rt.samples_seen == 1234 and rt.max_index[0, 0].item() == 7
    assert abs(rt.peak()[0, 0].item() - 20.0 * np.log10(0.5)) < 1e-5
    rt.reset()
    assert rt.samples_seen == 0 and not bool(rt.input_buffer.any()) and tuple(rt.max_peak.shape) == (3, 2)
    assert tuple(A.RealtimeTruePeak(sr=192000).input_buffer.shape) == (0,)


def test_loudness_normalize_takes_a_peak_limit():
    plain = A.LoudnessNormalize(target=-16.0, sr=48000)
    assert plain.peak_limit is None and not hasattr(plain, "true_peak") and set(plain.state_dict()) == set()
    assert repr(plain) == "LoudnessNormalize(target=-16.0, sr=48000, channel_weights=None, detach_gain=False)"
    lim = A.LoudnessNormalize(target=-16.0, sr=48000, peak_limit=-1)
    assert lim.peak_limit == -1.0 and isinstance(lim.true_peak, A.TruePeak) and lim.true_peak.sr == 48000
    assert repr(lim).endswith("detach_gain=False, peak_limit=-1.0)")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            A.LoudnessNormalize(peak_limit=bad)
    with pytest.raises(A.AcidsHipError):
        lim(torch.zeros(2, 48000))

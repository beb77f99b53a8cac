"""CPU side of the bankless sample-rate converter and PitchShift (ops.sinc_table / resample_direct, csrc/sinc_interp.hip,
transforms.PitchShift): that the half-table holds the bits of every bank entry that is not zero, that the float64 gather
of sinc_interp_cases.py is the conv1d model of resample_cases.py and that its adjoint is the gather with the roles
exchanged, the plan of the kernel, the C ABI entries, and the argument checks and constructor arithmetic that need no
device."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import resample_cases as RC
import sinc_interp_cases as C
from acids_transforms_amd import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_sinc_interp_plan", "at_sinc_interp")


@pytest.mark.parametrize("orig,new", C.RATIOS + (C.MID,))
def test_the_table_holds_the_bits_of_the_bank(orig, new):
    orig, new = C.reduced(orig, new)                               # as Resample does before it builds either
    h, width = RC.bank(orig, new)
    tab, Qi = C.table(orig, new)
    assert tab.dtype == torch.float32 and tab.shape == (Qi + 1,)
    assert Qi * 99 < 600 * max(orig, new) <= (Qi + 1) * 99         # the largest integer below lpw / rho, rho = 0.99 / max
    j = np.arange(new, dtype=np.int64)[:, None]
    k = np.arange(h.shape[1], dtype=np.int64)[None, :]
    q = np.abs((k - width) * new - j * orig)                       # n = i orig - width + k, o = i new + j
    inside = q <= Qi
    hb = h.numpy().view(np.int32)
    tb = tab.numpy().view(np.int32)[np.minimum(q, Qi)]
    assert np.array_equal(hb[inside], tb[inside])                  # bit for bit
    assert not h.numpy()[~inside].any()                            # and the bank is exactly 0 elsewhere
    # the k range [0, taps) cuts off no entry of the table that is not zero: every |q| <= Qi with table[q] != 0 occurs
    seen = np.zeros(Qi + 1, dtype=bool)
    seen[q[inside]] = True
    assert not tab.numpy()[~seen].any()
    live = int((h.numpy() != 0).sum(1).max())
    print("(%d, %d): Qi %d, %d B of table, at most %d of %d taps of a bank row are not zero"
          % (orig, new, Qi, tab.numel() * 4, live, h.shape[1]))
    assert live <= 2 * Qi // new + 1


@pytest.mark.parametrize("orig,new", C.RATIOS + (C.MID,))
def test_the_gather_is_the_conv1d_model(orig, new):
    orig, new = C.reduced(orig, new)
    worst = 0.0
    for L in (1, 2, orig - 1, orig, orig + 1, 3 * orig + 5, 1000):
        if L < 1:
            continue
        for lead in C.LEADS:
            x = C.audio(lead + (L,), 50 + L)
            want = RC.model(x, orig, new).numpy()
            got = C.model(x.numpy(), orig, new)
            assert got.shape == want.shape
            worst = max(worst, C.rel_max(got, want))
    print("(%d, %d): gather against the conv1d model, worst %.2e" % (orig, new, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("orig,new", C.RATIOS + (C.MID, C.BIG))
def test_the_adjoint_is_the_gather_with_the_roles_exchanged(orig, new):
    orig, new = C.reduced(orig, new)
    worst = 0.0
    for L in (1, 2, orig + 1, 1000) + (C.BIG_LENGTHS[:1] if (orig, new) == C.BIG else ()):
        x = C.audio((2, L), 60 + L).numpy()
        g = C.audio((2, C.out_len(L, orig, new)), 61 + L).numpy()
        lhs = float((C.model(x, orig, new) * g).sum())
        rhs = float((x * C.adjoint(g, L, orig, new)).sum())
        scale = float(np.abs(C.model(x, orig, new)).sum() * np.abs(g).max()) or 1.0
        worst = max(worst, abs(lhs - rhs) / scale)
    print("(%d, %d): <A x, g> against <x, A^T g>, worst %.2e" % (orig, new, worst))
    assert worst < 1e-12


def test_the_adjoint_is_the_models_gradient_where_a_bank_exists():
    for orig, new in ((3, 2), (147, 160), (441, 160)):
        L = 2 * orig + 3
        x, g, want = RC.model_case(orig, new, L, (3,))
        assert C.rel_max(C.adjoint(g.numpy(), L, orig, new), want.numpy()) < 1e-12


def test_the_plan():
    for orig, new in C.RATIOS + (C.reduced(*C.MID), C.BIG):
        Qi = C.table(orig, new)[1]
        for a, b in ((orig, new), (new, orig)):
            tile, in_lds = C.plan(a, b, Qi)
            assert (tile, in_lds) == C.plan(a, b, Qi)                                  # a pure function
            assert 1 <= tile <= 1024
            assert in_lds == ((orig, new) != C.BIG), (orig, new)
    assert C.table(*C.BIG)[0].numel() * 4 > 160 * 1024                                # why it is read from global memory
    # rates far apart shrink the tile until the window fits; one output's window beyond the LDS is refused
    assert C.plan(400, 1, 2424) == (16, True)                       # 1 : 400, 12 + 4848 inputs per output
    with pytest.raises(A.AcidsHipError):
        C.plan(4000, 1, 24242)                                        # 48 486 inputs per output: 194 KB
    for bad in ((0, 1, 5), (1, 0, 5), (1, 1, -1)):
        with pytest.raises(A.AcidsHipError):
            C.plan(*bad)
    # the cases reach one tile, a tile edge and several tiles of both directions
    for orig, new in C.RATIOS:
        Qi = C.table(orig, new)[1]
        tf, tb = C.plan(orig, new, Qi)[0], C.plan(new, orig, Qi)[0]
        Ls = C.lengths(orig, new)
        assert {1, 2, 3} <= {-(-C.out_len(L, orig, new) // tf) for L in Ls}, (orig, new)
        assert {1, 2, 3} <= {-(-L // tb) for L in Ls}, (orig, new)
        assert {1, 2, orig, orig + 1} <= set(Ls)


def test_c_abi():
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    declared = set(re.findall(r"\b(at_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in declared
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
    assert lib.at_abi_version() == 4                              # additive: the ABI version stays
    assert "ResampleDirectFunction" in autograd.__all__
    # argument checks come before any device call
    import ctypes
    one = ctypes.c_void_p(16)
    null = ctypes.c_void_p(0)
    call = lib.at_sinc_interp
    assert call(one, -1, 4, 3, 2, one, 5, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, -4, 3, 2, one, 5, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, 4, 0, 2, one, 5, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, 4, 3, 0, one, 5, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, 4, 3, 2, one, -1, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, 4, 3, 2, one, 5, -3, one, null) == _lib.AT_EINVAL
    assert call(null, 1, 4, 3, 2, one, 5, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, 4, 3, 2, null, 5, 3, one, null) == _lib.AT_EINVAL
    assert call(one, 1, 4, 3, 2, one, 5, 3, null, null) == _lib.AT_EINVAL
    assert call(null, 0, 4, 3, 2, null, 5, 3, null, null) == _lib.AT_OK               # empty work
    assert call(null, 3, 4, 3, 2, null, 5, 0, null, null) == _lib.AT_OK


def test_sinc_table_arguments():
    tab, Qi = ops.sinc_table(44100, 48000)
    same, Qs = ops.sinc_table(147, 160)
    assert Qi == Qs == 969 and torch.equal(tab, same)                                  # reduced by the gcd
    assert tab[0].item() == np.float32(0.99 * 147 / 147) and tab.numel() * 4 == 3880
    assert ops.sinc_table(*C.BIG)[0].numel() * 4 < 460 * 1024
    for bad in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(ValueError):
            ops.sinc_table(*bad)
    with pytest.raises(ValueError):
        ops.sinc_table(2 ** 22 + 1, 1)                                                 # more than 2^24 entries
    with pytest.raises(ValueError):
        ops.sinc_table(3, 2, rolloff=0.0)
    with pytest.raises(ValueError):
        ops.sinc_table(3, 2, lowpass_filter_width=0)


def test_errors_without_a_device():
    x = torch.zeros(2, 50)
    with pytest.raises(A.AcidsHipError):
        ops.resample_direct(x, 3, 2)
    with pytest.raises(A.AcidsHipError):
        ops.resample_direct_backward(torch.zeros(2, 34), 50, 3, 2)
    with pytest.raises(A.AcidsHipError):
        A.Resample(3, 2, direct=True)(x)
    with pytest.raises(A.AcidsHipError):
        A.Resample(3, 2, direct=True)(x.clone().requires_grad_())
    assert ops.resample_direct(x, 44100, 44100) is x                                    # equal rates: the argument itself
    assert A.Resample(5, 5, direct=True)(x) is x
    with pytest.raises(ValueError):
        ops.resample_direct(x, 0, 2)
    with pytest.raises(ValueError):
        A.RealtimeResample(3, 2, direct=True)
    with pytest.raises(ValueError):
        A.Resample(3, 2, direct=True).streaming()


def test_resample_direct_builds_no_bank_and_the_default_is_as_it_was():
    plain, direct = A.Resample(147, 160), A.Resample(147, 160, direct=True)
    assert set(dict(plain.named_buffers())) == {"kernel"} and not plain.direct
    assert torch.equal(plain.kernel, RC.bank(147, 160)[0])
    assert set(dict(direct.named_buffers())) == {"table"} and direct.Qi == 969
    assert torch.equal(direct.table, C.table(147, 160)[0])
    assert plain.state_dict() == {} and direct.state_dict() == {}                      # neither buffer is persistent
    big = A.Resample(18521, 14700, direct=True)                                        # 450 KB where the bank has 1 GB
    assert big.table.numel() == big.Qi + 1 == 112249


# ---- PitchShift ---------------------------------------------------------------------------------------------------------

def test_pitch_shift_constructor_arithmetic():
    """rate = 2 ** (-n_steps / 12) and orig_freq = int(sr / rate), as torchaudio derives them.  At 4 steps and 44100 Hz
    sr / rate = 55562.52, so orig_freq = 55562 and the converter reduces to (27781, 22050); (18521, 14700) -- C.BIG, the
    converter the kernel tests run -- is what rounding to 55563 would give, the same interval to five digits."""
    import math
    assert 55562.5 < 44100 / 2.0 ** (-4 / 12) < 55562.6 and C.reduced(55563, 44100) == C.BIG
    for n_steps, want in ((4, (27781, 22050)), (-3, (12361, 14700)), (12, (2, 1)), (-12, (1, 2)), (0, (1, 1))):
        ps = A.PitchShift(sr=44100, n_steps=n_steps)
        g = math.gcd(ps.orig_freq, 44100)
        assert (ps.orig_freq // g, 44100 // g) == want, n_steps
        assert ps.rate == 2.0 ** (-n_steps / 12) and ps.orig_freq == int(44100 / ps.rate)
        assert (ps.rate, ps.orig_freq) == C.pitch_rates(44100, n_steps)
    ps = A.PitchShift()
    assert (ps.sr, ps.n_steps, ps.bins_per_octave, ps.n_fft, ps.hop_length) == (44100, 0.0, 12, 512, 128)
    assert (ps.lowpass_filter_width, ps.rolloff) == (6, 0.99)
    assert A.PitchShift(n_fft=1024).hop_length == 256 and A.PitchShift(n_fft=1024, hop_length=100).hop_length == 100
    assert A.PitchShift(n_steps=5, bins_per_octave=24).rate == 2.0 ** (-5 / 24)
    assert isinstance(ps, A.AudioTransform) and not ps.invertible
    assert "PitchShift" in A.transforms.__all__


def test_pitch_shift_errors_and_identity():
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            A.PitchShift(n_steps=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            A.PitchShift(n_steps=2, bins_per_octave=bad)
    ps = A.PitchShift(n_steps=0)
    x = torch.zeros(2, 100)
    assert ps(x) is x                                                                   # orig_freq == sr: no kernel, no device
    y, t = ps.forward_with_time(x, torch.arange(3.0))
    assert y is x and torch.equal(t, torch.arange(3.0))
    with pytest.raises(A.NotInvertibleError):
        ps.invert(x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ps.realtime() is ps
    assert len(w) == 1 and "streaming" in str(w[0].message)
    with pytest.raises(A.AcidsHipError):
        A.PitchShift(n_steps=4)(torch.zeros(2, 2048))                                   # a CPU tensor

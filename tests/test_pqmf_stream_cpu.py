"""CPU side of the streaming PQMF (transforms.RealtimePQMF, autograd.PqmfStreamFunction / PqmfStreamInvertFunction, the
*_stream entries of csrc/pqmf.hip): the surface, the buffers and delays, the errors that need no device, the C ABI
entries, and -- in float64 -- that the definition of pqmf_stream_cases.py, chunked, is the delayed offline bank."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import acids_transforms_amd as A
import pqmf_cases as C
import pqmf_stream_cases as SC
from acids_transforms_amd import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_pqmf_analysis_stream", "at_pqmf_synthesis_stream")


def test_surface_and_exports():
    rt = A.RealtimePQMF(n_band=4, taps=65)
    assert isinstance(rt, A.PQMF) and isinstance(rt, A.AudioTransform)
    assert A.RealtimePQMF is A.pqmf.RealtimePQMF is A.transforms.RealtimePQMF
    assert "RealtimePQMF" in A.transforms.__all__ and "RealtimePQMF" in A.pqmf.__all__
    assert (A.RealtimePQMF.invertible, A.RealtimePQMF.needs_scaling, A.RealtimePQMF.scriptable) == (True, False, False)
    assert rt.ratio == 4 and repr(rt).startswith("RealtimePQMF(n_band=4, taps=65")
    for name in ("PqmfStreamFunction", "PqmfStreamInvertFunction"):
        assert name in autograd.__all__ and issubclass(getattr(autograd, name), torch.autograd.Function)
    for op in ("pqmf_analysis_stream", "pqmf_synthesis_stream", "pqmf_stream_sizes"):
        assert op in dir(ops)
    # realtime() is the module itself, silently; the hooks that cut audio to whole blocks are inherited
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert rt.realtime() is rt
    assert rt._whole_blocks(torch.zeros(2, 1003)).shape == (2, 1000)
    assert A.RealtimePQMF.test_forward is A.PQMF.test_forward and A.RealtimePQMF.test_inversion is A.PQMF.test_inversion


@pytest.mark.parametrize("n_band,taps", SC.CASES + SC.CPU_ONLY)
def test_buffers_and_delays(n_band, taps):
    rt = A.RealtimePQMF(n_band=n_band, taps=taps)
    P, D, Ha, Hs = SC.sizes(n_band, taps)
    assert ops.pqmf_stream_sizes(n_band, taps) == (D, Ha, Hs)
    assert sorted(k for k, _ in rt.named_buffers()) == ["band_buffer", "input_buffer", "modulation", "prototype"]
    assert rt.input_buffer.shape == (Ha,) and rt.band_buffer.shape == (n_band, Hs)
    assert rt.prototype.shape == (taps,) and rt.modulation.shape == (n_band, 2 * n_band)
    assert not rt.input_buffer.any() and not rt.band_buffer.any()
    assert rt.analysis_delay == rt.synthesis_delay == D * n_band and rt.latency == 2 * D * n_band


def test_delays_at_the_defaults_and_at_3_51():
    rt = A.RealtimePQMF()
    assert (rt.n_band, rt.taps) == (16, 513)
    assert rt.input_buffer.shape == (512,) and rt.band_buffer.shape == (16, 32)
    assert (rt.analysis_delay, rt.synthesis_delay, rt.latency) == (256, 256, 512) and rt.latency == rt.taps - 1
    odd = A.RealtimePQMF(n_band=3, taps=51)                       # P = 25, D = 9
    assert (odd.analysis_delay, odd.synthesis_delay, odd.latency) == (27, 27, 54)
    assert odd.input_buffer.shape == (52,) and odd.band_buffer.shape == (3, 17)


def test_offline_realtime_is_unchanged_and_streaming_shares_the_prototype():
    pq = A.PQMF(n_band=4, taps=65)
    with pytest.warns(UserWarning, match="no streaming form"):
        assert pq.realtime() is pq
    rt = pq.streaming()
    assert type(rt) is A.RealtimePQMF and rt.streaming() is rt
    assert rt.prototype is pq.prototype and rt.modulation is pq.modulation
    assert (rt.n_band, rt.taps, rt.cutoff, rt.attenuation, rt.sr) == (pq.n_band, pq.taps, pq.cutoff, pq.attenuation, pq.sr)
    assert sorted(k for k, _ in pq.named_buffers()) == ["modulation", "prototype"]       # the offline module gained none
    h = torch.from_numpy(C.prototype(0.4, 33, 60.0))
    user = A.PQMF(n_band=4, prototype=h).streaming()
    assert user.taps == 33 and user.cutoff is None and torch.equal(user.prototype, h.float())
    # the same constructor arguments
    assert torch.equal(A.RealtimePQMF(n_band=4, taps=65).prototype, pq.prototype)
    assert A.RealtimePQMF(n_band=4, prototype=h, sr=16000).sr == 16000


def test_reset_and_state_dict_of_any_batch_shape():
    rt = A.RealtimePQMF(n_band=4, taps=65)
    Ha, Hs = rt.input_buffer.shape[-1], rt.band_buffer.shape[-1]
    rt.input_buffer = torch.ones(2, 3, Ha)
    rt.band_buffer = torch.ones(2, 3, 4, Hs)
    sd = {k: v.clone() for k, v in rt.state_dict().items()}
    fresh = A.RealtimePQMF(n_band=4, taps=65)
    fresh.load_state_dict(sd)
    assert fresh.input_buffer.shape == (2, 3, Ha) and bool((fresh.input_buffer == 1).all())
    assert fresh.band_buffer.shape == (2, 3, 4, Hs) and bool((fresh.band_buffer == 1).all())
    rt.reset()
    assert rt.input_buffer.shape == (2, 3, Ha) and not rt.input_buffer.any() and not rt.band_buffer.any()


def test_errors_that_need_no_device():
    for bad in (1, 65):
        with pytest.raises(ValueError):
            A.RealtimePQMF(n_band=bad)
    with pytest.raises(ValueError):
        A.RealtimePQMF(n_band=4, taps=64)
    rt = A.RealtimePQMF(n_band=4, taps=65)
    with pytest.raises(ValueError):
        rt(torch.zeros(2, 1001))                                  # C % n_band
    with pytest.raises(ValueError):
        rt.invert(torch.zeros(2, 5, 100))                         # a wrong band axis
    with pytest.raises(ValueError):
        rt.invert(torch.zeros(100))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 1000))                                  # no CPU route
    with pytest.raises(A.AcidsHipError):
        rt.invert(torch.zeros(2, 4, 250))
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 1000, dtype=torch.float64))             # no silent narrowing
    assert rt.input_buffer.shape == (rt.input_buffer.shape[-1],) and not rt.input_buffer.any()      # a refused call leaves the state


def test_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    src = open(os.path.join(ROOT, "acids_transforms_amd", "_lib.py")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert re.search(r"\bint %s\s*\(" % name, hdr) and '"%s"' % name in src
    assert lib.at_abi_version() == 4                              # additive: the ABI version stays


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_answer_before_any_launch(entry):
    fn = getattr(_lib.lib(), entry)
    E, U, OK = _lib.AT_EINVAL, _lib.AT_EUNSUPPORTED, _lib.AT_OK
    null = ctypes.c_void_p(0)
    fake, other = ctypes.c_void_p(256), ctypes.c_void_p(512)      # never dereferenced: every call answers before a launch

    def call(rows, L, taps, n_band, p=null, shift=0, s_in=null, s_out=null):
        return fn(p, rows, L, s_in, s_out, shift, p, taps, n_band, p, 1.0, p, null)

    assert call(0, 64, 513, 16) == OK and call(3, 0, 513, 16) == OK and call(0, 0, 4, 1000, shift=99) == OK
    assert call(1, 65, 513, 16, fake) == E and call(1, 64, 512, 16, fake) == E and call(1, 64, 31, 16, fake) == E
    assert call(-1, 64, 513, 16, fake) == E and call(1, 64, 513, 0, fake) == E
    assert call(1, 64, 513, 1) == U and call(1, 130, 513, 65) == U and call(1, 64, 4099, 16, fake) == U
    assert call(1, 64, 513, 16) == E                              # a legal shape with null pointers
    # the shift is at most D = 16 blocks either way, and the new state never goes where the old one is read
    assert call(1, 64, 513, 16, fake, shift=17) == E and call(1, 64, 513, 16, fake, shift=-17) == E
    assert call(1, 64, 513, 16, fake, shift=-16, s_in=other, s_out=other) == E


@pytest.mark.parametrize("n_band,taps", SC.CASES + SC.CPU_ONLY)
def test_the_chunked_definition_is_the_delayed_offline_bank_in_float64(n_band, taps):
    hk = C.bank(C.prototype(3.141592653589793 / (2 * n_band) * 1.07, taps, 80.0), n_band)
    _, _, _, Hs = SC.sizes(n_band, taps)
    tile = ops.pqmf_tile_blocks(n_band, taps)
    blocks = SC.chunk_blocks(Hs, tile)
    T = sum(blocks)
    x = C.audio((2, n_band * T), 3)
    got = SC.stream_analysis(x, hk, blocks)
    want = SC.delayed_analysis(x, hk)
    assert got.shape == want.shape == (2, n_band, T)
    y = C.audio((2, n_band, T), 4)
    goti = SC.stream_synthesis(y, hk, blocks)
    wanti = SC.delayed_synthesis(y, hk)
    assert goti.shape == wanti.shape == (2, n_band * T)
    err_f, err_i = C.rel_max(got.numpy(), want.numpy()), C.rel_max(goti.numpy(), wanti.numpy())
    print("n_band %d taps %d blocks %s: analysis %.2e synthesis %.2e" % (n_band, taps, blocks, err_f, err_i))
    assert err_f < 1e-12 and err_i < 1e-12
    # and one call over the whole stream is one more chunking
    assert C.rel_max(SC.stream_analysis(x, hk, [T]).numpy(), want.numpy()) < 1e-12
    assert C.rel_max(SC.stream_synthesis(y, hk, [T]).numpy(), wanti.numpy()) < 1e-12

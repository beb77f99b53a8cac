"""CPU side of the differentiable and the streaming Resample (utils.Resample / RealtimeResample, autograd.ResampleFunction /
ResampleStreamFunction, at_resample_sinc_backward / at_resample_sinc_stream of csrc/resample.hip): that the cases reach
every plan of the backward kernel, that the adjoint formula the kernel is written from is the gradient of the conv1d model
in float64 -- offline and with the stream's lead --, that the chunked stream is the delayed offline converter, the C ABI
entries, and the errors that need no device."""
import ctypes
import os
import re

import pytest
import torch

import acids_transforms_amd as A
import resample_cases as C
from acids_transforms_amd import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_resample_backward_plan", "at_resample_sinc_backward", "at_resample_sinc_stream")


def test_the_cases_reach_every_plan():
    in_lds = {ratio: C.plan(*ratio)[1] for ratio in C.RATIOS}
    # the banks of the issue's table: 103 040 B and 102 312 B sit beside the window, 304 000 B and 165 816 B do not
    assert in_lds == {(1, 2): True, (2, 1): True, (3, 2): True, (2, 3): True, (147, 160): True, (160, 147): True,
                      (441, 160): False, (80, 441): False}
    assert C.bank(147, 160)[0].numel() * 4 == 103040 and C.bank(160, 147)[0].numel() * 4 == 102312
    assert C.bank(441, 160)[0].numel() * 4 == 304000 and C.bank(80, 441)[0].numel() * 4 == 165816
    assert (C.taps_of(147, 160), C.taps_of(160, 147), C.taps_of(1, 2), C.taps_of(2, 1), C.taps_of(3, 2),
            C.taps_of(441, 160), C.taps_of(80, 441)) == (161, 174, 15, 28, 23, 475, 94)
    for orig, new in C.RATIOS:
        tb = C.plan(orig, new)[0]
        tiles = {-(-(-(-L // orig)) // tb) for L in C.lengths(orig, new)}
        assert 1 in tiles and 2 in tiles and max(tiles) >= 4, (orig, new, tiles)      # one tile, a tile edge, several
        assert any(L % orig for L in C.lengths(orig, new)) or orig == 1              # a cropped last block
        # the stream's lead changes neither answer, and the plan is a pure function: twice the same
        Ha = C.stream_sizes(orig, new)[1]
        assert C.plan(orig, new, Ha) == C.plan(orig, new) == C.plan(orig, new)


@pytest.mark.parametrize("orig,new", C.RATIOS)
def test_the_adjoint_formula_is_the_models_gradient_in_float64(orig, new):
    worst = 0.0
    for L in C.lengths(orig, new):
        for lead in C.LEADS:
            x, g, want = C.model_case(orig, new, L, lead)
            got = C.adjoint(g.numpy(), L, orig, new)
            assert got.shape == want.shape == lead + (L,)
            worst = max(worst, C.rel_max(got, want.numpy()))
    print("(%d, %d): adjoint formula against autograd of the model, worst %.2e" % (orig, new, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("orig,new", C.RATIOS)
def test_the_chunked_stream_is_the_delayed_model_and_its_gradient_is_the_adjoint_with_lead_Ha(orig, new):
    D, Ha = C.stream_sizes(orig, new)
    width = C.bank(orig, new)[1]
    assert D * orig >= width and Ha - D * orig - width == 0
    blocks = C.STREAM_BLOCKS.get((orig, new), (1, 2, 3, 5))
    T = sum(blocks)
    x = C.audio((2, T * orig), 31)
    want = C.delayed(x, orig, new)
    assert want.shape == (2, T * new)
    for cut in (blocks, (1,) * T, (T,)):
        assert C.rel_max(C.stream(x, orig, new, cut).numpy(), want.numpy()) < 1e-12
    # the gradient of a chunk with the state a constant
    tb = C.plan(orig, new, Ha)[0]
    for c in (1, tb + 1):
        state = C.audio((2, Ha), 32)
        xc = C.audio((2, c * orig), 33).requires_grad_()
        g = C.audio((2, c * new), 34)
        y, new_state = C.stream_chunk(xc, state, orig, new)
        (y * g).sum().backward()
        assert torch.equal(new_state, torch.cat([state, xc.detach()], -1)[..., -Ha:])
        got = C.adjoint(g.numpy(), c * orig, orig, new, lead=Ha)
        assert C.rel_max(got, xc.grad.numpy()) < 1e-12


def test_surface():
    rs = A.Resample(44100, 48000)
    rt = rs.streaming()
    assert type(rt) is A.RealtimeResample and isinstance(rt, A.Resample) and rt.streaming() is rt
    assert A.RealtimeResample is A.utils.RealtimeResample and rt.kernel is rs.kernel
    assert (rt.orig, rt.new, rt.width) == (147, 160, 7)
    D, Ha = C.stream_sizes(147, 160)
    assert (D, Ha) == (1, 154) == ops.resample_stream_sizes(147, 7)
    assert rt.delay == 147 and rt.output_delay == 160 and rt.ratio == 160 / 147
    assert rt.input_buffer.shape == (Ha,) and not rt.input_buffer.any()
    assert sorted(rt.state_dict()) == ["input_buffer"] and sorted(rs.state_dict()) == []
    down = A.RealtimeResample(3, 2)
    assert down.delay == 12 and down.output_delay == 8 and down.input_buffer.shape == (22,)
    for name in ("ResampleFunction", "ResampleStreamFunction"):
        assert name in autograd.__all__ and issubclass(getattr(autograd, name), torch.autograd.Function)
    for op in ("resample_sinc_backward", "resample_backward_plan", "resample_sinc_stream", "resample_stream_sizes"):
        assert op in dir(ops)
    # equal rates stay the identity, streaming included
    same = A.RealtimeResample(8000, 8000)
    x = torch.zeros(2, 5, requires_grad=True)
    assert same(x) is x and A.Resample(8000, 8000)(x) is x and same.delay == 0


def test_reset_and_state_dict_of_any_batch_shape():
    rt = A.RealtimeResample(3, 2)
    rt.input_buffer = torch.ones(2, 3, 22)
    sd = {k: v.clone() for k, v in rt.state_dict().items()}
    fresh = A.RealtimeResample(3, 2)
    fresh.load_state_dict(sd)
    assert fresh.input_buffer.shape == (2, 3, 22) and bool((fresh.input_buffer == 1).all())
    rt.reset()
    assert rt.input_buffer.shape == (2, 3, 22) and not rt.input_buffer.any()


def test_errors_that_need_no_device():
    rt = A.RealtimeResample(3, 2)
    with pytest.raises(ValueError):
        rt(torch.zeros(2, 10))                                    # a ragged chunk
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 9))                                     # no CPU route
    with pytest.raises(A.AcidsHipError):
        rt(torch.zeros(2, 9, dtype=torch.float64))                # no silent narrowing
    assert rt.input_buffer.shape == (22,) and not rt.input_buffer.any()      # a refused call leaves the state
    rs = A.Resample(3, 2)
    with pytest.raises(A.AcidsHipError):
        rs(torch.zeros(2, 9, requires_grad=True))                 # the grad route raises what the plain one does
    with pytest.raises(A.AcidsHipError):
        rs(torch.zeros(2, 9))


def test_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    src = open(os.path.join(ROOT, "acids_transforms_amd", "_lib.py")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert re.search(r"\bint %s\s*\(" % name, hdr) and '"%s"' % name in src
    assert lib.at_abi_version() == 4                              # additive: the ABI version stays


def test_argument_checks_answer_before_any_launch():
    lib = _lib.lib()
    E, U, OK = _lib.AT_EINVAL, _lib.AT_EUNSUPPORTED, _lib.AT_OK
    null = ctypes.c_void_p(0)
    fake, other = ctypes.c_void_p(256), ctypes.c_void_p(512)      # never dereferenced: every call answers before a launch

    def bwd(rows, L, out_len, p=null, orig=3, new=2, taps=23, lead=10):
        return lib.at_resample_sinc_backward(p, rows, L, orig, new, taps, lead, p, out_len, p, null)

    assert bwd(0, 9, 6) == OK and bwd(4, 0, 0) == OK              # empty work
    assert bwd(1, 9, 6) == E                                      # a legal shape with null pointers
    assert bwd(-1, 9, 6, fake) == E and bwd(1, -9, 6, fake) == E and bwd(1, 9, -6, fake) == E
    assert bwd(1, 9, 6, fake, orig=0) == E and bwd(1, 9, 6, fake, new=0) == E and bwd(1, 9, 6, fake, taps=0) == E
    assert bwd(1, 9, 6, fake, lead=-1) == E
    assert bwd(1, 9, 7, fake) == E and bwd(1, 10, 6, fake) == E and bwd(0, 9, 7) == E      # out_len != ceil(new L / orig)
    assert bwd(65536, 9, 6, fake) == U                            # the forward's row limit
    assert lib.at_resample_sinc(fake, 65536, 9, 3, 2, 10, fake, 6, fake, null) == U

    def stream(rows, C, p=null, s_in=null, s_out=null, orig=3, new=2, width=10):
        return lib.at_resample_sinc_stream(p, rows, C, s_in, s_out, orig, new, width, p, p, null)

    assert stream(0, 9) == OK and stream(2, 0) == OK
    assert stream(1, 9) == E and stream(1, 10, fake) == E and stream(-1, 9, fake) == E
    assert stream(1, 9, fake, s_in=other, s_out=other) == E       # the new state never goes where the old one is read
    assert stream(1, 9, fake, orig=0) == E and stream(1, 9, fake, width=-1) == E
    assert stream(65536, 9, fake) == U

    tile, in_lds = ctypes.c_int(0), ctypes.c_int(0)
    plan = lib.at_resample_backward_plan
    assert plan(3, 2, 23, 10, ctypes.byref(tile), ctypes.byref(in_lds)) == OK and tile.value > 0
    assert plan(0, 2, 23, 10, ctypes.byref(tile), ctypes.byref(in_lds)) == E
    assert plan(3, 2, 23, 10, None, ctypes.byref(in_lds)) == E

"""Host side of the streaming partitioned convolution (ops.fft_convolve_stream_plan, at_fft_convolve_stream_plan /
at_spectral_fir_stream of csrc/fft_convolve.hip, transforms.RealtimeImpulseResponse): the streaming algorithm -- tail, ring
with its head, sub-chunks of 8, zeros before the start -- restated in float64 against numpy.convolve at every case of the
table, the plan, the C entry's answers that need no device, the module's buffers, state and errors.  No device needed."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import convolve_stream_cases as S
import fft_convolve_cases as C
from acids_transforms_amd import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the algorithm, in float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", S.TAPS)
def test_streaming_algorithm_against_numpy_convolve_in_float64(K):
    """Every chunking, all 70 rows (every leading shape of the table is a set of these rows); worst figure 6.2e-16."""
    x, h, _ = S.data(K)
    want = S.reference(K)
    xt, ht = torch.as_tensor(x.astype(np.float64)), torch.as_tensor(h.astype(np.float64))
    for chunks in S.CHUNKINGS:
        assert sum(chunks) == S.STREAM_BLOCKS
        got = S.stream(xt, ht, S.BLOCK, chunks).numpy()
        err = C.rel_max(got, want)
        print("K %d chunks %s: %.2e" % (K, chunks[:6], err))
        assert got.shape == want.shape and err < 1e-10
        for lead in S.LEADS:
            assert C.rel_max(C.take(got, lead), C.take(want, lead)) < 1e-10


@pytest.mark.parametrize("B,K,rows", S.BLOCK_CASES)
def test_streaming_algorithm_at_the_other_blocks(B, K, rows):
    x, h, _ = S.data(K, B, sum(S.BLOCK_CHUNKS), rows)
    got = S.stream(torch.as_tensor(x.astype(np.float64)), torch.as_tensor(h.astype(np.float64)), B, S.BLOCK_CHUNKS).numpy()
    err = C.rel_max(got, S.reference(K, B, sum(S.BLOCK_CHUNKS), rows))
    print("block %d K %d: %.2e" % (B, K, err))
    assert err < 1e-10


def test_case_table_covers_what_it_says():
    parts = [ops.fft_convolve_stream_plan(K, S.BLOCK)[1] for K in S.TAPS]
    assert parts == [1, 1, 2, 3, 8, 9, 18]
    for K in S.TAPS:                                                              # the ring wraps over 40 blocks
        assert ops.fft_convolve_stream_plan(K, S.BLOCK)[2] < S.STREAM_BLOCKS
    assert any(n > S.MAX_FRAMES for n in S.CHUNKINGS[2]) and S.MAX_FRAMES == ops.fft_convolve_stream_plan(1)[3]
    assert [ops.fft_convolve_stream_plan(K, B)[0] for B, K, _ in S.BLOCK_CASES] == [256, 512, 1024, 2048]
    # the gradient reference restates truncation at chunk boundaries: one chunk is plain conv1d autograd
    x, h, g = S.data(129, rows=2)
    gx, gh, _ = S.chunk_gradients(x, h, g, S.BLOCK, (S.STREAM_BLOCKS,))
    _, rx, rh = C.conv1d_autograd(x, h, np.pad(g, ((0, 0), (0, 128))))
    assert C.rel_max(gx, rx) < 1e-10 and C.rel_max(gh, rh) < 1e-10


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_stream_plan_follows_the_offline_rule():
    for K in (1, 2, 300, 513, 2048, 2049, 4096, 4097, 8192, 8193, 22050, 66150, 10 ** 6):
        B, P, R, n = ops.fft_convolve_stream_plan(K)
        assert B == ops.fft_convolve_plan(1, K)[0] and P == -(-K // B) and n == 8 and R == P - 1 + n
        for block in ops.FFT_CONVOLVE_BLOCKS:
            assert ops.fft_convolve_stream_plan(K, block) == (block, -(-K // block), -(-K // block) + 7, 8)
    assert ops.fft_convolve_stream_plan(513)[0] == 512 and ops.fft_convolve_stream_plan(66150)[:2] == (2048, 33)


def test_stream_plan_rejects_what_it_must():
    for block in (0, 64, 100, 129, 4096, -128, 128.5, True):
        with pytest.raises(ValueError):
            ops.fft_convolve_stream_plan(10, block)
    for K in (0, -3):
        with pytest.raises(ValueError):
            ops.fft_convolve_stream_plan(K)
    plan = _lib.lib().at_fft_convolve_stream_plan
    out = [ctypes.c_int64(0) for _ in range(4)]
    refs = [ctypes.byref(o) for o in out]
    assert plan(300, 0, *refs) == _lib.AT_OK and [o.value for o in out] == [512, 1, 8, 8]
    assert plan(300, 128, *refs) == _lib.AT_OK and [o.value for o in out] == [128, 3, 10, 8]
    assert plan(0, 0, *refs) == _lib.AT_EINVAL and plan(10, 100, *refs) == _lib.AT_EINVAL and plan(10, -1, *refs) == _lib.AT_EINVAL
    for i in range(4):
        assert plan(10, 0, *[None if j == i else r for j, r in enumerate(refs)]) == _lib.AT_EINVAL


# ---- the C entry, without a device ---------------------------------------------------------------------------------------------
def _stream(rows=0, Tc=0, P=1, R=8, head=0, F=129, X=64, ring=128, H=192, Y=256, xs=None):
    p = ctypes.c_void_p
    xs = Tc * F if xs is None else xs
    return _lib.lib().at_spectral_fir_stream(p(X), xs, p(ring), p(H), rows, Tc, P, R, head, F, p(Y), p(0))


def test_c_entry_answers_that_need_no_device():
    assert _stream() == _lib.AT_OK and _stream(rows=0, Tc=5) == _lib.AT_OK and _stream(rows=3, Tc=0) == _lib.AT_OK
    assert _stream(rows=3, Tc=0, X=0, ring=0, H=0, Y=0) == _lib.AT_OK                 # nothing arrived: nothing is looked at
    assert _stream(rows=-1) == _lib.AT_EINVAL and _stream(Tc=-1) == _lib.AT_EINVAL and _stream(Tc=9, R=16) == _lib.AT_EINVAL
    assert _stream(P=0) == _lib.AT_EINVAL and _stream(F=0) == _lib.AT_EINVAL and _stream(xs=-1) == _lib.AT_EINVAL
    assert _stream(rows=2, Tc=8, P=3, R=9) == _lib.AT_EINVAL                          # R < P - 1 + Tc
    assert _stream(rows=2, Tc=1, P=1, R=0) == _lib.AT_EINVAL
    assert _stream(head=-1) == _lib.AT_EINVAL and _stream(head=8) == _lib.AT_EINVAL and _stream(R=10, head=10) == _lib.AT_EINVAL
    for null in ("X", "ring", "H", "Y"):
        assert _stream(rows=2, Tc=3, **{null: 0}) == _lib.AT_EINVAL
    assert _stream(rows=2, Tc=3, xs=3 * 129 - 1) == _lib.AT_EINVAL
    assert _stream(rows=2, Tc=3, ring=132) == _lib.AT_EINVAL                          # complex64 is 8-byte aligned


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ("at_fft_convolve_stream_plan", "at_spectral_fir_stream"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert "ImpulseResponseStreamFunction" in autograd.__all__
    assert issubclass(autograd.ImpulseResponseStreamFunction, torch.autograd.Function)
    assert "RealtimeImpulseResponse" in A.transforms.__all__
    assert A.RealtimeImpulseResponse is A.transforms.RealtimeImpulseResponse is A.convolve.RealtimeImpulseResponse
    assert issubclass(A.RealtimeImpulseResponse, A.ImpulseResponse)


# ---- the module on the host --------------------------------------------------------------------------------------------------
def test_module_buffers_and_shapes():
    ir = torch.tensor([1.0, 0.5, 0.25])
    m = A.RealtimeImpulseResponse(ir)
    assert isinstance(m, A.AudioTransform) and not m.invertible and m.taps == 3 and m.latency == 0 and m.head == 0
    assert (m.block, m.partitions, m.ring_slots, m.max_frames) == (512, 1, 8, 8)
    bufs = dict(m.named_buffers())
    assert set(bufs) == {"ir", "input_buffer", "spectrum_ring"} and not list(m.parameters())
    assert bufs["input_buffer"].shape == (512,) and bufs["input_buffer"].dtype == torch.float32
    assert bufs["spectrum_ring"].shape == (8, 513) and bufs["spectrum_ring"].dtype == torch.complex64
    assert not bufs["input_buffer"].any() and not torch.view_as_real(bufs["spectrum_ring"]).any()
    small = A.RealtimeImpulseResponse(torch.ones(300), block=128, learnable=True, sr=48000)
    assert (small.block, small.partitions, small.ring_slots) == (128, 3, 10) and small.sr == 48000
    assert isinstance(small.ir, torch.nn.Parameter) and [n for n, _ in small.named_parameters()] == ["ir"]
    assert small.spectrum_ring.shape == (10, 129)
    assert m.realtime() is m and m.streaming() is m
    with pytest.raises(A.NotInvertibleError):
        m.invert(torch.zeros(2, 512))
    x = torch.zeros(3, 5)
    assert A.RealtimeImpulseResponse()(x) is x                                    # the pass-through, any length
    y, time = A.RealtimeImpulseResponse().forward_with_time(x, torch.ones(3))
    assert y is x and torch.equal(time, torch.ones(3))
    assert callable(m.test_forward) and callable(A.RealtimeImpulseResponse.test_scripted_transform)


def test_streaming_shares_the_response_and_realtime_stays():
    ir = torch.tensor([1.0, 0.5, 0.25])
    for learnable in (False, True):
        m = A.ImpulseResponse(ir, learnable=learnable)
        rt = m.streaming()
        assert isinstance(rt, A.RealtimeImpulseResponse) and rt.ir is m.ir and rt.learnable == learnable and rt.taps == 3
        assert isinstance(rt.ir, torch.nn.Parameter) == learnable
        assert m.streaming(block=128).block == 128 and m.streaming(block=128).ir is m.ir
        with pytest.warns(UserWarning):
            assert m.realtime() is m                                              # unchanged: the offline module, with the warning
    through = A.ImpulseResponse().streaming()
    assert isinstance(through, A.RealtimeImpulseResponse) and through.passthrough
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rt = A.RealtimeImpulseResponse(ir)
        assert rt.realtime() is rt                                                # no warning from the streaming form


def test_reset_and_state_dict_round_trip():
    m = A.RealtimeImpulseResponse(torch.ones(300), block=128)
    sd = m.state_dict()
    assert set(sd) == {"ir", "input_buffer", "spectrum_ring", "_extra_state"} and sd["_extra_state"] == {"head": 0}
    g = torch.Generator().manual_seed(0)
    m.input_buffer = torch.randn(2, 3, 128, generator=g)
    m.spectrum_ring = torch.randn(2, 3, 10, 129, 2, generator=g).view(torch.complex64).squeeze(-1)
    m.head = 7
    sd = m.state_dict()
    assert sd["_extra_state"] == {"head": 7} and not sd["input_buffer"].requires_grad
    fresh = A.RealtimeImpulseResponse(torch.zeros(300), block=128)
    fresh.load_state_dict(sd)                                                     # another batch shape, and head
    assert fresh.head == 7 and torch.equal(fresh.input_buffer, m.input_buffer) and fresh.input_buffer.shape == (2, 3, 128)
    assert torch.equal(torch.view_as_real(fresh.spectrum_ring), torch.view_as_real(m.spectrum_ring))
    assert torch.equal(fresh.ir, m.ir)
    fresh.reset()
    assert fresh.head == 0 and fresh.input_buffer.shape == (2, 3, 128) and not fresh.input_buffer.any()
    assert fresh.spectrum_ring.shape == (2, 3, 10, 129) and not torch.view_as_real(fresh.spectrum_ring).any()
    assert m.head == 7 and bool(m.input_buffer.any())                             # a load copies: the source keeps its stream


def test_shape_and_argument_errors_come_before_any_device():
    m = A.RealtimeImpulseResponse(torch.ones(300), block=128)
    for bad in (torch.zeros(3, 100), torch.zeros(3, 129), torch.zeros(3, 0), torch.zeros(0), torch.tensor(1.0)):
        with pytest.raises(ValueError):
            m(bad)
    assert m.head == 0 and m.input_buffer.shape == (128,)
    for bad_ir in (torch.zeros(0), torch.zeros(2, 3), 1.0):
        with pytest.raises(ValueError):
            A.RealtimeImpulseResponse(bad_ir)
    with pytest.raises(ValueError):
        A.RealtimeImpulseResponse(None, learnable=True)                           # the pass-through has nothing to learn
    for block in (0, 100, 4096, True):
        with pytest.raises(ValueError):
            A.RealtimeImpulseResponse(torch.ones(4), block=block)
    c = lambda *s: torch.zeros(*s, dtype=torch.complex64)
    for Xc, ring, H in ((c(2, 3), c(2, 10, 129), c(3, 129)), (c(2, 3, 129), c(3, 10, 129), c(3, 129)),
                        (c(2, 3, 129), c(2, 10, 129), c(3, 128)), (c(2, 3, 129), c(2, 10, 129), c(2, 3, 129)),
                        (c(2, 3, 129), torch.zeros(2, 10, 129), c(3, 129)), (c(2, 3, 129), c(2, 10, 258)[..., ::2], c(3, 129))):
        with pytest.raises(ValueError):
            ops.spectral_fir_stream(Xc, ring, 0, H)


def test_cpu_tensors_are_refused():
    x = torch.zeros(3, 256)
    for learnable in (False, True):                                               # the plain and the grad route
        m = A.RealtimeImpulseResponse(torch.ones(300), block=128, learnable=learnable)
        with pytest.raises(A.AcidsHipError):
            m(x)
        with pytest.raises(A.AcidsHipError):
            m(x.clone().requires_grad_())
        assert m.head == 0 and not m.input_buffer.any()
    c = lambda *s: torch.zeros(*s, dtype=torch.complex64)
    with pytest.raises(A.AcidsHipError):
        ops.spectral_fir_stream(c(2, 3, 129), c(2, 10, 129), 0, c(3, 129))
    with pytest.raises(A.AcidsHipError):
        ops.fft_convolve_stream(x, torch.zeros(3, 128), c(3, 10, 129), 0, c(3, 129), 128)

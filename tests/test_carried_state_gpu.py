"""The carried-state rule (transforms.carried.CarriedState) through the kernels, for every module that follows it: a new
leading shape restarts the stream, and a module cast between two chunks does not break it.  A few launches on a handful of
samples each; every comparison is torch.equal.

`module.double()` also widens the impulse response's own `ir`, and a float64 response is refused like float64 audio
(test_convolve_stream_gpu.py::test_float64_is_refused_without_the_opt_in).  That is no carried state: the case asserts the
refusal, hands `ir` its float32 values back (the round trip through float64 is exact) and leaves the two state buffers as
the cast made them."""
import pytest
import torch

import acids_transforms_amd as A
from carried_state_cases import MODULES, NAMES

pytestmark = pytest.mark.gpu


def _chunk(lead, tail, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(lead + tail, generator=g) * 2 - 1).to(dev)


@pytest.mark.parametrize("name", NAMES)
def test_a_new_leading_shape_restarts_the_stream(dev, name):
    make, dtypes, streams = MODULES[name]
    m, fresh = make().to(dev), make().to(dev)
    for method, tail in streams:
        getattr(m, method)(_chunk((2,), tail, 1, dev))
    for k in dtypes:
        assert getattr(m, k).shape[0] == 2 and bool(getattr(m, k).any())
    for method, tail in streams:
        x = _chunk((3,), tail, 2, dev)
        assert torch.equal(getattr(m, method)(x), getattr(fresh, method)(x))
    for k in dtypes:
        assert getattr(m, k).shape[0] == 3 and torch.equal(getattr(m, k), getattr(fresh, k))


@pytest.mark.parametrize("name", NAMES)
def test_a_module_cast_between_two_chunks_continues_the_stream(dev, name):
    make, dtypes, streams = MODULES[name]
    m, twin = make().to(dev), make().to(dev)
    for method, tail in streams:
        x = _chunk((2,), tail, 1, dev)
        assert torch.equal(getattr(m, method)(x), getattr(twin, method)(x))
    m = m.double()
    if name == "impulse_response":
        with pytest.raises(A.AcidsHipError, match="ir is float64"):
            m(_chunk((2,), streams[0][1], 2, dev))
        m.ir = m.ir.float()
    for method, tail in streams:
        x = _chunk((2,), tail, 2, dev)
        y = getattr(m, method)(x)
        assert y.dtype == torch.float32 and torch.equal(y, getattr(twin, method)(x))
    for k, dtype in dtypes.items():
        assert getattr(m, k).dtype == dtype and torch.equal(getattr(m, k), getattr(twin, k))

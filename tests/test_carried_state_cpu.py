"""The carried-state rule (transforms.carried.CarriedState) on host tensors, for every module that follows it: what starts a
new stream, that a module cast does not reach the state's dtype, and reset().  No kernel runs here; the per-module
test_reset_and_state_dict... tests cover the state_dict side."""
import pytest
import torch

from acids_transforms_amd.transforms.carried import CarriedState
from carried_state_cases import MODULES, NAMES


def _with_lead(m, dtypes, lead):
    """Gives every carried buffer the leading shape `lead`, filled with ones."""
    for k, dtype in dtypes.items():
        m._carry(k, torch.ones(lead + m._carried_tail(k), dtype=dtype), lead)


@pytest.mark.parametrize("name", NAMES)
def test_every_carried_buffer_is_named_once(name):
    make, dtypes, _ = MODULES[name]
    m = make()
    assert isinstance(m, CarriedState) and set(m._carried) == set(dtypes)
    for k, dtype in dtypes.items():
        buf = getattr(m, k)
        assert k in m._buffers and k in m.state_dict() and m._carried[k] == (tuple(buf.shape), dtype) and not buf.any()
    # the stream of the buffers' own leading shape: each as (rows,) + tail
    rows = m._carried_rows(list(dtypes), (), torch.zeros(1))
    assert [tuple(r.shape) for r in rows] == [(1,) + m._carried_tail(k) for k in dtypes]


@pytest.mark.parametrize("name", NAMES)
def test_a_new_leading_shape_or_device_starts_a_new_stream(name):
    make, dtypes, _ = MODULES[name]
    m = make()
    _with_lead(m, dtypes, (2,))
    names = list(dtypes)
    x = torch.zeros(1)
    assert [tuple(r.shape) for r in m._carried_rows(names, (2,), x)] == [(2,) + m._carried_tail(k) for k in names]
    for lead in ((3,), (), (2, 1), (1, 2)):
        assert m._carried_rows(names, lead, x) is None
    assert m._carried_rows(names, (2,), torch.zeros(1, device="meta")) is None
    if len(names) > 1:                                           # one buffer of another stream: none of them is handed back
        m._carry(names[0], torch.ones((3,) + m._carried_tail(names[0]), dtype=dtypes[names[0]]), (3,))
        assert m._carried_rows(names, (2,), x) is None and m._carried_rows(names, (3,), x) is None
        assert m._carried_rows(names[1:], (2,), x) is not None


@pytest.mark.parametrize("cast", ["double", "half"])
@pytest.mark.parametrize("name", NAMES)
def test_a_module_cast_does_not_reach_the_states_dtype(name, cast):
    make, dtypes, _ = MODULES[name]
    m = make()
    _with_lead(m, dtypes, (2,))
    m = getattr(m, cast)()
    rows = m._carried_rows(list(dtypes), (2,), torch.zeros(1))
    assert [r.dtype for r in rows] == list(dtypes.values())
    assert all(bool((r == 1).all()) for r in rows)               # ones survive every cast
    if name == "impulse_response":
        m.head = 5
    m.reset()
    for k, dtype in dtypes.items():
        buf = getattr(m, k)
        assert buf.dtype == dtype and tuple(buf.shape) == (2,) + m._carried_tail(k) and not buf.any()
    if name == "impulse_response":
        assert m.head == 0

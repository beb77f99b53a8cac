"""CarriedState: the one rule of the state a streaming module carries from chunk to chunk in its buffers (RealtimePQMF,
utils.RealtimeResample, RealtimeSOSFilter, RealtimeImpulseResponse).

A carried buffer has the shape (lead..., tail...): `tail` and the dtype are those it was registered with, `lead` is the
leading batch shape of the stream it belongs to.  It accepts any leading shape from a `state_dict`; `reset()` zeroes it in
place of its current shape; a chunk with another leading shape or on another device starts a new stream from zeros; the
state after a chunk is stored detached (it is a constant of the graph); and it keeps its own dtype whatever `.half()` or
`.double()` did to the module -- a state is no audio, nothing narrows or widens it.

OverlapAdd does not follow this rule: it mirrors the reference's buffer helpers and moves with its input's device."""
import math

import torch

__all__ = ["CarriedState"]


class CarriedState:
    """Mixin in front of an nn.Module.  The subclass registers its carried buffers, then names them once with `_carries`."""

    def _carries(self, *names) -> None:
        self._carried = {k: (tuple(self._buffers[k].shape), self._buffers[k].dtype) for k in names}

    def _carried_tail(self, name: str) -> tuple:
        """The shape of one row's state.  A subclass whose tail can change after construction (the sections of a filter
        loaded from a state_dict) answers from what it holds now."""
        return self._carried[name][0]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for k, (_, dtype) in self._carried.items():              # any batch shape, as OverlapAdd's
            if prefix + k in state_dict:
                self._buffers[k] = torch.zeros_like(state_dict[prefix + k], dtype=dtype)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def reset(self) -> None:
        """Forget the stream: every carried state becomes zeros (of its current shape)."""
        for k, (_, dtype) in self._carried.items():
            setattr(self, k, torch.zeros_like(self._buffers[k], dtype=dtype))
        self._reset_extra()

    def _reset_extra(self) -> None:
        """Host state that goes with the buffers (RealtimeImpulseResponse's ring head)."""

    def _carried_rows(self, names, lead, x: torch.Tensor):
        """The named states as the kernels read them, each (rows,) + tail in its own dtype, when all of them belong to
        the stream of x -- shape lead + tail, on x's device -- or None: a new leading batch shape or a new device starts
        a new stream for all of them."""
        lead, rows = tuple(lead), []
        for k in names:
            tail, buf = self._carried_tail(k), self._buffers[k]
            if tuple(buf.shape) != lead + tail or buf.device != x.device:
                return None
            dtype = self._carried[k][1]
            rows.append(buf.to(dtype).contiguous().view((math.prod(lead),) + tail))      # a view: a kernel may update it
        return rows

    def _carry(self, name: str, new: torch.Tensor, lead) -> None:
        """Stores the state after a chunk."""
        setattr(self, name, new.detach().reshape(tuple(lead) + self._carried_tail(name)))

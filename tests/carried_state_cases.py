"""Shared by test_carried_state_cpu.py and test_carried_state_gpu.py: the four streaming modules that carry their state by
transforms.carried.CarriedState, at their smallest constructions, the dtype each carried buffer is registered with, and the
streams each module runs -- (method, tail shape of a chunk two blocks long)."""
import torch

import acids_transforms_amd as A

SOS = [[1.0, 0.0, 0.0, 1.0, -0.5, 0.0], [1.0, 0.2, 0.0, 1.0, 0.1, 0.05]]


def _impulse_response():
    g = torch.Generator().manual_seed(3)
    return A.RealtimeImpulseResponse(torch.randn(200, generator=g) / 200, block=128)


# name: (constructor, {carried buffer: dtype}, [(method, chunk tail)])
MODULES = {
    "pqmf": (lambda: A.RealtimePQMF(n_band=4, taps=9), {"input_buffer": torch.float32, "band_buffer": torch.float32},
             [("forward", (8,)), ("invert", (4, 2))]),
    "resample": (lambda: A.RealtimeResample(3, 2), {"input_buffer": torch.float32}, [("forward", (6,))]),
    "sos": (lambda: A.RealtimeSOSFilter(SOS), {"state": torch.float64}, [("forward", (5,))]),
    "impulse_response": (_impulse_response, {"input_buffer": torch.float32, "spectrum_ring": torch.complex64},
                         [("forward", (256,))]),
}
NAMES = sorted(MODULES)

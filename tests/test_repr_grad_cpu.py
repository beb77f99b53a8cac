"""CPU side of the forward backward of Phase / IF / Polar / PolarIF / Cartesian (at_phase_scan_backward,
at_cartesian_pack_backward; autograd.PhaseScanFunction and its neighbours): the formulas the kernels implement
(repr_grad_cases.formula_*) against torch autograd of the reference's own expressions in float64, the sweep's coverage,
and the C ABI's argument checks, which touch no device.

The formula tests run no line of the library: both sides are restatements in the test tree (they pin down the maths the
kernels and test_repr_grad_gpu.py are held to, and pass with or without the feature).  What guards the change on the CPU
are the tests of the exported symbols, the header, the binding, the AT_EINVAL / AT_OK answers and autograd.__all__."""
import itertools
import math
import os
import re

import pytest
import torch

import repr_grad_cases as C
from acids_transforms_amd import _lib
from conftest import rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _spectrum(g, shape):
    return torch.randn(shape, dtype=torch.complex128, generator=g) * 3


# a single frame has no central difference: the reference's cat makes two rows of it, and the module builds that case
# from the angle, cat and affine (test_single_frame_central_composition)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode,T", [(m, T) for m in C.MODES for T in [1, 2, 3, 4, 5, 9, 16]
                                    if not (m == "central" and T == 1)])
def test_scan_backward_formula(mode, T, weighted):
    g = torch.Generator().manual_seed(1000 * T + 10 * C.MODES.index(mode) + weighted)
    X = _spectrum(g, (2, T, 6))
    gout = torch.randn(2, T, 6, generator=g, dtype=torch.float64)
    window = torch.rand(T, generator=g, dtype=torch.float64) + 0.5 if weighted else None
    off, sc = (0.3, 1.7) if weighted else (None, None)
    want = C.autograd_of(lambda t: C.ref_scan(t, mode, window, off, sc), X, gout)
    got = C.formula_scan_backward(X.numpy(), gout.numpy(), mode, None if window is None else window.numpy(), sc)
    assert rel_max(got, want.numpy()) < TOL


def test_unwrap_has_the_identity_as_its_derivative():
    """Jumps beyond pi on purpose (a spectrum whose phase advances by 2.5 rad per frame wraps every third frame)."""
    T = 12
    ph = torch.remainder(torch.arange(T, dtype=torch.float64).reshape(T, 1) * 2.5 + torch.tensor([0.0, 1.0, 2.0]) + math.pi,
                         2 * math.pi) - math.pi
    assert bool(((ph[1:] - ph[:-1]).abs() >= math.pi).any())
    leaf = ph.clone().requires_grad_()
    gout = torch.randn(T, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    u = C.ref_unwrap(leaf)
    assert float((u[1:] - u[:-1] - 2.5).detach().abs().max()) < 1e-9       # it did unwrap
    u.backward(gout)
    assert torch.equal(leaf.grad, gout)


@pytest.mark.parametrize("weighted", [False, True])
def test_single_frame_central_composition(weighted):
    """T == 1, central: two rows of the one frame's angle (weighted, normalised) -- what IF._scan composes from the
    angle's backward, torch's cat and product, and the affine's backward: g / sc summed over the two rows."""
    g = torch.Generator().manual_seed(7)
    X = _spectrum(g, (3, 1, 5))
    gout = torch.randn(3, 2, 5, generator=g, dtype=torch.float64)
    w = torch.tensor([0.4, 1.1], dtype=torch.float64) if weighted else None

    def ref(t):
        y = C.ref_fdiff(C.ref_unwrap(t.angle()), "central")
        assert y.shape[-2] == 2
        y = w.reshape(-1, 1) * y if weighted else y
        return (y - 0.2) / 1.9
    want = C.autograd_of(ref, X, gout)
    a = gout.numpy() / 1.9 * (w.numpy()[:, None] if weighted else 1.0)
    got = C.formula_scan_backward(X.numpy(), a.sum(-2, keepdims=True), "angle")
    assert rel_max(got, want.numpy()) < TOL


def test_zero_bins_get_a_zero_gradient():
    X = torch.zeros(1, 3, 4, dtype=torch.complex128)
    X[0, 1, 2] = 1 + 1j
    gout = torch.ones(1, 3, 4, dtype=torch.float64)
    for mode in C.MODES:
        want = C.autograd_of(lambda t: C.ref_scan(t, mode), X, gout).numpy()
        got = C.formula_scan_backward(X.numpy(), gout.numpy(), mode)
        assert (got[X.numpy() == 0] == 0).all() and rel_max(got, want) < TOL


@pytest.mark.parametrize("re_norm,im_norm", [((None, None), (None, None)), ((0.8, 1.6), (-1.25, 7.5)),
                                             ((None, None), (2.5, 3.75))])
def test_cartesian_forward_formula(re_norm, im_norm):
    g = torch.Generator().manual_seed(6)
    X = _spectrum(g, (3, 17))
    gout = torch.randn(3, 2, 17, generator=g, dtype=torch.float64)
    want = C.autograd_of(lambda t: C.ref_cartesian(t, re_norm, im_norm), X, gout)
    got = C.formula_cartesian_forward(gout.numpy(), re_norm[1], im_norm[1])
    assert rel_max(got, want.numpy()) < TOL


def test_affine_forward_gradient_is_g_over_scale():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 16, generator=g, dtype=torch.float64)
    gout = torch.randn(3, 16, generator=g, dtype=torch.float64)
    want = C.autograd_of(lambda t: C.ref_normalise(t, (0.8, 1.6)), x, gout)
    assert rel_max((gout / 1.6).numpy(), want.numpy()) < TOL


# ---- the sweep ------------------------------------------------------------------------------------------------------------

def test_sweep_covers_every_shape_and_every_pair_of_options():
    cases = C.kernel_cases()
    assert len(cases) == len(C.MODES) * len(C.SWEEP_T) * len(C.SWEEP_F) * len(C.SWEEP_B) - len(C.SWEEP_F) * len(C.SWEEP_B)
    shapes = {(c["mode"], c["T"], c["F"], c["B"]) for c in cases}
    assert shapes == {s for s in itertools.product(C.MODES, C.SWEEP_T, C.SWEEP_F, C.SWEEP_B)
                      if not (s[0] == "central" and s[1] == 1)}
    factors = {"mode": C.MODES, "T": C.SWEEP_T, "F": C.SWEEP_F, "B": C.SWEEP_B, "window": [False, True],
               "scale": [False, True], "stacked": [False, True], "accum": ["none", "separate", "out"],
               "out_is_x": [False, True]}

    def possible(a, va, b, vb):
        pair = {a: va, b: vb}
        if pair.get("window") and pair.get("mode") in ("angle", "unwrap"):
            return False
        if pair.get("mode") == "central" and pair.get("T") == 1:
            return False
        return not (pair.get("accum") == "out" and pair.get("out_is_x"))
    missing = [(a, va, b, vb) for a, b in itertools.combinations(factors, 2) for va in factors[a] for vb in factors[b]
               if possible(a, va, b, vb) and not any(c[a] == va and c[b] == vb for c in cases)]
    assert not missing, missing


def test_grid_loop_shape_makes_the_threads_loop():
    B, T, F = C.GRID_LOOP_SHAPE
    most, least = C.loop_trips(B * T * F)
    assert least >= 3 and most == least + 1       # every thread loops at least three times, the last trip is partial
    assert C.grid_blocks(B * T * F) == C.GRID_CAP_BLOCKS
    src = open(os.path.join(ROOT, "acids_transforms_amd", "csrc", "repr_grad.hip")).read()
    m = re.search(r"kScanBwdMaxBlocks\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) * int(m.group(2)) == C.GRID_CAP_BLOCKS


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

NEW = ("at_phase_scan_backward", "at_cartesian_pack_backward")


def test_new_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
        assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert lib.at_abi_version() == 4 == _lib.ABI_VERSION


def _psb(lib, X=8, B=2, T=3, F=513, mode=1, g=8, ld_g=None, window=None, scale=None, accum=None, out=16):
    return lib.at_phase_scan_backward(X, B, T, F, mode, g, F if ld_g is None else ld_g, window, scale, accum, out, None)


def test_phase_scan_backward_rejects_bad_arguments_without_a_device():
    lib = _lib.lib()
    E, OK = _lib.AT_EINVAL, _lib.AT_OK
    assert _psb(lib, X=None) == E and _psb(lib, g=None) == E and _psb(lib, out=None) == E
    assert _psb(lib, B=-1) == E and _psb(lib, T=-1) == E and _psb(lib, F=-1) == E
    assert _psb(lib, ld_g=512) == E and _psb(lib, ld_g=-1, F=0) == E
    assert _psb(lib, mode=-1) == E and _psb(lib, mode=5) == E
    assert _psb(lib, mode=0, window=8) == E and _psb(lib, mode=4, window=8) == E      # angle / unwrap take no frame weight
    assert _psb(lib, X=12) == E and _psb(lib, out=12) == E and _psb(lib, accum=20) == E  # complex64 elements: 8 bytes
    assert _psb(lib, g=10) == E and _psb(lib, window=6) == E and _psb(lib, scale=9) == E  # floats: 4 bytes
    assert _psb(lib, mode=5, B=0) == E and _psb(lib, ld_g=1, T=0) == E                   # ... also when there is nothing to do
    for zero in ({"B": 0}, {"T": 0}, {"F": 0, "ld_g": 0}):
        assert _psb(lib, X=None, g=None, out=None, **zero) == OK
    assert _psb(lib, X=None, g=None, out=None, B=0, ld_g=1026, window=8, scale=8, accum=8) == OK


def test_cartesian_pack_backward_rejects_bad_arguments_without_a_device():
    lib = _lib.lib()
    E, OK = _lib.AT_EINVAL, _lib.AT_OK
    cart = lib.at_cartesian_pack_backward
    assert cart(None, 3, 513, None, None, 8, None) == E and cart(8, 3, 513, None, None, None, None) == E
    assert cart(8, -1, 513, None, None, 8, None) == E and cart(8, 3, -1, None, None, 8, None) == E
    assert cart(8, 3, 513, None, None, 12, None) == E                                   # complex64 alignment
    assert cart(10, 3, 513, None, None, 8, None) == E and cart(8, 3, 513, 6, None, 8, None) == E
    assert cart(8, 3, 513, None, 9, 8, None) == E
    assert cart(None, 0, 513, None, None, None, None) == OK and cart(None, 3, 0, None, None, None, None) == OK


def test_forward_functions_are_first_order_and_exported():
    from acids_transforms_amd import autograd as AG
    for name in ("AffineForwardFunction", "PhaseScanFunction", "CartesianFunction", "PolarFunction", "PolarIFFunction",
                 "StftPolarFunction"):
        assert name in AG.__all__ and issubclass(getattr(AG, name), torch.autograd.Function)

"""CPU side of the invert backward (at_magnitude_invert_backward, at_polar_to_complex_backward,
at_cartesian_unpack_backward; autograd.MagnitudeInvertFunction and its neighbours): the formulas the kernels implement
(invert_grad_cases.formula_*) against torch autograd of the reference's own expressions in float64, and the C ABI's
argument checks, which touch no device.

The formula tests run no line of the library: both sides are restatements in the test tree (they pin down the maths the
kernels and test_invert_grad_gpu.py are held to, and pass with or without the feature).  What guards the change on the
CPU are the tests of the exported symbols, the header, the binding and the AT_EINVAL / AT_OK answers below."""
import os
import re

import pytest
import torch

import acids_transforms_amd as A
import invert_grad_cases as C
from acids_transforms_amd import _lib
from conftest import rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRASTS = ["log1p", "log", "log10", None]
# (offset, scale) standing for the statistics scale_data would set, per norm mode
NORMS = {None: (None, None), "unipolar": (-1.25, 7.5), "bipolar": (2.5, 3.75), "gaussian": (0.8, 1.6)}
TOL = 1e-12


def _params(contrast, norm, keep_nyquist, mel=True):
    mod = A.Magnitude(n_fft=64, n_mels=12, mel=mel, contrast=contrast, mode=None, keep_nyquist=keep_nyquist)
    p = C.magnitude_params(mod)
    p["offset"], p["scale"] = NORMS[norm]
    return p


def _y(g, shape, p):
    """Features whose de-normalised value stays within +-2."""
    z = torch.rand(shape, generator=g, dtype=torch.float64) * 4 - 2
    return (z - p["offset"]) / p["scale"] if p["offset"] is not None else z


@pytest.mark.parametrize("keep_nyquist", [True, False])
@pytest.mark.parametrize("mel", [True, False])
@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("contrast", CONTRASTS)
def test_magnitude_invert_formula(contrast, norm, mel, keep_nyquist):
    p = _params(contrast, norm, keep_nyquist, mel)
    g = torch.Generator().manual_seed(3)
    K = (12 if mel else 33) - (0 if keep_nyquist else 1)
    y = _y(g, (2, 3, K), p)
    gout = torch.randn(2, 3, 33, generator=g, dtype=torch.float64)
    want = C.autograd_of(lambda t: C.ref_magnitude_invert(t, p), y, gout)
    got = C.formula_magnitude_invert(y.numpy(), gout.numpy(), p)
    assert got.shape == y.shape and rel_max(got, want.numpy()) < TOL


@pytest.mark.parametrize("ph_norm", [None, "bipolar"])
@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("contrast", CONTRASTS)
def test_polar_invert_formula(contrast, norm, ph_norm):
    mod = A.Magnitude(n_fft=64, contrast=contrast, mode=None)
    p = C.magnitude_params(mod)
    p["offset"], p["scale"] = NORMS[norm]
    po, ps = NORMS[ph_norm]
    g = torch.Generator().manual_seed(4)
    y = torch.stack([_y(g, (5, 33), p), torch.rand(5, 33, generator=g, dtype=torch.float64) * 2 - 1], -2)
    gX = torch.randn(5, 33, generator=g, dtype=torch.complex128)
    want = C.autograd_of(lambda t: C.ref_polar_invert(t, p, po, ps), y, gX)
    got = C.formula_polar_invert(y.numpy(), gX.numpy(), p, po, ps)
    assert rel_max(got[:, 0], want.numpy()[:, 0]) < TOL and rel_max(got[:, 1], want.numpy()[:, 1]) < TOL


def test_polar_to_complex_formula():
    g = torch.Generator().manual_seed(5)
    mag = torch.rand(4, 9, generator=g, dtype=torch.float64).requires_grad_()
    phase = (torch.rand(4, 9, generator=g, dtype=torch.float64) * 6.283 - 3.1415).requires_grad_()
    gX = torch.randn(4, 9, generator=g, dtype=torch.complex128)
    (mag * torch.exp(1j * phase)).backward(gX)
    gm, gp = C.formula_polar_to_complex(gX.numpy(), mag.detach().numpy(), phase.detach().numpy())
    assert rel_max(gm, mag.grad.numpy()) < TOL and rel_max(gp, phase.grad.numpy()) < TOL


@pytest.mark.parametrize("re_norm,im_norm", [(None, None), ("gaussian", "unipolar"), (None, "bipolar")])
def test_cartesian_invert_formula(re_norm, im_norm):
    g = torch.Generator().manual_seed(6)
    y = torch.randn(3, 2, 17, generator=g, dtype=torch.float64)
    gX = torch.randn(3, 17, generator=g, dtype=torch.complex128)
    want = C.autograd_of(lambda t: C.ref_cartesian_invert(t, NORMS[re_norm], NORMS[im_norm]), y, gX)
    got = C.formula_cartesian(gX.numpy(), NORMS[re_norm][1], NORMS[im_norm][1])
    assert rel_max(got, want.numpy()) < TOL


@pytest.mark.parametrize("keep_nyquist", [True, False])
def test_affine_invert_gradient_is_g_times_scale(keep_nyquist):
    g = torch.Generator().manual_seed(7)
    y = torch.randn(3, 16 if keep_nyquist else 15, generator=g, dtype=torch.float64)
    gout = torch.randn(3, 16, generator=g, dtype=torch.float64)
    want = C.autograd_of(lambda t: C.ref_affine_invert(t, 0.8, 1.6, keep_nyquist), y, gout)
    assert rel_max((gout[..., :y.shape[-1]] * 1.6).numpy(), want.numpy()) < TOL


NEW = ("at_magnitude_invert_backward", "at_polar_to_complex_backward", "at_cartesian_unpack_backward")


def test_new_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
        assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert lib.at_abi_version() == 4


def _mib(lib, y=8, rows=1, K=513, N=513, pad=0, g=8, polar=0, f=(None,) * 4, f_nnz=0, t=(8, 8, 8, 8), t_nnz=4, contrast=1,
         off=None, sc=None, po=None, ps=None, dy=8):
    return lib.at_magnitude_invert_backward(y, rows, K, N, pad, g, polar, *f, f_nnz, *t, t_nnz, contrast, off, sc, 1e-7,
                                            po, ps, dy, None)


def test_magnitude_invert_backward_rejects_bad_arguments_without_a_device():
    lib = _lib.lib()
    E = _lib.AT_EINVAL
    assert _mib(lib, y=None) == E and _mib(lib, g=None) == E and _mib(lib, dy=None) == E
    assert _mib(lib, rows=-1) == E and _mib(lib, K=0) == E and _mib(lib, N=0) == E
    assert _mib(lib, contrast=4) == E and _mib(lib, pad=2) == E and _mib(lib, polar=2) == E
    assert _mib(lib, off=8) == E and _mib(lib, sc=8) == E                       # offset and scale come as a pair
    assert _mib(lib, po=8, ps=8) == E                                           # a phase affine without the polar form
    assert _mib(lib, t=(8, 8, None, 8)) == E and _mib(lib, t_nnz=0) == E        # incomplete tables
    assert _mib(lib, t=(None,) * 4, t_nnz=0, N=128) == E                        # mel=False needs N == K
    assert _mib(lib, polar=1) == E                                              # the polar form needs the bank's tables
    assert _mib(lib, polar=1, f=(8, 8, 8, 8), f_nnz=4, K=128) == E              # ... and a square bank
    assert _mib(lib, polar=1, f=(8, 8, 8, 8), f_nnz=4, pad=1) == E              # ... without the pad
    assert _mib(lib, polar=1, f=(8, 8, 8, 8), f_nnz=4, t=(None,) * 4, t_nnz=0) == E
    assert _mib(lib, y=10) == E and _mib(lib, g=10) == E and _mib(lib, dy=6) == E   # float alignment
    assert _mib(lib, polar=1, f=(8, 8, 8, 8), f_nnz=4, g=12) == E               # a complex gradient: 8 bytes
    assert _mib(lib, off=6, sc=8) == E and _mib(lib, off=8, sc=10) == E         # the scalars: float alignment
    assert _mib(lib, rows=0, y=None, g=None, dy=None) == _lib.AT_OK
    assert _mib(lib, rows=0, y=None, g=None, dy=None, polar=1, f=(8, 8, 8, 8), f_nnz=4) == _lib.AT_OK


def test_pointwise_backwards_reject_bad_arguments_without_a_device():
    lib = _lib.lib()
    E, OK = _lib.AT_EINVAL, _lib.AT_OK
    p2c, cart = lib.at_polar_to_complex_backward, lib.at_cartesian_unpack_backward
    assert p2c(None, 8, 8, 4, 8, 8, None) == E and p2c(8, 8, None, 4, 8, 8, None) == E
    assert p2c(8, None, 8, 4, 8, 8, None) == E          # gphase needs mag
    assert p2c(12, 8, 8, 4, 8, 8, None) == E            # complex64 alignment
    assert p2c(8, 10, 8, 4, 8, 8, None) == E and p2c(8, 8, 6, 4, 8, 8, None) == E       # float alignment
    assert p2c(8, 8, 8, 4, 9, 8, None) == E and p2c(8, 8, 8, 4, 8, 10, None) == E
    assert p2c(8, 8, 8, -1, 8, 8, None) == E
    assert p2c(None, None, None, 0, None, None, None) == OK
    assert p2c(8, 8, 8, 4, None, None, None) == OK      # neither gradient wanted: nothing to do
    assert cart(None, 3, 513, None, None, 8, None) == E and cart(8, 3, 513, None, None, None, None) == E
    assert cart(8, 3, 0, None, None, 8, None) == E and cart(8, -1, 513, None, None, 8, None) == E
    assert cart(12, 3, 513, None, None, 8, None) == E
    assert cart(8, 3, 513, None, None, 10, None) == E and cart(8, 3, 513, 6, None, 8, None) == E
    assert cart(8, 3, 513, None, 9, 8, None) == E
    assert cart(None, 0, 513, None, None, None, None) == OK


def test_invert_functions_are_first_order_and_exported():
    from acids_transforms_amd import autograd as AG
    for name in ("MagnitudeInvertFunction", "PolarInvertFunction", "CartesianInvertFunction", "PolarToComplexFunction",
                 "AffineInvertFunction"):
        assert name in AG.__all__ and issubclass(getattr(AG, name), torch.autograd.Function)

"""CPU side of PQMF (csrc/pqmf.hip, autograd.PqmfFunction / PqmfInvertFunction, transforms/pqmf.py): the C ABI entries and
their argument checks, the host-side design against the float64 restatement of pqmf_cases.py, the sanity of the
definition itself in float64, and what the module does without a GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import pqmf_cases as C
from acids_transforms_amd import _lib, autograd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("at_pqmf_tile_blocks", "at_pqmf_analysis", "at_pqmf_synthesis")


def test_entries_are_exported_declared_and_bound():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "acids_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert lib.at_abi_version() == 4                            # additive: the ABI version stays
    for op in ("pqmf_tile_blocks", "pqmf_analysis", "pqmf_synthesis"):
        assert op in dir(A.ops)


@pytest.mark.parametrize("entry", ["at_pqmf_analysis", "at_pqmf_synthesis"])
def test_argument_checks_answer_before_any_launch(entry):
    fn = getattr(_lib.lib(), entry)
    E, U, OK = _lib.AT_EINVAL, _lib.AT_EUNSUPPORTED, _lib.AT_OK
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(256)              # never dereferenced: every call below answers before a launch

    def call(rows, L, taps, n_band, p=null):
        return fn(p, rows, L, p, taps, n_band, p, 1.0, p, null)

    # nothing to do: AT_OK before any pointer check, whatever the rest says
    assert call(0, 64, 513, 16) == OK and call(3, 0, 513, 16) == OK and call(0, 0, 4, 1000) == OK
    # AT_EINVAL: L no multiple of n_band, even taps, taps below 2 n_band + 1, negative sizes
    assert call(1, 65, 513, 16, fake) == E
    assert call(1, 64, 512, 16, fake) == E
    assert call(1, 64, 31, 16, fake) == E and call(1, 64, 3, 2, fake) == E
    assert call(-1, 64, 513, 16, fake) == E and call(1, -64, 513, 16, fake) == E and call(1, 64, 513, 0, fake) == E
    # AT_EUNSUPPORTED: outside n_band 2 .. 64 and taps <= 4097, pointers or not
    assert call(1, 64, 513, 1) == U and call(1, 130, 513, 65) == U and call(1, 64, 4099, 16, fake) == U
    # a legal shape with null pointers
    assert call(1, 64, 513, 16) == E and call(1, 10, 5, 2) == E


def test_tile_blocks_over_the_supported_range():
    tb = _lib.lib().at_pqmf_tile_blocks
    for n_band in range(2, 65):
        for taps in (2 * n_band + 1, 32 * n_band + 1 if 32 * n_band + 1 <= 4097 else 4097, 4097):
            tile = tb(n_band, taps)
            assert tile > 0 and tile % 8 == 0, (n_band, taps, tile)
            assert A.ops.pqmf_tile_blocks(n_band, taps) == tile
    assert tb(16, 512) == _lib.AT_EINVAL and tb(16, 31) == _lib.AT_EINVAL and tb(0, 513) == _lib.AT_EINVAL
    assert tb(1, 513) == _lib.AT_EUNSUPPORTED and tb(65, 513) == _lib.AT_EUNSUPPORTED
    assert tb(16, 4099) == _lib.AT_EUNSUPPORTED
    with pytest.raises(A.AcidsHipError):
        A.ops.pqmf_tile_blocks(65, 513)


@pytest.fixture(scope="module")
def designs():
    return {d: A.PQMF(n_band=d[0], taps=d[1], attenuation=d[2]) for d in C.DESIGNS}


@pytest.mark.parametrize("design", C.DESIGNS)
def test_design_matches_the_restatement(designs, design):
    n_band, taps, att = design
    pq = designs[design]
    N = taps if taps is not None else C.default_taps(n_band)
    assert pq.taps == N and pq.n_band == n_band and pq.prototype.shape == (N,) and pq.prototype.dtype == torch.float32
    # the cutoff is a grid point
    grid = C.grid(n_band)
    i = int(np.argmin(np.abs(grid - pq.cutoff)))
    assert abs(grid[i] - pq.cutoff) <= 1e-15 * grid[i]
    # the prototype is the restatement at the module's own cutoff
    want = C.prototype(pq.cutoff, N, att)
    assert C.rel_max(pq.prototype.numpy(), want) <= 1e-6
    # and that cutoff minimises the restated objective over the whole grid (near-tied grid points may swap)
    phis = C.phi_grid(n_band, N, att)
    assert C.phi(want, n_band) <= (1 + 1e-6) * phis.min()
    # the modulation is C rounded to fp32
    assert pq.modulation.shape == (n_band, 2 * n_band) and pq.modulation.dtype == torch.float32
    assert np.array_equal(pq.modulation.numpy(), C.modulation(n_band, N).astype(np.float32))


def test_default_cutoff_is_the_recorded_one(designs):
    pq = designs[C.DESIGNS[0]]
    assert abs(pq.cutoff * 16 / math.pi - 0.53467) < 5e-5


@pytest.mark.parametrize("n_band", [4, 16])
def test_definition_round_trip_and_transpose_in_float64(n_band):
    N = C.default_taps(n_band)
    grid = C.grid(n_band)
    w = float(grid[int(np.argmin(C.phi_grid(n_band, N, 100.0)))])
    hk = C.bank(C.prototype(w, N, 100.0), n_band)
    L = n_band * ((4 * N) // n_band + 8)
    x = C.audio((2, L), 1)
    y = C.analysis(x, hk)
    assert y.shape == (2, n_band, L // n_band)
    xh = C.synthesis(y, hk)
    assert xh.shape == x.shape
    err = C.interior_rel_rms(xh.numpy(), x.numpy(), N)
    print("n_band %d taps %d: interior relative rms of the float64 round trip %.3e" % (n_band, N, err))
    assert err < 1e-2                  # near-perfect reconstruction: a condition on the design (measured 9e-4 .. 1.2e-3)
    # the folded form the kernels compute is the direct convolution
    M2, P = 2 * n_band, (N - 1) // 2
    G = -(-N // M2)
    hp = np.zeros(G * M2)
    hp[:N] = C.prototype(w, N, 100.0)
    xp = np.zeros(L + 2 * G * M2)
    xp[P:P + L] = x[0].numpy()
    t = 7
    u = np.array([sum((-1) ** j * hp[r + M2 * j] * xp[t * n_band + r + M2 * j] for j in range(G)) for r in range(M2)])
    folded = C.modulation(n_band, N) @ u
    assert np.abs(folded - y[0, :, t].numpy()).max() <= 1e-12 * np.abs(y[0, :, t].numpy()).max()
    # transpose identity: <A x, g> = <x, S g> / M
    g = C.audio(tuple(y.shape), 2)
    lhs, rhs = float((y * g).sum()), float((x * C.synthesis(g, hk)).sum()) / n_band
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), float(y.norm() * g.norm()))


@pytest.mark.parametrize("n_band,taps,T", [(2, 5, 1), (3, 51, 7), (5, 11, 40), (16, 257, 9)])
def test_the_two_readings_of_synthesis_agree(n_band, taps, T):
    hk = C.bank(C.prototype(math.pi / (2 * n_band) * 1.1, taps, 80.0), n_band)
    y = C.audio((2, 3, n_band, T), 5)
    got, want = C.synthesis(y, hk), C.synthesis_stuffed(y, hk)
    assert got.shape == want.shape == (2, 3, n_band * T)
    assert C.rel_max(got.numpy(), want.numpy()) <= 1e-13


def test_constructor_and_shape_errors():
    for bad in (1, 0, 65, -3):
        with pytest.raises(ValueError):
            A.PQMF(n_band=bad)
    with pytest.raises(ValueError):
        A.PQMF(n_band=4, taps=64)             # even
    with pytest.raises(ValueError):
        A.PQMF(n_band=4, taps=7)              # below 2 n_band + 1
    with pytest.raises(ValueError):
        A.PQMF(n_band=4, taps=4099)           # past the kernels' range
    with pytest.raises(ValueError):
        A.PQMF(n_band=4, prototype=torch.ones(64))
    with pytest.raises(ValueError):
        A.PQMF(n_band=4, prototype=torch.ones(3, 65))
    pq = A.PQMF(n_band=4, taps=65)
    with pytest.raises(ValueError):
        pq(torch.zeros(2, 1001))              # L % n_band
    with pytest.raises(ValueError):
        pq.invert(torch.zeros(2, 5, 100))     # a wrong band axis
    with pytest.raises(ValueError):
        pq.invert(torch.zeros(100))
    # no CPU route, and no silent narrowing
    with pytest.raises(A.AcidsHipError):
        pq(torch.zeros(2, 1000))
    with pytest.raises(A.AcidsHipError):
        pq.invert(torch.zeros(2, 4, 250))
    with pytest.raises(A.AcidsHipError):
        pq(torch.zeros(2, 1000, dtype=torch.float64))


def test_module_surface():
    pq = A.PQMF(n_band=4, taps=65)
    assert isinstance(pq, A.AudioTransform) and A.PQMF is A.pqmf.PQMF and A.pqmf is A.transforms.pqmf
    assert "PQMF" in A.transforms.__all__
    assert (A.PQMF.invertible, A.PQMF.needs_scaling, A.PQMF.scriptable) == (True, False, False)
    assert pq.ratio == 4 and A.PQMF().ratio == 16 and A.PQMF().taps == 513
    assert repr(pq).startswith("PQMF(n_band=4, taps=65")
    assert sorted(k for k, _ in pq.named_buffers()) == ["modulation", "prototype"]
    # no streaming form: realtime() says so and hands back the offline module (the replayed reference suite drives
    # realtime().test_forward of every transform, so it cannot raise)
    with pytest.warns(UserWarning, match="no streaming form"):
        assert pq.realtime() is pq
    # the self-test hooks cut their audio to whole blocks; forward itself refuses
    assert pq._whole_blocks(torch.zeros(2, 1003)).shape == (2, 1000)
    # a user prototype replaces the design
    h = torch.from_numpy(C.prototype(0.4, 33, 60.0))
    user = A.PQMF(n_band=4, taps=999, prototype=h)
    assert user.taps == 33 and user.cutoff is None and torch.equal(user.prototype, h.float())
    # composes with +
    chain = pq + A.PQMF(n_band=2, taps=9)
    assert isinstance(chain, A.ComposeAudioTransform) and chain.ratio == 8
    for name in ("PqmfFunction", "PqmfInvertFunction"):
        assert name in autograd.__all__ and issubclass(getattr(autograd, name), torch.autograd.Function)

"""CPU side of the plan-class sweep (sweep_cases.py): that the class functions restate the library's own plans
(at_pqmf_tile_blocks, at_resample_backward_plan, at_sinc_interp_plan, at_sos_hop_power_plan, at_fft_convolve_plan), which
classes each stage's table reached before the sweep and that the sweep's cases leave none, that every case is accepted, that
the generator repeats itself, and that the float64 models of the named cases agree with a second route."""
import numpy as np
import pytest
import torch
from scipy.signal import sosfilt as scipy_sosfilt

import acids_transforms_amd as A
import convolve_stream_cases as CS
import fft_convolve_cases as FC
import loudness_cases as LC
import pqmf_cases as PC
import pqmf_stream_cases as PS
import resample_cases as RC
import sinc_interp_cases as SI
import sos_filter_cases as SC
import sweep_cases as W
from acids_transforms_amd import _lib, ops


def _union(sets):
    out = set()
    for s in sets:
        out |= s
    return out


def _pq_cases(pairs):
    return [(M, N, T) for M, N in pairs for T in PC.block_counts(W.pqmf_plan(M, N)["TB"])]


def _fir_table():
    """(P, T) of every case of fft_convolve_cases.py, from the library's plan."""
    shapes = [(L, K, FC.BLOCK) for L in FC.LENGTHS for K in FC.TAPS] + [(L, K, FC.BLOCK) for L, K in FC.TILE_CASES]
    shapes += [(L, K, block) for L, K, _, block in FC.BLOCK_CASES] + [FC.LONG_CASE[:2] + (None,)]
    return sorted({ops.fft_convolve_plan(*s)[2:0:-1] for s in shapes})


# ---- 1. what the tables reached before the sweep -----------------------------------------------------------------------------
def test_the_tables_miss_exactly_these_classes():
    pq = _union(W.pqmf_classes(*c) for c in _pq_cases(sorted(set(PC.PARITY) | set(PC.SPECIALISED) | set(PS.CASES))))
    assert W.PQ_UNIVERSE - pq == {"G%4=0", "M>=32,G<4"} and pq <= W.PQ_UNIVERSE
    rb = _union(W.resample_classes(*r) for r in RC.RATIOS)
    assert W.RB_UNIVERSE - rb == {"tile=shrunk", "tile=one block"} and rb <= W.RB_UNIVERSE
    si = _union(W.sinc_classes(*SI.reduced(*r)) for r in SI.RATIOS + (SI.BIG, SI.MID))
    assert W.SI_UNIVERSE - si == {"fwd:tile=shrunk", "bwd:tile=shrunk"} and si <= W.SI_UNIVERSE
    hop = _union(W.hop_classes(L, h) for L in LC.PARITY_LENGTHS for h in LC.HOPS if L // h)
    assert W.HOP_UNIVERSE - hop == {"wave<=hop<tile", "hop holds a tile", "tiles>=5", "tiles>=5, hop wraps"}
    assert hop <= W.HOP_UNIVERSE
    table = _fir_table()
    assert {P for P, _ in table} == {1, 2, 3, 8, 20}
    fir = _union(W.fir_classes(P, T) for P, T in table)
    assert W.FIR_UNIVERSE - fir == ({"P%%8=%d" % i for i in (5, 6, 7)} | {"P>8,P%%8=%d" % i for i in (0, 1, 2, 3, 5, 6, 7)})
    assert fir <= W.FIR_UNIVERSE
    # the streaming tables: the same band counts and ratios, and partition counts of their own
    assert set(PS.CASES) <= set(PC.PARITY) | set(PC.SPECIALISED) and set(RC.STREAM_RATIOS) <= set(RC.RATIOS)
    assert sorted({-(-K // CS.BLOCK) for K in CS.TAPS}) == [1, 2, 3, 8, 9, 18]
    for name, missed in (("PQMF", W.PQ_UNIVERSE - pq), ("Resample backward", W.RB_UNIVERSE - rb), ("sinc converter", W.SI_UNIVERSE - si),
                         ("hop endings", W.HOP_UNIVERSE - hop), ("spectral FIR", W.FIR_UNIVERSE - fir)):
        print("%s: the table missed %s" % (name, sorted(missed)))


# ---- 2. the sweep leaves none ---------------------------------------------------------------------------------------------------
def test_named_and_generated_cases_reach_every_class():
    assert _union(W.pqmf_classes(*c) for c in _pq_cases(W.PQ_NAMED + W.pqmf_generated())) == W.PQ_UNIVERSE
    assert _union(W.resample_classes(*r) for r in W.RB_NAMED + W.resample_generated()) == W.RB_UNIVERSE
    assert _union(W.sinc_classes(*r) for r in W.SI_NAMED + W.sinc_generated()) == W.SI_UNIVERSE
    assert _union(W.hop_classes(L, h) for L, h in W.HOP_NAMED + W.hop_generated()) == W.HOP_UNIVERSE
    assert _union(W.fir_classes(P, T) for P, T in W.FIR_NAMED + W.fir_generated()) == W.FIR_UNIVERSE
    # and each gap of the tables has a NAMED case of its own
    named = _union(W.pqmf_classes(*c) for c in _pq_cases(W.PQ_NAMED))
    assert {"G%4=0", "M>=32,G<4", "G<4", "copy=own", "copy=general", "P%M=0"} <= named
    assert [W.pqmf_plan(M, N)["G"] for M, N in W.PQ_NAMED] == [4, 8, 5, 4, 2, 2, 2]
    assert [W.resample_plan(*r)[::2] for r in W.RB_NAMED[:3]] == [(512, 1024), (128, 1024), (25, 51)]
    assert W.resample_plan(1025, 1024) == (1, False, 1) and W.resample_classes(1025, 1024) >= {"tile=one block", "bank=global"}
    tiles = [(W.sinc_plan(a, b, W.sinc_qi(a, b))[0], W.sinc_plan(b, a, W.sinc_qi(a, b))[0]) for a, b in W.SI_NAMED[:4]]
    assert tiles == [(512, 1024), (128, 1024), (256, 1024), (512, 1024)]
    assert {"fwd:tile=shrunk", "fwd:table=global"} <= W.sinc_classes(22050, 689)
    assert {"bwd:tile=shrunk", "bwd:table=global"} <= W.sinc_classes(689, 22050)
    for n_steps, rates in zip(W.PITCH_STEPS, ((32, 1), (689, 22050))):
        assert SI.reduced(SI.pitch_rates(44100, n_steps)[1], 44100) == rates
        A.PitchShift(44100, n_steps)                                              # the argument checks admit both
    assert {"wave<=hop<tile", "hop holds a tile", "tiles>=5", "tiles>=5, hop wraps", "hop wave-aligned"} <= _union(
        W.hop_classes(L, h) for L, h in W.HOP_NAMED)
    assert W.fir_classes(9, 9) >= {"P>8,P%8=1"} and W.fir_classes(16, 8) >= {"P>8,P%8=0", "T=8"} and "P%8=7" in W.fir_classes(7, 7)
    assert [tuple(T for _, T in W.fir_lengths(P)) for P in W.FIR_NAMED_P] == [(7, 8, 9), (9,), (16, 17, 18), (17, 18, 19)]


# ---- 3. every case is accepted, and the restatement is the library's plan ----------------------------------------------------------
def test_every_case_is_accepted_and_the_restatements_are_the_librarys_plans():
    pairs = sorted(set(PC.PARITY) | set(PC.SPECIALISED)) + list(W.PQ_NAMED + W.pqmf_generated() + W.pqmf_random_pairs(300))
    assert len(W.pqmf_random_pairs(300)) == 300
    for M, N in pairs:
        p = W.pqmf_plan(M, N)
        assert p is not None and ops.pqmf_tile_blocks(M, N) == p["TB"], (M, N)
        assert 2 <= M <= 64 and 2 <= p["G"] <= 17
    lib = _lib.lib()
    for M, N in ((64, 4097), (64, 4099), (65, 131), (1, 3), (4, 7), (4, 10)):    # the edges of what is accepted, both ways
        assert (lib.at_pqmf_tile_blocks(M, N) > 0) == (W.pqmf_plan(M, N) is not None), (M, N)
    for r in RC.RATIOS + W.RB_NAMED + W.resample_generated():
        width = RC.bank(*r)[1]
        assert width == W.resample_width(*r) and RC.plan(*r) == W.resample_plan(*r)[:2], r
        lead = RC.stream_sizes(*r)[1]                                             # a stream's backward: lead = Ha
        assert RC.plan(*r, lead=lead) == W.resample_plan(*r, lead=lead)[:2], r
    for r in tuple(SI.reduced(*q) for q in SI.RATIOS + (SI.BIG, SI.MID)) + W.SI_NAMED + W.sinc_generated():
        Qi = SI.table(*r)[1]
        assert Qi == W.sinc_qi(*r), r
        for a, b in (r, r[::-1]):
            assert SI.plan(a, b, Qi) == W.sinc_plan(a, b, Qi), (a, b, Qi)
    for L, hop in W.HOP_NAMED + W.hop_generated():
        # (the named hop 9000 at tile + 1 samples has no whole hop: an empty result, which is a case too)
        assert 16 <= hop <= 10000 and (L // hop >= 1 or (L, hop) == (W.SOS_TILE + 1, 9000))
        for name in W.HOP_FILTERS:
            n = SC.FILTERS[name].shape[0]
            assert ops.sos_hop_power_plan(3, L, n, hop) == W.hop_plan(L, hop)[:2] + (0,)
    assert W.hop_plan(100, 15) is None and W.hop_plan(100, 16) is not None
    with pytest.raises(A.AcidsHipError):
        ops.sos_hop_power_plan(1, 100, 2, 15)
    for P in W.FIR_NAMED_P:
        for L, T in W.fir_lengths(P):
            assert ops.fft_convolve_plan(L, P * W.FIR_BLOCK, W.FIR_BLOCK)[:4] == W.fir_plan(L, P * W.FIR_BLOCK, W.FIR_BLOCK) \
                == (W.FIR_BLOCK, T, P, W.FIR_TILE)
    for P, T in W.FIR_NAMED + W.fir_generated():
        assert 1 <= P <= 24 and 1 <= T <= 17
        L = (T - 1) * W.FIR_BLOCK + 1                                             # the same (P, T) as a convolution, where T >= P
        K = (P - 1) * W.FIR_BLOCK + 1
        if L - K + 1 >= 1:
            assert ops.fft_convolve_plan(L - K + 1, K, W.FIR_BLOCK)[1:4] == (T, P, W.FIR_TILE)
    assert ops.fft_convolve_stream_plan(9 * W.FIR_BLOCK, W.FIR_BLOCK)[3] == W.FIR_TILE == FC.FRAME_TILE


# ---- 4. the generator repeats itself --------------------------------------------------------------------------------------------
def test_the_generator_returns_the_same_cases_again():
    for gen in (W.pqmf_generated, W.resample_generated, W.sinc_generated, W.hop_generated, W.fir_generated, W.pqmf_random_pairs):
        first, second = gen(), gen()
        assert first == second and len(first) == (300 if gen is W.pqmf_random_pairs else W.GENERATED)
        assert len(set(first)) == len(first) or gen is W.pqmf_random_pairs
    assert W.chunk_lists((4, 31), 256) == W.chunk_lists((4, 31), 256) != W.chunk_lists((4, 63), 256)
    for lists in (W.chunk_lists((7, 57), 128), W.chunk_lists((1,), 1)):
        assert len(lists) == 3 and all(len(c) == 4 for c in lists)
    assert all(1 <= c <= 129 for cs in W.chunk_lists((7, 57), 128) for c in cs)
    assert {c for cs in W.chunk_lists((1,), 1, lists=20) for c in cs} == {1, 2}


# ---- 5. the float64 models of the named cases against a second route -------------------------------------------------------------
@pytest.mark.parametrize("n_band,taps", W.PQ_NAMED)
def test_pqmf_synthesis_is_the_stuffed_convolution(n_band, taps):
    pq = A.PQMF(n_band=n_band, taps=taps)
    hk = PC.bank(pq.prototype.numpy(), n_band)
    tile = W.pqmf_plan(n_band, taps)["TB"]
    worst = 0.0
    for i, T in enumerate((1, 2, tile + 1)):
        y = PC.audio((2, n_band, T), 900 + i)
        worst = max(worst, PC.rel_max(PC.synthesis(y, hk).numpy(), PC.synthesis_stuffed(y, hk).numpy()))
    print("n_band %d taps %d: scatter against the stuffed convolution %.2e" % (n_band, taps, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("orig,new", W.SI_BANK_BUILDABLE)
def test_the_gather_is_the_conv1d_model_where_a_tile_shrinks(orig, new):
    lengths = SI.lengths(orig, new)
    worst = 0.0
    for L in sorted({lengths[0], lengths[len(lengths) // 2], lengths[-1]}):
        x = SI.audio((2, L), 910 + L)
        worst = max(worst, SI.rel_max(SI.model(x.numpy(), orig, new), RC.model(x, orig, new).numpy()))
    print("(%d, %d): gather against the conv1d model %.2e" % (orig, new, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("name", W.HOP_FILTERS)
def test_hop_power_of_the_recurrence_is_scipys(name):
    """sos_filter_cases.sosfilt (the oracle of the filter's tests) squared and summed per hop against loudness_cases.hop_power
    (scipy.signal.sosfilt, the oracle of the hop powers) at every named (L, hop).  Both run scipy's recurrence in float64; the
    docstring of sos_filter_cases.py puts that recurrence 6e-12 from an 80-bit run, and a square doubles a relative error:
    1e-10 bounds the distance of two such runs with room to spare."""
    sos = SC.FILTERS[name]
    worst = 0.0
    for L in W.HOP_LENGTHS:
        x = np.random.default_rng(920 + L).standard_normal((2, L))
        y = SC.sosfilt(sos, x)[0]
        assert SC.rel_max(y, scipy_sosfilt(np.array(sos), x, axis=-1)) < 1e-10
        for hop in W.HOP_NAMED_HOPS:
            nh = L // hop
            got = (y[:, :nh * hop].reshape(2, nh, hop) ** 2).sum(-1)
            worst = max(worst, LC.rel_max(got, LC.hop_power(sos, x, hop)))
    print("%s: hop power of the numpy recurrence against scipy's %.2e" % (name, worst))
    assert worst < 1e-10


def test_spectral_fir_references_are_the_convolution():
    """fft_convolve_cases.partitioned (the float64 loop the kernels are held to) against numpy.convolve at the named counts."""
    worst = 0.0
    for P in W.FIR_NAMED_P:
        K = P * W.FIR_BLOCK
        for L, _ in W.fir_lengths(P):
            d = FC.data(L, K, 3)
            for h in (d["h"], d["hr"]):
                got = FC.partitioned(torch.from_numpy(d["x"]).double(), torch.from_numpy(h).double(), W.FIR_BLOCK).numpy()
                worst = max(worst, FC.rel_max(got, FC.oracle(d["x"], h)))
    print("partitioned float64 against numpy.convolve %.2e" % worst)
    assert worst < 1e-12

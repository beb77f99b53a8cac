"""GPU side of the streaming R128 meter and of loudness range (ops.sos_hop_power_stream, ops.loudness_range,
transforms.RealtimeLoudness; csrc/sos_filter.hip's stream ending, csrc/loudness.hip's strided gate and range kernel) against
the float64 oracle of loudness_stream_cases.py: the stream ending's hop powers, open sum and filter state within the
library's normwise bound 1e-5 from a mid-stream state at every hop, fill and chunk length around the hop's end and the tile
cuts; chunk lists against the oracle and the one-call hop powers; the bit rules (batch, aliasing, NaN, zeros, guard bands);
the module under four chunkings within 1e-4 LU of the oracle and of the offline module; the range within 2e-4 LU and its
select exact.

Measured on an MI355X (worst figures, printed by the tests): see README, "RealtimeLoudness"."""

import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import loudness_cases as C
import loudness_stream_cases as S
import sos_filter_cases as F
from acids_transforms_amd import _lib, ops
from acids_transforms_amd.utils import filter_design as fd

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
KW = fd.k_weighting(S.SR)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _lu_error(got, ref_lufs, ref_p):
    """The worst distance in LU between block loudnesses; blocks below -100 LUFS in the reference are compared in power,
    against the power of -100 LUFS, on the same scale (test_loudness_gpu.py's measure)."""
    got, ref_lufs, ref_p = np.asarray(got, np.float64), np.asarray(ref_lufs), np.asarray(ref_p)
    assert got.shape == ref_lufs.shape, (got.shape, ref_lufs.shape)
    silent = ref_p == 0.0
    assert np.array_equal(np.isneginf(got), silent)
    loud = ~silent & (ref_lufs >= -100.0)
    quiet = ~silent & ~loud
    worst = float(np.abs(got[loud] - ref_lufs[loud]).max()) if loud.any() else 0.0
    if quiet.any():
        floor = 10.0 ** ((-100.0 + 0.691) / 10.0)
        rel = np.abs(10.0 ** ((got[quiet] + 0.691) / 10.0) - ref_p[quiet]) / floor
        worst = max(worst, float(10.0 * np.log10(1.0 + rel.max())))
    return worst


def _step(xd, sos, hop, filled, zi, open_in, first=2, pad=3):
    """One kernel call on copies of the state: (power (rows, ld) with its sentinel, done, zf, open_out)."""
    done = (filled + xd.shape[-1]) // hop
    power = torch.full(tuple(xd.shape[:-1]) + (first + done + pad,), SENTINEL, dtype=torch.float64, device=xd.device)
    zf, out = zi.clone(), open_in.clone()
    assert ops.sos_hop_power_stream(xd, sos, hop, filled, zf, out, power, first) == done
    return power, done, zf, out


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------

def _chunk_lengths(hop, filled):
    return sorted({1, hop - filled - 1, hop - filled, S.TILE - 1, S.TILE, S.TILE + 1, 2 * S.TILE + 5} - {0})


def _midstream(name):
    """A state taken from the oracle mid-stream, 2100 rows: (x (2100, 2 TILE + 5) float32, zi after a prefix of 5000 samples,
    the squares of the prefix's output, the squares of x's output from zi, n -> zf after n samples of x).  The output of a
    chunk of n samples is the first n samples of the longest chunk's, and its state comes from one pass cut at every n
    (chunked sosfilt is the whole call: test_loudness_stream_cpu.py)."""
    from scipy.signal import sosfilt
    sos = np.array(F.FILTERS[name], dtype=np.float64)
    rng = np.random.default_rng(len(name))
    pre = rng.standard_normal((2100, 5000)).astype(np.float32)
    x = rng.standard_normal((2100, 2 * S.TILE + 5)).astype(np.float32)
    y, z = sosfilt(sos, pre.astype(np.float64), axis=-1, zi=np.zeros((sos.shape[0], 2100, 2)))
    presq, zi = y * y, np.ascontiguousarray(np.moveaxis(z, 0, -2))
    cuts = sorted({n for hop in S.STREAM_HOPS for filled in (0, 1, hop - 1) for n in _chunk_lengths(hop, filled)})
    sq, zf, at = np.empty(x.shape), {}, 0
    for n in cuts:
        y, z = sosfilt(sos, x[:, at:n].astype(np.float64), axis=-1, zi=z)
        sq[:, at:n] = y * y
        zf[n], at = np.ascontiguousarray(np.moveaxis(z, 0, -2)), n
    return x, zi, presq, sq, zf


@pytest.mark.parametrize("name", ("kweighting", "cascade4"))
def test_stream_ending_matches_the_oracle_from_a_midstream_state(dev, name):
    """Hops 16, 17, 800, 4097; the open hop empty, holding one sample, and one short of full; chunks of 1 sample, one short of
    closing the hop, closing it exactly, and around the tile cuts; 2100 rows (the persistent workgroups' second turn), and
    rows alone and in a batch of 3 with the bits they have among the 2100; guard bands keep their sentinel."""
    sos = F.FILTERS[name]
    x, zi, presq, sq, ref_zf = _midstream(name)
    xd, zid = _dev(x, dev), _dev(zi, dev)
    worst = dict(power=0.0, open=0.0, zf=0.0)
    for hop in S.STREAM_HOPS:
        for filled in (0, 1, hop - 1):
            open_in = presq[:, presq.shape[1] - filled:].sum(-1)
            opd = _dev(open_in, dev)
            for n in _chunk_lengths(hop, filled):
                chunk = xd[:, :n].contiguous()
                power, done, zf, out = _step(chunk, sos, hop, filled, zid, opd)
                ref_p, ref_open = S.step_from_squares(sq[:, :n], hop, filled, open_in)
                got, o = power.cpu().numpy(), out.cpu().numpy()
                assert done == ref_p.shape[-1]
                assert np.all(got[:, :2] == SENTINEL) and np.all(got[:, 2 + done:] == SENTINEL), (hop, filled, n)
                if done:
                    worst["power"] = max(worst["power"], C.rel_max(got[:, 2:2 + done], ref_p))
                worst["open"] = max(worst["open"], C.rel_max(o, ref_open))
                worst["zf"] = max(worst["zf"], C.rel_max(zf.cpu().numpy(), ref_zf[n]))
                if (filled + n) % hop == 0:
                    assert np.all(o == 0.0) and not np.signbit(o).any()
                for rows in (slice(0, 1), slice(2047, 2050)):           # a row alone, three rows: the bits of the batch
                    p1, _, z1, o1 = _step(chunk[rows].contiguous(), sos, hop, filled, zid[rows].contiguous(), opd[rows].contiguous())
                    assert torch.equal(p1, power[rows]) and torch.equal(z1, zf[rows]) and torch.equal(o1, out[rows]), (hop, filled, n)
    print("%s: stream ending power %.2e, open sum %.2e, state %.2e" % (name, worst["power"], worst["open"], worst["zf"]))
    assert max(worst.values()) <= S.TOL


# ---- chunk lists ---------------------------------------------------------------------------------------------------------

def _run_list(xd, sos, chunks, hop, cap):
    lead = tuple(xd.shape[:-1])
    zi = torch.zeros(lead + (np.asarray(sos).shape[0], 2), dtype=torch.float64, device=xd.device)
    op = torch.zeros(lead, dtype=torch.float64, device=xd.device)
    hist = torch.full(lead + (cap,), SENTINEL, dtype=torch.float64, device=xd.device)
    seen = 0
    for n in chunks:
        seen += n
        ops.sos_hop_power_stream(xd[..., seen - n:seen], sos, hop, (seen - n) % hop, zi, op, hist, (seen - n) // hop)
    return hist, zi, op, seen


@pytest.mark.parametrize("chunks", [S.chunk_list(s, 5 * S.TILE + 77) for s in (1, 2, 3)] + [[1] * 50],
                         ids=("seed1", "seed2", "seed3", "ones"))
def test_chunk_lists_against_the_oracle_and_the_one_call(dev, chunks):
    hop = 17 if len(chunks) == 50 else S.H
    x = C._noise(sum(chunks), (3, sum(chunks)), 1.0)
    xd = _dev(x, dev)
    ref = S.stream(KW, x, chunks, hop)
    nh = ref["seen"] // hop
    hist, zi, op, seen = _run_list(xd, KW, chunks, hop, nh + 4)
    got = hist.cpu().numpy()
    assert seen == ref["seen"] and np.all(got[:, nh:] == SENTINEL)
    one_call = ops.sos_hop_power(xd, KW, hop).cpu().numpy()
    figures = (C.rel_max(got[:, :nh], ref["power"]), C.rel_max(got[:, :nh], one_call), C.rel_max(zi.cpu().numpy(), ref["zf"]),
               float(np.abs(op.cpu().numpy() - ref["open"]).max() / np.abs(ref["power"]).max()))
    print("%d chunks: history %.2e of the oracle, %.2e of the one call, state %.2e, open sum %.2e" % ((len(chunks),) + figures))
    assert max(figures) <= S.TOL
    again = _run_list(xd, KW, chunks, hop, nh + 4)
    assert torch.equal(again[0], hist) and torch.equal(again[1], zi) and torch.equal(again[2], op)


# ---- the bit rules -------------------------------------------------------------------------------------------------------

def test_a_stream_alone_has_the_bits_it_has_in_a_batch(dev):
    x = _dev(C.clips()["batch"], dev)                                    # (70, 2, 8 H - 1)
    chunks = S.chunk_list(7, x.shape[-1], 3 * S.H)
    runs = []
    for rows in (1, 3, 70):
        m = A.RealtimeLoudness(S.SR).to(dev)
        at, outs = 0, []
        for n in chunks:
            outs.append(m(x[:rows, :, at:at + n]))
            at += n
        runs.append((m, torch.cat(outs, -1), m.integrated(), m.block_loudness(4)))
    full = runs[2]
    for rows, (m, out, integ, blocks) in zip((1, 3), runs[:2]):
        assert torch.equal(out, full[1][:rows]) and torch.equal(integ, full[2][:rows]) and torch.equal(blocks, full[3][:rows])
        for k in ("filter_state", "open_power", "hop_power"):
            assert torch.equal(getattr(m, k), getattr(full[0], k)[:rows]), k
    assert full[1].shape == (70, x.shape[-1] // S.H - 3) and full[0].samples_seen == x.shape[-1]


def test_aliased_state_has_the_bits_of_separate_buffers(dev):
    lib = _lib.lib()
    co = ops.sos_coefficients(KW)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 2 * S.TILE + 5, generator=g).to(dev)
    zi = torch.randn(5, 2, 2, generator=g, dtype=torch.float64).to(dev) * 1e-3
    op = torch.rand(5, generator=g, dtype=torch.float64).to(dev)
    for hop, filled in ((16, 3), (800, 799), (4097, 0)):
        done = (filled + x.shape[1]) // hop
        alias = _step(x, KW, hop, filled, zi, op, first=0, pad=0)
        zf, out = torch.full_like(zi, SENTINEL), torch.full_like(op, SENTINEL)
        power = torch.empty(5, done, dtype=torch.float64, device=dev)
        _lib.check(lib.at_sos_hop_power_stream(_lib.ptr(x), 5, x.shape[1], co.ptr, co.n, hop, filled, _lib.ptr(zi), _lib.ptr(zf),
                                               _lib.ptr(op), _lib.ptr(out), _lib.ptr(power), done, 0, _lib.stream_ptr()), "stream")
        assert torch.equal(alias[0], power) and torch.equal(alias[2], zf) and torch.equal(alias[3], out), (hop, filled)
        # null zi / open_in are zeros
        _lib.check(lib.at_sos_hop_power_stream(_lib.ptr(x), 5, x.shape[1], co.ptr, co.n, hop, filled, None, _lib.ptr(zf), None,
                                               _lib.ptr(out), _lib.ptr(power), done, 0, _lib.stream_ptr()), "stream")
        zero = _step(x, KW, hop, filled, torch.zeros_like(zi), torch.zeros_like(op), first=0, pad=0)
        assert torch.equal(zero[0], power) and torch.equal(zero[2], zf) and torch.equal(zero[3], out)


def test_a_nan_stays_in_its_row_and_after_its_sample_and_zeros_give_plus_zero(dev):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 2 * S.TILE + 5, generator=g)
    zi = (torch.randn(4, 2, 2, generator=g, dtype=torch.float64) * 1e-3).to(dev)
    op = torch.rand(4, generator=g, dtype=torch.float64).to(dev)
    for hop, filled, m in ((17, 5, 1000), (800, 1, 4096), (800, 799, 0), (4097, 0, 8000)):
        clean = _step(x.to(dev), KW, hop, filled, zi, op)
        bad = x.clone()
        bad[2, m] = float("nan")
        got = _step(bad.to(dev), KW, hop, filled, zi, op)
        k = (filled + m) // hop                                          # the chunk's hop that holds sample m
        done = clean[1]
        for r in (0, 1, 3):
            assert torch.equal(got[0][r], clean[0][r]) and torch.equal(got[2][r], clean[2][r]) and torch.equal(got[3][r], clean[3][r])
        assert torch.equal(got[0][2, :2 + k], clean[0][2, :2 + k]), (hop, filled, m)
        assert bool(torch.isnan(got[0][2, 2 + k:2 + done]).all()) and bool(torch.isnan(got[3][2])) and bool(torch.isnan(got[2][2]).all())
        assert bool((got[0][2, 2 + done:] == SENTINEL).all())
    z = _step(torch.zeros(3, S.TILE + 1, device=dev), KW, 800, 7, torch.zeros(3, 2, 2, dtype=torch.float64, device=dev),
              torch.zeros(3, dtype=torch.float64, device=dev), first=0, pad=0)
    for t in (z[0], z[2], z[3]):
        t = t.cpu().numpy()
        assert np.all(t == 0.0) and not np.signbit(t).any()


# ---- the module ----------------------------------------------------------------------------------------------------------

def _chunkings(L):
    return {"all": [L], "one hop": [S.H] * (L // S.H) + ([L % S.H] if L % S.H else []),
            "799/801": [n for _ in range(L // 1600 + 1) for n in (799, 801)], "seeded": S.chunk_list(L, L)}


def _stream(m, xd, chunks):
    at, outs = 0, []
    for n in chunks:
        n = min(n, xd.shape[-1] - at)
        if n <= 0:
            break
        outs.append(m(xd[..., at:at + n]))
        at += n
    assert at == xd.shape[-1] == m.samples_seen
    return torch.cat(outs, -1)


@pytest.mark.parametrize("name", S.STREAM_CLIPS)
def test_module_under_chunkings_matches_the_oracle_and_the_offline_module(dev, name):
    x = S.clip(name)
    xd = _dev(x, dev)
    off = A.Loudness(S.SR).to(dev)
    worst, nh = 0.0, x.shape[-1] // S.H
    offline = {4: off.momentary(xd).cpu().numpy(), 30: off.short_term(xd).cpu().numpy() if nh >= 30 else None}
    for label, chunks in _chunkings(x.shape[-1]).items():
        m = off.streaming().to(dev)
        out = _stream(m, xd, chunks).cpu().numpy()
        assert m.hops == nh
        for hb, got in ((4, out), (4, m.block_loudness(4).cpu().numpy()), (30, m.block_loudness(30).cpu().numpy())):
            ref = S.block_reference(name, hb)
            if ref is None:
                assert got.shape == x.shape[:-2] + (0,)
                continue
            worst = max(worst, _lu_error(got, ref[1], ref[0]), _lu_error(got, offline[hb].astype(np.float64), ref[0]))
        assert torch.equal(m.momentary(), m.block_loudness(4)[..., -1])
        if nh >= 30:
            assert torch.equal(m.short_term(), m.block_loudness(30)[..., -1])
        else:
            assert bool(torch.isneginf(m.short_term()).all()) and m.short_term().shape == x.shape[:-2]
    print("%s: streamed block loudness %.2e LU" % (name, worst))
    assert worst <= S.TOL_LU


def test_integrated_over_a_stream(dev):
    """integrated() after the prefixes of `gated` (each keeps its margin: assert_margins) and at the end, against the oracle;
    and to the bit what ops.loudness's gate reads on a contiguous copy of the history -- the join order is a function of
    nb alone."""
    lib = _lib.lib()
    x = C.clips()["gated"]
    xd = _dev(x, dev)
    m = A.RealtimeLoudness(S.SR).to(dev)
    assert bool(torch.isneginf(m.integrated()).all()) and m(xd[:, :0]).shape == (0,)
    at, worst = 0, 0.0
    plan = ops.loudness_plan((2, 4 * S.H), S.SR)
    for hops in S.INTEGRATED_PREFIXES + (None,):
        end = x.shape[-1] if hops is None else hops * S.H
        for n in S.chunk_list(end, end - at, 1000):
            m(xd[:, at:at + n])
            at += n
        got = m.integrated()
        worst = max(worst, abs(float(got) - float(C.loudness(x[:, :end], S.SR))))
        copy = m.hop_power[..., :m.hops].contiguous()
        lufs = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        _lib.check(lib.at_loudness_gate(_lib.ptr(copy), 1, 2, m.hops, S.H, 4, plan.wptr, ops.LOUDNESS_ABS_THRESHOLD,
                                        ops.LOUDNESS_REL_RATIO, _lib.ptr(lufs), _lib.ptr(stats), None, _lib.stream_ptr()), "gate")
        assert torch.equal(got, lufs), hops
    print("integrated over a stream: %.2e LU" % worst)
    assert worst <= S.TOL_LU


def test_before_the_first_block_reset_state_dict_growth_and_new_shapes(dev):
    x = _dev(S.clip("range gated"), dev)
    m = A.RealtimeLoudness(S.SR).to(dev)
    out = m(x[:, :3 * S.H + 799])                                        # three hops and an open one: no block yet
    assert out.shape == (0,) and out.dtype == torch.float32 and m.hops == 3
    for v in (m.momentary(), m.short_term(), m.integrated()):
        assert v.shape == () and bool(torch.isneginf(v))
    assert m.block_loudness(4).shape == (0,) and float(m.loudness_range()) == 0.0
    assert m(x[:, 3 * S.H + 799:4 * S.H]).shape == (1,) and bool(torch.isfinite(m.momentary()))
    # a 1-D chunk is one mono stream; a new leading shape starts a new stream
    mono = m(x[0, :5 * S.H])
    assert mono.shape == (2,) and m.samples_seen == 5 * S.H and m.hop_power.shape == (1, 1024)
    assert float((mono - A.Loudness(S.SR).momentary(x[0, :5 * S.H])).abs().max()) <= S.TOL_LU
    # reset() restarts: the same chunks give the same bits
    chunks = S.chunk_list(4, x.shape[-1], 2000)
    m = A.RealtimeLoudness(S.SR).to(dev)
    first = _stream(m, x, chunks)
    state = [getattr(m, k).clone() for k in ("filter_state", "open_power", "hop_power")]
    m.reset()
    assert m.samples_seen == 0 and not bool(m.hop_power.any())
    assert torch.equal(_stream(m, x, chunks), first) and all(torch.equal(getattr(m, k), s) for k, s in zip(
        ("filter_state", "open_power", "hop_power"), state))
    # a state_dict loaded mid-stream continues to the bit; a history that grows past its cap (8 here) has the same bits
    half = len(chunks) // 2
    a, small = A.RealtimeLoudness(S.SR).to(dev), A.RealtimeLoudness(S.SR, _cap=8).to(dev)
    head = _stream_part(a, x, chunks[:half], 0)
    b = A.RealtimeLoudness(S.SR).half().to(dev)
    b.load_state_dict(a.state_dict())
    assert b.hop_power.dtype == torch.float64 and b.samples_seen == a.samples_seen
    tail = _stream_part(b, x, chunks[half:], a.samples_seen)
    assert torch.equal(torch.cat([head, tail], -1), first) and torch.equal(b.hop_power, m.hop_power)
    assert torch.equal(b.integrated(), m.integrated()) and torch.equal(b.loudness_range(), m.loudness_range())
    assert torch.equal(_stream(small, x, chunks), first) and small.hop_power.shape[-1] == 256
    assert torch.equal(small.hop_power[..., :m.hops], m.hop_power[..., :m.hops]) and torch.equal(small.integrated(), m.integrated())
    # the outputs carry no graph
    y = A.RealtimeLoudness(S.SR).to(dev)(x[:, :5 * S.H].clone().requires_grad_())
    assert not y.requires_grad


def _stream_part(m, xd, chunks, at):
    outs = []
    for n in chunks:
        outs.append(m(xd[..., at:at + n]))
        at += n
    return torch.cat(outs, -1)


# ---- loudness range ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.RANGE_PARITY + ("tech3341-3 short",))
def test_range_matches_the_oracle_and_the_select_is_exact(dev, name):
    x = S.clip(name)
    xd = _dev(x, dev)
    ref = S.range_reference(name)[0]
    lra, power, stats = ops.loudness_range(xd, S.SR, return_state=True)
    assert lra.shape == () and lra.dtype == torch.float32 and stats.shape == (4,)
    m = A.RealtimeLoudness(S.SR).to(dev)
    _stream(m, xd, S.chunk_list(3, x.shape[-1], 3000))
    errors = (abs(float(lra) - ref["lra"]), abs(float(m.loudness_range()) - ref["lra"]),
              abs(float(A.Loudness(S.SR).loudness_range(xd.clone().requires_grad_())) - ref["lra"]))
    # the select: numpy's sort of the block powers recomputed in float64 from the DEVICE's own hop powers
    s = power.cpu().numpy()
    nb = s.shape[-1] - 29
    p = np.einsum("c,cj->j", C.weights_for(2), sum(s[:, k:k + nb] for k in range(30))) / (30 * S.H)
    mine = S.range_of(p)
    st = stats.cpu().numpy()
    select = max(abs(st[0] - mine["lo"]) / mine["lo"], abs(st[1] - mine["hi"]) / mine["hi"])
    print("%s: range %.2e LU (streamed %.2e), select %.2e, n = %d" % (name, errors[0], errors[1], select, st[2]))
    assert (st[2], mine["n"]) == (ref["n"], ref["n"]) and abs(st[3] - mine["Pabs"]) <= 1e-12 * mine["Pabs"]
    assert select <= 1e-12
    assert max(errors) <= 2 * S.TOL_LU


def test_range_of_a_clip_does_not_depend_on_the_batch(dev):
    gains = (10.0 ** (np.linspace(-3.0, 3.0, 70) / 20.0)).astype(np.float32)
    x = _dev(S.clip("range gated")[None] * gains[:, None, None], dev)
    lra, _, stats = ops.loudness_range(x, S.SR, return_state=True)
    assert lra.shape == (70,) and bool(torch.isfinite(lra).all())
    for rows in (slice(0, 1), slice(0, 3), slice(69, 70)):
        l1, _, s1 = ops.loudness_range(x[rows].contiguous(), S.SR, return_state=True)
        assert torch.equal(l1, lra[rows]) and torch.equal(s1, stats[rows])
    assert torch.equal(ops.loudness_range(x.view(2, 35, 2, -1), S.SR), lra.view(2, 35))


def test_range_edge_cases_from_planted_hop_powers(dev):
    """n = 1 and n = 2 gated blocks, all blocks equal (every radix pass degenerate), nothing above the gate, a NaN clip between
    two clean ones, a window of a longer row, and 2100 clips (the persistent workgroups' second turn)."""
    loud = 30 * S.H * 1e-3                                               # a hop power whose 3 s block reads p = 1e-3 per hop

    def run(rows, nh=None):
        t = _dev(np.asarray(rows, dtype=np.float64)[:, None, :], dev)   # (clips, 1, ld)
        lra, stats = ops.loudness_range_from_power(t, t.shape[-1] if nh is None else nh, S.SR, return_state=True)
        return lra.cpu().numpy(), stats.cpu().numpy()
    one = np.full((1, 30), loud / 30)
    lra, st = run(one)
    assert lra[0] == 0.0 and st[0, 2] == 1 and st[0, 0] == st[0, 1] > 0
    two = np.full((1, 31), loud / 30)
    two[0, 30] *= 11.0                                                   # the second block: (29 + 11) / 30 of the first
    lra, st = run(two)
    ref = S.range_of(np.array([two[0, :30].sum(), two[0, 1:].sum()]) / (30 * S.H))
    assert st[0, 2] == 2 == ref["n"] and abs(st[0, 0] - ref["lo"]) <= 1e-12 * ref["lo"] \
        and abs(st[0, 1] - ref["hi"]) <= 1e-12 * ref["hi"] and abs(lra[0] - ref["lra"]) < 1e-5
    lra, st = run(np.full((1, 100), 0.25))                               # 71 equal blocks
    assert lra[0] == 0.0 and st[0, 2] == 71 and st[0, 0] == st[0, 1] == (30 * 0.25) / (30 * S.H)
    lra, st = run(np.full((1, 100), 1e-12))                              # nothing above the absolute gate
    assert lra[0] == 0.0 and not st[0, :3].any()
    lra, st = run(np.zeros((1, 29)))                                     # no 3 s block at all
    assert lra[0] == 0.0 and not st[0].any()
    rng = np.random.default_rng(8)
    clean = rng.uniform(0.5, 50.0, (3, 120)) * loud
    lra_clean, st_clean = run(clean)
    bad = clean.copy()
    bad[1, 60] = np.nan
    lra, st = run(bad)
    assert np.isnan(lra[1]) and np.isnan(st[1, :2]).all()
    assert np.array_equal(lra[[0, 2]], lra_clean[[0, 2]]) and np.array_equal(st[[0, 2]], st_clean[[0, 2]])
    for r in range(3):                                                   # random blocks: the select against numpy's sort
        p = np.array([clean[r, j:j + 30].sum() for j in range(91)]) / (30 * S.H)
        ref = S.range_of(p)
        assert st_clean[r, 2] == ref["n"] and abs(st_clean[r, 0] - ref["lo"]) <= 1e-12 * ref["lo"] \
            and abs(st_clean[r, 1] - ref["hi"]) <= 1e-12 * ref["hi"] and abs(lra_clean[r] - ref["lra"]) < 1e-5
    wide = np.concatenate([clean, np.full((3, 8), np.nan)], axis=1)      # a window of a longer row: the rest is not read
    lra_w, st_w = run(wide, nh=120)
    assert np.array_equal(lra_w, lra_clean) and np.array_equal(st_w, st_clean)
    many = rng.uniform(0.5, 50.0, (2100, 64)) * loud
    lra_m, st_m = run(many)
    for r in (0, 2047, 2048, 2099):
        l1, s1 = run(many[r:r + 1])
        assert l1[0] == lra_m[r] and np.array_equal(s1[0], st_m[r])

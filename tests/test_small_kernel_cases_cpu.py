"""The cases of test_small_kernels_gpu.py take every grid-stride loop of the pointwise, statistics and quantisation
kernels into its second and third trip, stand on both sides of every dispatch condition, and their inputs meet the
conditions the tolerances rest on (small_kernel_cases.py restates the launch arithmetic).  CPU only: this turns the GPU
file's coverage claims into checked facts."""
import numpy as np
import torch

import small_kernel_cases as C


def _hit(sizes, cap=C.CAP):
    return set().union(*(C.trip_classes(n, cap) for n in sizes))


def test_the_launch_rules_as_stated():
    assert C.TRIP == 524288 and C.WIDE_TRIP == 2097152
    assert C.blocks(1) == 1 and C.blocks(256) == 1 and C.blocks(257) == 2 and C.blocks(10 ** 9) == 2048
    assert C.trips(C.TRIP) == 1 and C.trips(C.TRIP + 1) == 2 and C.trips(2 * C.TRIP) == 2 and C.trips(2 * C.TRIP + 77) == 3
    assert C.trips(C.WIDE_TRIP, C.WIDE_CAP) == 1 and C.trips(4100 * 512, C.WIDE_CAP) == 2
    assert C.stats_plan(1) == (1, 1, 1) and C.stats_plan(2048) == (1, 8, 1) and C.stats_plan(2049) == (2, 5, 1)
    assert C.stats_plan(256 * 2048) == (256, 8, 1) and C.stats_plan(256 * 2048 + 1) == (257, 8, 2)
    assert C.stats_plan(2097152) == (1024, 8, 4) and C.stats_plan(2097153) == (1024, 9, 4)
    assert C.pack_form(64, 513) == "rows" and C.pack_form(63, 513) == "flat" and C.pack_form(64, 63) == "flat"
    assert C.pack_form(64, 64) == "flat" and C.pack_form(64, 65) == "rows" and C.pack_form(4100, 512) == "flat"
    assert C.mel_kernel(576) == "mfma" and C.mel_kernel(577) == "simple" and C.mel_kernel(16) == "mfma"
    assert C.mel_kernel(15) == "simple"


def test_every_plain_loop_reaches_every_trip_shape():
    assert _hit(C.SIZES) >= C.LOOP_WANT, sorted(C.LOOP_WANT - _hit(C.SIZES))
    for n in C.SIZES:                                                   # no size is there twice over: each adds a class
        assert not _hit([m for m in C.SIZES if m != n]) >= C.LOOP_WANT, n
    # the entries with tables of their own
    row_major = [int(np.prod(s)) * k for s, k, cm in C.ONEHOT if not cm]
    channel = [int(np.prod(s)) * k for s, k, cm in C.ONEHOT if cm]
    assert _hit(row_major) >= C.LOOP_WANT, sorted(C.LOOP_WANT - _hit(row_major))
    assert _hit(channel) >= C.ONEHOT_CHANNEL_WANT, sorted(C.ONEHOT_CHANNEL_WANT - _hit(channel))
    assert {k for _, k, cm in C.ONEHOT if not cm} == {1, 3, 256} == {k for _, k, cm in C.ONEHOT if cm}
    for s, k, cm in C.ONEHOT:
        if cm and s[-1] > 1:
            assert s[-1] % 2 == 1 and 256 % s[-1], s                    # odd inner length that does not divide 256
    rows = [r for r, _ in C.ARGMAX]
    assert _hit(rows) >= C.LOOP_WANT, sorted(C.LOOP_WANT - _hit(rows))
    assert {c for r, c in C.ARGMAX if r > C.TRIP} == {1, 2, 3} and (3000, 256) in C.ARGMAX
    assert all(r * c * 8 <= 32 << 20 for r, c in C.ARGMAX)
    totals = [S * bl for S, _, _, bl in C.OADD_FORWARD]
    assert _hit(totals) >= C.LOOP_WANT, sorted(C.LOOP_WANT - _hit(totals))
    assert all(bl >= keep + Cn and Cn >= 1 for _, Cn, keep, bl in C.OADD_FORWARD)
    assert any(Cn < keep for _, Cn, keep, _ in C.OADD_FORWARD) and any(bl > keep + Cn for _, Cn, keep, bl in C.OADD_FORWARD)
    assert set(C.LOOP_ENTRIES) == {"at_angle", "at_affine", "at_griffinlim_update", "at_scale_complex", "at_mag_pointwise",
                                   "at_mulaw_encode", "at_mulaw_decode", "at_onehot", "at_argmax_last", "at_oadd_forward"}


def test_cartesian_cases_stand_on_both_sides_of_every_condition():
    hit = set().union(*(C.pack_classes(r, F) for r, F in C.CARTESIAN))
    assert hit >= C.PACK_WANT, sorted(C.PACK_WANT - hit)
    forms = {(r, F): C.pack_form(r, F) for r, F in C.CARTESIAN}
    assert forms[(63, 513)] == "flat" and forms[(64, 513)] == "rows" and forms[(65, 513)] == "rows"
    assert forms[(64, 63)] == "flat" and forms[(65, 64)] == "flat" and forms[(64, 65)] == "rows"
    assert forms[(4100, 512)] == "flat" and C.trips(4100 * 512, C.WIDE_CAP) == 2        # the unpack's second trip too
    assert set(C.NORM_COMBOS) == {(a, b) for a in (False, True) for b in (False, True)}
    assert all(r * F < 1 << 32 for r, F in C.CARTESIAN)                 # the 64-bit index instantiations are not reached
    assert C.trips(C.WIDE_TRIP + 5, C.WIDE_CAP) == 2                    # at_polar_to_complex's case


def test_stats_cases_reach_every_fold():
    hit = set().union(*(C.stats_classes(n) for n in C.STATS_SIZES))
    assert hit >= C.STATS_WANT, sorted(C.STATS_WANT - hit)
    for n in C.STATS_SIZES:
        pos = C.stats_positions(n)
        b, t, _ = C.stats_plan(n)
        assert all(0 <= p < n for p in pos.values())
        assert pos["first"] == 0 and pos["last"] == n - 1 and (n - 1) // 256 % b == (C.cdiv(n, 256) - 1) % b
        if "second_trip" in pos:
            assert b * 256 <= pos["second_trip"] < 2 * b * 256
        assert ("second_trip" in pos) == (n > b * 256)
    assert "capped_ragged" in C.stats_classes(C.CAPPED_N) and C.CAPPED_N in C.STATS_SIZES
    assert "capped" in C.stats_classes(int(np.prod(C.CAPPED_SPECTRUM)))
    assert {"last_trip", "second_trip"} <= set(C.stats_positions(C.CAPPED_N))


def test_stats_inputs_meet_the_one_pass_condition():
    x = C.real_data(C.CAPPED_N)
    assert C.one_pass_condition(x) <= 100
    z = C.spectrum_data(C.CAPPED_SPECTRUM)
    for code in C.CONTRASTS.values():
        v = C.stats_values(z, 0, code)
        assert C.one_pass_condition(v) <= 100, code
        assert v.min() > 0                                              # one sign: the sums do not cancel
    assert np.abs(z).min() >= 1.49 and np.abs(z).max() <= 50.01
    # the one-pass variance in double is then far inside the 1e-6 bar
    s, ss, n = x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum(), x.size
    one_pass = np.sqrt((ss - s * s / n) / (n - 1))
    assert abs(one_pass / C.affine_ref64(x, "gaussian")[1] - 1) < 1e-9


def test_references_propagate_nan_like_the_reference():
    t = torch.tensor([1.0, float("nan"), 3.0])
    assert torch.isnan(t.min()) and torch.isnan(t.max())
    assert np.isnan(C.stats_ref(t.numpy())[:2]).all()
    for mode in ("unipolar", "bipolar", "gaussian"):
        assert np.isnan(C.affine_ref64(t.numpy(), mode)).all()
    rows = torch.tensor([[1.0, float("nan"), float("nan"), 5.0], [float("nan"), 9.0, 0.0, 0.0], [0.0, -0.0, 0.0, float("nan")],
                         [0.0, float("nan"), float("inf"), 0.0]])
    assert rows.argmax(-1).tolist() == [1, 0, 3, 1]                      # the first NaN wins, over +inf too
    assert torch.tensor([[-0.0, 0.0, 0.0]]).argmax(-1).tolist() == [0]


def test_argmax_rows_hold_every_kind():
    for rows, cols in C.ARGMAX:
        a = C.argmax_rows(rows, cols, True)
        assert a.shape == (rows, cols) and a.dtype == np.float32
        i = C.argmax_rows(rows, cols, False)
        assert i.dtype == np.int64 and i.shape == (rows, cols)
    a = C.argmax_rows(3000, 256, True)
    nan = np.isnan(a)
    assert nan[4::16, 0].all() and nan[5::16, 128].all() and nan[6::16, -1].all() and nan[7::16, 128].all()
    assert (a[3::16] == -np.inf).all() and np.signbit(a[2::16, ::2]).all() and not np.signbit(a[2::16, 1::2]).any()
    assert (a[1::16] == 1.5).all() and np.isinf(a[8::16, -1]).all() and nan[8::16, 128].all()
    assert len({tuple(r) for r in a[::16][:50]}) > 1                     # the plain rows are random, with ties
    assert any((r == r.max()).sum() > 1 for r in C.argmax_rows(257, 3, True)[::16])
    i = C.argmax_rows(3000, 256, False)
    assert (i[2::16].argmax(-1) == 255).all() and np.float32(i[2, 0]) == np.float32(i[2, -1])


def test_mulaw_inputs_stay_out_of_the_band():
    inside = total = 0
    for n in C.SIZES:
        x = C.mulaw_input(n)
        assert x.dtype == np.float32 and np.isfinite(x).all()
        if n >= 512:
            assert np.abs(x[256:512]).max() > 1.5 and np.abs(x[512:-8]).max() <= 1.0
        if n >= 8:
            assert C.same_bits(x[:8], C.MULAW_SPECIALS)
        for ch in C.MULAW_CHANNELS:
            q = C.mulaw_q64(x, ch)
            inside += int(C.mulaw_band(q).sum())
            total += x.size
            assert C.mulaw_band(q).mean() <= C.MULAW_BAND_SHARE or n < 2000, (n, ch)
    assert inside <= C.MULAW_BAND_SHARE * total
    # the closed form: the end points and zero land on codes 0, mu and (mu + 1) / 2 truncated
    assert np.trunc(C.mulaw_q64(np.array([-1.0, 0.0, 1.0], np.float32), 256)).tolist() == [0.0, 128.0, 255.0]


def test_special_values_reach_both_ends_and_the_middle():
    a = C.with_specials(C.randn32(2 * C.TRIP + 77, 1))
    k = len(C.SPECIALS)
    assert C.same_bits(a[:k], C.SPECIALS) and C.same_bits(a[-k:], C.SPECIALS[::-1]) and C.same_bits(a[a.size // 2:][:k], C.SPECIALS)
    s = C.SPECIALS
    assert np.isnan(s).any() and np.isinf(s).sum() == 2 and np.signbit(s[s == 0]).tolist() == [False, True]
    assert ((s != 0) & (np.abs(s) < np.finfo(np.float32).tiny)).sum() == 2          # denormals
    assert np.frexp(C.AFFINE_SCALE)[0] != 0.5 and all(np.frexp(v[1])[0] != 0.5 for v in (C.RE_AFFINE, C.IM_AFFINE, C.MEL_AFFINE))
    assert C.with_specials(C.randn32(1, 1)).size == 1
    # the exact references are the float32 expressions
    x = np.array([1.0, 3.0], np.float32)
    assert C.affine_ref(x, 0.3, 1.7, False).dtype == np.float32
    assert C.affine_ref(x, 0.3, 1.7, False)[0] == (np.float32(1.0) - np.float32(0.3)) / np.float32(1.7)
    assert C.affine_ref(x, 0.3, 1.7, True)[1] == np.float32(np.float32(3.0) * np.float32(1.7)) + np.float32(0.3)


def test_griffinlim_inputs_hold_exact_zeros():
    mag, reb, tp = C.griffinlim_data(1000)
    ref, bar, zero = C.griffinlim_ref(mag, reb, tp, C.GL_MOMENTUM)
    assert zero[::11].all() and zero.sum() == len(range(0, 1000, 11)) and (ref[zero] == 0).all()
    ref0, bar0, zero0 = C.griffinlim_ref(mag, reb, None, C.GL_MOMENTUM)
    assert zero0[::7].all() and zero0[::11].all() and np.isfinite(ref0).all()
    assert np.isfinite(bar[~zero]).all() and (bar[~zero] >= np.abs(mag[~zero]) * 8 * 2.0 ** -24).all()


def test_stream_cases_cross_the_block_limit():
    for table in ([S for S, _ in C.OADD_INVERT], [S for S, *_ in C.OADD_PUSH]):
        hit = set().union(*(C.stream_classes(S) for S in table))
        assert hit >= C.STREAM_WANT, sorted(C.STREAM_WANT - hit)
    assert {n for _, n in C.OADD_INVERT} == {1, 2, 3} and (C.OADD_N_FFT // C.OADD_HOP - 1) * C.OADD_HOP == C.OADD_KEEP
    big = [(Cn, keep) for S, Cn, keep, bl in C.OADD_PUSH if S > C.STREAM_BLOCKS]
    assert any(Cn < keep for Cn, keep in big) and any(Cn > keep for Cn, keep in big)
    assert any(keep > 256 and Cn < keep for _, Cn, keep, _ in C.OADD_PUSH)           # more than one element per thread
    assert all(bl >= keep + Cn for _, Cn, keep, bl in C.OADD_PUSH)


def test_resample_cases_reach_the_grid_limit_and_the_short_clips():
    from acids_transforms_amd.utils.audio_io import sinc_filter_bank
    h, width = sinc_filter_bank(C.RESAMPLE_ORIG, C.RESAMPLE_NEW)
    assert tuple(h.shape) == (C.RESAMPLE_NEW, 2 * width + C.RESAMPLE_ORIG) and h.dtype == torch.float32
    lens = {C.resample_out_len(L) for _, L in C.RESAMPLE}
    assert {255, 256, 257} <= lens
    assert any(1 < L < width for _, L in C.RESAMPLE) and any(L == 1 for _, L in C.RESAMPLE)
    assert max(r for r, _ in C.RESAMPLE) == C.GRID_Y and C.RESAMPLE_TOO_MANY[0] == C.GRID_Y + 1
    assert any(C.resample_out_len(L) > 2 * 256 for _, L in C.RESAMPLE)               # more than one block along x
    # the float64 reference is the header's sum: against a plain loop on a short clip
    x = C.randn32(2 * 7, 3).reshape(2, 7)
    y = C.resample_ref(x, h.numpy(), width)
    xp = np.zeros((2, 7 + 2 * width + C.RESAMPLE_ORIG))
    xp[:, width:width + 7] = x
    for o in range(y.shape[1]):
        i, j = divmod(o, C.RESAMPLE_NEW)
        want = sum(float(h[j, k]) * xp[:, i * C.RESAMPLE_ORIG + k] for k in range(h.shape[1]))
        assert np.allclose(y[:, o], want, rtol=0, atol=1e-15)


def test_projection_cases_reach_the_one_thread_per_output_kernel():
    hit = set().union(*(C.mel_classes(c) for c in C.MEL))
    assert hit >= C.MEL_WANT, sorted(C.MEL_WANT - hit)
    for c in C.MEL:
        assert C.mel_kernel(c.K) == "simple", c.name
        assert not c.T or c.rows % c.T == 0, c.name
        assert not c.inverse or (not c.complex and not c.T), c.name
        assert c.rows * c.K * (8 if c.complex else 4) <= 48 << 20, c.name
        # ops.mel_forward_real would take the register kernel at K <= 128, N <= 64: these go through mel_forward
    assert len({c.name for c in C.MEL}) == len(C.MEL)
    c = C.MEL[4]
    x, bank = C.mel_inputs(c)
    assert x.dtype == np.complex64 and bank.dtype == np.float32 and (bank == 0).mean() > 0.3 and bank.min() >= 0
    assert (np.abs(x) @ bank > 0).all()                                   # the log contrasts stay off their clamp

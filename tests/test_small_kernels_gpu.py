"""GPU: every index path of the pointwise, statistics and quantisation kernels (csrc/pointwise.hip, csrc/quant.hip,
csrc/resample.hip, mel_gemm_simple_kernel / mag_pointwise_kernel of csrc/mel.hip, polar_to_complex_kernel of
csrc/phase_repr.hip) against plain references: the same float32 expression where a kernel copies or rounds once,
float64 otherwise.  small_kernel_cases.py holds the launch rules, the cases, the inputs and the references;
test_small_kernel_cases_cpu.py checks that the cases reach every path.  Each toleranced case prints its worst error
next to its bar (pytest -s).

Not reached: the 64-bit index instantiations of the Cartesian kernels (2^32 elements: tens of GB).  Not pinned: mu-law
encoding of NaN or of values beyond the int64 range (undefined in the reference's own cast) and one-hot indices outside
[0, classes) (the reference raises, the kernel writes zeros)."""
import numpy as np
import pytest
import torch

import acids_transforms_amd as A
import small_kernel_cases as C
from acids_transforms_amd import _lib, ops
from acids_transforms_amd._lib import AcidsHipError
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def cpu(t):
    return t.detach().cpu().numpy()


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def scalar(v, dev):
    return torch.tensor(float(v), dtype=torch.float32, device=dev)


def report(what, worst, bar):
    print("FIGURE %-58s worst %.3e  bar %.3e" % (what, worst, bar))


# ---- copies and single correctly rounded operations: the same bits -------------------------------------------------------
def test_affine_same_bits_at_every_trip_shape(dev):
    off, sc = scalar(C.AFFINE_OFFSET, dev), scalar(C.AFFINE_SCALE, dev)
    for n in C.SIZES:
        x = C.with_specials(C.randn32(n, 1) * f32(3))
        for inverse in (False, True):
            got = cpu(ops.affine(up(x, dev), off, sc, inverse=inverse))
            assert C.same_bits(got, C.affine_ref(x, C.AFFINE_OFFSET, C.AFFINE_SCALE, inverse)), (n, inverse)


def test_scale_complex_same_bits_at_every_trip_shape(dev):
    for n in C.SIZES:
        mag = C.with_specials(C.randn32(n, 2))
        z = np.empty(n, np.complex64)
        z.real, z.imag = C.with_specials(C.randn32(n, 3), C.SPECIALS[::-1]), C.with_specials(C.randn32(n, 4), np.roll(C.SPECIALS, 3))
        got = cpu(ops.scale_complex(up(mag, dev), up(z, dev)))
        with np.errstate(all="ignore"):
            assert C.same_bits(got.real, mag * z.real) and C.same_bits(got.imag, mag * z.imag), n


@pytest.mark.parametrize("rows,F", C.CARTESIAN)
def test_cartesian_pack_and_unpack_same_bits(dev, rows, F):
    n = rows * F
    x = np.empty(n, np.complex64)
    x.real, x.imag = C.with_specials(C.randn32(n, 5)), C.with_specials(C.randn32(n, 6), C.SPECIALS[::-1])
    x = x.reshape(rows, F)
    y = np.stack([C.with_specials(C.randn32(n, 7)).reshape(rows, F),
                  C.with_specials(C.randn32(n, 8), C.SPECIALS[::-1]).reshape(rows, F)], 1)
    xd, yd = up(x, dev), up(y, dev)
    for on_re, on_im in C.NORM_COMBOS:
        re, im = (C.RE_AFFINE if on_re else None), (C.IM_AFFINE if on_im else None)
        kw = {}
        if re:
            kw.update(re_offset=scalar(re[0], dev), re_scale=scalar(re[1], dev))
        if im:
            kw.update(im_offset=scalar(im[0], dev), im_scale=scalar(im[1], dev))
        got = cpu(ops.cartesian_forward(xd, **kw))
        assert got.shape == (rows, 2, F) and C.same_bits(got, C.cartesian_pack_ref(x, re, im)), (on_re, on_im)
        back = cpu(ops.cartesian_inverse(yd, **kw))
        assert back.shape == (rows, F) and C.same_bits(back, C.cartesian_unpack_ref(y, re, im)), (on_re, on_im)


@pytest.mark.parametrize("S,Cn,keep,buf_len", C.OADD_FORWARD)
def test_oadd_forward_same_bits(dev, S, Cn, keep, buf_len):
    x = C.with_specials(C.randn32(S * Cn, 9)).reshape(S, Cn)
    hist = C.randn32(S * keep, 10).reshape(S, keep)
    xd = up(x, dev)
    for h in (hist, None):
        buf = torch.full((S, buf_len), 7.0, dtype=torch.float32, device=dev)
        new_hist = torch.full((S, max(keep, 1)), 7.0, dtype=torch.float32, device=dev)        # keep 0: never written
        hd = up(h, dev) if h is not None and keep else None
        _lib.check(_lib.lib().at_oadd_forward(_lib.ptr(xd), _lib.ptr(hd), S, Cn, keep, buf_len, _lib.ptr(buf),
                                              _lib.ptr(new_hist), _lib.stream_ptr()), "at_oadd_forward")
        want_buf, want_hist = C.oadd_forward_ref(x, h, keep, buf_len)
        assert C.same_bits(cpu(buf), want_buf)
        assert C.same_bits(cpu(new_hist)[:, :keep], want_hist)


@pytest.mark.parametrize("S,Cn,keep,buf_len", C.OADD_PUSH)
def test_oadd_push_same_bits(dev, S, Cn, keep, buf_len):
    buf = C.with_specials(C.randn32(S * buf_len, 11)).reshape(S, buf_len)
    bd = up(buf, dev)
    for step in range(2):
        x = C.randn32(S * Cn, 12 + step).reshape(S, Cn)
        ops.oadd_push_(bd, up(x, dev), keep)
        buf = C.oadd_push_ref(buf, x, keep)
        assert C.same_bits(cpu(bd), buf), step


# ---- angle, Griffin-Lim, the pointwise magnitude chain, polar to complex ---------------------------------------------------
def test_angle_at_every_trip_shape(dev):
    worst = 0.0
    for n in C.SIZES:
        re, im = C.angle_data(n)
        got = cpu(ops.angle(torch.complex(up(re, dev), up(im, dev))))
        err = float(np.abs(got - np.arctan2(im.astype(f64), re.astype(f64))).max())
        worst = max(worst, err)
        assert got.shape == (n,) and err < C.ANGLE_BAR, (n, err)
    report("angle", worst, C.ANGLE_BAR)


def test_griffinlim_update_at_every_trip_shape(dev):
    worst = 0.0
    m = float(C.GL_MOMENTUM)
    for n in C.SIZES:
        mag, reb, tp = C.griffinlim_data(n)
        md, rd = up(mag, dev), up(reb, dev)
        for t in (tp, None):
            got = cpu(ops.griffinlim_update(md, rd, up(t, dev) if t is not None else None, m)).astype(np.complex128)
            ref, bar, zero = C.griffinlim_ref(mag, reb, t, m)
            assert (got[zero] == 0).all(), n                            # a == 0: exactly 0, never NaN
            ratio = np.abs(got - ref)[~zero] / bar[~zero]
            if ratio.size:
                worst = max(worst, float(ratio.max()))
                assert ratio.max() <= 1.0, (n, float(ratio.max()))
        zeros = cpu(ops.griffinlim_update(md, rd, torch.zeros_like(rd), m))
        assert np.array_equal(zeros, cpu(ops.griffinlim_update(md, rd, None, m))), n
    report("griffinlim_update (error / its per-element bar)", worst, 1.0)


def test_mag_pointwise_at_every_trip_shape(dev):
    off, sc = scalar(C.MEL_AFFINE[0], dev), scalar(C.MEL_AFFINE[1], dev)
    o64, s64 = f64(C.MEL_AFFINE[0]), f64(C.MEL_AFFINE[1])
    worst = 0.0
    for n in C.SIZES:
        z = C.spectrum_data((n,), 14)
        y = np.random.RandomState(15).uniform(0.0, 1.5, n).astype(f32)
        zd, yd = up(z, dev), up(y, dev)
        for name, code in C.CONTRASTS.items():
            got = cpu(ops.mag_pointwise(zd, name, off, sc))
            e = C.rel_max(got, (C.stats_values(z, 0, code) - o64) / s64)
            got = cpu(ops.mag_pointwise(yd, name, off, sc, inverse=True))
            e = max(e, C.rel_max(got, C.contrast_inv_ref(y.astype(f64) * s64 + o64, code)))
            worst = max(worst, e)
            assert e < C.PARITY, (n, name, e)
        got = cpu(ops.mag_pointwise(yd, "log1p"))                      # no Normalize, |real|
        assert C.rel_max(got, np.log1p(y.astype(f64))) < C.PARITY
    report("mag_pointwise", worst, C.PARITY)


def test_polar_to_complex_second_trip(dev):
    n = C.WIDE_TRIP + 5
    rng = np.random.RandomState(16)
    mag, ph = rng.uniform(0.0, 3.0, n).astype(f32), rng.uniform(-np.pi, np.pi, n).astype(f32)
    got = cpu(ops.polar_to_complex(up(mag, dev), up(ph, dev)))
    e = C.rel_max(got, mag.astype(f64) * np.exp(1j * ph.astype(f64)))
    report("polar_to_complex", e, C.PARITY)
    assert e < C.PARITY


# ---- statistics ---------------------------------------------------------------------------------------------------------
def _stats(xd, kind, contrast=0):
    """at_stats through ops where it exposes the combination, through the C entry otherwise (kind 1 = |z|^2)."""
    name = {v: k for k, v in C.CONTRASTS.items()}[contrast]
    if kind == 0 or kind == 3:
        return cpu(ops.stats(xd, name, take_abs=True))
    if kind == 2 and contrast == 0:
        return cpu(ops.stats(xd, take_abs=False))
    L = _lib.lib()
    out = torch.empty(4, dtype=torch.float64, device=xd.device)
    wsb = L.at_stats_workspace_bytes()
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=xd.device)
    _lib.check(L.at_stats(_lib.ptr(xd), kind, xd.numel(), contrast, C.EPS, _lib.ptr(out), _lib.ptr(ws), wsb,
                          _lib.stream_ptr()), "at_stats")
    return cpu(out)


def _same(a, b):
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


@pytest.mark.parametrize("n", C.STATS_SIZES)
def test_stats_of_real_data_extremes_exact_sums_to_double_rounding(dev, n):
    x = C.real_data(n)
    xd = up(x, dev)
    for kind in (2, 3):
        v = C.stats_values(x, kind, 0)
        got, ref = _stats(xd, kind), C.stats_ref(v)
        assert got[0] == ref[0] and got[1] == ref[1], (kind, got, ref)
        bars = n * 2.0 ** -52 * np.abs(v).sum(), n * 2.0 ** -52 * (v * v).sum()
        report("stats kind %d n %d sum" % (kind, n), abs(got[2] - ref[2]), bars[0])
        report("stats kind %d n %d sum of squares" % (kind, n), abs(got[3] - ref[3]), bars[1])
        assert abs(got[2] - ref[2]) <= bars[0] and abs(got[3] - ref[3]) <= bars[1]
        for where, p in C.stats_positions(n).items():
            for val in (-1e30, 1e30, -np.inf, np.inf):
                xd[p] = val
                v2 = v.copy()
                v2[p] = C.stats_values(np.array([val], f32), kind, 0)[0]
                got = _stats(xd, kind)
                assert _same(got[0], v2.min()) and _same(got[1], v2.max()), (kind, where, val, got)
                if np.isfinite(val):
                    assert abs(got[2] - v2.sum()) <= n * 2.0 ** -52 * np.abs(v2).sum()
                xd[p] = float(x[p])
        assert np.array_equal(cpu(xd), x)


@pytest.mark.parametrize("n", C.STATS_SIZES[:-1] + (int(np.prod(C.CAPPED_SPECTRUM)),))
def test_stats_of_spectra_and_every_contrast(dev, n):
    z = C.spectrum_data((n,))
    zd = up(z, dev)
    worst_ulp = worst_sum = 0.0
    for kind in (0, 1):
        for code in C.CONTRASTS.values():
            v = C.stats_values(z, kind, code)
            places = C.stats_positions(n) if (kind == 0 or code == 0) else {}
            trials = [(None, None)] + [(p, val) for p in places.values() for val in (0.0, 1e4, np.inf)]
            for p, val in trials:
                v2 = v
                if p is not None:
                    zd[p] = complex(val, 0.0)
                    v2 = v.copy()
                    v2[p] = C.stats_values(np.array([val], np.complex64), kind, code)[0]
                got, ref = _stats(zd, kind, code), C.stats_ref(v2)
                for g, r in zip(got[:2], ref[:2]):
                    if np.isfinite(r):
                        ulps = abs(g - r) / float(np.spacing(np.abs(f32(r)))) if g != r else 0.0
                        worst_ulp = max(worst_ulp, ulps)
                        assert ulps <= 4, (kind, code, p, val, g, r)
                    else:
                        assert g == r, (kind, code, p, val, g, r)
                if np.isfinite(ref[2:]).all():
                    rel = max(abs(got[2] - ref[2]) / abs(ref[2]), abs(got[3] - ref[3]) / abs(ref[3]))
                    worst_sum = max(worst_sum, rel)
                    assert rel <= 1e-6, (kind, code, p, val, got, ref)
                if p is not None:
                    zd[p] = complex(z[p])
    report("stats of spectra n %d min / max (ulp)" % n, worst_ulp, 4)
    report("stats of spectra n %d sums (relative)" % n, worst_sum, 1e-6)


@pytest.mark.parametrize("n", C.STATS_SIZES)
def test_stats_nan_propagates_like_tensor_min_max(dev, n):
    """Tensor.min() / max() return NaN when the data hold one (the reference's Normalize.scale_data takes them)."""
    x = C.real_data(n)
    xd = up(x, dev)
    zd = up(C.spectrum_data((min(n, 700000),)), dev)
    for where, p in C.stats_positions(n).items():
        xd[p] = float("nan")
        for kind in (2, 3):
            got = _stats(xd, kind)
            assert np.isnan(got[0]) and np.isnan(got[1]), (where, kind, got)
        xd[p] = float(x[p])
        if p < zd.numel():
            keep = complex(zd[p])
            zd[p] = complex(float("nan"), 1.0)
            for kind, code in ((0, 0), (1, 0), (0, 1)):
                got = _stats(zd, kind, code)
                assert np.isnan(got[0]) and np.isnan(got[1]), (where, kind, code, got)
            zd[p] = keep
    assert not np.isnan(_stats(xd, 2)).any()


def test_normalize_and_magnitude_scale_data_at_a_capped_size(dev):
    x = C.real_data(C.CAPPED_N)
    xd = up(x, dev)
    worst = 0.0
    for mode in ("unipolar", "bipolar", "gaussian"):
        norm = A.Normalize(mode)
        norm.scale_data(xd)
        off, sc = C.affine_ref64(x, mode)
        e = max(abs(float(norm.offset) - off) / abs(off), abs(float(norm.scale) - sc) / abs(sc))
        worst = max(worst, e)
        assert e <= 1e-6, (mode, e)
        y = norm(xd)
        lo, hi = float(y.min()), float(y.max())
        if mode == "unipolar":
            assert lo == 0.0 and hi == 1.0
        if mode == "bipolar":
            # fl(offset) is half an ulp off the midpoint and the kernel rounds three times: the far end is -1 within
            # 2^-22 (1 + |offset| / scale)
            assert hi == 1.0 and abs(lo + 1.0) <= 2.0 ** -22 * (1 + abs(off) / sc), lo
    for where, p in C.stats_positions(C.CAPPED_N).items():
        xd[p] = float("nan")
        for mode in ("unipolar", "bipolar", "gaussian"):
            norm = A.Normalize(mode)
            norm.scale_data(xd)
            assert np.isnan(float(norm.offset)) and np.isnan(float(norm.scale)), (where, mode)
        xd[p] = float(x[p])
    z = C.spectrum_data(C.CAPPED_SPECTRUM)
    zd = up(z, dev)
    for name, code in C.CONTRASTS.items():
        v = C.stats_values(z, 0, code)
        for mode in ("unipolar", "bipolar", "gaussian"):
            mag = A.Magnitude(mode=mode, contrast=name).to(dev)
            mag.scale_data(zd)
            off, sc = C.affine_ref64(v, mode)
            e = max(abs(float(mag.norm.offset) - off) / abs(off), abs(float(mag.norm.scale) - sc) / abs(sc))
            worst = max(worst, e)
            assert e <= 1e-6, (name, mode, e)
    report("offset / scale of scale_data at a capped size (relative)", worst, 1e-6)


# ---- mu-law, one-hot, argmax ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
def test_mulaw_encode_against_the_oracle_and_the_closed_form(dev, n):
    x = C.mulaw_input(n)
    xd = up(x, dev)
    for ch in C.MULAW_CHANNELS:
        codes = ops.mulaw_encode(xd, ch)
        assert codes.dtype == torch.int64 and codes.shape == (n,)
        got = cpu(codes)
        assert np.array_equal(got, O.mulaw_encode(torch.from_numpy(x), ch).numpy()), ch
        q = C.mulaw_q64(x, ch)
        band = C.mulaw_band(q)
        want = np.trunc(q).astype(np.int64)
        assert np.array_equal(got[~band], want[~band]), ch
        assert np.abs(got[band] - want[band]).max(initial=0) <= 1, ch
        print("FIGURE mulaw_encode n %d channels %d: %d of %d samples in the band, %d of them differ"
              % (n, ch, int(band.sum()), n, int((got != want).sum())))


@pytest.mark.parametrize("n", C.SIZES)
def test_mulaw_decode_int_and_float_codes(dev, n):
    worst = 0.0
    for ch in C.MULAW_CHANNELS:
        codes = (np.arange(n, dtype=np.int64) * 7 + 3) % ch
        a = cpu(ops.mulaw_decode(up(codes, dev), ch))
        b = cpu(ops.mulaw_decode(up(codes.astype(f32), dev), ch))
        assert a.dtype == np.float32 and C.same_bits(a, b), ch
        ref = C.mulaw_decode_ref(codes, ch)
        worst = max(worst, float((np.abs(a - ref) / (1e-7 + 2e-6 * np.abs(ref))).max()))
        assert np.allclose(a, ref, rtol=2e-6, atol=1e-7), ch
    report("mulaw_decode n %d (error / (1e-7 + 2e-6 |ref|))" % n, worst, 1.0)


@pytest.mark.parametrize("shape,classes,channel_major", C.ONEHOT)
def test_onehot_both_layouts(dev, shape, classes, channel_major):
    x = torch.from_numpy(np.random.RandomState(17).randint(0, classes, shape).astype(np.int64))
    got = ops.onehot(x.to(dev), classes, channel_major=channel_major)
    ref = torch.nn.functional.one_hot(x, classes)
    if channel_major:
        ref = ref.transpose(-1, -2).contiguous()
    assert got.dtype == torch.int64 and got.shape == ref.shape and torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("rows,cols", C.ARGMAX)
def test_argmax_last_first_maximum_first_nan(dev, rows, cols):
    for floating in (True, False):
        a = torch.from_numpy(C.argmax_rows(rows, cols, floating))
        got = ops.argmax_last(a.to(dev)).cpu()
        ref = a.argmax(-1)
        bad = torch.nonzero(got != ref).flatten()[:5].tolist()
        assert got.dtype == torch.int64 and got.shape == (rows,)
        assert not bad, (floating, bad, [a[i].tolist()[:8] for i in bad[:2]], got[bad].tolist(), ref[bad].tolist())


# ---- a block per stream past the grid limit --------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n", C.OADD_INVERT)
def test_oadd_invert_past_65535_streams(dev, S, n):
    frames = C.randn32(S * n * C.OADD_N_FFT, 18).reshape(S, n, C.OADD_N_FFT)
    tail = C.randn32(S * C.OADD_KEEP, 19).reshape(S, C.OADD_KEEP)
    gain = scalar(1.5, dev)
    fd = up(frames, dev)
    worst = 0.0
    for t in (tail, None):
        td = up(t, dev) if t is not None else None
        out, new_tail = ops.oadd_invert(fd, td, C.OADD_N_FFT, C.OADD_HOP, C.OADD_KEEP, gain)
        want_out, want_tail = C.oadd_invert_ref(frames, t, 1.5)
        e = max(C.rel_max(cpu(out), want_out), C.rel_max(cpu(new_tail), want_tail))
        worst = max(worst, e)
        assert out.shape == want_out.shape and e < C.OADD_BAR, e
        if t is not None:
            out2, tail2 = ops.oadd_invert(fd, td, C.OADD_N_FFT, C.OADD_HOP, C.OADD_KEEP, gain, in_place=True)
            assert tail2 is td and C.same_bits(cpu(out2), cpu(out)) and C.same_bits(cpu(td), cpu(new_tail))
    report("oadd_invert S %d frames %d" % (S, n), worst, C.OADD_BAR)


# ---- resample ---------------------------------------------------------------------------------------------------------------
def test_resample_short_clips_block_edges_and_the_row_limit(dev):
    from acids_transforms_amd.utils.audio_io import sinc_filter_bank
    h, width = sinc_filter_bank(C.RESAMPLE_ORIG, C.RESAMPLE_NEW)
    hd = h.to(dev)
    worst = 0.0
    for rows, L in C.RESAMPLE:
        x = C.randn32(rows * L, 20).reshape(rows, L)
        got = cpu(ops.resample_sinc(up(x, dev), C.RESAMPLE_ORIG, C.RESAMPLE_NEW, width, hd))
        ref = C.resample_ref(x, h.numpy(), width)
        assert got.shape == ref.shape == (rows, C.resample_out_len(L))
        e = C.rel_max(got, ref)
        worst = max(worst, e)
        assert e < C.RESAMPLE_BAR, (rows, L, e)
    report("resample", worst, C.RESAMPLE_BAR)
    rows, L = C.RESAMPLE_TOO_MANY
    with pytest.raises(AcidsHipError):                                    # more rows than grid.y holds: refused, not wrong
        ops.resample_sinc(torch.zeros(rows, L, device=dev), C.RESAMPLE_ORIG, C.RESAMPLE_NEW, width, hd)


# ---- the one-thread-per-output projection -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MEL, ids=lambda c: c.name)
def test_projection_one_thread_per_output(dev, case):
    x, bank = C.mel_inputs(case)
    off, sc = (scalar(C.MEL_AFFINE[0], dev), scalar(C.MEL_AFFINE[1], dev)) if case.norm else (None, None)
    if case.inverse:
        got = ops.mel_inverse(up(x, dev), up(bank, dev), case.contrast, off, sc)
    else:
        got = ops.mel_forward(up(x, dev), up(bank, dev), case.contrast, off, sc, channel_major_T=case.T)
    ref = C.mel_ref(case, x, bank)
    assert tuple(got.shape) == ref.shape
    e = C.rel_max(cpu(got), ref)
    report("projection " + case.name, e, C.PARITY)
    assert e < C.PARITY

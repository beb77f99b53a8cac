/*
 * acids_hip.h -- C ABI of libacids_hip.so, the MI355X (gfx950) implementation
 * of the spectral hot path of acids_transforms.
 *
 * The reference is pure Python on torch CPU ops and has no FFI layer
 * (SURVEY.md 8b); every entry point below therefore cites the reference
 * *call site* it replaces (paths relative to acids_transforms/).  A maintainer
 * binds these with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - complex64 arrays are interleaved float pairs (re, im);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     all work is asynchronous on that stream; nothing allocates or
 *     synchronises except at_init();
 *   - return value: 0 on success, a negative AT_E* code otherwise; nothing
 *     throws across the boundary;
 *   - shapes use the reference's conventions: audio (B, L) float32, spectra
 *     (B, T, F) with F = n_fft/2 + 1, T = 1 + L / hop (center=True).
 */
#ifndef ACIDS_HIP_H
#define ACIDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AT_OK 0
#define AT_EINVAL (-1)     /* bad argument (size, null pointer, alignment) */
#define AT_EUNSUPPORTED (-2) /* valid in the reference, not implemented here (e.g. non power-of-two n_fft) */
#define AT_ENOTINIT (-3)   /* at_init() was not called for the current device */
#define AT_EWORKSPACE (-4) /* workspace too small */
#define AT_ELAUNCH (-5)    /* HIP launch / runtime error */

/* Returns 4.  History: 4 in round 4 (at_set_variant / at_get_variant).  Earlier history: 2 early in round 2 (at_sinebank_realtime gained the window argument; at_mel_*bf16*, at_oadd_push
 * added); 3 later in round 2 (at_pghi_realtime_seeded, at_phase_*_strided / _polar, at_cartesian_*).  Round 3 changed
 * kernels only: no signature moved. */
int at_abi_version(void);
const char *at_error_string(int code);

/* Kernel variants.  The library decides from a call's arguments which kernel runs; it reads NO environment variables
 * (the A/B switches of tools/ab*.sh exist only in -DAT_DEV_SWITCHES builds).  Where two kernels compute the same
 * result -- a form specialised for the headline shapes and the generic one -- this process-wide table lets a caller force
 * the generic one; the parity tests use it to compare the two.  No reference counterpart (the reference has one
 * implementation of everything).  value: 0 = default (0..4 for the kernel variants, 0..65535 for the plan variants);
 * returns AT_EINVAL for an unknown variant or value. */
#define AT_VARIANT_EPILOGUE 0          /* 1: generic mel epilogue / projection even for the 128-mel headline bank */
#define AT_VARIANT_FRAME_KERNELS 1     /* 1: frame-at-a-time forward at n_fft 512 / 2048 / 4096 (no sliding window) */
#define AT_VARIANT_SMALL_PROJECTION 2  /* 1: row kernel instead of the matrix-core form of the K <= 128 projection */
#define AT_VARIANT_SCAN_LAYOUT 3       /* 1: flattened columns instead of one block per clip in the phase scans */
#define AT_VARIANT_PGHI_KERNEL 4       /* 1: winner-bit offline heap kernel; 2: single-lane heap kernels; 3: realtime
                                        * flood on the heap only; 4: realtime flood on the rank bitmap / heap, without the
                                        * wavefront-parallel scan path (round 5) that is tried first by default */
#define AT_VARIANT_ISTFT_RUNS 5        /* 1: n_fft-1024 inverse as one long run per wave even for full batches (no workgroup
                                        * tiles with the overlap state handed over through LDS) */
/* Plan variants (round 6; table entries, no signature changed: ABI still 4).  value 0..65535, 0 = the launcher's plan. */
#define AT_VARIANT_RUN_LENGTH 6        /* v: runs of v units clamped to [8, units] (frames; frame pairs at n_fft 512; output
                                        * hops for the inverses) for the streaming STFT / ISTFT launchers: the n_fft-1024
                                        * forward (fused forms included), the 512 / 2048 / 4096 sliding-window forwards, the
                                        * long-run n_fft-1024 inverse and the fused 512 / 2048 / 4096 inverses (hop n/8,
                                        * n/4, n/2; complex and polar input) */
#define AT_VARIANT_ISTFT_TILE 7        /* v: hop-256 non-Griffin-Lim n_fft-1024 inverse (T >= 64) on workgroup tiles at any
                                        * batch, max(v, 6) frames per wave, no balancing; AT_VARIANT_ISTFT_RUNS = 1 wins */
#define AT_VARIANT_ROW_RUN 8           /* v: row cut of the projection kernels clamped to [1, total]: v rows per wave (banded,
                                        * fixed 513-bin, small row form; small MFMA form: v rounded up to 32), v frame pairs /
                                        * frames per wave (n_fft-512 / 2048 features-only forward), v 32-row tiles per
                                        * workgroup (dense MFMA GEMM), v 128-row tiles per workgroup (bf16 projection) */
#define AT_VARIANT_FRAME_WALKERS 9     /* v: min(v, frames) workgroups walk the frames of the fallback STFT kernels (generic and
                                        * mixed radix), min(v, blocks) blocks stride the overlap-add gather; same bits */
int at_set_variant(int which, int value);
int at_get_variant(int which);

/* One-time per-device setup (twiddle tables).  Synchronous; call before capture. */
int at_init(int device);

/* ---- K1/K2/K4: forward ------------------------------------------------ */
/* torch.stft(x, n_fft, hop, window, center=True, pad_mode="reflect",
 * onesided=True, return_complex=True).transpose(-2,-1)
 *     replaces transforms/stft.py:98-104 and transforms/dgt.py:64-70.
 * center=0: frame t starts at sample t*hop of its clip, zero padded past L
 *     (utils/misc.py:148-165 frame()) then rfft(x*window):
 *     replaces stft.py:249-253 / dgt.py:285-289 on OverlapAdd.forward output
 *     (oadd.py:69-74) without materialising the frames.
 * phase (optional, may be NULL): atan2(im, re) of every bin = the reference's
 *     phase_buffer side effect (stft.py:103).
 * Speed, not correctness (round 3): at n_fft 512 / 1024 / 2048 / 4096 with hop = n_fft / 4, center = 1, no phase
 *     output, clips starting on 16-byte boundaries (8 for n_fft <= 1024) and `out_complex` 512-byte aligned, the
 *     sliding-window kernels with aligned non-temporal stream stores run (0.59 - 0.64 of the HBM roofline); any other
 *     arguments take the frame-at-a-time / row-store kernels with identical results to 1e-6. */
int at_stft_forward(const float *x, int64_t B, int64_t L, int64_t clip_stride, int64_t T, int n_fft, int hop,
                    int center, const float *window, float *out_complex, float *phase, void *stream);

/* Fused forward for Compose(STFT|DGT -> Magnitude(mel)) and for MFCC (n_fft = 1024, hop = 256):
 * the same framing + rFFT kernel additionally emits normalise(contrast(|X|^p @ bank)) from registers, so
 * the spectrum is not re-read (spectral_repr.py:215-226 / mel.py:43-44,68-73 behind stft.py:98-104).
 * The bank is passed in banded form, as the walk of the kernel's epilogue: in pass q (n_passes <= 16) lane l
 * of a wavefront sums filter lane_filter[q*64 + l] (-1: none) over pass_len_host[q] bins starting at bin
 * lane_start[q*64 + l]; both arrays are DEVICE int32[n_passes*64], pass_len_host is a HOST array of
 * multiples of 4 (<= 128), lane_start entries are multiples of 4 with lane_start + pass_len <= 640.
 * band_weights (DEVICE, 16-byte aligned): the 4 weights lane l applies in step j of pass q are the floats at
 * ((quad_base[q] + j)*64 + l)*4, quad_base[q] = sum_{q' < q} pass_len[q']/4; zero outside the filter's band;
 * 64 * sum(pass_len) <= 8192 floats.  (utils/banded.py builds these from a dense bank and chooses the lanes so
 * that the LDS reads of the walk are bank-conflict free.)
 * Exact for any bank whose columns are zero outside their band; dense banks use at_mel_project.
 * out_complex_or_null == NULL: features only (MFCC).
 * feat: (B*T, n_filters), or (B, n_filters, T) when feat_channel_major.
 * n_fft = 1024; hop = 256, or 128 / 512 with row-major features (else AT_EUNSUPPORTED).
 * n_fft = 2048 (window 16-byte aligned) or 512, any hop (here lane_start + pass_len <= n_fft/2 + 1 + 128): features
 * only -- out_complex_or_null and phase_or_null must be NULL -- either layout: MelSpectrogram / MFCC in one kernel
 * (stft2048.hip, stft512.hip), the spectrum is never written. */
int at_stft_mel_forward(const float *x, int64_t B, int64_t L, int64_t clip_stride, int64_t T, int n_fft, int hop,
                        const float *window, const int32_t *lane_filter, const int32_t *lane_start,
                        const float *band_weights, int n_filters, int n_passes, const int32_t *pass_len_host,
                        int contrast, int power2, const float *offset, const float *scale, float eps,
                        float *out_complex_or_null, float *phase_or_null, float *feat, int feat_channel_major,
                        void *stream);

/* Compose(STFT -> Polar) in one kernel (spectral_repr.py:511-523 behind stft.py:98-104): framing + rFFT, then
 * out[r, 0, :] = normalise(contrast(|X| @ bank)) (banded bank with F = 513 filters, tables as above) and
 * out[r, 1, :] = normalise(angle X), r = clip * T + frame; out_stacked: (B*T, 2, F).  The complex spectrum
 * is never written. */
int at_stft_polar_forward(const float *x, int64_t B, int64_t L, int64_t clip_stride, int64_t T, int n_fft, int hop,
                          const float *window, const int32_t *lane_filter, const int32_t *lane_start,
                          const float *band_weights, int n_filters, int n_passes, const int32_t *pass_len_host,
                          int contrast, const float *mag_offset, const float *mag_scale, float eps,
                          const float *phase_offset, const float *phase_scale, float *out_stacked, void *stream);

/* ---- K3/K5/K15: inverse ------------------------------------------------ */
/* 2^R x hop table of window^2 sums (R = n_fft / hop = 2, 4 or 8: the frames that overlap one hop) used by the fused
 * at_istft path, n_fft = 1024 with hop = 512, 256 (the reference's default) or 128 -- torch.istft's window envelope
 * (stft.py:126-127) for every combination of present / missing neighbour frames.  env16: 2^R * hop floats.
 * Other ratios: AT_EUNSUPPORTED (at_istft then takes its workspace path). */
int at_istft_envelope_table(const float *inv_window, int n_fft, int hop, float *env16, void *stream);

/* Bytes of workspace at_istft needs: B * T * n_fft floats, or 0 for the fused shapes (n_fft 512 / 1024 / 2048 / 4096 at
 * hop n/8, n/4, n/2).  The zero holds for a 16-byte aligned inv_window (and env16 and y): a less aligned pointer takes
 * at_istft off the fused kernels, and it then returns AT_EWORKSPACE, launching nothing, unless B * T * n_fft floats are
 * passed all the same. */
size_t at_istft_workspace_bytes(int64_t B, int64_t T, int n_fft, int hop);

/* torch.istft(X.transpose(-2,-1), n_fft, hop, window=inv_window, onesided=True)
 *     replaces stft.py:120-128, dgt.py:86-93 (complex input: X != NULL), and
 *     `x * exp(1j*phase)` + istft, stft.py:157-161 / dgt.py:152-154
 *     (polar input: X == NULL, mag and phase given).
 * y: (B, hop*(T-1) + (n_fft & 1)) -- torch.istft trims n_fft/2 (floor) at both ends.  Any n_fft in [2, 16384] (odd
 * sizes below 8192): powers of two on the kernels named below, everything else on the mixed-radix kernels of
 * stft_mixed.hip (the same holds for at_stft_forward and at_irfft_frames).  env16 (at_istft_envelope_table) is
 * required for n_fft = 1024, 512, 2048 and 4096 with hop = n_fft/8, n_fft/4 or n_fft/2 -- the fused kernels, for which
 * at_istft_workspace_bytes is 0 -- and may be NULL otherwise.  n_fft = 128, 256, 512, 2048 and 4096 run on the
 * register FFT core (stft_small.hip, stft512.hip, stft2048.hip, stft4096.hip), the other powers of two on the generic
 * LDS kernel.  n_fft = 1024, hop = 256: a batch with at least two tiles of ~175 frames for every workgroup the chip
 * holds runs as workgroup tiles (the overlap state crosses the cuts between a workgroup's waves through LDS), anything
 * smaller as one run per wave; the window is taken inside the accumulation (fma, frame order) in both, so a clip's bits
 * do not depend on the batch it rides in (AT_VARIANT_ISTFT_RUNS = 1 forces the long runs). */
int at_istft(const float *X_complex, const float *mag, const float *phase, int64_t B, int64_t T, int n_fft, int hop,
             const float *inv_window, const float *env16, float *y, void *workspace, size_t workspace_bytes,
             void *stream);

/* torch.fft.irfft(X) * inv_window on (nframes, F) -> (nframes, n_fft)
 *     replaces stft.py:260-266,308-310 / dgt.py:296-302,325-328.
 * The call is ONE stream: at n_fft = 128 / 256 / 512, where 8 / 4 / 2 consecutive frames share a register FFT, a
 * frame's rounding (and a NaN) can reach its up to K - 1 neighbours in the call.  Frames of independent streams go
 * through at_irfft_frames_streams. */
int at_irfft_frames(const float *X_complex, const float *mag, const float *phase, int64_t nframes, int n_fft,
                    const float *inv_window, float *frames, void *stream);

/* The same on (nframes / frames_per_stream) independent streams of frames_per_stream consecutive frames each
 * (nframes % frames_per_stream == 0, else AT_EINVAL): frames share a transform within a stream only, the last
 * transform of a stream is filled with zeros, so a stream's output -- bits, accuracy, finiteness -- does not depend on
 * the other streams of the call.  frames_per_stream = 1: one frame per transform. */
int at_irfft_frames_streams(const float *X_complex, const float *mag, const float *phase, int64_t nframes,
                            int64_t frames_per_stream, int n_fft, const float *inv_window, float *frames,
                            void *stream);

/* ---- K8-K12: magnitude / mel projection ---------------------------------- */
/* a_kind: 0 = complex64 input, |.| taken on load; 1 = complex64, |.|^2 (power=2);
 *         2 = float32 input; 3 = float32 input, |.| taken.   contrast: 0 none, 1 log1p, 2 log, 3 log10.
 * forward (inverse=0):  out = normalise(contrast(A' @ bank))
 *     replaces  x.abs(); torch.matmul(mag, mel_bank); contrast; Normalize.forward
 *     (spectral_repr.py:215-226, norm.py:40-41) and, with a_kind=1 and
 *     T_transposed=T, torchaudio MelSpectrogram's |stft|^2 @ fbank with its
 *     channel-major (..., n_mels, T) output (mel.py:43-44, 68-73).
 * inverse (inverse=1, a_kind=2): out = invert_contrast(A*scale+offset) @ bank
 *     replaces  Normalize.invert; invert_contrast; matmul(mag, inverse_mel_bank)
 *     (spectral_repr.py:228-240, norm.py:43-44).
 * A: rows x K with row stride lda (elements); bank: K x N row-major, stride ldb;
 * out: rows x N with stride ld_out, or (rows/T, N, T) when T_transposed > 0.
 * offset/scale: device scalars, both NULL = no normalisation.  Exact fp32 MFMA. */
int at_mel_project(const void *A, int a_kind, int64_t rows, int64_t lda, int K, const float *bank, int ldb, int N,
                   int contrast, int inverse, const float *offset, const float *scale, float eps, float *out,
                   int64_t ld_out, int64_t T_transposed, void *stream);

/* The forward projection as a dense bf16 MFMA GEMM with fp32 accumulation (v_mfma_f32_32x32x16_bf16): BASELINE
 * config 5's "bf16 MFMA mel".  Same chain as at_mel_project with inverse = 0 -- normalise(contrast(A' @ bank)),
 * spectral_repr.py:215-226 -- but A' (|x|, |x|^2 or the real input) and the bank are rounded to bf16 (nearest even)
 * before the products; sums are fp32.  ~4e-3 relative to the fp32 chain: opt-in only (Magnitude(bank_dtype="bf16")),
 * never the default.  The bank is passed as the packed operand image written by at_mel_bf16_pack_bank
 * (at_mel_bf16_bank_bytes(K, N) bytes, 16-byte aligned): [ceil32(N)][ceil16(K)] bf16, k contiguous, zero padded.
 * out: rows x N fp32, row stride ld_out.  K up to 4096 (one 32-column tile of the bank must fit in LDS), else
 * AT_EUNSUPPORTED. */
size_t at_mel_bf16_bank_bytes(int K, int N);
int at_mel_bf16_pack_bank(const float *bank, int K, int ldb, int N, void *bank_bf16, void *stream);
int at_mel_project_bf16(const void *A, int a_kind, int64_t rows, int64_t lda, int K, const void *bank_bf16, int N,
                        int contrast, const float *offset, const float *scale, float eps, float *out, int64_t ld_out,
                        void *stream);

/* Magnitude with mel=False: the same chains without the projection (n elements). */
int at_mag_pointwise(const void *A, int a_kind, int64_t n, int contrast, int inverse, const float *offset,
                     const float *scale, float eps, float *out, void *stream);

/* {min, max, sum, sum of squares} (fp64) of contrast(|A|) over n elements:
 *     Normalize.scale_data (norm.py:25-38) / Magnitude.scale_data (spectral_repr.py:242-245). */
size_t at_stats_workspace_bytes(void);
int at_stats(const void *A, int a_kind, int64_t n, int contrast, float eps, double *out4, void *workspace,
             size_t workspace_bytes, void *stream);

/* Normalize.forward (inverse=0): (x-offset)/scale;  Normalize.invert (inverse=1): x*scale+offset
 *     (norm.py:40-44); offset/scale are device scalars. */
int at_affine(const float *x, int64_t n, const float *offset, const float *scale, int inverse, float *out,
              void *stream);

/* ---- K13/K14: PGHI --------------------------------------------------------- */
/* DGT.modgabphasegrad (dgt.py:222-236) on B clamped-on-the-fly (T,F) magnitude
 * arrays: tgradw, fgradw (B,T,F).  spec_or_null receives clamp(mag, eps). */
int at_pghi_gradients(const float *mag, int64_t B, int T, int F, float gamma, int n_fft, int hop, float eps,
                      float *tgradw, float *fgradw, float *spec_or_null, void *stream);

size_t at_pghi_offline_workspace_bytes(int64_t B, int T, int F);

/* DGT.pghi + perform_hgi for every clip of a batch (dgt.py:137-141, 156-220) with
 * the binary-heap order of utils/heapq.py:9-59.  abstol is both the clamp floor
 * and the "visited" marker (the reference passes eps for both, dgt.py:157-162).
 * phase: (B,T,F).  npops_or_null: (B) pops per clip.  order_or_null: (B, T*F)
 * row*F+col of every pop in order (parity tests).
 * T * F <= 2^26 - 64 bins per clip (32-bit heap positions; 12 minutes of audio at the default sizes), else
 * AT_EUNSUPPORTED. */
int at_pghi_offline(const float *mag, int64_t B, int T, int F, float gamma, int n_fft, int hop, float tol,
                    float abstol, float *phase, void *workspace, size_t workspace_bytes, int64_t *npops_or_null,
                    int32_t *order_or_null, void *stream);

/* DGT.perform_hgi (dgt.py:168-220) on its own: the heap integration of B (T,F) magnitude arrays along gradients the
 * CALLER supplies (tgradw is applied along the bin axis, fgradw along the frame axis, as the reference's method uses
 * them), same pop order, same threshold rule (bins below tol * max are never visited).  mag is not modified (the
 * reference integrates in its argument); workspace as for at_pghi_offline. */
int at_pghi_integrate(const float *mag, const float *tgradw, const float *fgradw, int64_t B, int T, int F, float tol,
                      float abstol, float *phase, void *workspace, size_t workspace_bytes, int64_t *npops_or_null,
                      int32_t *order_or_null, void *stream);

size_t at_pghi_rt_workspace_bytes(int S, int n, int F);

/* RealtimeDGT.pghi (dgt.py:338-354, 378-466) for S streams: mag_hist (S,2,F),
 * mag (S,n,F), prev_phase (S,F), noise (S,n,F) standard-normal draws for the bins
 * at or below the tolerance (dgt.py:404-405) -> phase (S,n,F).  The time-border
 * rows the reference leaves uninitialised (dgt.py:388-394) are defined as 0.
 * tgradw/fgradw_or_null: optional (S,n+2,F) outputs. */
int at_pghi_realtime(const float *mag_hist, const float *mag, const float *prev_phase, const float *noise, int S,
                     int n, int F, float gamma, int n_fft, int hop, float tol, float eps, float *phase,
                     float *tgradw_or_null, float *fgradw_or_null, void *workspace, size_t workspace_bytes,
                     void *stream);

/* The same with the standard-normal draws of dgt.py:404-405 (torch.randn_like) made on the device, so that a captured
 * streaming step needs no generator launch: Philox-4x32-10 keyed by rng_state[0..1] (seed), counter = (bin index,
 * rng_state[2]); the call advances rng_state[2] by one.  rng_state: 4 x uint32 in device memory, owned by the caller
 * (one per session).  Statistical parity only: the draws are not torch's. */
int at_pghi_realtime_seeded(const float *mag_hist, const float *mag, const float *prev_phase, uint32_t *rng_state, int S,
                            int n, int F, float gamma, int n_fft, int hop, float tol, float eps, float *phase,
                            void *workspace, size_t workspace_bytes, void *stream);

/* RealtimeDGT.update_buffers (dgt.py:330-336) for x = mag*exp(i*phase):
 * hist_out = |x[-2:]| (or [hist_in[1], |x[-1]|] when n == 1), phase_out = angle(x[-1]).  hist_out may alias hist_in
 * (every bin reads its history before it writes it). */
int at_rt_update_buffers(const float *mag, const float *phase, int S, int n, int F, const float *hist_in,
                         float *hist_out, float *phase_out, void *stream);

/* ---- pointwise ----------------------------------------------------------- */
/* x.angle() on n complex64 values: the phase_buffer of stft.py:103 / dgt.py:69,
 * and hgi_phase_buffer of dgt.py:336. */
int at_angle(const float *x_complex, int64_t n, float *out, void *stream);

/* Cartesian.forward / invert (spectral_repr.py:403-428) in one pass: (rows, F) complex64 <-> (rows, 2, F) float32
 * with [r, 0, :] = (x.real - re_offset) / re_scale and [r, 1, :] = (x.imag - im_offset) / im_scale (Normalize,
 * norm.py:40-44; a NULL offset/scale pair: that half is not normalised); unpack applies y * scale + offset. */
int at_cartesian_pack(const float *x_complex, int64_t rows, int F, const float *re_offset, const float *re_scale,
                      const float *im_offset, const float *im_scale, float *stacked, void *stream);
int at_cartesian_unpack(const float *stacked, int64_t rows, int F, const float *re_offset, const float *re_scale,
                        const float *im_offset, const float *im_scale, float *out_complex, void *stream);

/* ---- Griffin-Lim building blocks (STFT's default inversion mode, stft.py:37,174-178) ---- */
/* One phase update of torchaudio.functional.griffinlim:  a = rebuilt - m*tprev (tprev may be NULL);
 * X = mag * a / (|a| + 1e-16), with m = momentum / (1 + momentum).  n complex elements. */
int at_griffinlim_update(const float *mag, const float *rebuilt_complex, const float *tprev_complex_or_null,
                         float momentum_over_1p, int64_t n, float *X_complex, void *stream);
/* The same update fused into the inverse: at_istft(mag * normalise(rebuilt - m' * tprev)) in one kernel, the updated
 * spectrum never written (one Griffin-Lim iteration = this + at_stft_forward).  n_fft = 1024, hop 128 / 256 / 512 with
 * env16 from at_istft_envelope_table; anything else: AT_EUNSUPPORTED (use at_griffinlim_update + at_istft). */
int at_istft_griffinlim(const float *mag, const float *rebuilt_complex, const float *tprev_complex_or_null,
                        float momentum_over_1p, int64_t B, int64_t T, int n_fft, int hop, const float *inv_window,
                        const float *env16, float *y, void *stream);
/* X = mag * z (z complex): the random initialisation of the same algorithm. */
int at_scale_complex(const float *mag, const float *z_complex, int64_t n, float *X_complex, void *stream);

/* ---- K6/K7: OverlapAdd streaming framer / overlap-add ---------------------- */
/* OverlapAdd.forward (oadd.py:69-74, 33-42): buf (S, buf_len) = [history | chunk | 0...],
 * hist_out = last `keep` samples of [history | chunk].  The caller takes the
 * (S, n, n_fft) frames as a strided view of buf (utils/misc.py:148-165).  C < keep (down to one hop per step) is
 * an extension: the reference's own state breaks there (oadd.py:41); the frame sequence is that of any other
 * chunking of the same sample stream. */
int at_oadd_forward(const float *x, const float *hist_in_or_null, int S, int64_t C, int keep, int64_t buf_len,
                    float *buf, float *hist_out, void *stream);
/* OverlapAdd.invert (oadd.py:90-104): frames (S, n, n_fft) + carried tail (S, keep)
 * -> out (S, (n-1)*hop + n_fft - keep) / gain, tail_out (S, keep) undivided.  tail_out may alias tail_in_or_null
 * (state updated in place); n = 1 emits one hop.  keep <= 16384. */
int at_oadd_invert(const float *frames, const float *tail_in_or_null, int S, int n, int n_fft, int hop, int keep,
                   const float *gain, float *out, float *tail_out, void *stream);
/* The input side of the same state kept in place (streaming sessions, hipGraph replay): buf (S, buf_len) holds
 * [history(keep) | chunk(C) | pad]; one call moves the last `keep` samples of [history | chunk] to the front and
 * writes the new chunk x (S, C) behind them (oadd.py:33-42, 69-74).  Any C >= 1; buf_len >= keep + C. */
int at_oadd_push(const float *x, int S, int64_t C, int keep, int64_t buf_len, float *buf, void *stream);

/* ---- K16: integer transforms -------------------------------------------------- */
/* torchaudio MuLawEncoding / MuLawDecoding as used by MuLaw (raw.py:282-283, 316):
 * codes int64 in [0, channels). */
int at_mulaw_encode(const float *x, int64_t n, int channels, int64_t *codes, void *stream);
int at_mulaw_decode(const int64_t *codes_i64, const float *codes_f32, int64_t n, int channels, float *x,
                    void *stream);
/* F.one_hot(x, classes) (misc.py:183-185, raw.py:288-291): out (n, classes) int64, or with
 * channel_major_inner = t > 0 the transposed (n/t, classes, t) layout of raw.py:289-290. */
int at_onehot(const int64_t *x, int64_t n, int classes, int64_t channel_major_inner, int64_t *out, void *stream);
/* Tensor.argmax(-1) (misc.py:188-189): first index of the row maximum. */
int at_argmax_last(const int64_t *x_i64, const float *x_f32, int64_t rows, int cols, int64_t *out, void *stream);

/* The same projection for a BANDED bank (mel banks, the reference's default 513 x 513 one and its inverse
 * included): the K inputs of a frame go through the prologue into LDS and every lane walks the band of
 * one filter per pass -- the walk tables are those of at_stft_mel_forward (utils/banded.py).  HBM-bound (input
 * row in, n_filters floats out) where the dense contraction is MFMA-bound.  Arguments as at_mel_project.
 * Limits (wider than the fused epilogue's): K <= 2112 (every n_fft up to 4096), n_passes <= 40, pass_len <= 512,
 * and weight table + lane tables + one LDS row per wave within 160 KB (AT_EUNSUPPORTED otherwise: use
 * at_mel_project).
 * phase_out != NULL (complex input): also writes normalise(angle(x)) with row stride ld_phase -- Polar.forward
 * (spectral_repr.py:432-439) fills its stacked (.., T, 2, F) result in one pass over the spectrum.
 * phase_in != NULL (inverse only): `out` is complex64, out[r, f] = acc * exp(i * (phase_in[r*ld_phase + f] *
 * phase_scale + phase_offset)) -- Polar.invert (spectral_repr.py:441-451) in one pass. */
int at_mel_project_banded(const void *A, int a_kind, int64_t rows, int64_t lda, int K, const int32_t *lane_filter,
                          const int32_t *lane_start, const float *band_weights, int n_filters, int n_passes,
                          const int32_t *pass_len_host, int contrast, int inverse, const float *offset,
                          const float *scale, float eps, float *out, int64_t ld_out, int64_t T_transposed,
                          float *phase_out, int64_t ld_phase, const float *phase_offset, const float *phase_scale,
                          const float *phase_in, void *stream);

/* normalise(x @ W) for a small real matrix (K <= 128, N <= 64): the DCT-II behind MFCC(n_mfcc).  K = 128 / 80 / 64 with
 * a 16-byte aligned x: fp32 MFMA tiles (v_mfma_f32_16x16x4_f32, fp32 accumulate); otherwise one wavefront per row with
 * W's columns in registers.  out: (rows, N), or channel-major (rows/T, N, T) when T_transposed > 0; x and out must not
 * overlap. */
int at_project_small(const float *x, int64_t rows, int K, const float *W, int N, const float *offset,
                     const float *scale, float *out, int64_t T_transposed, void *stream);

/* ---- phase-side representations ------------------------------------------ */
/* Scan along the frame axis of a (B, T, F) spectrum, one of X_complex / phase given (the angle is taken
 * inside), optional per-frame weight frame_window[T] and Normalize affine (device scalars) applied last:
 *   mode 0  unwrap(angle)                      utils/misc.py:12-26   (Phase(unwrap=True), spectral_repr.py:271-274)
 *   mode 1  IF "forward"   fdiff_forward(unwrap)/pi   rows [0, T-2]   utils/misc.py:65-68, spectral_repr.py:323-325
 *   mode 2  IF "backward"  fdiff_backward(unwrap)/-pi rows [1, T-1]   utils/misc.py:71-75, spectral_repr.py:320-322
 *   mode 3  IF "central"   fdiff_central(unwrap)/2pi  rows [1, T-2]   utils/misc.py:77-81, spectral_repr.py:326-328
 *   mode 4  angle only                                                   (Phase(unwrap=False))
 * bare != 0 (modes 1-3, real input in `phase`): the plain fdiff_* of utils/misc.py:65-81, no unwrap, no division.
 * Sequential in t per (clip, bin) column with torch's CPU arithmetic (double cumsum accumulator). */
int at_phase_scan(const float *X_complex, const float *phase, int64_t B, int64_t T, int64_t F, int mode, int bare,
                  const float *frame_window, const float *offset, const float *scale, float *out, void *stream);

/* IF.invert (spectral_repr.py:360-373): de-normalise (offset/scale may be NULL), undo the per-row scaling of
 * `method` (1 forward, 2 backward, 3 central; skipped when rescale == 0: the bare fint_* of utils/misc.py:83-104)
 * and integrate along t.  out != y. */
int at_phase_integrate(const float *y, int64_t B, int64_t T, int64_t F, int method, int rescale, const float *offset,
                       const float *scale, float *out, void *stream);

/* The same scan writing frames ld_out >= F floats apart: the phase half of a stacked (.., T, 2, F) representation is
 * filled in place (out = stacked + F, ld_out = 2 F) -- PolarIF.forward without the torch.stack copy. */
int at_phase_scan_strided(const float *X_complex, const float *phase, int64_t B, int64_t T, int64_t F, int mode, int bare,
                          const float *frame_window, const float *offset, const float *scale, float *out, int64_t ld_out,
                          void *stream);
/* PolarIF.forward in one pass (spectral_repr.py:505-537 = Magnitude.forward :186-200, :222-227 next to IF.forward :318-335,
 * :350-358, stacked on dim -2): X (B, T, F) complex64 -> out_stacked (B, T, 2, F) with [.., 0, :] =
 * normalise(contrast(|X| @ bank)) and [.., 1, :] = normalise(IF(X)) (`method`, frame_window, if_offset / if_scale as in
 * at_phase_scan).  The bank is given by filter (device arrays): band_start[f] first bin with a non-zero weight,
 * band_len[f] bins up to the last one (0: empty filter), band_off[f] offset of those weights in band_w (n_w floats;
 * start + len <= F, off + len <= n_w are the caller's to guarantee).  Both halves equal at_mel_project_banded's and
 * at_phase_scan_strided's bit for bit; the spectrum is read once.  One block per clip: AT_EUNSUPPORTED unless B >= 64,
 * 256 <= F <= 2048 (two-column clip blocks; the four-column form is not built for the magnitude side), rows that are not whole
 * 64-byte segments and a bank whose weights fit LDS beside eight rows --
 * the caller then runs those two entry points. */
int at_polarif_forward(const float *X_complex, int64_t B, int64_t T, int64_t F, int method, const float *frame_window,
                       const float *if_offset, const float *if_scale, const int *band_start, const int *band_len,
                       const int *band_off, const float *band_w, int64_t n_w, int contrast, const float *mag_offset,
                       const float *mag_scale, float eps, float *out_stacked, void *stream);
/* IF.invert fused with SpectralRepresentation.invert's mag * exp(i * phase) (spectral_repr.py:360-373, 449-451): y has
 * frames ld_y >= F floats apart (the phase half of a stacked tensor: y = stacked + F, ld_y = 2 F), mag is (B, T, F)
 * contiguous, out_complex (B, T, F) complex64. */
int at_phase_integrate_polar(const float *y, int64_t ld_y, int64_t B, int64_t T, int64_t F, int method, const float *offset,
                             const float *scale, const float *mag, float *out_complex, void *stream);

/* mag * exp(i * phase) -> complex64 (SpectralRepresentation.invert, spectral_repr.py:449-451). */
int at_polar_to_complex(const float *mag, const float *phase, int64_t n, float *out_complex, void *stream);

/* ---- sinebank inversion --------------------------------------------------- */
/* STFT/DGT.get_sinebank_inversion (stft.py:180-191): y[b, n] = sum_k env[b,k,n] sin(c_k t_n + phi_k), env = linear
 * interpolation of x / max|x| along time, / 2 pi.  x: (B, T, F) magnitudes; c[F] = fl(2 pi) f_k, t[L], phi[F]: the
 * reference's own fp32 frequency / time / random-phase vectors (host-computed with the same torch calls).  Per
 * 128-sample block cb of the output: block_frame_offset[p * nblocks + cb] (int64, elements) = F * (first frame the
 * block interpolates from + p), clamped to the last frame, p = 0..n_pass-1 (3 for hop >= 128); W[p * L + n] =
 * weight of that frame for sample n (zero where unused).  max_abs: device scalar max|x|.  out: (B, L), before the
 * final division by its max.  n_pass exact-fp32 MFMA contractions against one shared oscillator matrix + a
 * pointwise combine. */
size_t at_sinebank_workspace_bytes(int64_t B, int F, int64_t L, int n_pass);
int at_sinebank_offline(const float *x, int64_t B, int64_t T, int F, const float *c, const float *t, const float *phi,
                        int64_t L, int n_pass, const int64_t *block_frame_offset, const float *W, const float *max_abs,
                        float *out, void *workspace, size_t workspace_bytes, void *stream);

/* RealtimeSTFT/RealtimeDGT.get_sinebank_inversion (stft.py:276-291, dgt.py:356-371):
 * out[s, t, n] = (1/F) sum_k x[s, t, k] sin(c_k tau[t, n] + phi[s, k]);  x (S, T, F), tau (T, N), phi (S, F), out (S, T, N).
 * window_or_null (N floats): the frames are multiplied by it -- what invert(mode="sinebank") hands to OverlapAdd
 * (stft.py:303-304, dgt.py:321-322: get_sinebank_inversion(x) * inv_window). */
int at_sinebank_realtime(const float *x, int64_t S, int T, int F, int N, const float *c, const float *tau,
                         const float *phi, const float *window_or_null, float *out, void *stream);

/* ---- backward passes (autograd.py) ------------------------------------------------------------------------------
 * Gradients follow torch's convention for complex tensors: G = dL/dRe + i dL/dIm. */

/* Adjoint of at_stft_forward(center=1), i.e. the gradient of torch.stft(x, n_fft, hop, window, center=True,
 * pad_mode="reflect", return_complex=True) with respect to x (reference stft.py:98-104; DGT: dgt.py's forward, with its
 * ANALYSIS window).  With P = n_fft // 2, N = n_fft and G (B, T, N/2+1) complex64 the upstream gradient:
 *   q[t, m]  = w[m] Re sum_{k=0}^{N/2} G[t, k] e^{+2 pi i k m / N}     (each bin once: N irfft(G') with the interior bins
 *              halved; the imaginary parts of DC and Nyquist drop out)
 *   dp[j]    = sum_t q[t, j - t hop]                                   (overlap-add, frames ascending, no envelope)
 *   dx[i]    = dp[i + P] + dp[P - i] (i in [1, P]) + dp[2L + P - 2 - i] (i in [L - P - 1, L - 2])   (reflect fold)
 * dx: (B, L) float32.  T must be the forward's frame count 1 + (L - (n_fft & 1)) / hop, and L > n_fft / 2.  Any n_fft the
 * forward takes.  Runs the irfft kernels of at_irfft_frames on a window scaled by N/2, then one overlap-add + fold kernel
 * that adds the halves of DC and Nyquist back (autograd.hip).  workspace: at_stft_backward_workspace_bytes, 256-byte
 * aligned (the clips are processed in chunks whose frames fit 1 GiB).  Every sample is summed in a fixed order by one
 * thread: a clip's bits do not depend on the batch. */
size_t at_stft_backward_workspace_bytes(int64_t B, int64_t T, int n_fft, int hop);
int at_stft_backward(const float *G_complex, int64_t B, int64_t T, int64_t L, int n_fft, int hop, const float *window,
                     float *dx, void *workspace, size_t workspace_bytes, void *stream);

/* Adjoint of at_istft (torch.istft, center=True, onesided, length=None) -- its backward.  w = inv_window, N = n_fft,
 * h = hop, P = N + h (T-1), env[m] = sum of w[m - t h]^2 over the frames t that cover m (oldest first, w^2 rounded before
 * each add, as the modules' table STFT._make_env16), Ly = h (T-1) + (N & 1):
 *   u[m]     = gy[m - N/2] / env[m] for N/2 <= m < N/2 + Ly, 0 elsewhere (no division in the padding)
 *   gX[t, k] = (c_k / N) rfft(w u[t h .. t h + N))[k],  c_0 = 1, c_{N/2} = 1 (even N), c_k = 2 otherwise
 * gy: (B, Ly) float32.  phase NULL: out = gX, (B, T, F) complex64.  phase (B, T, F) float32 given (polar input
 * X = mag e^{i phase}): out = gmag = Re gX cos phase + Im gX sin phase, (B, T, F) float32; gX is not written.  Ly == 0
 * (T == 1, even N): zeros.  Any n_fft at_istft takes; complex out must be 8-byte aligned (AT_EINVAL), gy, phase and
 * the window may have any float alignment.  Chunks of clips go through u (one prep kernel, which sums the envelope per
 * sample), at_stft_forward's kernels with center = 0 on the window scaled by 2/N (the generic one-frame kernel at
 * n_fft 128 / 256 / 512) and a kernel that halves DC and Nyquist or writes gmag.  env16 is accepted for symmetry with
 * at_istft and not read.  workspace: at_istft_backward_workspace_bytes (> 0 for every shape), 256-byte aligned.  A
 * clip's bits depend neither on its batch nor on the chunking. */
size_t at_istft_backward_workspace_bytes(int64_t B, int64_t T, int n_fft, int hop);
int at_istft_backward(const float *gy, int64_t B, int64_t T, int n_fft, int hop, const float *inv_window,
                      const float *env16, const float *phase, float *out, void *workspace, size_t workspace_bytes,
                      void *stream);

/* Gradient of Magnitude.forward (reference spectral_repr.py:215-226) with respect to its input A (rows x K): a = |A|,
 * M = a @ bank (K x N; M = a when f_w is NULL, then N == K), f = (c(M) - offset) / scale, dF (rows x (N - col_off)) the
 * gradient of f[..., col_off:] (keep_nyquist=False: col_off = 1; the dropped columns get no gradient):
 *   dM = dF / scale * c'(M),  c' = 1/(1+M) (log1p), 1/M (log), 1/(M ln 10) (log10) -- the last two 0 where M < eps,
 *        torch.clamp's mask --, 1 (none);  scale NULL: no Normalize (offset never matters)
 *   dA[k] = sum_j bank[k, j] dM[j],   dX = dA X / |X| (0 where X == 0, torch's sgn); real A: dA sign(A).
 * a_kind: 0 complex64, 3 float32.  Banks by column (CSR): column j of the forward bank has f_len[j] weights at
 * f_w[f_off[j] ..] for rows f_start[j] ..; f_nnz: length of f_w; t_* the same tables of the transposed bank (K
 * columns).  M is recomputed from A (one wave per row, |A| and dM in LDS; the tables too when they fit).  dX_accum (NULL or rows x K of A's type) is added to the result: the
 * spectrum's own gradient in the fused STFT -> Magnitude chain.  The bf16 projection's backward is this fp32 one. */
int at_magnitude_backward(const void *A, int a_kind, int64_t rows, int K, const float *dF, int N, int col_off,
                          const int *f_start, const int *f_len, const int *f_off, const float *f_w, int f_nnz,
                          const int *t_start, const int *t_len, const int *t_off, const float *t_w, int t_nnz, int contrast, const float *scale,
                          float eps, const void *dX_accum, void *dX, void *stream);

/* Gradient of MFCC.forward (the reference's mel power spectrogram, transforms/mel.py:31-73, and the n_mfcc build
 * extension) with respect to the spectrum X (B, T, K) complex64 of its STFT, given dF (B, C, T) float32, the gradient of
 * the channel-major output.  a = |X|^power (power 1 or 2), M = a @ bank (K x N):
 *   dct_t NULL (C == N):  f = (M - offset) / scale,                      dM = dF / scale
 *   dct_t (C x N), the DCT matrix (N x C, the 10 / ln 10 of the dB scale folded in) TRANSPOSED:
 *                         f = (ln(max(M, 1e-10)) @ dct - offset) / scale,
 *                         dM[j] = (sum_c dct_t[c, j] dF[c] / scale) / M[j] where M[j] >= 1e-10, else 0 (torch.clamp's mask)
 *   dA[k] = sum_j bank[k, j] dM[j],   dX = 2 dA X (power 2),  dA X / |X| (power 1; 0 where X == 0, torch's sgn)
 * scale NULL: no Normalize (offset never matters).  Banks by column, as at_magnitude_backward: t_* the tables of the
 * transposed bank (K columns), always read; f_* those of the forward bank (N columns), read -- with M recomputed from
 * X -- only when dct_t is given, and may be NULL otherwise.  dX_complex may be X_complex (in place: every lane reads the
 * bins it owns before it writes them); both 8-byte aligned.  One workgroup per tile of 32 consecutive frames of one clip
 * (the last tile of a clip is short) transposes the tile of dF through LDS, then one wave per frame walks the bands; the
 * tables sit in LDS when they fit 160 KB, in global memory otherwise (mfcc_grad.hip).  A clip's bits depend neither on
 * the batch nor on how the caller chunks it.  AT_EINVAL on null or ill-sized arguments (no device is touched),
 * AT_EUNSUPPORTED when a tile of dF (C >= 1280) or one frame's rows do not fit LDS. */
int at_mfcc_backward(const float *X_complex, int64_t B, int64_t T, int K, const float *dF, int C, int N, int power,
                     const int *f_start, const int *f_len, const int *f_off, const float *f_w, int f_nnz,
                     const int *t_start, const int *t_len, const int *t_off, const float *t_w, int t_nnz,
                     const float *dct_t, const float *scale, float *dX_complex, void *stream);

/* Gradient of Magnitude.invert (reference spectral_repr.py:229-240: norm.invert -> zero pad -> invert_contrast ->
 * matmul(inverse_mel_bank)) with respect to its input y, the adjoint of at_mel_project_banded(inverse=1) /
 * at_mel_project(inverse=1) / at_mag_pointwise(inverse=1).  z = y * scale + offset (z = y when both are NULL),
 * x = c(z) @ W with W the (K x N) inverse bank and c the inverse contrast; g (rows x N) the gradient of x:
 *   dy[k] = scale * c'(z[k]) * sum_n W[k, n] g[n],   c' = exp(z) (log1p, log), ln 10 * 10^z (log10), 1 (none)
 * pad_last = 1 (keep_nyquist=False): y and dy have K - 1 columns -- the reference pads a zero as the LAST of the K
 * columns after de-normalising, so that column's gradient is dropped.  The bank travels as the by-column tables of W^T
 * (K columns, as at_magnitude_backward's t_*): column k holds t_len[k] weights at t_w[t_off[k] ..] for the outputs
 * t_start[k] ..; t_w NULL: mel=False (W = I, N == K), one thread per element.  With a bank: one wave per row, g of the
 * row in LDS, the tables too when they fit 160 KB beside four rows (otherwise read from global memory by up to four
 * waves per workgroup); every dy[k] is summed by one lane in ascending n, so a row's bits do not depend on the batch.
 * polar = 1: the one-pass Polar.invert (reference :441-452; at_mel_project_banded with phase_in).  y and dy are the
 * stacked (rows, 2, K) tensors (K == N, no pad), g = gX is complex64 (rows x N), phi = y_phase * phase_scale +
 * phase_offset (or y_phase), M = c(z) @ W recomputed by a forward walk over f_* (the by-column tables of W itself, N
 * columns; NULL and unread when polar = 0):
 *   gM[n] = Re gX cos phi + Im gX sin phi,   dy_phase[n] = phase_scale * M[n] * (Im gX cos phi - Re gX sin phi),
 *   dy_mag[k] = scale * c'(z[k]) * sum_n W[k, n] gM[n].
 * y, dy, a real g and the scalars may have any float (4-byte) alignment, a complex g must be 8-byte aligned.  AT_EINVAL on null or ill-sized
 * arguments (no device is touched), AT_OK and nothing touched for rows == 0, AT_EUNSUPPORTED when one row's slice does
 * not fit LDS. */
int at_magnitude_invert_backward(const float *y, int64_t rows, int K, int N, int pad_last, const void *g, int polar,
                                 const int *f_start, const int *f_len, const int *f_off, const float *f_w, int f_nnz,
                                 const int *t_start, const int *t_len, const int *t_off, const float *t_w, int t_nnz,
                                 int contrast, const float *offset, const float *scale, float eps,
                                 const float *phase_offset, const float *phase_scale, float *dy, void *stream);

/* Adjoint of at_polar_to_complex (SpectralRepresentation.invert, reference spectral_repr.py:449-451), X = mag e^{i phase}:
 *   gmag = Re gX cos phase + Im gX sin phase,   gphase = mag * (Im gX cos phase - Re gX sin phase)
 * over n elements; gmag or gphase may be NULL (that gradient is not wanted; mag is read only for gphase).  gX_complex
 * must be 8-byte aligned, every other pointer 4-byte aligned (AT_EINVAL otherwise, as on null arguments). */
int at_polar_to_complex_backward(const float *gX_complex, const float *mag, const float *phase, int64_t n, float *gmag,
                                 float *gphase, void *stream);

/* Adjoint of at_cartesian_unpack (Cartesian.invert, reference spectral_repr.py:497-508): gX (rows, F) complex64 ->
 * dy (rows, 2, F) float32 with dy[r, 0, :] = Re gX * re_scale and dy[r, 1, :] = Im gX * im_scale (a NULL scale: 1, that
 * half is not normalised).  gX_complex must be 8-byte aligned, dy_stacked and the scales 4-byte aligned (AT_EINVAL
 * otherwise, as on null arguments). */
int at_cartesian_unpack_backward(const float *gX_complex, int64_t rows, int F, const float *re_scale,
                                 const float *im_scale, float *dy_stacked, void *stream);

/* Gradient of at_phase_scan / at_phase_scan_strided (Phase, IF and the phase halves of Polar / PolarIF; reference
 * utils/misc.py:12-26, 65-81 and spectral_repr.py:318-335) with respect to the complex spectrum X (B, T, F).  `mode`: the
 * codes of at_phase_scan.  In autograd of the reference's statements unwrap has the identity as its derivative, so for
 *   y_t = (w_t s_t fdiff(unwrap(angle X))_t - offset) / scale   and g = dL/dy (float32 rows of ld_g >= F floats; ld_g = 2 F
 *   reads the phase half of a stacked (.., T, 2, F) gradient in place):
 *   a_t = g_t w_t s_t / scale     (w = 1 without frame_window, scale NULL: 1; the offset never matters)
 *   s_t = 1/pi on rows 0..T-2 (forward), -1/pi on rows 1..T-1 (backward), 1/(2 pi) on rows 1..T-2 (central), else 1
 *   angle, unwrap:  gu_t = a_t
 *   forward:        gu_t = c_t a_t - a_{t+1}/2 (while t+1 <= T-1),  c_0 = 1, else 1/2
 *   backward:       gu_t = c_t a_t - a_{t-1}/2 (while t >= 1),      c_{T-1} = 1, else 1/2
 *   central:        gu_t = [t = 0] a_0 + [t = T-1] a_{T-1} + a_{t-1}/4 [1 <= t-1 <= T-2] - a_{t+1}/4 [1 <= t+1 <= T-2]
 *                   (T = 1: the one row at_phase_scan writes, gu_0 = a_0)
 *   out_t = accum_t + gu_t (-Im X_t + i Re X_t) / |X_t|^2,   the second term 0 where X_t == 0 (torch's angle backward)
 * frame_window (T floats) and scale (device scalar) may be NULL; accum_complex (NULL, or X's shape) is added to the
 * result.  out_complex may be X_complex or accum_complex (every thread reads its element before it writes it); g must
 * not overlap out_complex.  A flat pass over the B T F elements: a bin's bits depend neither on the batch nor on the grid,
 * and a NaN of g stays within rows t-1..t+1 of its bin.  X, accum and out must be 8-byte aligned, g, frame_window and
 * scale 4-byte aligned.  AT_EINVAL (no device is touched) on null pointers, negative sizes, ld_g < F, a mode out of
 * range, a frame_window with angle / unwrap, or misalignment; AT_OK and nothing touched when a size is 0. */
int at_phase_scan_backward(const float *X_complex, int64_t B, int64_t T, int64_t F, int mode, const float *g, int64_t ld_g,
                           const float *frame_window, const float *scale, const float *accum_complex, float *out_complex,
                           void *stream);

/* Adjoint of at_cartesian_pack (Cartesian.forward, reference spectral_repr.py:403-428): g (rows, 2, F) float32, the
 * gradient of the stacked tensor -> gX (rows, F) complex64 = g[r, 0, :] / re_scale + i g[r, 1, :] / im_scale (a NULL scale:
 * 1, that half is not normalised).  out_complex must be 8-byte aligned, g_stacked and the scales 4-byte aligned (AT_EINVAL
 * otherwise, as on null arguments and negative sizes); AT_OK and nothing touched when a size is 0. */
int at_cartesian_pack_backward(const float *g_stacked, int64_t rows, int F, const float *re_scale, const float *im_scale,
                               float *out_complex, void *stream);

/* ---- backward passes of the streaming path (OverlapAdd, RealtimeSTFT, RealtimeDGT; stream_grad.hip) -----------------
 * N = n_fft, h = hop, F = N / 2 + 1, keep = (N / h - 1) h.  The carried state (history, tail, phase) is a constant of the
 * graph: a chunk's gradient covers that chunk's own samples.  Frames are grouped in streams of frames_per_stream
 * consecutive frames (nframes a multiple of it): at n_fft 128 / 256 / 512 the register FFTs transform 8 / 4 / 2 frames
 * together, and only frames of one stream may share a transform, as at_irfft_frames_streams arranges for the forward --
 * a stream's bits do not depend on the batch it rides in.  Any n_fft the forward takes. */

/* Adjoint of the frame analysis X[r, k] = sum_m w[m] f[r, m] e^{-2 pi i k m / N} (reference stft.py:251, dgt.py:287:
 * torch.fft.rfft(x * window)), given G (nframes, F) complex64:
 *   q[r, m] = (N/2) w[m] irfft(G[r])[m] + w[m] (Re G[r,0] / 2 + Re G[r,N/2] (-1)^m / 2)      (the Nyquist term: even N only)
 * gframes: (nframes, N) float32.  Three steps: the window scaled by N/2 into the workspace, the irFFT kernels of
 * at_irfft_frames_streams into gframes, the edge term in place with one fused multiply-add per sample (the per-frame half
 * of at_stft_backward; no overlap-add follows).  G_complex must be 8-byte aligned (AT_EINVAL); a gframes less aligned
 * than the register irFFT kernels ask for (8 bytes; 16 at n_fft 2048 / 4096) takes the one-frame kernels.  workspace:
 * at_rfft_frames_backward_workspace_bytes, 256-byte aligned. */
size_t at_rfft_frames_backward_workspace_bytes(int64_t nframes, int n_fft);
int at_rfft_frames_backward(const float *G_complex, int64_t nframes, int64_t frames_per_stream, int n_fft,
                            const float *window, float *gframes, void *workspace, size_t workspace_bytes, void *stream);

/* Adjoint of the frame synthesis f[r, m] = w[m] irfft(X[r])[m] (reference stft.py:266, dgt.py:302:
 * torch.fft.irfft(x) * inv_window), given gframes (nframes, N) float32:
 *   gX[r, k] = (c_k / N) rfft(w gframes[r])[k],   c_0 = 1, c_{N/2} = 1 (even N), c_k = 2 otherwise
 * phase NULL: out = gX, (nframes, F) complex64, 8-byte aligned.  phase (nframes, F) float32 given (polar input
 * X = mag e^{i phase}, the phase a constant): out = gmag = Re gX cos phase + Im gX sin phase, (nframes, F) float32; the
 * rFFT rows then stay in the workspace, a chunk of streams at a time.  Runs the kernels of at_stft_forward with
 * center = 0, one clip of frames_per_stream back-to-back frames per stream, on the window scaled by 2/N, then the finish
 * kernel of at_istft_backward.  gframes and phase may have any float alignment.  workspace:
 * at_irfft_frames_backward_workspace_bytes (polar: 1 with a phase, 0 without), 256-byte aligned. */
size_t at_irfft_frames_backward_workspace_bytes(int64_t nframes, int64_t frames_per_stream, int n_fft, int polar);
int at_irfft_frames_backward(const float *gframes, const float *phase_or_null, int64_t nframes, int64_t frames_per_stream,
                             int n_fft, const float *inv_window, float *out, void *workspace, size_t workspace_bytes,
                             void *stream);

/* Adjoint of OverlapAdd.forward (reference oadd.py:69-74: the frames are a view of [history | chunk | zero pad]) with
 * respect to the chunk, given gframes (S, n, N), a DENSE gradient of the n frames of each of S streams:
 *   gx[s, c] = sum_t gframes[s, t, keep + c - t h]   over the frames t in [0, n) with 0 <= keep + c - t h < N
 * gx: (S, C) float32.  Summed in ascending t by one thread per sample (no atomics); the history's share is dropped, and a
 * chunk sample that no frame covers gets exactly 0.  16 bytes per lane when h, N and C are multiples of 4 and both
 * pointers 16-byte aligned, the same bits otherwise. */
int at_oadd_forward_backward(const float *gframes, int64_t S, int64_t n, int n_fft, int hop, int keep, int64_t C,
                             float *gx, void *stream);

/* Adjoint of OverlapAdd.invert (reference oadd.py:90-104: out[s, p] = (tail[s, p] [p < keep] + sum_t f[s, t, p - t h]) /
 * gain for p < out_len = (n - 1) h + N - keep) with respect to the frames, given gy (S, out_len):
 *   gframes[s, t, o] = gy[s, t h + o] / gain   where t h + o < out_len, else 0
 * gframes: (S, n, N) float32; the part of a frame that only reaches the new tail gets exactly 0.  gain: the device scalar
 * at_oadd_invert reads.  16 bytes per lane when h and N are multiples of 4 and both pointers 16-byte aligned, the same
 * bits otherwise.
 * All four: AT_EINVAL on null or ill-shaped arguments before any launch, AT_OK and nothing touched on empty input, no
 * allocation, asynchronous on `stream`. */
int at_oadd_invert_backward(const float *gy, int64_t S, int64_t n, int n_fft, int hop, int keep, const float *gain,
                            float *gframes, void *stream);

/* ---- spectral distance (spectral_distance.hip; losses.SpectralDistance, autograd.SpectralDistanceFunction) ------------ */
/* Per-clip sums of the distance between two spectra X (generated) and Y (target), both (B, n) complex64 with n = T F
 * bins per clip, A = |X|, Bm = |Y|:
 *   sums[b] = { S_D = sum (A - Bm)^2,  S_B = sum Bm^2,  S_L = sum |ln(A + eps) - ln(Bm + eps)| }      (B, 3) float64
 * from which the caller forms loss_b = lin_weight S_D / S_B + log_weight S_L / n.  16 bytes read per bin, nothing of
 * size written.  A clip is cut into slices of 4096 bins; one workgroup reduces one slice (fp32 per lane in bin order, a
 * fixed tree over the lanes) into the workspace, a second kernel adds a clip's slices in order in double: the order of
 * a clip's sums is a function of n alone, never of B, of the clip's place in the batch, or of the grid; no atomics.
 * One 8-byte bin per lane (odd clips of an odd n are only 8-byte aligned).  workspace: 4-byte aligned,
 * at_spectral_distance_workspace_bytes(B, n) bytes (AT_EWORKSPACE otherwise).  AT_EINVAL on null X, Y or sums, B < 0,
 * n < 1 or eps < 0, before any launch; AT_OK without a launch when B == 0. */
size_t at_spectral_distance_workspace_bytes(int64_t B, int64_t n);
int at_spectral_distance_sums(const float *X_complex, const float *Y_complex, int64_t B, int64_t n, float eps,
                              double *sums, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the above, in place: given the sums the forward wrote and gclip (B,) float32, the gradient g of loss_b,
 * X becomes G_X (need_x) and Y becomes G_Y (need_y), with d = A - Bm:
 *   dA  = g (lin_weight 2 d / S_B + log_weight sgn(d) / (n (A + eps)))
 *   dBm = g (lin_weight (-2 d / S_B - 2 Bm S_D / S_B^2) - log_weight sgn(d) / (n (Bm + eps)))
 *   G_X = dA X / A (0 where A == 0),   G_Y = dBm Y / Bm (0 where Bm == 0)
 * in the convention at_stft_backward takes (dRe + i dIm).  sgn(d) is the sign of the log difference (ln is monotone):
 * no logarithm.  Pointwise, one bin per lane; a spectrum whose need_* is 0 is read and not written.  AT_EINVAL on null
 * X, Y, sums or gclip, B < 0, n < 1, eps < 0 or both need_* zero; AT_OK without a launch when B == 0. */
int at_spectral_distance_backward(float *X_complex, float *Y_complex, int64_t B, int64_t n, const double *sums,
                                  const float *gclip, float lin_weight, float log_weight, float eps, int need_x,
                                  int need_y, void *stream);

/* ---- mel-scale spectral distance (mel_distance.hip; losses.MelSpectralDistance, autograd.MelSpectralDistanceFunction) - */
/* Mel rows of a spectrum: out[r, j] = sum_k |X[r, k]| W[k, j] for X (rows, K) complex64 (8-byte aligned) and the (K x N)
 * bank W by column (as at_magnitude_backward's f_*: column j holds f_len[j] weights at f_w[f_off[j] ..] for the bins
 * f_start[j] ..), summed in ascending k.  out: (rows, N) float32.  One wave per row, |X| of the row in LDS, lane l
 * writes mel l, l + 64, ...; persistent workgroups, the tables staged in LDS once per workgroup when they fit next to
 * four rows (160 KB), read from global memory otherwise.  8 bytes read per bin, N / K of that written.  AT_OK without
 * a launch when rows == 0; AT_EINVAL on null pointers, rows < 0, K or N < 1, f_nnz < 1 or X off its 8-byte grid;
 * AT_EUNSUPPORTED when one row exceeds the LDS budget. */
int at_mel_rows(const float *X_complex, int64_t rows, int K, int N, const int *f_start, const int *f_len,
                const int *f_off, const float *f_w, int f_nnz, float *out, void *stream);

/* Per-clip sums of the distance between two arrays of mel rows M (generated) and Q (target), both (B, n) float32 with
 * n = T N cells per clip:
 *   sums[b] = { S_D = sum (M - Q)^2,  S_B = sum Q^2,  S_L = sum |ln(M + eps) - ln(Q + eps)| }           (B, 3) float64
 * from which the caller forms loss_b = lin_weight S_D / S_B + log_weight S_L / n.  The order is
 * at_spectral_distance_sums's: slices of 4096 cells, one workgroup per slice (fp32 per lane in cell order, a fixed tree
 * over the lanes), a second kernel adds a clip's slices in order in double; a function of n alone, no atomics.
 * workspace: 4-byte aligned, at_mel_distance_workspace_bytes(B, n) bytes (AT_EWORKSPACE otherwise).  AT_OK without a
 * launch when B == 0; AT_EINVAL on null M, Q or sums, B < 0, n < 1 or eps < 0, before any launch. */
size_t at_mel_distance_workspace_bytes(int64_t B, int64_t n);
int at_mel_distance_sums(const float *M, const float *Q, int64_t B, int64_t n, float eps, double *sums,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the above with respect to ONE spectrum, in place.  S (B, T, K) complex64 is the spectrum of one signal,
 * other (B T, N) float32 the mel rows of the other one: side 0: S = X, other = Q, S becomes G_X; side 1: S = Y,
 * other = M, S becomes G_Y.  With sums (B, 3) what at_mel_distance_sums wrote, gclip (B,) float32 the gradient g of
 * loss_b, n = T N and d = M - Q:
 *   dM = g (lin_weight 2 d / S_B + log_weight sgn(d) / (n (M + eps)))
 *   dQ = g (lin_weight (-2 d / S_B - 2 Q S_D / S_B^2) - log_weight sgn(d) / (n (Q + eps)))
 *   dA[k] = sum_j W[k, j] dM[j],   G_X = dA X / |X| (0 where X == 0);   G_Y likewise from dQ and Y
 * in the convention at_stft_backward takes (dRe + i dIm); sgn(0) = 0, no logarithm.  The row's own mel values are
 * recomputed by at_mel_rows's device code, to its bits.  f_*: the bank by column (N columns), t_*: its transpose by
 * column (K columns), as at_magnitude_backward.  16 bytes moved per bin plus 4 N / K.  Plans as at_mel_rows (both
 * banks' tables and K + N floats per row).  AT_OK without a launch when B == 0; AT_EINVAL on null pointers, B < 0,
 * T, K or N < 1, eps < 0, S off its 8-byte grid or side outside {0, 1}; AT_EUNSUPPORTED when one row exceeds the LDS
 * budget. */
int at_mel_distance_backward(float *S_complex, const float *other, int64_t B, int64_t T, int K, int N,
                             const int *f_start, const int *f_len, const int *f_off, const float *f_w, int f_nnz,
                             const int *t_start, const int *t_len, const int *t_off, const float *t_w, int t_nnz,
                             const double *sums, const float *gclip, float lin_weight, float log_weight, float eps,
                             int side, void *stream);

/* ---- PQMF: multiband analysis and synthesis (pqmf.hip; transforms.PQMF, autograd.PqmfFunction / PqmfInvertFunction) - */
/* The cosine-modulated pseudo-QMF bank of M = n_band bands on a real prototype h of N = taps (odd) taps, P = (N - 1) / 2:
 *   h_k[n] = 2 h[n] cos((2k+1) pi / (2M) (n - P) + (-1)^k pi / 4)
 *   analysis   y[row, k, t] = scale sum_n h_k[n] x[row, tM + n - P]                    x (rows, L) -> y (rows, M, L / M)
 *   synthesis  x[row, m]    = scale sum_k sum_t h_k[m + P - tM] y[row, k, t]           y (rows, M, L / M) -> x (rows, L)
 * with x zero outside [0, L) and y outside [0, L / M): synthesis is the transpose of analysis.  PQMF.forward is analysis
 * with scale 1 and PQMF.invert synthesis with scale M; their backward passes are synthesis with scale 1 and analysis
 * with scale M.  L is the AUDIO length in both calls.  mod: (M, 2M) float32, mod[k, r] = 2 cos((2k+1) pi / (2M) (r - P)
 * + (-1)^k pi / 4), computed by the caller (the device evaluates no cosine); the kernels fold the taps that share a
 * phase, u[r] = sum_j (-1)^j h[r + 2Mj] x[tM + r + 2Mj - P], and modulate, y_k = sum_r mod[k, r] u[r]: N / M + 2M
 * multiply-adds per sample.  Every sum is one fmaf chain in ascending index order, a function of (M, N) alone: a row's
 * bits do not depend on the other rows, and away from the edges a shift by M samples is a shift by one block to the bit.
 * One workgroup per tile of at_pqmf_tile_blocks(M, N) blocks t of one row; rows and tiles share one 64-bit index, so
 * there is no row limit.  No allocation, no workspace, asynchronous on `stream`.
 * AT_OK without a launch when rows == 0 or L == 0 (before any pointer check); AT_EINVAL on rows or L < 0, n_band < 1,
 * L % n_band != 0, even taps, taps < 2 n_band + 1 or a null pointer; AT_EUNSUPPORTED outside n_band 2 .. 64 or taps
 * <= 4097.  at_pqmf_tile_blocks answers the same two errors, a positive count otherwise. */
int at_pqmf_tile_blocks(int n_band, int taps);
int at_pqmf_analysis(const float *x, int64_t rows, int64_t L, const float *proto, int taps, int n_band,
                     const float *mod, float scale, float *y, void *stream);
int at_pqmf_synthesis(const float *y, int64_t rows, int64_t L, const float *proto, int taps, int n_band,
                      const float *mod, float scale, float *x, void *stream);
/* The same two kernels on a chunk of a stream (transforms.RealtimePQMF, autograd.PqmfStreamFunction /
 * PqmfStreamInvertFunction): only what a tile stages differs, every sum is the chain of the entries above.  With
 * D = ceil(P / M), output block t is the offline sum at block t + shift_blocks of the signal [state | chunk | zeros]:
 *   analysis   y[row, k, t] = scale sum_n h_k[n] x[row, (t + shift) M + n - P]      state_in, state_out (rows, D M + P)
 *   synthesis  x[row, m]    = scale sum_k sum_t h_k[m + shift M + P - tM] y[row, k, t]
 *                                                                      state_in, state_out (rows, M, D + floor(P / M))
 * where the entries before the chunk are state_in (the last samples of the row, the last blocks of every band; null:
 * zeros) and the entries after it are zero.  shift_blocks = -D with the state is the causal bank delayed by D blocks:
 * no output reads past the chunk, so the outputs of any chunking of a stream are, for finite input, the bits of one
 * call over the whole stream.  shift_blocks = +D with null state is the transpose of the OTHER kernel's delayed form,
 * i.e. the backward passes of the streaming forward (synthesis, scale 1) and invert (analysis, scale M) with the state
 * a constant.  state_out (null: not wanted) receives the last entries of [state_in | chunk], written on the device by
 * the workgroup of each row's last tile; it must not be state_in (the caller swaps the two buffers).  L is the AUDIO
 * length of the chunk in both calls.  Everything else as above; additionally AT_EINVAL when |shift_blocks| > D or
 * state_out == state_in.  Nothing is written, state_out included, when rows == 0 or L == 0. */
int at_pqmf_analysis_stream(const float *x, int64_t rows, int64_t L, const float *state_in, float *state_out,
                            int shift_blocks, const float *proto, int taps, int n_band, const float *mod,
                            float scale, float *y, void *stream);
int at_pqmf_synthesis_stream(const float *y, int64_t rows, int64_t L, const float *state_in, float *state_out,
                             int shift_blocks, const float *proto, int taps, int n_band, const float *mod,
                             float scale, float *x, void *stream);

/* ---- audio front end ------------------------------------------------------------------------------------- */
/* torchaudio.transforms.Resample(orig, new) with default arguments, as utils/misc.py:31-33 uses it (algorithm
 * restated, torchaudio is not in the reference tree).  x: (rows, L); orig/new: the rates divided by their gcd;
 * filters: new x (2*width + orig) float32 polyphase bank; out: (rows, out_len), out_len = ceil(new * L / orig). */
int at_resample_sinc(const float *x, int64_t rows, int64_t L, int orig, int new_, int width, const float *filters,
                     int64_t out_len, float *out, void *stream);

/* The adjoint of at_resample_sinc with respect to x (autograd.ResampleFunction): g (rows, out_len) -> gx (rows, L),
 *   gx[n] = sum over (i, j) with o = i new + j < out_len and 0 <= k = n - i orig + lead < taps of filters[j][k] g[o],
 * lead = width and taps = 2 width + orig for the offline converter; at_resample_sinc_stream's gradient with respect to
 * its chunk is the same sum with lead = Ha over the chunk's own output blocks (L = C, out_len = C / orig * new), which is
 * why lead and taps are separate arguments.  Each gx[n] is one fmaf chain from +0 over o ascending: no atomics, and the
 * bits of a row depend on neither its batch nor the tiling.  One workgroup per tile of *tile_blocks whole input blocks
 * of one row, the window of g it reads in LDS, the bank in LDS too when it fits beside it (*bank_in_lds), read through
 * L1 / L2 otherwise: at_resample_backward_plan answers both for a shape; it is a pure function of its arguments.
 * AT_EINVAL: null pointers, negative sizes, out_len != ceil(new L / orig) when lead == width (taps == 2 lead + orig).
 * AT_OK without a launch when rows == 0 or L == 0.  AT_EUNSUPPORTED: rows > 65535 (at_resample_sinc's limit), or a bank
 * so wide that the window of a one-block tile exceeds the LDS. */
int at_resample_backward_plan(int orig, int new_, int taps, int lead, int *tile_blocks, int *bank_in_lds);
int at_resample_sinc_backward(const float *g, int64_t rows, int64_t L, int orig, int new_, int taps, int lead,
                              const float *filters, int64_t out_len, float *gx, void *stream);

/* The causal converter (utils.RealtimeResample): the next chunk x (rows, C), C a multiple of orig, of a stream whose
 * last Ha = D orig + width samples are state_in (rows, Ha) (null: zeros), D = ceil(width / orig) -> out (rows, C / orig *
 * new), out[t new + j] = sum_k filters[j][k] v[t orig + k] over v = [state_in | x]: at_resample_sinc's chain, delayed
 * by D blocks, so for finite input the bits of at_resample_sinc on the stream with D orig zeros in front.  state_out
 * (null: not wanted; never state_in) receives the last Ha samples of v from the same launch.  AT_EINVAL: negative sizes,
 * C % orig != 0, state_out == state_in, null x / filters / out; AT_OK without a launch (state_out untouched) when rows
 * == 0 or C == 0; AT_EUNSUPPORTED: rows > 65535. */
int at_resample_sinc_stream(const float *x, int64_t rows, int64_t C, const float *state_in, float *state_out, int orig,
                            int new_, int width, const float *filters, float *out, void *stream);

/* Sample-rate conversion without the bank (ops.resample_direct, PitchShift).  An entry of the polyphase bank depends only
 * on q = n new - o orig through one even function that is exactly 0 in float32 beyond |q| = Qi; table is its half,
 * table[0 .. Qi] (ops.sinc_table).  in: (rows, in_len) -> out: (rows, out_len),
 *   out[r][o] = sum over n ascending, max(0, ceil((o a - Qi) / b)) <= n <= min(in_len - 1, floor((o a + Qi) / b)),
 *               of table[|n b - o a|] in[r][n]
 * The converter is (in = x, a = orig, b = new, out_len = ceil(new L / orig)); its adjoint is the same routine with
 * (in = g, in_len = out_len, a = new, b = orig, out_len = L).  Each output is one fmaf chain from +0: a function of (a,
 * b, Qi, o, in_len) alone, so the bits of a row depend on neither its batch, the tile, the grid nor the place of the
 * table, and for finite input they are the bits of the bank routes above, which add only zero terms to the same chain.
 * One workgroup per tile of *tile_outputs consecutive outputs of one row, the input window they reach in LDS, the table in
 * LDS too when it fits beside it (*table_in_lds), read from global memory otherwise: the plan routine answers both for
 * a shape and is a pure function of its arguments.  Rows and tiles share one 64-bit index: no limit on the rows.
 * AT_EINVAL: null pointers, negative sizes, a or b < 1, Qi < 0.  AT_OK without a launch when rows == 0 or out_len == 0.
 * AT_EUNSUPPORTED: rates so far apart that one output's window exceeds the LDS, or sizes beyond 64-bit indexing. */
int at_sinc_interp_plan(int a, int b, int Qi, int *tile_outputs, int *table_in_lds);
int at_sinc_interp(const float *in, int64_t rows, int64_t in_len, int a, int b, const float *table, int Qi,
                   int64_t out_len, float *out, void *stream);

/* ---- time stretching ------------------------------------------------------------------------------------- */
/* The phase vocoder of torchaudio.functional.phase_vocoder / torchaudio.transforms.TimeStretch (algorithm restated,
 * torchaudio is not in the reference tree) on a time-major spectrum: X (B, T, F) complex64 -> out (B, N, F) complex64.
 * The step table is the caller's (ops.phase_vocoder_steps makes it on the host in float64): idx (N int32, device), alpha
 * (N float32, device), idx_j = floor(j rate), alpha_j = j rate - idx_j for every j with j rate < T; idx_0 = 0, idx never
 * decreases, idx_j + 1 may be T, and frame T is a frame of zeros.  The textbook phase increment wrap(a1 - a0 - adv) + adv
 * is congruent to a1 - a0 and only meets exp(i .), so the expected advance -- and hop_length -- cancels and the
 * accumulated phase is a running product of unit phasors:
 *   u(z) = z / |z| (1 where z == 0),  p_0 = u(X[0]),  p_{j+1} = p_j u(X[idx_j + 1]) conj(u(X[idx_j])),
 *   out[j] = (alpha_j |X[idx_j + 1]| + (1 - alpha_j) |X[idx_j]|) p_j.
 * One thread per (clip, bin) column walks j upwards; a column's bits depend neither on the batch nor on the layout (flat
 * columns, or one block per clip where rows are no whole 64-byte segments: AT_VARIANT_SCAN_LAYOUT = 1 forces the flat
 * one), and a NaN stays in its column.  Zero bins give magnitude 0 and u = 1; -0 + 0i counts as zero, where torch.angle
 * answers pi (the one divergence).  final_phasor (B, F) complex64 or NULL receives p_N, which the backward starts from.
 * An idx outside [0, T - 1] is read as the nearest frame inside: no table makes the kernel read out of bounds.
 * AT_EINVAL (no device is touched): negative sizes, N == 0 with T > 0 or the reverse, null X / idx / alpha / out, out ==
 * X, misalignment (8 bytes for the complex tensors, 4 for the table).  AT_OK and nothing touched when B T F == 0.
 * AT_EUNSUPPORTED: T or N beyond the int range of the row indices (N > INT_MAX - 8), or more columns than a grid holds. */
int at_phase_vocoder(const float *X_complex, int64_t B, int64_t T, int64_t F, const int *idx, const float *alpha, int64_t N,
                     float *out_complex, float *final_phasor, void *stream);

/* Gradient of at_phase_vocoder with respect to X: g (B, N, F) complex64 = dL/dout -> gX (B, T, F) complex64.  With
 * Z_j = out[j] = m_j p_j:  gphi_j = Im(conj(Z_j) g_j),  gm_j = Re(conj(p_j) g_j),  S_j = sum over j' >= j of gphi_j',
 *   G_abs[idx_j] += (1 - alpha_j) gm_j,  G_abs[idx_j + 1] += alpha_j gm_j,
 *   G_ang[0] += S_0,  and for j + 1 < N:  G_ang[idx_j + 1] += S_{j+1},  G_ang[idx_j] -= S_{j+1},
 *   gX[i] = G_abs[i] X[i] / |X[i]| + G_ang[i] (-Im X[i] + i Re X[i]) / |X[i]|^2,  0 where X[i] == 0;
 * the share of the frame of zeros T is dropped, frames no step reads get zeros.  One thread per column walks j downwards:
 * p_j comes back from final_phasor (B, F), what the forward wrote, by the conjugate step; a frame's gradient is written
 * when idx moves past it -- a gather, no atomics, no (B, N, F) intermediate, every element of gX written once.  First
 * order only.  Flat columns: a column's bits do not depend on the batch.  Return codes as at_phase_vocoder, with
 * final_phasor required and gX distinct from X and g. */
int at_phase_vocoder_backward(const float *X_complex, const float *g_complex, const int *idx, const float *alpha,
                              const float *final_phasor, int64_t B, int64_t T, int64_t F, int64_t N, float *gX_complex,
                              void *stream);

/* ---- recursive filters ----------------------------------------------------------------------------------- */
/* A cascade of second-order sections (scipy.signal.sosfilt's recurrence and state layout, restated; no reference
 * counterpart) along each row of x (rows, L) float32 -> y (rows, L) float32.  sos_host: n_sections x 6 doubles ON THE HOST,
 * b0 b1 b2 a0 a1 a2 per section with a0 == 1; they travel to the kernel by value.  Section k filters the output v of
 * section k - 1 by
 *   y = b0 v + z1,   z1' = b1 v - a1 y + z2,   z2' = b2 v - a2 y,
 * all in double; the signal between sections is not rounded, the last section's output is rounded to float once.  zi
 * (rows, n_sections, 2) doubles on the device, or NULL for zeros, is the state (z1, z2) before sample 0; zf (same shape, or
 * NULL; never zi) receives the state after sample L - 1, from the same launch.  reverse = 1 runs n from L - 1 down to 0
 * with zero state (the adjoint of the forward filter): bit for bit flip -> forward -> flip; it takes neither zi nor zf.
 * One workgroup of 256 lanes walks a row in tiles of *tile = 256 x *per_lane samples: a lane runs its samples from a zero
 * state, the lanes' end states are scanned (exclusive: a NaN at sample n leaves y[: n] bit-identical, and other rows
 * untouched), and y[i] += (A^i s_in)[0] with A = [[-a1, 1], [-a2, 0]].  y[r][n] is a function of (sos, L, n, reverse) and
 * row r's samples alone: there is one dispatch (*dispatch = 0), a constant tile, and no dependence on the batch or the
 * grid; the plan routine says so without a device.  Rows past the grid go to persistent workgroups: no limit on the rows.
 * All-zero input with zero state gives +0.  Stability is the caller's: an unstable section overflows as its recurrence
 * does (and a section whose A^1024 overflows a double gives NaN from the first tile).
 * AT_EINVAL (no device is touched): negative sizes, n_sections < 1, null sos_host or plan outputs, null x / y with rows L >
 * 0, a non-finite coefficient, a0 != 1, reverse outside {0, 1} or with zi / zf, zf == zi, misalignment (4 bytes audio, 8
 * state).  AT_EUNSUPPORTED: more than 16 sections.  AT_OK without a kernel when rows == 0 or L == 0 (with L == 0 and rows >
 * 0, zf receives zi, or zeros). */
int at_sos_filter_plan(int64_t rows, int64_t L, int n_sections, int64_t *tile, int64_t *per_lane, int *dispatch);
int at_sos_filter(const float *x, int64_t rows, int64_t L, const double *sos_host, int n_sections, int reverse,
                  const double *zi, double *zf, float *y, void *stream);

/* The same walk with two other endings (sos_filter.hip), forwards in time from zero state, for rows cut into hops of `hop`
 * samples: nh = L / hop whole hops, the samples past nh hop belong to none.
 * at_sos_hop_power: power (rows, nh) float64, power[r][h] = the sum over hop h of y[n]^2, with y the last section's DOUBLE
 * output, squared before any rounding; nothing of y is written.  The energy envelope of any SOS-filtered signal (one
 * section 1 0 0 1 0 0: of the signal itself).  hop >= 16 = *per_lane, so that a lane's samples touch at most two hops; a
 * hop that straddles lanes, waves or tiles is combined in one fixed order (a chain per lane, a segmented scan per wave, a
 * chain over the waves that lane 0 carries from tile to tile): power[r][h] is a function of (sos, L, hop, h) and row r's
 * samples alone -- no atomics, no workgroup waits for another, the batch and the grid do not enter.  Zeros give +0; a NaN at
 * sample n leaves the hops before n / hop bit-identical and other rows untouched.  The plan routine answers as
 * at_sos_filter_plan does, without a device.
 * at_sos_filter_hop_scaled: u (rows, L) float32, u[r][n] = (float)(w[r][n / hop] y[n]) for n < nh hop and +0 after, w (rows,
 * nh) float64: the gradient of a function of the hop powers with respect to y, ready for at_sos_filter(reverse = 1).
 * AT_EINVAL: as at_sos_filter, and hop < 1, a null power, w (with nh > 0) or u, misalignment (4 bytes audio, 8 power and
 * w).  AT_EUNSUPPORTED: more than 16 sections, hop < 16, hop >= 2^31 with nh > 0.  AT_OK without a kernel for rows == 0 and
 * for nh == 0 (at_sos_filter_hop_scaled then clears u). */
int at_sos_hop_power_plan(int64_t rows, int64_t L, int n_sections, int64_t hop, int64_t *tile, int64_t *per_lane,
                          int *dispatch);
int at_sos_hop_power(const float *x, int64_t rows, int64_t L, const double *sos_host, int n_sections, int64_t hop,
                     double *power, void *stream);
int at_sos_filter_hop_scaled(const float *x, int64_t rows, int64_t L, const double *sos_host, int n_sections, int64_t hop,
                             const double *w, float *u, void *stream);

/* at_sos_hop_power_stream: the hop-power ending over a STREAM.  x (rows, n) float32, n >= 1, is the next chunk of a stream
 * whose open hop already holds `filled` samples (0 <= filled < hop) with the partial sum open_in (rows) float64 (NULL:
 * zeros), and whose filter state is zi (rows, n_sections, 2) float64 (NULL: zeros).  done = (filled + n) / hop hops complete
 * inside the call: hop k of the chunk goes to power[r * ld + first + k], k < done -- k = 0 is open_in plus the first hop -
 * filled samples of the chunk -- and nothing else of power is touched; open_out[r] receives the sum over the trailing
 * (filled + n) % hop samples (+0 when there are none; open_in plus the whole chunk when done == 0) and zf the state after
 * the chunk, both from the same launch.  zf may be zi and open_out may be open_in: a row's state is read at the row's start
 * by the one workgroup that writes it at the row's end.  The tile grid is anchored at the chunk's first sample, so the hop
 * powers of a chunked stream agree with the one-call at_sos_hop_power WITHIN ROUNDING, not to the bit; power[r][first + k],
 * open_out[r] and zf[r] are functions of (sos, hop, filled, n), row r's samples and row r's incoming state alone -- no
 * atomics, no workgroup waits for another, sums are selected and never masked by a multiply -- so the same chunking gives
 * the same bits in any batch.  AT_EINVAL: null x / sos_host / zf / open_out / power, negative sizes, n < 1, filled outside
 * [0, hop), ld < first + done, a non-finite coefficient, a0 != 1, misalignment.  AT_EUNSUPPORTED: more than 16 sections,
 * hop < 16, hop >= 2^31.  AT_OK without a kernel for rows == 0. */
int at_sos_hop_power_stream(const float *x, int64_t rows, int64_t n, const double *sos_host, int n_sections, int64_t hop,
                            int64_t filled, const double *zi, double *zf, const double *open_in, double *open_out,
                            double *power, int64_t ld, int64_t first, void *stream);

/* ---- gated loudness (loudness.hip; ops.loudness, ops.loudness_blocks, transforms.Loudness) ------------------------- */
/* ITU-R BS.1770 / EBU R128 gating of hop powers (restated; no reference counterpart).  power (clips, C, nh) float64 is
 * at_sos_hop_power of the K-weighted channels, a hop has `hop` samples (100 ms), a block hb hops (4: momentary and the
 * integrated measure; 30: short-term), nb = nh - hb + 1, weights_host C doubles ON THE HOST (by value to the kernel):
 *   p_j = (sum over c ascending of G_c (power[c][j] + ... + power[c][j + hb - 1], ascending)) / (hb hop),
 *   block_lufs[j] = (float)(-0.691 + 10 log10 p_j)   (clips, nb), ungated, -inf where p_j == 0; NULL: not wanted,
 *   J1 = {j: p_j > abs_threshold}, Pabs = mean over J1, J2 = {j in J1: p_j > rel_ratio Pabs}, P = mean over J2, N2 = |J2|,
 *   lufs = (float)(-0.691 + 10 log10 P)   (clips), -inf when J1 is empty;  stats (clips, 3) float64 = Pabs, P, N2.
 * lufs == NULL skips the gates and writes block_lufs alone.  The gates compare powers in double with the thresholds given
 * (no logarithm decides one), as !(p <= threshold): a NaN block passes, so a clip with a NaN reads NaN.  One workgroup per
 * clip, persistent past the grid; a mean is 256 lane-strided chains in block order joined by a fixed halving tree, a function
 * of nb alone: a clip's bits do not depend on the batch.
 * at_loudness_gate_backward: g (clips) float32 = dL/dlufs -> w (clips, C, nh) float64 with dL/dy_c[n] = w[c][n / hop] y_c[n]:
 *   w[c][h] = g (10 / ln 10) / (P N2) G_c (2 / (hb hop)) m[h],   m[h] = the blocks of J2 that cover hop h,
 * the masks recomputed from power and stats; +0 is SELECTED where N2 == 0 or m[h] == 0 (a silent clip's gradient is exactly
 * zero whatever g is).  at_loudness_blocks_backward: g_blocks (clips, nb) float32 = dL/dblock_lufs ->
 *   w[c][h] = G_c (2 / (hb hop)) (sum over the blocks j that cover h, ascending, of g_j (10 / ln 10) / p_j),
 * blocks with p_j == 0 contributing nothing.  The gates are piecewise constant: constants of the graph.  First order only.
 * AT_EINVAL: negative sizes, C < 1, hop < 1, hb < 1, null weights_host, a non-finite weight, a negative or non-finite
 * threshold, null pointers for what is to be read or written (lufs and block_lufs both NULL; lufs without stats),
 * misalignment.  AT_EUNSUPPORTED: C > 32, hb > 4096.  AT_OK without a kernel when clips == 0 (backwards: or nh == 0); with
 * nh < hb there is no block: lufs is -inf, stats zeros, w zeros. */
int at_loudness_gate(const double *power, int64_t clips, int C, int64_t nh, int64_t hop, int hb, const double *weights_host,
                     double abs_threshold, double rel_ratio, float *lufs, double *stats, float *block_lufs, void *stream);
/* at_loudness_gate_ld: at_loudness_gate on a window of a longer history -- channel c of a clip begins at power + (clip C + c)
 * ld, ld >= nh hops apart (AT_EINVAL below) -- read where it lies; at_loudness_gate is this call with ld = nh, the same
 * addresses and the same bits.
 * at_loudness_range: loudness range of EBU Tech 3342 from the same hop powers (the host passes hb = 30, rel_ratio = 0.01,
 * -20 LU).  With p_j, J1, Pabs and J2 as above, n = |J2|, q the ascending order of {p_j: j in J2} and rnd(v) = floor(v + 0.5),
 *   lra = (float)(10 log10(q[rnd(0.95 (n - 1))] / q[rnd(0.10 (n - 1))]))   (clips);  stats (clips, 4) = P_low, P_high, n, Pabs.
 * n == 0: lra = 0 and P_low = P_high = 0.  A clip with a NaN block reads NaN (lra, P_low, P_high) and touches no other.  The
 * two order statistics are an exact radix select on the order-preserving unsigned image of the doubles' bits (eight passes of
 * eight bits, integer histograms in LDS): no sort, no float atomics, a function of the clip's hop powers alone.  workspace
 * (clips, nb) float64 receives the block powers.  AT_EINVAL as at_loudness_gate, and null lra / stats / workspace;
 * AT_EUNSUPPORTED also for nb >= 2^31. */
int at_loudness_gate_ld(const double *power, int64_t clips, int C, int64_t nh, int64_t ld, int64_t hop, int hb,
                        const double *weights_host, double abs_threshold, double rel_ratio, float *lufs, double *stats,
                        float *block_lufs, void *stream);
int at_loudness_range(const double *power, int64_t clips, int C, int64_t nh, int64_t ld, int64_t hop, int hb,
                      const double *weights_host, double abs_threshold, double rel_ratio, float *lra, double *stats,
                      double *workspace, void *stream);
int at_loudness_gate_backward(const double *power, const double *stats, const float *g, int64_t clips, int C, int64_t nh,
                              int64_t hop, int hb, const double *weights_host, double abs_threshold, double rel_ratio,
                              double *w, void *stream);
int at_loudness_blocks_backward(const double *power, const float *g_blocks, int64_t clips, int C, int64_t nh, int64_t hop,
                                int hb, const double *weights_host, double *w, void *stream);

/* ---- long-filter convolution (fft_convolve.hip; ops.fft_convolve, autograd.FFTConvolveFunction) -------------------- */
/* Uniformly partitioned overlap-save convolution of a row of L samples with K taps (torchaudio.functional.fftconvolve,
 * restated; no reference counterpart): block B, n_fft N = 2 B, F = B + 1, M = L + K - 1, T = ceil(M / B) frames,
 * P = ceil(K / B) partitions.  X[t] = rfft(x[tB - B, tB + B)), H[p] = rfft(h[pB, pB + B) then B zeros), Y[t] = sum_{p <=
 * min(t, P - 1)} H[p] X[t - p]; block t of the result is the last B samples of irfft(Y[t]).  The transforms are
 * at_stft_forward (center = 0, hop = B, a window of ones), at_irfft_frames_streams and, for the backward,
 * at_rfft_frames_backward / at_irfft_frames_backward; the two calls below are the part in between.
 *
 * at_fft_convolve_plan answers, on the host and without a device: *B (block = 0: the smallest of 512, 1024, 2048
 * with ceil(K / B) <= 4, else 2048; block = 128, 256 or a member of that ladder: that block), *T, *P, *frame_tile (the output frames a
 * lane of at_spectral_fir keeps in registers) and *chunk_rows (the most rows whose one spectrum T F stays within 2^26
 * complex64 elements, at least 1).  AT_EINVAL: L < 1, K < 1, a block outside the ladder, a null output. */
int at_fft_convolve_plan(int64_t L, int64_t K, int block, int64_t *B, int64_t *T, int64_t *P, int *frame_tile,
                         int64_t *chunk_rows);

/* Y[r][t][f] = sum_{p < P} Hc[p][f] X[r][s][f],  s = t - p (anticausal = 0) or t + p (anticausal = 1), terms with s outside
 * [0, T) skipped; Hc = H[r] (conj = 0) or its conjugate (conj = 1).  X: rows of T x F complex64, row r at x_row_stride
 * complex elements (>= T F: the frames of a row may be followed by others); H: (rows or 1, P, F) complex64, h_row_stride = P F
 * for one filter per row, 0 for one filter shared by all rows; Y: (rows, T, F) complex64, dense.  (0, 0) is the forward,
 * (1, 1) the backward with respect to X.  One lane per bin, *frame_tile consecutive frames per lane, the window of X in
 * registers: one load of X and one of H per (p, tile).  Rows x tiles x bin chunks on one 64-bit index, persistent
 * workgroups past 8192: no limit on the rows.  Every output element is one chain from +0 over p ascending, four fmaf per
 * complex multiply-add: a function of (T, P, t, direction) alone -- never of the batch, the tile or the grid; zeros give +0;
 * a NaN in X[r][s][f] stays in column (r, f).  P == 0 gives zeros.
 * AT_EINVAL: negative sizes or strides, F < 1, a flag outside {0, 1}, null X / Y (H with P > 0) where there is work, a
 * stride shorter than a row, a pointer that is not 8-byte aligned.  AT_OK without a launch when rows == 0 or T == 0. */
int at_spectral_fir(const float *X_complex, int64_t x_row_stride, const float *H_complex, int64_t h_row_stride, int64_t rows,
                    int64_t T, int64_t P, int F, int anticausal, int conj, float *Y_complex, void *stream);

/* gH[rh][p][f] = sum_r sum_{t = p .. T - 1} conj(X[r][t - p][f]) gY[r][t][f]: the backward of the causal FIR with respect
 * to H.  shared = 0: rh = r, gH (rows, P, F), no sum over rows; shared = 1: gH (1, P, F), rows added in ascending order.  X
 * as above, gY (rows, T, F) dense.  A row's frames are cut into slices of 64: within a slice fp32 fmaf chains from +0, t
 * ascending; slices (and, shared, rows) are added in double in ascending order, in groups of consecutive (row, slice)
 * units that leave one complex double per (p, f) in the workspace, and a second kernel adds the groups in order and rounds
 * once.  The grouping is a function of (rows, T, P, F) alone and there are no atomics: the same call gives the same bits;
 * with shared = 0 a row is its own group and its gradient does not depend on the batch.  workspace: 16-byte aligned,
 * at_spectral_fir_corr_workspace_bytes (AT_EWORKSPACE otherwise): at most 256 groups of P F complex doubles for a shared
 * filter, one per row otherwise.  AT_EINVAL as above; AT_OK without a launch when rows == 0 or P == 0; T == 0 gives zeros
 * (a memset, no workspace: at_spectral_fir_corr_workspace_bytes is 0 then). */
size_t at_spectral_fir_corr_workspace_bytes(int64_t rows, int64_t T, int64_t P, int F, int shared);
int at_spectral_fir_corr(const float *X_complex, int64_t x_row_stride, const float *gY_complex, int64_t rows, int64_t T,
                         int64_t P, int F, int shared, float *gH_complex, void *workspace, size_t workspace_bytes,
                         void *stream);

/* The causal FIR over a STREAM: per row a ring of R >= P - 1 + Tc spectrum frames, (rows, R, F) complex64, and `head`, the
 * slot of the next frame to arrive, kept by the caller on the host.  One launch takes a chunk of Tc <= *max_frames (8) new
 * frames X (rows of Tc x F at x_row_stride complex elements) and ONE filter H (P, F) for every row:
 *   Y[r][t][f] = sum_{p < P, ascending} H[p][f] V[r][t - p][f],   V[r][s] = X[r][s] (s >= 0) or ring[r][(head + s) mod R] (s < 0),
 * and then ring[r][(head + t) mod R] = X[r][t], t < Tc: the slots written are never among the P - 1 slots read, so the ring
 * is updated in place by the same launch; the caller then advances head by Tc modulo R.  A ring of zeros is a stream
 * that has not begun.  One lane per (row, bin) holds all Tc output frames; no term is skipped, every output is one chain
 * from +0 of four fmaf per term, a function of (P, t) alone -- never of head, R, the grid or the batch -- and for finite
 * input it has the bits of at_spectral_fir (causal) on the linearised history [ring in order | X].  Rows x bin chunks on one
 * 64-bit index, persistent workgroups past 8192.  at_fft_convolve_stream_plan answers on the host, without a device: *B as
 * at_fft_convolve_plan (block = 0: the shipped rule), *P = ceil(K / B), *R = P - 1 + 8, *max_frames = 8.
 * AT_EINVAL: a null pointer, negative sizes, Tc > 8, P < 1, F < 1, R < P - 1 + Tc, head outside [0, R), a stride shorter
 * than Tc F, a pointer that is not 8-byte aligned; for the plan K < 1, a block outside the ladder, a null output.  AT_OK
 * without a launch, the ring untouched, when rows == 0 or Tc == 0. */
int at_fft_convolve_stream_plan(int64_t K, int block, int64_t *B, int64_t *P, int64_t *R, int64_t *max_frames);
int at_spectral_fir_stream(const float *X_complex, int64_t x_row_stride, float *ring_complex, const float *H_complex,
                           int64_t rows, int64_t Tc, int64_t P, int64_t R, int64_t head, int F, float *Y_complex,
                           void *stream);

/* ---- true peak (true_peak.hip; ops.true_peak, transforms.TruePeak, RealtimeTruePeak) -------------------------------- */
/* The true-peak measure of ITU-R BS.1770-4 Annex 2 for any polyphase table (restated; no reference counterpart).  x (rows,
 * L) float32; taps (P, K) float32 ON THE DEVICE, P phases of K taps, 1 <= P <= 8, 1 <= K <= 64:
 *   y[P n + p] = sum over k = 0 .. K - 1 ascending of taps[p][k] x[n - k],   0 <= n < L,   x[n < 0] from state_in or 0,
 *   peak = max over m of |y[m]|,   index = index_offset + the smallest m that attains it,   sign = sign(y[m]) there.
 * Every y[m] is one fmaf chain from +0 over k ascending; the reduction is the maximum of the unsigned image of |y|'s bits
 * (every NaN one image above infinity's: a NaN in a row makes that row's peak NaN at the first NaN output, and no other row's)
 * paired with the smallest index -- exact, associative and commutative, so a row's bits depend neither on the batch, nor on
 * the tile, nor on the grid, nor on how a stream was cut into chunks.  No float maximum, no atomics.  Zeros give +0, index
 * index_offset and sign 0; sign is also 0 where the peak is NaN.  P = K = 1 with tap 1 is the sample peak.
 * Rows x tiles of *tile = 2048 samples share one 64-bit index on persistent workgroups: no limit on the rows, and one long
 * row spreads over the chip; a lane takes *per_lane = 8 consecutive samples with their K - 1 halo in registers.  *dispatch: 0
 * the compiled (4, 12) copy with its taps as uniform values, 1 the generic copy with the table in LDS.  *launches: 0 for
 * empty work, 1 where a row is one tile, else 2 (a 16-byte partial per tile, then a small kernel that joins them in tile
 * order) and a workspace of the size the _workspace_bytes entry answers (0 for one tile; 16-byte aligned; AT_EWORKSPACE).
 * Outputs, each (rows) and each optional except that peak or max_peak_io must be given: peak float32, linear; index int64;
 * sign float32; max_peak_io float32, read as the running maximum of a stream and replaced, with max_index_io int64, where
 * this call's peak has the larger image (a tie keeps the earlier index).
 * Stream form: state_in (rows, K - 1) float32 holds the samples before x, oldest first (NULL: zeros); state_out (rows, K - 1),
 * never state_in, receives the last K - 1 samples of [state | x] from the same launch; any L >= 1, shorter than K - 1 too.
 * The plan and workspace entries read no device.  AT_EINVAL: negative sizes, P or K out of range, null x / taps / plan
 * outputs, neither peak nor max_peak_io, max_index_io without max_peak_io, a state with K == 1, state_out == state_in,
 * misalignment (4 bytes, 8 for the indices).  AT_OK without a launch when rows == 0 or L == 0: nothing is written.
 *
 * The backward entry below: the measure is piecewise linear, so the subgradient at the attained maximum is used,
 *   gx[n] = g sign taps[p*][n* - n]   for 0 <= n* - n < K, with index = P n* + p*;   +0 elsewhere,
 * g, sign (rows) float32 and index (rows) int64 as the forward wrote them with index_offset 0, gx (rows, L) float32.  One
 * launch writes every element: no memset, no atomics.  A row whose sign is 0 gets +0 by selection, whatever g holds. */
int at_true_peak_plan(int64_t rows, int64_t L, int P, int K, int64_t *tile, int64_t *per_lane, int *launches, int *dispatch);
size_t at_true_peak_workspace_bytes(int64_t rows, int64_t L, int P, int K);
int at_true_peak(const float *x, int64_t rows, int64_t L, const float *taps, int P, int K, const float *state_in,
                 float *state_out, float *peak, int64_t *index, float *sign, float *max_peak_io, int64_t *max_index_io,
                 int64_t index_offset, void *workspace, size_t workspace_bytes, void *stream);
int at_true_peak_backward(const float *g, const float *sign, const int64_t *index, const float *taps, int P, int K,
                          int64_t rows, int64_t L, float *gx, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ACIDS_HIP_H */

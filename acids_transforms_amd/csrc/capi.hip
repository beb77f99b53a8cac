// capi.hip -- extern "C" boundary of libacids_hip.so (see include/acids_hip.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <vector>

#include "../../include/acids_hip.h"
#include "autograd.h"
#include "band_bank.h"
#include "fft512.h"
#include "stft_launch.h"

#include <atomic>
#include "variants.h"
namespace at_hip {
constexpr int kMaxDevices = 16;
static float2* g_twiddles[kMaxDevices] = {nullptr};
static float2* g_side[kMaxDevices] = {nullptr};       // the side table (stft_launch.h: kSide*)

// both twiddle tables of the current device: the fft512 table and the side table, or false before at_init
static bool device_tables(const float2*& tw, const float2*& side) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices || !g_twiddles[dev]) return false;
  tw = g_twiddles[dev];
  side = g_side[dev];
  return true;
}

static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
// every n_fft in [2, 16384] (odd sizes, transformed at full length, up to 8191: two LDS copies of the frame)
static bool fft_size_ok(int n) { return n >= 2 && n <= 16384 && (!(n & 1) || n < 8192); }
// sizes the mixed-radix kernels of stft_mixed.hip take (everything that is not a power of two >= 8)
static bool fft_mixed(int n) { return !is_pow2(n) || n < 8; }

__global__ void envelope_table_kernel(const float* w, int n_fft, int hop, int R, float* env) {
  // env[mask][r] = sum over q in mask (ascending) of w[hop*(R-1-q) + r]^2: the R = n_fft / hop frames that overlap a
  // hop, oldest first
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1 << R) * hop) return;
  int mask = i / hop, r = i - mask * hop;
  float s = 0.f;
  for (int q = 0; q < R; ++q)
    if (mask & (1 << q)) {
      int o = hop * (R - 1 - q) + r;
      if (o < n_fft) s += w[o] * w[o];
    }
  env[i] = s;
}
static std::atomic<int> g_variants[kVarCount];
int variant(int which) { return g_variants[which].load(std::memory_order_relaxed); }
}  // namespace at_hip

using namespace at_hip;

extern "C" {

// 2: at_sinebank_realtime takes the synthesis window; bf16 projection, at_oadd_push
// 3: any n_fft (odd sizes give torch.istft's hop (T-1) + 1 samples); Cartesian pack / unpack; strided phase scans
// 4: at_set_variant / at_get_variant (round 4; the library no longer reads environment variables).  The plan variants
//    (AT_VARIANT_RUN_LENGTH, AT_VARIANT_ISTFT_TILE, AT_VARIANT_ROW_RUN, AT_VARIANT_FRAME_WALKERS) are table entries, not
//    signatures: still 4.  So are the backward
//    entries (at_stft_backward, at_magnitude_backward, at_istft_backward, at_mfcc_backward, and invert_grad.hip's
//    at_magnitude_invert_backward, at_polar_to_complex_backward, at_cartesian_unpack_backward, and repr_grad.hip's
//    at_phase_scan_backward, at_cartesian_pack_backward, and the streaming path's at_rfft_frames_backward,
//    at_irfft_frames_backward, at_oadd_forward_backward, at_oadd_invert_backward) and spectral_distance.hip's
//    at_spectral_distance_sums / _backward and mel_distance.hip's at_mel_rows, at_mel_distance_sums / _backward and
//    pqmf.hip's at_pqmf_tile_blocks, at_pqmf_analysis, at_pqmf_synthesis and their streaming forms
//    at_pqmf_analysis_stream, at_pqmf_synthesis_stream, and true_peak.hip's at_true_peak, at_true_peak_plan,
//    at_true_peak_workspace_bytes, at_true_peak_backward: additions only.
int at_abi_version(void) { return 4; }

int at_set_variant(int which, int value) {
  if (which < 0 || which >= kVarCount || value < 0 || value > (which >= kVarFirstPlan ? 65535 : 4)) return AT_EINVAL;
  g_variants[which].store(value, std::memory_order_relaxed);
  return AT_OK;
}

int at_get_variant(int which) {
  if (which < 0 || which >= kVarCount) return AT_EINVAL;
  return g_variants[which].load(std::memory_order_relaxed);
}

const char* at_error_string(int code) {
  switch (code) {
    case AT_OK: return "ok";
    case AT_EINVAL: return "invalid argument";
    case AT_EUNSUPPORTED: return "unsupported configuration";
    case AT_ENOTINIT: return "at_init() not called for this device";
    case AT_EWORKSPACE: return "workspace too small";
    case AT_ELAUNCH: return "HIP launch/runtime error";
    default: return "unknown error";
  }
}

int at_init(int device) {
  if (device < 0 || device >= kMaxDevices) return AT_EINVAL;
  if (g_twiddles[device]) return AT_OK;
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess) return AT_ELAUNCH;
  if (hipSetDevice(device) != hipSuccess) return AT_ELAUNCH;
  std::vector<float2> tab(kTwiddleCount);
  const double two_pi = 6.283185307179586476925286766559;
  for (int k = 1; k < 8; ++k)
    for (int l = 0; l < 64; ++l) {
      double a1 = -two_pi * (double)(l * k) / 512.0;
      tab[(k - 1) * 64 + l] = make_float2((float)cos(a1), (float)sin(a1));
      double a2 = -two_pi * (double)((l & 7) * k) / 64.0;
      tab[(7 + k - 1) * 64 + l] = make_float2((float)cos(a2), (float)sin(a2));
    }
  for (int m = 0; m < 8; ++m)
    for (int l = 0; l < 64; ++l) {
      float2& w = tab[(14 + m) * 64 + l];
      inv1024::w1024(l + 64 * m, w.x, w.y);     // the inverse split relies on W^(512-k) = -conj(W^k) holding exactly
    }
  float2* d = nullptr;
  int rc = AT_OK;
  // the table, then the tile-counter ring of the persistent forward kernels (stft1024.hip: tile_counter_slot), zeroed
  if (hipMalloc((void**)&d, sizeof(float2) * (kTwiddleCount + kTileCtrSlots)) != hipSuccess) rc = AT_ELAUNCH;
  if (rc == AT_OK && hipMemcpy(d, tab.data(), sizeof(float2) * kTwiddleCount, hipMemcpyHostToDevice) != hipSuccess)
    rc = AT_ELAUNCH;
  if (rc == AT_OK && hipMemset(d + kTwiddleCount, 0, sizeof(float2) * kTileCtrSlots) != hipSuccess) rc = AT_ELAUNCH;
  float2* d2 = nullptr;
  if (rc == AT_OK) {
    // W_n^(r k), k < count, at t2[at + k]
    std::vector<float2> t2(kSideTableCount);
    auto fill = [&](int at, int count, int r, double n) {
      for (int k = 0; k < count; ++k) {
        const double a = -two_pi * (double)(r * k) / n;
        t2[at + k] = make_float2((float)cos(a), (float)sin(a));
      }
    };
    fill(kSideW2048, 1024, 1, 2048.0);
    fill(kSideW512, 256, 1, 512.0);
    for (int r = 1; r < 4; ++r) fill(kSide256 + (r - 1) * 128, 128, r, 512.0);
    for (int r = 1; r < 8; ++r) fill(kSide128 + (r - 1) * 64, 64, r, 512.0);
    fill(kSide4096, 2048, 1, 4096.0);
    for (int r = 1; r < 4; ++r) fill(kSide4096Radix + (r - 1) * 512, 512, r, 2048.0);
    if (hipMalloc((void**)&d2, sizeof(float2) * t2.size()) != hipSuccess) rc = AT_ELAUNCH;
    if (rc == AT_OK && hipMemcpy(d2, t2.data(), sizeof(float2) * t2.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = AT_ELAUNCH;
  }
  if (rc == AT_OK) {
    g_side[device] = d2;
    g_twiddles[device] = d;
  }
  (void)hipSetDevice(prev);
  return rc;
}

int at_stft_forward(const float* x, int64_t B, int64_t L, int64_t clip_stride, int64_t T, int n_fft, int hop,
                    int center, const float* window, float* out_complex, float* phase, void* stream) {
  if (B < 0 || T < 0 || L < 0 || hop <= 0 || n_fft <= 0) return AT_EINVAL;
  if (B * T == 0) return AT_OK;
  if (!x || !window || !out_complex) return AT_EINVAL;
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  if (center && L <= n_fft / 2) return AT_EINVAL;  // torch.stft: reflect pad must be < L
  hipStream_t s = (hipStream_t)stream;
  const uintptr_t walign = (uintptr_t)window;
  const float2 *tw = nullptr, *side = nullptr;
  if (n_fft == 1024 && (walign & 7) == 0) {
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    if ((hop == 256 || hop == 128 || hop == 512) && center && (clip_stride & 1) == 0)
      return launch_stft1024_h256_fwd(x, B, L, clip_stride, T, window, tw, (float2*)out_complex, phase, nullptr,
                                      nullptr, nullptr, nullptr, 0.f, 0, 0, 0, s, nullptr, hop);
    return launch_stft1024_fwd(x, B, L, clip_stride, T, hop, center, window, tw, (float2*)out_complex, phase, s);
  }
  if (n_fft == 2048 && (walign & 15) == 0) {      // two 512-point register FFTs + a radix-2 stage per frame
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    return launch_stft2048_fwd(x, B, L, clip_stride, T, hop, center, window, tw, side + kSideW2048, (float2*)out_complex,
                               phase, s);
  }
  if (n_fft == 4096 && (walign & 15) == 0) {      // four 512-point register FFTs + a radix-4 stage per frame
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    return launch_stft4096_fwd(x, B, L, clip_stride, T, hop, center, window, tw, side + kSide4096, (float2*)out_complex,
                               phase, s);
  }
  if ((n_fft == 256 || n_fft == 128) && (walign & 7) == 0) {     // four / eight frames per register FFT
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    return launch_stft_small_fwd(n_fft, x, B, L, clip_stride, T, hop, center, window, tw,
                                 side + (n_fft == 256 ? kSide256 : kSide128), (float2*)out_complex, phase, s);
  }
  if (n_fft == 512 && (walign & 7) == 0) {        // two frames per 512-point register FFT
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    return launch_stft512_fwd(x, B, L, clip_stride, T, hop, center, window, tw, side + kSideW512, (float2*)out_complex,
                              phase, s);
  }
  if (fft_mixed(n_fft))
    return launch_rfft_mixed(x, B, L, clip_stride, T, n_fft, hop, center, window, (float2*)out_complex, phase, s);
  return launch_rfft_generic(x, B, L, clip_stride, T, n_fft, hop, center, window, (float2*)out_complex, phase, s);
}

int at_stft_mel_forward(const float* x, int64_t B, int64_t L, int64_t clip_stride, int64_t T, int n_fft, int hop,
                        const float* window, const int32_t* lane_filter, const int32_t* lane_start,
                        const float* band_weights, int n_filters, int n_passes, const int32_t* pass_len_host,
                        int contrast, int power2, const float* offset, const float* scale, float eps,
                        float* out_complex_or_null, float* phase_or_null, float* feat, int feat_channel_major,
                        void* stream) {
  if (B < 0 || T < 0 || L < 0) return AT_EINVAL;
  // features only at n_fft 2048 / 512 (stft2048.hip, stft512.hip)
  const bool feat_only_2048 = (n_fft == 2048 || n_fft == 512) && hop >= 1 && !out_complex_or_null && !phase_or_null;
  if (!feat_only_2048) {
    if (n_fft != 1024 || (hop != 256 && hop != 128 && hop != 512) || (clip_stride & 1)) return AT_EUNSUPPORTED;
    if (hop != 256 && feat_channel_major) return AT_EUNSUPPORTED;
  }
  if (B * T == 0) return AT_OK;
  if (!x || !window || !feat || !lane_filter || !lane_start || !band_weights || !pass_len_host) return AT_EINVAL;
  if (n_filters <= 0 || n_passes <= 0 || n_passes > 16 || n_filters > 64 * n_passes) return AT_EINVAL;
  if ((offset == nullptr) != (scale == nullptr)) return AT_EINVAL;
  if (L <= n_fft / 2 || (((uintptr_t)window) & (n_fft == 2048 ? 15 : 7)) || (((uintptr_t)band_weights) & 15)) return AT_EINVAL;
  const float2 *tw = nullptr, *side = nullptr;
  if (!device_tables(tw, side)) return AT_ENOTINIT;
  BandBank bank = {lane_filter, lane_start, band_weights, n_filters, n_passes, {0}};
  long long table_floats = 0;
  for (int q = 0; q < n_passes; ++q) {
    if (pass_len_host[q] < 0 || pass_len_host[q] > 128 || (pass_len_host[q] & 3)) return AT_EINVAL;  // 4 bins per step
    bank.pass_len[q] = pass_len_host[q];
    table_floats += 64LL * pass_len_host[q];
  }
  if (table_floats > 8192) return AT_EUNSUPPORTED;   // LDS copy of the band weights
  if (feat_only_2048) {
    if (n_fft == 512)
      return launch_stft512_mel(x, B, L, clip_stride, T, hop, window, tw, side + kSideW512, &bank, contrast, power2, offset,
                                scale, eps, feat, feat_channel_major, (hipStream_t)stream);
    return launch_stft2048_mel(x, B, L, clip_stride, T, hop, window, tw, side + kSideW2048, &bank, contrast, power2, offset,
                               scale, eps, feat, feat_channel_major, (hipStream_t)stream);
  }
  return launch_stft1024_h256_fwd(x, B, L, clip_stride, T, window, tw, (float2*)out_complex_or_null, phase_or_null, &bank,
                                  feat, offset, scale, eps, contrast, power2, feat_channel_major, (hipStream_t)stream,
                                  nullptr, hop);
}

int at_stft_polar_forward(const float* x, int64_t B, int64_t L, int64_t clip_stride, int64_t T, int n_fft, int hop,
                          const float* window, const int32_t* lane_filter, const int32_t* lane_start,
                          const float* band_weights, int n_filters, int n_passes, const int32_t* pass_len_host,
                          int contrast, const float* mag_offset, const float* mag_scale, float eps,
                          const float* phase_offset, const float* phase_scale, float* out_stacked, void* stream) {
  if (B < 0 || T < 0 || L < 0) return AT_EINVAL;
  if (n_fft != 1024 || hop != 256 || (clip_stride & 1)) return AT_EUNSUPPORTED;
  if (B * T == 0) return AT_OK;
  if (!x || !window || !out_stacked || !lane_filter || !lane_start || !band_weights || !pass_len_host) return AT_EINVAL;
  const int F = n_fft / 2 + 1;
  if (n_filters != F || n_passes <= 0 || n_passes > 16 || n_filters > 64 * n_passes) return AT_EINVAL;   // stacked halves
  if ((mag_offset == nullptr) != (mag_scale == nullptr) || (phase_offset == nullptr) != (phase_scale == nullptr))
    return AT_EINVAL;
  if (L <= n_fft / 2 || (((uintptr_t)window) & 7) || (((uintptr_t)band_weights) & 15)) return AT_EINVAL;
  const float2 *tw = nullptr, *side = nullptr;
  if (!device_tables(tw, side)) return AT_ENOTINIT;
  BandBank bank = {lane_filter, lane_start, band_weights, n_filters, n_passes, {0}};
  long long table_floats = 0;
  for (int q = 0; q < n_passes; ++q) {
    if (pass_len_host[q] < 0 || pass_len_host[q] > 128 || (pass_len_host[q] & 3)) return AT_EINVAL;
    bank.pass_len[q] = pass_len_host[q];
    table_floats += 64LL * pass_len_host[q];
  }
  if (table_floats > 8192) return AT_EUNSUPPORTED;
  const PolarOut polar = {out_stacked + F, 2LL * F, 2LL * F, phase_offset, phase_scale};
  return launch_stft1024_h256_fwd(x, B, L, clip_stride, T, window, tw, nullptr, nullptr, &bank, out_stacked, mag_offset,
                                  mag_scale, eps, contrast, 0, 0, (hipStream_t)stream, &polar);
}

int at_istft_envelope_table(const float* inv_window, int n_fft, int hop, float* env16, void* stream) {
  if (!inv_window || !env16 || hop <= 0 || n_fft <= 0) return AT_EINVAL;
  if (n_fft % hop) return AT_EUNSUPPORTED;
  const int R = n_fft / hop;
  if (R != 2 && R != 4 && R != 8) return AT_EUNSUPPORTED;
  int total = (1 << R) * hop;
  hipLaunchKernelGGL(envelope_table_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, inv_window,
                     n_fft, hop, R, env16);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// The fused inverse (irfft + window + overlap-add + envelope in one kernel; stft512.hip ... stft4096.hip) exists at
// n_fft 512, 1024, 2048, 4096 with hop n/8, n/4, n/2 ...
static bool istft_fused_size(int n_fft, int hop) {
  return (n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096) &&
         (hop == n_fft / 8 || hop == n_fft / 4 || hop == n_fft / 2);
}
// ... and takes the envelope table, with window, table and output aligned to the size's vector width: 8 bytes at 512 and
// 1024, 16 bytes at 2048 and 4096
static bool istft_fused(int n_fft, int hop, const float* env16, const float* w, const float* y) {
  const uintptr_t mask = n_fft >= 2048 ? 15 : 7;
  return istft_fused_size(n_fft, hop) && env16 != nullptr &&
         ((((uintptr_t)w) | ((uintptr_t)env16) | ((uintptr_t)y)) & mask) == 0;
}

// irfft(X) * window of pre-framed spectra by size: the register kernels of n_fft 2048 / 4096 (window and frames 16-byte
// aligned) and 256 / 128 / 512 (8-byte aligned; several frames of one stream of frames_per_stream frames share a
// transform), else the mixed-radix or the generic kernel.  n_fft 1024 is NOT here: at_irfft_frames_streams takes its
// register kernel first, at_istft's workspace path (1024 at a hop outside {128, 256, 512}) the generic one.
static int launch_frames_inverse(int n_fft, const float2* X, const float* mag, const float* phase, long long nframes,
                                 long long frames_per_stream, const float* window, float* frames, hipStream_t s) {
  const uintptr_t align = ((uintptr_t)window) | ((uintptr_t)frames);
  if (((n_fft == 2048 || n_fft == 4096) && (align & 15) == 0) ||
      ((n_fft == 256 || n_fft == 128 || n_fft == 512) && (align & 7) == 0)) {
    const float2 *tw = nullptr, *side = nullptr;
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    switch (n_fft) {
      case 2048: return launch_irfft2048_frames(X, mag, phase, nframes, window, tw, side + kSideW2048, frames, s);
      case 4096: return launch_irfft4096_frames(X, mag, phase, nframes, window, tw, side + kSide4096, frames, s);
      case 512:
        return launch_irfft512_frames(X, mag, phase, nframes, frames_per_stream, window, tw, side + kSideW512, frames, s);
      default:
        return launch_irfft_small_frames(n_fft, X, mag, phase, nframes, frames_per_stream, window, tw,
                                         side + (n_fft == 256 ? kSide256 : kSide128), frames, s);
    }
  }
  if (fft_mixed(n_fft)) return launch_irfft_mixed(X, mag, phase, nframes, n_fft, window, frames, s);
  return launch_irfft_generic(X, mag, phase, nframes, n_fft, window, frames, s);
}

// The zeros below hold for a 16-byte aligned window (with env16 and y aligned alike): at_istft leaves the fused path for a
// less aligned one and then asks for the frames workspace (AT_EWORKSPACE before anything is launched).
size_t at_istft_workspace_bytes(int64_t B, int64_t T, int n_fft, int hop) {
  if (istft_fused_size(n_fft, hop)) return 0;   // with the envelope table; see at_istft
  return (size_t)B * (size_t)T * (size_t)n_fft * sizeof(float);
}

int at_istft(const float* X_complex, const float* mag, const float* phase, int64_t B, int64_t T, int n_fft, int hop,
             const float* inv_window, const float* env16, float* y, void* workspace, size_t workspace_bytes,
             void* stream) {
  if (B < 0 || T < 0 || hop <= 0 || n_fft <= 0) return AT_EINVAL;
  if (B == 0 || T == 0 || (T == 1 && !(n_fft & 1))) return AT_OK;     // hop * (T - 1) + (n_fft & 1) samples per clip
  if (!inv_window || !y) return AT_EINVAL;
  if (!X_complex && !(mag && phase)) return AT_EINVAL;
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const float2* X = (const float2*)X_complex;
  if (istft_fused(n_fft, hop, env16, inv_window, y)) {
    const float2 *tw = nullptr, *side = nullptr;
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    switch (n_fft) {
      case 512: return launch_istft512_ola(X, mag, phase, B, T, hop, inv_window, env16, tw, side + kSideW512, y, s);
      case 1024: return launch_istft1024_ola(X, mag, phase, B, T, hop, inv_window, env16, tw, y, s);
      case 2048: return launch_istft2048_ola(X, mag, phase, B, T, hop, inv_window, env16, tw, side + kSideW2048, y, s);
      default: return launch_istft4096_ola(X, mag, phase, B, T, hop, inv_window, env16, tw, side + kSide4096, y, s);
    }
  }
  size_t need = (size_t)B * (size_t)T * (size_t)n_fft * sizeof(float);
  if (!workspace || workspace_bytes < need) return AT_EWORKSPACE;
  const int rc = launch_frames_inverse(n_fft, X, mag, phase, B * T, T, inv_window, (float*)workspace, s);
  if (rc) return rc;
  return launch_ola_gather((const float*)workspace, B, T, n_fft, hop, inv_window, y, s);
}

int at_istft_griffinlim(const float* mag, const float* rebuilt_complex, const float* tprev_complex_or_null,
                        float momentum_over_1p, int64_t B, int64_t T, int n_fft, int hop, const float* inv_window,
                        const float* env16, float* y, void* stream) {
  if (B < 0 || T < 0 || hop <= 0 || n_fft <= 0) return AT_EINVAL;
  if (B == 0 || T <= 1) return AT_OK;
  if (!mag || !rebuilt_complex || !inv_window || !y) return AT_EINVAL;
  if (n_fft != 1024 || !istft_fused(n_fft, hop, env16, inv_window, y)) return AT_EUNSUPPORTED;
  const float2 *tw = nullptr, *side = nullptr;
  if (!device_tables(tw, side)) return AT_ENOTINIT;
  // first iteration (no previous spectrum): momentum 0 against the rebuilt spectrum itself
  const float2* tprev = tprev_complex_or_null ? (const float2*)tprev_complex_or_null : (const float2*)rebuilt_complex;
  const float mom = tprev_complex_or_null ? momentum_over_1p : 0.0f;
  return launch_istft1024_ola((const float2*)rebuilt_complex, mag, nullptr, B, T, hop, inv_window, env16, tw, y,
                              (hipStream_t)stream, tprev, mom);
}

// frames_per_stream: at n_fft 128 / 256 / 512 several frames share one register FFT (stft_small.hip, stft512.hip), and
// only frames of the same stream may: nothing outside a stream reaches its output.  The other sizes take one frame per
// transform and ignore it.
int at_irfft_frames_streams(const float* X_complex, const float* mag, const float* phase, int64_t nframes,
                            int64_t frames_per_stream, int n_fft, const float* inv_window, float* frames, void* stream) {
  if (nframes < 0 || n_fft <= 0) return AT_EINVAL;
  if (nframes == 0) return AT_OK;
  if (frames_per_stream <= 0 || nframes % frames_per_stream) return AT_EINVAL;
  if (!inv_window || !frames) return AT_EINVAL;
  if (!X_complex && !(mag && phase)) return AT_EINVAL;
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const float2* X = (const float2*)X_complex;
  // only here, ahead of the shared chain: at_istft's workspace path sends n_fft 1024 to the generic kernel
  if (n_fft == 1024 && (((uintptr_t)inv_window) & 7) == 0 && (((uintptr_t)frames) & 7) == 0) {
    const float2 *tw = nullptr, *side = nullptr;
    if (!device_tables(tw, side)) return AT_ENOTINIT;
    return launch_irfft1024_frames(X, mag, phase, nframes, inv_window, tw, frames, s);
  }
  return launch_frames_inverse(n_fft, X, mag, phase, nframes, frames_per_stream, inv_window, frames, s);
}

// the whole call is one stream
int at_irfft_frames(const float* X_complex, const float* mag, const float* phase, int64_t nframes, int n_fft,
                    const float* inv_window, float* frames, void* stream) {
  if (nframes < 0) return AT_EINVAL;
  return at_irfft_frames_streams(X_complex, mag, phase, nframes, nframes > 0 ? nframes : 1, n_fft, inv_window, frames,
                                 stream);
}


// ---- backward passes (autograd.hip) ----------------------------------------------------------------------------------

// clips per chunk of the STFT adjoint: its irFFT frames (clips x T x n_fft floats) stay within 1 GiB of workspace
static int64_t adj_chunk_clips(int64_t B, int64_t T, int n_fft) {
  const int64_t per_clip = T * (int64_t)n_fft;
  int64_t c = per_clip > 0 ? (int64_t(1) << 28) / per_clip : B;
  if (c < 1) c = 1;
  return c < B ? c : B;
}

static size_t adj_window_bytes(int n_fft) { return ((size_t)n_fft * sizeof(float) + 255) / 256 * 256; }

size_t at_stft_backward_workspace_bytes(int64_t B, int64_t T, int n_fft, int hop) {
  if (B <= 0 || T <= 0 || n_fft <= 0 || hop <= 0) return 0;
  return adj_window_bytes(n_fft) + (size_t)adj_chunk_clips(B, T, n_fft) * (size_t)T * (size_t)n_fft * sizeof(float);
}

int at_stft_backward(const float* G_complex, int64_t B, int64_t T, int64_t L, int n_fft, int hop, const float* window,
                     float* dx, void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || T <= 0 || L <= 0 || hop <= 0 || n_fft <= 0) return AT_EINVAL;
  if (L <= n_fft / 2 || T != 1 + (L - (n_fft & 1)) / hop) return AT_EINVAL;   // the forward's frames of a reflect-padded clip
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  if (B == 0) return AT_OK;
  if (!G_complex || !window || !dx || !workspace) return AT_EINVAL;
  if ((((uintptr_t)workspace) & 255) || workspace_bytes < at_stft_backward_workspace_bytes(B, T, n_fft, hop))
    return AT_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* wscaled = (float*)workspace;
  float* frames = (float*)((char*)workspace + adj_window_bytes(n_fft));
  int rc = launch_adj_window(window, n_fft, 0.5f * (float)n_fft, wscaled, s);
  if (rc) return rc;
  const int64_t F = n_fft / 2 + 1, chunk = adj_chunk_clips(B, T, n_fft);
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = (B - b0 < chunk) ? B - b0 : chunk;
    const float* G = G_complex + 2 * b0 * T * F;
    // n_fft 128 / 256 / 512: the register kernels transform 8 / 4 / 2 consecutive frames together, so a frame's bits
    // would depend on the next clip's frames when a group straddles two clips; the generic kernel takes one frame at a
    // time and keeps a clip's gradient independent of its batch
    if (n_fft == 128 || n_fft == 256 || n_fft == 512)
      rc = launch_irfft_generic((const float2*)G, nullptr, nullptr, nb * T, n_fft, wscaled, frames, s);
    else
      rc = at_irfft_frames(G, nullptr, nullptr, nb * T, n_fft, wscaled, frames, stream);
    if (rc) return rc;
    rc = launch_adj_ola_fold(frames, (const float2*)G, window, dx + b0 * L, nb, T, L, n_fft, hop, s);
    if (rc) return rc;
  }
  return AT_OK;
}

// ISTFT adjoint: clips per chunk so that u (P floats per clip) and the polar form's rFFT rows (T F
// complex) stay within 1 GiB of workspace
static int64_t istft_adj_chunk_clips(int64_t B, int64_t T, int n_fft, int hop) {
  const int64_t per_clip = (int64_t)n_fft + (int64_t)hop * (T - 1) + 2 * T * (int64_t)(n_fft / 2 + 1);
  int64_t c = (int64_t(1) << 28) / per_clip;
  if (c < 1) c = 1;
  return c < B ? c : B;
}

size_t at_istft_backward_workspace_bytes(int64_t B, int64_t T, int n_fft, int hop) {
  if (B <= 0 || T <= 0 || n_fft <= 0 || hop <= 0) return 0;
  const int64_t c = istft_adj_chunk_clips(B, T, n_fft, hop), P = (int64_t)n_fft + (int64_t)hop * (T - 1);
  return adj_window_bytes(n_fft) + ((size_t)c * (size_t)P * sizeof(float) + 255) / 256 * 256 +
         (size_t)c * (size_t)T * (size_t)(n_fft / 2 + 1) * 2 * sizeof(float);
}

int at_istft_backward(const float* gy, int64_t B, int64_t T, int n_fft, int hop, const float* inv_window,
                      const float* env16, const float* phase, float* out, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (B < 0 || T < 0 || hop <= 0 || n_fft <= 0) return AT_EINVAL;
  if (B == 0 || T == 0) return AT_OK;
  if (!inv_window || !out) return AT_EINVAL;
  if (!phase && (((uintptr_t)out) & 7)) return AT_EINVAL;    // complex64 rows
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t F = n_fft / 2 + 1;
  if (T == 1 && !(n_fft & 1)) {       // no output sample: nothing flows back
    const size_t bytes = (size_t)B * (size_t)F * (phase ? sizeof(float) : 2 * sizeof(float));
    return hipMemsetAsync(out, 0, bytes, s) == hipSuccess ? AT_OK : AT_ELAUNCH;
  }
  if (!gy) return AT_EINVAL;
  (void)env16;   // the envelope is summed per sample (prep kernel); the table is not needed
  const int64_t chunk = istft_adj_chunk_clips(B, T, n_fft, hop), P = (int64_t)n_fft + (int64_t)hop * (T - 1);
  const int64_t Ly = (int64_t)hop * (T - 1) + (n_fft & 1);
  const size_t u_bytes = ((size_t)chunk * (size_t)P * sizeof(float) + 255) / 256 * 256;
  if (!workspace || (((uintptr_t)workspace) & 255) ||
      workspace_bytes < adj_window_bytes(n_fft) + u_bytes + (size_t)chunk * (size_t)T * (size_t)F * 2 * sizeof(float))
    return AT_EWORKSPACE;
  float* wscaled = (float*)workspace;
  float* u = (float*)((char*)workspace + adj_window_bytes(n_fft));
  float2* gx = (float2*)((char*)u + u_bytes);
  int rc = launch_adj_window(inv_window, n_fft, 2.0f / (float)n_fft, wscaled, s);
  if (rc) return rc;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = (B - b0 < chunk) ? B - b0 : chunk;
    rc = launch_istft_adj_prep(gy + b0 * Ly, inv_window, u, nb, T, n_fft, hop, s);
    if (rc) return rc;
    // the complex form writes the caller's rows directly, the polar form the workspace rows
    float2* X = phase ? gx : (float2*)out + b0 * T * F;
    // n_fft 128 / 256 / 512: the register kernels transform 8 / 4 / 2 consecutive frames together, which would mix the
    // rounding of a clip's last frames with the next clip's first (odd T): the generic kernel takes one frame at a time
    if (n_fft == 128 || n_fft == 256 || n_fft == 512)
      rc = launch_rfft_generic(u, nb, P, P, T, n_fft, hop, 0, wscaled, X, nullptr, s);
    else
      rc = at_stft_forward(u, nb, P, P, T, n_fft, hop, 0, wscaled, (float*)X, nullptr, stream);
    if (rc) return rc;
    rc = launch_istft_adj_finish(X, phase ? phase + b0 * T * F : nullptr, phase ? (void*)(out + b0 * T * F) : (void*)X,
                                 nb * T, n_fft, s);
    if (rc) return rc;
  }
  return AT_OK;
}

// ---- the streaming path (stream_grad.hip): per-frame adjoints, no overlap-add --------------------------------------------

size_t at_rfft_frames_backward_workspace_bytes(int64_t nframes, int n_fft) {
  if (nframes <= 0 || n_fft <= 0) return 0;
  return adj_window_bytes(n_fft);
}

int at_rfft_frames_backward(const float* G_complex, int64_t nframes, int64_t frames_per_stream, int n_fft,
                            const float* window, float* gframes, void* workspace, size_t workspace_bytes, void* stream) {
  if (nframes < 0 || n_fft <= 0) return AT_EINVAL;
  if (nframes == 0) return AT_OK;
  if (frames_per_stream <= 0 || nframes % frames_per_stream) return AT_EINVAL;
  if (!G_complex || !window || !gframes) return AT_EINVAL;
  if (((uintptr_t)G_complex) & 7) return AT_EINVAL;    // complex64 rows
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  if (!workspace || (((uintptr_t)workspace) & 255) || workspace_bytes < adj_window_bytes(n_fft)) return AT_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* wscaled = (float*)workspace;
  int rc = launch_adj_window(window, n_fft, 0.5f * (float)n_fft, wscaled, s);
  if (rc) return rc;
  // the forward's own arrangement: at n_fft 128 / 256 / 512 the frames that share a register FFT belong to one stream
  rc = at_irfft_frames_streams(G_complex, nullptr, nullptr, nframes, frames_per_stream, n_fft, wscaled, gframes, stream);
  if (rc) return rc;
  return launch_rfft_adj_edge(gframes, (const float2*)G_complex, window, nframes, n_fft, s);
}

// streams per chunk of the polar form: its rFFT rows (streams x frames_per_stream x F complex) stay within 1 GiB
static int64_t rt_adj_chunk_streams(int64_t streams, int64_t frames_per_stream, int n_fft) {
  const int64_t per_stream = frames_per_stream * (int64_t)(n_fft / 2 + 1);
  int64_t c = (int64_t(1) << 27) / per_stream;
  if (c < 1) c = 1;
  return c < streams ? c : streams;
}

size_t at_irfft_frames_backward_workspace_bytes(int64_t nframes, int64_t frames_per_stream, int n_fft, int polar) {
  if (nframes <= 0 || frames_per_stream <= 0 || n_fft <= 0 || nframes % frames_per_stream) return 0;
  size_t bytes = adj_window_bytes(n_fft);
  if (polar)
    bytes += (size_t)rt_adj_chunk_streams(nframes / frames_per_stream, frames_per_stream, n_fft) *
             (size_t)frames_per_stream * (size_t)(n_fft / 2 + 1) * 2 * sizeof(float);
  return bytes;
}

int at_irfft_frames_backward(const float* gframes, const float* phase_or_null, int64_t nframes, int64_t frames_per_stream,
                             int n_fft, const float* inv_window, float* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (nframes < 0 || n_fft <= 0) return AT_EINVAL;
  if (nframes == 0) return AT_OK;
  if (frames_per_stream <= 0 || nframes % frames_per_stream) return AT_EINVAL;
  if (!gframes || !inv_window || !out) return AT_EINVAL;
  const float* phase = phase_or_null;
  if (!phase && (((uintptr_t)out) & 7)) return AT_EINVAL;    // complex64 rows
  if (!fft_size_ok(n_fft)) return AT_EUNSUPPORTED;
  if (!workspace || (((uintptr_t)workspace) & 255) ||
      workspace_bytes < at_irfft_frames_backward_workspace_bytes(nframes, frames_per_stream, n_fft, phase != nullptr))
    return AT_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t F = n_fft / 2 + 1, S = nframes / frames_per_stream, n = frames_per_stream;
  const int64_t L = n * (int64_t)n_fft;                 // a stream: n back-to-back frames, hop = n_fft
  float* wscaled = (float*)workspace;
  float2* rows = (float2*)((char*)workspace + adj_window_bytes(n_fft));
  int rc = launch_adj_window(inv_window, n_fft, 2.0f / (float)n_fft, wscaled, s);
  if (rc) return rc;
  // the complex form writes the caller's rows in one go, the polar form the workspace rows a chunk of streams at a time
  const int64_t chunk = phase ? rt_adj_chunk_streams(S, n, n_fft) : S;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t ns = (S - s0 < chunk) ? S - s0 : chunk;
    float2* X = phase ? rows : (float2*)out;
    // the forward's own arrangement (RealtimeSTFT on dense frames): one clip per stream, so that the frames that share a
    // register FFT at n_fft 128 / 256 / 512 belong to one stream
    rc = at_stft_forward(gframes + s0 * L, ns, L, L, n, n_fft, n_fft, 0, wscaled, (float*)X, nullptr, stream);
    if (rc) return rc;
    rc = launch_istft_adj_finish(X, phase ? phase + s0 * n * F : nullptr, phase ? (void*)(out + s0 * n * F) : (void*)X,
                                 ns * n, n_fft, s);
    if (rc) return rc;
  }
  return AT_OK;
}

int at_oadd_forward_backward(const float* gframes, int64_t S, int64_t n, int n_fft, int hop, int keep, int64_t C,
                             float* gx, void* stream) {
  if (S < 0 || n <= 0 || n_fft <= 0 || hop <= 0 || keep < 0 || C <= 0) return AT_EINVAL;
  if (S == 0) return AT_OK;
  if (!gframes || !gx) return AT_EINVAL;
  return launch_oadd_forward_adj(gframes, S, n, n_fft, hop, keep, C, gx, (hipStream_t)stream);
}

int at_oadd_invert_backward(const float* gy, int64_t S, int64_t n, int n_fft, int hop, int keep, const float* gain,
                            float* gframes, void* stream) {
  if (S < 0 || n <= 0 || n_fft <= 0 || hop <= 0 || keep < 0) return AT_EINVAL;
  if ((n - 1) * (int64_t)hop + n_fft < keep) return AT_EINVAL;
  if (S == 0) return AT_OK;
  if (!gain || !gframes) return AT_EINVAL;
  if (!gy && (n - 1) * (int64_t)hop + n_fft > keep) return AT_EINVAL;    // no output sample: gy is not read
  return launch_oadd_invert_adj(gy, S, n, n_fft, hop, keep, gain, gframes, (hipStream_t)stream);
}

int at_magnitude_backward(const void* A, int a_kind, int64_t rows, int K, const float* dF, int N, int col_off,
                          const int* f_start, const int* f_len, const int* f_off, const float* f_w, int f_nnz,
                          const int* t_start, const int* t_len, const int* t_off, const float* t_w, int t_nnz, int contrast, const float* scale,
                          float eps, const void* dX_accum, void* dX, void* stream) {
  if (rows < 0 || K <= 0 || N <= 0 || col_off < 0 || col_off >= N) return AT_EINVAL;
  if ((a_kind != 0 && a_kind != 3) || contrast < 0 || contrast > 3) return AT_EINVAL;
  if (rows == 0) return AT_OK;
  if (!A || !dF || !dX) return AT_EINVAL;
  const bool banked = f_w != nullptr;
  if (banked && !(f_start && f_len && f_off && t_start && t_len && t_off && t_w && f_nnz > 0 && t_nnz > 0)) return AT_EINVAL;
  if (!banked && N != K) return AT_EINVAL;
  at_hip::MagBwdParams p = {A, a_kind, rows, K, N, col_off, dF, {f_start, f_len, f_off, f_w, N, f_nnz},
                            {t_start, t_len, t_off, t_w, K, t_nnz}, contrast, scale, eps, dX_accum, dX};
  return at_hip::launch_magnitude_backward(p, (hipStream_t)stream);
}

int at_mfcc_backward(const float* X_complex, int64_t B, int64_t T, int K, const float* dF, int C, int N, int power,
                     const int* f_start, const int* f_len, const int* f_off, const float* f_w, int f_nnz,
                     const int* t_start, const int* t_len, const int* t_off, const float* t_w, int t_nnz,
                     const float* dct_t, const float* scale, float* dX_complex, void* stream) {
  if (B < 0 || T <= 0 || K <= 0 || N <= 0 || C <= 0 || (power != 1 && power != 2)) return AT_EINVAL;
  if (!dct_t && C != N) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!X_complex || !dF || !dX_complex) return AT_EINVAL;
  if ((((uintptr_t)X_complex) & 7) || (((uintptr_t)dX_complex) & 7)) return AT_EINVAL;    // complex64 rows
  if (!(t_start && t_len && t_off && t_w && t_nnz > 0)) return AT_EINVAL;
  if (dct_t && !(f_start && f_len && f_off && f_w && f_nnz > 0)) return AT_EINVAL;
  at_hip::MfccBwdParams p = {(const float2*)X_complex, (float2*)dX_complex, dF, B, T, K, N, C, power,
                             {f_start, f_len, f_off, f_w, N, f_nnz}, {t_start, t_len, t_off, t_w, K, t_nnz}, dct_t, scale};
  return at_hip::launch_mfcc_backward(p, (hipStream_t)stream);
}

}  // extern "C"

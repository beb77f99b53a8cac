// spectral_distance.hip -- the two kernels of SpectralDistance (losses.py, autograd.SpectralDistanceFunction): the
// per-clip sums of a spectral distance between two complex spectra of one shape, and its backward, which turns the
// spectra into their own gradients in place.  The STFTs around them are ops.stft_forward / ops.stft_backward.
//
// For clip b, X and Y its n = T F bins of the generated and of the target spectrum, A = |X|, Bm = |Y|:
//     S_D = sum (A - Bm)^2      S_B = sum Bm^2      S_L = sum |ln(A + eps) - ln(Bm + eps)|
//     loss_b = lin_weight S_D / S_B + log_weight S_L / n                        (summed over scales by the caller)
// Backward, g the upstream gradient of loss_b, d = A - Bm:
//     dA  = g (lin_weight 2 d / S_B + log_weight sgn(d) / (n (A + eps)))
//     dBm = g (lin_weight (-2 d / S_B - 2 Bm S_D / S_B^2) - log_weight sgn(d) / (n (Bm + eps)))
//     G_X = dA X / A (0 where A == 0),   G_Y = dBm Y / Bm (0 where Bm == 0)      (dRe + i dIm, as at_mfcc_backward)
// ln is monotone, so sgn(d) is the sign of the log difference: the backward takes no logarithm.
//
// Order of the sums.  A clip is cut into slices of kSdSlice bins; ONE workgroup of kSdThreads lanes reduces one slice:
// lane t adds bins t, t + 256, ... of the slice in that order in fp32, the 64 lanes of a wave fold by a fixed xor tree,
// lane 0 adds the four waves in wave order and stores the slice's three partials.  A second kernel adds a clip's
// partials in slice order in double.  The order is thus a function of n alone -- not of B, of the clip's place in the
// batch, or of the grid, which is exactly B x ceil(n / kSdSlice) workgroups -- and there are no float atomics: a clip's
// bits do not depend on what it rides with, and a NaN stays in its clip.
//
// Lanes move 8 bytes (one complex64 bin), a wave 512 contiguous bytes.  A clip starts at byte b n 8: with n odd (F is
// odd, so every odd T) odd clips are only 8-byte aligned, and a 16-byte lane would have to pair bins differently in
// odd and even clips -- another order per clip position.  So no lane is wider than a bin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "sd_fold.h"   // sd_block_fold, sd_clip_sums_kernel: shared with mel_distance.hip

namespace at_hip {

constexpr int kSdThreads = 256;
constexpr int kSdPerLane = 16;
constexpr int kSdSlice = kSdThreads * kSdPerLane;   // bins per slice (spectral_distance_cases.py restates it)

__device__ __forceinline__ float sd_abs(float2 v) { return sqrtf(fmaf(v.x, v.x, v.y * v.y)); }

// workgroup blk reduces slice blk % slices of clip blk / slices into partial[blk][3]
__global__ __launch_bounds__(kSdThreads) void sd_slice_sums_kernel(const float2* __restrict__ X,
                                                                    const float2* __restrict__ Y, long long n,
                                                                    long long slices, float eps,
                                                                    float* __restrict__ partial) {
  const long long blk = blockIdx.x;
  const long long b = blk / slices;
  const long long i0 = (blk - b * slices) * kSdSlice + threadIdx.x;
  const float2* xr = X + b * n;
  const float2* yr = Y + b * n;
  float sd = 0.f, sb = 0.f, sl = 0.f;
  float2 xv[kSdPerLane], yv[kSdPerLane];
#pragma unroll
  for (int j = 0; j < kSdPerLane; ++j) {      // every load of the slice is issued before the first use
    const long long i = i0 + (long long)j * kSdThreads;
    const bool live = i < n;
    xv[j] = live ? xr[i] : make_float2(0.f, 0.f);
    yv[j] = live ? yr[i] : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < kSdPerLane; ++j) {
    if (i0 + (long long)j * kSdThreads < n) {
      const float a = sd_abs(xv[j]), bm = sd_abs(yv[j]);
      const float d = a - bm;
      sd = fmaf(d, d, sd);
      sb = fmaf(bm, bm, sb);
      sl += fabsf(logf(a + eps) - logf(bm + eps));
    }
  }
  sd_block_fold<kSdThreads>(sd, sb, sl);
  if (threadIdx.x == 0) {
    float* dst = partial + 3 * blk;
    dst[0] = sd; dst[1] = sb; dst[2] = sl;
  }
}

// workgroup blk turns slice blk % slices of clip blk / slices of X (NEED_X) and of Y (NEED_Y) into its gradient
template <bool NEED_X, bool NEED_Y>
__global__ __launch_bounds__(kSdThreads) void sd_backward_kernel(float2* __restrict__ X, float2* __restrict__ Y,
                                                                  long long n, long long slices,
                                                                  const double* __restrict__ sums,
                                                                  const float* __restrict__ gclip, float lin_weight,
                                                                  float log_weight, float eps) {
  const long long blk = blockIdx.x;
  const long long b = blk / slices;
  const long long i0 = (blk - b * slices) * kSdSlice + threadIdx.x;
  float2* xr = X + b * n;
  float2* yr = Y + b * n;
  // the clip's constants, in double: S_B^2 of a loud clip leaves fp32's range
  const double g = (double)gclip[b], s_d = sums[3 * b], inv_sb = 1.0 / sums[3 * b + 1];
  const double lin2 = 2.0 * g * (double)lin_weight * inv_sb;
  const float c_lin = (float)lin2;                                  // g lin_weight 2 / S_B
  const float c_sq = (float)(lin2 * s_d * inv_sb);                  // g lin_weight 2 S_D / S_B^2
  const float c_log = (float)(g * (double)log_weight / (double)n);  // g log_weight / n
  float2 xv[kSdPerLane], yv[kSdPerLane];
#pragma unroll
  for (int j = 0; j < kSdPerLane; ++j) {
    const long long i = i0 + (long long)j * kSdThreads;
    const bool live = i < n;
    xv[j] = live ? xr[i] : make_float2(0.f, 0.f);
    yv[j] = live ? yr[i] : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < kSdPerLane; ++j) {
    const long long i = i0 + (long long)j * kSdThreads;
    if (i < n) {
      const float a = sd_abs(xv[j]), bm = sd_abs(yv[j]);
      const float d = a - bm;
      const float lg = d > 0.f ? c_log : (d < 0.f ? -c_log : 0.f * d);    // c_log sgn(d); NaN stays NaN
      const float lind = c_lin * d;
      if (NEED_X) {
        const float da = lind + lg / (a + eps);
        const float r = da / a;
        xr[i] = a == 0.f ? make_float2(0.f, 0.f) : make_float2(r * xv[j].x, r * xv[j].y);
      }
      if (NEED_Y) {
        const float db = -lind - c_sq * bm - lg / (bm + eps);
        const float r = db / bm;
        yr[i] = bm == 0.f ? make_float2(0.f, 0.f) : make_float2(r * yv[j].x, r * yv[j].y);
      }
    }
  }
}

static inline long long sd_slices(long long n) { return (n + kSdSlice - 1) / kSdSlice; }

}  // namespace at_hip

extern "C" {

size_t at_spectral_distance_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n < 1) return 0;
  return sizeof(float) * 3 * (size_t)B * (size_t)at_hip::sd_slices(n);
}

int at_spectral_distance_sums(const float* X_complex, const float* Y_complex, int64_t B, int64_t n, float eps,
                              double* sums, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace at_hip;
  if (B < 0 || n < 1 || !(eps >= 0.f)) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!X_complex || !Y_complex || !sums) return AT_EINVAL;
  if ((((uintptr_t)X_complex) & 7) || (((uintptr_t)Y_complex) & 7)) return AT_EINVAL;    // complex64 bins
  const long long slices = sd_slices(n), blocks = (long long)B * slices;
  if (blocks > 0x7fffffffLL) return AT_EUNSUPPORTED;
  if (!workspace || (((uintptr_t)workspace) & 3) || workspace_bytes < at_spectral_distance_workspace_bytes(B, n))
    return AT_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sd_slice_sums_kernel, dim3((unsigned)blocks), dim3(kSdThreads), 0, s, (const float2*)X_complex,
                     (const float2*)Y_complex, (long long)n, slices, eps, (float*)workspace);
  hipLaunchKernelGGL(sd_clip_sums_kernel<kSdThreads>, dim3((unsigned)((3 * B + kSdThreads - 1) / kSdThreads)), dim3(kSdThreads), 0, s,
                     (const float*)workspace, (long long)B, slices, sums);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_spectral_distance_backward(float* X_complex, float* Y_complex, int64_t B, int64_t n, const double* sums,
                                  const float* gclip, float lin_weight, float log_weight, float eps, int need_x,
                                  int need_y, void* stream) {
  using namespace at_hip;
  if (B < 0 || n < 1 || !(eps >= 0.f) || (!need_x && !need_y)) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!X_complex || !Y_complex || !sums || !gclip) return AT_EINVAL;
  if ((((uintptr_t)X_complex) & 7) || (((uintptr_t)Y_complex) & 7)) return AT_EINVAL;
  const long long slices = sd_slices(n), blocks = (long long)B * slices;
  if (blocks > 0x7fffffffLL) return AT_EUNSUPPORTED;
  auto run = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kSdThreads), 0, (hipStream_t)stream, (float2*)X_complex,
                       (float2*)Y_complex, (long long)n, slices, sums, gclip, lin_weight, log_weight, eps);
  };
  if (need_x && need_y) run(sd_backward_kernel<true, true>);
  else if (need_x) run(sd_backward_kernel<true, false>);
  else run(sd_backward_kernel<false, true>);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

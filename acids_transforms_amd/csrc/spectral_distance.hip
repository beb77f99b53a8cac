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
// Order of the sums: distance_core.h, on slices of kDistSlice bins.
//
// Lanes move 8 bytes (one complex64 bin), a wave 512 contiguous bytes.  A clip starts at byte b n 8: with n odd (F is
// odd, so every odd T) odd clips are only 8-byte aligned, and a 16-byte lane would have to pair bins differently in
// odd and even clips -- another order per clip position.  So no lane is wider than a bin.
#include "distance_core.h"   // the slice geometry, the sums, the constants and derivatives: shared with mel_distance.hip

namespace at_hip {

// workgroup blk turns slice blk % slices of clip blk / slices of X (NEED_X) and of Y (NEED_Y) into its gradient
template <bool NEED_X, bool NEED_Y>
__global__ __launch_bounds__(kDistThreads) void sd_backward_kernel(float2* __restrict__ X, float2* __restrict__ Y,
                                                                    long long n, long long slices,
                                                                    const double* __restrict__ sums,
                                                                    const float* __restrict__ gclip, float lin_weight,
                                                                    float log_weight, float eps) {
  const long long blk = blockIdx.x;
  const long long b = blk / slices;
  const long long i0 = (blk - b * slices) * kDistSlice + threadIdx.x;
  float2* xr = X + b * n;
  float2* yr = Y + b * n;
  float c_lin, c_sq, c_log;
  dist_consts((double)gclip[b], sums[3 * b], sums[3 * b + 1], lin_weight, log_weight, n, c_lin, c_sq, c_log);
  float2 xv[kDistPerLane], yv[kDistPerLane];
#pragma unroll
  for (int j = 0; j < kDistPerLane; ++j) {
    const long long i = i0 + (long long)j * kDistThreads;
    const bool live = i < n;
    xv[j] = live ? xr[i] : make_float2(0.f, 0.f);
    yv[j] = live ? yr[i] : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < kDistPerLane; ++j) {
    const long long i = i0 + (long long)j * kDistThreads;
    if (i < n) {
      const float a = sd_abs(xv[j]), bm = sd_abs(yv[j]);
      const float d = a - bm;
      const float lg = dist_lg(d, c_log);
      const float lind = c_lin * d;
      if (NEED_X) xr[i] = dist_bin_grad(dist_d_generated(lind, lg, a, eps), a, xv[j]);
      if (NEED_Y) yr[i] = dist_bin_grad(dist_d_target(lind, lg, bm, c_sq, eps), bm, yv[j]);
    }
  }
}

}  // namespace at_hip

extern "C" {

size_t at_spectral_distance_workspace_bytes(int64_t B, int64_t n) { return at_hip::dist_workspace_bytes(B, n); }

int at_spectral_distance_sums(const float* X_complex, const float* Y_complex, int64_t B, int64_t n, float eps,
                              double* sums, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace at_hip;
  if (B < 0 || n < 1 || !(eps >= 0.f)) return AT_EINVAL;      // before B == 0, unlike at_mel_distance_sums
  if (B == 0) return AT_OK;
  if ((((uintptr_t)X_complex) & 7) || (((uintptr_t)Y_complex) & 7)) return AT_EINVAL;    // complex64 bins
  return dist_sums((const float2*)X_complex, (const float2*)Y_complex, B, n, eps, sums, workspace,
                                 workspace_bytes, (hipStream_t)stream);
}

int at_spectral_distance_backward(float* X_complex, float* Y_complex, int64_t B, int64_t n, const double* sums,
                                  const float* gclip, float lin_weight, float log_weight, float eps, int need_x,
                                  int need_y, void* stream) {
  using namespace at_hip;
  if (B < 0 || n < 1 || !(eps >= 0.f) || (!need_x && !need_y)) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!X_complex || !Y_complex || !sums || !gclip) return AT_EINVAL;
  if ((((uintptr_t)X_complex) & 7) || (((uintptr_t)Y_complex) & 7)) return AT_EINVAL;
  const long long slices = dist_slices(n), blocks = (long long)B * slices;
  if (blocks > 0x7fffffffLL) return AT_EUNSUPPORTED;
  auto run = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kDistThreads), 0, (hipStream_t)stream, (float2*)X_complex,
                       (float2*)Y_complex, (long long)n, slices, sums, gclip, lin_weight, log_weight, eps);
  };
  if (need_x && need_y) run(sd_backward_kernel<true, true>);
  else if (need_x) run(sd_backward_kernel<true, false>);
  else run(sd_backward_kernel<false, true>);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

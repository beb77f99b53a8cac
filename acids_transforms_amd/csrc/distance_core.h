// distance_core.h -- the distance of spectral_distance.hip (complex bins through a magnitude) and of mel_distance.hip
// (float mel cells as stored), stated once: the slice geometry, the per-clip sums with their launcher, the clip's
// constants and the per-cell derivatives of the backward (formulas: the two files' headers).
//
// Order of the sums.  ONE workgroup of kDistThreads lanes reduces one slice of kDistSlice cells: lane t adds cells t,
// t + 256, ... in that order in fp32, a wave folds by a fixed xor tree, lane 0 adds the four waves in order; a second
// kernel adds a clip's slices in order in double.  The grid is exactly B x ceil(n / kDistSlice) and there are no float
// atomics: a clip's bits are a function of n alone, and a NaN stays in its clip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"

namespace at_hip {

constexpr int kDistThreads = 256;
constexpr int kDistPerLane = 16;
constexpr int kDistSlice = kDistThreads * kDistPerLane;   // cells per slice (the tests' *_distance_cases.py restate it)

static inline long long dist_slices(long long n) { return (n + kDistSlice - 1) / kDistSlice; }

// Two magnitudes, and they stay two: the sums and the pointwise backward take sqrtf, the row kernels the bare hardware
// square root, as mag_abs of autograd.hip; one for both would change the bits of one of the two losses.
__device__ __forceinline__ float sd_abs(float2 v) { return sqrtf(fmaf(v.x, v.x, v.y * v.y)); }
__device__ __forceinline__ float md_abs(float2 v) { return __builtin_amdgcn_sqrtf(fmaf(v.x, v.x, v.y * v.y)); }

// the cell policy of the sums, by stored type: a complex bin is compared through its magnitude, a mel cell as stored
__device__ __forceinline__ float dist_value(float2 v) { return sd_abs(v); }
__device__ __forceinline__ float dist_value(float v) { return v; }

// ---- sums ---------------------------------------------------------------------------------------------------------------

// three sums over the workgroup: xor tree inside a wave, then the waves in order; valid in thread 0
template <int THREADS>
__device__ __forceinline__ void sd_block_fold(float& a, float& b, float& c) {
  __shared__ float part[THREADS / 64][3];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[w][0] = a; part[w][1] = b; part[w][2] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < THREADS / 64; ++i) {
      a += part[i][0]; b += part[i][1]; c += part[i][2];
    }
  }
}

// workgroup blk reduces slice blk % slices of clip blk / slices into partial[blk][3]
template <typename T>
__global__ __launch_bounds__(kDistThreads) void dist_slice_sums_kernel(const T* __restrict__ X, const T* __restrict__ Y,
                                                                        long long n, long long slices, float eps,
                                                                        float* __restrict__ partial) {
  const long long blk = blockIdx.x;
  const long long b = blk / slices;
  const long long i0 = (blk - b * slices) * kDistSlice + threadIdx.x;
  const T* xr = X + b * n;
  const T* yr = Y + b * n;
  float sd = 0.f, sb = 0.f, sl = 0.f;
  T xv[kDistPerLane], yv[kDistPerLane];
#pragma unroll
  for (int j = 0; j < kDistPerLane; ++j) {      // every load of the slice is issued before the first use
    const long long i = i0 + (long long)j * kDistThreads;
    const bool live = i < n;
    xv[j] = live ? xr[i] : T{};      // a dead lane reads a zero
    yv[j] = live ? yr[i] : T{};
  }
#pragma unroll
  for (int j = 0; j < kDistPerLane; ++j) {
    if (i0 + (long long)j * kDistThreads < n) {
      const float a = dist_value(xv[j]), bm = dist_value(yv[j]);
      const float d = a - bm;
      sd = fmaf(d, d, sd);
      sb = fmaf(bm, bm, sb);
      sl += fabsf(logf(a + eps) - logf(bm + eps));
    }
  }
  sd_block_fold<kDistThreads>(sd, sb, sl);
  if (threadIdx.x == 0) {
    float* dst = partial + 3 * blk;
    dst[0] = sd; dst[1] = sb; dst[2] = sl;
  }
}

// thread (b, k): sums[b][k] = the clip's partials k in slice order, in double
template <int THREADS>
__global__ __launch_bounds__(THREADS) void sd_clip_sums_kernel(const float* __restrict__ partial, long long B,
                                                                long long slices, double* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= 3 * B) return;
  const long long b = i / 3;
  const int k = (int)(i - 3 * b);
  const float* src = partial + 3 * b * slices + k;
  double s = 0.0;
  for (long long q = 0; q < slices; ++q) s += (double)src[3 * q];
  sums[i] = s;
}

// three floats per slice, whatever the cell
static inline size_t dist_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n < 1) return 0;
  return sizeof(float) * 3 * (size_t)B * (size_t)dist_slices(n);
}

// The two launches of at_spectral_distance_sums / at_mel_distance_sums behind the checks they share.  B > 0, n >= 1
// and eps are the entry's to check: the two entries answer B == 0 and a bad n or eps in different orders.
template <typename T>
static int dist_sums(const T* X, const T* Y, int64_t B, int64_t n, float eps, double* sums,
                     void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (!X || !Y || !sums) return AT_EINVAL;
  const long long slices = dist_slices(n), blocks = (long long)B * slices;
  if (blocks > 0x7fffffffLL) return AT_EUNSUPPORTED;
  if (!workspace || (((uintptr_t)workspace) & 3) || workspace_bytes < dist_workspace_bytes(B, n)) return AT_EWORKSPACE;
  hipLaunchKernelGGL(dist_slice_sums_kernel<T>, dim3((unsigned)blocks), dim3(kDistThreads), 0, s, X, Y, (long long)n,
                     slices, eps, (float*)workspace);
  hipLaunchKernelGGL(sd_clip_sums_kernel<kDistThreads>, dim3((unsigned)((3 * B + kDistThreads - 1) / kDistThreads)),
                     dim3(kDistThreads), 0, s, (const float*)workspace, (long long)B, slices, sums);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// ---- backward -----------------------------------------------------------------------------------------------------------

// The clip's constants, in double: S_B^2 of a loud clip leaves fp32's range.  n: the clip's cells, of any number type.
//     c_lin = g lin_weight 2 / S_B      c_sq = g lin_weight 2 S_D / S_B^2      c_log = g log_weight / n
// Written into the caller's three floats: md_backward_kernel holds them across the rows of a clip.
template <typename N>
__device__ __forceinline__ void dist_consts(double g, double s_d, double s_b, float lin_weight, float log_weight, N n,
                                            float& c_lin, float& c_sq, float& c_log) {
  const double inv_sb = 1.0 / s_b;
  const double lin2 = 2.0 * g * (double)lin_weight * inv_sb;
  c_lin = (float)lin2;
  c_sq = (float)(lin2 * s_d * inv_sb);
  c_log = (float)(g * (double)log_weight / (double)n);
}

// c_log sgn(d); NaN stays NaN
__device__ __forceinline__ float dist_lg(float d, float c_log) {
  return d > 0.f ? c_log : (d < 0.f ? -c_log : 0.f * d);
}

// The two derivatives of a cell, by its generated value a (dA) and by its target value bm (dBm).  Both take the two
// terms they share, lind = c_lin d and lg = dist_lg(d, c_log), from the kernel, which forms each once: which of the
// two products of dBm is fused into a multiply-add depends on whether lind has a second use.
__device__ __forceinline__ float dist_d_generated(float lind, float lg, float a, float eps) { return lind + lg / (a + eps); }
__device__ __forceinline__ float dist_d_target(float lind, float lg, float bm, float c_sq, float eps) {
  return -lind - c_sq * bm - lg / (bm + eps);
}

// the derivative dA of the loss by the magnitude a of the bin x -> the gradient of the bin; 0 where a == 0
__device__ __forceinline__ float2 dist_bin_grad(float dA, float a, const float2& x) {
  const float r = dA / a;
  return a == 0.f ? make_float2(0.f, 0.f) : make_float2(r * x.x, r * x.y);
}

}  // namespace at_hip

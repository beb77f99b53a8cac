// sd_fold.h -- what the per-clip sums of spectral_distance.hip and of mel_distance.hip share: the fold of three fp32
// sums over one workgroup, and the kernel that adds a clip's slice partials in double.  Both files cut a clip into
// slices of THREADS x 16 cells, reduce one slice per workgroup of THREADS lanes and hand the partials to
// sd_clip_sums_kernel: the order of a clip's sums is a function of its cell count alone.
#pragma once
#include <hip/hip_runtime.h>

namespace at_hip {

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

}  // namespace at_hip

// band_cols.h -- what the banded backward kernels share (mag_bwd_banded_kernel of autograd.hip, maginv_bwd_banded_kernel
// of invert_grad.hip, mfcc_bwd_kernel of mfcc_grad.hip): a bank as bands by column, its staging in LDS, the walk of one
// column, the row kept in registers, the LDS plan (band_plan.h) and the launch of a row plan (persistent_launch.h).
//
// A (K x N) bank by column (utils.banded.bank_columns): column j holds len[j] weights at w[off[j] ..] for the rows
// start[j] .. start[j] + len[j] - 1.  The transposed bank is the same tables of bank^T (K columns).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "band_plan.h"
#include "persistent_launch.h"

namespace at_hip {

struct BandCols {
  const int *start, *len, *off;   // n entries each
  const float* w;                 // nnz weights; null: no bank
  int n, nnz;
};

// floats of one bank's tables in LDS
inline long long band_cols_floats(const BandCols& c) { return 3LL * c.n + c.nnz; }

// ---- device side ------------------------------------------------------------------------------------------------------

// Copies c's tables to LDS at cur as start | len | off | w, the whole workgroup together, moves cur past them and returns
// the tables in LDS.  No barrier in here: the caller's first __syncthreads() before a walk publishes them.
__device__ __forceinline__ BandCols band_stage(const BandCols& c, float*& cur) {
  int* start = reinterpret_cast<int*>(cur);
  int *len = start + c.n, *off = len + c.n;
  float* w = reinterpret_cast<float*>(off + c.n);
  for (int i = threadIdx.x; i < c.n; i += blockDim.x) {
    start[i] = c.start[i];
    len[i] = c.len[i];
    off[i] = c.off[i];
  }
  for (int i = threadIdx.x; i < c.nnz; i += blockDim.x) w[i] = c.w[i];
  cur = w + c.nnz;
  return {start, len, off, w, c.n, c.nnz};
}

// sum_i w[i] v[start[j] + i] over column j in ascending i: every "bits do not depend on batch or grid" rests on that order
__device__ __forceinline__ float band_dot(const BandCols& c, int j, const float* v) {
  const int s = c.start[j], n = c.len[j];
  const float* w = c.w + c.off[j];
  float acc = 0.f;
#pragma unroll 4
  for (int i = 0; i < n; ++i) acc = fmaf(w[i], v[s + i], acc);
  return acc;
}

// The row's K <= 64 KIT elements in registers, element lane + 64 q in xv[q]: all loads are issued before any is used.
// Fully unrolled, so that xv never leaves the registers.  KIT == 0: nothing.
template <int KIT>
__device__ __forceinline__ void band_row_load(float2 (&xv)[KIT > 0 ? KIT : 1], const float2* row, int lane, int K) {
#pragma unroll
  for (int q = 0; q < KIT; ++q) {
    const int k = lane + 64 * q;
    if (k < K) xv[q] = row[k];
  }
}

// a real row, as (x, 0)
template <int KIT>
__device__ __forceinline__ void band_row_load(float2 (&xv)[KIT > 0 ? KIT : 1], const float* row, int lane, int K) {
#pragma unroll
  for (int q = 0; q < KIT; ++q) {
    const int k = lane + 64 * q;
    if (k < K) xv[q] = make_float2(row[k], 0.f);
  }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------

// persistent_launch of a one-wave-per-row kernel under the plan pl (the tables are staged once per workgroup): one work
// unit is a row group, the wpb rows of a workgroup
template <typename Kernel, typename... Args>
int band_launch_rows(Kernel kernel, const BandPlan& pl, long long rows, hipStream_t stream, Args... args) {
  return persistent_launch(kernel, 64 * pl.wpb, pl.lds, (rows + pl.wpb - 1) / pl.wpb, stream, args...);
}

}  // namespace at_hip

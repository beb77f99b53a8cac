// true_peak.hip -- the true-peak measure of ITU-R BS.1770-4 Annex 2 / EBU R128, generalised to any polyphase table:
//     y[P n + p] = sum over k = 0 .. K - 1 ascending of h[p][k] x[n - k],     0 <= n < L, 0 <= p < P,
//     peak = max over m of |y[m]|,   index = the smallest m that attains it,
// with x[n] for n < 0 taken from the K - 1 samples of state_in (oldest first), or zeros.  Causal, no flush past L - 1.
//
// ORDER RULE: every y[m] is ONE fmaf chain from +0 over k ascending, a function of the taps and of the row's samples alone
// (built with -ffp-contract=off: the chains are the fmaf that are written).  The reduction is exact: the maximum of the
// unsigned image of |y|'s bits -- every NaN mapped to ONE image above infinity's, so a NaN wins and the first one is
// kept -- paired with the smallest index.  That key is associative and commutative, so a row's bits depend neither on the
// batch, nor on the tile, nor on the grid, nor on how a stream was cut into chunks.  No float maximum, no atomics.
//
// Work: rows x tiles of kTpTile = 2048 samples on one 64-bit index, persistent workgroups of 256 lanes past the grid
// (persistent_launch.h): no limit on the rows, and one long row spreads over the chip.  A workgroup stages its tile and the
// K - 1 samples before it in LDS (coalesced; slot l + l / 32, so that the lanes' windows, 8 samples apart, fall on 32
// different banks), each lane takes kTpPerLane = 8 consecutive samples with their halo in registers and forms all P K
// products from that window.  The (4, 12) table runs a compiled copy, fully unrolled, its 48 taps uniform values read once
// (scalar registers); every other table a generic copy with the table in LDS and the window taken kTpChunk taps at a time.
// A row of one tile is finished by its workgroup (one launch); otherwise every tile leaves a 16-byte partial and a small
// second kernel joins a row's partials in tile order.
//
// Backward (the measure is piecewise linear: the subgradient at the attained maximum):
//     gx[n] = g sign(y[index]) h[p*][n* - n]   for 0 <= n* - n < K,  index = P n* + p*;   +0 elsewhere,
// one launch that writes every element, no memset, no atomics; a row whose sign is 0 (peak 0 or NaN) gets +0 by selection.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "persistent_launch.h"

namespace at_hip {

constexpr int kTpLanes = 256;
constexpr int kTpPerLane = 8;
constexpr int kTpTile = kTpLanes * kTpPerLane;           // 2048 samples
constexpr int kTpMaxPhases = 8;
constexpr int kTpMaxTaps = 64;                           // per phase
constexpr int kTpChunk = 8;                              // generic copy: taps per register window
constexpr unsigned kTpNanImage = 0x7f800001u;            // the one image of every NaN: just above infinity's
constexpr int kTpFinishLanes = 64;
constexpr int kTpBackwardSpan = 1024;                    // samples of a row per unit of the backward

struct TpPartial {                                       // what a tile leaves: 16 bytes
  unsigned bits;                                         // the image of |y| at the tile's maximum
  unsigned negative;                                     // 1 where that y was negative
  long long index;                                       // its index in the row's oversampled signal
};

struct TpOut {
  float* peak;                                           // (rows) this call's maximum, or null
  long long* index;                                      // (rows) offset + its index, or null
  float* sign;                                           // (rows) +1 / -1, 0 where the peak is 0 or NaN, or null
  float* max_peak;                                       // (rows) running maximum, read and updated, or null
  long long* max_index;                                  // (rows) its index, updated with it, or null
  long long offset;                                      // added to every index written
};

// LDS slot of logical sample l of a tile (l = 0 is the oldest halo sample)
__device__ __forceinline__ int tp_slot(int l) { return l + (l >> 5); }
constexpr int kTpSlots = kTpTile + kTpMaxTaps - 1 + ((kTpTile + kTpMaxTaps - 1) >> 5) + 1;

__device__ __forceinline__ unsigned tp_image(unsigned ybits) {
  const unsigned a = ybits & 0x7fffffffu;
  return a < kTpNanImage ? a : kTpNanImage;
}

// the row's result: written by the one lane that holds it
__device__ __forceinline__ void tp_write_row(const TpOut& o, long long row, unsigned bits, unsigned negative, long long index) {
  const bool nan = bits > 0x7f800000u;
  const float pk = __uint_as_float(nan ? 0x7fc00000u : bits);
  if (o.peak) o.peak[row] = pk;
  if (o.index) o.index[row] = o.offset + index;
  if (o.sign) o.sign[row] = (nan || bits == 0u) ? 0.0f : (negative ? -1.0f : 1.0f);
  if (o.max_peak) {
    const unsigned old = tp_image(__float_as_uint(o.max_peak[row]));
    if (bits > old) {                                    // a tie keeps the earlier index
      o.max_peak[row] = pk;
      if (o.max_index) o.max_index[row] = o.offset + index;
    }
  }
}

// (image, smallest local index, sign) as one 64-bit key: the maximum key is the result
__device__ __forceinline__ unsigned long long tp_key(unsigned bits, unsigned m, unsigned ybits) {
  return ((unsigned long long)bits << 32) | (unsigned long long)(((0x7fffffffu - m) << 1) | (ybits >> 31));
}

__device__ __forceinline__ unsigned long long tp_wave_max(unsigned long long key) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off, 64);
    key = other > key ? other : key;
  }
  return key;
}

// stages samples [start - (K - 1), start + kTpTile) of the row into LDS; past the row's end: zeros
__device__ __forceinline__ void tp_stage(const float* __restrict__ xr, const float* __restrict__ sr, long long L, int K,
                                         long long start, float* tile, int tid) {
  for (int i = tid; i < kTpTile + K - 1; i += kTpLanes) {
    const long long n = start - (K - 1) + i;
    float v = 0.0f;
    if (n >= 0) {
      if (n < L) v = xr[n];
    } else if (sr) {
      v = sr[(K - 1) + n];
    }
    tile[tp_slot(i)] = v;
  }
}

// the compiled copy: the whole window in registers, every loop unrolled, the taps uniform
template <int P, int K>
__device__ __forceinline__ unsigned long long tp_lane_fixed(const float (&h)[P * K], const float* tile, int tid, int nv) {
  float w[kTpPerLane + K - 1];
#pragma unroll
  for (int i = 0; i < kTpPerLane + K - 1; ++i) w[i] = tile[tp_slot(tid * kTpPerLane + i)];
  unsigned best = 0u, bestm = (unsigned)(tid * kTpPerLane * P), besty = 0u;
#pragma unroll
  for (int j = 0; j < kTpPerLane; ++j) {
    if (j < nv) {
#pragma unroll
      for (int p = 0; p < P; ++p) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) acc = fmaf(h[p * K + k], w[j + K - 1 - k], acc);
        const unsigned yb = __float_as_uint(acc), a = tp_image(yb);
        if (a > best) {                                  // ascending index: the first maximum stays
          best = a;
          bestm = (unsigned)((tid * kTpPerLane + j) * P + p);
          besty = yb;
        }
      }
    }
  }
  return tp_key(best, bestm, besty);
}

// the generic copy: the table in LDS, kTpChunk taps of the window at a time
__device__ __forceinline__ unsigned long long tp_lane_generic(const float* tab, int P, int K, const float* tile, int tid,
                                                              int nv) {
  unsigned long long key = tp_key(0u, (unsigned)(tid * kTpPerLane * P), 0u);
  for (int p = 0; p < P; ++p) {
    float acc[kTpPerLane];
#pragma unroll
    for (int j = 0; j < kTpPerLane; ++j) acc[j] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kTpChunk) {
      float v[kTpPerLane + kTpChunk - 1];
      const int base = tid * kTpPerLane + (K - 1) - k0 - (kTpChunk - 1);     // < 0 only where no tap reads it
#pragma unroll
      for (int i = 0; i < kTpPerLane + kTpChunk - 1; ++i) v[i] = base + i >= 0 ? tile[tp_slot(base + i)] : 0.0f;
#pragma unroll
      for (int kk = 0; kk < kTpChunk; ++kk) {
        if (k0 + kk < K) {                               // (uniform)
          const float hk = tab[p * K + k0 + kk];
#pragma unroll
          for (int j = 0; j < kTpPerLane; ++j) acc[j] = fmaf(hk, v[j + kTpChunk - 1 - kk], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kTpPerLane; ++j) {
      if (j < nv) {
        const unsigned yb = __float_as_uint(acc[j]);
        const unsigned long long cand = tp_key(tp_image(yb), (unsigned)((tid * kTpPerLane + j) * P + p), yb);
        key = cand > key ? cand : key;
      }
    }
  }
  return key;
}

// FP, FK > 0: the compiled copy of that table shape; 0, 0: the generic copy
template <int FP, int FK>
__global__ __launch_bounds__(kTpLanes) void true_peak_kernel(const float* __restrict__ x, long long rows, long long L,
                                                             const float* __restrict__ taps, int P, int K,
                                                             const float* __restrict__ state_in, float* __restrict__ state_out,
                                                             long long tiles, TpPartial* __restrict__ partial, TpOut out) {
  __shared__ float tile[kTpSlots];
  __shared__ float tab[FP > 0 ? 1 : kTpMaxPhases * kTpMaxTaps];
  __shared__ unsigned long long red[kTpLanes / 64];
  const int tid = threadIdx.x;
  float h[FP > 0 ? FP * FK : 1];
  if constexpr (FP > 0) {
#pragma unroll
    for (int i = 0; i < FP * FK; ++i) h[i] = taps[i];
  } else {
    for (int i = tid; i < P * K; i += kTpLanes) tab[i] = taps[i];
  }
  const long long units = rows * tiles;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long row = u / tiles, t = u - row * tiles, start = t * kTpTile;
    const float* xr = x + row * L;
    const float* sr = state_in ? state_in + row * (K - 1) : nullptr;
    tp_stage(xr, sr, L, K, start, tile, tid);
    if (state_out && t == tiles - 1 && tid < K - 1) {     // the last K - 1 samples of [state | chunk]
      const long long n = L - (K - 1) + tid;
      state_out[row * (K - 1) + tid] = n >= 0 ? xr[n] : (sr ? sr[L + tid] : 0.0f);
    }
    __syncthreads();
    const long long left = L - start;
    const int count = left < kTpTile ? (int)left : kTpTile;
    const int nv = count - tid * kTpPerLane;              // this lane's samples inside the row
    unsigned long long key;
    if constexpr (FP > 0) key = tp_lane_fixed<FP, FK>(h, tile, tid, nv);
    else key = tp_lane_generic(tab, P, K, tile, tid, nv);
    key = tp_wave_max(key);
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int wv = 1; wv < kTpLanes / 64; ++wv) key = red[wv] > key ? red[wv] : key;
      const unsigned bits = (unsigned)(key >> 32), low = (unsigned)key;
      const long long index = start * P + (long long)(0x7fffffffu - (low >> 1));
      if (tiles == 1) {
        tp_write_row(out, row, bits, low & 1u, index);
      } else {
        TpPartial r = {bits, low & 1u, index};
        partial[u] = r;
      }
    }
  }
}

// joins a row's partials: one wave per row, lane-strided in tile order, then across the lanes; (image, smallest index)
__global__ __launch_bounds__(kTpFinishLanes) void true_peak_finish_kernel(const TpPartial* __restrict__ partial, long long rows,
                                                                          long long tiles, TpOut out) {
  const int lane = threadIdx.x;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    unsigned bits = 0u, negative = 0u;
    long long index = INT64_MAX;
    for (long long t = lane; t < tiles; t += kTpFinishLanes) {
      const TpPartial r = partial[row * tiles + t];
      if (r.bits > bits || (r.bits == bits && r.index < index)) {
        bits = r.bits;
        negative = r.negative;
        index = r.index;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned ob = __shfl_xor(bits, off, 64), on = __shfl_xor(negative, off, 64);
      const long long oi = __shfl_xor(index, off, 64);
      if (ob > bits || (ob == bits && oi < index)) {
        bits = ob;
        negative = on;
        index = oi;
      }
    }
    if (lane == 0) tp_write_row(out, row, bits, negative, index);
  }
}

__global__ __launch_bounds__(kTpLanes) void true_peak_backward_kernel(const float* __restrict__ g, const float* __restrict__ sign,
                                                                      const long long* __restrict__ index,
                                                                      const float* __restrict__ taps, int P, int K,
                                                                      long long rows, long long L, long long spans,
                                                                      float* __restrict__ gx) {
  const long long units = rows * spans;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long row = u / spans, first = (u - row * spans) * kTpBackwardSpan;
    const float s = sign[row], gv = g[row];
    const long long idx = index[row];
    const bool live = s != 0.0f && idx >= 0;             // peak 0 or NaN: +0 by selection, whatever g is
    const long long nstar = live ? idx / P : -1;
    const int pstar = live ? (int)(idx - nstar * P) : 0;
    const float gs = s > 0.0f ? gv : -gv;
    for (int q = 0; q < kTpBackwardSpan / kTpLanes; ++q) {
      const long long n = first + q * kTpLanes + threadIdx.x;
      if (n < L) {
        const long long d = nstar - n;
        float v = 0.0f;
        if (live && d >= 0 && d < K) v = gs * taps[pstar * K + (int)d];
        gx[row * L + n] = v;
      }
    }
  }
}

static int tp_check(int64_t rows, int64_t L, int P, int K) {
  if (rows < 0 || L < 0 || P < 1 || P > kTpMaxPhases || K < 1 || K > kTpMaxTaps) return AT_EINVAL;
  if (rows > 0 && L > INT64_MAX / 16 / rows) return AT_EUNSUPPORTED;     // 64-bit byte offsets, P L in 63 bits
  return AT_OK;
}

static int64_t tp_tiles(int64_t L) { return (L + kTpTile - 1) / kTpTile; }

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_true_peak_plan(int64_t rows, int64_t L, int P, int K, int64_t* tile, int64_t* per_lane, int* launches, int* dispatch) {
  if (!tile || !per_lane || !launches || !dispatch) return AT_EINVAL;
  const int rc = tp_check(rows, L, P, K);
  if (rc != AT_OK) return rc;
  *tile = kTpTile;
  *per_lane = kTpPerLane;
  *launches = (rows == 0 || L == 0) ? 0 : (tp_tiles(L) == 1 ? 1 : 2);
  *dispatch = (P == 4 && K == 12) ? 0 : 1;
  return AT_OK;
}

size_t at_true_peak_workspace_bytes(int64_t rows, int64_t L, int P, int K) {
  if (tp_check(rows, L, P, K) != AT_OK || rows == 0 || tp_tiles(L) <= 1) return 0;
  return (size_t)rows * (size_t)tp_tiles(L) * sizeof(TpPartial);
}

int at_true_peak(const float* x, int64_t rows, int64_t L, const float* taps, int P, int K, const float* state_in,
                 float* state_out, float* peak, int64_t* index, float* sign, float* max_peak_io, int64_t* max_index_io,
                 int64_t index_offset, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = tp_check(rows, L, P, K);
  if (rc != AT_OK) return rc;
  if (rows == 0 || L == 0) return AT_OK;
  if (!x || !taps || (!peak && !max_peak_io) || (max_index_io && !max_peak_io)) return AT_EINVAL;
  if (state_out && (state_out == state_in || K == 1)) return AT_EINVAL;
  if (state_in && K == 1) return AT_EINVAL;
  if ((((uintptr_t)x | (uintptr_t)taps | (uintptr_t)state_in | (uintptr_t)state_out | (uintptr_t)peak | (uintptr_t)sign |
        (uintptr_t)max_peak_io) & 3) || (((uintptr_t)index | (uintptr_t)max_index_io) & 7))
    return AT_EINVAL;
  const int64_t tiles = tp_tiles(L);
  const size_t need = at_true_peak_workspace_bytes(rows, L, P, K);
  if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) return AT_EWORKSPACE;
  const TpOut out = {peak, (long long*)index, sign, max_peak_io, (long long*)max_index_io, (long long)index_offset};
  TpPartial* partial = (TpPartial*)workspace;
  int lrc;
  if (P == 4 && K == 12)
    lrc = persistent_launch(true_peak_kernel<4, 12>, kTpLanes, 0, (long long)(rows * tiles), (hipStream_t)stream, x,
                            (long long)rows, (long long)L, taps, P, K, state_in, state_out, (long long)tiles, partial, out);
  else
    lrc = persistent_launch(true_peak_kernel<0, 0>, kTpLanes, 0, (long long)(rows * tiles), (hipStream_t)stream, x,
                            (long long)rows, (long long)L, taps, P, K, state_in, state_out, (long long)tiles, partial, out);
  if (lrc != AT_OK || tiles == 1) return lrc;
  return persistent_launch(true_peak_finish_kernel, kTpFinishLanes, 0, (long long)rows, (hipStream_t)stream,
                           (const TpPartial*)partial, (long long)rows, (long long)tiles, out);
}

int at_true_peak_backward(const float* g, const float* sign, const int64_t* index, const float* taps, int P, int K,
                          int64_t rows, int64_t L, float* gx, void* stream) {
  const int rc = tp_check(rows, L, P, K);
  if (rc != AT_OK) return rc;
  if (rows == 0 || L == 0) return AT_OK;
  if (!g || !sign || !index || !taps || !gx) return AT_EINVAL;
  if ((((uintptr_t)g | (uintptr_t)sign | (uintptr_t)taps | (uintptr_t)gx) & 3) || ((uintptr_t)index & 7)) return AT_EINVAL;
  const int64_t spans = (L + kTpBackwardSpan - 1) / kTpBackwardSpan;
  return persistent_launch(true_peak_backward_kernel, kTpLanes, 0, (long long)(rows * spans), (hipStream_t)stream, g, sign,
                           (const long long*)index, taps, P, K, (long long)rows, (long long)L, (long long)spans, gx);
}

}  // extern "C"

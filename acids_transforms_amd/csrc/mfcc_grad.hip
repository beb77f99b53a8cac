// mfcc_grad.hip -- the backward of MFCC.forward from the spectrum on: |X|^power -> HTK bank -> (optional) ln, DCT ->
// Normalize, with the channel-major (B, C, T) gradient MFCC.forward's output has.  The STFT in front of it is
// differentiated by the STFT adjoint (autograd.hip); autograd.MfccFunction chains the two over chunks of clips.
//
// Forward, per frame (b, t), X the K = n_fft/2 + 1 bins of its spectrum, p = power (1 or 2):
//     a[k] = |X[k]|^p,   M[j] = sum_k fbank[k, j] a[k]                       (N = n_mels filters)
//     n_mfcc None:  y[j] = (M[j] - offset) / scale                            C = N channels
//     n_mfcc set:   y[c] = (sum_j ln(max(M[j], 1e-10)) dct[j, c] - offset) / scale     C = n_mfcc channels
// (the dct buffer carries the 10 / ln 10 of the dB scale).  Backward, dF (B, C, T) the upstream gradient:
//     n_mfcc None:  dM[j] = dF[b, j, t] / scale                               (no division without a Normalize)
//     n_mfcc set:   dlnM[j] = sum_c dct[j, c] dF[b, c, t] / scale,  dM[j] = dlnM[j] / M[j] where M[j] >= 1e-10, else 0
//                   (torch.clamp's mask: what an empty filter, or a silent frame, gets); M is recomputed from X
//     dA[k] = sum_j fbank[k, j] dM[j]                                          (the transposed bank's band tables)
//     p = 2: dX = 2 dA X;      p = 1: dX = dA X / |X|, 0 where X == 0 (torch's sgn)
// Nothing is recomputed from X on the n_mfcc None route except |X| for p = 1.
//
// Layout.  dF is channel-major: a lane that walks one frame's channels would read it with stride T.  A workgroup
// therefore takes a tile of kMfccTile consecutive frames of ONE clip, reads each channel's run of the tile contiguous in
// t (dividing by scale on the way), and writes it transposed into LDS: g[frame of the tile][channel], row stride C | 1
// (odd, so that the 32 frames of one channel fall on 32 different banks).  Then one wave per frame does the walks
// (band_cols.h): on the n_mfcc None route straight on the frame's row of g, with no barrier in between; on
// the n_mfcc route through two wave-private LDS rows (a, then dM) with a workgroup barrier after each.  The last tile of a
// clip is short when 32 does not divide T; a tile never spans two clips.
//
// Every dX element is produced by one lane, from its frame's row of X, its frame's column of dF and the tables alone,
// summed in table order: a clip's bits depend neither on the batch nor on how the caller cuts it into chunks, and a NaN
// stays in its frame.  dX may alias X: each lane reads the elements it owns (k = lane + 64 q) before it writes them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "autograd.h"

namespace at_hip {

constexpr int kMfccTile = 32;   // frames per tile (mfcc_grad_cases.py restates it)

__device__ __forceinline__ float mfcc_pow(float2 x, int power) {
  const float s = fmaf(x.x, x.x, x.y * x.y);
  return power == 2 ? s : __builtin_amdgcn_sqrtf(s);
}

__device__ __forceinline__ float2 mfcc_dx(float dA, float2 x, int power) {
  if (power == 2) {
    const float r = 2.0f * dA;
    return make_float2(r * x.x, r * x.y);
  }
  const float a = __builtin_amdgcn_sqrtf(fmaf(x.x, x.x, x.y * x.y));
  if (a == 0.f) return make_float2(0.f, 0.f);
  const float r = dA / a;
  return make_float2(r * x.x, r * x.y);
}

// TAB_LDS: the band tables (and the DCT matrix) are staged in LDS once per workgroup.  DCT: the n_mfcc route.
// KIT > 0: the frame's spectrum stays in registers from its load to the store (K <= 64 KIT).
template <bool TAB_LDS, bool DCT, int KIT>
__global__ void mfcc_bwd_kernel(MfccBwdParams p, int gs, int g_floats, int k_pad, int n_pad, int tab_floats,
                                long long tiles_per_clip, long long tiles) {
  extern __shared__ __attribute__((aligned(16))) float mf_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int K = p.K, N = p.N, C = p.C, power = p.power;
  BandCols f = p.f, t = p.t;
  const float* dct = p.dct_t;
  if (TAB_LDS) {
    float* cur = mf_lds;
    t = band_stage(p.t, cur);
    if (DCT) {
      f = band_stage(p.f, cur);
      for (int i = threadIdx.x; i < C * N; i += blockDim.x) cur[i] = p.dct_t[i];
      dct = cur;
    }
  }
  float* g = mf_lds + tab_floats;
  float* a = g + g_floats + (DCT ? wave * (k_pad + n_pad) : 0);   // DCT only
  float* dm = a + k_pad;
  const bool scaled = p.scale != nullptr;
  const float sc = scaled ? p.scale[0] : 1.0f;

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long b = tile / tiles_per_clip;
    const long long t0 = (tile - b * tiles_per_clip) * kMfccTile;
    const int nt = (p.T - t0 < kMfccTile) ? (int)(p.T - t0) : kMfccTile;
    // the tile of dF, transposed: 32 consecutive lanes read 32 consecutive frames of one channel
    const float* src = p.dF + b * C * p.T + t0;
    for (int i = threadIdx.x; i < C * kMfccTile; i += blockDim.x) {
      const int c = i / kMfccTile, fr = i % kMfccTile;
      if (fr < nt) {
        const float v = src[(long long)c * p.T + fr];
        g[fr * gs + c] = scaled ? v / sc : v;
      }
    }
    __syncthreads();   // (also the tables, the first time round)
    for (int f0 = 0; f0 < nt; f0 += wpb) {      // workgroup-uniform: every wave reaches the barriers
      const int fr = f0 + wave;
      const bool live = fr < nt;
      const long long row = b * p.T + t0 + fr;
      const float2* xr = p.X + row * K;
      float2* dxr = p.dX + row * K;
      const float* grow = g + fr * gs;
      float2 xv[KIT > 0 ? KIT : 1];
      if (live) band_row_load<KIT>(xv, xr, lane, K);
      if (DCT) {
        if (live) {
          if (KIT > 0) {
#pragma unroll
            for (int q = 0; q < KIT; ++q) {
              const int k = lane + 64 * q;
              if (k < K) a[k] = mfcc_pow(xv[q], power);
            }
          } else {
            for (int k = lane; k < K; k += 64) a[k] = mfcc_pow(xr[k], power);
          }
        }
        __syncthreads();
        if (live)
          for (int j = lane; j < N; j += 64) {
            const float M = band_dot(f, j, a);
            float dl = 0.f;
#pragma unroll 4
            for (int c = 0; c < C; ++c) dl = fmaf(dct[c * N + j], grow[c], dl);
            dm[j] = M >= 1e-10f ? dl / M : 0.f;
          }
        __syncthreads();
      }
      if (live) {
        const float* d = DCT ? dm : grow;
        if (KIT > 0) {
#pragma unroll
          for (int q = 0; q < KIT; ++q) {
            const int k = lane + 64 * q;
            if (k < K) dxr[k] = mfcc_dx(band_dot(t, k, d), xv[q], power);
          }
        } else {
          for (int k = lane; k < K; k += 64) {
            const float2 x = xr[k];          // read before the write: dX may alias X
            dxr[k] = mfcc_dx(band_dot(t, k, d), x, power);
          }
        }
      }
    }
    __syncthreads();   // the tile is restaged
  }
}

int launch_mfcc_backward(const MfccBwdParams& p, hipStream_t stream) {
  if (p.B == 0) return 0;
  const bool dct = p.dct_t != nullptr;
  const int gs = p.C | 1;
  const int g_floats = (kMfccTile * gs + 3) / 4 * 4;
  const int k_pad = pad64(p.K), n_pad = pad64(p.N);
  const size_t g_bytes = sizeof(float) * (size_t)g_floats;
  const size_t per_wave = dct ? sizeof(float) * (size_t)(k_pad + n_pad) : 0;
  if (g_bytes > kBandLdsBudget) return -2;
  // tables: the transposed bank's; the n_mfcc route adds the forward bank's and the DCT matrix
  const long long tab =
      band_tab_floats(band_cols_floats(p.t) + (dct ? band_cols_floats(p.f) + (long long)p.C * p.N : 0));
  const long long tiles_per_clip = (p.T + kMfccTile - 1) / kMfccTile, tiles = p.B * tiles_per_clip;
  auto run = [&](auto kernel, long long tab_floats) {   // four waves on a tile at a time
    return persistent_launch(kernel, 64 * 4, sizeof(float) * tab_floats + g_bytes + 4 * per_wave, tiles, stream, p, gs,
                             g_floats, k_pad, n_pad, (int)tab_floats, tiles_per_clip, tiles);
  };
  if (sizeof(float) * tab + g_bytes + 4 * per_wave <= kBandLdsBudget) {
    if (p.K <= 9 * 64)   // n_fft <= 1024
      return dct ? run(mfcc_bwd_kernel<true, true, 9>, tab) : run(mfcc_bwd_kernel<true, false, 9>, tab);
    return dct ? run(mfcc_bwd_kernel<true, true, 0>, tab) : run(mfcc_bwd_kernel<true, false, 0>, tab);
  }
  if (!dct) return run(mfcc_bwd_kernel<false, false, 0>, 0);
  if (g_bytes + 4 * per_wave > kBandLdsBudget) return -2;   // (n_fft 16384 with 128 mels and 40 coefficients: 136 KB)
  return run(mfcc_bwd_kernel<false, true, 0>, 0);
}

}  // namespace at_hip

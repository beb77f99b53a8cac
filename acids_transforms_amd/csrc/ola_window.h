// ola_window.h -- the overlap-add register window of the fused ISTFT kernels at n_fft = 2048 and 4096
// (istft2048_ola_kernel, istft4096_ola_kernel; n_fft = 512 adds frame pairs by lane parity, its own scheme).
//
// A wave walks consecutive frames of one clip.  A frame is 8 register slots of n_fft / 8 samples, a slot V float4 per
// lane (V = 1: 2048, V = 2: 4096); a hop is HS slots, so the R = 8 / HS frames that overlap a hop are summed in
// registers: after frame t has been added, block t of the padded signal (samples [t hop, (t + 1) hop)) is complete -- it
// is divided by the window envelope of the frames that exist around it (the 2^R x hop table of at_istft_envelope_table)
// and stored once.  Output sample s is padded sample s + n_fft / 2 (center = True trims n_fft / 2 at both ends): block c
// is output hop c - LEAD, LEAD = n_fft / 2 / hop.  A run of blocks [c0, c1) starts R - 1 frames early (warm-up) to have
// its first block complete.
#pragma once
#include <hip/hip_runtime.h>

#include "fft512.h"     // v2f
#include "run_plan.h"

namespace at_hip {

struct POla {
  const float2* X;       // (B*T, n_fft / 2 + 1) complex64, or null
  const float* mag;      // polar input
  const float* phase;
  const float* window;   // n_fft synthesis window samples
  const float* env;      // 2^R x hop
  const float2* tw;      // fft512 twiddle table
  const float2* tw_n;    // the size's own table (W2048^k; the n_fft-4096 block of the side table)
  float* y;              // (B, hop (T - 1))
  long long B, T, runs_per_clip, blocks_per_run;
};

// the clip b and the blocks [c0, c1) of wave `run`; false: the wave has nothing to do
__device__ __forceinline__ bool ola_run_blocks(const POla& p, long long run, int lead, long long& b, long long& c0,
                                               long long& c1) {
  b = run / p.runs_per_clip;
  if (b >= p.B) return false;
  const long long r = run - b * p.runs_per_clip;
  c0 = lead + r * p.blocks_per_run;                     // output hops q = 0 .. T - 2 are blocks c = q + lead
  c1 = c0 + p.blocks_per_run;
  if (c1 > lead + p.T - 1) c1 = lead + p.T - 1;
  return c0 < c1;
}

// the synthesis window with the transform's 1 / n_fft folded in, staged in LDS for the block's waves (n_fft / 4 float4;
// the caller's __syncthreads() follows): read from global memory per frame it was as many bytes through the
// vector-memory path as the spectrum row itself
template <int N, int THREADS>
__device__ __forceinline__ void stage_ola_window(const float* window, float4* wintab) {
  for (int i = threadIdx.x; i < N / 4; i += THREADS) {
    const float4 w = reinterpret_cast<const float4*>(window)[i];
    const float sc = 1.0f / N;
    wintab[i] = make_float4(w.x * sc, w.y * sc, w.z * sc, w.w * sc);
  }
}

template <int HS, int V>
struct OlaWindow {
  static constexpr int R = 8 / HS, FULL = (1 << R) - 1, HOP4 = 64 * V * HS;     // HOP4: float4 per hop
  float4 acc[8][V];
  float4 rcp_full[HS][V];

  // zero sums, and the reciprocal of the fully overlapped envelope: one division per wave instead of 4 V per hop
  // (<= 1 ulp from acc / e)
  __device__ __forceinline__ void init(const float4* env4, int lane) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < V; ++c) acc[j][c] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < HS; ++j)
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float4 e = env4[(size_t)FULL * HOP4 + V * (lane + 64 * j) + c];
        rcp_full[j][c] = make_float4(1.0f / e.x, 1.0f / e.y, 1.0f / e.z, 1.0f / e.w);
      }
  }

  // add one frame: y[2 c], y[2 c + 1] are the sub-transform outputs (two samples each) behind float4 c of a slot
  __device__ __forceinline__ void add_frame(const v2f (&y)[2 * V][8], const float4* wintab, int lane) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float4 w = wintab[V * (lane + 64 * j) + c];
        acc[j][c].x += y[2 * c][j].x * w.x;
        acc[j][c].y += y[2 * c][j].y * w.y;
        acc[j][c].z += y[2 * c + 1][j].x * w.z;
        acc[j][c].w += y[2 * c + 1][j].y * w.w;
      }
  }

  // which of the R frames that cover block t exist: bit q is frame t - (R - 1) + q, oldest first (at_istft_envelope_table)
  static __device__ __forceinline__ int frame_mask(long long t, long long T) {
    int mask = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const long long ft = t - (R - 1) + q;
      if (ft >= 0 && ft < T) mask |= 1 << q;
    }
    return mask;
  }

  // the completed block (slots 0 .. HS - 1) over its envelope, to dst.  A hop's value must not depend on how the launch
  // cut the clip into runs: every fully overlapped hop takes the reciprocal form, whichever run emits it
  __device__ __forceinline__ void emit(float* dst, const float4* env4, int mask, int lane) const {
    typedef float v4f __attribute__((ext_vector_type(4)));
    if (mask == FULL) {
#pragma unroll
      for (int j = 0; j < HS; ++j)
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const float4 a = acc[j][c], r = rcp_full[j][c];
          __builtin_nontemporal_store((v4f){a.x * r.x, a.y * r.y, a.z * r.z, a.w * r.w},
                                      reinterpret_cast<v4f*>(dst) + V * (lane + 64 * j) + c);
        }
    } else {
#pragma unroll
      for (int j = 0; j < HS; ++j)
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const float4 a = acc[j][c], e = env4[(size_t)mask * HOP4 + V * (lane + 64 * j) + c];
          reinterpret_cast<float4*>(dst)[V * (lane + 64 * j) + c] = make_float4(a.x / e.x, a.y / e.y, a.z / e.z, a.w / e.w);
        }
    }
  }

  // one hop on: the emitted slots leave, zeros enter
  __device__ __forceinline__ void slide() {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < V; ++c) acc[j][c] = (j + HS < 8) ? acc[j + HS][c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
};

// One launcher for both sizes: kernels[polar][log2 HS], HS = hop / (n_fft / 8) = 1, 2, 4; `waves` per block.
inline int launch_istft_ola(void (*const (&kernels)[2][3])(POla), int n_fft, int waves_per_block, const float2* X,
                            const float* mag, const float* phase, long long B, long long T, int hop, const float* window,
                            const float* env, const float2* tw, const float2* tw_n, float* y, hipStream_t stream) {
  if (B == 0 || T <= 1) return 0;
  const int slot = n_fft / 8;
  const int hs_log2 = hop == slot ? 0 : hop == 2 * slot ? 1 : hop == 4 * slot ? 2 : -1;
  if (hs_log2 < 0) return AT_EUNSUPPORTED;
  POla p = {X, mag, phase, window, env, tw, tw_n, y, B, T, 0, 0};
  const long long blocks = T - 1;                        // output hops per clip
  p.blocks_per_run = plan_ola_runs(B, blocks, 2048, 8);
  p.runs_per_clip = (blocks + p.blocks_per_run - 1) / p.blocks_per_run;
  const long long waves = B * p.runs_per_clip;
  const unsigned grid = (unsigned)((waves + waves_per_block - 1) / waves_per_block);
  hipLaunchKernelGGL(kernels[X == nullptr][hs_log2], dim3(grid), dim3(64 * waves_per_block), 0, stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // namespace at_hip

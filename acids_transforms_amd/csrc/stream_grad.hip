// stream_grad.hip -- what the backward passes of the streaming path (OverlapAdd, RealtimeSTFT, RealtimeDGT) need beyond
// autograd.hip: the per-frame FFT work is the irFFT / rFFT kernels that already exist, driven by capi.hip; here are the
// three small kernels around them.  N = n_fft, h = hop, keep = (N / h - 1) h.
//
//   * edge term of the frame-analysis adjoint (X[r] = rfft(w f[r]), reference stft.py:251, dgt.py:287):
//         q[r, m] = (N/2) w[m] irfft(G[r])[m] + w[m] (Re G[r,0] / 2 + Re G[r,N/2] (-1)^m / 2)      (Nyquist: even N only)
//     The first term is in `frames` already (the irFFT kernels on the window scaled by N/2); this kernel adds the second in
//     place with the fmaf(w[o], edge, frame) of autograd.hip's adj_dp, so both round alike.  No overlap-add follows.
//   * adjoint of OverlapAdd.forward (frames = a strided view of [history | chunk | zero pad], reference oadd.py:69-74):
//         gx[s, c] = sum_t gf[s, t, keep + c - t h]   over the frames t in [0, n) with 0 <= keep + c - t h < N,
//     t ascending, one thread per output sample (gather, no atomics).  The history's share is dropped (the carried state is
//     a constant of the graph) and a chunk sample that no frame covers gets exactly 0.
//   * adjoint of OverlapAdd.invert (out[s, p] = (tail[s, p] [p < keep] + sum_t f[s, t, p - t h]) / gain for
//     p < out_len = (n - 1) h + N - keep, reference oadd.py:90-104):
//         gf[s, t, o] = gy[s, t h + o] / gain   where t h + o < out_len, else 0
//     (the part of a frame that only reaches the new tail gets exactly 0).
// Each kernel moves 16 bytes per lane where hop, n_fft and the pointers allow it and gives the bits of its scalar form:
// the four samples of a lane see the same frames and every sum is taken in the same order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "autograd.h"

namespace at_hip {

// ---- edge term of the frame-analysis adjoint ---------------------------------------------------------------------------

// thread = VEC consecutive samples of one frame; VEC == 4 needs n_fft % 4 == 0 and 16-byte aligned frames and window
template <int VEC>
__global__ void rfft_adj_edge_kernel(float* frames, const float2* G, const float* w, long long rows, int n_fft) {
  const int N = n_fft, F = N / 2 + 1, per_row = N / VEC;
  const long long total = rows * per_row;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / per_row;
    const int o = (int)(e - r * per_row) * VEC;
    const float2* g = G + r * F;
    const float e0 = 0.5f * g[0].x;
    if (VEC == 4) {
      const float en = 0.5f * g[N / 2].x;             // n_fft % 4 == 0: even
      const float ep = e0 + en, em = e0 + -en;        // o even / odd (o is a multiple of 4)
      float4* dst = reinterpret_cast<float4*>(frames + r * N + o);
      const float4 wv = *reinterpret_cast<const float4*>(w + o);
      float4 fr = *dst;
      fr.x = fmaf(wv.x, ep, fr.x);
      fr.y = fmaf(wv.y, em, fr.y);
      fr.z = fmaf(wv.z, ep, fr.z);
      fr.w = fmaf(wv.w, em, fr.w);
      *dst = fr;
    } else {
      float edge = e0;
      if (!(N & 1)) edge += (o & 1) ? -0.5f * g[N / 2].x : 0.5f * g[N / 2].x;
      frames[r * N + o] = fmaf(w[o], edge, frames[r * N + o]);
    }
  }
}

int launch_rfft_adj_edge(float* frames, const float2* G, const float* window, long long rows, int n_fft,
                         hipStream_t stream) {
  if (rows <= 0) return 0;
  const bool vec4 = (n_fft % 4 == 0) && ((((uintptr_t)frames) | ((uintptr_t)window)) & 15) == 0;
  if (vec4)
    hipLaunchKernelGGL(rfft_adj_edge_kernel<4>, dim3(flat_grid(rows * (n_fft / 4))), dim3(256), 0, stream, frames, G,
                       window, rows, n_fft);
  else
    hipLaunchKernelGGL(rfft_adj_edge_kernel<1>, dim3(flat_grid(rows * n_fft)), dim3(256), 0, stream, frames, G, window,
                       rows, n_fft);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// ---- adjoint of OverlapAdd.forward --------------------------------------------------------------------------------------

struct OaddFwdAdjParams {
  const float* gf;   // (S, n, N)
  float* gx;         // (S, C)
  long long S, n, C;
  int n_fft, hop, keep;
};

// the frames that cover sample j of [history | chunk | pad], oldest first: t_lo .. t_hi (empty when t_lo > t_hi)
__device__ __forceinline__ void oadd_cover(const OaddFwdAdjParams& p, long long j, long long& t_lo, long long& t_hi) {
  t_hi = j / p.hop;
  if (t_hi > p.n - 1) t_hi = p.n - 1;
  t_lo = (j - p.n_fft + 1 <= 0) ? 0 : (j - p.n_fft + p.hop) / p.hop;   // ceil((j - N + 1) / h)
}

// grid: (chunk samples / (256 VEC) rounded up, streams); thread: samples c0 .. c0 + VEC - 1 of the streams blockIdx.y,
// blockIdx.y + gridDim.y, ...  VEC == 4: hop, n_fft and C multiples of 4 (keep is a multiple of hop), gf and gx 16-byte
// aligned -- the four samples then see the same frames
template <int VEC>
__global__ void oadd_forward_adj_kernel(OaddFwdAdjParams p) {
  const long long c0 = VEC * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
  if (c0 >= p.C) return;
  const int N = p.n_fft, h = p.hop;
  long long t_lo, t_hi;
  oadd_cover(p, p.keep + c0, t_lo, t_hi);
  for (long long s = blockIdx.y; s < p.S; s += gridDim.y) {
    const float* gf = p.gf + s * p.n * N;
    if (VEC == 4) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (long long t = t_lo; t <= t_hi; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(gf + t * N + (p.keep + c0 - t * h));
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
      *reinterpret_cast<float4*>(p.gx + s * p.C + c0) = acc;
    } else {
      float acc = 0.f;
      for (long long t = t_lo; t <= t_hi; ++t) acc += gf[t * N + (p.keep + c0 - t * h)];   // offset in [0, N)
      p.gx[s * p.C + c0] = acc;
    }
  }
}

int launch_oadd_forward_adj(const float* gframes, long long S, long long n, int n_fft, int hop, int keep, long long C,
                            float* gx, hipStream_t stream) {
  if (S <= 0 || C <= 0) return 0;
  OaddFwdAdjParams p = {gframes, gx, S, n, C, n_fft, hop, keep};
  const bool vec4 = (hop % 4 == 0) && (n_fft % 4 == 0) && (keep % 4 == 0) && (C % 4 == 0) &&
                    ((((uintptr_t)gframes) | ((uintptr_t)gx)) & 15) == 0;
  const unsigned gy = (unsigned)(S < 65535 ? S : 65535);
  if (vec4)
    hipLaunchKernelGGL(oadd_forward_adj_kernel<4>, dim3((unsigned)((C / 4 + 255) / 256), gy), dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(oadd_forward_adj_kernel<1>, dim3((unsigned)((C + 255) / 256), gy), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// ---- adjoint of OverlapAdd.invert ---------------------------------------------------------------------------------------

// grid: (samples of one stream's frames / (256 VEC) rounded up, streams); VEC == 4: hop and n_fft multiples of 4 (so are
// keep and out_len), gy and gf 16-byte aligned -- the four samples then lie on one side of out_len
template <int VEC>
__global__ void oadd_invert_adj_kernel(const float* gy, const float* gain, float* gf, long long S, long long n, int n_fft,
                                       int hop, long long out_len) {
  const long long e0 = VEC * ((long long)blockIdx.x * blockDim.x + threadIdx.x);   // t * N + o
  if (e0 >= n * n_fft) return;
  const long long t = e0 / n_fft;
  const long long pos = t * hop + (e0 - t * n_fft);
  const bool live = pos < out_len;
  const float g = *gain;
  for (long long s = blockIdx.y; s < S; s += gridDim.y) {
    float* dst = gf + s * n * n_fft + e0;
    if (VEC == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) {
        v = *reinterpret_cast<const float4*>(gy + s * out_len + pos);
        v = make_float4(v.x / g, v.y / g, v.z / g, v.w / g);
      }
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      *dst = live ? gy[s * out_len + pos] / g : 0.f;
    }
  }
}

int launch_oadd_invert_adj(const float* gy, long long S, long long n, int n_fft, int hop, int keep, const float* gain,
                           float* gframes, hipStream_t stream) {
  if (S <= 0 || n <= 0) return 0;
  const long long out_len = (n - 1) * hop + n_fft - keep, per_stream = n * n_fft;
  const bool vec4 = (hop % 4 == 0) && (n_fft % 4 == 0) && (keep % 4 == 0) &&
                    ((((uintptr_t)gy) | ((uintptr_t)gframes)) & 15) == 0;
  const unsigned grid_y = (unsigned)(S < 65535 ? S : 65535);
  if (vec4)
    hipLaunchKernelGGL(oadd_invert_adj_kernel<4>, dim3((unsigned)((per_stream / 4 + 255) / 256), grid_y), dim3(256), 0,
                       stream, gy, gain, gframes, S, n, n_fft, hop, out_len);
  else
    hipLaunchKernelGGL(oadd_invert_adj_kernel<1>, dim3((unsigned)((per_stream + 255) / 256), grid_y), dim3(256), 0, stream,
                       gy, gain, gframes, S, n, n_fft, hop, out_len);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // namespace at_hip

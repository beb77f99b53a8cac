// autograd.hip -- the backward passes of STFT / DGT (the adjoint of the centred, reflect-padded STFT) and of
// Magnitude (|.|, mel projection, contrast, Normalize), so that both can sit inside a training loss.
//
// Gradient convention (torch's, for a complex tensor): G = dL/dRe + i dL/dIm.
//
// STFT adjoint.  Forward, with P = n_fft // 2 and N = n_fft:
//     p = reflect_pad(x, P),   X[t, k] = sum_m w[m] p[t h + m] e^{-2 pi i k m / N},   k = 0 .. N/2
// (reference stft.py:98-104, torch.stft(center=True, pad_mode="reflect")).  Its adjoint:
//   * per frame   q[t, m] = w[m] Re sum_{k=0}^{N/2} G[t, k] e^{+2 pi i k m / N}   -- each bin counts ONCE.
//     That is N irfft(G') with the interior bins of G halved (even N: 1 .. N/2-1; odd N: 1 .. N/2), the imaginary parts
//     of DC and Nyquist dropped.  It is computed as irfft(G) times the window scaled by N/2 (the existing irfft kernels,
//     which already drop those imaginary parts), plus the halves of DC and Nyquist they miss:
//         q[t, m] = (N/2) w[m] irfft(G)[m] + w[m] (Re G[t,0] / 2 + Re G[t,N/2] (-1)^m / 2)   (Nyquist: even N only)
//   * overlap-add WITHOUT the ISTFT's envelope division:  dp[j] = sum_t q[t, j - t h]   (t ascending);
//   * reflect fold:  dx[i] = dp[i + P]  + dp[P - i]        for i in [1, P]
//                                       + dp[2L + P - 2 - i] for i in [L - P - 1, L - 2].
// Every output sample is summed by one thread in that fixed order (main term, left fold, right fold; frames ascending), so
// a clip's gradient bits do not depend on the batch it rides in or on how the clips are cut into chunks.
//
// Magnitude backward.  a = |X| (or |x| for real input), M = a @ mel_bank (M = a with mel=False),
// f = (c(M) - offset) / scale (reference spectral_repr.py:215-226):
//     dM    = dF / scale * c'(M)
//     c'    = 1 / (1 + M)                                      log1p
//           = 1 / M           where M >= eps, else 0           log   (torch.clamp's backward mask)
//           = 1 / (M ln 10)   where M >= eps, else 0           log10
//           = 1                                                none
//     dA[k] = sum_j mel_bank[k, j] dM[j]
//     dX    = dA X / |X|   (0 where X == 0: torch's sgn);   real input: dx = dA sign(x)
// M is recomputed from X (nothing is stored by the forward).  Both banks travel as bands (CSR by column): for column j of
// a (K x N) bank, start[j], len[j], off[j] and len[j] weights at w[off[j] ..]; the transposed bank is the same tables of
// mel_bank^T (513 "filters" of a few mels each at n_fft 1024).  keep_nyquist=False: dF has N - col_off columns, column c
// belongs to M column c + col_off, and the dropped columns get zero gradient.
//
// ISTFT adjoint.  Forward (torch.istft, center=True, onesided, length=None), with w the synthesis window, h the hop and
// T frames: P = N + h (T-1) padded samples, env[m] = sum of w[m - t h]^2 over the frames t covering m,
// y[i] = ola[i + N/2] / env[i + N/2] for i < Ly = h (T-1) + (N & 1).  Its adjoint, given gy:
//   * u[m] = gy[m - N/2] / env[m] for N/2 <= m < N/2 + Ly, 0 elsewhere (never divided in the padding: env may vanish there);
//   * gX[t, k] = (c_k / N) rfft(w u[t h .. t h + N))[k],  c_0 = c_{N/2} = 1 (even N), 2 for every other bin.
// Computed as the forward rFFT on the window scaled by 2/N, then DC (and Nyquist, even N) halved -- exact at every N.
// Polar input X = mag e^{i phi}: gmag = Re gX cos phi + Im gX sin phi (the phase is a constant: no gradient).
// Every size runs the same three steps, in chunks of clips: a prep kernel writes u (the envelope summed per sample from
// the oldest frame), the forward's rFFT kernels run with center = 0, and one kernel halves DC / Nyquist or writes gmag.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "autograd.h"

namespace at_hip {

// ---- STFT adjoint -----------------------------------------------------------------------------------------------------

__global__ void adj_window_kernel(const float* w, int n, float s, float* out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = w[i] * s;
}

struct AdjOlaParams {
  const float* frames;   // (B, T, N): (N/2) w[m] irfft(G[t])[m]
  const float2* G;       // (B, T, N/2 + 1)
  const float* window;   // N floats, unscaled
  float* dx;             // (B, L)
  long long B, T, L;
  int n_fft, hop;
};

// dp[j] of clip b: the frames that cover padded sample j, oldest first
__device__ __forceinline__ float adj_dp(const AdjOlaParams& p, long long b, long long j) {
  const int N = p.n_fft, h = p.hop, F = N / 2 + 1;
  long long t_hi = j / h;
  if (t_hi > p.T - 1) t_hi = p.T - 1;
  const long long t_lo = (j - N + 1 <= 0) ? 0 : (j - N + h) / h;   // ceil((j - N + 1) / h)
  float acc = 0.f;
  for (long long t = t_lo; t <= t_hi; ++t) {
    const int o = (int)(j - t * h);                                   // in [0, N) by the bounds above
    const long long f = b * p.T + t;
    const float2* g = p.G + f * F;
    float edge = 0.5f * g[0].x;
    if (!(N & 1)) edge += (o & 1) ? -0.5f * g[N / 2].x : 0.5f * g[N / 2].x;
    acc += fmaf(p.window[o], edge, p.frames[f * N + o]);
  }
  return acc;
}

// four consecutive padded samples j .. j+3 (j, hop and n_fft multiples of 4): they see the same frames, and every lane
// sums in the order of adj_dp, so the bits are those of four adj_dp calls
__device__ __forceinline__ float4 adj_dp4(const AdjOlaParams& p, long long b, long long j) {
  const int N = p.n_fft, h = p.hop, F = N / 2 + 1;
  long long t_hi = j / h;
  if (t_hi > p.T - 1) t_hi = p.T - 1;
  const long long t_lo = (j - N + 1 <= 0) ? 0 : (j - N + h) / h;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long t = t_lo; t <= t_hi; ++t) {
    const int o = (int)(j - t * h);
    const long long f = b * p.T + t;
    const float2* g = p.G + f * F;
    const float e0 = 0.5f * g[0].x, en = 0.5f * g[N / 2].x;
    const float ep = e0 + en, em = e0 + -en;        // o even / odd (o is a multiple of 4)
    const float4 fr = *reinterpret_cast<const float4*>(p.frames + f * N + o);
    const float4 w = *reinterpret_cast<const float4*>(p.window + o);
    acc.x += fmaf(w.x, ep, fr.x);
    acc.y += fmaf(w.y, em, fr.y);
    acc.z += fmaf(w.z, ep, fr.z);
    acc.w += fmaf(w.w, em, fr.w);
  }
  return acc;
}

// grid: (samples / 1024 rounded up, clips); thread: samples s0 .. s0+3 of clip blockIdx.y (+ multiples of gridDim.y)
__global__ void adj_ola_fold_kernel(AdjOlaParams p, int vec4) {
  const long long P = p.n_fft / 2, L = p.L;
  const long long s0 = 4 * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
  if (s0 >= L) return;
  for (long long b = blockIdx.y; b < p.B; b += gridDim.y) {
    float* dst = p.dx + b * L;
    if (vec4 && s0 > P && s0 + 3 < L - P - 1) {       // no fold touches these four samples
      const float4 v = adj_dp4(p, b, s0 + P);
      dst[s0] = v.x;
      dst[s0 + 1] = v.y;
      dst[s0 + 2] = v.z;
      dst[s0 + 3] = v.w;
      continue;
    }
    for (long long s = s0; s < s0 + 4 && s < L; ++s) {
      float v = adj_dp(p, b, s + P);
      if (s >= 1 && s <= P) v += adj_dp(p, b, P - s);
      if (s >= L - P - 1 && s <= L - 2) v += adj_dp(p, b, 2 * L + P - 2 - s);
      dst[s] = v;
    }
  }
}

int launch_adj_window(const float* w, int n_fft, float scale, float* out, hipStream_t stream) {
  const int blocks = (n_fft + 255) / 256;
  hipLaunchKernelGGL(adj_window_kernel, dim3(blocks), dim3(256), 0, stream, w, n_fft, scale, out);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int launch_adj_ola_fold(const float* frames, const float2* G, const float* window, float* dx, long long B, long long T,
                        long long L, int n_fft, int hop, hipStream_t stream) {
  if (B <= 0 || L <= 0) return 0;
  AdjOlaParams p = {frames, G, window, dx, B, T, L, n_fft, hop};
  const int vec4 = (hop % 4 == 0) && (n_fft % 8 == 0) && (((uintptr_t)frames) & 15) == 0 && (((uintptr_t)window) & 15) == 0;
  const long long bx = (L + 1023) / 1024;
  hipLaunchKernelGGL(adj_ola_fold_kernel, dim3((unsigned)bx, (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, stream, p,
                     vec4);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// ---- ISTFT adjoint ----------------------------------------------------------------------------------------------------

// gmag of one bin: Re(g e^{-i phi}), spelled out so that both paths round alike
__device__ __forceinline__ float adj_polar(float2 g, float phi) {
  float s, c;
  sincosf(phi, &s, &c);
  return fmaf(g.x, c, __fmul_rn(g.y, s));
}

// u of the ISTFT adjoint: thread = padded sample m of the clips blockIdx.y, blockIdx.y + gridDim.y, ... (gridDim.y is
// at most kPrepClipRows, so the envelope of m is summed once for many clips)
constexpr int kPrepClipRows = 8;

__global__ void istft_adj_prep_kernel(const float* gy, const float* w, float* u, long long B, long long T, long long Ly,
                                      long long P, int n_fft, int hop) {
  const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= P) return;
  const long long i = m - n_fft / 2;
  const bool live = i >= 0 && i < Ly;
  float env = 0.f;
  if (live) {
    long long t_hi = m / hop;
    if (t_hi > T - 1) t_hi = T - 1;
    const long long t_lo = (m - n_fft + 1 <= 0) ? 0 : (m - n_fft + hop) / hop;   // ceil((m - n_fft + 1) / hop)
    for (long long t = t_lo; t <= t_hi; ++t) {
#pragma clang fp contract(off)   // w^2 rounded before the add (as STFT._make_env16 sums it): no fma
      const float v = w[m - t * hop];
      env = env + v * v;
    }
  }
  for (long long b = blockIdx.y; b < B; b += gridDim.y) u[b * P + m] = live ? gy[b * Ly + i] / env : 0.f;
}

// complex output: DC and Nyquist (even N) halved in place, one thread per frame
__global__ void istft_adj_halve_kernel(float2* gX, long long rows, int F, int nyq) {
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
    float2* row = gX + r * F;
    row[0] = make_float2(0.5f * row[0].x, 0.5f * row[0].y);
    if (nyq > 0) row[nyq] = make_float2(0.5f * row[nyq].x, 0.5f * row[nyq].y);
  }
}

// polar output: gmag from the rFFT rows (DC and Nyquist halved on the way)
__global__ void istft_adj_polar_kernel(const float2* gX, const float* phase, float* gmag, long long rows, int F, int nyq) {
  const long long total = rows * F;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(e % F);
    float2 g = gX[e];
    if (k == 0 || k == nyq) g = make_float2(0.5f * g.x, 0.5f * g.y);
    gmag[e] = adj_polar(g, phase[e]);
  }
}

int launch_istft_adj_prep(const float* gy, const float* window, float* u, long long B, long long T, int n_fft, int hop,
                          hipStream_t stream) {
  const long long P = n_fft + (long long)hop * (T - 1), Ly = (long long)hop * (T - 1) + (n_fft & 1);
  if (B <= 0 || P <= 0) return 0;
  hipLaunchKernelGGL(istft_adj_prep_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)(B < kPrepClipRows ? B : kPrepClipRows)), dim3(256),
                     0, stream, gy, window, u, B, T, Ly, P, n_fft, hop);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int launch_istft_adj_finish(const float2* gX, const float* phase, void* out, long long rows, int n_fft, hipStream_t stream) {
  if (rows <= 0) return 0;
  const int F = n_fft / 2 + 1, nyq = (n_fft & 1) ? -1 : n_fft / 2;
  if (phase) {
    hipLaunchKernelGGL(istft_adj_polar_kernel, dim3(flat_grid(rows * F)), dim3(256), 0, stream, gX, phase,
                       (float*)out, rows, F, nyq);
  } else {
    hipLaunchKernelGGL(istft_adj_halve_kernel, dim3(flat_grid(rows)), dim3(256), 0, stream, (float2*)out, rows, F, nyq);
  }
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// ---- Magnitude backward -----------------------------------------------------------------------------------------------

__device__ __forceinline__ float mag_cprime(float M, int contrast, float eps) {
  switch (contrast) {
    case 1: return 1.0f / (1.0f + M);
    case 2: return M >= eps ? 1.0f / M : 0.0f;
    case 3: return M >= eps ? 1.0f / (M * 2.30258509299404568402f) : 0.0f;
    default: return 1.0f;
  }
}

// dA at element e of the input -> the input's gradient (sgn of the input x, loaded by the caller; plus the optional
// incoming gradient).  Real input: x.y == 0.
__device__ __forceinline__ void mag_put_x(const MagBwdParams& p, long long e, float dA, float2 x) {
  if (p.a_kind == 0) {
    const float a = __builtin_amdgcn_sqrtf(fmaf(x.x, x.x, x.y * x.y));
    float2 g = make_float2(0.f, 0.f);
    if (a > 0.f) {
      const float r = dA / a;
      g = make_float2(r * x.x, r * x.y);
    }
    if (p.dX_in) {
      const float2 d = reinterpret_cast<const float2*>(p.dX_in)[e];
      g.x += d.x;
      g.y += d.y;
    }
    reinterpret_cast<float2*>(p.dX)[e] = g;
  } else {
    float g = x.x > 0.f ? dA : (x.x < 0.f ? -dA : 0.f);
    if (p.dX_in) g += reinterpret_cast<const float*>(p.dX_in)[e];
    reinterpret_cast<float*>(p.dX)[e] = g;
  }
}

__device__ __forceinline__ void mag_put(const MagBwdParams& p, long long e, float dA) {
  const float2 x = p.a_kind == 0 ? reinterpret_cast<const float2*>(p.A)[e]
                                 : make_float2(reinterpret_cast<const float*>(p.A)[e], 0.f);
  mag_put_x(p, e, dA, x);
}

__device__ __forceinline__ float mag_abs(const MagBwdParams& p, long long e) {
  if (p.a_kind == 0) {
    const float2 x = reinterpret_cast<const float2*>(p.A)[e];
    return __builtin_amdgcn_sqrtf(fmaf(x.x, x.x, x.y * x.y));
  }
  return fabsf(reinterpret_cast<const float*>(p.A)[e]);
}

__device__ __forceinline__ float mag_dm(const MagBwdParams& p, long long row, int j, float M) {
  const int n_out = p.N - p.col_off;
  if (j < p.col_off) return 0.f;
  const float g = p.dF[row * n_out + (j - p.col_off)];
  const float gs = p.scale ? g / p.scale[0] : g;
  return gs * mag_cprime(M, p.contrast, p.eps);
}

// mel=False: one thread per element
__global__ void mag_bwd_pointwise_kernel(MagBwdParams p) {
  const long long total = p.rows * p.K;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / p.K;
    const int k = (int)(e - row * p.K);
    mag_put(p, e, mag_dm(p, row, k, mag_abs(p, e)));
  }
}

// banks: one wave per row, |X| and dM of the row in the wave's LDS slice; the loop over row groups is workgroup-uniform
// so that every wave reaches the barriers.  TAB_LDS: both banks' tables are staged in LDS once per workgroup (the walks'
// loads are serially dependent: from global memory each one would cost a round trip to L2); the first barrier of the
// row loop publishes them.  KIT > 0: the row's input stays in registers from the first phase to the last.
template <bool TAB_LDS, int KIT>
__global__ void mag_bwd_banded_kernel(MagBwdParams p, int k_pad, int n_pad, int tab_floats) {
  extern __shared__ float mb_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int K = p.K, N = p.N;
  BandCols f = p.f, t = p.t;
  if (TAB_LDS) {
    float* cur = mb_lds;
    t = band_stage(p.t, cur);
    f = band_stage(p.f, cur);
  }
  float* a = mb_lds + (TAB_LDS ? tab_floats : 0) + wave * (k_pad + n_pad);
  float* dm = a + k_pad;
  for (long long r0 = (long long)blockIdx.x * wpb; r0 < p.rows; r0 += (long long)gridDim.x * wpb) {
    const long long row = r0 + wave;
    const bool live = row < p.rows;
    float2 xv[KIT > 0 ? KIT : 1];
    if (live) {
      if (KIT > 0) {
        if (p.a_kind == 0)
          band_row_load<KIT>(xv, reinterpret_cast<const float2*>(p.A) + row * K, lane, K);
        else
          band_row_load<KIT>(xv, reinterpret_cast<const float*>(p.A) + row * K, lane, K);
#pragma unroll
        for (int q = 0; q < KIT; ++q) {
          const int k = lane + 64 * q;
          if (k < K) a[k] = __builtin_amdgcn_sqrtf(fmaf(xv[q].x, xv[q].x, xv[q].y * xv[q].y));
        }
      } else {
        for (int k = lane; k < K; k += 64) a[k] = mag_abs(p, row * K + k);
      }
    }
    __syncthreads();
    if (live)
      for (int j = lane; j < N; j += 64) dm[j] = mag_dm(p, row, j, band_dot(f, j, a));
    __syncthreads();
    if (live) {
      if (KIT > 0) {
#pragma unroll
        for (int q = 0; q < KIT; ++q) {
          const int k = lane + 64 * q;
          if (k < K) mag_put_x(p, row * K + k, band_dot(t, k, dm), xv[q]);
        }
      } else {
        for (int k = lane; k < K; k += 64) mag_put(p, row * K + k, band_dot(t, k, dm));
      }
    }
    __syncthreads();
  }
}

int launch_magnitude_backward(const MagBwdParams& p, hipStream_t stream) {
  if (p.rows == 0) return 0;
  if (!p.f.w) {
    hipLaunchKernelGGL(mag_bwd_pointwise_kernel, dim3(flat_grid(p.rows * p.K)), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
  }
  const int k_pad = pad64(p.K), n_pad = pad64(p.N);
  const size_t per_wave = sizeof(float) * (size_t)(k_pad + n_pad);
  const BandPlan pl = band_plan(band_tab_floats(band_cols_floats(p.t) + band_cols_floats(p.f)), per_wave);
  if (!pl.ok) return AT_EUNSUPPORTED;
  auto run = [&](auto kernel) { return band_launch_rows(kernel, pl, p.rows, stream, p, k_pad, n_pad, (int)pl.tab_floats); };
  if (!pl.tab_lds) return run(mag_bwd_banded_kernel<false, 0>);
  return p.K <= kBandKit * 64 ? run(mag_bwd_banded_kernel<true, kBandKit>) : run(mag_bwd_banded_kernel<true, 0>);
}

}  // namespace at_hip

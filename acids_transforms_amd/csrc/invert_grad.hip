// invert_grad.hip -- the backward passes of the representations' invert: Magnitude.invert (and the one-pass Polar.invert),
// polar_to_complex and the one-pass Cartesian.invert, so that a decoder that emits these representations can be trained
// against an audio loss (the ISTFT adjoint of autograd.hip takes it from there).
//
// Gradient convention (torch's, for a complex tensor and a real loss): gX = dL/dRe + i dL/dIm.
//
// Magnitude.invert (reference spectral_repr.py:229-240): z = y * scale + offset (z = y without Normalize), x = c(z) @ W
// with W the (K x N) inverse bank and c the inverse contrast (exp(z) - 1, exp(z) - eps, 10^z, z).  Given g (N per row):
//     dy[k] = scale * c'(z[k]) * sum_n W[k, n] g[n],    c' = exp(z) (log1p, log), ln 10 * 10^z (log10), 1 (none)
// keep_nyquist=False (pad_last): the reference de-normalises, pads a zero as the LAST of the K columns, then inverts the
// contrast, so y and dy have K - 1 columns and the padded column's gradient is dropped.  mel=False: W = I.
// The sum walks column k of W^T (the by-column tables of the transposed inverse bank: a band of outputs n per input k),
// one lane per k, in ascending n: a row's bits do not depend on the batch or on the grid.
//
// Polar.invert in one pass (ops.polar_inverse; reference :441-452 over :229-240): y (rows, 2, F) stacked,
// X[n] = M[n] e^{i phi[n]}, M = c(z) @ W, phi = y_phase * ps + po.  Given gX:
//     gM[n]       = Re gX cos phi + Im gX sin phi
//     dy_phase[n] = ps * M[n] * (Im gX cos phi - Re gX sin phi)          (M recomputed: a forward walk over W's columns)
//     dy_mag[k]   = the formula above with g = gM
//
// polar_to_complex (reference :449-451), X = mag e^{i phase}:  gmag = Re gX cos + Im gX sin,  gphase = mag (Im gX cos - Re gX sin).
// Cartesian.invert (reference :497-508), X = (y_re s_re + o_re) + i (y_im s_im + o_im):  dy_re = Re gX s_re, dy_im = Im gX s_im.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "autograd.h"
#include "mel_gemm.h"

namespace at_hip {

__device__ __forceinline__ float maginv_z(float y, bool norm, float sc, float off) {
  return norm ? __fadd_rn(__fmul_rn(y, sc), off) : y;       // as the forward's prologue rounds it
}

__device__ __forceinline__ float maginv_cprime(float z, int contrast) {
  switch (contrast) {
    case C_LOG1P:
    case C_LOG: return expf(z);
    case C_LOG10: return 2.30258509299404568402f * powf(10.0f, z);
    default: return 1.0f;
  }
}

// dy of one input from the walked sum
__device__ __forceinline__ float maginv_dy(float acc, float cp, bool norm, float sc) {
  const float v = acc * cp;
  return norm ? v * sc : v;
}

// mel=False: one thread per element of y (k_in = K - pad_last columns; g has K)
__global__ void maginv_bwd_pointwise_kernel(MagInvBwdParams p) {
  const int k_in = p.K - p.pad_last;
  const long long total = p.rows * k_in;
  const bool norm = p.scale != nullptr;
  const float sc = norm ? p.scale[0] : 1.f, off = norm ? p.offset[0] : 0.f;
  const float* g = reinterpret_cast<const float*>(p.g);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / k_in;
    const int k = (int)(e - row * k_in);
    const float z = maginv_z(p.y[row * p.ld_y + k], norm, sc, off);
    p.dy[row * p.ld_y + k] = maginv_dy(g[row * p.N + k],maginv_cprime(z, p.contrast), norm, sc);
  }
}

// banks: one wave per row; the wave's LDS slice holds g (N floats) -- in the polar form gM, next to c(z) and c'(z) (K
// floats each).  The loop over row groups is workgroup-uniform so that every wave reaches the barriers.  TAB_LDS: the
// tables are staged in LDS once per workgroup (the walks' loads are serially dependent); the first barrier of the row
// loop publishes them.
template <bool TAB_LDS, bool POLAR>
__global__ void maginv_bwd_banded_kernel(MagInvBwdParams p, int k_pad, int n_pad, int tab_floats) {
  extern __shared__ __attribute__((aligned(16))) float mi_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int K = p.K, N = p.N, k_in = p.K - p.pad_last;
  BandCols f = p.f, t = p.t;
  if (TAB_LDS) {
    float* cur = mi_lds;
    t = band_stage(p.t, cur);
    if (POLAR) f = band_stage(p.f, cur);
  }
  const int per_wave = POLAR ? n_pad + 2 * k_pad : n_pad;
  float* gl = mi_lds + (TAB_LDS ? tab_floats : 0) + wave * per_wave;
  float* cz = gl + n_pad;       // POLAR only
  float* cp = cz + k_pad;       // POLAR only
  const bool norm = p.scale != nullptr;
  const float sc = norm ? p.scale[0] : 1.f, off = norm ? p.offset[0] : 0.f;
  const bool pnorm = POLAR && p.ph_scale != nullptr;
  const float ps = pnorm ? p.ph_scale[0] : 1.f, po = pnorm ? p.ph_offset[0] : 0.f;
  for (long long r0 = (long long)blockIdx.x * wpb; r0 < p.rows; r0 += (long long)gridDim.x * wpb) {
    const long long row = r0 + wave;
    const bool live = row < p.rows;
    const float* y = p.y + row * p.ld_y;
    float* dy = p.dy + row * p.ld_y;
    if (live) {
      if (POLAR) {
        for (int k = lane; k < K; k += 64) {
          const float z = maginv_z(y[k], norm, sc, off);
          cz[k] = banded_contrast_inv(z, p.contrast, p.eps);
          cp[k] = maginv_cprime(z, p.contrast);
        }
      } else {
        const float* g = reinterpret_cast<const float*>(p.g) + row * N;
        for (int n = lane; n < N; n += 64) gl[n] = g[n];
      }
    }
    __syncthreads();
    if (POLAR) {
      if (live) {
        const float2* g = reinterpret_cast<const float2*>(p.g) + row * N;
        for (int n = lane; n < N; n += 64) {
          const float2 gx = g[n];
          const float phi = maginv_z(y[N + n], pnorm, ps, po);
          const float M = band_dot(f, n, cz);
          float sn, cs;
          sincosf(phi, &sn, &cs);
          gl[n] = fmaf(gx.x, cs, __fmul_rn(gx.y, sn));
          const float d = M * fmaf(gx.y, cs, -__fmul_rn(gx.x, sn));
          dy[N + n] = pnorm ? d * ps : d;
        }
      }
      __syncthreads();
    }
    if (live)
      for (int k = lane; k < k_in; k += 64) {
        const float acc = band_dot(t, k, gl);
        const float c = POLAR ? cp[k] : maginv_cprime(maginv_z(y[k], norm, sc, off), p.contrast);
        dy[k] = maginv_dy(acc, c, norm, sc);
      }
    __syncthreads();
  }
}

template <bool POLAR>
static int launch_maginv_form(const MagInvBwdParams& p, hipStream_t stream) {
  const int k_pad = pad64(p.K), n_pad = pad64(p.N);
  const size_t per_wave = sizeof(float) * (size_t)(POLAR ? n_pad + 2 * k_pad : n_pad);
  // tables: the transposed bank's and, polar, the bank's
  const BandPlan pl = band_plan(band_tab_floats(band_cols_floats(p.t) + (POLAR ? band_cols_floats(p.f) : 0)), per_wave);
  if (!pl.ok) return AT_EUNSUPPORTED;
  auto run = [&](auto kernel) { return band_launch_rows(kernel, pl, p.rows, stream, p, k_pad, n_pad, (int)pl.tab_floats); };
  return pl.tab_lds ? run(maginv_bwd_banded_kernel<true, POLAR>) : run(maginv_bwd_banded_kernel<false, POLAR>);
}

int launch_magnitude_invert_backward(const MagInvBwdParams& p, hipStream_t stream) {
  if (p.rows == 0) return 0;
  if (!p.t.w) {
    const long long total = p.rows * (p.K - p.pad_last);
    if (total < 1) return 0;
    hipLaunchKernelGGL(maginv_bwd_pointwise_kernel, dim3(flat_grid(total)), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
  }
  return p.polar ? launch_maginv_form<true>(p, stream) : launch_maginv_form<false>(p, stream);
}

// ---- polar_to_complex and Cartesian.invert ------------------------------------------------------------------------------

__global__ void polar_to_complex_bwd_kernel(const float2* gX, const float* mag, const float* phase, long long n,
                                            float* gmag, float* gphase) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const float2 g = gX[e];
    float sn, cs;
    sincosf(phase[e], &sn, &cs);
    if (gmag) gmag[e] = fmaf(g.x, cs, __fmul_rn(g.y, sn));
    if (gphase) gphase[e] = mag[e] * fmaf(g.y, cs, -__fmul_rn(g.x, sn));
  }
}

__global__ void cartesian_unpack_bwd_kernel(const float2* gX, long long rows, int F, const float* re_scale,
                                            const float* im_scale, float* dy) {
  const long long total = rows * F;
  const float rs = re_scale ? re_scale[0] : 1.f, is = im_scale ? im_scale[0] : 1.f;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / F;
    const int f = (int)(e - row * F);
    const float2 g = gX[e];
    float* d = dy + row * 2 * F;
    d[f] = re_scale ? g.x * rs : g.x;
    d[F + f] = im_scale ? g.y * is : g.y;
  }
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_magnitude_invert_backward(const float* y, int64_t rows, int K, int N, int pad_last, const void* g, int polar,
                                 const int* f_start, const int* f_len, const int* f_off, const float* f_w, int f_nnz,
                                 const int* t_start, const int* t_len, const int* t_off, const float* t_w, int t_nnz,
                                 int contrast, const float* offset, const float* scale, float eps,
                                 const float* phase_offset, const float* phase_scale, float* dy, void* stream) {
  if (rows < 0 || K <= 0 || N <= 0 || contrast < 0 || contrast > 3) return AT_EINVAL;
  if ((pad_last != 0 && pad_last != 1) || (polar != 0 && polar != 1) || K - pad_last < 0) return AT_EINVAL;
  if ((offset == nullptr) != (scale == nullptr) || (phase_offset == nullptr) != (phase_scale == nullptr)) return AT_EINVAL;
  const bool banked = t_w != nullptr;
  if (banked && !(t_start && t_len && t_off && t_nnz > 0)) return AT_EINVAL;
  if (!banked && (N != K || t_start || t_len || t_off)) return AT_EINVAL;
  if (polar) {
    if (!banked || pad_last || K != N || !(f_start && f_len && f_off && f_w && f_nnz > 0)) return AT_EINVAL;
  } else if (phase_offset) {
    return AT_EINVAL;
  }
  if (rows == 0 || K - pad_last == 0) return AT_OK;
  if (!y || !g || !dy) return AT_EINVAL;
  if ((((uintptr_t)y) & 3) || (((uintptr_t)dy) & 3) || (((uintptr_t)g) & (polar ? 7 : 3))) return AT_EINVAL;
  if (((uintptr_t)offset | (uintptr_t)scale | (uintptr_t)phase_offset | (uintptr_t)phase_scale) & 3) return AT_EINVAL;
  MagInvBwdParams p = {y, polar ? 2LL * K : (long long)(K - pad_last), rows, K, N, pad_last, g, polar,
                       {f_start, f_len, f_off, f_w, N, f_nnz}, {t_start, t_len, t_off, t_w, K, t_nnz},
                       contrast, offset, scale, eps, phase_offset, phase_scale, dy};
  return launch_magnitude_invert_backward(p, (hipStream_t)stream);
}

int at_polar_to_complex_backward(const float* gX_complex, const float* mag, const float* phase, int64_t n, float* gmag,
                                 float* gphase, void* stream) {
  if (n < 0) return AT_EINVAL;
  if (n == 0 || (!gmag && !gphase)) return AT_OK;
  if (!gX_complex || !phase || (gphase && !mag)) return AT_EINVAL;
  if (((uintptr_t)gX_complex) & 7) return AT_EINVAL;    // complex64 elements
  if (((uintptr_t)mag | (uintptr_t)phase | (uintptr_t)gmag | (uintptr_t)gphase) & 3) return AT_EINVAL;
  hipLaunchKernelGGL(polar_to_complex_bwd_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)gX_complex, mag, phase, (long long)n, gmag, gphase);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_cartesian_unpack_backward(const float* gX_complex, int64_t rows, int F, const float* re_scale,
                                 const float* im_scale, float* dy_stacked, void* stream) {
  if (rows < 0 || F <= 0) return AT_EINVAL;
  if (rows == 0) return AT_OK;
  if (!gX_complex || !dy_stacked) return AT_EINVAL;
  if (((uintptr_t)gX_complex) & 7) return AT_EINVAL;    // complex64 elements
  if (((uintptr_t)dy_stacked | (uintptr_t)re_scale | (uintptr_t)im_scale) & 3) return AT_EINVAL;
  hipLaunchKernelGGL(cartesian_unpack_bwd_kernel, dim3(flat_grid((long long)rows * F)), dim3(256), 0,
                     (hipStream_t)stream, (const float2*)gX_complex, (long long)rows, F, re_scale, im_scale, dy_stacked);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

// phase_vocoder.hip -- time-stretching of a complex spectrum (the phase vocoder of torchaudio.functional.phase_vocoder /
// torchaudio.transforms.TimeStretch, restated from the published algorithm) and its gradient, each as one scan along the
// frame axis of a (B, T, F) tensor.
//
// The textbook form takes the angle of two input frames per output frame, wraps their difference around the expected
// advance pi hop f / (F - 1), adds the advance back, runs a cumsum and goes through exp(i .).  The increment
// wrap(a1 - a0 - adv) + adv is congruent to a1 - a0 modulo 2 pi and only ever meets exp(i .): the advance, and with it
// hop_length, cancels.  What is left is a running product of unit phasors,
//     u(z) = z / |z|  (1 where z == 0),   p_0 = u(X[0]),   p_{j+1} = p_j u(X[idx_j + 1]) conj(u(X[idx_j])),
//     Z[j] = (alpha_j |X[idx_j + 1]| + (1 - alpha_j) |X[idx_j]|) p_j,        frame T a frame of zeros,
// with the step table (idx_j, alpha_j) = (floor(j rate), frac(j rate)) made on the host in float64: no atan2, no sincos, no
// wrap and no range reduction -- one reciprocal square root per input bin and two complex products per output bin.  The
// angle route in fp32 is off the float64 textbook result by 1.5e-2 (normwise) at 690 frames: the advance reaches 800 rad
// per step at hop 256 and one ulp there is 6e-5 rad.
//
// One thread owns a (clip, bin) column and walks j in order with p in registers, as the scans of phase_repr.hip do; the
// step table is the same for every column, so everything that depends on it is uniform across the launch.  The thread
// keeps the two input frames of the current step and loads a frame only when idx moves on (at rate > 2 frames are
// skipped and never read).  Built with -ffp-contract=off and every product written out, so a column's chain is the same
// instruction sequence in both layouts: its bits depend neither on the batch nor on the layout.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/acids_hip.h"
#include "variants.h"

namespace at_hip {

// output rows whose input frames are requested before the recurrence consumes them: 8 per thread over its NC columns (64
// bytes of X[idx + 1] in flight, twice that where frames are skipped; eight rows of two columns are 126 registers, and a
// fourth block of five wavefronts no longer fits a CU)
constexpr int kPvRowsAhead = 8;

// what the recurrences need of one input bin
struct PvBin {
  float m;        // |z|
  float ux, uy;   // z / |z|, (1, 0) where z == 0
  float rm;       // 1 / |z|, 0 where z == 0 (the backward's angle term)
};

// z = (x, y) scaled by a power of two into [0.5, 1) first: the sum of squares neither overflows nor loses a denormal,
// whatever the spectrum's level.  v_rsq_f32 (1 ulp) takes one Newton step, so |u| is 1 to about an ulp.  -0 + 0i counts as
// zero: u = 1, where torch.angle answers pi.
__device__ __forceinline__ PvBin pv_bin(float2 z) {
  const float s = fmaxf(fabsf(z.x), fabsf(z.y));
  const int e = __builtin_amdgcn_frexp_expf(s);
  const float x = ldexpf(z.x, -e), y = ldexpf(z.y, -e);
  const float n2 = fmaf(x, x, y * y);
  const float r0 = __builtin_amdgcn_rsqf(n2);
  const float r = r0 * fmaf(-0.5f * n2, r0 * r0, 1.5f);
  PvBin b;
  b.ux = x * r;
  b.uy = y * r;
  b.m = ldexpf(n2 * r, e);
  b.rm = ldexpf(r, -e);
  if (z.x == 0.0f && z.y == 0.0f) {
    b.m = 0.0f;
    b.ux = 1.0f;
    b.uy = 0.0f;
    b.rm = 0.0f;
  }
  return b;
}

__device__ __forceinline__ PvBin pv_zero_bin() {
  PvBin b;
  b.m = 0.0f;
  b.ux = 1.0f;
  b.uy = 0.0f;
  b.rm = 0.0f;
  return b;
}

// The accumulated phasor is kept in double.  With every product rounded to fp32 its phase walks off by 2e-6 over 1380 steps
// and the magnitude of a product of fp32 unit vectors by as much again: the forward would stay inside 1e-5 (3.1e-6 at 690
// frames, rate 0.5), the gradient, which meets the drift on the way up and on the way down, only just (7.8e-6 in an fp32
// restatement on the CPU).  In double the two products of fp32 factors are exact to 1e-16, the rounding of a frame's u
// cancels between the step that enters the frame and the step that leaves it, and one Newton step towards |p| = 1 per row
// takes out what |u| != 1 leaves: thirteen double operations per bin, where the kernel waits on memory.
struct PvPhasor {
  double x, y;
};
// p w (forward) or p conj(w) (backward), w = u(X[idx + 1]) conj(u(X[idx])), then p (1.5 - |p|^2 / 2)
template <bool BACK>
__device__ __forceinline__ PvPhasor pv_turn(PvPhasor p, const PvBin& lo, const PvBin& hi) {
  const double ax = hi.ux, ay = hi.uy, bx = lo.ux, by = lo.uy;
  const double wx = fma(ax, bx, ay * by), wy = fma(ay, bx, -(ax * by));
  PvPhasor q;
  if (BACK) {
    q.x = fma(p.x, wx, p.y * wy);
    q.y = fma(p.y, wx, -(p.x * wy));
  } else {
    q.x = fma(p.x, wx, -(p.y * wy));
    q.y = fma(p.x, wy, p.y * wx);
  }
  const double s = fma(-0.5, fma(q.x, q.x, q.y * q.y), 1.5);
  q.x *= s;
  q.y *= s;
  return q;
}
__device__ __forceinline__ float pv_mag(float a, const PvBin& lo, const PvBin& hi) { return fmaf(a, hi.m, (1.0f - a) * lo.m); }

// an entry of the step table, kept inside the clip whatever the table holds (the kernels never read out of bounds)
__device__ __forceinline__ int pv_idx(const int* __restrict__ idx, int j, int T) {
  const int i = idx[j];
  return i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
}

// The columns of a thread, as in phase_scan_kernel.  NC = 1: flattened (clip, bin) columns, 256 per block.  NC = 2 / 4:
// one block per clip, thread j walks columns j + k H, H = ceil(F / NC), the block's wavefronts in lockstep (one barrier
// per batch of rows), so that the 64-byte segments two wavefronts share (rows of 513 complex values are 4104 bytes) are
// written whole.  Threads past H stay for the barriers, walk a valid column again and store nothing.
template <int NC>
__device__ __forceinline__ bool pv_columns(long long B, long long F, long long& b, long long (&fk)[NC], bool (&on)[NC]) {
  if (NC == 1) {
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= B * F) return false;
    b = col / F;
    fk[0] = col - b * F;
    on[0] = true;
    return true;
  }
  b = blockIdx.x;
  const long long H = (F + NC - 1) / NC;
  const bool live = (long long)threadIdx.x < H;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const long long f = threadIdx.x + k * H;
    on[k] = live && f < F;
    fk[k] = on[k] ? f : (live ? (long long)threadIdx.x : 0);
  }
  return true;
}

// ---- forward -----------------------------------------------------------------------------------------------------------
// A batch of R output rows: the step table of the batch (uniform), then every input frame the batch is the first to need
// -- X[idx + 1] when idx moved, X[idx] too when it moved by more than one -- requested before the first row is worked on,
// then the rows in order.  Rows whose idx did not move load nothing: at rate 0.5 every second row.
template <int NC>
__global__ __launch_bounds__(NC > 1 ? 1024 : 256) void phase_vocoder_kernel(const float2* __restrict__ X, const int* __restrict__ idx,
                                                                            const float* __restrict__ alpha, float2* __restrict__ out,
                                                                            float2* __restrict__ fin, long long B, int T, long long F,
                                                                            int N) {
  long long b, fk[NC];
  bool on[NC];
  if (!pv_columns<NC>(B, F, b, fk, on)) return;
  const float2* src = X + b * T * F;
  float2* dst = out + b * N * F;
  PvBin lo[NC], hi[NC];
  PvPhasor p[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    lo[k] = hi[k] = pv_zero_bin();
    p[k].x = 1.0;
    p[k].y = 0.0;
  }
  int prev = -2;                    // idx of the row before: the first row loads both its frames
  auto batch = [&](auto rows, int j0) {
    constexpr int R = decltype(rows)::value;
    int id[R], adv[R];
    float al[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      id[r] = pv_idx(idx, j0 + r, T);
      al[r] = alpha[j0 + r];
      adv[r] = id[r] - (r ? id[r - 1] : prev);
    }
    prev = id[R - 1];
    float2 v0[NC][R], v1[NC][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (adv[r] != 0) {
        const bool inside = id[r] + 1 < T;          // frame T is the frame of zeros
#pragma unroll
        for (int k = 0; k < NC; ++k) v1[k][r] = inside ? src[(long long)(id[r] + 1) * F + fk[k]] : make_float2(0.0f, 0.0f);
        if (adv[r] != 1) {
#pragma unroll
          for (int k = 0; k < NC; ++k) v0[k][r] = src[(long long)id[r] * F + fk[k]];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (adv[r] != 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          if (adv[r] == 1) lo[k] = hi[k];
          else lo[k] = pv_bin(v0[k][r]);
          hi[k] = pv_bin(v1[k][r]);
        }
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        if (r == 0 && j0 == 0) {                // p_0 = u(X[0])
          p[k].x = lo[k].ux;
          p[k].y = lo[k].uy;
        }
        const float m = pv_mag(al[r], lo[k], hi[k]);
        if (NC == 1 || on[k]) dst[(long long)(j0 + r) * F + fk[k]] = make_float2(m * (float)p[k].x, m * (float)p[k].y);
        p[k] = pv_turn<false>(p[k], lo[k], hi[k]);
      }
    }
  };
  constexpr int R = kPvRowsAhead / NC;
  int j = 0;
  for (; j + R <= N; j += R) {
    batch(std::integral_constant<int, R>(), j);
    if (NC > 1) __syncthreads();        // lockstep: see phase_scan_kernel
  }
  for (; j < N; ++j) batch(std::integral_constant<int, 1>(), j);
  if (fin) {
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (NC == 1 || on[k]) fin[b * F + fk[k]] = make_float2((float)p[k].x, (float)p[k].y);
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// With Z_j = m_j p_j, p_j = exp(i phi_j) and g_j = dL/dZ_j:  gphi_j = Im(conj(Z_j) g_j),  gm_j = Re(conj(p_j) g_j),
// S_j = sum_{j' >= j} gphi_j'.  Per input frame i:
//   G_abs[idx_j] += (1 - alpha_j) gm_j,  G_abs[idx_j + 1] += alpha_j gm_j,
//   G_ang[0] += S_0,  and for j + 1 < N:  G_ang[idx_j + 1] += S_{j+1},  G_ang[idx_j] -= S_{j+1},
//   gX[i] = G_abs[i] u(X[i]) + G_ang[i] (-Im X[i] + i Re X[i]) / |X[i]|^2,   0 where X[i] == 0.
// The thread walks j downwards: p_j comes back from the saved final phasor by the conjugate step, S is a running sum, and
// the two frames of the step carry their own G_abs / G_ang.  idx only ever moves down, so when it does the upper frame has
// received everything and is written: a gather -- no atomics, no (B, N, F) intermediate.  Frames no step reads (rate > 2,
// or past the last step) get zeros; the frame of zeros T takes its share and is dropped.
// Flat columns only.  The clip-per-block form of this walk (two columns per thread, three rows ahead: 116 registers, so
// three blocks of five wavefronts per CU and 1024 clips in two rounds; four rows ahead spill) was measured beside it at
// 1024 x 690 x 513 and lost: 2.653 / 2.218 / 1.848 ms against 2.430 / 1.943 / 1.884 ms at rates 0.8 / 1.25 / 2.0.
struct PvAcc {
  float ga, gp;   // G_abs, G_ang of the frame
};

__device__ __forceinline__ float2 pv_grad(const PvBin& x, const PvAcc& a) {
  const float t = a.gp * x.rm;
  const float2 g = make_float2(fmaf(a.ga, x.ux, -(t * x.uy)), fmaf(a.ga, x.uy, t * x.ux));
  return (x.rm == 0.0f) ? make_float2(0.0f, 0.0f) : g;       // X == 0 (rm is NaN, not 0, for a NaN bin)
}

__global__ __launch_bounds__(256) void phase_vocoder_backward_kernel(const float2* __restrict__ X, const float2* __restrict__ g,
                                                                     const int* __restrict__ idx, const float* __restrict__ alpha,
                                                                     const float2* __restrict__ fin, float2* __restrict__ gX,
                                                                     long long B, int T, long long F, int N) {
  const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= B * F) return;
  const long long b = col / F, f = col - b * F;
  const float2* src = X + b * T * F + f;
  const float2* gsrc = g + b * N * F + f;
  float2* dst = gX + b * T * F + f;
  PvBin lo = pv_zero_bin(), hi = pv_zero_bin();
  PvAcc alo = {0.0f, 0.0f}, ahi = {0.0f, 0.0f};
  const float2 pN = fin[col];
  PvPhasor p = {pN.x, pN.y};
  double S = 0.0;                   // the suffix sum of gphi: N terms of either sign
  int cur = T + 1;                  // idx of the row after (none yet): the last row loads both its frames
  auto batch = [&](auto rows, int j0) {       // rows j0, j0 - 1, ..., j0 - R + 1
    constexpr int R = decltype(rows)::value;
    int id[R], adv[R];
    float al[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      id[r] = pv_idx(idx, j0 - r, T);
      al[r] = alpha[j0 - r];
      adv[r] = (r ? id[r - 1] : cur) - id[r];
    }
    float2 gv[R], v0[R], v1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      gv[r] = gsrc[(long long)(j0 - r) * F];
      if (adv[r] != 0) {
        v0[r] = src[(long long)id[r] * F];
        if (adv[r] != 1) v1[r] = (id[r] + 1 < T) ? src[(long long)(id[r] + 1) * F] : make_float2(0.0f, 0.0f);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (adv[r] != 0) {
        const int was = r ? id[r - 1] : cur;      // frames was, was + 1 are held (none before the first row: was = T + 1)
        if (was + 1 < T) dst[(long long)(was + 1) * F] = pv_grad(hi, ahi);
        if (adv[r] == 1) {
          hi = lo;
          ahi = alo;
        } else {
          if (was < T) dst[(long long)was * F] = pv_grad(lo, alo);
          // frames between the two pairs: nothing reads them (a table that moves up again rewrites, it never reads)
          const int top = was < T ? was : T;
          for (int t = id[r] + 2; t < top; ++t) dst[(long long)t * F] = make_float2(0.0f, 0.0f);
          hi = pv_bin(v1[r]);
          ahi.ga = ahi.gp = 0.0f;
        }
        lo = pv_bin(v0[r]);
        alo.ga = alo.gp = 0.0f;
      }
      p = pv_turn<true>(p, lo, hi);              // p_j
      const float px = (float)p.x, py = (float)p.y;
      const float m = pv_mag(al[r], lo, hi);
      const float2 z = make_float2(m * px, m * py);             // the forward's Z_j
      const float gphi = fmaf(z.x, gv[r].y, -(z.y * gv[r].x));
      const float gm = fmaf(px, gv[r].x, py * gv[r].y);
      const float Sf = (float)S;                 // S_{j+1}: 0 at the last row
      ahi.gp += Sf;
      alo.gp -= Sf;
      alo.ga = fmaf(1.0f - al[r], gm, alo.ga);
      ahi.ga = fmaf(al[r], gm, ahi.ga);
      S += (double)gphi;
    }
    cur = id[R - 1];
  };
  int j = N - 1;
  for (; j - (kPvRowsAhead - 1) >= 0; j -= kPvRowsAhead) batch(std::integral_constant<int, kPvRowsAhead>(), j);
  for (; j >= 0; --j) batch(std::integral_constant<int, 1>(), j);
  alo.gp += (float)S;                             // G_ang[0] += S_0: row 0 reads frame 0
  if (cur + 1 < T) dst[(long long)(cur + 1) * F] = pv_grad(hi, ahi);
  dst[(long long)cur * F] = pv_grad(lo, alo);
  for (int t = 0; t < cur; ++t) dst[(long long)t * F] = make_float2(0.0f, 0.0f);
}

// columns per thread of the clip-per-block layout (0: flattened columns), as clip_block_columns of phase_repr.hip for
// rows of complex64
static int pv_clip_block_columns(long long F, long long B) {
  if (variant(kVarScanLayout) == 1) return 0;
  if ((F * 8) % 64 == 0 || F < 256 || B < 64) return 0;
  return F <= 2048 ? 2 : F <= 4096 ? 4 : 0;
}

static int pv_check(int64_t B, int64_t T, int64_t F, int64_t N) {
  if (B < 0 || T < 0 || F < 0 || N < 0) return AT_EINVAL;
  if ((T == 0) != (N == 0)) return AT_EINVAL;          // every clip with a frame has row 0, and only those
  if (T > INT_MAX - 2 || N > INT_MAX - kPvRowsAhead) return AT_EUNSUPPORTED;     // int frame and row indices
  if (B > INT_MAX || (B > 0 && F > (long long)INT_MAX * 256 / B)) return AT_EUNSUPPORTED;   // the grid
  return AT_OK;
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_phase_vocoder(const float* X_complex, int64_t B, int64_t T, int64_t F, const int* idx, const float* alpha, int64_t N,
                     float* out_complex, float* final_phasor, void* stream) {
  const int rc = pv_check(B, T, F, N);
  if (rc != AT_OK) return rc;
  if (B * T * F == 0) return AT_OK;
  if (!X_complex || !idx || !alpha || !out_complex || X_complex == out_complex) return AT_EINVAL;
  if (((uintptr_t)X_complex | (uintptr_t)out_complex | (uintptr_t)final_phasor) & 7) return AT_EINVAL;    // complex64 elements
  if (((uintptr_t)idx | (uintptr_t)alpha) & 3) return AT_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const float2* x = (const float2*)X_complex;
  float2 *o = (float2*)out_complex, *fin = (float2*)final_phasor;
  const int nc = pv_clip_block_columns(F, B);
  if (nc) {
    const dim3 grid((unsigned)B), block((unsigned)((((F + nc - 1) / nc) + 63) / 64 * 64));
    if (nc == 2) hipLaunchKernelGGL(phase_vocoder_kernel<2>, grid, block, 0, s, x, idx, alpha, o, fin, (long long)B, (int)T, (long long)F, (int)N);
    else hipLaunchKernelGGL(phase_vocoder_kernel<4>, grid, block, 0, s, x, idx, alpha, o, fin, (long long)B, (int)T, (long long)F, (int)N);
  } else {
    const dim3 grid((unsigned)((B * F + 255) / 256)), block(256);
    hipLaunchKernelGGL(phase_vocoder_kernel<1>, grid, block, 0, s, x, idx, alpha, o, fin, (long long)B, (int)T, (long long)F, (int)N);
  }
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_phase_vocoder_backward(const float* X_complex, const float* g_complex, const int* idx, const float* alpha,
                              const float* final_phasor, int64_t B, int64_t T, int64_t F, int64_t N, float* gX_complex,
                              void* stream) {
  const int rc = pv_check(B, T, F, N);
  if (rc != AT_OK) return rc;
  if (B * T * F == 0) return AT_OK;
  if (!X_complex || !g_complex || !idx || !alpha || !final_phasor || !gX_complex) return AT_EINVAL;
  if (gX_complex == X_complex || gX_complex == g_complex) return AT_EINVAL;
  if (((uintptr_t)X_complex | (uintptr_t)g_complex | (uintptr_t)final_phasor | (uintptr_t)gX_complex) & 7) return AT_EINVAL;
  if (((uintptr_t)idx | (uintptr_t)alpha) & 3) return AT_EINVAL;
  const dim3 grid((unsigned)((B * F + 255) / 256)), block(256);
  hipLaunchKernelGGL(phase_vocoder_backward_kernel, grid, block, 0, (hipStream_t)stream, (const float2*)X_complex,
                     (const float2*)g_complex, idx, alpha, (const float2*)final_phasor, (float2*)gX_complex, (long long)B, (int)T,
                     (long long)F, (int)N);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

// repr_grad.hip -- the backward passes of the phase-side representations' FORWARD: Phase / IF (at_phase_scan and its
// strided form, the phase halves of Polar and PolarIF) and the one-pass Cartesian.forward, so that a spectral loss built
// on these representations trains what produced the spectrum (the STFT adjoint of autograd.hip takes it from there).
//
// Gradient convention (torch's, for a complex tensor and a real loss): gX = dL/dRe + i dL/dIm.
//
// The scans (reference utils/misc.py:12-26, 65-81; spectral_repr.py:318-335).  In autograd of the reference's own
// statements `unwrap` has the identity as its derivative (ddmod - diff contributes g - g, the masked assignment zeroes
// the rest, so the cumsum gets no gradient): the forward is a scan along time, the backward is not.  For
//     y_t = (w_t s_t fdiff(unwrap(angle X))_t - off) / sc           and G = dL/dy
//     a_t = G_t w_t s_t / sc      (w = 1 unweighted, sc = 1 without Normalize)
//     s_t = 1/pi on rows 0..T-2 (forward), -1/pi on rows 1..T-1 (backward), 1/(2 pi) on rows 1..T-2 (central), else 1
//   angle, unwrap:  gu_t = a_t
//   forward:        gu_t = c_t a_t - a_{t+1}/2 (while t+1 <= T-1),   c_0 = 1, else 1/2
//   backward:       gu_t = c_t a_t - a_{t-1}/2 (while t >= 1),       c_{T-1} = 1, else 1/2
//   central:        gu_t = [t = 0] a_0 + [t = T-1] a_{T-1} + a_{t-1}/4 [1 <= t-1 <= T-2] - a_{t+1}/4 [1 <= t+1 <= T-2]
//                   (T = 1: at_phase_scan writes the one row once, so gu_0 = a_0)
//     gX_t = gu_t (-Im X_t + i Re X_t) / |X_t|^2,   0 where X_t == 0 (torch's angle backward)
//
// The output is a contiguous complex64 stream and nothing is carried along time, so this is a flat grid-stride pass:
// consecutive lanes write consecutive 8-byte elements (as phase_angle_kernel of phase_repr.hip; the row misalignment at
// F = 513 that shaped the forward scans does not touch a flat stream).  The rows t-1 and t+1 of g are re-reads of lines
// some neighbouring lane fetched as its row t: L2 serves them.  Algorithmic bytes per bin: 8 (X) + 4 (g) + 8 (out) = 20,
// 28 with the accumulated gradient.  Every bin is a function of its own X, its (up to) three g and the scalars alone: its
// bits depend neither on the batch nor on the grid.  Neighbouring rows that the stencil does not use are never
// multiplied in (their loads are re-pointed at the row itself and discarded by a select), so a NaN of g stays within
// rows t-1..t+1.
//
// Cartesian.forward (reference :403-428), y = [(Re X - o_re) / s_re, (Im X - o_im) / s_im] stacked:
//     gX = G[.., 0, :] / s_re + i G[.., 1, :] / s_im.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"

namespace at_hip {

// as phase_repr.hip
enum { SCAN_UNWRAP = 0, SCAN_IF_FORWARD = 1, SCAN_IF_BACKWARD = 2, SCAN_IF_CENTRAL = 3, SCAN_ANGLE = 4 };
// the stencils: angle and unwrap share the first
enum { ST_NONE = 0, ST_FORWARD = 1, ST_BACKWARD = 2, ST_CENTRAL = 3 };

constexpr float kInvPi = 1.0f / 3.14159265358979323846f;
constexpr float kInvTwoPi = 1.0f / 6.28318530717958647692f;
// blocks of the flat passes: beyond kScanBwdMaxBlocks * 256 elements the threads loop (tests/repr_grad_cases.py sizes
// its grid-loop case from this)
constexpr long long kScanBwdMaxBlocks = 256 * 64;

struct ScanBwdParams {
  const float2* X;        // (B, T, F) complex64
  const float* g;         // rows of ld_g floats, F of them read
  const float* window;    // T floats, or null
  const float* scale;     // device scalar, or null
  const float2* accum;    // (B, T, F) complex64 added to the result, or null; may be `out`
  float2* out;            // (B, T, F) complex64; may be X
  long long rows, T, F, ld_g;
};

// (row, bin) of a flat index and of the grid stride: one division per thread (32-bit when everything fits), then carried
struct FlatWalk {
  long long row, f, d_row, d_f;
  __device__ __forceinline__ FlatWalk(unsigned long long i, unsigned long long stride, unsigned long long total, long long F) {
    if (total <= 0xffffffffull && stride <= 0xffffffffull) {
      const unsigned Fu = (unsigned)F, r = (unsigned)i / Fu, dr = (unsigned)stride / Fu;
      row = r;
      f = (unsigned)i - r * Fu;
      d_row = dr;
      d_f = (unsigned)stride - dr * Fu;
    } else {
      const unsigned long long Fu = (unsigned long long)F, r = i / Fu, dr = stride / Fu;
      row = (long long)r;
      f = (long long)(i - r * Fu);
      d_row = (long long)dr;
      d_f = (long long)(stride - dr * Fu);
    }
  }
  // returns 1 when the bin wrapped into the next row
  __device__ __forceinline__ int advance(long long F) {
    row += d_row;
    f += d_f;
    if (f >= F) {
      f -= F;
      ++row;
      return 1;
    }
    return 0;
  }
};

template <int ST>
__device__ __forceinline__ float row_scale(long long t, long long T) {
  if (ST == ST_FORWARD) return t < T - 1 ? kInvPi : 1.0f;
  if (ST == ST_BACKWARD) return t >= 1 ? -kInvPi : 1.0f;
  if (ST == ST_CENTRAL) return (t >= 1 && t < T - 1) ? kInvTwoPi : 1.0f;
  return 1.0f;
}

// Stencil, window, scale, stride of g and accum are template flags, as in phase_scan_kernel (whose header comment has
// what run-time tests in the loop cost).
template <int ST, bool WIN, bool SCALE, bool STRIDED, bool ACCUM>
__global__ __launch_bounds__(256) void phase_scan_bwd_kernel(ScanBwdParams p) {
  const long long T = p.T, F = p.F;
  const unsigned long long total = (unsigned long long)p.rows * (unsigned long long)F;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
  unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= total) return;
  FlatWalk at(i, stride, total, F);
  long long t = at.row % T;
  const long long d_t = at.d_row % T;
  const long long ldg = STRIDED ? p.ld_g : F;
  const float inv_sc = SCALE ? 1.0f / *p.scale : 1.0f;
  // a_t' = G_t' (w_t' s_t' / sc)
  auto coeff = [&](long long tt) -> float {
    float k = row_scale<ST>(tt, T);
    if (WIN) k *= p.window[tt];
    if (SCALE) k *= inv_sc;
    return k;
  };
  for (; i < total; i += stride) {
    const float2 x = p.X[i];
    float2 acc = make_float2(0.f, 0.f);
    if (ACCUM) acc = p.accum[i];
    const float* gp = p.g + at.row * ldg + at.f;
    const bool has_prev = t >= 1, has_next = t + 1 < T;
    // all loads up front; a neighbour outside the clip is the row itself, read again and dropped by the selects below
    const float g0 = gp[0];
    float gu;
    if (ST == ST_NONE) {
      gu = SCALE ? g0 * inv_sc : g0;
    } else if (ST == ST_FORWARD) {
      const float g1 = gp[has_next ? ldg : 0];
      const float a0 = g0 * coeff(t), a1 = g1 * coeff(has_next ? t + 1 : t);
      gu = t == 0 ? a0 : 0.5f * a0;
      gu = has_next ? gu - 0.5f * a1 : gu;
    } else if (ST == ST_BACKWARD) {
      const float g1 = gp[has_prev ? -ldg : 0];
      const float a0 = g0 * coeff(t), a1 = g1 * coeff(has_prev ? t - 1 : t);
      gu = t == T - 1 ? a0 : 0.5f * a0;
      gu = has_prev ? gu - 0.5f * a1 : gu;
    } else {
      const bool use_prev = t >= 2, use_next = t + 2 < T;     // rows 1..T-2 are the interior rows of the forward
      const float gm = gp[use_prev ? -ldg : 0], gn = gp[use_next ? ldg : 0];
      const float a0 = g0 * coeff(t);
      const float am = gm * coeff(use_prev ? t - 1 : t), an = gn * coeff(use_next ? t + 1 : t);
      gu = (t == 0 || t == T - 1) ? a0 : 0.0f;
      gu = use_prev ? gu + 0.25f * am : gu;
      gu = use_next ? gu - 0.25f * an : gu;
    }
    const float q = gu / (x.x * x.x + x.y * x.y);
    float re = -x.y * q, im = x.x * q;
    const bool zero = x.x == 0.0f && x.y == 0.0f;
    re = zero ? 0.0f : re;
    im = zero ? 0.0f : im;
    if (ACCUM) {
      re += acc.x;
      im += acc.y;
    }
    p.out[i] = make_float2(re, im);
    t += d_t + at.advance(F);
    if (t >= T) t -= T;
  }
}

template <int ST, bool WIN, bool SCALE, bool STRIDED>
static void launch_scan_bwd4(bool accum, dim3 grid, hipStream_t s, const ScanBwdParams& p) {
  if (accum) hipLaunchKernelGGL((phase_scan_bwd_kernel<ST, WIN, SCALE, STRIDED, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((phase_scan_bwd_kernel<ST, WIN, SCALE, STRIDED, false>), grid, dim3(256), 0, s, p);
}
template <int ST, bool WIN, bool SCALE>
static void launch_scan_bwd3(bool strided, bool accum, dim3 grid, hipStream_t s, const ScanBwdParams& p) {
  if (strided) launch_scan_bwd4<ST, WIN, SCALE, true>(accum, grid, s, p);
  else launch_scan_bwd4<ST, WIN, SCALE, false>(accum, grid, s, p);
}
template <int ST, bool WIN>
static void launch_scan_bwd2(bool scale, bool strided, bool accum, dim3 grid, hipStream_t s, const ScanBwdParams& p) {
  if (scale) launch_scan_bwd3<ST, WIN, true>(strided, accum, grid, s, p);
  else launch_scan_bwd3<ST, WIN, false>(strided, accum, grid, s, p);
}
template <int ST>
static void launch_scan_bwd1(bool win, bool scale, bool strided, bool accum, dim3 grid, hipStream_t s, const ScanBwdParams& p) {
  if (win) launch_scan_bwd2<ST, true>(scale, strided, accum, grid, s, p);
  else launch_scan_bwd2<ST, false>(scale, strided, accum, grid, s, p);
}

static unsigned flat_blocks(long long n) {
  const long long blocks = (n + 255) / 256;
  return (unsigned)(blocks > kScanBwdMaxBlocks ? kScanBwdMaxBlocks : blocks);
}

// (rows, 2, F) float32 -> (rows, F) complex64
__global__ __launch_bounds__(256) void cartesian_pack_bwd_kernel(const float* __restrict__ g, long long rows, int F,
                                                                 const float* re_scale, const float* im_scale,
                                                                 float2* __restrict__ out) {
  const unsigned long long total = (unsigned long long)rows * (unsigned long long)F;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
  unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= total) return;
  const float rs = re_scale ? *re_scale : 1.f, is = im_scale ? *im_scale : 1.f;
  FlatWalk at(i, stride, total, F);
  for (; i < total; i += stride) {
    const float* src = g + 2 * at.row * F + at.f;
    const float a = src[0], b = src[F];
    out[i] = make_float2(re_scale ? a / rs : a, im_scale ? b / is : b);
    at.advance(F);
  }
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_phase_scan_backward(const float* X_complex, int64_t B, int64_t T, int64_t F, int mode, const float* g, int64_t ld_g,
                           const float* frame_window, const float* scale, const float* accum_complex, float* out_complex,
                           void* stream) {
  if (B < 0 || T < 0 || F < 0 || ld_g < F) return AT_EINVAL;
  if (mode < SCAN_UNWRAP || mode > SCAN_ANGLE) return AT_EINVAL;
  if (frame_window && (mode == SCAN_UNWRAP || mode == SCAN_ANGLE)) return AT_EINVAL;
  if (B == 0 || T == 0 || F == 0) return AT_OK;
  if (!X_complex || !g || !out_complex) return AT_EINVAL;
  if (((uintptr_t)X_complex | (uintptr_t)accum_complex | (uintptr_t)out_complex) & 7) return AT_EINVAL;   // complex64 elements
  if (((uintptr_t)g | (uintptr_t)frame_window | (uintptr_t)scale) & 3) return AT_EINVAL;
  if (B > (1LL << 62) / T || B * T > (1LL << 62) / ld_g) return AT_EINVAL;
  ScanBwdParams p = {(const float2*)X_complex, g, frame_window, scale, (const float2*)accum_complex, (float2*)out_complex,
                     B * T, T, F, ld_g};
  const dim3 grid(flat_blocks(B * T * F));
  hipStream_t s = (hipStream_t)stream;
  const bool win = frame_window != nullptr, sc = scale != nullptr, strided = ld_g != F, accum = accum_complex != nullptr;
  switch (mode) {
    case SCAN_IF_FORWARD: launch_scan_bwd1<ST_FORWARD>(win, sc, strided, accum, grid, s, p); break;
    case SCAN_IF_BACKWARD: launch_scan_bwd1<ST_BACKWARD>(win, sc, strided, accum, grid, s, p); break;
    case SCAN_IF_CENTRAL: launch_scan_bwd1<ST_CENTRAL>(win, sc, strided, accum, grid, s, p); break;
    default: launch_scan_bwd2<ST_NONE, false>(sc, strided, accum, grid, s, p); break;
  }
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_cartesian_pack_backward(const float* g_stacked, int64_t rows, int F, const float* re_scale, const float* im_scale,
                               float* out_complex, void* stream) {
  if (rows < 0 || F < 0) return AT_EINVAL;
  if (rows == 0 || F == 0) return AT_OK;
  if (!g_stacked || !out_complex) return AT_EINVAL;
  if (((uintptr_t)out_complex) & 7) return AT_EINVAL;    // complex64 elements
  if (((uintptr_t)g_stacked | (uintptr_t)re_scale | (uintptr_t)im_scale) & 3) return AT_EINVAL;
  if (rows > (1LL << 61) / F) return AT_EINVAL;
  hipLaunchKernelGGL(cartesian_pack_bwd_kernel, dim3(flat_blocks((long long)rows * F)), dim3(256), 0, (hipStream_t)stream,
                     g_stacked, (long long)rows, F, re_scale, im_scale, (float2*)out_complex);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

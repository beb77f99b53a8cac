// mel_distance.hip -- the kernels of MelSpectralDistance (losses.py, autograd.MelSpectralDistanceFunction): the mel rows
// of a spectrum, the per-clip sums of a distance between two arrays of mel rows, and the backward, which turns ONE
// spectrum into its own gradient in place given the OTHER signal's mel rows.  The STFTs around them are
// ops.stft_forward / ops.stft_backward.
//
// For clip b at one scale, W the (K x N) mel bank, M = |X| W and Q = |Y| W, both (T, N), n = T N cells:
//     S_D = sum (M - Q)^2      S_B = sum Q^2      S_L = sum |ln(M + eps) - ln(Q + eps)|
//     loss_b = lin_weight S_D / S_B + log_weight S_L / n                        (summed over scales by the caller)
// Backward, g the upstream gradient of loss_b, d = M - Q:
//     dM = g (lin_weight 2 d / S_B + log_weight sgn(d) / (n (M + eps)))
//     dQ = g (lin_weight (-2 d / S_B - 2 Q S_D / S_B^2) - log_weight sgn(d) / (n (Q + eps)))
//     dA[k] = sum_j W[k, j] dM[j],   G_X = dA X / |X| (0 where X == 0);   G_Y likewise from dQ and Y
// ln is monotone, so sgn(d) is the sign of the log difference: the backward takes no logarithm.
//
// Only a mel row of the other signal is needed to differentiate one signal: the backward holds one spectrum, reads
// N / K of another and recomputes its own mel row with md_row_abs + band_dot, the device code md_rows_kernel itself
// runs -- the recomputed value has the bits of the stored one, so x == y gives an exactly zero d in every cell.
//
// Rows: one wave per row, wpb rows per workgroup, persistent workgroups, the bank tables staged in LDS once per
// workgroup (band_cols.h), under the one row plan of the banded backward kernels (band_plan.h).
// md_rows_kernel strides its row groups over the grid; md_backward_kernel gives each workgroup a contiguous run of
// them, so that a clip's constants are formed once per clip and workgroup, not once per row.
// Sums, the clip's constants and the per-cell derivatives: distance_core.h, the sums on float cells as stored.
#include "band_cols.h"
#include "distance_core.h"

namespace at_hip {

// |row| into the wave's LDS slice a; KIT > 0: the row stays in xv.  The one place a magnitude is formed in this file.
// The register row is band_row_load's, element lane + 64 q in xv[q], but loaded without a branch (the index clamped to
// the row's last bin): behind band_row_load's guards the in-place backward got a wait for all earlier loads in front
// of each of the nine, one trip to memory after the other.
template <int KIT>
__device__ __forceinline__ void md_row_abs(float2 (&xv)[KIT > 0 ? KIT : 1], const float2* row, int lane, int K,
                                           float* a) {
  if (KIT > 0) {
#pragma unroll
    for (int q = 0; q < KIT; ++q) {
      const int k = lane + 64 * q;
      xv[q] = row[k < K ? k : K - 1];
    }
#pragma unroll
    for (int q = 0; q < KIT; ++q) {
      const int k = lane + 64 * q;
      if (k < K) a[k] = md_abs(xv[q]);
    }
  } else {
    for (int k = lane; k < K; k += 64) a[k] = md_abs(row[k]);
  }
}

// ---- 1. mel rows ------------------------------------------------------------------------------------------------------

struct MelRowsParams {
  const float2* X;        // rows x K
  long long rows;
  int K, N;
  BandCols f;             // the bank by column (N columns)
  float* out;             // rows x N
};

template <bool TAB_LDS, int KIT>
__global__ void md_rows_kernel(MelRowsParams p, int k_pad, int tab_floats) {
  extern __shared__ float md_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int K = p.K, N = p.N;
  BandCols f = p.f;
  if (TAB_LDS) {
    float* cur = md_lds;
    f = band_stage(p.f, cur);
  }
  float* a = md_lds + (TAB_LDS ? tab_floats : 0) + wave * k_pad;
  for (long long r0 = (long long)blockIdx.x * wpb; r0 < p.rows; r0 += (long long)gridDim.x * wpb) {
    const long long row = r0 + wave;
    const bool live = row < p.rows;
    float2 xv[KIT > 0 ? KIT : 1];
    if (live) md_row_abs<KIT>(xv, p.X + row * K, lane, K, a);
    __syncthreads();
    if (live)
      for (int j = lane; j < N; j += 64) p.out[row * N + j] = band_dot(f, j, a);
    __syncthreads();
  }
}

static int launch_mel_rows(const MelRowsParams& p, hipStream_t stream) {
  const int k_pad = pad64(p.K);
  const size_t per_wave = sizeof(float) * (size_t)k_pad;
  const BandPlan pl = band_plan(band_tab_floats(band_cols_floats(p.f)), per_wave);
  if (!pl.ok) return AT_EUNSUPPORTED;
  auto run = [&](auto kernel) { return band_launch_rows(kernel, pl, p.rows, stream, p, k_pad, (int)pl.tab_floats); };
  if (!pl.tab_lds) return run(md_rows_kernel<false, 0>);
  return p.K <= kBandKit * 64 ? run(md_rows_kernel<true, kBandKit>) : run(md_rows_kernel<true, 0>);
}

// ---- 2. backward ------------------------------------------------------------------------------------------------------

struct MelDistBwdParams {
  float2* S;              // (B T) x K: the spectrum, overwritten by its gradient
  const float* O;         // (B T) x N: the other signal's mel rows
  long long rows, T;
  int K, N;
  BandCols f;             // the bank by column (N columns)
  BandCols t;             // the transposed bank by column (K columns)
  const double* sums;     // (B, 3)
  const float* gclip;     // (B)
  float lin_weight, log_weight, eps;
  int side;               // 0: S = X, O = Q;  1: S = Y, O = M
};

template <bool TAB_LDS, int KIT>
__global__ void md_backward_kernel(MelDistBwdParams p, int k_pad, int n_pad, int tab_floats) {
  extern __shared__ float md_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int K = p.K, N = p.N;
  BandCols f = p.f, t = p.t;
  if (TAB_LDS) {
    float* cur = md_lds;
    t = band_stage(p.t, cur);
    f = band_stage(p.f, cur);
  }
  float* a = md_lds + (TAB_LDS ? tab_floats : 0) + wave * (k_pad + n_pad);
  float* dm = a + k_pad;
  const double cells = (double)p.T * (double)N;
  // A workgroup takes a contiguous run of row groups, so that its rows change clip once in T rows: the clip's constants
  // (a 64-bit division for the clip and a double division for 1 / S_B) are formed on that change alone.  They are a
  // function of the clip, whichever workgroup or wave forms them.
  const long long groups = (p.rows + wpb - 1) / wpb;
  const long long per_block = (groups + gridDim.x - 1) / gridDim.x;
  const long long g0 = (long long)blockIdx.x * per_block;
  const long long g1 = g0 + per_block < groups ? g0 + per_block : groups;
  long long clip_end = 0;                      // the first row past the clip whose constants are held
  float c_lin = 0.f, c_sq = 0.f, c_log = 0.f;
  for (long long grp = g0; grp < g1; ++grp) {
    const long long row = grp * wpb + wave;
    const bool live = row < p.rows;
    float2* srow = p.S + row * K;
    float2 xv[KIT > 0 ? KIT : 1];
    if (live) md_row_abs<KIT>(xv, srow, lane, K, a);
    if (live && row >= clip_end) {
      const long long b = row / p.T;
      dist_consts((double)p.gclip[b], p.sums[3 * b], p.sums[3 * b + 1], p.lin_weight, p.log_weight, cells, c_lin, c_sq, c_log);
      clip_end = (b + 1) * p.T;
    }
    __syncthreads();
    if (live) {
      const float* orow = p.O + row * N;
      for (int j = lane; j < N; j += 64) {
        const float other = orow[j];                                     // in flight during the walk
        const float own = band_dot(f, j, a);
        const float d = p.side == 0 ? own - other : other - own;         // M - Q
        const float lg = dist_lg(d, c_log);
        const float lind = c_lin * d;
        dm[j] = p.side == 0 ? dist_d_generated(lind, lg, own, p.eps) : dist_d_target(lind, lg, own, c_sq, p.eps);
      }
    }
    __syncthreads();
    if (live) {
      if (KIT > 0) {
#pragma unroll
        for (int q = 0; q < KIT; ++q) {
          const int k = lane + 64 * q;
          if (k < K) srow[k] = dist_bin_grad(band_dot(t, k, dm), md_abs(xv[q]), xv[q]);
        }
      } else {
        for (int k = lane; k < K; k += 64) {
          const float2 x = srow[k];
          srow[k] = dist_bin_grad(band_dot(t, k, dm), md_abs(x), x);
        }
      }
    }
    __syncthreads();
  }
}

static int launch_mel_distance_backward(const MelDistBwdParams& p, hipStream_t stream) {
  const int k_pad = pad64(p.K), n_pad = pad64(p.N);
  const size_t per_wave = sizeof(float) * (size_t)(k_pad + n_pad);
  const BandPlan pl = band_plan(band_tab_floats(band_cols_floats(p.t) + band_cols_floats(p.f)), per_wave);
  if (!pl.ok) return AT_EUNSUPPORTED;
  auto run = [&](auto kernel) { return band_launch_rows(kernel, pl, p.rows, stream, p, k_pad, n_pad, (int)pl.tab_floats); };
  if (!pl.tab_lds) return run(md_backward_kernel<false, 0>);
  return p.K <= kBandKit * 64 ? run(md_backward_kernel<true, kBandKit>) : run(md_backward_kernel<true, 0>);
}

static inline bool md_cols_ok(const int* start, const int* len, const int* off, const float* w, int nnz) {
  return start && len && off && w && nnz > 0;
}

}  // namespace at_hip

extern "C" {

int at_mel_rows(const float* X_complex, int64_t rows, int K, int N, const int* f_start, const int* f_len,
                const int* f_off, const float* f_w, int f_nnz, float* out, void* stream) {
  using namespace at_hip;
  if (rows == 0) return AT_OK;
  if (rows < 0 || K <= 0 || N <= 0) return AT_EINVAL;
  if (!X_complex || !out || !md_cols_ok(f_start, f_len, f_off, f_w, f_nnz)) return AT_EINVAL;
  if (((uintptr_t)X_complex) & 7) return AT_EINVAL;    // complex64 bins
  MelRowsParams p = {(const float2*)X_complex, rows, K, N, {f_start, f_len, f_off, f_w, N, f_nnz}, out};
  return launch_mel_rows(p, (hipStream_t)stream);
}

size_t at_mel_distance_workspace_bytes(int64_t B, int64_t n) { return at_hip::dist_workspace_bytes(B, n); }

int at_mel_distance_sums(const float* M, const float* Q, int64_t B, int64_t n, float eps, double* sums, void* workspace,
                         size_t workspace_bytes, void* stream) {
  using namespace at_hip;
  if (B == 0) return AT_OK;                                   // before n and eps, unlike at_spectral_distance_sums
  if (B < 0 || n < 1 || !(eps >= 0.f)) return AT_EINVAL;
  return dist_sums(M, Q, B, n, eps, sums, workspace, workspace_bytes, (hipStream_t)stream);
}

int at_mel_distance_backward(float* S_complex, const float* other, int64_t B, int64_t T, int K, int N,
                             const int* f_start, const int* f_len, const int* f_off, const float* f_w, int f_nnz,
                             const int* t_start, const int* t_len, const int* t_off, const float* t_w, int t_nnz,
                             const double* sums, const float* gclip, float lin_weight, float log_weight, float eps,
                             int side, void* stream) {
  using namespace at_hip;
  if (B == 0) return AT_OK;
  if (B < 0 || T <= 0 || K <= 0 || N <= 0 || !(eps >= 0.f) || (side != 0 && side != 1)) return AT_EINVAL;
  if (!S_complex || !other || !sums || !gclip) return AT_EINVAL;
  if (!md_cols_ok(f_start, f_len, f_off, f_w, f_nnz) || !md_cols_ok(t_start, t_len, t_off, t_w, t_nnz)) return AT_EINVAL;
  if (((uintptr_t)S_complex) & 7) return AT_EINVAL;    // complex64 bins
  MelDistBwdParams p = {(float2*)S_complex, other, (long long)B * T, (long long)T, K, N,
                        {f_start, f_len, f_off, f_w, N, f_nnz}, {t_start, t_len, t_off, t_w, K, t_nnz},
                        sums, gclip, lin_weight, log_weight, eps, side};
  return launch_mel_distance_backward(p, (hipStream_t)stream);
}

}  // extern "C"

// autograd.h -- launchers of autograd.hip (the STFT and ISTFT adjoints and the Magnitude backward), of mfcc_grad.hip
// (the MFCC backward), of invert_grad.hip (the Magnitude.invert / Polar.invert backward) and of stream_grad.hip (the
// streaming path: OverlapAdd, RealtimeSTFT, RealtimeDGT), for the C entry points.  The three banded backward kernels
// take their banks as BandCols (band_cols.h, with everything else they share): f the bank by column, t its transpose.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/acids_hip.h"     // the launchers return AT_OK or an AT_E* code
#include "band_cols.h"

namespace at_hip {

// blocks of 256 threads of a flat grid-stride pass over n > 0 elements
inline unsigned flat_grid(long long n) {
  const long long blocks = (n + 255) / 256;
  return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

struct MagBwdParams {
  const void* A;          // rows x K: complex64 (a_kind 0) or float32 (a_kind 3)
  int a_kind;
  long long rows;
  int K, N, col_off;      // dF: rows x (N - col_off)
  const float* dF;
  BandCols f;             // forward bank by column (N columns); f.w null: mel=False
  BandCols t;             // transposed bank by column (K columns)
  int contrast;
  const float* scale;     // null: no Normalize
  float eps;
  const void* dX_in;      // null, or rows x K of the same type: added to the result
  void* dX;
};

// the MFCC backward (mfcc_grad.hip): spectrum and channel-major gradient of one chunk of clips
struct MfccBwdParams {
  const float2* X;        // (B, T, K)
  float2* dX;             // (B, T, K); may be X
  const float* dF;        // (B, C, T)
  long long B, T;
  int K, N, C, power;     // N filters; C == N without a DCT; power 1 or 2
  BandCols f;             // forward bank by column (N columns); read on the DCT route only
  BandCols t;             // transposed bank by column (K columns)
  const float* dct_t;     // (C, N): the DCT matrix transposed; null: no DCT
  const float* scale;     // null: no Normalize
};

// the backward of Magnitude.invert and of the one-pass Polar.invert (invert_grad.hip)
struct MagInvBwdParams {
  const float* y;         // rows x (K - pad_last), row stride ld_y; polar: rows x 2 x K stacked (ld_y = 2 K)
  long long ld_y;         // also dy's row stride
  long long rows;
  int K, N, pad_last;     // the (K x N) inverse bank; pad_last: the last of the K columns is the reference's zero pad
  const void* g;          // rows x N: float32, or complex64 (polar)
  int polar;
  BandCols f;             // inverse bank by column (N columns); read by the polar form only
  BandCols t;             // transposed inverse bank by column (K columns); t.w null: mel=False
  int contrast;
  const float *offset, *scale;          // null: no Normalize
  float eps;
  const float *ph_offset, *ph_scale;    // polar: the phase half's Normalize, or null
  float* dy;
};

int launch_magnitude_invert_backward(const MagInvBwdParams& p, hipStream_t stream);
int launch_mfcc_backward(const MfccBwdParams& p, hipStream_t stream);
int launch_adj_window(const float* w, int n_fft, float scale, float* out, hipStream_t stream);
int launch_adj_ola_fold(const float* frames, const float2* G, const float* window, float* dx, long long B, long long T,
                        long long L, int n_fft, int hop, hipStream_t stream);
int launch_magnitude_backward(const MagBwdParams& p, hipStream_t stream);
// ISTFT adjoint: u (prep), then, after the forward's rFFT, the DC / Nyquist halves or the polar epilogue (finish)
int launch_istft_adj_prep(const float* gy, const float* window, float* u, long long B, long long T, int n_fft, int hop,
                          hipStream_t stream);
int launch_istft_adj_finish(const float2* gX, const float* phase, void* out, long long rows, int n_fft, hipStream_t stream);
// the streaming path (stream_grad.hip): the DC / Nyquist halves of the frame-analysis adjoint added to its irFFT frames in
// place, and the adjoints of OverlapAdd.forward and OverlapAdd.invert
int launch_rfft_adj_edge(float* frames, const float2* G, const float* window, long long rows, int n_fft,
                         hipStream_t stream);
int launch_oadd_forward_adj(const float* gframes, long long S, long long n, int n_fft, int hop, int keep, long long C,
                            float* gx, hipStream_t stream);
int launch_oadd_invert_adj(const float* gy, long long S, long long n, int n_fft, int hop, int keep, const float* gain,
                           float* gframes, hipStream_t stream);

}  // namespace at_hip

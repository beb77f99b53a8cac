// stft_launch.h -- what the STFT translation units share with capi.hip: every launch_* that crosses a file (each file
// that defines one includes this header, so a declaration cannot drift from its definition unseen) and the layout of
// the side twiddle table that at_init fills and the size-specific kernels read.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/acids_hip.h"     // the launchers return AT_OK or an AT_E* code
#include "band_bank.h"

namespace at_hip {

// The side table (float2 entries, forward sign), segment by segment.  A launcher is handed the start of its segment.
constexpr int kSideW2048 = 0;        // W2048^k, k < 1024                                       (stft2048.hip)
constexpr int kSideW512 = 1024;      // W512^k, k < 256                                         (stft512.hip)
constexpr int kSide256 = 1280;       // W512^(r k), r = 1..3, k < 128                           (stft_small.hip, n_fft 256)
constexpr int kSide128 = 1664;       // W512^(r k), r = 1..7, k < 64                            (stft_small.hip, n_fft 128)
constexpr int kSide4096 = 2112;      // W4096^k, k < 2048; then W2048^(r k), r = 1..3, k < 512  (stft4096.hip)
constexpr int kSide4096Radix = kSide4096 + 2048;
constexpr int kSideTableCount = kSide4096Radix + 3 * 512;
static_assert(kSideW512 == kSideW2048 + 1024 && kSide256 == kSideW512 + 256 && kSide128 == kSide256 + 3 * 128 &&
              kSide4096 == kSide128 + 7 * 64 && kSideTableCount == 5696, "the segments of the side table are contiguous");

// stft1024.hip
int launch_stft1024_fwd(const float* x, long long B, long long L, long long clip_stride, long long T, int hop, int center,
                        const float* window, const float2* tw, float2* out, float* phase, hipStream_t stream);
int launch_stft1024_h256_fwd(const float* x, long long B, long long L, long long clip_stride, long long T,
                             const float* window, const float2* tw, float2* out, float* phase, const BandBank* bank,
                             float* feat, const float* offset, const float* scale, float eps, int contrast, int power2,
                             int feat_channel_major, hipStream_t stream, const PolarOut* polar = nullptr, int hop = 256);
int launch_istft1024_ola(const float2* X, const float* mag, const float* phase, long long B, long long T, int hop,
                         const float* window, const float* env16, const float2* tw, float* y, hipStream_t stream,
                         const float2* gl_tprev = nullptr, float gl_mom = 0.f);
int launch_irfft1024_frames(const float2* X, const float* mag, const float* phase, long long nframes, const float* window,
                            const float2* tw, float* y, hipStream_t stream);
// stft_generic.hip, stft_mixed.hip
int launch_rfft_generic(const float* x, long long B, long long L, long long clip_stride, long long T, int n_fft, int hop,
                        int center, const float* window, float2* out, float* phase, hipStream_t stream);
int launch_rfft_mixed(const float* x, long long B, long long L, long long clip_stride, long long T, int n_fft, int hop,
                      int center, const float* window, float2* out, float* phase, hipStream_t stream);
int launch_irfft_generic(const float2* X, const float* mag, const float* phase, long long nframes, int n_fft,
                         const float* window, float* frames, hipStream_t stream);
int launch_irfft_mixed(const float2* X, const float* mag, const float* phase, long long nframes, int n_fft,
                       const float* window, float* frames, hipStream_t stream);
int launch_ola_gather(const float* frames, long long B, long long T, int n_fft, int hop, const float* window, float* y,
                      hipStream_t stream);
// stft2048.hip (tw2k: the table at kSideW2048)
int launch_stft2048_fwd(const float* x, long long B, long long L, long long clip_stride, long long T, int hop, int center,
                        const float* window, const float2* tw, const float2* tw2k, float2* out, float* phase,
                        hipStream_t stream);
int launch_stft2048_mel(const float* x, long long B, long long L, long long clip_stride, long long T, int hop,
                        const float* window, const float2* tw, const float2* tw2k, const BandBank* bank, int contrast,
                        int power2, const float* offset, const float* scale, float eps, float* feat, int channel_major,
                        hipStream_t stream);
int launch_istft2048_ola(const float2* X, const float* mag, const float* phase, long long B, long long T, int hop,
                         const float* window, const float* env, const float2* tw, const float2* tw2k, float* y,
                         hipStream_t stream);
int launch_irfft2048_frames(const float2* X, const float* mag, const float* phase, long long nframes, const float* window,
                            const float2* tw, const float2* tw2k, float* frames, hipStream_t stream);
// stft4096.hip (tw4k: at kSide4096)
int launch_stft4096_fwd(const float* x, long long B, long long L, long long clip_stride, long long T, int hop, int center,
                        const float* window, const float2* tw, const float2* tw4k, float2* out, float* phase,
                        hipStream_t stream);
int launch_istft4096_ola(const float2* X, const float* mag, const float* phase, long long B, long long T, int hop,
                         const float* window, const float* env, const float2* tw, const float2* tw4k, float* y,
                         hipStream_t stream);
int launch_irfft4096_frames(const float2* X, const float* mag, const float* phase, long long nframes, const float* window,
                            const float2* tw, const float2* tw4k, float* frames, hipStream_t stream);
// stft_small.hip (n_fft 256 / 128: four / eight frames per wave-level FFT; twk: at kSide256 / kSide128)
int launch_stft_small_fwd(int n_fft, const float* x, long long B, long long L, long long clip_stride, long long T, int hop,
                          int center, const float* window, const float2* tw, const float2* twk, float2* out, float* phase,
                          hipStream_t stream);
int launch_irfft_small_frames(int n_fft, const float2* X, const float* mag, const float* phase, long long nframes,
                              long long frames_per_clip, const float* window, const float2* tw, const float2* twk,
                              float* frames, hipStream_t stream);
// stft512.hip (tw512: at kSideW512)
int launch_stft512_fwd(const float* x, long long B, long long L, long long clip_stride, long long T, int hop, int center,
                       const float* window, const float2* tw, const float2* tw512, float2* out, float* phase,
                       hipStream_t stream);
int launch_stft512_mel(const float* x, long long B, long long L, long long clip_stride, long long T, int hop,
                       const float* window, const float2* tw, const float2* tw512, const BandBank* bank, int contrast,
                       int power2, const float* offset, const float* scale, float eps, float* feat, int channel_major,
                       hipStream_t stream);
int launch_irfft512_frames(const float2* X, const float* mag, const float* phase, long long nframes,
                           long long frames_per_clip, const float* window, const float2* tw, const float2* tw512,
                           float* frames, hipStream_t stream);
int launch_istft512_ola(const float2* X, const float* mag, const float* phase, long long B, long long T, int hop,
                        const float* window, const float* env, const float2* tw, const float2* tw512, float* y,
                        hipStream_t stream);

}  // namespace at_hip

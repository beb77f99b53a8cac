// stft2048.hip -- n_fft = 2048 on the one-wavefront register FFT core (fft512.h).
//
// Replaces, for n_fft = 2048 (any hop):
//   torch.stft(...).transpose(-2,-1)          reference transforms/stft.py:98-104, dgt.py:64-70
//   torch.fft.rfft(x*window) on frames        stft.py:249-253, dgt.py:285-289
//   torch.fft.irfft(X) * inv_window           stft.py:260-266, dgt.py:296-302; the frames of torch.istft
//                                             (stft.py:120-128), overlap-added by stft_generic.hip's gather
// Until round 2 this size ran on the workgroup-per-frame LDS Stockham kernel of stft_generic.hip (~1.4 TB/s).
//
// A 2048-point real transform is a 1024-point complex FFT of z[n] = x[2n] + i x[2n+1] plus the real split; the
// 1024-point FFT is two 512-point FFTs (the wave-level radix-8 core: 8 complex points per lane) of the even and the
// odd complex samples plus one radix-2 stage:
//   ze[m] = z[2m]   = x[4m]   + i x[4m+1]        -> one float4 load per lane and register holds (ze, zo) of the
//   zo[m] = z[2m+1] = x[4m+2] + i x[4m+3]           same m: 1 KB contiguous per wave instruction
//   Z[k] = Ze[k] + W1024^k Zo[k],  Z[k+512] = Ze[k] - W1024^k Zo[k]     (k = lane + 64 m: lane-local)
//   X[k] = (Z[k] + conj Z[1024-k])/2 - (i/2) W2048^k (Z[k] - conj Z[1024-k]),  k = 0 .. 1024
// The mirror partner Z[1024-k] lives in lane 64-lane, register 15-m (lane 0: its own register 16-m).  The inverse
// runs the same steps backwards.  One wave = one frame at a time, frames of a block interleaved over its four
// waves, the next frame's loads issued before the current frame's FFTs.
//
// Each direction's arithmetic is written once: fwd_core2k (two FFTs, radix-2, mirror, merge; plain or with rotated
// output columns) serves the frame, run and mel kernels, inv_core2k (radix-2 backwards, two FFTs) behind fft512.h's
// load_spectrum_row / irfft_presplit serves the frames and the fused overlap-add kernel (ola_window.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "fastmath.h"
#include "fft512.h"
#include "band_bank.h"
#include "mel_gemm.h"   // C_* contrast codes
#include "ola_window.h"
#include "row_stream.h"
#include "run_plan.h"
#include "stft_launch.h"
#include "variants.h"
#include <stdlib.h>

namespace at_hip {

constexpr int N2K = 2048;
constexpr int F2K = N2K / 2 + 1;     // 1025
constexpr int W2K = 4;               // waves per block

// q[j] = x[s + 4 (lane + 64 j) .. + 3] of frame f (reflect padding with center, zero padding without)
__device__ __forceinline__ void load_frame2k(const float* x, long long clip_stride, long long L, long long T, int hop,
                                             int center, long long f, int lane, float4 (&q)[8]) {
  const long long b = f / T, t = f - b * T;
  const float* clip = x + b * clip_stride;
  const long long start = t * (long long)hop - (center ? N2K / 2 : 0);
  const bool interior = (start >= 0) && (start + N2K <= L);
  if (interior && ((((uintptr_t)(clip + start)) & 15) == 0)) {
    const float4* src = reinterpret_cast<const float4*>(clip + start);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = src[lane + 64 * j];
  } else if (interior) {
    const float* src = clip + start;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = 4 * (lane + 64 * j);
      q[j] = make_float4(src[i], src[i + 1], src[i + 2], src[i + 3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long i0 = start + 4 * (lane + 64 * j);
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long long i = i0 + c;
        if (center) v[c] = clip[reflect_index(i, L)];
        else v[c] = (i >= 0 && i < L) ? clip[i] : 0.0f;     // zero padding past the end (utils/misc.py:156)
      }
      q[j] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// All kernels keep the constant tables in LDS, shared by the block's waves and read at the point of use (the fft512
// twiddles: 11 KB; W2048^k: 8 KB): held in registers they cost 76 VGPRs and leave one wave per SIMD.  Ends with the
// block's __syncthreads(): a kernel that stages more (a window, a bank) does so first.
template <bool INV, int THREADS>
__device__ __forceinline__ void stage_tables2k(const float2* tw, const float2* tw2k, float2* tab, float2* w2tab) {
  for (int i = threadIdx.x; i < kTwiddleCount; i += THREADS) tab[i] = twiddle_for_lds<INV>(tw, i);
  for (int i = threadIdx.x; i < 1024; i += THREADS) w2tab[i] = tw2k[i];
  __syncthreads();
}

// a frame's raw samples times the window (global memory or LDS) -> the inputs of the two 512-point FFTs
__device__ __forceinline__ void window2k(const float4 (&q)[8], const float4* win, int lane, v2f (&ze)[8], v2f (&zo)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float4 w = win[lane + 64 * j];
    ze[j] = (v2f){q[j].x * w.x, q[j].y * w.y};
    zo[j] = (v2f){q[j].z * w.z, q[j].w * w.w};
  }
}

// The forward core: the windowed even / odd complex samples -> out(m, X[col + 64 m]), m = 0 .. 15, in that order; returns
// X[1024] (real; meaningful on the lane whose column is 0).  ROT: the output columns are rotated over the lanes, this lane
// holds column col = (lane - rot) & 63 (the run kernel; the radix-2 stage is lane-local and does not care, the twiddles
// W1024^k / 2 and W2048^k and the mirror lane follow the column); otherwise rot = 0, col = lane.  The rotated form reads
// W2048^k one ds_read_b64 at a time, as its fft512 twiddles are; the plain form leaves the pairing of those reads to the
// compiler.  The bins go to a consumer, not to an array: a kernel that stores or reduces them does so inside the merge
// loop, as the kernels did before they shared this core -- through an array stft2048_mel_kernel<2, false> took 174 VGPRs
// instead of 168 and lost a resident wave per SIMD (profiles/nfft_cores.md).
template <bool ROT, typename OUT>
__device__ __forceinline__ float fwd_core2k(v2f (&ze)[8], v2f (&zo)[8], const float2* tab, float2* lds, int lane, int rot,
                                            int col, OUT&& out) {
  v2f z[16];
  const LdsTwiddles<false> tw = {tab, lane}, twc = {tab, col};     // getr(m) = W1024^(. + 64 m) / 2
  const v2f hh = {0.5f, 0.5f};
  fft512<false>(ze, tw, lds, lane, col);
  fft512<false>(zo, tw, lds, lane, col);
  // radix-2: H = Z / 2 (the real split wants the half): H[k] = Ze/2 + (W1024^k / 2) Zo, H[k+512] = Ze/2 - ...
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const v2f t = cmul_v(zo[m], twc.getr(m));
    const v2f e = ze[m] * hh;
    z[m] = e + t;
    z[m + 8] = e - t;
  }
  v2f pm[16];
  mirror_regs_rot<16>(z, pm, lane, rot, col);
  // X[k] = (H[k] + conj H') - i W2048^k (H[k] - conj H'),  H = Z / 2,  H' = H[1024 - k]  (k = 0: H' = H[0], X[0] real)
  const float nyq = 2.0f * (z[0].x - z[0].y);                     // X[1024] = Re Z[0] - Im Z[0]
  const v2f* w2 = reinterpret_cast<const v2f*>(tab + kTwiddleCount) + col;     // w2[64 m] = W2048^(col + 64 m)
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const v2f e = add_conj(z[m], pm[m]);
    const v2f d = sub_conj(z[m], pm[m]);
    out(m, add_mi(e, cmul_v(d, ROT ? lds_read_single(w2 + 64 * m) : w2[64 * m])));      // e - i W d
  }
  return nyq;
}

template <bool WRITE_PHASE>
__global__ __launch_bounds__(64 * W2K, 3) void stft2048_fwd_kernel(PFrames p) {
  __shared__ float2 lds_all[W2K * kFftLdsFloat2PerWave + kTwiddleCount + 1024];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W2K * kFftLdsFloat2PerWave;      // the fft512 twiddles, W2048^k behind them
  stage_tables2k<false, 64 * W2K>(p.tw, p.tw_n, tab, tab + kTwiddleCount);
  const long long f_begin = (long long)blockIdx.x * p.frames_per_block;
  long long f_end = f_begin + p.frames_per_block;
  if (f_end > p.total_frames) f_end = p.total_frames;
  const float4* win4 = reinterpret_cast<const float4*>(p.window);    // L1/L2-resident (8 KB), re-read per frame instead of 32 VGPRs

  long long f = f_begin + wave;
  float4 nxt[8];
  if (f < f_end) load_frame2k(p.x, p.clip_stride, p.L, p.T, p.hop, p.center, f, lane, nxt);
  for (; f < f_end; f += W2K) {
    v2f ze[8], zo[8];
    window2k(nxt, win4, lane, ze, zo);
    if (f + W2K < f_end) load_frame2k(p.x, p.clip_stride, p.L, p.T, p.hop, p.center, f + W2K, lane, nxt);
    float2* row = p.X + f * F2K;
    float* prow = WRITE_PHASE ? p.phase_out + f * F2K : nullptr;
    const float nyq = fwd_core2k<false>(ze, zo, tab, lds, lane, 0, lane, [&](int m, v2f xk) {
      row[lane + 64 * m] = to_f2(xk);
      if (WRITE_PHASE) prow[lane + 64 * m] = fast_atan2f(xk.y, xk.x);
    });
    if (lane == 0) {
      row[1024] = make_float2(nyq, 0.0f);
      if (WRITE_PHASE) prow[1024] = fast_atan2f(0.0f, nyq);
    }
  }
}


// ---------------------------------------------------------------------------
// forward, hop = 512 = N/4, center = True: the sliding-window / aligned-stream form of the n_fft-1024 kernel (round 3).
// A wave walks a run of consecutive frames of one clip.  Register j of a lane holds x[s + 4 (lane + 64 j) .. + 3], so the
// next frame is "registers j + 2 of the same lane": the raw samples stay in registers, shifted by two slots per frame,
// and only the 512 new samples (two 16-byte loads per lane) are fetched -- 2 KB of loads per frame instead of 8 KB.
// The spectrum leaves through the aligned row stream of row_stream.h (NB = 16: sixteen full-block non-temporal stores
// per frame): the output columns of both 512-point FFTs are rotated over the lanes, the radix-2 stage is lane-local
// and does not care, the merge's twiddles (W1024^k / 2, W2048^k) and mirror lane follow the column.
// ---------------------------------------------------------------------------

// 256 samples (one register slot of the wave) starting at original index i0 of the clip, reflect-padded
__device__ __forceinline__ float4 load_slot2k(const float* clip, long long L, long long i0, int lane) {
  const long long i = i0 + 4 * lane;
  if (i0 >= 0 && i0 + 256 <= L) return *reinterpret_cast<const float4*>(clip + i);     // clip base 16-byte aligned (launcher)
  return make_float4(clip[reflect_index(i, L)], clip[reflect_index(i + 1, L)], clip[reflect_index(i + 2, L)],
                     clip[reflect_index(i + 3, L)]);
}

constexpr int W2KR = 8;     // waves per block of the run kernel: two blocks per CU, four waves per SIMD (126 VGPRs)
__global__ __launch_bounds__(64 * W2KR, 4) void stft2048_run_fwd_kernel(PRunFwd p) {
  __shared__ float2 lds_all[W2KR * kFftLdsFloat2PerWave + kTwiddleCount + 1024 + 1024];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W2KR * kFftLdsFloat2PerWave;
  float4* wintab = reinterpret_cast<float4*>(tab + kTwiddleCount + 1024);          // analysis window, 512 float4
  for (int i = threadIdx.x; i < 512; i += 64 * W2KR) wintab[i] = reinterpret_cast<const float4*>(p.window)[i];
  stage_tables2k<false, 64 * W2KR>(p.tw, p.tw_n, tab, tab + kTwiddleCount);

  const long long run = (long long)blockIdx.x * W2KR + wave, b = run / p.runs_per_clip;
  if (b >= p.B) return;
  long long t0, t1;
  if (!run_units(run - b * p.runs_per_clip, p.units_per_run, p.T, t0, t1)) return;
  const float* clip = p.x + b * p.clip_stride;
  const long long L = p.L;

  float4 raw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) raw[j] = load_slot2k(clip, L, t0 * 512 - 1024 + 256 * j, lane);
#pragma unroll
  for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(raw[j].x), "+v"(raw[j].y), "+v"(raw[j].z), "+v"(raw[j].w));

  RowStream<16, v2f> out;
  out.begin(reinterpret_cast<v2f*>(p.X), (b * p.T + t0) * F2K, lane);

  auto frame_body = [&](const float4 (&fresh)[2]) {
    wave_priority<3>();        // transform > stores, as in stft1024.hip
    v2f ze[8], zo[8], z[16];
    window2k(raw, wintab, lane, ze, zo);
#pragma unroll
    for (int j = 0; j < 6; ++j) raw[j] = raw[j + 2];
    raw[6] = fresh[0];
    raw[7] = fresh[1];
    const v2f nyq = {fwd_core2k<true>(ze, zo, tab, lds, lane, out.rot, (lane - out.rot) & 63, [&](int m, v2f xk) { z[m] = xk; }), 0.0f};
    wave_priority<1>();
    out.emit(z, nyq, lane);
    wave_priority<0>();
  };

  long long t = t0;
  long long t_fast_end = (L >= 1536) ? (L - 1536) / 512 + 1 : 0;     // first t whose successor's new samples need reflection
  if (t_fast_end > t1 - 1) t_fast_end = t1 - 1;
  if (t < t_fast_end) {
    const float4* nsrc = reinterpret_cast<const float4*>(clip + t * 512 + 1024) + lane;
    for (; t < t_fast_end; ++t) {
      float4 fresh[2];
      fresh[0] = nsrc[0];
      fresh[1] = nsrc[64];
      nsrc += 128;
      frame_body(fresh);
    }
  }
  for (; t < t1; ++t) {
    float4 fresh[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (t + 1 < t1) {
      fresh[0] = load_slot2k(clip, L, t * 512 + 1024, lane);
      fresh[1] = load_slot2k(clip, L, t * 512 + 1280, lane);
    }
    frame_body(fresh);
  }
  out.end(lane);
}

// The inverse core: v[m] = Z[lane + 64 m] of irfft_presplit<16> (fft512.h) -> the unnormalised time samples,
// (y[0][j], y[1][j]) = x[4 n .. 4 n + 3], n = lane + 64 j -- the radix-2 stage backwards and the two 512-point FFTs.
__device__ __forceinline__ void inv_core2k(const v2f (&v)[16], const LdsTwiddles<true>& tw, float2* lds, int lane,
                                           v2f (&y)[2][8]) {
  // radix-2 backwards: even samples from Z[k] + Z[k+512], odd ones from (Z[k] - Z[k+512]) conj(W1024^k)
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    y[0][m] = v[m] + v[m + 8];
    y[1][m] = cmul_conj_v(v[m] - v[m + 8], tw.getr(m));
  }
  fft512<true>(y[0], tw, lds, lane);
  fft512<true>(y[1], tw, lds, lane);
}

// irfft(X) * window, frames out (the overlap-add is stft_generic.hip's gather): complex or polar input
template <bool POLAR>
__global__ __launch_bounds__(64 * W2K, 3) void irfft2048_frames_kernel(PFrames p) {
  __shared__ float2 lds_all[W2K * kFftLdsFloat2PerWave + kTwiddleCount + 1024];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W2K * kFftLdsFloat2PerWave;
  const v2f* w2 = reinterpret_cast<const v2f*>(tab + kTwiddleCount) + lane;     // w2[64 m] = W2048^(lane + 64 m)
  stage_tables2k<true, 64 * W2K>(p.tw, p.tw_n, tab, tab + kTwiddleCount);
  const LdsTwiddles<true> tw = {tab, lane};      // tw.getr(m) = W1024^(lane + 64 m)
  const long long f_begin = (long long)blockIdx.x * p.frames_per_block;
  long long f_end = f_begin + p.frames_per_block;
  if (f_end > p.total_frames) f_end = p.total_frames;
  const float4* win4 = reinterpret_cast<const float4*>(p.window);
  const float scale = 1.0f / 2048.0f;             // the split's factor 2 is in here
  for (long long f = f_begin + wave; f < f_end; f += W2K) {
    v2f v[16], z[16], y[2][8];
    float nyq_re;
    load_spectrum_row<16, POLAR>(p.X, p.mag, p.phase, f * F2K, lane, v, nyq_re);
    irfft_presplit<16, 64>(v, nyq_re, lane, w2, z);
    inv_core2k(z, tw, lds, lane, y);
    float4* dst = reinterpret_cast<float4*>(p.y + f * N2K);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 w = win4[lane + 64 * j];
      dst[lane + 64 * j] = make_float4(y[0][j].x * (w.x * scale), y[0][j].y * (w.y * scale), y[1][j].x * (w.z * scale),
                                       y[1][j].y * (w.w * scale));
    }
  }
}

// ---------------------------------------------------------------------------
// torch.istft for n_fft = 2048, hop = 256 / 512 / 1024 in one kernel: irfft + window + overlap-add + envelope
// (reference stft.py:120-128, dgt.py:86-93; polar input: stft.py:157-161, dgt.py:152-154).  The inverse core above into
// the register window of ola_window.h, one float4 per lane and 256-sample slot.
// ---------------------------------------------------------------------------
template <bool POLAR, int HS>
__global__ __launch_bounds__(64 * W2K, 2) void istft2048_ola_kernel(POla p) {
  constexpr int HOP = 256 * HS, R = 8 / HS, LEAD = 1024 / HOP;      // LEAD: blocks trimmed at the front
  __shared__ float2 lds_all[W2K * kFftLdsFloat2PerWave + kTwiddleCount + 1024 + 1024];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W2K * kFftLdsFloat2PerWave;
  const v2f* w2 = reinterpret_cast<const v2f*>(tab + kTwiddleCount) + lane;
  float4* wintab = reinterpret_cast<float4*>(tab + kTwiddleCount + 1024);
  stage_ola_window<N2K, 64 * W2K>(p.window, wintab);
  stage_tables2k<true, 64 * W2K>(p.tw, p.tw_n, tab, tab + kTwiddleCount);
  const LdsTwiddles<true> tw = {tab, lane};
  long long b, c0, c1;
  if (!ola_run_blocks(p, (long long)blockIdx.x * W2K + wave, LEAD, b, c0, c1)) return;
  const long long T = p.T;
  const float4* env4 = reinterpret_cast<const float4*>(p.env);
  float* yclip = p.y + b * (HOP * (T - 1));

  // Complex input: the next frame's row is requested before the current one is transformed (one frame = 8 KB per wave
  // in flight; the index is clamped into the clip so that the load is unconditional -- a conditional load would make
  // the compiler drain vmcnt on the spot).  Until round 3 every frame's loads were issued and consumed back to back.
  v2f nxt[16];
  float nxt_nyq = 0.f;
  auto request = [&](long long t) {
    const long long tc = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    const float2* row = p.X + (b * T + tc) * F2K;
#pragma unroll
    for (int m = 0; m < 16; ++m) nxt[m] = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(row) + lane + 64 * m);
    nxt_nyq = reinterpret_cast<const float*>(row + 1024)[0];
  };
  if constexpr (!POLAR) request(c0 - (R - 1));
  OlaWindow<HS, 1> ola;
  ola.init(env4, lane);

  for (long long t = c0 - (R - 1); t < c1; ++t) {
    v2f cur[16], z[16], y[2][8];
    float cur_nyq = 0.f;
    if constexpr (!POLAR) {
#pragma unroll
      for (int m = 0; m < 16; ++m) cur[m] = nxt[m];
      cur_nyq = nxt_nyq;
      request(t + 1);
    }
    if (t >= 0 && t < T) {
      if constexpr (POLAR) load_spectrum_row<16, true>(nullptr, p.mag, p.phase, (b * T + t) * F2K, lane, cur, cur_nyq);
      irfft_presplit<16, 64>(cur, cur_nyq, lane, w2, z);
      inv_core2k(z, tw, lds, lane, y);
      ola.add_frame(y, wintab, lane);
    }
    // block t is complete: frames t - R + 1 .. t are all that cover it
    if (t >= c0) ola.emit(yclip + (t - LEAD) * HOP, env4, ola.frame_mask(t, T), lane);
    ola.slide();
  }
}

// ---------------------------------------------------------------------------
// Features-only forward: audio -> normalise(contrast(|X|^p @ bank)) for a banded bank, n_fft = 2048, any hop
// (MelSpectrogram / MFCC at torchaudio's and librosa's usual 2048 / 512: mel.py:43-44, 68-73 behind stft.py:98-104).
// The forward kernel above with the spectrum kept in registers: |X|^p goes into an LDS row of the wave, every lane walks
// the band of its filter(s) (band_bank.h, the walk of mel_banded.hip) and the features leave row-major, or channel-major
// through the eight-frame register window with sector-aligned flushes.  The 2.9 GB spectrum of 1024 clips is never
// written: STFT 1.06 ms + projection 0.78 ms -> one kernel.
// A wave takes a run of consecutive frames (the window wants the frames of a clip in order).
// ---------------------------------------------------------------------------
struct P2kMel {
  const float* x;
  const float* window;
  const float2* tw;
  const float2* tw2k;
  float* feat;           // (B*T, N) or (B, N, T)
  const float* offset;   // Normalize (device scalars) or null
  const float* scale;
  long long L, clip_stride, T, total_frames, frames_per_wave;
  int win_off_f2;        // where the window table starts in dynamic LDS, in float2 units (16-byte aligned)
  BandBank bank;
  int hop, contrast, power2, channel_major, row_floats, table_floats;
  float eps;
};

// One pass of the band walk: this lane's filter over `quads` float4 of the |X|^p row from `a` on, its weights at w[64 j]
// (the pass's block of the lane-interleaved table); moves w past the block and returns the sum.
__device__ __forceinline__ float band_walk2k(const float* a, const float4*& w, int quads) {
  const float4* a4 = reinterpret_cast<const float4*>(a);
  v2f acc2 = {0.f, 0.f};
  int j = 0;
  for (; j + 4 <= quads; j += 4) {          // four steps' reads ahead of the multiply-adds
    float4 av[4], wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = a4[j + u];
      wv[u] = w[(j + u) * 64];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc2 = __builtin_elementwise_fma((v2f){av[u].x, av[u].y}, (v2f){wv[u].x, wv[u].y}, acc2);
      acc2 = __builtin_elementwise_fma((v2f){av[u].z, av[u].w}, (v2f){wv[u].z, wv[u].w}, acc2);
    }
  }
  for (; j < quads; ++j) {
    const float4 av = a4[j], wv = w[j * 64];
    acc2 = __builtin_elementwise_fma((v2f){av.x, av.y}, (v2f){wv.x, wv.y}, acc2);
    acc2 = __builtin_elementwise_fma((v2f){av.z, av.w}, (v2f){wv.z, wv.w}, acc2);
  }
  w += quads * 64;
  return acc2.x + acc2.y;
}

// CMW 1 / 2: channel-major output of a bank with that many passes (register window); 0: anything else.  WINLDS: the
// analysis window staged in LDS (when the bank's tables leave 8 KB of the two-blocks-per-CU budget).
template <int CMW, bool WINLDS>
__global__ __launch_bounds__(64 * W2K, 2) void stft2048_mel_kernel(P2kMel p) {
  extern __shared__ __attribute__((aligned(16))) float2 lds_all[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W2K * kFftLdsFloat2PerWave;
  float* rows = reinterpret_cast<float*>(tab + kTwiddleCount + 1024);
  float* absrow = rows + wave * p.row_floats;
  float* wlds = rows + W2K * p.row_floats;
  int* lane_tab = reinterpret_cast<int*>(wlds + p.table_floats);
  for (int i = threadIdx.x; i < p.table_floats; i += 64 * W2K) wlds[i] = p.bank.weights[i];
  for (int i = threadIdx.x; i < 64 * p.bank.n_passes; i += 64 * W2K) {
    lane_tab[i] = p.bank.lane_start[i];
    lane_tab[64 * p.bank.n_passes + i] = p.bank.lane_filter[i];
  }
  for (int k = 1024 + lane; k < p.row_floats; k += 64) absrow[k] = 0.0f;     // bin 1024 is rewritten per frame
  // the analysis window, shared by the block's waves (round 3): read from global memory per frame it was 8 KB per frame
  // through the vector-memory path, as much as the frame's samples
  float4* wintab = reinterpret_cast<float4*>(lds_all + (WINLDS ? p.win_off_f2 : 0));
  if constexpr (WINLDS)
    for (int i = threadIdx.x; i < 512; i += 64 * W2K) wintab[i] = reinterpret_cast<const float4*>(p.window)[i];
  const float4* win4 = reinterpret_cast<const float4*>(p.window);
  stage_tables2k<false, 64 * W2K>(p.tw, p.tw2k, tab, tab + kTwiddleCount);
  const long long f_begin = ((long long)blockIdx.x * W2K + wave) * p.frames_per_wave;
  long long f_end = f_begin + p.frames_per_wave;
  if (f_end > p.total_frames) f_end = p.total_frames;
  if (f_begin >= f_end) return;
  float off = 0.f, sc = 1.f;
  if (p.offset) {
    off = *p.offset;
    sc = *p.scale;
  }

  float cm[CMW > 0 ? CMW : 1][8];
  long long e_next[CMW > 0 ? CMW : 1];
  int held[CMW > 0 ? CMW : 1];
#pragma unroll
  for (int q = 0; q < (CMW > 0 ? CMW : 1); ++q) {
    held[q] = 0;
    e_next[q] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cm[q][k] = 0.f;
  }
  bool e_valid = false;
  long long cb = f_begin / p.T, ct = f_begin - cb * p.T;

  float4 nxt[8];
  load_frame2k(p.x, p.clip_stride, p.L, p.T, p.hop, 1, f_begin, lane, nxt);
  for (long long f = f_begin; f < f_end; ++f) {
    wave_priority<3>();        // transform > epilogue
    v2f ze[8], zo[8];
    if constexpr (WINLDS) window2k(nxt, wintab, lane, ze, zo);
    else window2k(nxt, win4, lane, ze, zo);
    if (f + 1 < f_end) load_frame2k(p.x, p.clip_stride, p.L, p.T, p.hop, 1, f + 1, lane, nxt);
    const float nyq = fwd_core2k<false>(ze, zo, tab, lds, lane, 0, lane, [&](int m, v2f xk) {
      const float s2 = fmaf(xk.x, xk.x, xk.y * xk.y);
      absrow[lane + 64 * m] = p.power2 ? s2 : __builtin_amdgcn_sqrtf(s2);
    });                                                  // X[1024] (lane 0), real
    if (lane == 0) absrow[1024] = p.power2 ? nyq * nyq : fabsf(nyq);
    wave_lds_sync();
    wave_priority<0>();

    const long long b = cb, t = ct;
    if (++ct == p.T) {
      ct = 0;
      ++cb;
    }
    const float4* w = reinterpret_cast<const float4*>(wlds) + lane;
    if constexpr (CMW > 0) {
      int fq[CMW];
      const bool last_of_run = (t == p.T - 1) || (f == f_end - 1);
#pragma unroll
      for (int q = 0; q < CMW; ++q) {
        fq[q] = lane_tab[(CMW + q) * 64 + lane];
        float acc = contrast_fwd(band_walk2k(absrow + lane_tab[q * 64 + lane], w, p.bank.pass_len[q] >> 2), p.contrast, p.eps);
        if (p.offset) acc = (acc - off) / sc;
#pragma unroll
        for (int k = 0; k < 7; ++k) cm[q][k] = cm[q][k + 1];
        cm[q][7] = acc;
        ++held[q];
        if (fq[q] >= 0) {
          if (!e_valid) e_next[q] = (b * p.bank.n_filters + fq[q]) * p.T + t + 1;   // one past frame t in this lane's row
          const long long e = e_next[q];
          e_next[q] = e + ((t == p.T - 1) ? (long long)(p.bank.n_filters - 1) * p.T + 1 : 1);
          if ((e & 7) == 0 || last_of_run) {            // whole 32-byte sectors (see mel_banded.hip)
            float* dst = p.feat + e - 8;
            if (held[q] >= 8) {
              if ((e & 3) == 0) {
                reinterpret_cast<float4*>(dst)[0] = make_float4(cm[q][0], cm[q][1], cm[q][2], cm[q][3]);
                reinterpret_cast<float4*>(dst)[1] = make_float4(cm[q][4], cm[q][5], cm[q][6], cm[q][7]);
              } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) dst[k] = cm[q][k];
              }
            } else {
#pragma unroll
              for (int k = 0; k < 8; ++k)
                if (k >= 8 - held[q]) dst[k] = cm[q][k];
            }
            held[q] = 0;
          }
        } else if (last_of_run) {
          held[q] = 0;
        }
      }
      e_valid = true;
    } else {
      for (int q = 0; q < p.bank.n_passes; ++q) {
        const int filt = lane_tab[(p.bank.n_passes + q) * 64 + lane];
        const float sum = band_walk2k(absrow + lane_tab[q * 64 + lane], w, p.bank.pass_len[q] >> 2);
        if (filt >= 0) {
          float acc = contrast_fwd(sum, p.contrast, p.eps);
          if (p.offset) acc = (acc - off) / sc;
          if (p.channel_major) p.feat[(b * p.bank.n_filters + filt) * p.T + t] = acc;
          else p.feat[f * p.bank.n_filters + filt] = acc;
        }
      }
    }
    wave_lds_sync();
  }
}

int launch_stft2048_mel(const float* x, long long B, long long L, long long clip_stride, long long T, int hop,
                        const float* window, const float2* tw, const float2* tw2k, const BandBank* bank, int contrast,
                        int power2, const float* offset, const float* scale, float eps, float* feat, int channel_major,
                        hipStream_t stream) {
  const long long nframes = B * T;
  if (nframes == 0) return 0;
  P2kMel p = {};
  p.x = x; p.window = window; p.tw = tw; p.tw2k = tw2k; p.feat = feat; p.offset = offset; p.scale = scale;
  p.L = L; p.clip_stride = clip_stride; p.T = T; p.total_frames = nframes; p.bank = *bank; p.hop = hop;
  p.contrast = contrast; p.power2 = power2; p.channel_major = channel_major; p.eps = eps;
  int max_walk = 0, table_floats = 0;
  for (int q = 0; q < bank->n_passes; ++q) {
    max_walk = bank->pass_len[q] > max_walk ? bank->pass_len[q] : max_walk;
    table_floats += 64 * bank->pass_len[q];
  }
  p.table_floats = table_floats;
  p.row_floats = (F2K + max_walk + 63) / 64 * 64;      // a walk that starts on the last bins runs into zeros
  size_t lds = sizeof(float2) * (size_t)(W2K * kFftLdsFloat2PerWave + kTwiddleCount + 1024) +
               sizeof(float) * ((size_t)W2K * p.row_floats + table_floats) + sizeof(int) * (size_t)2 * 64 * bank->n_passes;
  if (lds > 80 * 1024) return AT_EUNSUPPORTED;                       // two workgroups per CU or not at all
  lds = (lds + 15) / 16 * 16;
  const bool winlds = lds + 8192 <= 80 * 1024;          // the analysis window (512 float4) too, when it fits
  if (winlds) {
    p.win_off_f2 = (int)(lds / sizeof(float2));
    lds += 8192;
  }
  // runs of consecutive frames per wave: long enough for the window and the table staging, short enough to fill the chip
  long long fpw = (nframes + 256LL * 8 * W2K - 1) / (256LL * 8 * W2K);
  if (fpw < 8) fpw = 8;
  if (const long long forced = forced_row_run(nframes)) fpw = forced;    // AT_VARIANT_ROW_RUN (tests)
  p.frames_per_wave = fpw;
  const long long waves = (nframes + fpw - 1) / fpw;
  const unsigned grid = (unsigned)((waves + W2K - 1) / W2K);
  void (*kernel)(P2kMel) = winlds ? stft2048_mel_kernel<0, true> : stft2048_mel_kernel<0, false>;
  if (channel_major && bank->n_passes == 1) kernel = winlds ? stft2048_mel_kernel<1, true> : stft2048_mel_kernel<1, false>;
  else if (channel_major && bank->n_passes == 2) kernel = winlds ? stft2048_mel_kernel<2, true> : stft2048_mel_kernel<2, false>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return AT_ELAUNCH;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * W2K), lds, stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int launch_istft2048_ola(const float2* X, const float* mag, const float* phase, long long B, long long T, int hop,
                         const float* window, const float* env, const float2* tw, const float2* tw2k, float* y,
                         hipStream_t stream) {
  static void (*const kernels[2][3])(POla) = {
      {istft2048_ola_kernel<false, 1>, istft2048_ola_kernel<false, 2>, istft2048_ola_kernel<false, 4>},
      {istft2048_ola_kernel<true, 1>, istft2048_ola_kernel<true, 2>, istft2048_ola_kernel<true, 4>}};
  return launch_istft_ola(kernels, N2K, W2K, X, mag, phase, B, T, hop, window, env, tw, tw2k, y, stream);
}

int launch_stft2048_fwd(const float* x, long long B, long long L, long long clip_stride, long long T, int hop, int center,
                        const float* window, const float2* tw, const float2* tw2k, float2* out, float* phase,
                        hipStream_t stream) {
  const long long nframes = B * T;
  if (nframes == 0) return 0;
  PFrames p = {};
  p.x = x; p.window = window; p.tw = tw; p.tw_n = tw2k; p.X = out; p.phase_out = phase;
  p.L = L; p.clip_stride = clip_stride; p.T = T; p.total_frames = nframes; p.hop = hop; p.center = center;
  // the sliding-window / aligned-stream kernel: torch.stft's framing at hop n/4, 16-byte aligned clips, a 512-byte
  // aligned output (torch allocations are), no phase side output
  if (center && hop == 512 && !phase && L >= 2048 && (clip_stride & 3) == 0 && (((uintptr_t)x) & 15) == 0 &&
      (((uintptr_t)out) & 511) == 0 && (((uintptr_t)window) & 15) == 0 && variant(kVarFrameKernels) == 0) {
    return launch_run_fwd(stft2048_run_fwd_kernel, W2KR, T, {x, window, tw, tw2k, out, B, L, clip_stride, T, 0, 0}, stream);
  }
  static void (*const kernels[2])(PFrames) = {stft2048_fwd_kernel<false>, stft2048_fwd_kernel<true>};
  return launch_frames(kernels, phase != nullptr, W2K, p, stream);
}

int launch_irfft2048_frames(const float2* X, const float* mag, const float* phase, long long nframes, const float* window,
                            const float2* tw, const float2* tw2k, float* frames, hipStream_t stream) {
  if (nframes == 0) return 0;
  PFrames p = {};
  p.X = const_cast<float2*>(X); p.mag = mag; p.phase = phase; p.window = window; p.tw = tw; p.tw_n = tw2k; p.y = frames;
  p.total_frames = nframes;
  static void (*const kernels[2])(PFrames) = {irfft2048_frames_kernel<false>, irfft2048_frames_kernel<true>};
  return launch_frames(kernels, X == nullptr, W2K, p, stream);
}

}  // namespace at_hip

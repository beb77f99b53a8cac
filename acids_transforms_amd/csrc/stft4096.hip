// stft4096.hip -- n_fft = 4096 on the one-wavefront register FFT core (fft512.h).
//
// Replaces, for n_fft = 4096 (any hop):
//   torch.stft(...).transpose(-2,-1)          reference transforms/stft.py:98-104, dgt.py:64-70
//   torch.fft.rfft(x*window) on frames        stft.py:249-253, dgt.py:285-289
//   torch.fft.irfft(X) * inv_window           stft.py:260-266, dgt.py:296-302; the frames of torch.istft
//                                             (stft.py:120-128), overlap-added by stft_generic.hip's gather
// Until this file the size ran on the workgroup-per-frame LDS Stockham kernel of stft_generic.hip (~1.3 TB/s).
//
// A 4096-point real transform is a 2048-point complex FFT of z[n] = x[2n] + i x[2n+1] plus the real split; the
// 2048-point FFT is four 512-point FFTs (the wave-level radix-8 core: 8 complex points per lane) of the samples
// z[4m + r], r = 0..3, plus one radix-4 stage:
//   z_r[m] = z[4m + r] = x[8m + 2r] + i x[8m + 2r + 1]     -> two float4 loads per lane and register hold
//                                                              (z0, z1) and (z2, z3) of the same m
//   Z[k + 512 q] = sum_r (-i)^(r q) W2048^(r k) Z_r[k],  k = lane + 64 m  (lane-local: registers m + 8 q)
//   X[k] = (Z[k] + conj Z[2048-k])/2 - (i/2) W4096^k (Z[k] - conj Z[2048-k]),  k = 0 .. 2048
// The mirror partner Z[2048-k] lives in lane 64-lane, register 31-m (lane 0: its own register 32-m).  The inverse
// runs the same steps backwards.  One wave = one frame at a time, frames of a block interleaved over its four waves.
//
// Each direction's arithmetic is written once: fwd_core4k (four FFTs, radix-4, mirror, merge; plain or with rotated
// output columns) serves the frame and the run kernel, inv_core4k (radix-4 backwards, four FFTs) behind fft512.h's
// load_spectrum_row / irfft_presplit serves the frames and the fused overlap-add kernel (ola_window.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "fastmath.h"
#include "fft512.h"
#include "ola_window.h"
#include "row_stream.h"
#include "run_plan.h"
#include "stft_launch.h"
#include "variants.h"
#include <stdlib.h>

namespace at_hip {

constexpr int N4K = 4096;
constexpr int F4K = N4K / 2 + 1;     // 2049
constexpr int W4K = 4;               // waves per block
constexpr int kTab4k = kSideTableCount - kSide4096;   // the n_fft-4096 block of the side table (stft_launch.h)

// (qa[j], qb[j]) = x[s + 8 (lane + 64 j) .. + 7] of frame f (reflect padding with center, zero padding without)
__device__ __forceinline__ void load_frame4k(const PFrames& p, long long f, int lane, float4 (&qa)[8], float4 (&qb)[8]) {
  const long long b = f / p.T, t = f - b * p.T;
  const float* clip = p.x + b * p.clip_stride;
  const long long start = t * (long long)p.hop - (p.center ? N4K / 2 : 0);
  const bool interior = (start >= 0) && (start + N4K <= p.L);
  if (interior && ((((uintptr_t)(clip + start)) & 15) == 0)) {
    const float4* src = reinterpret_cast<const float4*>(clip + start);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      qa[j] = src[2 * (lane + 64 * j)];
      qb[j] = src[2 * (lane + 64 * j) + 1];
    }
  } else if (interior) {
    const float* src = clip + start;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = 8 * (lane + 64 * j);
      qa[j] = make_float4(src[i], src[i + 1], src[i + 2], src[i + 3]);
      qb[j] = make_float4(src[i + 4], src[i + 5], src[i + 6], src[i + 7]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long i0 = start + 8 * (lane + 64 * j);
      float v[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const long long i = i0 + c;
        if (p.center) v[c] = clip[reflect_index(i, p.L)];
        else v[c] = (i >= 0 && i < p.L) ? clip[i] : 0.0f;     // zero padding past the end (utils/misc.py:156)
      }
      qa[j] = make_float4(v[0], v[1], v[2], v[3]);
      qb[j] = make_float4(v[4], v[5], v[6], v[7]);
    }
  }
}

// Constant tables in LDS, shared by the block's four waves: the fft512 twiddles (11 KB), W4096^k (16 KB; halved in the
// forward kernel: the real split wants W / 2) and the radix-4 twiddles W2048^(r k) (12 KB).
template <bool INV>
__device__ __forceinline__ void stage_tables4k(const float2* tw, const float2* tw4k, float2* tab, float2* t4) {
  for (int i = threadIdx.x; i < kTwiddleCount; i += 64 * W4K) tab[i] = tw[i];
  for (int i = threadIdx.x; i < kTab4k; i += 64 * W4K) {
    float2 a = tw4k[i];
    if (!INV && i < 2048) a = make_float2(0.5f * a.x, 0.5f * a.y);
    t4[i] = a;
  }
  __syncthreads();
}

constexpr int kLds4k = W4K * kFftLdsFloat2PerWave + kTwiddleCount + kTab4k;

// a frame's raw samples times the window (global memory or LDS) -> the inputs y[r] of the four 512-point FFTs
__device__ __forceinline__ void window4k(const float4 (&qa)[8], const float4 (&qb)[8], const float4* win, int lane,
                                         v2f (&y)[4][8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float4 wa = win[2 * (lane + 64 * j)];
    const float4 wb = win[2 * (lane + 64 * j) + 1];
    y[0][j] = (v2f){qa[j].x * wa.x, qa[j].y * wa.y};
    y[1][j] = (v2f){qa[j].z * wa.z, qa[j].w * wa.w};
    y[2][j] = (v2f){qb[j].x * wb.x, qb[j].y * wb.y};
    y[3][j] = (v2f){qb[j].z * wb.z, qb[j].w * wb.w};
  }
}

// The forward core: the windowed samples y[r][m] = z[4 (lane + 64 m) + r] -> out(m, X[col + 64 m]), m = 0 .. 31, in that
// order; returns X[2048] (real; meaningful on the lane whose column is 0).  t4: the staged n_fft-4096 tables.  The run
// kernel rotates the output columns over the lanes: this lane holds column col = (lane - rot) & 63 (the radix-4 stage is
// lane-local; its twiddles, the merge's and the mirror lane follow the column); the frame kernel passes rot = 0, col = lane.
// The bins go to a consumer, not to an array: a kernel that stores or reduces them does so inside the merge loop, as the
// kernels did before they shared this core, and keeps their register count (profiles/nfft_cores.md).
template <typename OUT>
__device__ __forceinline__ float fwd_core4k(v2f (&y)[4][8], const LdsTwiddles<false>& tw, const float2* t4, float2* lds,
                                            int lane, int rot, int col, OUT&& out) {
  const v2f hh = {0.5f, 0.5f};
#pragma unroll
  for (int r = 0; r < 4; ++r) fft512<false>(y[r], tw, lds, lane, col);
  const v2f* wh = reinterpret_cast<const v2f*>(t4) + col;            // wh[64 m] = W4096^(col + 64 m) / 2
  const v2f* wr = reinterpret_cast<const v2f*>(t4 + 2048) + col;     // wr[(r - 1) 512 + 64 m] = W2048^(r (col + 64 m))
  // radix-4: registers m, m + 8, m + 16, m + 24 hold Z[k], Z[k + 512], Z[k + 1024], Z[k + 1536]
  v2f z[32];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const v2f t1 = cmul_v(y[1][m], wr[64 * m]);
    const v2f t2 = cmul_v(y[2][m], wr[512 + 64 * m]);
    const v2f t3 = cmul_v(y[3][m], wr[1024 + 64 * m]);
    const v2f a = y[0][m] + t2, b = y[0][m] - t2, c = t1 + t3, d = t1 - t3;
    z[m] = a + c;
    z[m + 16] = a - c;
    z[m + 8] = add_mi(b, d);        // b - i d
    z[m + 24] = add_pi(b, d);       // b + i d
  }
  v2f pm[32];
  mirror_regs_rot<32>(z, pm, lane, rot, col);
  // X[k] = (Z[k] + conj Z')/2 - i (W4096^k / 2) (Z[k] - conj Z'),  Z' = Z[2048 - k]  (k = 0: Z' = Z[0], X[0] real)
  const float nyq = z[0].x - z[0].y;                                // X[2048] = Re Z[0] - Im Z[0]
#pragma unroll
  for (int m = 0; m < 32; ++m) {
    const v2f e = add_conj(z[m], pm[m]);
    const v2f d = sub_conj(z[m], pm[m]);
    out(m, scale_add_mi(e, hh, cmul_v(d, wh[64 * m])));             // e / 2 - i (W / 2) d
  }
  return nyq;
}

template <bool WRITE_PHASE>
__global__ __launch_bounds__(64 * W4K, 2) void stft4096_fwd_kernel(PFrames p) {
  __shared__ float2 lds_all[kLds4k];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W4K * kFftLdsFloat2PerWave;
  float2* t4 = tab + kTwiddleCount;
  stage_tables4k<false>(p.tw, p.tw_n, tab, t4);
  const LdsTwiddles<false> tw = {tab, lane};
  const long long f_begin = (long long)blockIdx.x * p.frames_per_block;
  long long f_end = f_begin + p.frames_per_block;
  if (f_end > p.total_frames) f_end = p.total_frames;
  const float4* win4 = reinterpret_cast<const float4*>(p.window);     // L2-resident (16 KB), re-read per frame

  long long f = f_begin + wave;
  float4 na[8], nb[8];
  if (f < f_end) load_frame4k(p, f, lane, na, nb);
  for (; f < f_end; f += W4K) {
    v2f y[4][8];
    window4k(na, nb, win4, lane, y);
    if (f + W4K < f_end) load_frame4k(p, f + W4K, lane, na, nb);
    float2* row = p.X + f * F4K;
    float* prow = WRITE_PHASE ? p.phase_out + f * F4K : nullptr;
    const float nyq = fwd_core4k(y, tw, t4, lds, lane, 0, lane, [&](int m, v2f xk) {
      row[lane + 64 * m] = to_f2(xk);
      if (WRITE_PHASE) prow[lane + 64 * m] = fast_atan2f(xk.y, xk.x);
    });
    if (lane == 0) {
      row[2048] = make_float2(nyq, 0.0f);
      if (WRITE_PHASE) prow[2048] = fast_atan2f(0.0f, nyq);
    }
  }
}


// ---------------------------------------------------------------------------
// forward, hop = 1024 = N/4, center = True: sliding window in registers + aligned stream stores (round 3; the scheme of
// stft1024.hip's AL kernel and stft2048.hip's run kernel).  Register slot j of a lane holds x[s + 8 (lane + 64 j) .. + 7]
// (two float4): the next frame is "slots j + 2 of the same lane", so the raw samples stay in registers and only the
// 1024 new samples (four 16-byte loads per lane) are fetched per frame -- 4 KB instead of 16 KB.  The spectrum leaves
// through the aligned row stream of row_stream.h (NB = 32: 32 full-block non-temporal stores per frame): the output
// columns of the four 512-point FFTs are rotated over the lanes, the radix-4 stage is lane-local, the twiddles of the
// radix-4 stage and of the merge and the mirror lane follow the column.
// ---------------------------------------------------------------------------

// 512 samples (one register slot of the wave) starting at original index i0 of the clip, reflect-padded
__device__ __forceinline__ void load_slot4k(const float* clip, long long L, long long i0, int lane, float4& a, float4& b) {
  const long long i = i0 + 8 * lane;
  if (i0 >= 0 && i0 + 512 <= L) {                                 // clip base 16-byte aligned (launcher)
    a = *reinterpret_cast<const float4*>(clip + i);
    b = *reinterpret_cast<const float4*>(clip + i + 4);
    return;
  }
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = clip[reflect_index(i + c, L)];
  a = make_float4(v[0], v[1], v[2], v[3]);
  b = make_float4(v[4], v[5], v[6], v[7]);
}

constexpr int kLds4kRun = kLds4k + 2048;          // + the analysis window (1024 float4)

__global__ __launch_bounds__(64 * W4K, 2) void stft4096_run_fwd_kernel(PRunFwd p) {
  __shared__ float2 lds_all[kLds4kRun];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W4K * kFftLdsFloat2PerWave;
  float2* t4 = tab + kTwiddleCount;
  float4* wintab = reinterpret_cast<float4*>(t4 + kTab4k);
  for (int i = threadIdx.x; i < 1024; i += 64 * W4K) wintab[i] = reinterpret_cast<const float4*>(p.window)[i];
  stage_tables4k<false>(p.tw, p.tw_n, tab, t4);       // ends with __syncthreads()

  const long long run = (long long)blockIdx.x * W4K + wave, b = run / p.runs_per_clip;
  if (b >= p.B) return;
  long long t0, t1;
  if (!run_units(run - b * p.runs_per_clip, p.units_per_run, p.T, t0, t1)) return;
  const float* clip = p.x + b * p.clip_stride;
  const long long L = p.L;
  const LdsTwiddles<false> tw = {tab, lane};

  float4 ra[8], rb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) load_slot4k(clip, L, t0 * 1024 - 2048 + 512 * j, lane, ra[j], rb[j]);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    asm volatile("" : "+v"(ra[j].x), "+v"(ra[j].y), "+v"(ra[j].z), "+v"(ra[j].w));
    asm volatile("" : "+v"(rb[j].x), "+v"(rb[j].y), "+v"(rb[j].z), "+v"(rb[j].w));
  }

  RowStream<32, v2f> out;
  out.begin(reinterpret_cast<v2f*>(p.X), (b * p.T + t0) * F4K, lane);

  auto frame_body = [&](const float4 (&fa)[2], const float4 (&fb)[2]) {
    wave_priority<3>();        // transform > stores, as in stft1024.hip
    v2f y[4][8], z[32];
    window4k(ra, rb, wintab, lane, y);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      ra[j] = ra[j + 2];
      rb[j] = rb[j + 2];
    }
    ra[6] = fa[0]; rb[6] = fb[0];
    ra[7] = fa[1]; rb[7] = fb[1];
    const v2f nyq = {fwd_core4k(y, tw, t4, lds, lane, out.rot, (lane - out.rot) & 63, [&](int m, v2f xk) { z[m] = xk; }), 0.0f};
    wave_priority<1>();
    out.emit(z, nyq, lane);
    wave_priority<0>();
  };

  long long t = t0;
  long long t_fast_end = (L >= 3072) ? (L - 3072) / 1024 + 1 : 0;     // first t whose successor's new samples need reflection
  if (t_fast_end > t1 - 1) t_fast_end = t1 - 1;
  if (t < t_fast_end) {
    const float4* nsrc = reinterpret_cast<const float4*>(clip + t * 1024 + 2048) + 2 * lane;
    for (; t < t_fast_end; ++t) {
      float4 fa[2], fb[2];
      fa[0] = nsrc[0];   fb[0] = nsrc[1];
      fa[1] = nsrc[128]; fb[1] = nsrc[129];
      nsrc += 256;
      frame_body(fa, fb);
    }
  }
  for (; t < t1; ++t) {
    float4 fa[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    float4 fb[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (t + 1 < t1) {
      load_slot4k(clip, L, t * 1024 + 2048, lane, fa[0], fb[0]);
      load_slot4k(clip, L, t * 1024 + 2560, lane, fa[1], fb[1]);
    }
    frame_body(fa, fb);
  }
  out.end(lane);
}

// The inverse core: v[m] = Z[lane + 64 m] of irfft_presplit<32> (fft512.h) -> the unnormalised time samples,
// (y[0][j], .., y[3][j]) = x[8 n .. 8 n + 7], n = lane + 64 j -- the radix-4 stage backwards and the four 512-point FFTs.
// wr[(r - 1) 512 + 64 m] = W2048^(r (lane + 64 m)).
__device__ __forceinline__ void inv_core4k(const v2f (&v)[32], const LdsTwiddles<true>& tw, const v2f* wr, float2* lds,
                                           int lane, v2f (&y)[4][8]) {
  // radix-4 backwards: y_r[k] = conj(W2048^(r k)) sum_q (+i)^(r q) Z[k + 512 q]
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const v2f a = v[m] + v[m + 16], b = v[m] - v[m + 16], c = v[m + 8] + v[m + 24], d = v[m + 8] - v[m + 24];
    y[0][m] = a + c;
    y[2][m] = cmul_conj_v(a - c, wr[512 + 64 * m]);
    y[1][m] = cmul_conj_v(add_pi(b, d), wr[64 * m]);          // b + i d
    y[3][m] = cmul_conj_v(add_mi(b, d), wr[1024 + 64 * m]);   // b - i d
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) fft512<true>(y[r], tw, lds, lane);
}

// irfft(X) * window, frames out (the overlap-add is stft_generic.hip's gather): complex or polar input
template <bool POLAR>
__global__ __launch_bounds__(64 * W4K, 2) void irfft4096_frames_kernel(PFrames p) {
  __shared__ float2 lds_all[kLds4k];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W4K * kFftLdsFloat2PerWave;
  float2* t4 = tab + kTwiddleCount;
  const v2f* w4 = reinterpret_cast<const v2f*>(t4) + lane;            // w4[64 m] = W4096^(lane + 64 m)
  const v2f* wr = reinterpret_cast<const v2f*>(t4 + 2048) + lane;
  stage_tables4k<true>(p.tw, p.tw_n, tab, t4);
  const LdsTwiddles<true> tw = {tab, lane};
  const long long f_begin = (long long)blockIdx.x * p.frames_per_block;
  long long f_end = f_begin + p.frames_per_block;
  if (f_end > p.total_frames) f_end = p.total_frames;
  const float4* win4 = reinterpret_cast<const float4*>(p.window);
  const float scale = 1.0f / 4096.0f;             // the split's factor 2 is in here
  for (long long f = f_begin + wave; f < f_end; f += W4K) {
    v2f v[32], z[32], y[4][8];
    float nyq_re;
    load_spectrum_row<32, POLAR>(p.X, p.mag, p.phase, f * F4K, lane, v, nyq_re);
    irfft_presplit<32, 64>(v, nyq_re, lane, w4, z);
    inv_core4k(z, tw, wr, lds, lane, y);
    float4* dst = reinterpret_cast<float4*>(p.y + f * N4K);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 wa = win4[2 * (lane + 64 * j)];
      const float4 wb = win4[2 * (lane + 64 * j) + 1];
      dst[2 * (lane + 64 * j)] = make_float4(y[0][j].x * (wa.x * scale), y[0][j].y * (wa.y * scale),
                                             y[1][j].x * (wa.z * scale), y[1][j].y * (wa.w * scale));
      dst[2 * (lane + 64 * j) + 1] = make_float4(y[2][j].x * (wb.x * scale), y[2][j].y * (wb.y * scale),
                                                 y[3][j].x * (wb.z * scale), y[3][j].y * (wb.w * scale));
    }
  }
}

// ---------------------------------------------------------------------------
// torch.istft for n_fft = 4096, hop = 512 / 1024 / 2048 in one kernel: irfft + window + overlap-add + envelope
// (reference stft.py:120-128, dgt.py:86-93; polar input: stft.py:157-161, dgt.py:152-154).  The inverse core above into
// the register window of ola_window.h, two float4 per lane and 512-sample slot.
// ---------------------------------------------------------------------------
template <bool POLAR, int HS>
__global__ __launch_bounds__(64 * W4K, 2) void istft4096_ola_kernel(POla p) {
  constexpr int HOP = 512 * HS, R = 8 / HS, LEAD = 2048 / HOP;      // LEAD: blocks trimmed at the front
  __shared__ float2 lds_all[kLds4k + 2048];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: run bookkeeping on the scalar unit
  float2* lds = lds_all + wave * kFftLdsFloat2PerWave;
  float2* tab = lds_all + W4K * kFftLdsFloat2PerWave;
  float2* t4 = tab + kTwiddleCount;
  const v2f* w4 = reinterpret_cast<const v2f*>(t4) + lane;
  const v2f* wr = reinterpret_cast<const v2f*>(t4 + 2048) + lane;
  float4* wintab = reinterpret_cast<float4*>(t4 + kTab4k);            // 16 KB
  stage_ola_window<N4K, 64 * W4K>(p.window, wintab);
  stage_tables4k<true>(p.tw, p.tw_n, tab, t4);
  const LdsTwiddles<true> tw = {tab, lane};
  long long b, c0, c1;
  if (!ola_run_blocks(p, (long long)blockIdx.x * W4K + wave, LEAD, b, c0, c1)) return;
  const long long T = p.T;
  const float4* env4 = reinterpret_cast<const float4*>(p.env);
  float* yclip = p.y + b * (HOP * (T - 1));
  OlaWindow<HS, 2> ola;
  ola.init(env4, lane);

  for (long long t = c0 - (R - 1); t < c1; ++t) {
    if (t >= 0 && t < T) {
      v2f v[32], z[32], y[4][8];
      float nyq_re;
      load_spectrum_row<32, POLAR>(p.X, p.mag, p.phase, (b * T + t) * F4K, lane, v, nyq_re);
      irfft_presplit<32, 64>(v, nyq_re, lane, w4, z);
      inv_core4k(z, tw, wr, lds, lane, y);
      ola.add_frame(y, wintab, lane);
    }
    // block t is complete: frames t - R + 1 .. t are all that cover it
    if (t >= c0) ola.emit(yclip + (t - LEAD) * HOP, env4, ola.frame_mask(t, T), lane);
    ola.slide();
  }
}

int launch_istft4096_ola(const float2* X, const float* mag, const float* phase, long long B, long long T, int hop,
                         const float* window, const float* env, const float2* tw, const float2* tw4k, float* y,
                         hipStream_t stream) {
  static void (*const kernels[2][3])(POla) = {
      {istft4096_ola_kernel<false, 1>, istft4096_ola_kernel<false, 2>, istft4096_ola_kernel<false, 4>},
      {istft4096_ola_kernel<true, 1>, istft4096_ola_kernel<true, 2>, istft4096_ola_kernel<true, 4>}};
  return launch_istft_ola(kernels, N4K, W4K, X, mag, phase, B, T, hop, window, env, tw, tw4k, y, stream);
}

int launch_stft4096_fwd(const float* x, long long B, long long L, long long clip_stride, long long T, int hop, int center,
                        const float* window, const float2* tw, const float2* tw4k, float2* out, float* phase,
                        hipStream_t stream) {
  const long long nframes = B * T;
  if (nframes == 0) return 0;
  PFrames p = {};
  p.x = x; p.window = window; p.tw = tw; p.tw_n = tw4k; p.X = out; p.phase_out = phase;
  p.L = L; p.clip_stride = clip_stride; p.T = T; p.total_frames = nframes; p.hop = hop; p.center = center;
  // the sliding-window / aligned-stream kernel: torch.stft's framing at hop n/4, 16-byte aligned clips, a 512-byte
  // aligned output, no phase side output
  if (center && hop == 1024 && !phase && L >= 4096 && (clip_stride & 3) == 0 && (((uintptr_t)x) & 15) == 0 &&
      (((uintptr_t)out) & 511) == 0 && (((uintptr_t)window) & 15) == 0 && variant(kVarFrameKernels) == 0) {
    return launch_run_fwd(stft4096_run_fwd_kernel, W4K, T, {x, window, tw, tw4k, out, B, L, clip_stride, T, 0, 0}, stream);
  }
  static void (*const kernels[2])(PFrames) = {stft4096_fwd_kernel<false>, stft4096_fwd_kernel<true>};
  return launch_frames(kernels, phase != nullptr, W4K, p, stream);
}

int launch_irfft4096_frames(const float2* X, const float* mag, const float* phase, long long nframes, const float* window,
                            const float2* tw, const float2* tw4k, float* frames, hipStream_t stream) {
  if (nframes == 0) return 0;
  PFrames p = {};
  p.X = const_cast<float2*>(X); p.mag = mag; p.phase = phase; p.window = window; p.tw = tw; p.tw_n = tw4k; p.y = frames;
  p.total_frames = nframes;
  static void (*const kernels[2])(PFrames) = {irfft4096_frames_kernel<false>, irfft4096_frames_kernel<true>};
  return launch_frames(kernels, X == nullptr, W4K, p, stream);
}

}  // namespace at_hip

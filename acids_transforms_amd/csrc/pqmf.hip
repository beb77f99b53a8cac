// pqmf.hip -- the two kernels of the pseudo-quadrature mirror filterbank (transforms/pqmf.py, autograd.PqmfFunction /
// PqmfInvertFunction): cosine-modulated analysis of (rows, L) audio into M critically sampled bands, and the mirrored
// synthesis.  Synthesis is M x the transpose of analysis, so the pair serves forward, invert and both backward passes.
//
// With M bands, N taps (odd), P = (N - 1) / 2, h the prototype extended by zeros to Np = 2 M G taps (G = ceil(N / 2M))
// and C[k, r] = 2 cos((2k+1) pi / (2M) (r - P) + (-1)^k pi / 4) (from the host, fp32; no cosine on the device):
//   analysis    u[t, r] = sum_j (-1)^j h[r + 2Mj] x[tM + r + 2Mj - P]          r = 0 .. 2M-1   (the fold)
//               y[k, t] = scale sum_r C[k, r] u[t, r]                                          (the modulation)
//   synthesis   v[t, r] = sum_k C[k, r] y[k, t]
//               xh[bM + a] = scale sum_e sum_j (-1)^j h[n0 + eM + 2Mj] v[b + c - e - 2j, n0 + eM]      e = 0, 1
//               with n0 = (a + P) mod M and c = (a + P) div M
// x is zero outside [0, L), y outside [0, L / M).
//
// Streaming (transforms.RealtimePQMF, autograd.PqmfStreamFunction / PqmfStreamInvertFunction) is the same two kernels
// with a generalised STAGING, not other arithmetic.  A PqStream says where a call sits: the output grid lies `shift`
// blocks from the input grid (output block t is the sum above at block t + shift), and the H entries before the input
// (analysis: samples of the row; synthesis: blocks of every band) come from a state buffer instead of being zero.
// With D = ceil(P / M): shift -D with state is the causal bank delayed by D blocks (Ha = D M + P samples, Hs = D +
// floor(P / M) blocks of history are all it reads); shift +D without state is the transpose of the other kernel's
// delayed form, i.e. the streaming backward passes.  The state of the NEXT call -- the last H entries of
// [state | input] -- is written into a second buffer by the workgroup of each row's last tile, so that no tile reads
// what another one overwrites.  The offline entries pass no state and shift 0, and run a copy of the kernels compiled
// without any of this (template flag ST): run-time loop counts cost them 6 ... 10 % when the code was shared.
//
// One workgroup of 256 lanes handles a tile of TB = at_pqmf_tile_blocks(M, N) consecutive blocks t of one row: the
// signed prototype and C sit in LDS for the workgroup's whole life, the tile's window (analysis: TB M + Np - M samples;
// synthesis: the M band runs of the TB + ~N / M blocks that reach the tile) is staged with coalesced loads, kPqStage of
// them in flight per lane.  Rows and tiles are one flat 64-bit index that persistent workgroups stride over, so there
// is no row limit.  The kernels are templates on the band count: 4, 8, 16, 32 and 64 bands run a copy in which the LDS
// offsets are immediates and the index divisions shifts, every other count the general copy -- the same chains.
//
// Order of the additions.  Every u, y, v and xh is ONE fmaf chain: over j ascending (xh: e = 0 then e = 1), over r
// ascending, over k ascending.  A lane carries four chains whose blocks are two apart -- they share the window
// samples and the taps in registers (8 LDS reads for 16 FMAs) -- but each chain is its own.  The order is a function
// of (M, N) alone: not of the rows, the tile, the place in the clip, or the chunking of a stream.  No atomics.  A
// streaming tile with fewer than TB blocks left (a short chunk) runs only the groups of chains that hold a live
// block: which chains run depends on the length, never what a chain adds.
//
// LDS layouts (banking is by instruction width): the fold's lanes walk r, so window, prototype and v are read at
// consecutive dwords; u has the odd row stride 2M + 1 because the modulation's lanes walk t; C is stored (2M, M
// rounded up to 4) for analysis so that four bands of one r are one 16-byte broadcast read, and y (M, Ts rounded up to
// 4) for synthesis so that four blocks of one band are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "persistent_launch.h"
#include "stream_source.h"

namespace at_hip {

constexpr int kPqThreads = 256;
constexpr int kPqMinBand = 2, kPqMaxBand = 64, kPqMaxTaps = 4097;
constexpr size_t kPqLdsBytes = 160 * 1024;
constexpr int kPqStage = 8;      // global loads a lane has in flight while a tile is staged

__host__ __device__ static inline int pq_up4(int v) { return (v + 3) & ~3; }

// blocks of a tile: a multiple of 64 (the modulation's lanes walk t), about AT_PQ_TILE samples when the bands are few
#ifndef AT_PQ_TILE
#define AT_PQ_TILE 1024
#endif
__host__ __device__ static inline int pq_tile_blocks(int M) { return 64 * (M * 64 < AT_PQ_TILE ? AT_PQ_TILE / 64 / M : 1); }

// the plan of a (M, N): every length below is in floats
struct PqPlan {
  int M, N, P, G, Np, TB;
  int Mp;          // analysis: bands rounded up to 4 (row length of the transposed C)
  int wlen;        // analysis: window samples of a tile
  int us;          // analysis: row stride of u
  int lo, tv, ys;  // synthesis: blocks of halo before the tile, rows of v that are used, row stride of y (>= tv)
  size_t lds_analysis, lds_synthesis;
};

static inline PqPlan pq_plan(int M, int N) {
  PqPlan p;
  p.M = M; p.N = N; p.P = (N - 1) / 2;
  p.G = (N + 2 * M - 1) / (2 * M);
  p.Np = 2 * M * p.G;
  p.TB = pq_tile_blocks(M);
  p.Mp = pq_up4(M);
  p.wlen = p.TB * M + p.Np - M;
  p.us = 2 * M + 1;
  p.lo = 2 * p.G - 1 - p.P / M;
  p.tv = p.TB + (M - 1 + p.P) / M + p.lo;
  p.ys = pq_up4(p.tv);
  p.lds_analysis = sizeof(float) * ((size_t)pq_up4(p.Np) + (size_t)2 * M * p.Mp + pq_up4(p.wlen) + (size_t)p.TB * p.us);
  p.lds_synthesis = sizeof(float) * ((size_t)pq_up4(p.Np) + (size_t)pq_up4(2 * M * M) + (size_t)M * p.ys + (size_t)p.ys * 2 * M);
  return p;
}

// where a call sits in a stream (the header of this file); every offline call is {nullptr, nullptr, 0, 0}
struct PqStream {
  const float* state_in;   // (rows, H) or (rows, M, H): the H entries before the input; nullptr: zeros
  float* state_out;        // the same shape: the last H entries of [state_in | input]; nullptr: not wanted
  int H;
  int shift;               // output block t reads the input as block t + shift of the offline sums
};

// D = ceil(P / M): the blocks of delay of the causal bank
__host__ __device__ static inline int pq_delay_blocks(int M, int N) { return ((N - 1) / 2 + M - 1) / M; }

// hs[n] = (-1)^(n div 2M) h[n], zero from N on
__device__ __forceinline__ void pq_stage_proto(float* hs, const float* __restrict__ proto, int N, int Np, int M2) {
  for (int n = threadIdx.x; n < Np; n += kPqThreads) {
    const float v = n < N ? proto[n] : 0.f;
    hs[n] = ((n / M2) & 1) ? -v : v;
  }
}

// MT: the band count as a compile-time constant (LDS offsets become immediates, the divisions shifts), 0: p.M
// ST: the streaming copy reads its PqStream and bounds its loops by the tile's live blocks; the offline copy (ST false)
// has no state, shift 0 and whole-tile loop counts as constants -- the code it had before there was a streaming form
template <int MT, bool ST>
__global__ __launch_bounds__(kPqThreads) void pqmf_analysis_kernel(const float* __restrict__ x, long long L, long long T,
                                                                    long long tiles, long long units,
                                                                    const float* __restrict__ proto,
                                                                    const float* __restrict__ mod, float scale,
                                                                    float* __restrict__ y, PqPlan p, PqStream st) {
  extern __shared__ __attribute__((aligned(16))) float pq_lds[];
  const int M = MT ? MT : p.M, M2 = 2 * M, G = p.G, TB = pq_tile_blocks(M), Mp = (M + 3) & ~3, us = 2 * M + 1;
  float* hs = pq_lds;                         // Np (every array starts on a 16-byte boundary)
  float* ct = hs + pq_up4(p.Np);              // (2M, Mp): ct[r Mp + k] = C[k, r]
  float* win = ct + M2 * Mp;                  // wlen, rounded up to 4
  float* u = win + pq_up4(p.wlen);            // (TB, us)
  pq_stage_proto(hs, proto, p.N, p.Np, M2);
  for (int i = threadIdx.x; i < M2 * Mp; i += kPqThreads) {
    const int r = i / Mp, k = i - r * Mp;
    ct[i] = k < M ? mod[k * M2 + r] : 0.f;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long row = unit / tiles;
    const long long t0 = (unit - row * tiles) * TB;
    const float* xr = x + row * L;
    const long long s0 = (t0 + (ST ? st.shift : 0)) * M - p.P;        // clip sample of win[0]
    // the live blocks of the tile, in the groups of eight a pair of fold items carries, and the window they read
    const int nb = ST && T - t0 < (long long)TB ? (int)(T - t0) : TB;
    const int nsb = ST ? (nb + 7) >> 3 : TB / 8;
    const int wlive = ST ? nsb * 8 * M + p.Np - M : p.wlen;
    const float* state = ST ? st.state_in : nullptr;
    __syncthreads();                          // the tables are staged; the previous tile's u is read
    // window samples [qlo, qhi) lie inside the clip, [qs, qlo) in the carried state, the rest is zero
    const int nlo = s0 < 0 ? (int)-s0 : 0;
    const int qlo = ST && nlo > wlive ? wlive : nlo;
    const int qhi = L - s0 < (long long)wlive ? (int)(L - s0) : wlive;
    const int qs = !state ? qlo : nlo > st.H ? nlo - st.H : 0;
    const float* xw = xr + s0;
    const float* sw = state + (row + 1) * st.H + s0;      // the state's last sample is clip sample -1
    for (int q0 = threadIdx.x; q0 < wlive; q0 += kPqThreads * kPqStage) {
      float val[kPqStage];
#pragma unroll
      for (int i = 0; i < kPqStage; ++i) {      // every load of the pass is issued before the first LDS store
        const int q = q0 + i * kPqThreads;
        val[i] = (q >= qlo && q < qhi) ? xw[q] : (q >= qs && q < qlo) ? sw[q] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kPqStage; ++i) {
        const int q = q0 + i * kPqThreads;
        if (q < wlive) win[q] = val[i];
      }
    }
    if (ST && st.state_out && t0 + TB >= T) {       // the row's last tile: the last H samples of [state | chunk]
      float* so = st.state_out + row * st.H;
      const StreamSource src = {state ? state + row * st.H : nullptr, xr, L, st.H};
      for (int i = threadIdx.x; i < st.H; i += kPqThreads) so[i] = src.tail(i);
    }
    __syncthreads();
    // fold: item = (r, parity of t, group of four same-parity blocks)
    const int items = M2 * 2 * nsb;
    for (int i = threadIdx.x; i < items; i += kPqThreads) {
      const int rest = i / M2, r = i - rest * M2;
      const int tp = rest & 1, sblk = rest >> 1;
      const float* hp = hs + r;
      const float* wp = win + r + M * tp + 4 * M2 * sblk;      // X[q] = wp[q M2]; block s of the lane reads X[s + j]
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      float x0 = wp[0], x1 = wp[M2], x2 = wp[2 * M2];
      int j = 0;
#pragma unroll 2
      for (; j + 4 <= G; j += 4) {
        const float h0 = hp[j * M2], h1 = hp[(j + 1) * M2], h2 = hp[(j + 2) * M2], h3 = hp[(j + 3) * M2];
        const float x3 = wp[(j + 3) * M2], x4 = wp[(j + 4) * M2], x5 = wp[(j + 5) * M2], x6 = wp[(j + 6) * M2];
        a0 = fmaf(h0, x0, a0); a1 = fmaf(h0, x1, a1); a2 = fmaf(h0, x2, a2); a3 = fmaf(h0, x3, a3);
        a0 = fmaf(h1, x1, a0); a1 = fmaf(h1, x2, a1); a2 = fmaf(h1, x3, a2); a3 = fmaf(h1, x4, a3);
        a0 = fmaf(h2, x2, a0); a1 = fmaf(h2, x3, a1); a2 = fmaf(h2, x4, a2); a3 = fmaf(h2, x5, a3);
        a0 = fmaf(h3, x3, a0); a1 = fmaf(h3, x4, a1); a2 = fmaf(h3, x5, a2); a3 = fmaf(h3, x6, a3);
        x0 = x4; x1 = x5; x2 = x6;
      }
      for (; j < G; ++j) {
        const float h0 = hp[j * M2], x3 = wp[(j + 3) * M2];
        a0 = fmaf(h0, x0, a0); a1 = fmaf(h0, x1, a1); a2 = fmaf(h0, x2, a2); a3 = fmaf(h0, x3, a3);
        x0 = x1; x1 = x2; x2 = x3;
      }
      float* up = u + (tp + 8 * sblk) * us + r;
      up[0] = a0; up[2 * us] = a1; up[4 * us] = a2; up[6 * us] = a3;
    }
    __syncthreads();
    // modulation: a wave's item = (64 blocks, four bands); lane = block
    const int kchunks = Mp / 4, mitems = (ST ? (nb + 63) >> 6 : TB / 64) * kchunks;
    float* yr = y + row * M * T;
    for (int it = wave; it < mitems; it += kPqThreads / 64) {
      const int tc = it / kchunks, k0 = 4 * (it - tc * kchunks);
      const int tl = tc * 64 + lane;
      const float* up = u + tl * us;
      const float* cp = ct + k0;
      float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
#pragma unroll 4
      for (int r = 0; r < M2; ++r) {
        const float uv = up[r];
        const float4 c = *reinterpret_cast<const float4*>(cp + r * Mp);
        b0 = fmaf(c.x, uv, b0); b1 = fmaf(c.y, uv, b1); b2 = fmaf(c.z, uv, b2); b3 = fmaf(c.w, uv, b3);
      }
      const long long t = t0 + tl;
      if (t < T) {
        float* yp = yr + (long long)k0 * T + t;
        yp[0] = scale * b0;
        if (k0 + 1 < M) yp[T] = scale * b1;
        if (k0 + 2 < M) yp[2 * T] = scale * b2;
        if (k0 + 3 < M) yp[3 * T] = scale * b3;
      }
    }
  }
}

template <int MT, bool ST>
__global__ __launch_bounds__(kPqThreads) void pqmf_synthesis_kernel(const float* __restrict__ y, long long L, long long T,
                                                                     long long tiles, long long units,
                                                                     const float* __restrict__ proto,
                                                                     const float* __restrict__ mod, float scale,
                                                                     float* __restrict__ x, PqPlan p, PqStream st) {
  extern __shared__ __attribute__((aligned(16))) float pq_lds[];
  const int M = MT ? MT : p.M, M2 = 2 * M, G = p.G, TB = pq_tile_blocks(M), ys = p.ys;
  float* hs = pq_lds;                         // Np (every array starts on a 16-byte boundary)
  float* cm = hs + pq_up4(p.Np);              // (M, 2M) as the host gives it
  float* yl = cm + pq_up4(M * M2);                  // (M, ys): the band runs; later the tile's output (TB M <= M ys)
  float* v = yl + M * ys;                     // (ys, 2M)
  pq_stage_proto(hs, proto, p.N, p.Np, M2);
  for (int i = threadIdx.x; i < M * M2; i += kPqThreads) cm[i] = mod[i];
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long row = unit / tiles;
    const long long t0 = (unit - row * tiles) * TB;
    const float* yr = y + row * M * T;
    const long long tlo = t0 + (ST ? st.shift : 0) - p.lo;          // block of v's row 0
    // the live blocks of the tile, in the groups of eight a pair of accumulation items carries, and the rows of v
    // they read (a multiple of four: the modulation's items)
    const int nb = ST && T - t0 < (long long)TB ? (int)(T - t0) : TB;
    const int nsb = ST ? (nb + 7) >> 3 : TB / 8;
    const int ysl = ST ? pq_up4(8 * nsb + (M - 1 + p.P) / M + p.lo) : ys;
    const float* state = ST ? st.state_in : nullptr;
    __syncthreads();                          // the tables are staged; the previous tile's output is stored
    // v rows [rlo, rhi) lie inside the clip, [rs, rlo) in the carried state, the rest is zero; (k, tl) of a lane's
    // next element by steps, no division
    const int nlo = tlo < 0 ? (int)-tlo : 0;
    const int rlo = ST && nlo > ysl ? ysl : nlo;
    const int rhi = T - tlo < (long long)ysl ? (int)(T - tlo) : ysl;
    const int rs = !state ? rlo : nlo > st.H ? nlo - st.H : 0;
    const float* sr = state + row * M * st.H + st.H + tlo;      // a band's last state block is block -1
    const int dk = kPqThreads / ys, dt = kPqThreads - dk * ys;
    int k = threadIdx.x / ys, tl = threadIdx.x - k * ys;
    for (int i0 = threadIdx.x; i0 < M * ys; i0 += kPqThreads * kPqStage) {
      float val[kPqStage];
#pragma unroll
      for (int q = 0; q < kPqStage; ++q) {      // every load of the pass is issued before the first LDS store
        val[q] = (k < M && tl >= rlo && tl < rhi) ? yr[(long long)k * T + tlo + tl]
                 : (ST && k < M && tl >= rs && tl < rlo) ? sr[k * st.H + tl] : 0.f;
        k += dk; tl += dt;
        if (tl >= ys) { tl -= ys; ++k; }
      }
#pragma unroll
      for (int q = 0; q < kPqStage; ++q) {
        const int i = i0 + q * kPqThreads;
        if (i < M * ys) yl[i] = val[q];
      }
    }
    if (ST && st.state_out && t0 + TB >= T) {       // the row's last tile: the last H blocks of every band of [state | chunk]
      float* so = st.state_out + row * M * st.H;
      for (int i = threadIdx.x; i < M * st.H; i += kPqThreads) {
        const int kb = i / st.H;
        const StreamSource src = {state ? state + (row * M + kb) * st.H : nullptr, yr + (long long)kb * T, T, st.H};
        so[i] = src.tail(i - kb * st.H);
      }
    }
    __syncthreads();
    // modulation: item = (r, four blocks)
    const int vitems = M2 * (ysl / 4);
    for (int i = threadIdx.x; i < vitems; i += kPqThreads) {
      const int tg = i / M2, r = i - tg * M2;
      const float* cp = cm + r;
      const float* yp = yl + 4 * tg;
      float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {
        const float c = cp[k * M2];
        const float4 yv = *reinterpret_cast<const float4*>(yp + k * ys);
        b0 = fmaf(c, yv.x, b0); b1 = fmaf(c, yv.y, b1); b2 = fmaf(c, yv.z, b2); b3 = fmaf(c, yv.w, b3);
      }
      float* vp = v + 4 * tg * M2 + r;
      vp[0] = b0; vp[M2] = b1; vp[2 * M2] = b2; vp[3 * M2] = b3;
    }
    __syncthreads();
    // accumulation: item = (a, parity of the block, group of four same-parity blocks); the result goes over yl
    const int items = M * 2 * nsb;
    for (int i = threadIdx.x; i < items; i += kPqThreads) {
      const int rest = i / M, a = i - rest * M;
      const int bp = rest & 1, sblk = rest >> 1;
      const int c = (a + p.P) / M, n0 = a + p.P - c * M;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int e = 0; e < 2; ++e) {
        const float* hp = hs + n0 + e * M;
        // Z[q] = zp[2 q M2]: block s of the lane reads Z[s - j]
        const float* zp = v + (bp + 8 * sblk + c - e + p.lo) * M2 + n0 + e * M;
        const int st = 2 * M2;
        float w1 = zp[st], w2 = zp[2 * st], w3 = zp[3 * st];
        int j = 0;
#pragma unroll 2
        for (; j + 4 <= G; j += 4) {
          const float h0 = hp[j * M2], h1 = hp[(j + 1) * M2], h2 = hp[(j + 2) * M2], h3 = hp[(j + 3) * M2];
          const float z0 = zp[-j * st], z1 = zp[-(j + 1) * st], z2 = zp[-(j + 2) * st], z3 = zp[-(j + 3) * st];
          a0 = fmaf(h0, z0, a0); a1 = fmaf(h0, w1, a1); a2 = fmaf(h0, w2, a2); a3 = fmaf(h0, w3, a3);
          a0 = fmaf(h1, z1, a0); a1 = fmaf(h1, z0, a1); a2 = fmaf(h1, w1, a2); a3 = fmaf(h1, w2, a3);
          a0 = fmaf(h2, z2, a0); a1 = fmaf(h2, z1, a1); a2 = fmaf(h2, z0, a2); a3 = fmaf(h2, w1, a3);
          a0 = fmaf(h3, z3, a0); a1 = fmaf(h3, z2, a1); a2 = fmaf(h3, z1, a2); a3 = fmaf(h3, z0, a3);
          w1 = z3; w2 = z2; w3 = z1;
        }
        for (; j < G; ++j) {
          const float h0 = hp[j * M2], z0 = zp[-j * st];
          a0 = fmaf(h0, z0, a0); a1 = fmaf(h0, w1, a1); a2 = fmaf(h0, w2, a2); a3 = fmaf(h0, w3, a3);
          w3 = w2; w2 = w1; w1 = z0;
        }
      }
      float* op = yl + (bp + 8 * sblk) * M + a;
      op[0] = scale * a0; op[2 * M] = scale * a1; op[4 * M] = scale * a2; op[6 * M] = scale * a3;
    }
    __syncthreads();
    const long long m0 = t0 * M;
    const long long left = L - m0;
    const int n = left < (long long)TB * M ? (int)left : TB * M;
    float* xr = x + row * L + m0;
    for (int i = threadIdx.x; i < n; i += kPqThreads) xr[i] = yl[i];
  }
}

// AT_OK when there is something to launch and the arguments are sound, 1 when there is nothing to do
static int pq_check(const void* in, int64_t rows, int64_t L, const void* proto, int taps, int n_band, const void* mod,
                    const void* out) {
  if (rows == 0 || L == 0) return 1;
  if (rows < 0 || L < 0 || n_band < 1 || taps < 1) return AT_EINVAL;
  if (L % n_band != 0 || !(taps & 1) || taps < 2 * (int64_t)n_band + 1) return AT_EINVAL;
  if (n_band < kPqMinBand || n_band > kPqMaxBand || taps > kPqMaxTaps) return AT_EUNSUPPORTED;
  if (!in || !proto || !mod || !out) return AT_EINVAL;
  return AT_OK;
}

// Persistent workgroups, at most one per tile.  `pick` chooses the kernel: it is handed `run` and calls run(kernel).
template <typename Pick>
static int pq_tiles(size_t lds, const float* in, int64_t rows, int64_t L, const float* proto, const float* mod, float scale,
                    float* out, const PqPlan& p, const PqStream& st, hipStream_t stream, Pick pick) {
  if (lds > kPqLdsBytes) return AT_EUNSUPPORTED;
  const long long T = L / p.M;
  const long long tiles = (T + p.TB - 1) / p.TB;
  if (rows > 0x7fffffffffffffffLL / tiles) return AT_EUNSUPPORTED;
  const long long units = (long long)rows * tiles;
  return pick([&](auto kernel) {
    return persistent_launch(kernel, kPqThreads, lds, units, stream, in, (long long)L, T, tiles, units, proto, mod, scale,
                             out, p, st);
  });
}

// the kernel of a band count: a specialisation for the usual counts, the general one otherwise -- same sums, same bits
#define PQ_DISPATCH(kernel)              \
  switch (n_band) {                      \
    case 4: return run(kernel<4, ST>);   \
    case 8: return run(kernel<8, ST>);   \
    case 16: return run(kernel<16, ST>); \
    case 32: return run(kernel<32, ST>); \
    case 64: return run(kernel<64, ST>); \
    default: return run(kernel<0, ST>);  \
  }

template <bool ST>
static int pq_analysis(const float* in, int64_t rows, int64_t L, const float* proto, const float* mod, float scale,
                       float* out, int n_band, const PqPlan& p, const PqStream& st, hipStream_t s) {
  return pq_tiles(p.lds_analysis, in, rows, L, proto, mod, scale, out, p, st, s,
                  [&](auto run) { PQ_DISPATCH(pqmf_analysis_kernel) });
}

template <bool ST>
static int pq_synthesis(const float* in, int64_t rows, int64_t L, const float* proto, const float* mod, float scale,
                        float* out, int n_band, const PqPlan& p, const PqStream& st, hipStream_t s) {
  return pq_tiles(p.lds_synthesis, in, rows, L, proto, mod, scale, out, p, st, s,
                  [&](auto run) { PQ_DISPATCH(pqmf_synthesis_kernel) });
}
#undef PQ_DISPATCH

}  // namespace at_hip

extern "C" {

int at_pqmf_tile_blocks(int n_band, int taps) {
  using namespace at_hip;
  if (n_band < 1 || taps < 1 || !(taps & 1) || taps < 2 * (int64_t)n_band + 1) return AT_EINVAL;
  if (n_band < kPqMinBand || n_band > kPqMaxBand || taps > kPqMaxTaps) return AT_EUNSUPPORTED;
  const PqPlan p = pq_plan(n_band, taps);
  if (p.lds_analysis > kPqLdsBytes || p.lds_synthesis > kPqLdsBytes) return AT_EUNSUPPORTED;
  return p.TB;
}

int at_pqmf_analysis(const float* x, int64_t rows, int64_t L, const float* proto, int taps, int n_band, const float* mod,
                     float scale, float* y, void* stream) {
  using namespace at_hip;
  const int rc = pq_check(x, rows, L, proto, taps, n_band, mod, y);
  if (rc) return rc > 0 ? AT_OK : rc;
  const PqPlan p = pq_plan(n_band, taps);
  return pq_analysis<false>(x, rows, L, proto, mod, scale, y, n_band, p, PqStream{nullptr, nullptr, 0, 0}, (hipStream_t)stream);
}

int at_pqmf_synthesis(const float* y, int64_t rows, int64_t L, const float* proto, int taps, int n_band, const float* mod,
                      float scale, float* x, void* stream) {
  using namespace at_hip;
  const int rc = pq_check(y, rows, L, proto, taps, n_band, mod, x);
  if (rc) return rc > 0 ? AT_OK : rc;
  const PqPlan p = pq_plan(n_band, taps);
  return pq_synthesis<false>(y, rows, L, proto, mod, scale, x, n_band, p, PqStream{nullptr, nullptr, 0, 0}, (hipStream_t)stream);
}

int at_pqmf_analysis_stream(const float* x, int64_t rows, int64_t L, const float* state_in, float* state_out,
                            int shift_blocks, const float* proto, int taps, int n_band, const float* mod, float scale,
                            float* y, void* stream) {
  using namespace at_hip;
  const int rc = pq_check(x, rows, L, proto, taps, n_band, mod, y);
  if (rc) return rc > 0 ? AT_OK : rc;
  const int D = pq_delay_blocks(n_band, taps);
  if (shift_blocks < -D || shift_blocks > D || (state_out && state_out == state_in)) return AT_EINVAL;
  const PqPlan p = pq_plan(n_band, taps);
  const PqStream st = {state_in, state_out, D * n_band + p.P, shift_blocks};
  return pq_analysis<true>(x, rows, L, proto, mod, scale, y, n_band, p, st, (hipStream_t)stream);
}

int at_pqmf_synthesis_stream(const float* y, int64_t rows, int64_t L, const float* state_in, float* state_out,
                             int shift_blocks, const float* proto, int taps, int n_band, const float* mod, float scale,
                             float* x, void* stream) {
  using namespace at_hip;
  const int rc = pq_check(y, rows, L, proto, taps, n_band, mod, x);
  if (rc) return rc > 0 ? AT_OK : rc;
  const int D = pq_delay_blocks(n_band, taps);
  if (shift_blocks < -D || shift_blocks > D || (state_out && state_out == state_in)) return AT_EINVAL;
  const PqPlan p = pq_plan(n_band, taps);
  const PqStream st = {state_in, state_out, D + p.P / n_band, shift_blocks};
  return pq_synthesis<true>(y, rows, L, proto, mod, scale, x, n_band, p, st, (hipStream_t)stream);
}

}  // extern "C"

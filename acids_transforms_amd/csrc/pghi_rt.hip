// pghi_rt.hip -- realtime PGHI on gfx950: RealtimeDGT.modgabphasegrad / pghi / perform_hgi (transforms/dgt.py:338-466), one
// wavefront per stream.  The heap, its cooperative operations and the contract they keep are in pghi_heap.h.
// Compiled with -ffp-contract=off, like pghi_offline.hip.
#include "pghi_heap.h"

namespace at_hip {

// ---------------------------------------------------------------------------
// realtime: gradients on the (R = n+2, F) stack [2 history frames ; n new frames]
// (dgt.py:378-397).  The reference's uninitialised time-border rows are defined as 0.
// ---------------------------------------------------------------------------
struct RtParams {
  const float* mag_hist;    // (S, 2, F)
  const float* mag;         // (S, n, F)
  const float* prev_phase;  // (S, F)
  const float* noise;       // (S, n, F): caller's draws, or the workspace array the gradient kernel fills (seeded mode)
  float* noise_gen;         // seeded mode: where the gradient kernel writes its draws (== noise), else null
  unsigned* rng_state;      // seeded mode: {seed lo, seed hi, step counter, unused}; the heap kernel bumps the counter
  float* phase_out;         // (S, n, F)
  float* spec;              // (S, R, F) work
  float* hist;              // (S, R, F) work (untouched copy)
  float* tgradw;            // (S, R, F) work
  float* fgradw;            // (S, R, F) work
  float* phase;             // (S, R, F) work
  HeapItem* heap;           // (S, 4F + 8)
  int S, n, F, n_fft, hop;
  float gamma, tol, eps;
  int lds_floats_per_wave;  // cooperative kernel: LDS floats per stream (several streams per workgroup)
  // rank fast path (pghi_rt_rank_kernel -> pghi_hgi_rt_coop_kernel): per (stream, new frame) the 2F candidates of the
  // frame's flood -- rows f-1 and f -- sorted by magnitude: ent_of_rank[2F], rank_of_ent[2F] (u16 each), then one bit per
  // rank: "same magnitude as the rank before".  Null: heap path only.
  unsigned short* ranks;
  long long rank_stride;    // u16 elements per (stream, frame) record
  int scan_path;            // 1: try the wavefront-parallel closure (rt_scan_frame) before the rank / heap floods
};

// one record: u16 ent_of_rank[2F], u16 rank_of_ent[2F], u32 same_as_previous[ceil(2F / 32)] (bit r: the magnitude at rank r
// equals the one at rank r - 1), padded to 16 bytes
__host__ __device__ inline long long rt_rank_stride_u16(int F) {
  return ((8LL * F + 4LL * ((2 * F + 31) / 32) + 15) & ~15LL) / 2;
}

__device__ __forceinline__ float rt_mag(const RtParams& p, int s, int j, int k) {
  const float v = (j < 2) ? p.mag_hist[((long long)s * 2 + j) * p.F + k] : p.mag[((long long)s * p.n + (j - 2)) * p.F + k];
  return fmaxf(v, p.eps);
}

// Standard-normal draws for the bins at or below the tolerance (dgt.py:404-405: torch.randn_like), generated on the
// device so that a captured streaming step needs no generator launch: Philox-4x32-10 keyed by the session's seed, counter
// = (element index, step counter), Box-Muller on two of the four outputs.  Statistical parity only (the reference's
// draws are torch's; tests/test_stream_quant_gpu.py checks mean / variance / tails / step-to-step independence).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float philox_normal(unsigned long long index, unsigned step, const unsigned* state) {
  unsigned r[4];
  philox4x32_10((unsigned)index, (unsigned)(index >> 32), step, 0x5eedu, state[0], state[1], r);
  const float u1 = ((float)(r[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);    // (0, 1]
  const float u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);             // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * __builtin_amdgcn_cosf(u2);             // v_cos_f32 takes revolutions
}

__global__ __launch_bounds__(256) void pghi_grad_rt_kernel(RtParams p) {
  const float fmul = p.gamma / (float)((long long)p.hop * (long long)p.n_fft);
  const float fstep = ((float)(2.0 * 3.14159265358979323846) * (float)p.hop) / (float)p.n_fft;
  const float pi_f = (float)3.14159265358979323846;
  const int R = p.n + 2;
  const long long per = (long long)R * p.F;
  const long long total = (long long)p.S * per;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int s = (int)(i / per);
    const long long r = i - (long long)s * per;
    const int j = (int)(r / p.F), k = (int)(r - (long long)j * p.F);
    const int kr = k + 1 < p.F ? k + 1 : p.F - 1, kl = k > 0 ? k - 1 : 0;
    const float c = rt_mag(p, s, j, k);
    const float right = logf(rt_mag(p, s, j, kr));
    const float left = logf(rt_mag(p, s, j, kl));
    const float nxt = (j + 1 < R) ? logf(rt_mag(p, s, j + 1, k)) : 0.0f;
    const float prv = (j > 0) ? logf(rt_mag(p, s, j - 1, k)) : 0.0f;
    const float dxdw = (right - left) / 2.0f;                          // :393
    const float dxdt = (3.0f * nxt - 4.0f * logf(c) + prv) / 2.0f;     // :394
    p.fgradw[i] = dxdw / fmul + fstep * (float)k;                      // :395
    p.tgradw[i] = (-fmul) * dxdt + pi_f;                               // :396
    p.spec[i] = c;
    p.hist[i] = c;
    if (p.noise_gen && j >= 2)      // one draw per new bin (rows 2 .. n + 1), same indexing as a caller-supplied array
      p.noise_gen[(long long)s * p.n * p.F + (long long)(j - 2) * p.F + k] =
          philox_normal((unsigned long long)s * p.n * p.F + (unsigned long long)(j - 2) * p.F + k, p.rng_state[2], p.rng_state);
  }
}

// ---- what the realtime kernels share ---------------------------------------------------------------------------
// the next step draws from a new counter (the gradient kernel has finished)
__device__ __forceinline__ void rt_bump_step(const RtParams& p) {
  if (p.rng_state && blockIdx.x == 0 && threadIdx.x == 0) p.rng_state[2] += 1u;
}

// :400 abstol = clamp(tol * max(spec), eps) over the stream's whole (R, F) stack
__device__ __forceinline__ float rt_abstol(const float* spec, long long n, int lane, float tol, float eps) {
  float smax = -1.0f;
  for (long long i = lane; i < n; i += 64) smax = fmaxf(smax, spec[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) smax = fmaxf(smax, __shfl_xor(smax, o, 64));
  const float abstol = tol * smax;
  return abstol < eps ? eps : abstol;
}

// LDS written by some lanes of the wave, read by others
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float ufloat(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// The rows one frame step (dgt.py:413-465, frame f) touches: LDS buffers refilled every frame, or pointers into the
// stream's global arrays set once per frame.  The reference front-pads the gradients with two zero rows (:408-410): its gradient row r is
// row r - 2 of tgradw / fgradw, and tg0 of the first frame (f = 2) is a row of zeros.
struct RtRows {
  float* srow;        // spectrogram row f: the flood marks visited bins (<- abstol)
  const float* hrow;  // untouched row f-1 (spectrogram_history, dgt.py:411)
  const float* ph0;   // phase row f-1
  float* ph1;         // phase row f
  const float* tg0;   // padded tgradw row f-1; null: zeros
  const float* tg1;   // padded tgradw row f
  const float* fg1;   // padded fgradw row f
};

// The flood of one frame by a single lane (lane 0 of the caller) with the single-lane heap: seed, push row f-1, pop,
// propagate in time, propagate up and down in frequency, reseed.  `max_val` at bin `max_k` is the maximum of row f.
// An entry's index is k for bin k of row f-1 and F + k for bin k of row f, whatever the rows' storage (and not the bin's
// offset in the stream's arrays): the heap compares keys only (heapq.py:9-59 on HeapItem::key), the index is payload, so
// the pop order -- and with it every phase bit -- does not depend on how the index is encoded.
__device__ __forceinline__ void rt_serial_flood(const RtRows& R, HeapItem* heap, int F, float abstol, float max_val, int max_k) {
  int hn = 0;
  heap[0].key = -max_val;  // :427 the seed is NOT marked visited
  heap[0].idx = F + max_k;
  hn = 1;
  for (int k = 0; k < F; ++k) {  // :428-430
    const float hv = R.hrow[k];
    if (hv > abstol) h_push(heap, hn, -hv, k);
  }
  while (max_val > abstol) {  // :433
    while (hn > 0) {
      const HeapItem it = h_pop(heap, hn);
      const bool cur_row = it.idx >= F;
      const int k = cur_row ? it.idx - F : it.idx;
      if (!cur_row) {  // :436-443 propagate in time
        const float sv = R.srow[k];
        if (sv > abstol) {
          R.ph1[k] = R.ph0[k] + 0.5f * ((R.tg0 ? R.tg0[k] : 0.0f) + R.tg1[k]);
          h_push(heap, hn, -sv, F + k);
          R.srow[k] = abstol;
        }
      } else {  // :444-460 propagate in frequency
        if (k + 1 < F) {
          const float sv = R.srow[k + 1];
          if (sv > abstol) {
            R.ph1[k + 1] = R.ph1[k] + 0.5f * (R.fg1[k] + R.fg1[k + 1]);
            h_push(heap, hn, -sv, F + k + 1);
            R.srow[k + 1] = abstol;
          }
        }
        if (k - 1 > 0) {  // bin 0 is never reached downward (:453)
          const float sv = R.srow[k - 1];
          if (sv > abstol) {
            R.ph1[k - 1] = R.ph1[k] - 0.5f * (R.fg1[k] + R.fg1[k - 1]);
            h_push(heap, hn, -sv, F + k - 1);
            R.srow[k - 1] = abstol;
          }
        }
      }
    }
    // :461-465 reseed inside the frame
    max_val = R.srow[0];
    int mk = 0;
    for (int k = 1; k < F; ++k)
      if (R.srow[k] > max_val) {
        max_val = R.srow[k];
        mk = k;
      }
    h_push(heap, hn, -max_val, F + mk);
    R.srow[mk] = abstol;
  }
}

// dgt.py:399-466, one wave per stream, everything in global memory: rows of any length (the product path of the rows
// that do not fit the LDS kernels, n_fft 4096 included)
__global__ __launch_bounds__(64) void pghi_hgi_rt_kernel(RtParams p) {
  rt_bump_step(p);
  const int s = blockIdx.x;
  if (s >= p.S) return;
  const int lane = threadIdx.x;
  const int F = p.F, R = p.n + 2;
  const long long n = (long long)R * F;
  float* spec = p.spec + (long long)s * n;
  const float* hist = p.hist + (long long)s * n;
  const float* tgw = p.tgradw + (long long)s * n;
  const float* fgw = p.fgradw + (long long)s * n;
  float* phase = p.phase + (long long)s * n;
  HeapItem* heap = p.heap + (long long)s * (4LL * F + 8);
  const float abstol = rt_abstol(spec, n, lane, p.tol, p.eps);

  // :402-405 initial phase: row 0 zeros, row 1 previous phase, rows >= 2 zero above abstol else noise
  for (long long i = lane; i < n; i += 64) {
    float v;
    if (i < F) v = 0.0f;
    else if (i < 2LL * F) v = p.prev_phase[(long long)s * F + (i - F)];
    else v = (spec[i] > abstol) ? 0.0f : p.noise[(long long)s * p.n * F + (i - 2LL * F)];
    phase[i] = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __threadfence_block();

  for (int f = 2; f < R; ++f) {  // :413
    const RtRows rows = {spec + (long long)f * F,        hist + (long long)(f - 1) * F,
                         phase + (long long)(f - 1) * F, phase + (long long)f * F,
                         f >= 3 ? tgw + (long long)(f - 3) * F : nullptr,
                         tgw + (long long)(f - 2) * F,   fgw + (long long)(f - 2) * F};
    float max_val = -1.0f;
    long long max_k = F;
    for (int k = lane; k < F; k += 64) {
      const float v = rows.srow[k];
      if (v > max_val) {
        max_val = v;
        max_k = k;
      }
    }
    wave_argmax(max_val, max_k);
    if (max_val <= abstol) continue;  // :416-417
    if (lane == 0) rt_serial_flood(rows, heap, F, abstol, max_val, (int)max_k);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __threadfence_block();
  }
  for (long long i = lane; i < (long long)p.n * F; i += 64) p.phase_out[(long long)s * p.n * F + i] = phase[2LL * F + i];
}

// Same algorithm with the per-frame state in LDS: a frame's heap holds at most ~2F entries and touches only
// two rows of each array, so the whole frame step runs out of the CU's LDS (one wave per stream, F <= 1025).
__global__ __launch_bounds__(64) void pghi_hgi_rt_lds_kernel(RtParams p) {
  rt_bump_step(p);
  extern __shared__ __attribute__((aligned(16))) float rt_smem[];
  const int s = blockIdx.x;
  if (s >= p.S) return;
  const int lane = threadIdx.x;
  const int F = p.F, R = p.n + 2;
  const long long n = (long long)R * F;
  const float* spec = p.spec + (long long)s * n;
  const float* tgw = p.tgradw + (long long)s * n;
  const float* fgw = p.fgradw + (long long)s * n;
  float* phase = p.phase + (long long)s * n;
  float* srow = rt_smem;       // the seven rows of RtRows, in its order
  float* hrow = srow + F;
  float* ph0 = hrow + F;
  float* ph1 = ph0 + F;
  float* tg0 = ph1 + F;        // (= rows f-3, f-2 of the unpadded array, or 0)
  float* tg1 = tg0 + F;
  float* fg1 = tg1 + F;
  const RtRows rows = {srow, hrow, ph0, ph1, tg0, tg1, fg1};
  HeapItem* heap = reinterpret_cast<HeapItem*>(fg1 + F + (F & 1));
  const float abstol = rt_abstol(spec, n, lane, p.tol, p.eps);

  for (int k = lane; k < F; k += 64) {  // :402-403 rows 0 and 1 of the phase array
    phase[k] = 0.0f;
    phase[F + k] = p.prev_phase[(long long)s * F + k];
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");

  for (int f = 2; f < R; ++f) {  // :413
    float max_val = -1.0f;
    long long max_k = F;
    for (int k = lane; k < F; k += 64) {
      const float v = spec[(long long)f * F + k];
      srow[k] = v;
      hrow[k] = spec[(long long)(f - 1) * F + k];
      ph0[k] = phase[(long long)(f - 1) * F + k];
      ph1[k] = (v > abstol) ? 0.0f : p.noise[(long long)s * p.n * F + (long long)(f - 2) * F + k];  // :404-405
      tg0[k] = (f - 1 >= 2) ? tgw[(long long)(f - 3) * F + k] : 0.0f;  // :408-410 two-row front padding
      tg1[k] = tgw[(long long)(f - 2) * F + k];
      fg1[k] = fgw[(long long)(f - 2) * F + k];
      if (v > max_val) {
        max_val = v;
        max_k = k;
      }
    }
    wave_argmax(max_val, max_k);
    __syncthreads();
    if (max_val > abstol && lane == 0) rt_serial_flood(rows, heap, F, abstol, max_val, (int)max_k);  // :416-417
    __syncthreads();
    for (int k = lane; k < F; k += 64) {
      const float v = ph1[k];
      phase[(long long)f * F + k] = v;
      p.phase_out[(long long)s * p.n * F + (long long)(f - 2) * F + k] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    __syncthreads();
  }
}

#ifdef AT_DEV_SWITCHES
__device__ unsigned g_rt_stats[8];     // dev builds: frames, scan successes, resolution rounds, declined: reseed / tie
#define RT_STAT(i, v) do { if (lane == 0) atomicAdd(&g_rt_stats[i], (unsigned)(v)); } while (0)
#else
#define RT_STAT(i, v) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------------------------
// Realtime flood of ONE frame without a queue (round 5): the wavefront-parallel closure.
//
// The frame's flood (dgt.py:413-465) runs on a two-row strip: every live bin of row f-1 is a SOURCE in the heap from the
// start (key a_k = its magnitude, phase known), row f is unvisited (key b_k); a popped source (f-1, k) visits (f, k), a
// popped (f, k) visits (f, k+1) and -- unless that would be bin 0 (:453) -- (f, k-1); "visit" = take the phase from the
// popping entry, push, mark.  With DISTINCT keys the order of pops does not depend on the queue, and neither does the
// one thing the phases depend on: WHICH neighbour reaches a bin first.  An entry pops at the level
//     lev(e) = min(key(e), level at which e was pushed)        (the running minimum of the popped keys when e leaves)
// and entries leave in order of decreasing level, so bin k is visited at R(k) = max(a_k, lev(f, k-1), lev(f, k+1)) by
// whichever of the three attains the maximum, and lev(f, k) = min(b_k, R(k)).  On a path graph the closure is two
// directional scans of clamp functions x -> min(b_k, max(a_k, x)) (a composition of clamps is a clamp: a parallel prefix
// over the lanes), and the phases follow the parent pointers: chains along the row, each bin ONE float addition onto its
// parent's final phase -- the same additions as the heap flood, so the same bits.
//
// The unmarked seed (:427: the frame maximum is pushed first and NOT marked visited) is an extra entry S at bin kmax that
// pops at level b_kmax whatever happens to the bin itself, and hands its neighbours the phase the bin holds AT THAT TIME:
// the visited one if the bin's own source is larger than b_kmax, the initial one otherwise (the bin is then visited
// later, possibly by one of S's own children).
//
// Declined (returns false, nothing written; the caller runs the rank / heap flood): islands of several live bins that
// nothing reaches (the reference reseeds, :461-465 -- onsets in sparse spectra; a one-bin island just keeps its initial
// phase), two candidates for a bin's parent with EQUAL levels (tied magnitudes that actually compete: only the heap
// knows their order), the seed's bin visited at exactly the seed's level.  Ties that never meet are harmless.
//
// Lane l owns the CONTIGUOUS bins [l C, (l + 1) C), C = ceil(F / 64) <= CM (compile-time: every loop below is unrolled
// and predicated): the row is read from LDS once, the four scan walks, the parent choice and the rounds along the parent
// chains run on registers, chunk boundaries cross lanes by shuffles.  (A first version kept the arrivals and the chains
// in LDS: 15.6 us per frame against 10.5.)
template <int CM>
__device__ bool rt_scan_frame(const RtRows R, const int F, const int lane, const float abstol, const int kmax, float* scratch) {
  const float *srow = R.srow, *hrow = R.hrow, *ph0 = R.ph0, *tg0 = R.tg0, *tg1 = R.tg1, *fg1 = R.fg1;   // (tg0 is never null: LDS rows)
  float* ph1 = R.ph1;
  const float NEG = -__builtin_inff(), POS = __builtin_inff();
  int* par = reinterpret_cast<int*>(scratch);             // parent codes, for the island test across lane boundaries
  auto apply = [](float lo, float hi, float v) { return fminf(hi, fmaxf(lo, v)); };
  const int C = (F + 63) >> 6;
  const int k0 = lane * C < F ? lane * C : F;
  const int k1 = k0 + C < F ? k0 + C : F;
  const int nb = k1 - k0;                                // bins this lane owns (0 .. C)
  float b_[CM], c_[CM], lo_[CM], hi_[CM], fg_[CM];
#pragma unroll
  for (int i = 0; i < CM; ++i) {
    const bool in = i < nb;
    const int k = in ? k0 + i : 0;
    const float b = srow[k], a = hrow[k];
    fg_[i] = fg1[k];
    b_[i] = b;
    c_[i] = a > abstol ? a : NEG;
    if (!in) {                                           // identity: the chunk ends before CM bins
      lo_[i] = NEG;
      hi_[i] = POS;
      b_[i] = NEG;
    } else if (k == kmax) {
      lo_[i] = hi_[i] = b;
    } else if (!(b > abstol)) {
      lo_[i] = hi_[i] = NEG;
    } else {
      hi_[i] = b;
      lo_[i] = fminf(c_[i], b);
    }
  }
  float x_[CM], y_[CM];
  {
    float lo = NEG, hi = POS;
#pragma unroll
    for (int i = 0; i < CM; ++i) {
      lo = apply(lo_[i], hi_[i], lo);
      hi = apply(lo_[i], hi_[i], hi);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float plo = __shfl_up(lo, d, 64), phi = __shfl_up(hi, d, 64);
      if (lane >= d) {
        const float nlo = apply(lo, hi, plo), nhi = apply(lo, hi, phi);
        lo = nlo;
        hi = nhi;
      }
    }
    float arr = __shfl_up(lo, 1, 64);
    if (lane == 0) arr = NEG;
#pragma unroll
    for (int i = 0; i < CM; ++i) {
      x_[i] = arr;
      arr = apply(lo_[i], hi_[i], arr);
    }
  }
  {
    float lo = NEG, hi = POS;
#pragma unroll
    for (int i = CM - 1; i >= 0; --i) {
      lo = apply(lo_[i], hi_[i], lo);
      hi = apply(lo_[i], hi_[i], hi);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float plo = __shfl_down(lo, d, 64), phi = __shfl_down(hi, d, 64);
      if (lane + d < 64) {
        const float nlo = apply(lo, hi, plo), nhi = apply(lo, hi, phi);
        lo = nlo;
        hi = nhi;
      }
    }
    float arr = __shfl_down(lo, 1, 64);
    if (lane == 63) arr = NEG;
#pragma unroll
    for (int i = CM - 1; i >= 0; --i) {
      y_[i] = (k0 + i >= 1) ? arr : NEG;                 // bin 0 is never reached downward
      arr = apply(lo_[i], hi_[i], arr);
    }
  }
  // ---- parents
  const float bmax = srow[kmax];
  const float amax = hrow[kmax];
  const float cmax = amax > abstol ? amax : NEG;
  const float b_below = kmax - 1 >= 1 ? srow[kmax - 1] : 0.0f;          // the seed's neighbours, as S's children
  const float b_above = (kmax >= 1 && kmax + 1 < F) ? srow[kmax + 1] : 0.0f;
  bool bad = false, bad_reseed = false, seed_tie = false;
  int code_[CM];
#pragma unroll
  for (int i = 0; i < CM; ++i) {
    const int k = k0 + i;
    int code = 0;
    if (i < nb && b_[i] > abstol) {
      const float c = c_[i];
      float x = x_[i], y = y_[i];
      if (k == kmax) {
        if (b_below > abstol) x = b_below;
        if (b_above > abstol) y = b_above;
      }
      const float m = fmaxf(c, fmaxf(x, y));
      if ((int)(c == m) + (int)(x == m) + (int)(y == m) > 1 && m != NEG) bad = true;
      // the seed's bin visited at the very level S pops at (its source, or a neighbour, ties with the frame maximum):
      // which phase S hands on is the heap's to say -- and matters only if S has a child (below)
      if (k == kmax && m == bmax) seed_tie = true;
      code = m == NEG ? 4 : (c == m ? 1 : (x == m ? 2 : 3));
    }
    code_[i] = code;
    if (i < nb) par[k] = code;
  }
  lds_sync();
  // S's children: the bins next to the seed whose parent is the seed's side.  A held frame (row f equal to row f-1: a
  // stationary signal, hop-periodic tones) ties every source with its own bin -- harmless everywhere (a source only ever
  // visits its own bin) except at the seed, and there only if somebody takes S's phase.
  // ... and only if some source is LARGER than the frame maximum: S is pushed first (:427) and an entry only rises past an
  // equal key on a strict comparison (heapq.py:9-21), so with no larger source S is still the root when the flood starts and
  // is its very first pop -- it hands on the initial phase, whatever ties with it (a held frame: the row maxima are equal).
  if (__ballot(seed_tie) != 0 &&
      ((kmax + 1 < F && par[kmax + 1] == 2) || (kmax - 1 >= 1 && par[kmax - 1] == 3))) {
    float src_max = NEG;
#pragma unroll
    for (int i = 0; i < CM; ++i)
      if (i < nb) src_max = fmaxf(src_max, c_[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) src_max = fmaxf(src_max, __shfl_xor(src_max, o, 64));
    if (src_max > bmax) bad = true;
  }
#pragma unroll
  for (int i = 0; i < CM; ++i) {
    const int k = k0 + i;
    if (i < nb && code_[i] == 4 && ((k >= 1 && par[k - 1] == 4) || (k + 1 < F && par[k + 1] == 4))) bad = bad_reseed = true;
  }
  RT_STAT(0, 1);
  if (__ballot(bad) != 0) {
    RT_STAT(__ballot(bad_reseed) != 0 ? 3 : 4, 1);
    return false;
  }
  const float phi_s = cmax > bmax ? ph0[kmax] + 0.5f * (tg0[kmax] + tg1[kmax]) : ph1[kmax];
  // ---- phases: sources at once, then the chains; a bin adds its own step onto its parent's FINAL phase, nothing else
  float val_[CM];
  bool done_[CM];
#pragma unroll
  for (int i = 0; i < CM; ++i) {
    const int k = i < nb ? k0 + i : 0;
    done_[i] = false;
    val_[i] = 0.0f;
    if (code_[i] == 1) {
      val_[i] = ph0[k] + 0.5f * (tg0[k] + tg1[k]);
      done_[i] = true;
    }
  }
  const float fg_left = fg1[k0 >= 1 ? k0 - 1 : 0];       // the neighbours' frequency gradients across the chunk boundaries
  const float fg_right = fg1[k1 < F ? k1 : F - 1];
  for (int round = 0; round <= 64; ++round) {
    // what the lane to the left / right holds at the boundary: its last / first bin
    float last_val = 0.0f, first_val = val_[0];
    bool last_done = false, first_done = done_[0];
#pragma unroll
    for (int i = 0; i < CM; ++i)
      if (i == nb - 1) {
        last_val = val_[i];
        last_done = done_[i];
      }
    const float lv = __shfl_up(last_val, 1, 64), rv = __shfl_down(first_val, 1, 64);
    const bool ld = __shfl_up((int)last_done, 1, 64) != 0 && lane >= 1;
    const bool rd = __shfl_down((int)first_done, 1, 64) != 0 && lane < 63;
    bool pending = false;
#pragma unroll
    for (int i = 0; i < CM; ++i) {
      if (code_[i] == 2 && !done_[i]) {
        const int j = k0 + i - 1;
        const bool ready = j == kmax || (i == 0 ? ld : done_[i > 0 ? i - 1 : 0]);
        if (ready) {
          const float pp = j == kmax ? phi_s : (i == 0 ? lv : val_[i > 0 ? i - 1 : 0]);
          val_[i] = pp + 0.5f * ((i == 0 ? fg_left : fg_[i > 0 ? i - 1 : 0]) + fg_[i]);
          done_[i] = true;
        } else {
          pending = true;
        }
      }
    }
#pragma unroll
    for (int i = CM - 1; i >= 0; --i) {
      if (code_[i] == 3 && !done_[i]) {
        const int j = k0 + i + 1;
        const bool at_end = i == nb - 1;                 // the parent is the right-hand lane's first bin
        const bool ready = j == kmax || (at_end ? rd : done_[i + 1 < CM ? i + 1 : CM - 1]);
        if (ready) {
          const float pp = j == kmax ? phi_s : (at_end ? rv : val_[i + 1 < CM ? i + 1 : CM - 1]);
          val_[i] = pp - 0.5f * ((at_end ? fg_right : fg_[i + 1 < CM ? i + 1 : CM - 1]) + fg_[i]);
          done_[i] = true;
        } else {
          pending = true;
        }
      }
    }
    RT_STAT(2, 1);
    if (__ballot(pending) == 0) break;
  }
#pragma unroll
  for (int i = 0; i < CM; ++i)
    if (i < nb && code_[i] >= 1 && code_[i] <= 3) ph1[k0 + i] = val_[i];
  lds_sync();
  RT_STAT(1, 1);
  return true;
}

// Rank pre-pass of the realtime flood.  A frame's flood (dgt.py:413-465) pops, in descending magnitude, entries that are
// known before it starts: the bins of row f-1 (pushed up front) and the bins of row f (pushed as the flood reaches
// them).  When no two of those magnitudes are equal, WHICH priority queue hands them out is immaterial -- the pop order
// is the strict order of the keys -- and a bitmap over the ranks replaces the heap: pop = find-first-set, push = set a
// bit.  Ranks are a sort, and a sort is parallel: one workgroup per (stream, frame) on the chip the one-wave-per-stream
// flood leaves idle.  Equal magnitudes are marked per rank (`same_as_previous`); what the flood does about them is in
// pghi_hgi_rt_coop_kernel.
__global__ __launch_bounds__(256) void pghi_rt_rank_kernel(RtParams p, int n2) {
  extern __shared__ __attribute__((aligned(16))) u64 rk_items[];
  const int F = p.F, R = p.n + 2, E = 2 * F;
  const int s = blockIdx.x / p.n, fr = blockIdx.x - s * p.n;          // new frame fr: rows fr + 1 (f - 1) and fr + 2 (f)
  const float* rows = p.spec + ((long long)s * R + fr + 1) * F;       // 2F consecutive floats: row f-1, then row f
  for (int i = threadIdx.x; i < n2; i += blockDim.x)
    rk_items[i] = i < E ? (((u64)(~__float_as_uint(rows[i]))) << 32) | (unsigned)i : ~0ull;   // ascending = descending magnitude
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        const int x = i ^ j;
        if (x > i) {
          const u64 a = rk_items[i], b = rk_items[x];
          if ((a > b) == ((i & k) == 0)) {
            rk_items[i] = b;
            rk_items[x] = a;
          }
        }
      }
      __syncthreads();
    }
  unsigned short* rec = p.ranks + ((long long)s * p.n + fr) * p.rank_stride;
  unsigned* sp = reinterpret_cast<unsigned*>(rec + 2 * E);
  for (int r = threadIdx.x; r < E; r += blockDim.x) {
    const u64 it = rk_items[r];
    const unsigned e = (unsigned)it & 0xffffu;
    rec[r] = (unsigned short)e;
    rec[E + e] = (unsigned short)r;
  }
  // same-as-previous bits, one thread per word (magnitudes are compared as the bit patterns they were sorted by)
  for (int w = threadIdx.x; w < (E + 31) / 32; w += blockDim.x) {
    unsigned bits = 0u;
    for (int b = 0; b < 32; ++b) {
      const int r = 32 * w + b;
      if (r >= 1 && r < E && (unsigned)(rk_items[r] >> 32) == (unsigned)(rk_items[r - 1] >> 32)) bits |= 1u << b;
    }
    sp[w] = bits;
  }
}

// Rank fast path (see pghi_rt_rank_kernel): the frontier is a bitmap over the ranks of the frame's 2F candidates.
//
// Ties.  Among 1026 float32 magnitudes SOME two are equal in ~2 % of all frames -- with 256 streams in nearly every
// step -- so a tie cannot simply send the frame to the heap.  Tied entries leave the queue back to back in an order
// only the heap knows (its sift rules, utils/heapq.py:9-59).  Call a tied entry's pop together with everything that
// pops because of it before the next tied entry gets its turn (entries it pushes whose keys are larger) its BLOCK.
// A block's effect depends on the state only through the bins it looks at (its own phase, the availability of its
// targets): T; it changes the state only by visiting bins: V (subset of T).  If for every two blocks of a tie group
// V of one misses T of the other, every block does the same whatever order the group is taken in, and the result
// is the heap's.  That is checked as the group runs (in rank order); a collision abandons the fast path and the
// frame is redone on the heap.  (tools/fuzz_rt_ties.py: injected ties, bit for bit against the heap kernel.)
//
// LDS: per-rank records where the heap would be (ONE ds_read_b128 per pop), the rank tables and two bitmaps behind
// them (the launcher sized the allocation for that).  A record is {phase, targets, step up, step down}:
//   row f-1, bin k:  {ph0[k],            rank of (f, k)   | 0xffff << 16,        0.5 (tg0[k] + tg1[k]),  0}
//   row f,   bin k:  {ph1[k] (written    rank of (f, k+1) | rank of (f, k-1) << 16, 0.5 (fg[k] + fg[k+1]), 0.5 (fg[k] + fg[k-1])}
//                     when reached),
// so that one pop is: target `up` gets phase + step up, target `down` gets phase - step down, whatever the row
// (dgt.py:438-440, 447-449, 455-457); 0xffff: no such target (k + 1 = F; k - 1 <= 0: bin 0 is never reached
// downward, :453).
// (an offset in floats, not a rounded address: a pointer that has been through uintptr_t is a generic pointer and
//  every access through it a flat_load / flat_store)
//
// One frame on the rank bitmap.  Like rt_scan_frame it returns false when it declines (pervasive or colliding ties: the
// caller runs the heap flood; R.ph1 and R.srow are untouched), true when row f of the phase is final in R.ph1.
// (The table setup stays in this body: as a helper of its own it cost the rank and heap floods 2.3 % and 1.1 % -- the
// kernel spills scalar registers, and their allocation is that sensitive.)
__device__ __forceinline__ bool rt_rank_flood(const RtRows& R, float* rt_smem, const unsigned short* grec, int F, int lane,
                                              float abstol) {
  // Pervasive ties: a held frame, a hop-periodic tone or a test signal makes row f equal row f-1, every
  // pop then lands in a tie group whose block visits its tied partner and the frame is redone on the heap anyway --
  // after paying for the tables, the records and the aborted flood.  The pre-pass has already marked the tied ranks:
  // when more than a quarter of the 2F candidates are tied the attempt is skipped.
  int nt = (lane < (2 * F + 31) / 32) ? __popc(reinterpret_cast<const unsigned*>(grec + 4 * F)[lane]) : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nt += __shfl_xor(nt, o, 64);
  if (2 * nt > F) return false;
  int4* recs = reinterpret_cast<int4*>(rt_smem + ((7 * F + 3) & ~3));         // [2F], 16-byte aligned (the wave's LDS is)
  unsigned short* eor = reinterpret_cast<unsigned short*>(recs + 2 * F);     // entry at rank r (e < F: row f-1, bin e; else row f, bin e - F)
  unsigned short* roe = eor + 2 * F;                                          // rank of entry e
  unsigned* bm = reinterpret_cast<unsigned*>(roe + 2 * F);                    // [0,64): row f-1 live, [64,128): row f live, by rank
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(grec);
    unsigned* dst = reinterpret_cast<unsigned*>(eor);
    for (int i = lane; i < 2 * F; i += 64) dst[i] = src[i];              // 4F u16 = 2F words
    bm[lane] = 0u;
    bm[64 + lane] = 0u;
  }
  const unsigned sp = (lane < (2 * F + 31) / 32) ? reinterpret_cast<const unsigned*>(grec + 4 * F)[lane] : 0u;   // same-as-previous, by rank
  // rank r is part of a tie: same as its predecessor or as its successor (whose bit may sit in the next lane's word)
  const unsigned tied_bits = sp | (sp >> 1) | ((unsigned)__shfl_down((int)sp, 1, 64) << 31);
  lds_sync();
  for (int k = lane; k < F; k += 64) {
    const unsigned ra = roe[k], rb = roe[F + k];
    if (R.hrow[k] > abstol) atomicOr(&bm[ra >> 5], 1u << (ra & 31));
    if (R.srow[k] > abstol) atomicOr(&bm[64 + (rb >> 5)], 1u << (rb & 31));
    recs[ra] = make_int4(__float_as_int(R.ph0[k]), (int)(rb | 0xffff0000u), __float_as_int(0.5f * (R.tg0[k] + R.tg1[k])), 0);
    const unsigned ru = (k + 1 < F) ? (unsigned)roe[F + k + 1] : 0xffffu;
    const unsigned rd = (k - 1 > 0) ? (unsigned)roe[F + k - 1] : 0xffffu;
    const float gk = R.fg1[k];
    recs[rb] = make_int4(__float_as_int(R.ph1[k]), (int)(ru | (rd << 16)), __float_as_int(0.5f * (gk + R.fg1[k + 1 < F ? k + 1 : k])),
                         __float_as_int(0.5f * (gk + R.fg1[k >= 1 ? k - 1 : 0])));
  }
  lds_sync();
  unsigned qbits = bm[lane];          // the frontier, by rank: lane i holds ranks 32 i .. 32 i + 31
  unsigned bav = bm[64 + lane];       // row-f entries that are live and not yet visited, by rank
  // rec_word[4 r] = phase of rank r as its bit pattern: written through the SAME type the records are read with (int4
  // words), so the compiler may not reorder the lane-0 store against the next pop's 16-byte load (a float*
  // alias of the int4 records relied on in-order DS issue only)
  int* rec_word = reinterpret_cast<int*>(recs);
  auto bit_of = [&](unsigned bits, int i) -> bool {
    return (((unsigned)__builtin_amdgcn_readlane((int)bits, i >> 5)) >> (i & 31)) & 1u;
  };
  auto first_of = [&](unsigned bits, int& r) -> bool {       // lowest set rank of a lane-distributed bitmap
    const u64 nz = __ballot(bits != 0u);
    if (nz == 0) return false;
    const int L = __builtin_ctzll(nz);
    const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)bits, L);
    r = 32 * L + __builtin_ctz(w);
    return true;
  };
  // tie-group state: cur_* = the running block, acc_* = the group's earlier blocks; T / V are sets of entries by rank
  unsigned cur_v = 0u, cur_t = 0u, acc_v = 0u, acc_t = 0u;
  // one pop of rank r (already off the frontier), its record in hand.  TRACK: inside a tie group, with the block
  // bookkeeping.  Returns, for the caller's prefetch, whether rank `watch` had its phase written.
  auto process = [&](int r, const int4 rec, int watch, auto track) -> bool {
    constexpr bool TRACK = decltype(track)::value;
    const unsigned w1 = (unsigned)uni(rec.y);
    const int ru = (int)(w1 & 0xffffu), rd = (int)(w1 >> 16);
    const float pk = __int_as_float(rec.x);
    // availability of the two targets, without branching on "is there one": the lane index is masked, the verdict is not
    const unsigned wu = (unsigned)__builtin_amdgcn_readlane((int)bav, (ru >> 5) & 63);
    const unsigned wd = (unsigned)__builtin_amdgcn_readlane((int)bav, (rd >> 5) & 63);
    const bool up = ru != 0xffff && ((wu >> (ru & 31)) & 1u);
    const bool dn = rd != 0xffff && ((wd >> (rd & 31)) & 1u);
    if (up && lane == 0) rec_word[4 * ru] = __float_as_int(pk + __int_as_float(rec.z));
    if (dn && lane == 0) rec_word[4 * rd] = __float_as_int(pk - __int_as_float(rec.w));
    const unsigned mu = up ? (1u << (ru & 31)) : 0u, md = dn ? (1u << (rd & 31)) : 0u;
    const unsigned add = ((lane == (ru >> 5)) ? mu : 0u) | ((lane == (rd >> 5)) ? md : 0u);
    qbits |= add;                       // the reached entries join the frontier ...
    bav &= ~add;                        // ... and are no longer unvisited
    if (TRACK) {
      cur_v |= add;
      cur_t |= add | ((lane == (r >> 5)) ? (1u << (r & 31)) : 0u) |
               ((ru != 0xffff && lane == (ru >> 5)) ? (1u << (ru & 31)) : 0u) |
               ((rd != 0xffff && lane == (rd >> 5)) ? (1u << (rd & 31)) : 0u);
    }
    return (up && ru == watch) || (dn && rd == watch);
  };
  auto close_block = [&]() -> bool {    // the running block against the group's earlier ones; then it joins them
    const bool clash = __ballot(((cur_v & acc_t) | (cur_t & acc_v)) != 0u) != 0;
    acc_v |= cur_v;
    acc_t |= cur_t;
    cur_v = 0u;
    cur_t = 0u;
    return !clash;
  };
  bool ok = true;
  int r = 0;
  if (first_of(bav, r)) {               // :427 the frame maximum seeds the frontier and is NOT marked visited
    if (lane == (r >> 5)) qbits |= 1u << (r & 31);
  }
  while (true) {
    // ---- the common case: pops whose magnitude is nobody else's
    // (Requesting the next pop's record ahead -- the frontier's next rank as it stands, read again when this pop reaches
    //  something larger -- was built and measured: 0.26 -> 0.39 ms per frame; the select between the two records and
    //  the extra find-first cost more than the round trip they hide.)
    bool tied = false;
    while (first_of(qbits, r)) {
      if (bit_of(tied_bits, r)) {
        tied = true;
        break;
      }
      if (lane == (r >> 5)) qbits &= ~(1u << (r & 31));
      process(r, recs[r], -1, std::integral_constant<bool, false>());
    }
    if (!tied) {                        // :461-465 the frontier ran dry: the largest unvisited bin of the row, marked
      if (!first_of(bav, r)) break;     // (the reference pushes one last entry at or below abstol and leaves: no effect)
      if (lane == (r >> 5)) {
        bav &= ~(1u << (r & 31));
        qbits |= 1u << (r & 31);        // popped at once by the next trip
      }
      continue;
    }
    // ---- a tie group: ranks [g_lo, g_hi] share one magnitude; rank r, still on the frontier, is its first member out
    int g_lo = r, g_hi = r;
    while (bit_of(sp, g_lo)) --g_lo;                                  // (bit 0 is never set)
    while (g_hi + 1 < 2 * F && bit_of(sp, g_hi + 1)) ++g_hi;
    cur_v = cur_t = acc_v = acc_t = 0u;
    bool finished = false;
    while (true) {
      if (!first_of(qbits, r)) {        // reseed inside the group's span: part of the running block
        if (!first_of(bav, r)) {
          finished = true;
          break;
        }
        if (lane == (r >> 5)) {
          bav &= ~(1u << (r & 31));
          qbits |= 1u << (r & 31);
          cur_v |= 1u << (r & 31);
          cur_t |= 1u << (r & 31);
        }
        continue;
      }
      if (r > g_hi) break;              // the group is over; rank r stays on the frontier for the common loop
      if (lane == (r >> 5)) qbits &= ~(1u << (r & 31));
      if (r >= g_lo && !close_block()) {       // the next tied entry: the running block is complete
        ok = false;
        break;
      }
      process(r, recs[r], -1, std::integral_constant<bool, true>());
    }
    if (ok && !close_block()) ok = false;
    if (!ok || finished) break;
  }
  lds_sync();
  if (ok) {                             // back to bin order
    for (int k = lane; k < F; k += 64) R.ph1[k] = __int_as_float(rec_word[4 * roe[F + k]]);
    lds_sync();
  }
  return ok;
}

// One frame on the wave-cooperative heap (pghi_heap.h), the whole heap in LDS: what the scan and rank paths fall back to.
// `max_val` at bin `max_k` is the maximum of row f (uniform).
__device__ __forceinline__ void rt_heap_flood(const RtRows& R, const HeapT<false>& H, int F, int lane, float abstol, u64 anc_mask,
                                              float max_val, int max_k) {
  int hn = 1;
  if (lane == 0) H.store(0, pack_item(-max_val, F + (int)max_k));   // :427 the seed is NOT marked visited
  lds_sync();
  auto push = [&](float key, int idx) {     // heappush (heapq.py:45-48)
    coop_siftdown(H, hn, pack_item(key, idx), lane);
    ++hn;
    lds_sync();
  };
  // :428-430 every live bin of row f-1, in bin order.  64 bins per LDS read, then a scalar walk over the live
  // ones (one LDS round trip per bin costs as much as a fifth of the push it decides about)
  for (int k0 = 0; k0 < F; k0 += 64) {
    const float mine = (k0 + lane < F) ? R.hrow[k0 + lane] : 0.0f;
    u64 live_bins = __ballot(mine > abstol);
    while (live_bins) {
      const int j = __builtin_ctzll(live_bins);
      live_bins &= live_bins - 1;
      const float hv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), j));
      push(-hv, k0 + j);
    }
  }
  while (max_val > abstol) {  // :433
    while (hn > 0) {
      // heappop (heapq.py:51-59)
      const u64 top63 = H.top[(lane >= 1 && lane - 1 < 4 * F + 8) ? lane - 1 : 0];   // the heap holds 4F + 8 entries
      const u64 last = H.load(hn - 1);
      hn -= 1;
      const int idx = uni(item_idx(hn == 0 ? last : readlane64(top63, 1)));
      const bool cur_row = idx >= F;
      const int k = cur_row ? idx - F : idx;
      // the magnitudes this pop may propagate to, requested before the heap repair (they come back first:
      // LDS returns in order) instead of one round trip each afterwards
      const float s_here = R.srow[k];
      const float s_up = R.srow[k + 1 < F ? k + 1 : k];
      const float s_dn = R.srow[k >= 1 ? k - 1 : 0];
      if (hn > 0) {
        coop_pop_repair(H, hn, last, top63, lane, anc_mask);
        lds_sync();
      }
      if (!cur_row) {  // :436-443 propagate in time
        const float sv = ufloat(s_here);
        if (sv > abstol) {
          if (lane == 0) {
            R.ph1[k] = R.ph0[k] + 0.5f * (R.tg0[k] + R.tg1[k]);
            R.srow[k] = abstol;
          }
          push(-sv, F + k);
        }
      } else {  // :444-460 propagate in frequency
        if (k + 1 < F) {
          const float sv = ufloat(s_up);
          if (sv > abstol) {
            if (lane == 0) {
              R.ph1[k + 1] = R.ph1[k] + 0.5f * (R.fg1[k] + R.fg1[k + 1]);
              R.srow[k + 1] = abstol;
            }
            push(-sv, F + k + 1);
          }
        }
        if (k - 1 > 0) {  // bin 0 is never reached downward (:453)
          const float sv = ufloat(s_dn);
          if (sv > abstol) {
            if (lane == 0) {
              R.ph1[k - 1] = R.ph1[k] - 0.5f * (R.fg1[k] + R.fg1[k - 1]);
              R.srow[k - 1] = abstol;
            }
            push(-sv, F + k - 1);
          }
        }
      }
    }
    // :461-465 reseed inside the frame: first index of the row maximum, lane-parallel
    float mv = -3.402823466e+38f;
    long long mk = F;
    for (int k = lane; k < F; k += 64) {
      const float v = R.srow[k];
      if (v > mv) {
        mv = v;
        mk = k;
      }
    }
    wave_argmax(mv, mk);
    max_val = ufloat(mv);
    const int mki = uni((int)mk);
    push(-max_val, F + mki);
    if (lane == 0) R.srow[mki] = abstol;
    lds_sync();
  }
}

// The same frame step as the single-lane kernels with the rows in LDS and three floods to choose from, in this order: the
// queue-free scan path (rt_scan_frame), the rank bitmap (rt_rank_flood, where the pre-pass ran) and the wave-cooperative
// heap of the offline kernel, the whole heap in LDS (rt_heap_flood).  A frame pops up to 2F entries from a heap of ~1000:
// done by one lane that is ~10 dependent LDS round trips down and a few up per pop (~3600 cycles); the cooperative pop
// resolves five levels per round with one wide LDS gather.  Same binary heap, same sift rules, same pop order.
__global__ __launch_bounds__(256) void pghi_hgi_rt_coop_kernel(RtParams p) {
  rt_bump_step(p);
  extern __shared__ __attribute__((aligned(16))) float rt_smem_all[];
  // one wave per stream, 1 to 4 independent waves per workgroup (see pghi_hgi_offline_coop_kernel)
  const int wave = threadIdx.x >> 6;
  const int s = blockIdx.x * (blockDim.x >> 6) + wave;
  if (s >= p.S) return;
  const int lane = threadIdx.x & 63;
  const int F = p.F, R = p.n + 2;
  float* rt_smem = rt_smem_all + (size_t)wave * p.lds_floats_per_wave;
  const long long n = (long long)R * F;
  const float* spec = p.spec + (long long)s * n;
  const float* tgw = p.tgradw + (long long)s * n;
  const float* fgw = p.fgradw + (long long)s * n;
  float* srow = rt_smem;       // the seven rows of RtRows, in its order
  float* hrow = srow + F;
  float* ph0 = hrow + F;
  float* ph1 = ph0 + F;
  float* tg0 = ph1 + F;
  float* tg1 = tg0 + F;
  float* fg1 = tg1 + F;
  const RtRows rows = {srow, hrow, ph0, ph1, tg0, tg1, fg1};
  const HeapT<false> H = {reinterpret_cast<u64*>(fg1 + F + (F & 1)), nullptr, 0x7fffffff};
  const u64 anc_mask = chain_mask(lane);
  const float abstol = rt_abstol(spec, n, lane, p.tol, p.eps);

  // :402-403 row 1 of the phase array is the previous call's last row.  The phase row of the frame before and its time
  // gradient stay in LDS from frame to frame (round 5): the work array in global memory was written, fenced at agent
  // scope and read back by the same wave every frame -- a third of the scan path's time per frame.
  for (int k = lane; k < F; k += 64) {
    ph1[k] = p.prev_phase[(long long)s * F + k];
    tg1[k] = 0.0f;                       // :408-410 two-row front padding: the gradient row "before" frame 2
  }
  lds_sync();

  for (int f = 2; f < R; ++f) {  // :413
#ifdef AT_DEV_SWITCHES
    const unsigned long long tickf0 = wall_clock64();
#endif
    // ---- load the rows; the frame maximum
    float max_val = -1.0f;
    long long max_k = F;
    for (int k = lane; k < F; k += 64) {   // rows f-1 of the phase and of tgradw: last frame's ph1 / tg1
      ph0[k] = ph1[k];
      tg0[k] = tg1[k];
    }
    lds_sync();
    // four strides of 64 bins per trip, all 28 loads requested before the first is used: one wave per SIMD hides nothing,
    // and a trip per 64 bins was nine dependent round trips to global memory per frame (11 us of the scan path's 27)
    for (int kb = lane; kb < F; kb += 256) {
      float v_[4], h_[4], nz_[4], t1_[4], g1_[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = kb + 64 * u;
        const bool in = k < F;
        const long long kk = in ? k : 0;
        v_[u] = spec[(long long)f * F + kk];
        h_[u] = spec[(long long)(f - 1) * F + kk];
        nz_[u] = p.noise[(long long)s * p.n * F + (long long)(f - 2) * F + kk];
        t1_[u] = tgw[(long long)(f - 2) * F + kk];
        g1_[u] = fgw[(long long)(f - 2) * F + kk];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = kb + 64 * u;
        if (k < F) {
          const float v = v_[u];
          srow[k] = v;
          hrow[k] = h_[u];
          ph1[k] = (v > abstol) ? 0.0f : nz_[u];  // :404-405
          tg1[k] = t1_[u];
          fg1[k] = g1_[u];
          if (v > max_val) {
            max_val = v;
            max_k = k;
          }
        }
      }
    }
    wave_argmax(max_val, max_k);
    max_val = ufloat(max_val);
    lds_sync();
    // ---- scan path
    bool fast_done = false;
    if (p.scan_path && max_val > abstol) {
#ifdef AT_DEV_SWITCHES
      const unsigned long long tick0 = wall_clock64();
#endif
      float* scan_scratch = fg1 + F + (F & 1);            // where the heap would be
      const int kmx = uni((int)max_k);
      if (F <= 64 * 9) fast_done = rt_scan_frame<9>(rows, F, lane, abstol, kmx, scan_scratch);
      else if (F <= 64 * 17) fast_done = rt_scan_frame<17>(rows, F, lane, abstol, kmx, scan_scratch);
      // (rows of more than 1088 bins do not fit this kernel's LDS budget anyway: n_fft 4096 runs on the global-memory kernels)
      lds_sync();
#ifdef AT_DEV_SWITCHES
      RT_STAT(5, wall_clock64() - tick0);      // 100 MHz ticks inside the scan path
#endif
    }
    // ---- rank path
    if (!fast_done && p.ranks != nullptr && max_val > abstol)
      fast_done = rt_rank_flood(rows, rt_smem, p.ranks + ((long long)s * p.n + (f - 2)) * p.rank_stride, F, lane, abstol);
    // ---- heap path
    if (!fast_done && max_val > abstol) rt_heap_flood(rows, H, F, lane, abstol, anc_mask, max_val, (int)max_k);  // :416-417
    // ---- store
    lds_sync();
    for (int k = lane; k < F; k += 64) p.phase_out[(long long)s * p.n * F + (long long)(f - 2) * F + k] = ph1[k];
    lds_sync();
#ifdef AT_DEV_SWITCHES
    RT_STAT(6, wall_clock64() - tickf0);     // 100 MHz ticks per frame, everything included
#endif
  }
}

// x = mag * exp(i phase): refresh the PGHI history (|x[-2:]|, angle(x[-1]))   dgt.py:325-336
struct RtUpdParams {
  const float* mag;       // (S, n, F)
  const float* phase;     // (S, n, F)
  const float* hist_in;   // (S, 2, F)
  float* hist_out;        // (S, 2, F)
  float* phase_out;       // (S, F)
  int S, n, F;
};

__global__ __launch_bounds__(256) void rt_update_kernel(RtUpdParams p) {
  const long long total = (long long)p.S * p.F;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int s = (int)(i / p.F), k = (int)(i - (long long)s * p.F);
    const long long last = ((long long)s * p.n + (p.n - 1)) * p.F + k;
    float sn, cs;
    sincosf(p.phase[last], &sn, &cs);
    const float re = p.mag[last] * cs, im = p.mag[last] * sn;
    float prev;
    if (p.n > 1) {
      const long long l2 = last - p.F;
      float s2, c2;
      sincosf(p.phase[l2], &s2, &c2);
      prev = hypotf(p.mag[l2] * c2, p.mag[l2] * s2);
    } else {
      prev = p.hist_in[((long long)s * 2 + 1) * p.F + k];
    }
    p.hist_out[((long long)s * 2) * p.F + k] = prev;
    p.hist_out[((long long)s * 2 + 1) * p.F + k] = hypotf(re, im);
    p.phase_out[i] = fast_atan2f(im, re);
  }
}

// the workspace: spec | hist | tgradw | fgradw | phase (n + 2 rows each) | device-drawn noise (n rows) | 16-byte-aligned heap
// (4F + 8 entries per stream) | 16-byte-aligned rank records (rt_rank_stride_u16 per stream and new frame)
struct RtWorkspace {
  float *spec, *hist, *tgradw, *fgradw, *phase, *noise;
  HeapItem* heap;
  unsigned short* ranks;
};
static RtWorkspace carve_rt(void* workspace, int S, int n, int F) {
  const size_t arr = (size_t)S * (size_t)(n + 2) * (size_t)F;
  float* f = (float*)workspace;
  RtWorkspace w = {f, f + arr, f + 2 * arr, f + 3 * arr, f + 4 * arr, f + 5 * arr, nullptr, nullptr};
  w.heap = (HeapItem*)(((uintptr_t)(f + 6 * arr) + 15) & ~(uintptr_t)15);
  w.ranks = (unsigned short*)(((uintptr_t)(w.heap + (size_t)S * (4 * (size_t)F + 8)) + 15) & ~(uintptr_t)15);
  return w;
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

size_t at_pghi_rt_workspace_bytes(int S, int n, int F) {
  const size_t per = (size_t)(n + 2) * (size_t)F;
  // spec, hist, tgradw, fgradw, phase (n + 2 rows each) + device-drawn noise (n rows) + heap + the rank records
  return (size_t)S * (6 * per * sizeof(float) + (4 * (size_t)F + 8) * sizeof(HeapItem) +
                      (size_t)n * (size_t)at_hip::rt_rank_stride_u16(F) * 2) + 512;
}

static int pghi_realtime_impl(const float* mag_hist, const float* mag, const float* prev_phase, const float* noise,
                              unsigned* rng_state, int S, int n, int F, float gamma, int n_fft, int hop, float tol, float eps,
                              float* phase, float* tgradw_or_null, float* fgradw_or_null, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (S < 0 || n <= 0 || F <= 0 || n_fft <= 0 || hop <= 0) return AT_EINVAL;
  if (S == 0) return AT_OK;
  if (!mag_hist || !mag || !prev_phase || !phase) return AT_EINVAL;
  if ((noise == nullptr) == (rng_state == nullptr)) return AT_EINVAL;     // exactly one source of draws
  if (!workspace || workspace_bytes < at_pghi_rt_workspace_bytes(S, n, F)) return AT_EWORKSPACE;
  const RtWorkspace w = carve_rt(workspace, S, n, F);
  RtParams p;
  p.mag_hist = mag_hist; p.mag = mag; p.prev_phase = prev_phase; p.phase_out = phase;
  p.noise_gen = noise ? nullptr : w.noise;
  p.noise = noise ? noise : p.noise_gen;
  p.rng_state = rng_state;
  p.spec = w.spec; p.hist = w.hist;
  p.tgradw = tgradw_or_null ? tgradw_or_null : w.tgradw;
  p.fgradw = fgradw_or_null ? fgradw_or_null : w.fgradw;
  p.phase = w.phase;
  p.heap = w.heap;
  p.S = S; p.n = n; p.F = F; p.n_fft = n_fft; p.hop = hop; p.gamma = gamma; p.tol = tol; p.eps = eps;
  p.lds_floats_per_wave = 0;
  p.ranks = nullptr;
  p.rank_stride = rt_rank_stride_u16(F);
  p.scan_path = 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pghi_grad_rt_kernel, dim3(grid1d((long long)S * (n + 2) * F)), dim3(256), 0, s, p);
  const size_t lds = sizeof(float) * (7 * (size_t)F + 1) + sizeof(HeapItem) * (4 * (size_t)F + 8);
  // at_set_variant(AT_VARIANT_PGHI_KERNEL, 2) selects the single-lane kernels (debugging aid; identical results), 3 the
  // cooperative heap kernel without the rank fast path
  const int pghi_kernel = variant(kVarPghiKernel);
  const bool serial_rt = pghi_kernel == 2;
  p.scan_path = pghi_kernel == 0;            // 4: the rank fast path without the scan path in front of it
  // the fast path keeps 2F 16-byte records where the heap would be and 8F + 512 bytes of tables behind them
  const size_t lds_fast = sizeof(float) * (7 * (size_t)F + 4) + 16 * (2 * (size_t)F) + 8 * (size_t)F + 512 + 16;
  // Default (variant 0): the scan path resolves a frame without a queue and declines only competing ties and islands of
  // several unreached bins (dense noise: none in 8e4 frames; sparse frames that decline are cheap on the heap), so the
  // rank pre-pass -- 84 us per call at 256 streams x 4 frames, more than the scan path's whole flood -- is not run:
  // scan -> heap.  Variant 4 keeps round 4's chain rank bitmap -> heap (and its tests), variant 3 the heap alone.
  bool rank_path = false;
  if (pghi_kernel == 4 && lds_fast <= 64 * 1024 && 2 * F <= 2048 && F >= 8 && (long long)S * n < (1LL << 31)) {
    rank_path = true;
    // rank pre-pass: one workgroup per (stream, new frame) sorts the frame's 2F candidates
    p.ranks = w.ranks;
    int n2 = 2;
    while (n2 < 2 * F) n2 <<= 1;
    hipLaunchKernelGGL(pghi_rt_rank_kernel, dim3((unsigned)((long long)S * n)), dim3(256), (size_t)n2 * sizeof(u64), s, p, n2);
  }
  if (lds <= 64 * 1024 && !serial_rt) {
    const size_t per_wave = ((rank_path ? (lds_fast > lds ? lds_fast : lds) : lds) + 15) & ~(size_t)15;
    p.lds_floats_per_wave = (int)(per_wave / sizeof(float));
    // up to one stream per CU spreads best (256 streams: 3.5 ms alone on their CUs, 3.7 ms packed four to a CU);
    // from four per CU on, a workgroup of four loads the CU's SIMDs evenly (1024 streams: 4.15 -> 3.88 ms)
    return launch_waves(pghi_hgi_rt_coop_kernel, S, S >= 4 * 256 ? 4 : 1, per_wave, 1024, s, p);
  }
  if (lds <= 64 * 1024)
    hipLaunchKernelGGL(pghi_hgi_rt_lds_kernel, dim3((unsigned)S), dim3(64), lds, s, p);
  else
    hipLaunchKernelGGL(pghi_hgi_rt_kernel, dim3((unsigned)S), dim3(64), 0, s, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_pghi_realtime(const float* mag_hist, const float* mag, const float* prev_phase, const float* noise, int S, int n,
                     int F, float gamma, int n_fft, int hop, float tol, float eps, float* phase, float* tgradw_or_null,
                     float* fgradw_or_null, void* workspace, size_t workspace_bytes, void* stream) {
  if (!noise) return AT_EINVAL;
  return pghi_realtime_impl(mag_hist, mag, prev_phase, noise, nullptr, S, n, F, gamma, n_fft, hop, tol, eps, phase,
                            tgradw_or_null, fgradw_or_null, workspace, workspace_bytes, stream);
}

int at_pghi_realtime_seeded(const float* mag_hist, const float* mag, const float* prev_phase, uint32_t* rng_state, int S, int n,
                            int F, float gamma, int n_fft, int hop, float tol, float eps, float* phase, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!rng_state) return AT_EINVAL;
  return pghi_realtime_impl(mag_hist, mag, prev_phase, nullptr, rng_state, S, n, F, gamma, n_fft, hop, tol, eps, phase, nullptr,
                            nullptr, workspace, workspace_bytes, stream);
}

int at_rt_update_buffers(const float* mag, const float* phase, int S, int n, int F, const float* hist_in,
                         float* hist_out, float* phase_out, void* stream) {
  if (S < 0 || n <= 0 || F <= 0) return AT_EINVAL;
  if (S == 0) return AT_OK;
  if (!mag || !phase || !hist_in || !hist_out || !phase_out) return AT_EINVAL;
  RtUpdParams p = {mag, phase, hist_in, hist_out, phase_out, S, n, F};
  hipLaunchKernelGGL(rt_update_kernel, dim3(grid1d((long long)S * F)), dim3(256), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

#ifdef AT_DEV_SWITCHES
extern "C" int at_dev_rt_stats(unsigned* out8, int reset) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(at_hip::g_rt_stats), 8 * sizeof(unsigned)) != hipSuccess) return -5;
  if (reset) {
    unsigned z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(at_hip::g_rt_stats), z, sizeof(z)) != hipSuccess) return -5;
  }
  return 0;
}
#endif

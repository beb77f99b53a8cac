// fft_convolve.hip -- the frequency-domain half of a uniformly partitioned overlap-save convolution: a complex FIR along
// the FRAME axis of a spectrum, one filter per bin, and its correlation (the filter's gradient).
//
// With block B, n_fft N = 2 B, F = B + 1 bins, frames X[t] = rfft(x[tB - B, tB + B)) and partitions H[p] = rfft(h[pB, pB + B)
// followed by B zeros), the last B samples of irfft(Y[t]), Y[t] = sum_p H[p] X[t - p], are block t of the full convolution.
// The transforms on both sides are the library's (at_stft_forward with center = 0, at_irfft_frames_streams and the two
// adjoints); this file holds
//
//   at_spectral_fir        Y[r][t][f]  = sum_{p < P} Hc[p][f] X[r][s][f],   s = t - p (causal) or t + p (anticausal), terms with
//                                        s outside [0, T) skipped, Hc = H or conj(H): the forward is (causal, H), the
//                                        signal's backward (anticausal, conj H)
//   at_spectral_fir_corr   gH[rh][p][f] = sum_r sum_{t >= p} conj(X[r][t - p][f]) gY[r][t][f]
//   at_spectral_fir_stream the causal forward over one chunk of a stream, the P - 1 frames before it read from a ring of
//                          spectra that the same launch then updates in place (below)
//
// spectral_fir.  A lane owns ONE bin and kFirTile consecutive output frames in registers, so a wavefront reads and writes
// 64 consecutive bins (512 bytes) of a frame.  The kFirTile frames of X that the tile needs at partition p are the ones it
// needed at p - 1 moved by one frame: the window stays in registers (its slots rotate with p, the p loop is unrolled by the
// tile so that every slot index is a constant) and costs ONE new load of X per p, next to one load of H[p][f].  A work
// item is (row, frame tile, chunk of 256 bins) on one 64-bit index; workgroups past kFirMaxGrid walk the items in turn.
// A tile writes kFirTile whole rows of F complex values, one contiguous range: rows of B + 1 values are no whole 64-byte
// segments, but only the two ends of the range share a segment with another workgroup.
//
// Order.  Every output element is ONE chain from +0 over p ascending, each complex multiply-add four fmaf in a fixed order
// (built with -ffp-contract=off), a skipped term leaves the chain as it is (a select, never a product with zero).  The
// chain is a function of (T, P, t, direction) alone: the tile, the grid and the batch do not enter; zeros give +0; a lane
// never looks at another lane's values, so a NaN in X[r][s][f] stays in column (r, f).
//
// spectral_fir_stream.  Per row a ring of R >= P - 1 + Tc spectrum frames and a host integer `head`, the slot of the next
// frame to arrive; a chunk brings Tc <= kFirTile frames.  A lane owns one bin of one row and ALL Tc output frames (one frame
// tile per row), so the window slides through registers exactly as in fir_step with t0 = 0: frame s < 0 is ring slot
// (head + s) mod R.  The slots written, [head, head + Tc), are never among the slots read, [head - (P - 1), head), and a lane
// touches the column (row, bin) alone: the ring is updated in place by the launch that reads it, with no order between
// workgroups and no barrier.  No term is skipped -- a frame the stream has not received yet is a frame of zeros in the
// ring, and fmaf(h, +-0, acc) leaves a chain that started at +0 as it is for finite h -- so every output is the chain of
// at_spectral_fir on the linearised history, to the bit, and a function of (P, t) alone: head, R, the grid and the batch
// do not enter.
//
// spectral_fir_corr.  A lane owns one bin and kFirTile consecutive partitions; a row's frames are cut into slices of
// kCorrSlice = 64 (t ascending), the unit of work is (row, slice), units ordered by row, then slice.  Within a unit every
// accumulator is an fp32 fmaf chain from +0 over t ascending (the window of X slides through registers as above, gY[t] is
// loaded once per t); a unit's result is added to a double accumulator; a GROUP of consecutive units is one workgroup
// item and leaves one complex double per (p, f) in the workspace; a second kernel adds the groups in ascending order in
// double and rounds once.  Per-row filters: the units are the row's own slices, one group per row -- a row's gradient does
// not depend on the batch.  Shared filter: units of all rows, cut into groups by corr_plan(rows, T, P, F); the order is a
// function of the shape alone, so the same call gives the same bits.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"

namespace at_hip {

constexpr int kFirLanes = 256;
constexpr int kFirTile = 8;                              // output frames (fir) or partitions (corr) per lane
constexpr int kFirMaxGrid = 8192;                        // persistent workgroups past this grid
constexpr int kCorrSlice = 64;                           // frames per fp32 chain of the correlation
constexpr int kCorrMaxGroups = 256;
constexpr int kCorrWantItems = 2048;                     // the shared filter's groups are chosen to give about this many items
constexpr int kConvBlocks[5] = {128, 256, 512, 1024, 2048};
constexpr int kConvMaxPartitions = 4;                    // the block rule: the smallest block from 512 up with ceil(K / B) <= 4
constexpr int kConvFirstRuleBlock = 2;                   // (128 and 256 by request only: measured slower than 512 even at 513 taps)
constexpr int64_t kConvChunkElems = (int64_t)1 << 26;    // complex64 elements of one spectrum per chunk of rows

static_assert((kFirTile & (kFirTile - 1)) == 0, "slot indices are taken modulo the tile");
static_assert(kCorrSlice % kFirTile == 0, "a slice starts on a multiple of the tile");

// acc += h * x, four fmaf in this order
__device__ __forceinline__ float2 cmla(float2 acc, float2 h, float2 x) {
  acc.x = fmaf(h.x, x.x, acc.x);
  acc.x = fmaf(-h.y, x.y, acc.x);
  acc.y = fmaf(h.x, x.y, acc.y);
  acc.y = fmaf(h.y, x.x, acc.y);
  return acc;
}

// Where a step's frames of one (row, bin) column come from.  load(s): frame s; whole(lo, hi) and has(s): do frames lo .. hi,
// does frame s, exist -- the term of a frame that does not is skipped.
struct ClipFrames {                                      // the frames [0, T) of a clip
  const float2* __restrict__ Xc;
  long long F, T;
  __device__ __forceinline__ bool has(long long s) const { return s >= 0 && s < T; }
  __device__ __forceinline__ bool whole(long long lo, long long hi) const { return lo >= 0 && hi < T; }
  __device__ __forceinline__ float2 load(long long s) const { return has(s) ? Xc[s * F] : make_float2(0.f, 0.f); }
};
struct RingFrames {                                      // the frames s < 0 before a stream's chunk: ring slot (head + s) mod R
  const float2* ring;
  long long F, R, head;
  // every frame exists (one the stream has not received yet is a frame of zeros): a constant, so that no term is skipped
  static constexpr __device__ bool has(long long) { return true; }
  static constexpr __device__ bool whole(long long, long long) { return true; }
  __device__ __forceinline__ float2 load(long long s) const {
    long long slot = head + s;                           // -s <= P - 1 <= R - Tc: one wrap at the most
    if (slot < 0) slot += R;
    return ring[slot * F];
  }
};

// One partition step of the FIR.  Q = p mod kFirTile is a constant, so that the slot of every frame is one.
// Causal: output i reads X[t0 + i - p] from slot (i - Q) mod tile; the new frame X[t0 - p] replaces X[t0 + tile - p].
// Anticausal: output i reads X[t0 + i + p] from slot (i + Q) mod tile; the new frame X[t0 + tile - 1 + p] replaces X[t0 + p - 1].
template <typename Frames, bool ANTI, int Q>
__device__ __forceinline__ void fir_step(float2 (&acc)[kFirTile], float2 (&win)[kFirTile], const Frames& src,
                                         const float2* __restrict__ Hc, long long F, long long t0, long long p, bool conj) {
  constexpr int M = kFirTile - 1;
  if (p > 0) {                                           // p = 0: the window was loaded whole
    constexpr int slot = ANTI ? ((M + Q) & M) : ((kFirTile - Q) & M);
    win[slot] = src.load(ANTI ? t0 + M + p : t0 - p);
  }
  float2 h = Hc[p * F];
  if (conj) h.y = -h.y;
  const long long lo = ANTI ? t0 + p : t0 - p, hi = lo + M;          // the frames of X this step reads
  if (src.whole(lo, hi)) {
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) acc[i] = cmla(acc[i], h, win[ANTI ? ((i + Q) & M) : ((i - Q) & M)]);
  } else {
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) {
      const float2 v = cmla(acc[i], h, win[ANTI ? ((i + Q) & M) : ((i - Q) & M)]);
      if (src.has(lo + i)) acc[i] = v;                   // a skipped term leaves the chain untouched
    }
  }
}

template <typename Frames, bool ANTI, int Q>
struct FirSteps {
  static __device__ __forceinline__ void run(float2 (&acc)[kFirTile], float2 (&win)[kFirTile], const Frames& src,
                                             const float2* __restrict__ Hc, long long F, long long t0, long long p0,
                                             long long P, bool conj) {
    if (p0 + Q >= P) return;
    fir_step<Frames, ANTI, Q>(acc, win, src, Hc, F, t0, p0 + Q, conj);
    FirSteps<Frames, ANTI, Q + 1>::run(acc, win, src, Hc, F, t0, p0, P, conj);
  }
};
template <typename Frames, bool ANTI>
struct FirSteps<Frames, ANTI, kFirTile> {
  static __device__ __forceinline__ void run(float2 (&)[kFirTile], float2 (&)[kFirTile], const Frames&,
                                             const float2* __restrict__, long long, long long, long long, long long, bool) {}
};

template <bool ANTI>
__global__ __launch_bounds__(kFirLanes) void spectral_fir_kernel(const float2* __restrict__ X, long long x_row_stride,
                                                                 const float2* __restrict__ H, long long h_row_stride,
                                                                 float2* __restrict__ Y, long long rows, long long T,
                                                                 long long P, long long F, int conj) {
  const long long tiles = (T + kFirTile - 1) / kFirTile, chunks = (F + kFirLanes - 1) / kFirLanes;
  const long long items = rows * tiles * chunks;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long c = item % chunks, rt = item / chunks;
    const long long r = rt / tiles, t0 = (rt - r * tiles) * kFirTile;
    const long long f = c * kFirLanes + threadIdx.x;
    if (f >= F) continue;                                // no barrier in this kernel: a lane without a bin just leaves
    const float2* Xc = X + r * x_row_stride + f;
    const float2* Hc = H + r * h_row_stride + f;
    float2 acc[kFirTile], win[kFirTile];
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) {
      acc[i] = make_float2(0.f, 0.f);
      win[i] = (t0 + i < T) ? Xc[(t0 + i) * F] : make_float2(0.f, 0.f);
    }
    const ClipFrames src = {Xc, F, T};
    for (long long p0 = 0; p0 < P; p0 += kFirTile)
      FirSteps<ClipFrames, ANTI, 0>::run(acc, win, src, Hc, F, t0, p0, P, conj != 0);
    float2* Yc = Y + r * T * F + f;
#pragma unroll
    for (int i = 0; i < kFirTile; ++i)
      if (t0 + i < T) Yc[(t0 + i) * F] = acc[i];
  }
}

// The causal steps at t0 = 0 over the ring: frame -p comes from it and replaces frame kFirTile - p in the window.
// X: rows of Tc frames at x_row_stride; ring: (rows, R, F), read at [head - (P - 1), head) and written at [head, head + Tc)
// modulo R; Y: (rows, Tc, F).  Accumulators past Tc run on zeros and are not stored.
__global__ __launch_bounds__(kFirLanes) void spectral_fir_stream_kernel(const float2* __restrict__ X, long long x_row_stride,
                                                                        float2* ring, const float2* __restrict__ H,
                                                                        float2* __restrict__ Y, long long rows, int Tc,
                                                                        long long P, long long R, long long head,
                                                                        long long F) {
  const long long chunks = (F + kFirLanes - 1) / kFirLanes;
  const long long items = rows * chunks;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long c = item % chunks, r = item / chunks;
    const long long f = c * kFirLanes + threadIdx.x;
    if (f >= F) continue;                                // no barrier in this kernel: a lane without a bin just leaves
    const float2* Xc = X + r * x_row_stride + f;
    const float2* Hc = H + f;
    float2* ring_c = ring + r * R * F + f;
    float2 acc[kFirTile], win[kFirTile], in[kFirTile];
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) {
      acc[i] = make_float2(0.f, 0.f);
      win[i] = in[i] = (i < Tc) ? Xc[i * F] : make_float2(0.f, 0.f);
    }
    const RingFrames src = {ring_c, F, R, head};
    for (long long p0 = 0; p0 < P; p0 += kFirTile)
      FirSteps<RingFrames, false, 0>::run(acc, win, src, Hc, F, 0, p0, P, false);
    float2* Yc = Y + r * Tc * F + f;
#pragma unroll
    for (int i = 0; i < kFirTile; ++i)
      if (i < Tc) {
        Yc[i * F] = acc[i];
        long long slot = head + i;
        if (slot >= R) slot -= R;
        ring_c[slot * F] = in[i];                        // after every read of this column: the slots differ anyway
      }
  }
}

// One frame step of the correlation.  Q = (t - slice start) mod tile is a constant.  Accumulator i (partition p0 + i) reads
// X[t - p0 - i] from slot (Q - i) mod tile; the new frame X[t - p0] goes to slot Q, where X[t - p0 - tile] was.
template <int Q>
__device__ __forceinline__ void corr_step(float2 (&acc)[kFirTile], float2 (&win)[kFirTile], const float2* __restrict__ Xc,
                                          const float2* __restrict__ Gc, long long F, long long T, long long p0, long long t) {
  constexpr int M = kFirTile - 1;
  const long long s0 = t - p0;
  win[Q] = (s0 >= 0 && s0 < T) ? Xc[s0 * F] : make_float2(0.f, 0.f);
  const float2 g = Gc[t * F];
  if (s0 - M >= 0) {
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) {
      const float2 x = win[(Q - i) & M];
      acc[i] = cmla(acc[i], make_float2(x.x, -x.y), g);  // conj(X) gY
    }
  } else {
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) {
      const float2 x = win[(Q - i) & M];
      const float2 v = cmla(acc[i], make_float2(x.x, -x.y), g);
      if (s0 - i >= 0) acc[i] = v;                       // t < p: no such term
    }
  }
}

template <int Q>
struct CorrSteps {
  static __device__ __forceinline__ void run(float2 (&acc)[kFirTile], float2 (&win)[kFirTile], const float2* __restrict__ Xc,
                                             const float2* __restrict__ Gc, long long F, long long T, long long p0,
                                             long long t8, long long t_hi) {
    if (t8 + Q >= t_hi) return;
    corr_step<Q>(acc, win, Xc, Gc, F, T, p0, t8 + Q);
    CorrSteps<Q + 1>::run(acc, win, Xc, Gc, F, T, p0, t8, t_hi);
  }
};
template <>
struct CorrSteps<kFirTile> {
  static __device__ __forceinline__ void run(float2 (&)[kFirTile], float2 (&)[kFirTile], const float2* __restrict__,
                                             const float2* __restrict__, long long, long long, long long, long long, long long) {}
};

// units: (row, slice), row-major.  Filter row rh owns units [rh * units_per_filter, (rh + 1) * units_per_filter), cut into
// `groups` groups of `per_group` consecutive units (the last one shorter).  part: (filters, groups, P, F) complex double.
__global__ __launch_bounds__(kFirLanes) void spectral_corr_kernel(const float2* __restrict__ X, long long x_row_stride,
                                                                  const float2* __restrict__ G, double2* __restrict__ part,
                                                                  long long filters, long long units_per_filter,
                                                                  long long groups, long long per_group, long long slices,
                                                                  long long T, long long P, long long F) {
  const long long ptiles = (P + kFirTile - 1) / kFirTile, chunks = (F + kFirLanes - 1) / kFirLanes;
  const long long items = filters * groups * ptiles * chunks;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long c = item % chunks;
    long long q = item / chunks;
    const long long p0 = (q % ptiles) * kFirTile;
    q /= ptiles;
    const long long g = q % groups, rh = q / groups;
    const long long f = c * kFirLanes + threadIdx.x;
    if (f >= F) continue;
    double2 sum[kFirTile];
#pragma unroll
    for (int i = 0; i < kFirTile; ++i) sum[i] = make_double2(0.0, 0.0);
    const long long u_lo = g * per_group, u_end = u_lo + per_group < units_per_filter ? u_lo + per_group : units_per_filter;
    for (long long u = rh * units_per_filter + u_lo; u < rh * units_per_filter + u_end; ++u) {
      const long long r = u / slices, sl = u - r * slices;
      const long long t_lo = sl * kCorrSlice, t_hi = t_lo + kCorrSlice < T ? t_lo + kCorrSlice : T;
      if (t_hi <= p0) continue;                          // every term of this slice has t < p: exact zeros, nothing to add
      const float2* Xc = X + r * x_row_stride + f;
      const float2* Gc = G + r * T * F + f;
      float2 acc[kFirTile], win[kFirTile];
#pragma unroll
      for (int i = 0; i < kFirTile; ++i) {
        acc[i] = make_float2(0.f, 0.f);
        const long long s = t_lo - p0 - i;               // the window before the slice's first frame; slot 0 is loaded by it
        win[(kFirTile - i) & (kFirTile - 1)] = (i > 0 && s >= 0 && s < T) ? Xc[s * F] : make_float2(0.f, 0.f);
      }
      for (long long t8 = t_lo; t8 < t_hi; t8 += kFirTile) CorrSteps<0>::run(acc, win, Xc, Gc, F, T, p0, t8, t_hi);
#pragma unroll
      for (int i = 0; i < kFirTile; ++i) {
        sum[i].x += (double)acc[i].x;
        sum[i].y += (double)acc[i].y;
      }
    }
    double2* out = part + ((rh * groups + g) * P + p0) * F + f;
#pragma unroll
    for (int i = 0; i < kFirTile; ++i)
      if (p0 + i < P) out[i * F] = sum[i];
  }
}

// gH[rh][p][f] = round(sum over the groups, ascending, in double)
__global__ __launch_bounds__(kFirLanes) void spectral_corr_finish_kernel(const double2* __restrict__ part,
                                                                         float2* __restrict__ gH, long long filters,
                                                                         long long groups, long long PF) {
  const long long n = filters * PF;
  for (long long e = (long long)blockIdx.x * kFirLanes + threadIdx.x; e < n; e += (long long)gridDim.x * kFirLanes) {
    const long long rh = e / PF, j = e - rh * PF;
    const double2* src = part + rh * groups * PF + j;
    double2 s = make_double2(0.0, 0.0);
    for (long long g = 0; g < groups; ++g) {
      s.x += src[g * PF].x;
      s.y += src[g * PF].y;
    }
    gH[e] = make_float2((float)s.x, (float)s.y);
  }
}

struct CorrPlan {
  long long filters, units_per_filter, groups, per_group, slices;
};

// groups of the shared filter: enough items to fill the chip, a function of the shape alone.  T >= 1: the callers answer
// T == 0 before they plan (no units, nothing to group)
static CorrPlan corr_plan(int64_t rows, int64_t T, int64_t P, int F, int shared) {
  CorrPlan pl;
  pl.slices = (T + kCorrSlice - 1) / kCorrSlice;
  if (!shared) {
    pl.filters = rows;
    pl.units_per_filter = pl.slices;
    pl.groups = 1;
    pl.per_group = pl.slices;
    return pl;
  }
  pl.filters = 1;
  pl.units_per_filter = rows * pl.slices;
  const long long per_group_items = ((P + kFirTile - 1) / kFirTile) * ((F + kFirLanes - 1) / kFirLanes);
  long long want = (kCorrWantItems + per_group_items - 1) / per_group_items;
  if (want > kCorrMaxGroups) want = kCorrMaxGroups;
  if (want > pl.units_per_filter) want = pl.units_per_filter;
  if (want < 1) want = 1;
  pl.per_group = (pl.units_per_filter + want - 1) / want;
  pl.groups = (pl.units_per_filter + pl.per_group - 1) / pl.per_group;
  return pl;
}

static int fir_check_shape(int64_t rows, int64_t T, int64_t P, int F) {
  if (rows < 0 || T < 0 || P < 0 || F < 1) return AT_EINVAL;
  if (rows > 0 && T > 0 && T > INT64_MAX / 16 / F / rows) return AT_EUNSUPPORTED;     // 64-bit byte offsets
  if (rows > 0 && P > 0 && P > INT64_MAX / 16 / F / rows / kCorrMaxGroups) return AT_EUNSUPPORTED;
  return AT_OK;
}

static unsigned fir_grid(long long items) { return (unsigned)(items < kFirMaxGrid ? items : kFirMaxGrid); }

// the block of K taps: block = 0 is the shipped rule, any other value must be a member of the ladder (0: it is not)
static int64_t conv_block(int64_t K, int block) {
  if (block == 0) {
    for (int i = kConvFirstRuleBlock; i < 5; ++i)
      if ((K + kConvBlocks[i] - 1) / kConvBlocks[i] <= kConvMaxPartitions) return kConvBlocks[i];
    return kConvBlocks[4];
  }
  for (int i = 0; i < 5; ++i)
    if (block == kConvBlocks[i]) return block;
  return 0;
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_fft_convolve_plan(int64_t L, int64_t K, int block, int64_t* B, int64_t* T, int64_t* P, int* frame_tile,
                         int64_t* chunk_rows) {
  if (!B || !T || !P || !frame_tile || !chunk_rows) return AT_EINVAL;
  if (L < 1 || K < 1 || block < 0) return AT_EINVAL;
  if (L > INT64_MAX / 4 - K) return AT_EUNSUPPORTED;
  const int64_t b = conv_block(K, block);
  if (b == 0) return AT_EINVAL;
  const int64_t M = L + K - 1;
  *B = b;
  *T = (M + b - 1) / b;
  *P = (K + b - 1) / b;
  *frame_tile = kFirTile;
  const int64_t per_row = *T * (b + 1);
  *chunk_rows = per_row >= kConvChunkElems ? 1 : kConvChunkElems / per_row;
  return AT_OK;
}

int at_spectral_fir(const float* X_complex, int64_t x_row_stride, const float* H_complex, int64_t h_row_stride, int64_t rows,
                    int64_t T, int64_t P, int F, int anticausal, int conj, float* Y_complex, void* stream) {
  const int rc = fir_check_shape(rows, T, P, F);
  if (rc != AT_OK) return rc;
  if ((anticausal != 0 && anticausal != 1) || (conj != 0 && conj != 1)) return AT_EINVAL;
  if (x_row_stride < 0 || h_row_stride < 0) return AT_EINVAL;
  if (rows == 0 || T == 0) return AT_OK;
  if (!X_complex || !Y_complex || (P > 0 && !H_complex)) return AT_EINVAL;
  if (x_row_stride < T * F || (h_row_stride != 0 && h_row_stride < P * F)) return AT_EINVAL;
  if (((uintptr_t)X_complex | (uintptr_t)H_complex | (uintptr_t)Y_complex) & 7) return AT_EINVAL;
  const long long items = (long long)rows * ((T + kFirTile - 1) / kFirTile) * ((F + kFirLanes - 1) / kFirLanes);
  const dim3 grid(fir_grid(items)), block(kFirLanes);
  hipStream_t st = (hipStream_t)stream;
  if (anticausal)
    hipLaunchKernelGGL(spectral_fir_kernel<true>, grid, block, 0, st, (const float2*)X_complex, (long long)x_row_stride,
                       (const float2*)H_complex, (long long)h_row_stride, (float2*)Y_complex, (long long)rows, (long long)T,
                       (long long)P, (long long)F, conj);
  else
    hipLaunchKernelGGL(spectral_fir_kernel<false>, grid, block, 0, st, (const float2*)X_complex, (long long)x_row_stride,
                       (const float2*)H_complex, (long long)h_row_stride, (float2*)Y_complex, (long long)rows, (long long)T,
                       (long long)P, (long long)F, conj);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_fft_convolve_stream_plan(int64_t K, int block, int64_t* B, int64_t* P, int64_t* R, int64_t* max_frames) {
  if (!B || !P || !R || !max_frames) return AT_EINVAL;
  if (K < 1 || block < 0) return AT_EINVAL;
  if (K > INT64_MAX / 4) return AT_EUNSUPPORTED;
  const int64_t b = conv_block(K, block);
  if (b == 0) return AT_EINVAL;
  *B = b;
  *P = (K + b - 1) / b;
  *R = *P - 1 + kFirTile;
  *max_frames = kFirTile;
  return AT_OK;
}

int at_spectral_fir_stream(const float* X_complex, int64_t x_row_stride, float* ring_complex, const float* H_complex,
                           int64_t rows, int64_t Tc, int64_t P, int64_t R, int64_t head, int F, float* Y_complex,
                           void* stream) {
  if (rows < 0 || Tc < 0 || Tc > kFirTile || P < 1 || F < 1 || x_row_stride < 0) return AT_EINVAL;
  if (R < P - 1 + Tc || head < 0 || head >= R) return AT_EINVAL;
  if (rows > 0 && R > INT64_MAX / 16 / F / rows) return AT_EUNSUPPORTED;               // 64-bit byte offsets
  if (rows > 0 && x_row_stride > INT64_MAX / 16 / rows) return AT_EUNSUPPORTED;
  if (rows == 0 || Tc == 0) return AT_OK;                // nothing arrived: the ring stays as it is
  if (!X_complex || !ring_complex || !H_complex || !Y_complex) return AT_EINVAL;
  if (x_row_stride < Tc * F) return AT_EINVAL;
  if (((uintptr_t)X_complex | (uintptr_t)ring_complex | (uintptr_t)H_complex | (uintptr_t)Y_complex) & 7) return AT_EINVAL;
  const long long items = (long long)rows * ((F + kFirLanes - 1) / kFirLanes);
  hipLaunchKernelGGL(spectral_fir_stream_kernel, dim3(fir_grid(items)), dim3(kFirLanes), 0, (hipStream_t)stream,
                     (const float2*)X_complex, (long long)x_row_stride, (float2*)ring_complex, (const float2*)H_complex,
                     (float2*)Y_complex, (long long)rows, (int)Tc, (long long)P, (long long)R, (long long)head, (long long)F);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

size_t at_spectral_fir_corr_workspace_bytes(int64_t rows, int64_t T, int64_t P, int F, int shared) {
  if (fir_check_shape(rows, T, P, F) != AT_OK || rows == 0 || P == 0 || T == 0) return 0;   // T == 0: zeros, no partial sums
  const CorrPlan pl = corr_plan(rows, T, P, F, shared);
  return (size_t)pl.filters * pl.groups * P * F * sizeof(double2);
}

int at_spectral_fir_corr(const float* X_complex, int64_t x_row_stride, const float* gY_complex, int64_t rows, int64_t T,
                         int64_t P, int F, int shared, float* gH_complex, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const int rc = fir_check_shape(rows, T, P, F);
  if (rc != AT_OK) return rc;
  if ((shared != 0 && shared != 1) || x_row_stride < 0) return AT_EINVAL;
  if (rows == 0 || P == 0) return AT_OK;
  if (!gH_complex || (T > 0 && (!X_complex || !gY_complex))) return AT_EINVAL;
  if (x_row_stride < T * F) return AT_EINVAL;
  if (((uintptr_t)X_complex | (uintptr_t)gY_complex | (uintptr_t)gH_complex) & 7) return AT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (T == 0) {                                          // no frames: the gradient is +0 (and there are no units to plan)
    const hipError_t e = hipMemsetAsync(gH_complex, 0, (size_t)(shared ? 1 : rows) * P * F * sizeof(float2), st);
    return e == hipSuccess ? AT_OK : AT_ELAUNCH;
  }
  const CorrPlan pl = corr_plan(rows, T, P, F, shared);
  const size_t need = (size_t)pl.filters * pl.groups * P * F * sizeof(double2);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) return AT_EWORKSPACE;
  const long long items = pl.filters * pl.groups * ((P + kFirTile - 1) / kFirTile) * ((F + kFirLanes - 1) / kFirLanes);
  hipLaunchKernelGGL(spectral_corr_kernel, dim3(fir_grid(items)), dim3(kFirLanes), 0, st, (const float2*)X_complex,
                     (long long)x_row_stride, (const float2*)gY_complex, (double2*)workspace, pl.filters, pl.units_per_filter,
                     pl.groups, pl.per_group, pl.slices, (long long)T, (long long)P, (long long)F);
  if (hipGetLastError() != hipSuccess) return AT_ELAUNCH;
  const long long n = pl.filters * P * F;
  hipLaunchKernelGGL(spectral_corr_finish_kernel, dim3(fir_grid((n + kFirLanes - 1) / kFirLanes)), dim3(kFirLanes), 0, st,
                     (const double2*)workspace, (float2*)gH_complex, pl.filters, pl.groups, (long long)P * F);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

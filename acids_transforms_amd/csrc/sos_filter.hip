// sos_filter.hip -- recursive (IIR) filtering by a cascade of second-order sections (scipy.signal.sosfilt's recurrence and
// state layout, restated), forwards or backwards in time, as one scan along each row of a (rows, L) tensor.
//
// Section k filters the output v of section k - 1 in the transposed direct form II,
//     y = b0 v + z1,   z1' = b1 v - a1 y + z2,   z2' = b2 v - a2 y           (a0 == 1),
// which is linear in its state s = (z1, z2):  s' = A s + Bv v,  y = b0 v + s[0],  A = [[-a1, 1], [-a2, 0]].  A lane that
// owns S consecutive samples runs them from a ZERO state in registers and gets outputs y_zs[i] and an end state e; with
// the true state s_in at the lane's first sample
//     y[i] = y_zs[i] + (A^i s_in)[0],        s_in(next lane) = A^S s_in + e,
// and since every lane uses the same matrices the second relation is a scan whose only constants are powers of A^S.
//
// One workgroup of 256 lanes owns a row and walks it in tiles of 256 x 16 samples.  A tile is requested with coalesced
// loads one tile ahead (16 floats per lane in registers), goes through LDS with a stride of 17 floats per lane so that a
// lane can pick up its 16 consecutive samples without bank conflicts, and leaves the same way.  Per section: the
// zero-state recurrence; an inclusive Hillis-Steele scan of the end states inside each wavefront (__shfl_up on the two
// doubles, constants (A^S)^(2^m)); the four wave totals meet in LDS, where every lane chains them onto the tile's incoming
// state in one order; the lane's own s_in = (A^S)^lane s_wave + (what the lanes below it in the wave add: the scan's value
// one lane down, an EXCLUSIVE prefix); the fix-up above, as the homogeneous recurrence from s_in.  The tile's outgoing state goes to the next tile through LDS.
// A lane's s_in is built from lanes before it only, and values are selected, never multiplied by a zero mask: a NaN at
// sample n cannot reach a sample before n.
//
// Everything but the audio is double: the state, the coefficients (kernel arguments, by value) and the signal between
// sections, which is rounded to float once, after the last section.  An fp32 state, or fp32 coefficients, are 1e-4 off on
// a 20 Hz high-pass at 44.1 kHz.  Each workgroup computes the powers it needs into LDS in one fixed order (square and
// multiply, an entry per lane), so y[r][n] is a function of (sos, L, n, reverse) and row r's samples alone: the tile and the
// samples per lane are constants, there is one dispatch, and neither the batch nor the grid enters.  Built with
// -ffp-contract=off and every fma written out.
//
// reverse = 1 is the same walk over the row read and written back to front (logical sample m is x[L - 1 - m]), the tiling
// anchored at the row's last sample: bit for bit flip -> forward -> flip.  It is the adjoint of the forward filter with
// zero state, so this one kernel is the forward, the backward and both halves of zero-phase filtering.
//
// The same walk has three more endings (MODE below), forwards in time and (the first two) from zero state, for a row cut
// into hops of `hop` >= 16 samples, nh = L / hop of them whole (the samples past nh hop belong to no hop):
//   hop power   nothing of y is written: the last section's DOUBLE output is squared before any rounding and summed into
//               power[r][h], float64.  hop >= S, so a lane's samples touch at most two hops: a head sum and a tail sum, each a
//               chain in sample order.  The lane below's tail joins the head (tail + head), a segmented Hillis-Steele scan
//               keyed by the hop index adds the heads of a wave that share a hop, a hop that begins and ends inside one wave
//               is stored by its last lane, and lane 0 of the workgroup chains what is left -- per wave: the piece of the hop
//               that came in, the piece of the hop that goes out, the last lane's tail -- onto the open hop it carries from
//               tile to tile in registers; it does so behind the NEXT tile's first barrier (the ending has none of its own),
//               and behind one more at the row's end.  The tiling is anchored at sample 0, so which lanes, waves and tiles a hop meets
//               is a function of (hop, h): power[r][h] is a function of (sos, L, hop, h) and row r's samples alone.  No
//               atomics; sums are selected, never masked by a multiply, so a NaN at sample n leaves the hops before n / hop
//               as they were; zeros give +0.
//   hop scaled  u[r][n] = (float)(w[r][n / hop] y[n]) with w (rows, nh) float64, +0 for n >= nh hop: the backward of a
//               function of the hop powers, before the reverse filter.
//   hop stream  hop power over a STREAM: the row is the next chunk, it begins `filled` samples inside a hop that already holds
//               open_in[r], and the filter starts from zi.  The hops that complete, done = (filled + L) / hop of them, go to
//               power[r ld + first + k]; the trailing partial hop is hop index `done` -- every sample of the chunk is live --
//               and its sum goes to open_out[r] (+0 when the chunk ends where a hop ends); zf comes from the owner lane.
//               zf may be zi and open_out may be open_in: a row's state is read at the row's start by the one workgroup
//               that writes it at the row's end.  The tiling is anchored at the CHUNK's first sample, so a chunked stream's
//               hop powers agree with the one call within rounding, not to the bit; power, open_out and zf of row r are
//               functions of (sos, hop, filled, L), the row's samples and the row's incoming state alone.
// The hop index of a lane's first sample comes from one 32-bit division per tile (the tile's own offset into its first hop
// is carried along by additions); there is no division per sample.
//
// No workgroup ever waits for another one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/acids_hip.h"

namespace at_hip {

constexpr int kSosLanes = 256;
constexpr int kSosPerLane = 16;                          // S
constexpr int kSosTile = kSosLanes * kSosPerLane;
constexpr int kSosStride = kSosPerLane + 1;              // floats per lane in LDS: 17 is odd, so 64 lanes hit 64 banks
constexpr int kSosWaves = kSosLanes / 64;
constexpr int kSosMaxSections = 16;
constexpr int kSosMaxGrid = 2048;                        // persistent workgroups: rows past the grid are walked in turn
// a section's table of 2 x 2 matrices in LDS: (A^S)^0 .. (A^S)^64
constexpr int kSosEntries = 65;
// how a tile leaves: y as float; its squares summed per hop in double; y times a per-hop weight as float
constexpr int kSosFilter = 0, kSosHopPower = 1, kSosHopScaled = 2;
// hop power over a stream: the row is a chunk that begins `filled` samples inside a hop, from a filter state
constexpr int kSosHopStream = 3;
constexpr int kSosMinHop = kSosPerLane;                  // a lane's samples touch at most two hops

struct SosHop {
  int hop;                                               // samples per hop
  long long nh;                                          // whole hops in a row: L / hop
  const double* w;                                       // hop scaled: (rows, nh)
  double* power;                                         // hop power: (rows, nh)
};

// hop power over a stream.  nh counts the hops that complete inside the chunk, (filled + L) / hop: hop k of the chunk is
// power[r ld + first + k], and the trailing partial hop is hop index nh, which goes to open_out.  The states are not the
// kernel's __restrict__ arguments: zf may be zi and open_out may be open_in.
struct SosStream : SosHop {
  unsigned filled;                                       // samples the open hop already holds: 0 .. hop - 1
  long long ld, first;
  const double* zi;                                      // (rows, n, 2), or null for zeros
  double* zf;
  const double* open_in;                                 // (rows,), or null for zeros
  double* open_out;
};
template <int MODE>
using SosEnding = std::conditional_t<MODE == kSosHopStream, SosStream, SosHop>;

struct SosCoef {
  double c[kSosMaxSections][5];                          // b0 b1 b2 a1 a2
};

struct SosMat {
  double a, b, c, d;                                     // [[a, b], [c, d]]
};

__device__ __forceinline__ SosMat sos_mul(const SosMat& x, const SosMat& y) {
  SosMat r;
  r.a = fma(x.a, y.a, x.b * y.c);
  r.b = fma(x.a, y.b, x.b * y.d);
  r.c = fma(x.c, y.a, x.d * y.c);
  r.d = fma(x.c, y.b, x.d * y.d);
  return r;
}
__device__ __forceinline__ void sos_put(double* t, const SosMat& m) {
  t[0] = m.a;
  t[1] = m.b;
  t[2] = m.c;
  t[3] = m.d;
}
__device__ __forceinline__ SosMat sos_get(const double* t) {
  SosMat m;
  m.a = t[0];
  m.b = t[1];
  m.c = t[2];
  m.d = t[3];
  return m;
}
// m s + t
__device__ __forceinline__ void sos_step(const SosMat& m, double s0, double s1, double t0, double t1, double& r0, double& r1) {
  r0 = fma(m.a, s0, fma(m.b, s1, t0));
  r1 = fma(m.c, s0, fma(m.d, s1, t1));
}
// The lane's index as a value the compiler takes for new: what is derived from it (addresses, bound masks of sixteen loads)
// is worked out where it is used, not once before all loops and kept in registers across them (64 of them, an occupancy step)
__device__ __forceinline__ int sos_fresh(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}
// where a tile's sample q 256 + tid sits in the staging buffer: t + t / S, written so that q is an immediate offset
__device__ __forceinline__ int sos_slot(int q, int tid) {
  return (tid + tid / kSosPerLane) + q * (kSosLanes + kSosLanes / kSosPerLane);
}

template <bool REV, int MODE>
__global__ __launch_bounds__(kSosLanes) void sos_filter_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               const double* __restrict__ zi, double* __restrict__ zf,
                                                               long long rows, long long L, SosCoef co, int n,
                                                               SosEnding<MODE> hp) {
  static_assert(MODE == kSosFilter || !REV, "the hop endings run forwards in time");
  constexpr bool STREAM = MODE == kSosHopStream;
  constexpr bool SUMS = MODE == kSosHopPower || STREAM;  // the two endings that sum squares per hop
  extern __shared__ double sos_tab[];                    // n x kSosEntries matrices
  __shared__ float stage[kSosLanes * kSosStride];
  __shared__ double wtot[kSosMaxSections][kSosWaves][2];
  __shared__ double carry[2][kSosMaxSections][2];        // the tile's incoming state, and the next tile's
  __shared__ double aside[kSosPerLane];                  // one lane's: see `owner`
  // hop power: what each wave hands to lane 0 of the workgroup -- the sums of the hops of its first and of its last lane,
  // its last lane's tail, and those two hop indices (counted from the tile's first hop) with the tail's flag
  __shared__ double hop_sum[SUMS ? kSosWaves : 1][3];
  __shared__ unsigned hop_idx[SUMS ? kSosWaves : 1][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // (A^S)^l for l = 0 .. 64 and every section: A^S by four squarings, then lane l raises it to its own power, bit by bit
  // from the top -- each entry in one fixed order, whatever the launch
  for (int k = 0; k < n; ++k) {
    SosMat P;
    P.a = -co.c[k][3];
    P.b = 1.0;
    P.c = -co.c[k][4];
    P.d = 0.0;
#pragma unroll
    for (int i = 1; i < kSosPerLane; i *= 2) P = sos_mul(P, P);
    if (tid <= 64) {
      SosMat Q = {1.0, 0.0, 0.0, 1.0};
      for (int bit = 6; bit >= 0; --bit) {
        Q = sos_mul(Q, Q);
        if ((tid >> bit) & 1) Q = sos_mul(P, Q);
      }
      sos_put(sos_tab + ((size_t)k * kSosEntries + tid) * 4, Q);
    }
  }

  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const float* xr = x + r * L;
    float* yr = y + r * L;
    if constexpr (STREAM) {                              // a row's state is read here by the one workgroup that writes it
      if (tid < n) {
        carry[0][tid][0] = hp.zi ? hp.zi[(r * n + tid) * 2] : 0.0;
        carry[0][tid][1] = hp.zi ? hp.zi[(r * n + tid) * 2 + 1] : 0.0;
      }
    } else if (tid < n) {
      carry[0][tid][0] = zi ? zi[(r * n + tid) * 2] : 0.0;
      carry[0][tid][1] = zi ? zi[(r * n + tid) * 2 + 1] : 0.0;
    }
    float pf[kSosPerLane];                               // the tile to come, as it was read: sample q 256 + tid
    auto request = [&](long long t0) {                   // logical sample t is x[L - 1 - t] when REV
      const int tid = sos_fresh(threadIdx.x);
      const float* p = REV ? xr + (L - 1 - t0 - tid) : xr + (t0 + tid);
      if (L - t0 >= kSosTile) {
#pragma unroll
        for (int q = 0; q < kSosPerLane; ++q) pf[q] = p[REV ? -q * kSosLanes : q * kSosLanes];
      } else {
        const int left = (int)(L - t0);                  // samples past L are zeros
#pragma unroll
        for (int q = 0; q < kSosPerLane; ++q) pf[q] = tid < left - q * kSosLanes ? p[REV ? -q * kSosLanes : q * kSosLanes] : 0.0f;
      }
    };
    request(0);
    int par = 0;
    // the hop endings: the tile's first sample lies in hop hop_base, hop_off samples after that hop's first one; lane 0
    // of the workgroup carries the hop that is still open, open_hop, and what it has of its sum
    long long hop_base = 0, open_hop = 0, handed_hop = 0;
    unsigned hop_off = 0;
    double open_sum = 0.0;
    if constexpr (STREAM) {                              // the chunk begins inside hop 0, which holds open_in already
      hop_off = hp.filled;
      if (tid == 0 && hp.open_in) open_sum = hp.open_in[r];
    }
    // hop power, lane 0 of the workgroup: what the waves handed over for the tile whose first hop is handed_hop goes onto
    // the open hop, wave by wave -- the piece of the hop that came into the wave, the hop that leaves it, its last lane's
    // tail -- and a hop is stored when the next one opens (and the open one at the row's end).  All twelve cells are read
    // first; the tile after has passed one barrier by then and rewrites them only behind another.
    auto chain = [&](bool row_ends) {
      double sum[kSosWaves][3];
      unsigned idx[kSosWaves][3];
#pragma unroll
      for (int w = 0; w < kSosWaves; ++w)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          sum[w][j] = hop_sum[w][j];
          idx[w][j] = hop_idx[w][j];
        }
      double* pr;
      if constexpr (STREAM) pr = hp.power + (r * hp.ld + hp.first);
      else pr = hp.power + r * hp.nh;
      auto close = [&]() {
        if (open_hop < hp.nh) pr[open_hop] = open_sum;
        else if constexpr (STREAM) {
          if (open_hop == hp.nh) hp.open_out[r] = open_sum;              // the trailing partial hop
        }
      };
#pragma unroll
      for (int w = 0; w < kSosWaves; ++w) {
        const long long h = handed_hop + idx[w][0];
        if (h == open_hop) {
          open_sum = open_sum + sum[w][0];
        } else {                                         // the wave begins where a hop begins
          close();
          open_sum = sum[w][0];
          open_hop = h;
        }
        if (idx[w][1] != idx[w][0]) {
          close();
          open_sum = sum[w][1];
          open_hop = handed_hop + idx[w][1];
        }
        if (idx[w][2]) {
          close();
          open_sum = sum[w][2];
          ++open_hop;
        }
      }
      if (row_ends) {
        close();
        if constexpr (STREAM) {
          if (open_hop < hp.nh) hp.open_out[r] = 0.0;    // the chunk ended where a hop ends: no lane met hop nh
        }
      }
    };
    auto tile = [&](auto tail, long long t0) {
      constexpr bool TAIL = decltype(tail)::value;       // the row's last tile: partial stores, and the final state
      const int rem = TAIL ? (int)(L - t0) : kSosTile;   // 1 .. kSosTile
#pragma unroll
      for (int q = 0; q < kSosPerLane; ++q) stage[sos_slot(q, tid)] = pf[q];
      __syncthreads();                                   // (also: the tables, and carry[0] at a row's first tile)
      if constexpr (SUMS) {
        if (t0 > 0 && tid == 0) chain(false);            // the tile before's hand-over, behind this tile's first barrier
      }
      double v[kSosPerLane];
#pragma unroll
      for (int i = 0; i < kSosPerLane; ++i) v[i] = (double)stage[tid * kSosStride + i];
      if (!TAIL) request(t0 + kSosTile);
      // where the lane's samples fall: its first one in hop hop_base + hr, the first `cut` of them (1 .. S) in that hop and
      // the rest in the next, and only the first `live` (0 .. S) inside a whole hop.  hop < 2^31, so `at` < 2^31 + tile.
      unsigned hr = 0;
      int cut = kSosPerLane, live = kSosPerLane;
      double w0 = 0.0, w1 = 0.0;
      const long long tile_hop = hop_base;
      if constexpr (MODE != kSosFilter) {
        const unsigned at = hop_off + (unsigned)(tid * kSosPerLane);
        hr = at / (unsigned)hp.hop;
        const long long ends = (long long)(hr + 1) * hp.hop - at;
        // (a stream's trailing partial hop counts: every sample of the chunk is live, and none past it)
        const long long left = (STREAM ? L : hp.nh * hp.hop) - (t0 + tid * kSosPerLane);
        cut = ends < kSosPerLane ? (int)ends : kSosPerLane;
        live = left < 0 ? 0 : left < kSosPerLane ? (int)left : kSosPerLane;
        if constexpr (MODE == kSosHopScaled) {
          const long long h = tile_hop + hr;
          if (h < hp.nh) w0 = hp.w[r * hp.nh + h];
          if (h + 1 < hp.nh) w1 = hp.w[r * hp.nh + h + 1];
        }
        hop_base += kSosTile / hp.hop;                   // the next tile's first sample, by additions
        hop_off += (unsigned)(kSosTile % hp.hop);
        if (hop_off >= (unsigned)hp.hop) {
          hop_off -= (unsigned)hp.hop;
          ++hop_base;
        }
      }
      // the lane of the row's last sample hands out the final state: it keeps each section's input to its cnt samples
      // aside and, once it knows its s_in, runs the recurrence itself over them
      double* zout = zf;
      if constexpr (STREAM) zout = hp.zf;
      const bool owner = TAIL && zout && tid == (rem - 1) / kSosPerLane;
      const int cnt = rem - tid * kSosPerLane;           // 1 .. S for the owner
      for (int k = 0; k < n; ++k) {
        const double b0 = co.c[k][0], b1 = co.c[k][1], b2 = co.c[k][2], na1 = -co.c[k][3], na2 = -co.c[k][4];
        const double* T = sos_tab + (size_t)k * kSosEntries * 4;
        double z1 = 0.0, z2 = 0.0;
        if (owner) {
#pragma unroll
          for (int i = 0; i < kSosPerLane; ++i) aside[i] = v[i];
        }
#pragma unroll
        for (int i = 0; i < kSosPerLane; ++i) {
          const double u = v[i];
          const double w = fma(b0, u, z1);
          z1 = fma(b1, u, fma(na1, w, z2));
          z2 = fma(b2, u, na2 * w);
          v[i] = w;
        }
        double e0 = z1, e1 = z2;
#pragma unroll 1
        for (int m = 0; m < 6; ++m) {
          const int d = 1 << m;
          const double u0 = __shfl_up(e0, d), u1 = __shfl_up(e1, d);
          const SosMat M = sos_get(T + d * 4);
          double f0, f1;
          sos_step(M, u0, u1, e0, e1, f0, f1);
          if (lane >= d) {
            e0 = f0;
            e1 = f1;
          }
        }
        if (lane == 63) {
          wtot[k][wave][0] = e0;
          wtot[k][wave][1] = e1;
        }
        double x0 = __shfl_up(e0, 1), x1 = __shfl_up(e1, 1);
        if (lane == 0) x0 = x1 = 0.0;
        __syncthreads();
        double g0 = carry[par][k][0], g1 = carry[par][k][1], h0 = g0, h1 = g1;
        const SosMat M64 = sos_get(T + 64 * 4);
#pragma unroll
        for (int w = 0; w < kSosWaves; ++w) {
          if (w == wave) {
            h0 = g0;
            h1 = g1;
          }
          sos_step(M64, g0, g1, wtot[k][w][0], wtot[k][w][1], g0, g1);
        }
        if (tid == 0) {
          carry[par ^ 1][k][0] = g0;
          carry[par ^ 1][k][1] = g1;
        }
        double s0, s1;
        sos_step(sos_get(T + lane * 4), h0, h1, x0, x1, s0, s1);
        if (owner) {
          double q1 = s0, q2 = s1;
#pragma unroll 1
          for (int i = 0; i < cnt; ++i) {
            const double u = aside[i];
            const double w = fma(b0, u, q1);
            q1 = fma(b1, u, fma(na1, w, q2));
            q2 = fma(b2, u, na2 * w);
          }
          zout[(r * n + k) * 2] = q1;
          zout[(r * n + k) * 2 + 1] = q2;
        }
        // the fix-up: y[i] += (A^i s_in)[0], the homogeneous recurrence from s_in
#pragma unroll
        for (int i = 0; i < kSosPerLane; ++i) {
          v[i] = v[i] + s0;
          const double t = fma(na1, s0, s1);
          s1 = na2 * s0;
          s0 = t;
        }
      }
      if constexpr (SUMS) {
        double head = 0.0, rest = 0.0;                   // the squares in the lane's first hop, and in the next
        if (__all(cut == kSosPerLane && live == kSosPerLane)) {          // the same sums without the selects
#pragma unroll
          for (int i = 0; i < kSosPerLane; ++i) head = head + v[i] * v[i];
        } else {
#pragma unroll
          for (int i = 0; i < kSosPerLane; ++i) {
            const double sq = v[i] * v[i];
            head = head + (i < cut && i < live ? sq : 0.0);
            rest = rest + (i >= cut && i < live ? sq : 0.0);
          }
        }
        const bool has_rest = cut < kSosPerLane;
        // (shuffles first, conditions after: a shuffle under `lane == 0 ||` would leave lane 0 out, and lane 1 reads it)
        const double below = __shfl_up(rest, 1);
        const int below_has = __shfl_up((int)has_rest, 1);
        const unsigned hr_below = __shfl_up(hr, 1);
        const bool opens = lane == 0 || hr_below != hr;                  // the first lane of its hop in this wave
        const unsigned long long heads = __ballot(opens);
        // hop indices ascend along the wave, so the lanes of a hop are a run: from `first` up to the lane below the next head
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        double c = lane > 0 && below_has ? below + head : head;
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
          const double u = __shfl_up(c, d);
          if (lane - d >= first) c = u + c;
        }
        const unsigned hr_first = __shfl(hr, 0);         // (a shuffle: every lane takes part)
        if (lane == 63 || ((heads >> (lane + 1)) & 1)) {   // the last lane of its hop in this wave
          if (first == 0) hop_sum[wave][0] = c;
          else if (lane == 63) hop_sum[wave][1] = c;
          else if constexpr (STREAM) {                   // begun and ended inside this wave
            const long long h = tile_hop + hr;
            if (h < hp.nh) hp.power[r * hp.ld + hp.first + h] = c;
            else if (h == hp.nh) hp.open_out[r] = c;     // (the lanes after it lie past the chunk)
          } else if (tile_hop + hr < hp.nh) hp.power[r * hp.nh + tile_hop + hr] = c;      // begun and ended inside this wave
        }
        if (lane == 63) {
          hop_sum[wave][2] = rest;
          hop_idx[wave][0] = hr_first;
          hop_idx[wave][1] = hr;
          hop_idx[wave][2] = has_rest;
        }
        handed_hop = tile_hop;                           // lane 0 chains these behind the next barrier
        par ^= 1;
        return;
      }
      if constexpr (MODE == kSosHopScaled) {
#pragma unroll
        for (int i = 0; i < kSosPerLane; ++i) v[i] = i < live ? (i < cut ? w0 : w1) * v[i] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < kSosPerLane; ++i) stage[tid * kSosStride + i] = (float)v[i] + 0.0f;     // -0 -> +0
      __syncthreads();
      const int tid = sos_fresh(threadIdx.x);
      float* p = REV ? yr + (L - 1 - t0 - tid) : yr + (t0 + tid);
#pragma unroll
      for (int q = 0; q < kSosPerLane; ++q) {
        if (!TAIL || tid < rem - q * kSosLanes) p[REV ? -q * kSosLanes : q * kSosLanes] = stage[sos_slot(q, tid)];
      }
      __syncthreads();
      par ^= 1;
    };
    long long t0 = 0;
    for (; t0 + kSosTile < L; t0 += kSosTile) tile(std::false_type(), t0);
    tile(std::true_type(), t0);
    if constexpr (SUMS) {
      __syncthreads();
      if (tid == 0) chain(true);
    }
  }
}

static int sos_check_shape(int64_t rows, int64_t L, int n_sections) {
  if (rows < 0 || L < 0 || n_sections < 1) return AT_EINVAL;
  if (n_sections > kSosMaxSections) return AT_EUNSUPPORTED;
  if (rows > 0 && L > INT64_MAX / 8 / rows) return AT_EUNSUPPORTED;        // 64-bit byte offsets
  return AT_OK;
}

// the sections as the kernels take them; false for a non-finite coefficient or a0 != 1
static bool sos_pack(const double* sos, int n_sections, SosCoef& co) {
  for (int k = 0; k < kSosMaxSections; ++k)
    for (int j = 0; j < 5; ++j) co.c[k][j] = 0.0;
  for (int k = 0; k < n_sections; ++k) {
    const double* s = sos + k * 6;
    for (int j = 0; j < 6; ++j)
      if (!isfinite(s[j])) return false;
    if (s[3] != 1.0) return false;
    co.c[k][0] = s[0];
    co.c[k][1] = s[1];
    co.c[k][2] = s[2];
    co.c[k][3] = s[4];
    co.c[k][4] = s[5];
  }
  return true;
}

// what the two hop endings share: the checks, then the forward walk from zero state with the ending MODE
template <int MODE>
static int sos_hop_launch(const float* x, int64_t rows, int64_t L, const double* sos, int n_sections, int64_t hop,
                          const double* w, double* power, float* u, void* stream) {
  const int rc = sos_check_shape(rows, L, n_sections);
  if (rc != AT_OK) return rc;
  if (!sos || hop < 1) return AT_EINVAL;
  if (hop < kSosMinHop) return AT_EUNSUPPORTED;
  SosCoef co;
  if (!sos_pack(sos, n_sections, co)) return AT_EINVAL;
  const int64_t nh = L / hop;
  if (rows == 0 || (MODE == kSosHopPower ? nh : L) == 0) return AT_OK;
  if (!x || (MODE == kSosHopPower ? !power : !u || (nh > 0 && !w))) return AT_EINVAL;
  if ((((uintptr_t)x | (uintptr_t)u) & 3) || (((uintptr_t)w | (uintptr_t)power) & 7)) return AT_EINVAL;
  if (nh == 0)                                           // hop scaled, no whole hop: every sample is past the last one
    return hipMemsetAsync(u, 0, (size_t)rows * L * sizeof(float), (hipStream_t)stream) == hipSuccess ? AT_OK : AT_ELAUNCH;
  if (hop > INT32_MAX) return AT_EUNSUPPORTED;           // (L >= 2^31 then)
  SosHop hp;
  hp.hop = (int)hop;
  hp.nh = nh;
  hp.w = w;
  hp.power = power;
  const dim3 grid((unsigned)(rows < kSosMaxGrid ? rows : kSosMaxGrid)), block(kSosLanes);
  const size_t lds = (size_t)n_sections * kSosEntries * 4 * sizeof(double);
  hipLaunchKernelGGL((sos_filter_kernel<false, MODE>), grid, block, lds, (hipStream_t)stream, x, u, (const double*)nullptr,
                     (double*)nullptr, (long long)rows, (long long)L, co, n_sections, hp);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_sos_filter_plan(int64_t rows, int64_t L, int n_sections, int64_t* tile, int64_t* per_lane, int* dispatch) {
  if (!tile || !per_lane || !dispatch) return AT_EINVAL;
  const int rc = sos_check_shape(rows, L, n_sections);
  if (rc != AT_OK) return rc;
  *tile = kSosTile;
  *per_lane = kSosPerLane;
  *dispatch = 0;                                         // one dispatch: a workgroup per row
  return AT_OK;
}

int at_sos_filter(const float* x, int64_t rows, int64_t L, const double* sos, int n_sections, int reverse, const double* zi,
                  double* zf, float* y, void* stream) {
  const int rc = sos_check_shape(rows, L, n_sections);
  if (rc != AT_OK) return rc;
  if (!sos || (reverse != 0 && reverse != 1) || (reverse && (zi || zf))) return AT_EINVAL;
  SosCoef co;
  if (!sos_pack(sos, n_sections, co)) return AT_EINVAL;
  if (((uintptr_t)zi | (uintptr_t)zf) & 7) return AT_EINVAL;
  if (zf && zf == zi) return AT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) return AT_OK;
  if (L == 0) {                                          // nothing to filter: the state passes through
    if (!zf) return AT_OK;
    const size_t bytes = (size_t)rows * n_sections * 2 * sizeof(double);
    const hipError_t e = zi ? hipMemcpyAsync(zf, zi, bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync(zf, 0, bytes, st);
    return e == hipSuccess ? AT_OK : AT_ELAUNCH;
  }
  if (!x || !y) return AT_EINVAL;
  if (((uintptr_t)x | (uintptr_t)y) & 3) return AT_EINVAL;
  const dim3 grid((unsigned)(rows < kSosMaxGrid ? rows : kSosMaxGrid)), block(kSosLanes);
  const size_t lds = (size_t)n_sections * kSosEntries * 4 * sizeof(double);
  const SosHop none = {0, 0, nullptr, nullptr};
  if (reverse) hipLaunchKernelGGL((sos_filter_kernel<true, kSosFilter>), grid, block, lds, st, x, y, zi, zf, (long long)rows, (long long)L, co, n_sections, none);
  else hipLaunchKernelGGL((sos_filter_kernel<false, kSosFilter>), grid, block, lds, st, x, y, zi, zf, (long long)rows, (long long)L, co, n_sections, none);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_sos_hop_power_plan(int64_t rows, int64_t L, int n_sections, int64_t hop, int64_t* tile, int64_t* per_lane,
                          int* dispatch) {
  if (!tile || !per_lane || !dispatch) return AT_EINVAL;
  const int rc = sos_check_shape(rows, L, n_sections);
  if (rc != AT_OK) return rc;
  if (hop < 1) return AT_EINVAL;
  if (hop < kSosMinHop || (hop > INT32_MAX && L / hop > 0)) return AT_EUNSUPPORTED;
  *tile = kSosTile;
  *per_lane = kSosPerLane;
  *dispatch = 0;                                         // one dispatch, the filter's: a workgroup per row
  return AT_OK;
}

int at_sos_hop_power(const float* x, int64_t rows, int64_t L, const double* sos, int n_sections, int64_t hop, double* power,
                     void* stream) {
  return sos_hop_launch<kSosHopPower>(x, rows, L, sos, n_sections, hop, nullptr, power, nullptr, stream);
}

int at_sos_filter_hop_scaled(const float* x, int64_t rows, int64_t L, const double* sos, int n_sections, int64_t hop,
                             const double* w, float* u, void* stream) {
  return sos_hop_launch<kSosHopScaled>(x, rows, L, sos, n_sections, hop, w, nullptr, u, stream);
}

int at_sos_hop_power_stream(const float* x, int64_t rows, int64_t n, const double* sos, int n_sections, int64_t hop,
                            int64_t filled, const double* zi, double* zf, const double* open_in, double* open_out,
                            double* power, int64_t ld, int64_t first, void* stream) {
  const int rc = sos_check_shape(rows, n, n_sections);
  if (rc != AT_OK) return rc;
  if (!sos || hop < 1 || n < 1 || ld < 0 || first < 0) return AT_EINVAL;
  if (hop < kSosMinHop) return AT_EUNSUPPORTED;
  if (filled < 0 || filled >= hop) return AT_EINVAL;
  SosCoef co;
  if (!sos_pack(sos, n_sections, co)) return AT_EINVAL;
  if (!x || !zf || !open_out || !power) return AT_EINVAL;
  if (n > INT64_MAX - filled) return AT_EUNSUPPORTED;
  const int64_t done = (filled + n) / hop;               // the hops that complete inside this chunk
  if (first > INT64_MAX - done || ld < first + done) return AT_EINVAL;
  if (((uintptr_t)x & 3) || (((uintptr_t)zi | (uintptr_t)zf | (uintptr_t)open_in | (uintptr_t)open_out | (uintptr_t)power) & 7))
    return AT_EINVAL;
  if (rows == 0) return AT_OK;
  if (hop > INT32_MAX) return AT_EUNSUPPORTED;
  if (ld > INT64_MAX / 8 / rows) return AT_EUNSUPPORTED;  // 64-bit byte offsets
  SosStream hp;
  hp.hop = (int)hop;
  hp.nh = done;
  hp.w = nullptr;
  hp.power = power;
  hp.filled = (unsigned)filled;
  hp.ld = ld;
  hp.first = first;
  hp.zi = zi;
  hp.zf = zf;
  hp.open_in = open_in;
  hp.open_out = open_out;
  const dim3 grid((unsigned)(rows < kSosMaxGrid ? rows : kSosMaxGrid)), block(kSosLanes);
  const size_t lds = (size_t)n_sections * kSosEntries * 4 * sizeof(double);
  hipLaunchKernelGGL((sos_filter_kernel<false, kSosHopStream>), grid, block, lds, (hipStream_t)stream, x, (float*)nullptr,
                     (const double*)nullptr, (double*)nullptr, (long long)rows, (long long)n, co, n_sections, hp);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

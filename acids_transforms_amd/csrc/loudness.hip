// loudness.hip -- the gating of ITU-R BS.1770 / EBU R128 on top of the hop powers of sos_filter.hip (at_sos_hop_power with
// the K-weighting sections), and what its backward needs.  Everything here is float64 and small: one number per 100 ms hop.
//
// power (clips, C, nh) holds s[c][h], the sum of the squared K-weighted samples of hop h of channel c; a hop has `hop`
// samples and a block `hb` hops (4: the 400 ms block with 75 % overlap; 30: the 3 s short-term window), nb = nh - hb + 1.
//     p_j = (sum over c ascending of G_c (s[c][j] + ... + s[c][j + hb - 1], hop ascending)) / (hb hop)
//     l_j = -0.691 + 10 log10 p_j                                        (block loudness; -inf where p_j == 0)
//     J1 = {j : p_j > abs_threshold},  Pabs = mean over J1,  J2 = {j in J1 : p_j > rel_ratio Pabs},  P = mean over J2,
//     loudness = -0.691 + 10 log10 P,  -inf when J1 is empty.
// The gates compare powers with thresholds that the host computed in double; no logarithm decides a gate.  `p > t` is
// evaluated as !(p <= t), so a NaN block passes both gates and a clip with a NaN reads NaN instead of dropping it.
//
// One workgroup of 256 lanes per clip, persistent past the grid; no workgroup waits for another one.  A mean is 256
// lane-strided chains in block order (lane t adds blocks t, t + 256, ...) joined by a fixed halving tree: the order is a
// function of nb alone, so a clip's result does not depend on the batch.  Every lane that needs p_j forms it with the same
// routine, so the masks that the backward recomputes from `power` and `stats` are the forward's.
//
// Backward: the gates are piecewise constant, hence constants of the graph, and what is left is linear in the hop powers:
// the kernels below write the weight w[c][h] of hop h of channel c such that dL/dy_c[n] = w[c][n / hop] y_c[n];
// at_sos_filter_hop_scaled forms that product and the reverse filter finishes.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/acids_hip.h"

namespace at_hip {

constexpr int kLoudLanes = 256;
constexpr int kLoudMaxGrid = 2048;                       // persistent workgroups: clips past the grid are taken in turn
constexpr int kLoudMaxChannels = 32;                     // the weights travel by value
constexpr int kLoudMaxBlockHops = 4096;                  // the backward keeps kLoudLanes + hb - 1 block terms in LDS
constexpr double kLoudOffset = -0.691;
constexpr double kLoudTenOverLn10 = 4.342944819032518;   // 10 / ln 10

struct LoudWeights {
  double g[kLoudMaxChannels];
};

// (ld: the hops between one channel's row and the next -- nh for a packed tensor, more for a window of a longer history)
__device__ __forceinline__ double loud_block_power(const double* __restrict__ pc, int C, long long ld, int hb, long long j,
                                                   const LoudWeights& G, double norm) {
  double acc = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* s = pc + c * ld + j;
    double sum = 0.0;
    for (int k = 0; k < hb; ++k) sum = sum + s[k];
    acc = acc + G.g[c] * sum;
  }
  return acc / norm;
}

__device__ __forceinline__ bool loud_above(double p, double threshold) {
  return !(p <= threshold);                              // a NaN is above every threshold
}

// the lanes' (sum, count) chains joined by a halving tree; every lane gets the totals
__device__ __forceinline__ void loud_join(double* rs, double* rn, int tid, double& s, double& n) {
  rs[tid] = s;
  rn[tid] = n;
  __syncthreads();
  for (int half = kLoudLanes / 2; half > 0; half /= 2) {
    if (tid < half) {
      rs[tid] = rs[tid] + rs[tid + half];
      rn[tid] = rn[tid] + rn[tid + half];
    }
    __syncthreads();
  }
  s = rs[0];
  n = rn[0];
  __syncthreads();
}

__global__ __launch_bounds__(kLoudLanes) void loudness_gate_kernel(const double* __restrict__ power, long long clips, int C,
                                                                   long long nh, long long ld, int hb, LoudWeights G, double norm,
                                                                   double abs_threshold, double rel_ratio,
                                                                   float* __restrict__ lufs, double* __restrict__ stats,
                                                                   float* __restrict__ block_lufs) {
  __shared__ double rs[kLoudLanes], rn[kLoudLanes];
  const int tid = threadIdx.x;
  const long long nb = nh - hb + 1;
  for (long long clip = blockIdx.x; clip < clips; clip += gridDim.x) {
    const double* pc = power + clip * C * ld;
    double s1 = 0.0, n1 = 0.0;
    for (long long j = tid; j < nb; j += kLoudLanes) {
      const double p = loud_block_power(pc, C, ld, hb, j, G, norm);
      if (block_lufs) block_lufs[clip * nb + j] = (float)(kLoudOffset + 10.0 * log10(p));
      if (loud_above(p, abs_threshold)) {
        s1 = s1 + p;
        n1 = n1 + 1.0;
      }
    }
    if (!lufs) continue;
    loud_join(rs, rn, tid, s1, n1);
    const double p_abs = n1 > 0.0 ? s1 / n1 : 0.0;
    const double rel_threshold = rel_ratio * p_abs;
    double s2 = 0.0, n2 = 0.0;
    if (n1 > 0.0) {
      for (long long j = tid; j < nb; j += kLoudLanes) {
        const double p = loud_block_power(pc, C, ld, hb, j, G, norm);
        if (loud_above(p, abs_threshold) && loud_above(p, rel_threshold)) {
          s2 = s2 + p;
          n2 = n2 + 1.0;
        }
      }
    }
    loud_join(rs, rn, tid, s2, n2);
    if (tid == 0) {
      const double p_rel = n2 > 0.0 ? s2 / n2 : 0.0;
      lufs[clip] = n2 > 0.0 ? (float)(kLoudOffset + 10.0 * log10(p_rel)) : -INFINITY;
      stats[clip * 3] = p_abs;
      stats[clip * 3 + 1] = p_rel;
      stats[clip * 3 + 2] = n2;
    }
  }
}

// Loudness range (EBU Tech 3342) of the block powers (hb = 30 by the host): with J2 as above (rel_ratio 0.01 by the host),
// n = |J2| and q the ascending order of {p_j : j in J2},
//     lra = 10 log10(q[rnd(0.95 (n - 1))] / q[rnd(0.10 (n - 1))]),   rnd(v) = floor(v + 0.5);   0 when n == 0.
// The two order statistics come from a radix select on the order-preserving unsigned image of the double's bits: eight
// passes of eight bits from the top, each a 256-bin histogram in LDS of the keys that share the prefix found so far, one
// histogram per statistic.  The counts are integers, so the LDS atomics cannot change the result: it is a function of the
// clip's hop powers alone.  The block powers are formed once, into `work`, by the lanes that read them back.
__device__ __forceinline__ unsigned long long loud_key(double p) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(p);
  return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double loud_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

__global__ __launch_bounds__(kLoudLanes) void loudness_range_kernel(const double* __restrict__ power, long long clips, int C,
                                                                    long long nh, long long ld, int hb, LoudWeights G,
                                                                    double norm, double abs_threshold, double rel_ratio,
                                                                    float* __restrict__ lra, double* __restrict__ stats,
                                                                    double* __restrict__ work) {
  __shared__ double rs[kLoudLanes], rn[kLoudLanes];
  __shared__ unsigned hist[2][256];
  __shared__ unsigned long long prefix[2], rank[2];
  const int tid = threadIdx.x;
  const long long nb = nh - hb + 1;
  for (long long clip = blockIdx.x; clip < clips; clip += gridDim.x) {
    const double* pc = power + clip * C * ld;
    double* ws = work + clip * nb;                       // lane t writes and reads blocks t, t + 256, ...: no barrier
    double s1 = 0.0, n1 = 0.0;
    for (long long j = tid; j < nb; j += kLoudLanes) {
      const double p = loud_block_power(pc, C, ld, hb, j, G, norm);
      ws[j] = p;
      if (loud_above(p, abs_threshold)) {
        s1 = s1 + p;
        n1 = n1 + 1.0;
      }
    }
    loud_join(rs, rn, tid, s1, n1);
    const double p_abs = n1 > 0.0 ? s1 / n1 : 0.0;
    const double rel_threshold = rel_ratio * p_abs;
    double nans = 0.0, n2 = 0.0;
    if (n1 > 0.0) {
      for (long long j = tid; j < nb; j += kLoudLanes) {
        const double p = ws[j];
        if (loud_above(p, abs_threshold) && loud_above(p, rel_threshold)) {
          n2 = n2 + 1.0;
          if (p != p) nans = nans + 1.0;
        }
      }
    }
    loud_join(rs, rn, tid, nans, n2);
    if (!(n2 > 0.0) || nans > 0.0) {                     // (uniform: every lane holds the joined values)
      if (tid == 0) {
        const double v = nans > 0.0 ? (double)NAN : 0.0;
        lra[clip] = (float)v;
        stats[clip * 4] = v;
        stats[clip * 4 + 1] = v;
        stats[clip * 4 + 2] = n2;
        stats[clip * 4 + 3] = p_abs;
      }
      continue;
    }
    if (tid < 2) {
      prefix[tid] = 0;
      rank[tid] = (unsigned long long)floor((tid ? 0.95 : 0.10) * (n2 - 1.0) + 0.5);
    }
    for (int byte = 7; byte >= 0; --byte) {
      hist[0][tid] = 0;
      hist[1][tid] = 0;
      __syncthreads();                                   // (also: prefix and rank)
      const unsigned long long pre0 = prefix[0], pre1 = prefix[1];
      for (long long j = tid; j < nb; j += kLoudLanes) {
        const double p = ws[j];
        if (loud_above(p, abs_threshold) && loud_above(p, rel_threshold)) {
          const unsigned long long key = loud_key(p);
          const unsigned long long above = byte == 7 ? 0ull : key >> (8 * byte + 8);
          const unsigned bin = (unsigned)(key >> (8 * byte)) & 255u;
          if (above == pre0) atomicAdd(&hist[0][bin], 1u);
          if (above == pre1) atomicAdd(&hist[1][bin], 1u);
        }
      }
      __syncthreads();
      if (tid == 0 || tid == 64) {                       // one lane per statistic walks its bins
        const int s = tid >> 6;
        unsigned long long k = rank[s], before = 0;
        int bin = 0;
        for (; bin < 255; ++bin) {
          const unsigned long long c = hist[s][bin];
          if (k < before + c) break;
          before += c;
        }
        rank[s] = k - before;
        prefix[s] = (prefix[s] << 8) | (unsigned long long)bin;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double lo = loud_unkey(prefix[0]), hi = loud_unkey(prefix[1]);
      lra[clip] = (float)(10.0 * log10(hi / lo));
      stats[clip * 4] = lo;
      stats[clip * 4 + 1] = hi;
      stats[clip * 4 + 2] = n2;
      stats[clip * 4 + 3] = p_abs;
    }
    __syncthreads();                                     // prefix is rewritten for the next clip
  }
}

// GATED: g (clips), the gradient of the integrated loudness; a block's term is 1 where it passed both gates, and
//   w[c][h] = g (10 / ln 10) / (P N2) G_c (2 / (hb hop)) (terms of the blocks that cover hop h), +0 SELECTED where N2 == 0.
// else:  g (clips, nb), the gradients of the block loudnesses; a block's term is g_j (10 / ln 10) / p_j, nothing where
//   p_j == 0, and w[c][h] = G_c (2 / (hb hop)) (terms of the blocks that cover hop h, j ascending).
// The hops are taken 256 at a time; the terms of the blocks that cover them meet in LDS, each formed once.
template <bool GATED>
__global__ __launch_bounds__(kLoudLanes) void loudness_weights_kernel(const double* __restrict__ power,
                                                                      const double* __restrict__ stats,
                                                                      const float* __restrict__ g, long long clips, int C,
                                                                      long long nh, int hb, LoudWeights G, double norm,
                                                                      double abs_threshold, double rel_ratio,
                                                                      double* __restrict__ w) {
  extern __shared__ double terms[];                      // kLoudLanes + hb - 1
  const int tid = threadIdx.x;
  const long long nb = nh - hb + 1;
  for (long long clip = blockIdx.x; clip < clips; clip += gridDim.x) {
    const double* pc = power + clip * C * nh;
    double rel_threshold = 0.0, scale = 0.0;
    bool any = true;
    if (GATED) {
      const double p_abs = stats[clip * 3], p_rel = stats[clip * 3 + 1], n2 = stats[clip * 3 + 2];
      rel_threshold = rel_ratio * p_abs;
      any = n2 > 0.0;
      scale = (double)g[clip] * kLoudTenOverLn10 / (p_rel * n2);
    }
    for (long long h0 = 0; h0 < nh; h0 += kLoudLanes) {
      for (int e = tid; e < kLoudLanes + hb - 1; e += kLoudLanes) {
        const long long j = h0 - (hb - 1) + e;           // terms[e] belongs to block j
        double term = 0.0;
        if (j >= 0 && j < nb && any) {
          const double p = loud_block_power(pc, C, nh, hb, j, G, norm);
          if (GATED) term = loud_above(p, abs_threshold) && loud_above(p, rel_threshold) ? 1.0 : 0.0;
          else term = p == 0.0 ? 0.0 : (double)g[clip * nb + j] * kLoudTenOverLn10 / p;
        }
        terms[e] = term;
      }
      __syncthreads();
      const long long h = h0 + tid;
      if (h < nh) {
        double sum = 0.0;                                // blocks h - hb + 1 .. h, those that exist
        for (int k = 0; k < hb; ++k) sum = sum + terms[tid + k];
        for (int c = 0; c < C; ++c) {
          const double share = G.g[c] * (2.0 / norm);
          double out;
          if (GATED) out = any && sum > 0.0 ? scale * share * sum : 0.0;
          else out = share * sum;
          w[(clip * C + c) * nh + h] = out;
        }
      }
      __syncthreads();
    }
  }
}

static int loud_check(int64_t clips, int C, int64_t nh, int64_t hop, int hb, const double* weights, LoudWeights& G) {
  if (clips < 0 || C < 1 || nh < 0 || hop < 1 || hb < 1 || !weights) return AT_EINVAL;
  if (C > kLoudMaxChannels || hb > kLoudMaxBlockHops) return AT_EUNSUPPORTED;
  if (clips > 0 && nh > INT64_MAX / 8 / C / clips) return AT_EUNSUPPORTED;          // 64-bit byte offsets
  for (int c = 0; c < kLoudMaxChannels; ++c) G.g[c] = 0.0;
  for (int c = 0; c < C; ++c) {
    if (!isfinite(weights[c])) return AT_EINVAL;
    G.g[c] = weights[c];
  }
  return AT_OK;
}

// a window of nh hops of rows that lie ld hops apart
static int loud_check_ld(int64_t clips, int C, int64_t nh, int64_t ld, int64_t hop, int hb, const double* weights, LoudWeights& G) {
  if (ld < nh) return AT_EINVAL;
  const int rc = loud_check(clips, C, nh, hop, hb, weights, G);
  if (rc != AT_OK) return rc;
  if (clips > 0 && ld > INT64_MAX / 8 / C / clips) return AT_EUNSUPPORTED;          // 64-bit byte offsets
  return AT_OK;
}

static dim3 loud_grid(int64_t clips) {
  return dim3((unsigned)(clips < kLoudMaxGrid ? clips : kLoudMaxGrid));
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_loudness_gate_ld(const double* power, int64_t clips, int C, int64_t nh, int64_t ld, int64_t hop, int hb,
                        const double* weights_host, double abs_threshold, double rel_ratio, float* lufs, double* stats,
                        float* block_lufs, void* stream) {
  LoudWeights G;
  const int rc = loud_check_ld(clips, C, nh, ld, hop, hb, weights_host, G);
  if (rc != AT_OK) return rc;
  if (lufs && (!isfinite(abs_threshold) || !isfinite(rel_ratio) || abs_threshold < 0.0 || rel_ratio < 0.0)) return AT_EINVAL;
  if ((!lufs && !block_lufs) || (lufs && !stats)) return AT_EINVAL;
  if (clips == 0) return AT_OK;
  if (nh < hb && !lufs) return AT_OK;                    // no block: nothing to write (the gated measure of it is -inf)
  if (!power && nh >= hb) return AT_EINVAL;
  if ((((uintptr_t)power | (uintptr_t)stats) & 7) || (((uintptr_t)lufs | (uintptr_t)block_lufs) & 3)) return AT_EINVAL;
  hipLaunchKernelGGL(loudness_gate_kernel, loud_grid(clips), dim3(kLoudLanes), 0, (hipStream_t)stream, power, (long long)clips,
                     C, (long long)nh, (long long)ld, hb, G, (double)hb * (double)hop, abs_threshold, rel_ratio, lufs, stats,
                     block_lufs);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_loudness_gate(const double* power, int64_t clips, int C, int64_t nh, int64_t hop, int hb, const double* weights_host,
                     double abs_threshold, double rel_ratio, float* lufs, double* stats, float* block_lufs, void* stream) {
  return at_loudness_gate_ld(power, clips, C, nh, nh, hop, hb, weights_host, abs_threshold, rel_ratio, lufs, stats, block_lufs,
                             stream);
}

int at_loudness_range(const double* power, int64_t clips, int C, int64_t nh, int64_t ld, int64_t hop, int hb,
                      const double* weights_host, double abs_threshold, double rel_ratio, float* lra, double* stats,
                      double* workspace, void* stream) {
  LoudWeights G;
  const int rc = loud_check_ld(clips, C, nh, ld, hop, hb, weights_host, G);
  if (rc != AT_OK) return rc;
  if (!isfinite(abs_threshold) || !isfinite(rel_ratio) || abs_threshold < 0.0 || rel_ratio < 0.0) return AT_EINVAL;
  if (!lra || !stats) return AT_EINVAL;
  if (clips == 0) return AT_OK;
  if (nh >= hb && (!power || !workspace)) return AT_EINVAL;
  if (nh - hb + 1 > INT32_MAX) return AT_EUNSUPPORTED;   // the histograms count in 32 bits
  if ((((uintptr_t)power | (uintptr_t)stats | (uintptr_t)workspace) & 7) || ((uintptr_t)lra & 3)) return AT_EINVAL;
  hipLaunchKernelGGL(loudness_range_kernel, loud_grid(clips), dim3(kLoudLanes), 0, (hipStream_t)stream, power, (long long)clips,
                     C, (long long)nh, (long long)ld, hb, G, (double)hb * (double)hop, abs_threshold, rel_ratio, lra, stats,
                     workspace);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_loudness_gate_backward(const double* power, const double* stats, const float* g, int64_t clips, int C, int64_t nh,
                              int64_t hop, int hb, const double* weights_host, double abs_threshold, double rel_ratio,
                              double* w, void* stream) {
  LoudWeights G;
  const int rc = loud_check(clips, C, nh, hop, hb, weights_host, G);
  if (rc != AT_OK) return rc;
  if (!isfinite(abs_threshold) || !isfinite(rel_ratio) || abs_threshold < 0.0 || rel_ratio < 0.0) return AT_EINVAL;
  if (clips == 0 || nh == 0) return AT_OK;
  if (!power || !stats || !g || !w) return AT_EINVAL;
  if ((((uintptr_t)power | (uintptr_t)stats | (uintptr_t)w) & 7) || ((uintptr_t)g & 3)) return AT_EINVAL;
  const size_t lds = (size_t)(kLoudLanes + hb - 1) * sizeof(double);
  hipLaunchKernelGGL(loudness_weights_kernel<true>, loud_grid(clips), dim3(kLoudLanes), lds, (hipStream_t)stream, power, stats,
                     g, (long long)clips, C, (long long)nh, hb, G, (double)hb * (double)hop, abs_threshold, rel_ratio, w);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_loudness_blocks_backward(const double* power, const float* g_blocks, int64_t clips, int C, int64_t nh, int64_t hop,
                                int hb, const double* weights_host, double* w, void* stream) {
  LoudWeights G;
  const int rc = loud_check(clips, C, nh, hop, hb, weights_host, G);
  if (rc != AT_OK) return rc;
  if (clips == 0 || nh == 0) return AT_OK;
  if (!power || !w || (nh >= hb && !g_blocks)) return AT_EINVAL;
  if ((((uintptr_t)power | (uintptr_t)w) & 7) || ((uintptr_t)g_blocks & 3)) return AT_EINVAL;
  const size_t lds = (size_t)(kLoudLanes + hb - 1) * sizeof(double);
  hipLaunchKernelGGL(loudness_weights_kernel<false>, loud_grid(clips), dim3(kLoudLanes), lds, (hipStream_t)stream, power,
                     (const double*)nullptr, g_blocks, (long long)clips, C, (long long)nh, hb, G, (double)hb * (double)hop, 0.0,
                     0.0, w);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

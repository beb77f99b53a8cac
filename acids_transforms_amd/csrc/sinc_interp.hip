// sinc_interp.hip -- band-limited sample-rate conversion without a polyphase bank (ops.resample_direct, PitchShift).
//
// With the rates reduced by their gcd to (orig, new), an entry of resample.hip's bank depends only on the integer
//     q = n new - o orig                    (n: input sample, o: output sample)
// through one even function h(q) that is exactly 0 in float32 beyond |q| = Qi (ops.sinc_table builds its half
// table[0 .. Qi] on the host in float64).  So the converter, and its adjoint with the two signals and the two rates
// exchanged, is ONE routine:
//     out[r][o] = sum over n ascending, 0 <= n < in_len, |n b - o a| <= Qi, of table[|n b - o a|] in[r][n]
// forward: (in = x, a = orig, b = new); backward: (in = g, a = new, b = orig).  A bank row of 2 width + orig taps holds
// only about 2 Qi / new + 1 entries that are not zero (13 of 161 at 147 -> 160), and this walks only those: one fmaf chain
// from +0.f over n ascending, which for finite input has the bits of at_resample_sinc's chain (fmaf(0, v, acc) == acc) and
// of at_resample_sinc_backward's (o ascending).  The chain is a function of (a, b, Qi, o, in_len) alone.
//
// One workgroup of 256 lanes takes a tile of T consecutive outputs of one row and stages the input window they reach,
// n = ceil((o0 a - Qi) / b) .. floor(((o0 + T - 1) a + Qi) / b), in LDS.  Lanes take consecutive outputs, so at one step
// of the chain neighbouring lanes read the window at the same or the next place (a broadcast or unit stride) and the
// table `a` entries apart, less b whenever the input index moves on.  Where b is several times an even a, a run of lanes
// strides by a with no such step between them and stacks on few of the 32 banks a 4-byte LDS read sees: 12 and 14 places
// on the busiest bank at 16 -> 441 and 32 -> 441.  The table is therefore staged at swz(q) = q + (q >> 5) + (q >> 10),
// which turns a stride of 32 m into 33 m and of 1024 m into 1057 m: 2 ... 4 places at every pair of rates counted, 3 %
// more LDS, and 1.5 ... 1.7 x faster at those two (profiles/sinc_interp_probe.md; at 147 <-> 160 and 441 -> 160, where the
// plain layout counts 1 ... 2, the difference does not show in the time).  The table goes into LDS once per persistent
// workgroup when it fits beside the window, and is read from global memory through L1 / L2, as it is, when it does not
// (450 KB at 18521 -> 14700).
// Rows and tiles are one flat 64-bit index that the workgroups stride over: no limit on the rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "persistent_launch.h"

namespace at_hip {

#ifndef AT_SI_SWIZZLE
#define AT_SI_SWIZZLE 1                          // A/B builds: EXTRA=-DAT_SI_SWIZZLE=0 stages the table as it is
#endif

constexpr int kSiThreads = 256;
constexpr int kSiTile = 1024;                    // outputs of a tile, at most
constexpr size_t kSiLdsBytes = 160 * 1024;
constexpr size_t kSiWindowBytes = 64 * 1024;     // T shrinks until the window is at most this

struct SiPlan {
  int a, b, Qi;
  int T;               // outputs of a tile
  int wlen;            // floats of the window a tile stages
  int table_in_lds;
  size_t lds;
};

// the place of table[q] in LDS
__host__ __device__ static inline int si_swz(int q) { return AT_SI_SWIZZLE ? q + (q >> 5) + (q >> 10) : q; }

// floats of the window of T outputs: the last output's last input is at most ((T - 1) a + 2 Qi) / b places behind the first
static inline long long si_window(long long T, long long a, long long b, long long Qi) {
  return ((T - 1) * a + 2 * Qi) / b + 2;
}

// AT_OK, or AT_EUNSUPPORTED when not even a one-output tile fits the LDS or the kernel's 32-bit tile arithmetic
static int si_plan(int a, int b, int Qi, SiPlan* p) {
  p->a = a; p->b = b; p->Qi = Qi;
  long long T = kSiTile;
  // inside a tile q and the numerators of the two divisions are ints: |.| <= T a + 2 Qi + 2 b
  while (T > 1 && (T * a + 2LL * Qi + 2LL * b > 0x7fffffffLL ||
                   (size_t)si_window(T, a, b, Qi) * sizeof(float) > kSiWindowBytes))
    T /= 2;
  if (T * a + 2LL * Qi + 2LL * b > 0x7fffffffLL) return AT_EUNSUPPORTED;
  const long long wlen = si_window(T, a, b, Qi);
  const size_t window = (size_t)((wlen + 3) & ~3LL) * sizeof(float);
  if (window > kSiLdsBytes) return AT_EUNSUPPORTED;
  p->T = (int)T;
  p->wlen = (int)wlen;
  const size_t table = ((size_t)si_swz(Qi) + 1) * sizeof(float);
  p->table_in_lds = window + table <= kSiLdsBytes;
  p->lds = window + (p->table_in_lds ? table : 0);
  return AT_OK;
}

// TL: the table is staged in LDS
template <bool TL>
__global__ __launch_bounds__(kSiThreads) void sinc_interp_kernel(const float* __restrict__ in, long long in_len,
                                                                  const float* __restrict__ table, long long out_len,
                                                                  long long tiles, long long units,
                                                                  float* __restrict__ out, SiPlan p) {
  extern __shared__ __attribute__((aligned(16))) float si_lds[];
  const int a = p.a, b = p.b, Qi = p.Qi;
  float* win = si_lds;                             // wlen, rounded up to 4
  float* tab = win + ((p.wlen + 3) & ~3);          // swz(Qi) + 1 when TL
  if (TL)
    for (int q = threadIdx.x; q <= Qi; q += kSiThreads) tab[si_swz(q)] = table[q];
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long row = unit / tiles;
    const long long o0 = (unit - row * tiles) * p.T;
    const float* ir = in + row * in_len;
    // the window starts at wn0 = ceil((o0 a - Qi) / b), the first input the tile's first output may reach
    const long long base = o0 * a - Qi;
    long long wn0 = base / b;
    if (base % b > 0) ++wn0;
    const int rel = (int)(base - wn0 * b);         // in (-b, 0]
    __syncthreads();                               // the table is staged; the previous tile's window is read
    for (int w = threadIdx.x; w < p.wlen; w += kSiThreads) {
      const long long n = wn0 + w;
      win[w] = (n >= 0 && n < in_len) ? ir[n] : 0.f;
    }
    __syncthreads();
    const int ns = out_len - o0 < (long long)p.T ? (int)(out_len - o0) : p.T;
    // the window places of the clip's own samples: n = wn0 + k with 0 <= n < in_len
    const long long last = in_len - 1 - wn0;       // may lie far before the window when out_len is not the converter's
    const int kmin = wn0 < 0 ? (int)(-wn0 < (long long)p.wlen ? -wn0 : p.wlen) : 0;
    const int kmax = last < 0 ? -1 : last < (long long)p.wlen - 1 ? (int)last : p.wlen - 1;
    float* orow = out + row * out_len + o0;
    for (int m = threadIdx.x; m < ns; m += kSiThreads) {
      // output o = o0 + m reaches n = wn0 + k, k = ceil(num / b) .. floor((num + 2 Qi) / b), num = o a - Qi - wn0 b > -b
      const int num = rel + m * a;
      int klo = (int)((unsigned)(num + b - 1) / (unsigned)b);
      const int numh = num + 2 * Qi;
      int khi = numh >= 0 ? (int)((unsigned)numh / (unsigned)b) : -1;
      klo = klo > kmin ? klo : kmin;
      khi = khi < kmax ? khi : kmax;
      // q = n b - o a, formed in 64 bits at the head of the chain; |q| <= Qi along it, so an int carries it on
      int q = (int)((wn0 + klo) * (long long)b - (o0 + m) * (long long)a);
      float acc = 0.f;
      for (int k = klo; k <= khi; ++k, q += b) {
        const int aq = q < 0 ? -q : q;
        acc = fmaf(TL ? tab[si_swz(aq)] : table[aq], win[k], acc);
      }
      orow[m] = acc;
    }
  }
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_sinc_interp_plan(int a, int b, int Qi, int* tile_outputs, int* table_in_lds) {
  if (a < 1 || b < 1 || Qi < 0 || !tile_outputs || !table_in_lds) return AT_EINVAL;
  SiPlan p;
  const int rc = si_plan(a, b, Qi, &p);
  if (rc != AT_OK) return rc;
  *tile_outputs = p.T;
  *table_in_lds = p.table_in_lds;
  return AT_OK;
}

int at_sinc_interp(const float* in, int64_t rows, int64_t in_len, int a, int b, const float* table, int Qi,
                   int64_t out_len, float* out, void* stream) {
  if (rows < 0 || in_len < 0 || out_len < 0 || a < 1 || b < 1 || Qi < 0) return AT_EINVAL;
  if (rows == 0 || out_len == 0) return AT_OK;
  if ((!in && in_len > 0) || !table || !out) return AT_EINVAL;
  // o a, n b and the flat unit index stay inside 64 bits
  if (out_len > 0x3fffffffffffffffLL / a || in_len > 0x3fffffffffffffffLL / b) return AT_EUNSUPPORTED;
  SiPlan p;
  const int rc = si_plan(a, b, Qi, &p);
  if (rc != AT_OK) return rc;
  const long long tiles = (out_len + p.T - 1) / p.T;
  if (rows > 0x7fffffffffffffffLL / tiles) return AT_EUNSUPPORTED;
  const long long units = (long long)rows * tiles;
  auto run = [&](auto kernel) {
    return persistent_launch(kernel, kSiThreads, p.lds, units, (hipStream_t)stream, in, (long long)in_len, table,
                             (long long)out_len, tiles, units, out, p);
  };
  return p.table_in_lds ? run(sinc_interp_kernel<true>) : run(sinc_interp_kernel<false>);
}

}  // extern "C"

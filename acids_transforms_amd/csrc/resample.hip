// resample.hip -- band-limited sample-rate conversion for the audio front end (`import_data`).
//
// Replaces torchaudio.transforms.Resample as the reference calls it (utils/misc.py:31-33: default arguments,
// i.e. Hann-windowed sinc interpolation, lowpass_filter_width 6, rolloff 0.99).  torchaudio is not part of the
// reference tree (requirements.txt:3, unpinned), so its published algorithm is restated: with the rates reduced
// by their gcd to (orig, new), every block of `orig` input samples yields `new` output samples,
//     y[i * new + j] = sum_k h[j][k] * xpad[i * orig + k],    k = 0 .. 2 width + orig - 1,
// xpad = x zero-padded by `width` in front and `width + orig` behind, h = the polyphase filter bank the host
// builds in float64 (utils/audio_io.py), rounded to float32.  One thread per output sample; the filter bank and
// the input window of a block of outputs sit in L1/L2 (h is at most a few hundred KB).
//
// The same kernel is the causal form of the chain, reading its window from a carried state (utils.RealtimeResample).  Below
// it: the adjoint of both, the transposed polyphase filter as a gather (autograd.ResampleFunction / ResampleStreamFunction).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "persistent_launch.h"
#include "stream_source.h"

namespace at_hip {

// The chain of both forms, over the source v = [state (H) | x (C) | zeros] of stream_source.h: the window of output block t
// starts H places before the chunk's sample t orig,
//     out[t new + j] = sum_k h[j][k] v[t orig + k],      k ascending, one fmaf each, from +0.f
// Offline (ST false): no state, H = width, C = L and the caller's out_len -- v is xpad.  The state reads and the
// workgroups that write one are compiled away.
// The causal form (ST true; utils.RealtimeResample): with D = ceil(width / orig) blocks of delay and H = Ha = D orig + width
// the sum is offline block t - D of the stream, with zeros before its start, and reads nothing behind the chunk (D orig >=
// width).  The workgroups behind the output's write the next state, the last Ha samples of v, into a second buffer.
template <bool ST>
__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, long long C,
                                                             const float* __restrict__ state_in,
                                                             float* __restrict__ state_out, int H, int orig, int nw,
                                                             int width, const float* __restrict__ h, long long out_len,
                                                             unsigned out_blocks, float* __restrict__ out) {
  const long long row = blockIdx.y;
  const StreamSource src = {ST && state_in ? state_in + row * H : nullptr, x + row * C, C, H};
  if (ST && blockIdx.x >= out_blocks) {
    const int s = (int)(blockIdx.x - out_blocks) * 256 + (int)threadIdx.x;
    if (s < H) state_out[row * H + s] = src.tail(s);
    return;
  }
  const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= out_len) return;
  const long long i = o / nw;
  const int j = (int)(o - i * nw);
  const int taps = 2 * width + orig;
  const float* hj = h + (long long)j * taps;
  out[row * out_len + o] = src.dot(hj, taps, i * orig - H, 0.f);      // tap 0 reads place i orig - H of the chunk
}

// ---- the adjoint (autograd.ResampleFunction / ResampleStreamFunction) -------------------------------------------------
// Output block i reads the inputs i orig - lead + k, k = 0 .. taps - 1 (lead = width offline, Ha in a stream), so
//     gx[n] = sum_{(i, j): 0 <= k = n - i orig + lead < taps} h[j][k] g[i new + j],      g zero outside [0, out_len)
// With n = b orig + r the blocks that reach n are i = b + d, d = dlo .. dhi, where k = r + lead - d orig: dlo =
// -floor((taps - 1 - lead) / orig) and dhi = floor((lead + orig - 1) / orig) bound every r, and a lane skips the d at
// which its own k leaves [0, taps).  One lane carries one input sample: ONE fmaf chain from +0.f over d ascending, j
// ascending -- o ascending -- so the chain is a function of (orig, new, taps, lead, n, out_len) alone: not of the rows,
// the tile or the grid.  No atomics.  Blocks i outside the gradient add h * 0 terms, which leave a chain's bits alone.
//
// One workgroup of 1024 lanes handles a tile of TB whole input blocks of one row (about kRbTile samples).  The window of g
// the tile reads, blocks b0 + dlo .. b0 + TB - 1 + dhi, is staged in LDS; at one step of the chain the lanes of an input
// block read ONE g (a broadcast) and neighbouring k of one bank row, so the bank is read at unit stride whether it sits
// in LDS (when it fits next to the window; staged once per workgroup) or comes through L1 / L2.  Rows and tiles are one
// flat 64-bit index that persistent workgroups stride over.
constexpr int kRbThreads = 1024;
constexpr int kRbTile = 1024;                    // input samples of a tile, about
constexpr size_t kRbLdsBytes = 160 * 1024;
constexpr size_t kRbWindowBytes = 64 * 1024;     // TB shrinks until the window is at most this

struct RbPlan {
  int orig, nw, taps, lead;
  int dlo, dhi;        // output block b + d reaches input block b for d = dlo .. dhi
  int TB;              // input blocks of a tile
  int wlen;            // floats of the window: (TB + dhi - dlo) new
  int bank_in_lds;
  size_t lds;
};

static inline long long rb_floor_div(long long a, long long b) { return a / b - ((a % b) < 0 ? 1 : 0); }      // b > 0

// AT_OK, or AT_EUNSUPPORTED when not even a one-block tile's window fits
static int rb_plan(int orig, int nw, int taps, int lead, RbPlan* p) {
  p->orig = orig; p->nw = nw; p->taps = taps; p->lead = lead;
  p->dlo = (int)-rb_floor_div((long long)taps - 1 - lead, orig);
  p->dhi = (int)rb_floor_div((long long)lead + orig - 1, orig);
  if ((long long)nw * taps > 0x7fffffffLL / 4 || (long long)lead + orig + taps > 0x7fffffffLL) return AT_EUNSUPPORTED;
  const long long halo = (long long)p->dhi - p->dlo;
  int TB = orig >= kRbTile ? 1 : kRbTile / orig;
  while (TB > 1 && (size_t)((TB + halo) * nw) * sizeof(float) > kRbWindowBytes) TB /= 2;
  const size_t window = (size_t)(((TB + halo) * nw + 3) & ~3LL) * sizeof(float);
  if (window > kRbLdsBytes) return AT_EUNSUPPORTED;
  p->TB = TB;
  p->wlen = (int)((TB + halo) * nw);
  const size_t bank = (size_t)nw * taps * sizeof(float);
  p->bank_in_lds = window + bank <= kRbLdsBytes;
  p->lds = window + (p->bank_in_lds ? bank : 0);
  return AT_OK;
}

// BL: the bank is staged in LDS.  NW: `new` as a compile-time constant (the x2 / :2 / 3:2 / 2:3 converters of a model's
// layers: the j loop is straight-line code), 0: p.nw -- the same chains
template <bool BL, int NW>
__global__ __launch_bounds__(kRbThreads) void resample_sinc_backward_kernel(const float* __restrict__ g, long long L,
                                                                             long long out_len, long long tiles,
                                                                             long long units, const float* __restrict__ h,
                                                                             float* __restrict__ gx, RbPlan p) {
  extern __shared__ __attribute__((aligned(16))) float rb_lds[];
  const int orig = p.orig, nw = NW ? NW : p.nw, taps = p.taps;
  float* gw = rb_lds;                              // wlen, rounded up to 4
  float* hb = gw + ((p.wlen + 3) & ~3);            // (new, taps) when BL
  if (BL)
    for (int i = threadIdx.x; i < nw * taps; i += kRbThreads) hb[i] = h[i];
  const float* hh = BL ? hb : h;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long row = unit / tiles;
    const long long b0 = (unit - row * tiles) * p.TB;
    const float* gr = g + row * out_len;
    const long long o0 = (b0 + p.dlo) * nw;        // output sample of gw[0]
    __syncthreads();                               // the bank is staged; the previous tile's window is read
    for (int q = threadIdx.x; q < p.wlen; q += kRbThreads) {
      const long long o = o0 + q;
      gw[q] = (o >= 0 && o < out_len) ? gr[o] : 0.f;
    }
    __syncthreads();
    const long long n0 = b0 * orig;
    const int ns = L - n0 < (long long)p.TB * orig ? (int)(L - n0) : p.TB * orig;
    float* gxr = gx + row * L + n0;
    for (int m = threadIdx.x; m < ns; m += kRbThreads) {
      const int bl = m / orig, r = m - bl * orig;
      float acc = 0.f;
      int k = r + p.lead - p.dlo * orig;           // of d = dlo; one block of outputs later it is orig less
      const float* gp = gw + bl * nw;
      for (int d = p.dlo; d <= p.dhi; ++d, k -= orig, gp += nw) {
        if ((unsigned)k >= (unsigned)taps) continue;
        const float* hp = hh + k;
        if (NW) {
#pragma unroll
          for (int j = 0; j < NW; ++j) acc = fmaf(hp[j * taps], gp[j], acc);
        } else {
#pragma unroll 8
          for (int j = 0; j < nw; ++j) acc = fmaf(hp[j * taps], gp[j], acc);
        }
      }
      gxr[m] = acc;
    }
  }
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_resample_backward_plan(int orig, int new_, int taps, int lead, int* tile_blocks, int* bank_in_lds) {
  if (orig <= 0 || new_ <= 0 || taps <= 0 || lead < 0 || !tile_blocks || !bank_in_lds) return AT_EINVAL;
  RbPlan p;
  const int rc = rb_plan(orig, new_, taps, lead, &p);
  if (rc != AT_OK) return rc;
  *tile_blocks = p.TB;
  *bank_in_lds = p.bank_in_lds;
  return AT_OK;
}

int at_resample_sinc_backward(const float* g, int64_t rows, int64_t L, int orig, int new_, int taps, int lead,
                              const float* filters, int64_t out_len, float* gx, void* stream) {
  if (rows < 0 || L < 0 || orig <= 0 || new_ <= 0 || taps <= 0 || lead < 0 || out_len < 0) return AT_EINVAL;
  if (L > 0x7fffffffffffffffLL / new_) return AT_EINVAL;
  if (taps == 2 * (int64_t)lead + orig && out_len != (L * new_ + orig - 1) / orig) return AT_EINVAL;      // lead == width
  if (rows == 0 || L == 0) return AT_OK;
  if ((!g && out_len > 0) || !filters || !gx) return AT_EINVAL;
  if (rows > 65535) return AT_EUNSUPPORTED;
  RbPlan p;
  const int rc = rb_plan(orig, new_, taps, lead, &p);
  if (rc != AT_OK) return rc;
  const long long nblk = (L + p.orig - 1) / p.orig;
  const long long tiles = (nblk + p.TB - 1) / p.TB;
  const long long units = (long long)rows * tiles;          // rows <= 65535
  auto run = [&](auto kernel) {
    return persistent_launch(kernel, kRbThreads, p.lds, units, (hipStream_t)stream, g, (long long)L, (long long)out_len,
                             tiles, units, filters, gx, p);
  };
  if (!p.bank_in_lds) return run(resample_sinc_backward_kernel<false, 0>);
  switch (new_) {
    case 1: return run(resample_sinc_backward_kernel<true, 1>);
    case 2: return run(resample_sinc_backward_kernel<true, 2>);
    case 3: return run(resample_sinc_backward_kernel<true, 3>);
    default: return run(resample_sinc_backward_kernel<true, 0>);
  }
}

int at_resample_sinc_stream(const float* x, int64_t rows, int64_t C, const float* state_in, float* state_out, int orig,
                            int new_, int width, const float* filters, float* out, void* stream) {
  if (rows < 0 || C < 0 || orig <= 0 || new_ <= 0 || width < 0) return AT_EINVAL;
  if (C % orig != 0 || (state_out && state_out == state_in)) return AT_EINVAL;
  if (rows == 0 || C == 0) return AT_OK;
  if (!x || !filters || !out) return AT_EINVAL;
  if (rows > 65535) return AT_EUNSUPPORTED;
  const int Ha = (width + orig - 1) / orig * orig + width;
  if (C / orig > 0x7fffffffLL * 128 / new_) return AT_EUNSUPPORTED;      // the grid's x extent
  const long long out_len = C / orig * new_;
  const unsigned out_blocks = (unsigned)((out_len + 255) / 256);
  const unsigned state_blocks = state_out ? (unsigned)((Ha + 255) / 256) : 0u;
  hipLaunchKernelGGL(resample_sinc_kernel<true>, dim3(out_blocks + state_blocks, (unsigned)rows), dim3(256), 0,
                     (hipStream_t)stream, x, (long long)C, state_in, state_out, Ha, orig, new_, width, filters, out_len,
                     out_blocks, out);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_resample_sinc(const float* x, int64_t rows, int64_t L, int orig, int new_, int width, const float* filters,
                     int64_t out_len, float* out, void* stream) {
  if (rows < 0 || L < 0 || orig <= 0 || new_ <= 0 || width < 0 || out_len < 0) return AT_EINVAL;
  if (rows == 0 || out_len == 0) return AT_OK;
  if (!x || !filters || !out) return AT_EINVAL;
  if (rows > 65535) return AT_EUNSUPPORTED;
  const unsigned out_blocks = (unsigned)((out_len + 255) / 256);
  hipLaunchKernelGGL(resample_sinc_kernel<false>, dim3(out_blocks, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, x,
                     (long long)L, (const float*)nullptr, (float*)nullptr, width, orig, new_, width, filters,
                     (long long)out_len, out_blocks, out);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // extern "C"

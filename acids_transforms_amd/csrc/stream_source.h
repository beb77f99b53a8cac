// stream_source.h -- what a streaming time-domain stage reads: the chunk of a row, the H entries before it from a carried
// state (or zeros), zeros behind it; and what it carries on.  Used by resample.hip (both forms of the forward chain) and by
// the state writes of pqmf.hip.  No HIP include: tests/stream_source_main.cpp compiles it alone with the host compiler.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define AT_HD __host__ __device__
#else
#define AT_HD
#endif

namespace at_hip {

// One row of s = [state (H) | chunk (C) | zeros], indexed by the place c in the chunk: the state's last entry is c = -1.
struct StreamSource {
  const float* state;   // H entries, or null: zeros
  const float* x;       // C entries
  long long C;
  int H;

  AT_HD float at(long long c) const {
    if (c >= C) return 0.0f;
    if (c >= 0) return x[c];
    return state && c >= -(long long)H ? state[c + H] : 0.0f;
  }
  // entry i of the next state, the last H entries of [state | chunk]
  AT_HD float tail(int i) const { return at(C - H + i); }

  // acc = fmaf(h[k], at(first + k), acc) for k = 0 .. n - 1 in this order: the chain a filter runs over a window that
  // starts at place `first`.  The taps at which the source changes (zeros | state | chunk | zeros) are found once, so that
  // no tap tests its place; a tap on zeros still is one fmaf, which keeps the chain's bits whatever h holds.
  AT_HD float dot(const float* h, int n, long long first, float acc) const {
    const int k1 = tap_of(0, first, n), k2 = tap_of(C, first, n);       // the chunk is taps [k1, k2)
    const int k0 = state ? tap_of(-(long long)H, first, n) : k1;        // the state is taps [k0, k1)
    int k = 0;
    for (; k < k0; ++k) acc = fmaf(h[k], 0.0f, acc);
    if (state)                                                          // (none: k0 == k1, and a kernel compiled without
      for (; k < k1; ++k) acc = fmaf(h[k], state[first + H + k], acc);  // state loses the loop)
    for (; k < k2; ++k) acc = fmaf(h[k], x[first + k], acc);
    for (; k < n; ++k) acc = fmaf(h[k], 0.0f, acc);
    return acc;
  }
  // the tap that reads place c, clamped to [0, n]
  static AT_HD int tap_of(long long c, long long first, int n) {
    const long long k = c - first;
    return k < 0 ? 0 : k > n ? n : (int)k;
  }
};

}  // namespace at_hip

// Host program of tests/test_stream_source_cpu.py: csrc/stream_source.h without a GPU.
//   stream_source   reads lines "C H has_state" from stdin, fills state with 1 .. H and x with 101 .. 100 + C, and prints
//                   one line each: at(c) for c = -H - 2 .. C + 2, then tail(i) for i = 0 .. H - 1, then "|" and, for every
//                   window of n = 4 taps h = 1, 10, 100, 1000 starting at first = -H - 5 .. C + 1, dot(h, n, first, 0.5)
//                   followed by the same chain written with at()
#include <math.h>
#include <stdio.h>

#include <vector>

#include "stream_source.h"

using namespace at_hip;

int main() {
  long long C;
  int H, has_state;
  const float h[4] = {1.f, 10.f, 100.f, 1000.f};
  while (scanf("%lld %d %d", &C, &H, &has_state) == 3) {
    if (C < 0 || H < 0) return 2;
    std::vector<float> state(H), x(C);
    for (int i = 0; i < H; ++i) state[i] = (float)(1 + i);
    for (long long i = 0; i < C; ++i) x[i] = (float)(101 + i);
    const StreamSource s = {has_state ? state.data() : nullptr, x.data(), C, H};
    for (long long c = -H - 2; c <= C + 2; ++c) printf("%g ", s.at(c));
    for (int i = 0; i < H; ++i) printf("%g ", s.tail(i));
    printf("|");
    for (long long first = -H - 5; first <= C + 1; ++first) {
      float chain = 0.5f;
      for (int k = 0; k < 4; ++k) chain = fmaf(h[k], s.at(first + k), chain);
      printf(" %.9g %.9g", s.dot(h, 4, first, 0.5f), chain);
    }
    printf("\n");
  }
  return 0;
}

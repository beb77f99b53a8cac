// Host program of tests/test_row_stream_cpu.py: csrc/row_stream.h without a GPU.
//   row_stream stream   for NB = 4, 8, 16, 32, every start frame g0 = 0 .. 63 and every run length n of kLengths: 64 lane
//                       instances of RowStream<NB> in lockstep write the run of frames g0 .. g0 + n - 1 (e0 = g0 F) into
//                       a recording store; the value of an element is its own index in the stream.  One line per case:
//                       "NB g0 n  good  bad  outside" -- elements of [e0, e0 + n F) written exactly once with their own
//                       index, writes that hit such an element again or with another value, writes outside the range.
//   row_stream cut      reads lines "units units_per_run" from stdin and prints the units of run r = 0, 1, .. as
//                       "u0:u1", up to and including the first run that has none ("-").
#include <stdio.h>
#include <string.h>

#include <vector>

#include "row_stream.h"

using namespace at_hip;

static const int kLengths[] = {1, 2, 3, 63, 64, 65, 130};

// the stream as the store sees it: hits per element of [lo, hi), and what went wrong
static long long* g_base;
static long long g_lo, g_hi, g_bad, g_outside;
static std::vector<int> g_hits;

struct Record {
  void operator()(long long* dst, long long val) const {
    const long long e = dst - g_base;
    if (e < g_lo || e >= g_hi) {
      ++g_outside;
      return;
    }
    if (val != e || g_hits[e - g_lo]++) ++g_bad;
  }
};

template <int NB>
static void run_case(int g0, int n) {
  constexpr long long F = 64 * NB + 1;
  std::vector<long long> stream((g0 + n) * F + 128);      // every slot a lane may point at; the store only records
  g_base = stream.data();
  g_lo = g0 * F;
  g_hi = g_lo + n * F;
  g_bad = g_outside = 0;
  g_hits.assign(n * F, 0);
  RowStream<NB, long long, Record> lanes[64];
  for (int lane = 0; lane < 64; ++lane) lanes[lane].begin(g_base, g_lo, lane);
  for (int g = g0; g < g0 + n; ++g) {
    for (int lane = 0; lane < 64; ++lane) {
      // what the transform core hands this lane: bins col + 64 m of frame g, and the Nyquist bin where col is 0
      const int col = (lane - lanes[lane].rot) & 63;
      long long z[NB];
      for (int m = 0; m < NB; ++m) z[m] = g * F + col + 64 * m;
      lanes[lane].emit(z, col == 0 ? g * F + 64 * NB : -1, lane);
    }
  }
  for (int lane = 0; lane < 64; ++lane) lanes[lane].end(lane);
  long long good = 0;
  for (int h : g_hits) good += h == 1;
  printf("%d %d %d  %lld %lld %lld\n", NB, g0, n, good, g_bad, g_outside);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "stream")) {
    for (int g0 = 0; g0 < 64; ++g0)
      for (int n : kLengths) {
        run_case<4>(g0, n);
        run_case<8>(g0, n);
        run_case<16>(g0, n);
        run_case<32>(g0, n);
      }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "cut")) {
    long long units, per;
    while (scanf("%lld %lld", &units, &per) == 2) {
      if (units < 1 || per < 1) return 2;
      for (long long r = 0;; ++r) {
        long long u0, u1;
        if (!run_units(r, per, units, u0, u1)) break;
        printf("%lld:%lld ", u0, u1);
      }
      printf("-\n");
    }
    return 0;
  }
  return 2;
}

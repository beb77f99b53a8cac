// Host program of tests/test_band_plan_cpu.py: the row plan of csrc/band_plan.h without a GPU.
//   band_plan            reads lines "tab_floats per_wave_bytes" (table floats before rounding, bytes of one wave's rows)
//                        from stdin and prints, one line each: ok tab_lds wpb tab_floats lds_bytes
//   band_plan --consts   prints kBandLdsBudget kBandKit pad64(1) pad64(64) pad64(65) band_tab_floats(5)
#include <stdio.h>
#include <string.h>

#include "band_plan.h"

using namespace at_hip;

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--consts")) {
    printf("%zu %d %d %d %d %lld\n", kBandLdsBudget, kBandKit, pad64(1), pad64(64), pad64(65), band_tab_floats(5));
    return 0;
  }
  if (argc != 1) return 2;
  long long floats;
  unsigned long long per_wave;
  while (scanf("%lld %llu", &floats, &per_wave) == 2) {
    const BandPlan pl = band_plan(band_tab_floats(floats), (size_t)per_wave);
    printf("%d %d %d %lld %zu\n", (int)pl.ok, (int)pl.tab_lds, pl.wpb, pl.tab_floats, pl.lds);
  }
  return 0;
}

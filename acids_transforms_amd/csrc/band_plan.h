// band_plan.h -- the row plan of the banded kernels that give one wave one row (autograd.hip, invert_grad.hip,
// mel_distance.hip), host only: no HIP include, so that tests/band_plan_main.cpp compiles it alone.
// mfcc_bwd_kernel plans for itself (always four waves, a tile of dF next to the tables, no cap on the waves of its
// global-memory form) and shares the budget and the two roundings only.
#pragma once
#include <stddef.h>

namespace at_hip {

constexpr size_t kBandLdsBudget = 160 * 1024;   // dynamic LDS of one workgroup (the tests' case files restate it)
constexpr int kBandKit = 9;                     // a row of K <= 64 * kBandKit = 576 bins stays in registers (staged tables)

inline int pad64(int x) { return (x + 63) / 64 * 64; }
// the staged tables end on a float4 boundary
inline long long band_tab_floats(long long floats) { return (floats + 3) / 4 * 4; }

struct BandPlan {
  bool ok;                // false: one wave's rows exceed the budget (AT_EUNSUPPORTED, -2)
  bool tab_lds;           // the tables are staged in LDS
  int wpb;                // waves, that is rows, per workgroup
  long long tab_floats;   // floats of the staged tables; 0 when they stay in global memory
  size_t lds;             // dynamic LDS bytes of a workgroup
};

// Tables in LDS when they (tab_floats, band_tab_floats of all of them) and four waves' rows (per_wave bytes each, > 0)
// fit the budget; else tables in global memory and as many waves as fit, four at the most; a row over the budget: !ok.
inline BandPlan band_plan(long long tab_floats, size_t per_wave) {
  const size_t staged = sizeof(float) * tab_floats + 4 * per_wave;
  if (staged <= kBandLdsBudget) return {true, true, 4, tab_floats, staged};
  if (per_wave > kBandLdsBudget) return {false, false, 0, 0, 0};
  int wpb = (int)(kBandLdsBudget / per_wave);
  if (wpb > 4) wpb = 4;
  return {true, false, wpb, 0, wpb * per_wave};
}

}  // namespace at_hip

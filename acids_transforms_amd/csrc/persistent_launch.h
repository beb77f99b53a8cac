// persistent_launch.h -- the one launcher of the kernels whose workgroups stride over a flat index of work units (the
// banded backward kernels of band_cols.h, pqmf.hip, resample.hip's backward, sinc_interp.hip): as many workgroups as the
// chip holds at once, at most one per unit.  The kernels that plan run lengths and rounds (run_plan.h, mel_banded.hip,
// mel_bf16.hip, pghi_heap.h, stft_*.hip) follow another rule and launch for themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/acids_hip.h"

namespace at_hip {

// Launches kernel(args...) with `threads` lanes per workgroup and lds bytes of dynamic LDS on min(occupancy x CUs, units)
// workgroups; what a workgroup stages, it stages once.  The device is asked on every call: the current one, on a host
// with several.  AT_OK, or AT_ELAUNCH.
template <typename Kernel, typename... Args>
int persistent_launch(Kernel kernel, int threads, size_t lds, long long units, hipStream_t stream, Args... args) {
  const void* fn = (const void*)kernel;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return AT_ELAUNCH;
  }
  int per_cu = 0, cus = 0, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess) {
    (void)hipGetLastError();
    return AT_ELAUNCH;
  }
  long long blocks = (long long)(per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
  if (blocks > units) blocks = units;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds, stream, args...);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // namespace at_hip

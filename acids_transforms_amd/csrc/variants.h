// variants.h -- how a launcher chooses between kernels that compute the SAME result.
//
// Product builds decide from the call's arguments alone, plus the explicit variant table below, which the C ABI exposes
// as at_set_variant / at_get_variant (include/acids_hip.h): the parity tests use it to run the generic forms of kernels
// whose headline shapes have a specialised form, and compare the two.  One relaxed atomic load on the launch path.
//
// The environment switches of the kernel A/B scripts (tools/ab*.sh) exist only in -DAT_DEV_SWITCHES builds
// (make EXTRA=-DAT_DEV_SWITCHES): dev_env() is getenv() there and a constant nullptr in the product library, so the
// compiler drops the branches behind it.
#pragma once
#include <stdlib.h>

namespace at_hip {

enum {
  kVarEpilogue = 0,         // 0: fixed-length epilogue / projection where the bank has the headline shape; 1: always generic
  kVarFrameKernels = 1,     // 1: frame-at-a-time forward at n_fft 512 / 2048 / 4096 instead of the sliding-window kernels
  kVarSmallProjection = 2,  // 0: matrix-core form of the K <= 128 projection (the DCT behind MFCC); 1: row kernel
  kVarScanLayout = 3,       // 0: one block per clip for rows that are not whole 64-byte segments; 1: flattened columns
  kVarPghiKernel = 4,       // 0: cooperative heap kernels (+ rank fast path, realtime); 1: winner-bit offline kernel;
                            // 2: single-lane kernels; 3: cooperative kernels, realtime on the heap only; 4: realtime with the
                            // rank fast path but without the wavefront-parallel scan path in front of it
  kVarIstftRuns = 5,        // 1: the n_fft-1024 inverse always as one long run per wave (no workgroup tiles with LDS hand-over)
  // Plan variants: same kernel, a different cut of the clips.  0 leaves the plan to the launcher (device-dependent).
  kVarRunLength = 6,        // v > 0: runs of v units (clamped to [8, units]) for the streaming STFT / ISTFT launchers: the
                            // n_fft-1024 forward (fused forms included), the 512 / 2048 / 4096 sliding-window forwards,
                            // the long-run n_fft-1024 inverse and the fused 512 / 2048 / 4096 inverses (istft512_ola_kernel
                            // in frame pairs, istft2048_ola_kernel / istft4096_ola_kernel in output hops)
  kVarIstftTile = 7,        // v > 0: the n_fft-1024 inverse on workgroup tiles whatever the batch, v (>= 6) frames per wave
  kVarRowRun = 8,           // v > 0: the row cut of the projection launchers, clamped to [1, total] (forced_row_run):
                            // v rows per wave (banded, fixed, small row form), v rounded up to 32 rows (small MFMA form,
                            // whole 32-row tile pairs), v frame pairs (n_fft-512 features), v frames (n_fft-2048 features),
                            // v 32-row tiles per workgroup (dense GEMM), v 128-row tiles per workgroup (bf16)
  kVarFrameWalkers = 9,     // v > 0: min(v, frames) workgroups walk the frames of the fallback STFT kernels (stft_generic.hip,
                            // stft_mixed.hip: frames blockIdx.x + k gridDim.x) and min(v, blocks) blocks stride the
                            // overlap-add gather (forced_walkers)
  kVarCount = 10,
  kVarFirstPlan = kVarRunLength
};

int variant(int which);     // capi.hip

// The unit count a projection launcher must cut per wave (or workgroup) in place of its own plan: AT_VARIANT_ROW_RUN
// clamped to [1, total], or 0 = keep the plan.  Runs of any length already occur in last waves, so 1 is legal everywhere.
inline long long forced_row_run(long long total) {
  const long long v = variant(kVarRowRun);
  if (v <= 0) return 0;
  return v < total ? v : (total > 0 ? total : 1);
}

// Workgroups of a launch whose kernel strides over `units` (frames, 256-thread blocks of outputs) with its grid:
// AT_VARIANT_FRAME_WALKERS clamped to [1, units] in place of the launcher's `plan`.  Any count >= 1 is legal.
inline unsigned forced_walkers(long long units, long long plan) {
  const long long v = variant(kVarFrameWalkers);
  if (v <= 0) return (unsigned)plan;
  return (unsigned)(v < units ? v : units);
}

#ifdef AT_DEV_SWITCHES
inline const char* dev_env(const char* name) { return getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; }
#endif

}  // namespace at_hip

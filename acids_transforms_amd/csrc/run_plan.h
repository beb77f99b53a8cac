// run_plan.h -- how the streaming STFT kernels cut clips into per-wave runs (shared by the size-specific launchers).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/acids_hip.h"
#include "variants.h"

namespace at_hip {

inline int num_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

// wave slots the chip offers one kernel variant (occupancy x CUs), cached per variant by the caller
template <typename K>
inline long long resident_waves(K kernel, int block_threads, size_t dyn_lds) {
  struct Entry { const void* k; size_t lds; long long waves; };
  static thread_local Entry cache[16];
  static thread_local int n_cached = 0;
  for (int i = 0; i < n_cached; ++i)
    if (cache[i].k == (const void*)kernel && cache[i].lds == dyn_lds) return cache[i].waves;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block_threads, dyn_lds) != hipSuccess || nb <= 0) nb = 2;
  const long long waves = (long long)nb * (block_threads / 64) * num_cus();
  if (n_cached < 16) cache[n_cached++] = {(const void*)kernel, dyn_lds, waves};
  return waves;
}

// Split each of the B clips' `units` (frames / hop slots) into equal runs, one wave per run.  Every wave of a
// streaming kernel takes the same time, so the launch costs ceil(waves / slots) rounds of (run length +
// per-run overhead): 4096 waves on 3072 slots is two rounds, the second one a third full -- pick the run
// count that minimises rounds x run length instead of aiming at a fixed wave count.
inline long long plan_units_per_run(long long B, long long units, long long slots, long long min_units,
                                    long long overhead_units) {
  long long best_upr = units, best_cost = -1;
  long long max_runs = units / (min_units > 0 ? min_units : 1);
  if (max_runs < 1) max_runs = 1;
  for (long long runs = 1; runs <= max_runs; ++runs) {
    const long long upr = (units + runs - 1) / runs;
    const long long waves = B * ((units + upr - 1) / upr);
    const long long cost = ((waves + slots - 1) / slots) * (upr + overhead_units);
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best_upr = upr;
    }
  }
  return best_upr;
}

// The plain forwards (no epilogue) with work for every slot at least twice over take SHORT runs instead of the planner's
// one long run per wave: a workgroup's runs are then one tile of the output stream and the hardware dispatches the tiles
// in address order -- the compact, advancing write front of profiles/r04_launch_shape.md (n_fft 1024: 0.730 -> 0.699 ms).
// Only there: at n_fft 2048 / 4096 (8-frame runs) the same cut is 5-10 % SLOWER (a run start re-reads 3/4 of a longer
// window), at 512 it is lost in the noise.
inline long long short_runs_if_full(long long B, long long units, long long slots, long long planned, long long target) {
  if (planned > target && B * ((units + target - 1) / target) >= 2 * slots) return target;
  return planned;
}

// The run length a launcher must use in place of its own plan: AT_VARIANT_RUN_LENGTH clamped to [8, units] (what the
// kernels assume, as the dev switches do), or 0 = keep the plan.  The tests force every run cut with it, whatever the device.
inline long long forced_units_per_run(long long units) {
  const long long v = variant(kVarRunLength);
  if (v <= 0) return 0;
  if (v > units) return units;
  return v < 8 ? (units < 8 ? units : 8) : v;
}

// The frame-per-wave kernels (a block's `waves` waves interleave over its units: frames, pairs or groups of frames):
// units per block in whole rounds of the block's waves, at least one round, at most 2048 workgroups (256 CUs x 8).
inline long long units_per_block(long long n, int waves) {
  const long long max_blocks = 256LL * 8;
  long long upb = (n + max_blocks - 1) / max_blocks;
  upb = ((upb + waves - 1) / waves) * waves;
  return upb < waves ? waves : upb;
}

// What the frame-per-wave kernels of n_fft 2048 and 4096 take, forward and irfft*_frames (n_fft 512 counts pairs: P5).
struct PFrames {
  const float* x;        // forward: audio, clip b at x + b*clip_stride
  const float* window;   // n_fft samples (analysis or synthesis)
  const float2* tw;      // fft512 twiddle table (capi.hip)
  const float2* tw_n;    // the size's own table (W2048^k; the n_fft-4096 block of the side table)
  float2* X;             // (frames, n_fft / 2 + 1) complex64: forward output / inverse input
  const float* mag;      // inverse, polar input
  const float* phase;
  float* phase_out;      // forward: optional angle output (frames, n_fft / 2 + 1)
  float* y;              // inverse: (frames, n_fft) windowed time frames
  long long L, clip_stride, T, total_frames, frames_per_block;
  int hop, center;
};

// kernels[second] over p.total_frames frames, units_per_block of them per workgroup of `waves_per_block` waves
inline int launch_frames(void (*const (&kernels)[2])(PFrames), bool second, int waves_per_block, PFrames p,
                         hipStream_t stream) {
  p.frames_per_block = units_per_block(p.total_frames, waves_per_block);
  const long long blocks = (p.total_frames + p.frames_per_block - 1) / p.frames_per_block;
  hipLaunchKernelGGL(kernels[second], dim3((unsigned)blocks), dim3(64 * waves_per_block), 0, stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// What the sliding-window forwards of n_fft 512, 2048 and 4096 take (row_stream.h): a wave walks one run of a clip.
struct PRunFwd {
  const float* x;
  const float* window;
  const float2* tw;      // fft512 twiddle table
  const float2* tw_n;    // the size's own table
  float2* X;
  long long B, L, clip_stride, T, runs_per_clip, units_per_run;     // units: frames; frame pairs at n_fft 512
};

// The plan those three share: runs of at least 8 of the clip's `units`, one unit of overhead per run start, or the
// forced length (tests); one wave per run.
inline int launch_run_fwd(void (*kernel)(PRunFwd), int waves_per_block, long long units, PRunFwd p, hipStream_t stream) {
  const long long slots = resident_waves(kernel, 64 * waves_per_block, 0);
  p.units_per_run = plan_units_per_run(p.B, units, slots, 8, 1);
  if (const long long v = forced_units_per_run(units)) p.units_per_run = v;
  p.runs_per_clip = (units + p.units_per_run - 1) / p.units_per_run;
  const long long waves = p.B * p.runs_per_clip;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((waves + waves_per_block - 1) / waves_per_block)), dim3(64 * waves_per_block), 0,
                     stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

// Run length of the fused overlap-add kernels, one wave per run of a clip's `units` (output hops; frame pairs at n_fft
// 512): about `target_waves` waves in the launch, but runs of at least `min_units` -- long enough that the R - 1 warm-up
// frames stay a small share, short enough to fill the chip -- and never longer than the clip.  The floor is a throughput
// choice: the kernels take runs of any length >= 1 (warm-up, carry and masks are per unit), so AT_VARIANT_RUN_LENGTH
// (tests) replaces the plan with its own clamp to [8, units].
inline long long plan_ola_runs(long long B, long long units, long long target_waves, long long min_units) {
  const long long runs = (B >= target_waves) ? 1 : (target_waves + B - 1) / B;
  long long per = (units + runs - 1) / runs;
  if (per < min_units) per = min_units < units ? min_units : units;
  if (per < 1) per = 1;
  if (const long long v = forced_units_per_run(units)) per = v;
  return per;
}

}  // namespace at_hip

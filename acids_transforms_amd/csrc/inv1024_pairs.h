// inv1024_pairs.h -- which bin of a one-sided 1024-point spectrum each lane and register of the n_fft-1024 inverse
// kernels (stft1024.hip) loads, so that the real-FFT split (fft512.h: irfft_split) finds both members of every mirror
// pair (X[k], X[512 - k]) in ONE lane and computes the pair once.
//
//   load      lane L, register m:  m < 4: bin L + 64 m;   m >= 4: bin (64 - L) + 64 m
//             registers m and 7 - m of a lane are mirror partners in every lane: L + 64 m + (64 - L) + 64 (7 - m) = 512.
//             Lane 0's registers 4..7 are bins 320, 384, 448 and 512 (the Nyquist bin comes through a regular load);
//             bin 256, its own partner, is in no register: one extra element, used by lane 0.
//   split     in place: register m -> Z[its bin], one W1024 twiddle per pair (row m < 4 of the table, W1024^(L + 64 m);
//             the partner's W1024^(512 - k) is its negated conjugate, exactly, in the host's table)
//   rotate    lane 0 alone, whose registers 4..7 hold Z[320], Z[384], Z[448] and an unused "Z[512]", moves registers
//             4..6 up by one and takes Z[256] into register 4: column 0 at its natural index
//   exchange  registers 4..7 travel between lanes L and (64 - L) & 63 (lanes 0 and 32 address themselves): they held
//             column 64 - L at its natural index, so lane L now has Z[L + 64 m] in every register
// After that fft512<true> runs on its usual input, v[m] = Z[lane + 64 m].  (Lane 0 exchanges with itself, so its
// rotation may come on either side of the exchange; before it, the rotation waits for no cross-lane result.)
//
// No HIP in here: tests/test_inv1024_pairs_cpu.py compiles these functions on the host and walks all 64 lanes.
#pragma once
#include <math.h>

namespace at_hip {
namespace inv1024 {

// W1024^k = exp(-2 pi i k / 1024) as the host builds the device's table (capi.hip: at_init), k = 0..511
inline void w1024(int k, float& re, float& im) {
  const double a = -6.283185307179586476925286766559 * (double)k / 1024.0;
  re = (float)cos(a);
  im = (float)sin(a);
}

constexpr int kLanes = 64, kRegs = 8, kPairs = 4;
constexpr int kSelfPairedBin = 256;    // lane 0's extra element
constexpr int kSelfPairedRow = 4;      // its twiddle W1024^256 is row 4, lane 0 of the W1024 rows

// the bin that lane `lane` loads into register `m`: one of two lane-dependent starts plus a step that only depends on m
// (the kernels form the two start addresses once and reach every register through an immediate offset)
constexpr int load_start(int lane, int m) { return m < kPairs ? lane : 64 - lane; }
constexpr int load_step(int m) { return 64 * m; }
constexpr int load_bin(int lane, int m) { return load_start(lane, m) + load_step(m); }
// the register of the same lane that holds the mirror partner of register m
constexpr int partner_reg(int m) { return kRegs - 1 - m; }
// the lane whose registers 4..7 this lane takes in the exchange
constexpr int exchange_lane(int lane) { return (64 - lane) & 63; }
// register m of the pair (m, 7 - m), m < 4, uses W1024^(lane + 64 m): row m of the table at this lane
constexpr int twiddle_bin(int lane, int m) { return lane + 64 * m; }

// the bin whose Z sits in register m of lane `lane` after the split and lane 0's rotation
constexpr int rotated_bin(int lane, int m) {
  return (lane == 0 && m >= kPairs) ? (m == kPairs ? kSelfPairedBin : load_bin(0, m - 1)) : load_bin(lane, m);
}
// ... and after the exchange: what fft512<true> is given
constexpr int final_bin(int lane, int m) { return m < kPairs ? rotated_bin(lane, m) : rotated_bin(exchange_lane(lane), m); }

constexpr bool pairs_and_order_hold() {
  for (int lane = 0; lane < kLanes; ++lane)
    for (int m = 0; m < kRegs; ++m) {
      if (load_bin(lane, m) + load_bin(lane, partner_reg(m)) != 512) return false;
      if (final_bin(lane, m) != lane + 64 * m) return false;
    }
  return true;
}
static_assert(pairs_and_order_hold(), "registers m and 7 - m are mirror partners; fft512<true> gets Z[lane + 64 m]");

}  // namespace inv1024
}  // namespace at_hip

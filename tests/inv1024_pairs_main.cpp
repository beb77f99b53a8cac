// Host program of tests/test_inv1024_pairs_cpu.py: the paired layout of csrc/inv1024_pairs.h without a GPU.
//   inv1024_pairs --layout     one line per (lane, register): lane m load_bin partner_reg exchange_lane rotated_bin final_bin
//                              twiddle_bin
//   inv1024_pairs --table      one line per k = 0..511: k and the bit patterns of Re, Im W1024^k as the host builds them
//   inv1024_pairs --split S    a random one-sided spectrum (seed S) split twice in fp32 with the kernels' operation order:
//                              bin by bin, every bin with its own table entry (the split before the pairing), and pair by pair
//                              through the layout (load, split with rows 0..3 only, lane 0's rotation, exchange).  One line per
//                              k = 0..511: k and the bit patterns of both results (Re, Im each).
// Build without fp contraction: every fma below is spelled out.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "inv1024_pairs.h"

using namespace at_hip::inv1024;

struct C { float x, y; };
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// fft512.h, one function each: add_conj, sub_conj, cmul_conj_v, add_pi, conj_add_mi
static C add_conj(C a, C b) { return {a.x + b.x, a.y - b.y}; }
static C sub_conj(C a, C b) { return {a.x - b.x, a.y + b.y}; }
static C cmul_conj(C a, C w) {
  const float t0 = a.y * w.y, t1 = a.y * w.x;
  return {fmaf(a.x, w.x, t0), fmaf(a.x, -w.y, t1)};
}
static C add_pi(C a, C b) { return {a.x - b.y, a.y + b.x}; }
static C conj_add_mi(C a, C b) { return {a.x + b.y, -a.y + b.x}; }
static C w_of(int k) { C w; w1024(k, w.x, w.y); return w; }

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--layout")) {
    for (int l = 0; l < kLanes; ++l)
      for (int m = 0; m < kRegs; ++m)
        printf("%d %d %d %d %d %d %d %d\n", l, m, load_bin(l, m), partner_reg(m), exchange_lane(l), rotated_bin(l, m),
               final_bin(l, m), twiddle_bin(l, m));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "--table")) {
    for (int k = 0; k < 512; ++k) {
      const C w = w_of(k);
      printf("%d %u %u\n", k, bits(w.x), bits(w.y));
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "--split")) {
    srand((unsigned)atoi(argv[2]));
    C X[513];
    for (int k = 0; k <= 512; ++k) {
      X[k].x = (float)rand() / (float)RAND_MAX - 0.5f;
      X[k].y = (float)rand() / (float)RAND_MAX - 0.5f;
    }
    // bin by bin: Z[k] = e + i d, e = X[k] + conj X[512-k], d = (X[k] - conj X[512-k]) conj(W^k); Im X[0] = Im X[512] = 0
    C zref[512];
    for (int k = 0; k < 512; ++k) {
      C v = X[k], p = X[512 - k];
      if (k == 0) { v.y = 0.0f; p.y = 0.0f; }
      zref[k] = add_pi(add_conj(v, p), cmul_conj(sub_conj(v, p), w_of(k)));
    }
    // pair by pair through the layout
    static C v[kLanes][kRegs], z[kLanes][kRegs];
    for (int l = 0; l < kLanes; ++l) {
      for (int m = 0; m < kRegs; ++m) v[l][m] = X[load_bin(l, m)];
      if (l == 0) v[0][0].y = v[0][7].y = 0.0f;
      for (int m = 0; m < kPairs; ++m) {
        const int n = partner_reg(m);
        const C e = add_conj(v[l][m], v[l][n]);
        const C d = cmul_conj(sub_conj(v[l][m], v[l][n]), w_of(twiddle_bin(l, m)));
        v[l][m] = add_pi(e, d);
        v[l][n] = conj_add_mi(e, d);
      }
    }
    {
      const C x = X[kSelfPairedBin];
      const C mid = add_pi(add_conj(x, x), cmul_conj(sub_conj(x, x), w_of(kSelfPairedBin)));
      v[0][7] = v[0][6];
      v[0][6] = v[0][5];
      v[0][5] = v[0][4];
      v[0][4] = mid;
    }
    for (int l = 0; l < kLanes; ++l)
      for (int m = 0; m < kRegs; ++m) z[l][m] = m < kPairs ? v[l][m] : v[exchange_lane(l)][m];
    for (int k = 0; k < 512; ++k) {
      const C a = zref[k], b = z[k & 63][k >> 6];
      printf("%d %u %u %u %u\n", k, bits(a.x), bits(a.y), bits(b.x), bits(b.y));
    }
    return 0;
  }
  return 2;
}

// pghi_heap.h -- what the two PGHI modes share (pghi_offline.hip, pghi_rt.hip): phase-gradient heap integration on gfx950.
//
// Replaces the reference's pure-Python heap loops:
//   DGT.modgabphasegrad / pghi / perform_hgi              transforms/dgt.py:156-236   (K13, K14)
//   RealtimeDGT.modgabphasegrad / pghi / perform_hgi      transforms/dgt.py:338-466
//   utils/heapq.py:9-59 (binary min-heap on keys only, strict '<', right child on ties)
//
// The integration order is part of the contract: it is
// defined by exact fp32 compares of magnitudes and by the heap's tie-breaking,
// so the heap here is the same array-embedded binary heap with the same
// sift rules.  One wavefront owns one clip (offline) or one stream (realtime):
// the flood is inherently serial per clip, the batch supplies the parallelism.
// Wave-wide work (gradients, maxima / reseeds, thresholding) is lane-parallel.
//
// Both PGHI sources are compiled with -ffp-contract=off: every fp32 expression keeps
// the reference's rounding sequence (no FMA contraction), and the phases of the
// different paths are compared bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "fastmath.h"
#include <stdint.h>
#include <stdlib.h>

#include "../../include/acids_hip.h"
#include "run_plan.h"
#include "variants.h"

namespace at_hip {

struct HeapItem {
  float key;  // -magnitude
  int idx;    // payload, never compared.  Offline: frame * F + bin; realtime: bin (row f-1) or F + bin (row f)
};

// ---- heap primitives, single lane (utils/heapq.py) --------------------------
__device__ __forceinline__ void h_siftdown(HeapItem* h, int startpos, int pos) {
  HeapItem newitem = h[pos];
  while (pos > startpos) {
    const int parentpos = (pos - 1) >> 1;
    const HeapItem parent = h[parentpos];
    if (newitem.key < parent.key) {
      h[pos] = parent;
      pos = parentpos;
      continue;
    }
    break;
  }
  h[pos] = newitem;
}

__device__ __forceinline__ void h_siftup(HeapItem* h, int endpos, int pos) {
  const int startpos = pos;
  const HeapItem newitem = h[pos];
  int childpos = 2 * pos + 1;
  while (childpos < endpos) {
    const int rightpos = childpos + 1;
    if (rightpos < endpos && !(h[childpos].key < h[rightpos].key)) childpos = rightpos;
    h[pos] = h[childpos];
    pos = childpos;
    childpos = 2 * pos + 1;
  }
  h[pos] = newitem;
  h_siftdown(h, startpos, pos);
}

__device__ __forceinline__ void h_push(HeapItem* h, int& n, float key, int idx) {
  h[n].key = key;
  h[n].idx = idx;
  ++n;
  h_siftdown(h, 0, n - 1);
}

__device__ __forceinline__ HeapItem h_pop(HeapItem* h, int& n) {
  const HeapItem last = h[n - 1];
  --n;
  if (n > 0) {
    const HeapItem ret = h[0];
    h[0] = last;
    h_siftup(h, n, 0);
    return ret;
  }
  return last;
}

// ---- wave-wide (value, first index) arg-max --------------------------------
__device__ __forceinline__ void wave_argmax(float& v, long long& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const long long oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// ---------------------------------------------------------------------------
// The wave-cooperative heap (pghi_hgi_offline_coop_kernel, pghi_hgi_rt_coop_kernel).  Same binary heap, same sift rules,
// same pop order as the single-lane version above -- but every heap operation is done
// by the whole wavefront so that its ~log2(n) *dependent* memory accesses become
// a few wide ones:
//   pop  : the bubble-up path from the hole is resolved five levels per round:
//          63 lanes gather the depth-6 subtree under the hole (node i of the
//          subtree on lane i), every inner lane picks its smaller child (right
//          child on ties, utils/heapq.py:33), the path is read off with five
//          v_readlane steps and all moved entries are written by one store;
//   push / final sift-down: every ancestor of the insertion point is known from
//          its index alone, so lane L loads ancestor L, one ballot finds how far
//          the item rises (strict '<', heapq.py:16) and one store shifts the chain;
//   neighbours: lanes 0-3 handle next-frame / prev-frame / next-bin / prev-bin.
// Heap words are read with agent-scope loads (L2-served): entries written by one
// lane are re-read by other lanes of the same wave a few instructions later.
// ---------------------------------------------------------------------------
typedef unsigned long long u64;

__device__ __forceinline__ u64 pack_item(float key, int idx) {
  return ((u64)__float_as_uint(key) << 32) | (unsigned)idx;
}
__device__ __forceinline__ float item_key(u64 e) { return __uint_as_float((unsigned)(e >> 32)); }
__device__ __forceinline__ int item_idx(u64 e) { return (int)(unsigned)e; }

// Heap words and cell state in global memory are written and re-read by lanes of ONE wave only.  A CU's vector L1
// is write-through and coherent for the waves of that CU, so workgroup scope is all the visibility this needs
// (ACIDS_PGHI_SCOPE=__HIP_MEMORY_SCOPE_AGENT at compile time restores the L2-served sc1 accesses: those write
// through to memory and DROP the line from L2 -- MI355X_MICROARCH.md, "stores of each flavour" -- so every later read
// of a heap entry paid a trip beyond L2).  The relaxed atomics only pin the compiler's ordering.
#ifndef ACIDS_PGHI_SCOPE
#define ACIDS_PGHI_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
#endif
__device__ __forceinline__ u64 gload(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, ACIDS_PGHI_SCOPE);
}
__device__ __forceinline__ void gstore(u64* p, u64 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, ACIDS_PGHI_SCOPE);
}

// The heap array: positions [0, cap) live in this wave's LDS (the top levels, where every pop starts),
// the rest in the clip's global workspace.  Same array, same indices -- only the storage differs.
// cap = 2^k - 1 is chosen at launch from the batch size: 4095 entries (32 KB) while <= 4 clips share a
// CU, fewer when more clips have to be resident at once.
// SPILLS = false: the whole heap is in LDS (realtime kernel) and the global paths compile away.
template <bool SPILLS>
struct HeapT {
  u64* top;   // LDS, cap entries
  u64* rest;  // global, indexed by absolute position
  int cap;
  __device__ __forceinline__ u64 load(long long pos) const {
    if constexpr (!SPILLS) return top[pos];
    return pos < cap ? top[pos] : gload(rest + pos);
  }
  __device__ __forceinline__ void store(long long pos, u64 v) const {
    if constexpr (!SPILLS) {
      top[pos] = v;
      return;
    }
    if (pos < cap) top[pos] = v;
    else gstore(rest + pos, v);
  }
  // entry `pos` for the lanes that `want` it, `dflt` for the others.  The LDS read is unconditional (slot 0 for
  // lanes that do not want it or whose entry is global): one divergent region -- the global load -- instead of
  // a nest of three, and none at all while the whole subtree is in LDS.
  __device__ __forceinline__ u64 load_if(int pos, bool want, u64 dflt) const {
    if constexpr (!SPILLS) {
      const u64 v = top[want ? pos : 0];
      return want ? v : dflt;
    }
    const bool in_lds = pos < cap;
    u64 v = top[(want && in_lds) ? pos : 0];
    if (want && !in_lds) {
      v = gload(rest + pos);
      // Wait for it here, inside the branch.  Left to the compiler, the wait lands after the join as vmcnt(0),
      // and rounds that touched LDS only would then sit out the neighbourhood loads the pop has in flight
      // (memory returns in order): an HBM round trip exposed on every pop.
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt / lgkmcnt untouched
    }
    return want ? v : dflt;
  }
};
typedef HeapT<true> Heap;
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const unsigned lo = __shfl((unsigned)v, src, 64);
  const unsigned hi = __shfl((unsigned)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float fload(const float* p) {   // a cell another lane of this wave may have just written
  return __hip_atomic_load(p, __ATOMIC_RELAXED, ACIDS_PGHI_SCOPE);
}

// place `item` at `pos` and let it rise (utils/heapq.py:9-21 with startpos = 0)
template <typename HEAP>
__device__ __forceinline__ void coop_siftdown(const HEAP& H, int pos, u64 item, int lane) {
  const unsigned q = (unsigned)pos + 1u;
  const int depth = 31 - __clz(q);                // number of ancestors (< 31)
  const int sh = lane < 31 ? lane : 30;           // lanes >= depth are idle; keep their shifts defined
  const int my_dst = (int)(q >> sh) - 1;          // lane L: position of ancestor L-1 (L = 0: pos itself)
  const int my_anc = (int)(q >> (sh + 1)) - 1;    // lane L: position of ancestor L
  const u64 anc = H.load_if(my_anc, lane < depth, 0);
  const bool rises = (lane < depth) && (item_key(item) < item_key(anc));
  const u64 mask = __ballot(rises);
  const int m = (mask == ~0ull) ? 64 : __builtin_ctzll(~mask);  // item passes ancestors 0 .. m-1
  // lanes 0 .. m-1 move their ancestor one step down, lane m drops the item: one store site
  if (lane <= m) H.store(my_dst, lane == m ? item : anc);
}

// sibling's value through DPP (lane ^ 1): pure VALU, no LDS crossbar
__device__ __forceinline__ float dpp_xor1(float v) {
  return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ int dpp_xor1_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }

__device__ __forceinline__ u64 readlane64(u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

// utils/heapq.py:51-59 (+ :24-42): the bubble-up part of heappop after `last` was taken off the end
// (n = remaining size >= 1).  Returns the leaf position where `last` has to be placed.
// lanes {L, L >> 1, L >> 2, ...} >= 2: the nodes that must all be chosen children for local node L to bubble up
__device__ __forceinline__ u64 chain_mask(int lane) {
  u64 m = 0;
  for (int a = lane; a >= 2; a >>= 1) m |= 1ull << a;
  return m;
}

// `top63`: positions 0..62 as lane L - 1 holds them (lane 0: anything), read by the caller before the pop began --
// the first round always gathers from there, so its load is off the critical path.
template <typename HEAP>
__device__ __forceinline__ int coop_bubble(const HEAP& H, int n, int lane, u64 anc_mask, u64& leaf_old, u64 top63) {
  int pos = 0;  // the hole
  const int lvl = 31 - __clz((unsigned)lane | 1u);
  const int off = lane - (1 << lvl);
  const u64 kInf = (u64)0x7f800000u << 32;
  // Rounds are aligned to the *bottom* of the heap: the first one descends only ((D - 1) mod 5) + 1 levels
  // (D = the last level), so that the last round covers levels D-4 .. D.  With the top 12 levels in LDS a heap
  // of up to 2^17 entries then pays one global round per pop, where top-aligned rounds (1-5, 6-10, 11-15, 16)
  // pay two as soon as D = 16 -- a third of all pops on dense spectra.  Same number of rounds either way.
  const int last_level = 31 - __clz((unsigned)n | 1u);
  int limit = last_level >= 1 ? ((last_level - 1) % 5) + 1 : 5;
  bool first = true;
#ifndef AT_PGHI_NO_ROOT_STEP
  if (limit == 1) {
    // A first round of ONE level (last level 1, 6, 11 or 16 -- a third of all pops on dense spectra sit at 16) is the
    // root choosing between its two children: both are in `top63` (positions 1 and 2 on lanes 2 and 3), so the round is
    // two readlanes, one compare (heapq.py:33: the right child unless left < right; a missing child reads +inf) and one
    // store, all on the scalar side, instead of the 64-lane machinery below and its LDS round trip.
    const u64 v1 = readlane64(top63, 2);
    const u64 v2 = (2 < n) ? readlane64(top63, 3) : kInf;
    const bool left = item_key(v1) < item_key(v2);
    const u64 vc = left ? v1 : v2;
    pos = left ? 1 : 2;
    if (lane == 0) H.store(0, vc);
    if (2 * pos + 1 >= n) {
      leaf_old = vc;
      return pos;
    }
    limit = 5;
    first = false;
  }
#endif
  for (;;) {
    // subtree under the hole: local node `lane` (1..63) <-> global index g
    const int g = ((pos + 1) << lvl) - 1 + off;           // < 2^25: heap positions are < T F < 2^31 >> 5
    const bool valid = (lane >= 1) && (lvl <= limit) && (g < n);
    const u64 val = first ? (valid ? top63 : kInf) : H.load_if(g, valid, kInf);
    first = false;
    const float key = item_key(val);
    // "am I the child my parent bubbles up?"  children 2i (left, even lane) and 2i+1 (right, odd lane) are
    // DPP neighbours.  heapq.py:33: take the right child iff it exists and not (left < right); a missing child
    // reads as +inf (real keys are -magnitude, finite), so one compare `left < right` decides for both lanes.
    // As lane masks (scalar unit): left children are chosen where key < sibling, right ones where not
    // (sibling < key).
    const float sib = dpp_xor1(key);
    const u64 kOdd = 0xAAAAAAAAAAAAAAAAull;
    const u64 m_lt = __ballot(key < sib), m_gt = __ballot(sib < key);
    const u64 W = __ballot(valid) & ((~kOdd & m_lt) | (kOdd & ~m_gt)) & ~3ull;
    // The chain of bubbled-up nodes below the subtree root: node L belongs to it iff L and every ancestor of
    // L down to level 1 is its parent's chosen child, i.e. iff W covers the lane's ancestor mask; below a
    // leaf no bit is set, so the chain simply ends there.
    const bool on_chain = (lane >= 2) && ((W & anc_mask) == anc_mask);
    const u64 chain = __ballot(on_chain);
    const int steps = __builtin_popcountll(chain);
    const int cur = steps ? 63 - __builtin_clzll(chain) : 1;          // the final hole of this round
    // every bubbled-up entry moves into its parent's slot (the hole, or the chain node above it)
    if (on_chain) H.store((g - 1) >> 1, val);
    const int gcur = __builtin_amdgcn_readlane(g, cur);
    pos = gcur;
    if (steps < limit || 2 * gcur + 1 >= n) {
      leaf_old = readlane64(val, cur);   // what the final hole held: now the value of its parent
      break;
    }
    limit = 5;
  }
  return pos;
}

// heappop, part 2 (heapq.py:56-59): `last` was taken off the end and hn >= 1 entries remain.  Bubble the smaller children
// up from the root, drop `last` into the leaf, let it rise while it is smaller than its parent (heapq.py:39-42).  The
// parent of the leaf now holds the entry that just left the leaf, which is still in registers: in the common case
// (`last` does not rise at all) no ancestor has to be read back.
// PROF (the offline profiling build): returns the clock between the bubble and the sift; otherwise 0 and no clock read.
template <bool PROF = false, typename HEAP>
__device__ __forceinline__ long long coop_pop_repair(const HEAP& H, int hn, u64 last, u64 top63, int lane, u64 anc_mask) {
  u64 leaf_old = 0;
  const int leaf = coop_bubble(H, hn, lane, anc_mask, leaf_old, top63);
  const long long tick = PROF ? (long long)__builtin_amdgcn_s_memtime() : 0;
  if (leaf == 0 || !(item_key(last) < item_key(leaf_old))) {
    if (lane == 0) H.store(leaf, last);
  } else {
    coop_siftdown(H, leaf, last, lane);
  }
  return tick;
}

// ---- host side -----------------------------------------------------------------------------------------------
static inline unsigned grid1d(long long n) {
  long long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// One wave per unit (clip, stream), `wpb` independent waves per workgroup, `per_wave_lds` bytes of dynamic LDS each:
// halve wpb until the workgroup fits the CU's 160 KB less `lds_margin`, raise the kernel's dynamic-LDS limit where the
// workgroup needs more than the default 48 KB, launch ceil(units / wpb) workgroups.
template <typename P>
static inline int launch_waves(void (*kernel)(P), long long units, int wpb, size_t per_wave_lds, size_t lds_margin,
                               hipStream_t stream, const P& params) {
  while (wpb > 1 && per_wave_lds * wpb > 160 * 1024 - lds_margin) wpb >>= 1;
  const size_t block_lds = per_wave_lds * wpb;
  if (block_lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)block_lds) != hipSuccess) {
    (void)hipGetLastError();
    return AT_ELAUNCH;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)((units + wpb - 1) / wpb)), dim3(64 * wpb), block_lds, stream, params);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

}  // namespace at_hip

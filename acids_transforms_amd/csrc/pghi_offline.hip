// pghi_offline.hip -- offline PGHI on gfx950: DGT.modgabphasegrad / pghi / perform_hgi (transforms/dgt.py:156-236, K13 and
// K14), one wavefront per clip.  The heap, its cooperative operations and the contract they keep are in pghi_heap.h.
// Compiled with -ffp-contract=off, like pghi_rt.hip.
#include "pghi_heap.h"

namespace at_hip {

// ---------------------------------------------------------------------------
// K13 offline: s = clamp(mag, eps); log; replicate-padded central differences
// ---------------------------------------------------------------------------
struct GradParams {
  const float* mag;  // (B, T, F)
  float* spec;       // (B, T, F) clamped work copy (may be null)
  float* tgradw;
  float* fgradw;
  long long B;
  int T, F, n_fft, hop;
  float gamma, eps;
};

__global__ __launch_bounds__(256) void pghi_grad_offline_kernel(GradParams p) {
  const float fmul = p.gamma / (float)((long long)p.hop * (long long)p.n_fft);
  const float fstep = ((float)(2.0 * 3.14159265358979323846) * (float)p.hop) / (float)p.n_fft;
  const float pi_f = (float)3.14159265358979323846;
  const long long per = (long long)p.T * p.F;
  const long long total = p.B * per;
  // (clip, frame, bin) of the flat index are carried along the grid stride: two 64-bit divisions per thread instead of
  // two per element (1.63 -> 1.43 ms per 1024 clips, tools/grad_probe.py; the rest is four logf per bin)
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long b = i0 / per;
  const long long r0 = i0 - b * per;
  int t = (int)(r0 / p.F), k = (int)(r0 - (long long)t * p.F);
  const long long sb = stride / per;
  const long long sr = stride - sb * per;
  const int st = (int)(sr / p.F), sk = (int)(sr - (long long)st * p.F);
  for (long long i = i0; i < total; i += stride, b += sb, t += st, k += sk) {
    if (k >= p.F) {
      k -= p.F;
      ++t;
    }
    if (t >= p.T) {
      t -= p.T;
      ++b;
    }
    const long long r = (long long)t * p.F + k;
    const float* m = p.mag + b * per;
    const int tu = t + 1 < p.T ? t + 1 : p.T - 1, td = t > 0 ? t - 1 : 0;
    const int kr = k + 1 < p.F ? k + 1 : p.F - 1, kl = k > 0 ? k - 1 : 0;
    const float c = fmaxf(m[r], p.eps);
    const float right = logf(fmaxf(m[(long long)t * p.F + kr], p.eps));
    const float left = logf(fmaxf(m[(long long)t * p.F + kl], p.eps));
    const float up = logf(fmaxf(m[(long long)tu * p.F + k], p.eps));
    const float dn = logf(fmaxf(m[(long long)td * p.F + k], p.eps));
    const float dxdw = (right - left) / 2.0f;
    const float dxdt = (up - dn) / 2.0f;
    p.fgradw[i] = dxdw / fmul + fstep * (float)k;
    p.tgradw[i] = (-fmul) * dxdt + pi_f;
    if (p.spec) p.spec[i] = c;
  }
}

// ---------------------------------------------------------------------------
// K14 offline: one wave per clip
// ---------------------------------------------------------------------------
struct HgiParams {
  float* spec;          // (B, T, F) clamped magnitudes, consumed (visited cells <- abstol)
  const float* tgradw;  // (B, T, F)
  const float* fgradw;
  float* phase;         // (B, T, F) output
  HeapItem* heap;       // (B, T*F + 2)
  long long B;
  int T, F;
  float abstol, tol;
  long long* npops;     // optional (B) number of pops per clip
  int heap_lds_cap;     // heap entries kept in LDS per clip (2^k - 1)
  int seg_cap;          // cooperative kernel: segment maxima kept in LDS per clip (reseeding), behind the heap's top
  int prof;             // dev only (ACIDS_PGHI_PROF=1): cycle counters go to `order` instead of the pop order
  int* order;           // optional (B, T*F) pop order (row*F+col), for the parity tests
};

// The reference rewrites every cell below max*tol to abstol up front
// (dgt.py:177-178); here that threshold is applied when a cell is read.
__device__ __forceinline__ bool live(float v, float abstol, float thr) { return v > abstol && !(v < thr); }

// global (value, first row-major index) maximum over the live cells of one clip.  Eight independent loads per trip:
// a plain one-load loop pays a full memory round trip per 64 cells (2.5 ms per scan of a 4-second clip).
__device__ __forceinline__ void clip_argmax(const float* spec, long long n, float abstol, float thr, bool use_thr,
                                            int lane, float& best, long long& besti) {
  float v = -1.0f;
  long long vi = n;
  for (long long base = 0; base < n; base += 512) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = base + lane + 64 * u;
      x[u] = spec[i < n ? i : n - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = base + lane + 64 * u;
      float sv = x[u];
      if (use_thr && sv < thr) sv = abstol;
      if (i < n && sv > v) {
        v = sv;
        vi = i;
      }
    }
  }
  wave_argmax(v, vi);
  best = v;
  besti = vi;
}

// ---- reseeding without rescanning the clip -------------------------------------------------------------------
// dgt.py:216-219 takes the global maximum of what is left every time the heap runs empty; a decaying sound does that
// hundreds of times per clip (301 seeds in one second of decaying noise), and a full scan of a
// 4-second clip is 354 k cells.  The clip is cut into S <= seg_cap segments of SL cells (row-major order) with an
// UPPER BOUND of each segment's live maximum in LDS: exact at the start, stale-high afterwards (the flood only
// lowers cells).  A reseed takes the first segment holding the largest bound, rescans that one segment, and is done
// if the bound was exact -- every earlier segment has a smaller bound, every later one at most the same -- otherwise
// it repairs the bound and repeats.  The result is the full scan's (value, first row-major index), cell for cell.
struct SegMax {
  float* m;        // LDS, S entries
  int S;
  long long SL;    // cells per segment (multiple of 512)
};

// maximum of a non-negative value over the wave (DPP row reduction + row broadcasts), valid on every lane
__device__ __forceinline__ float wave_max_nonneg(float v) {
  int x = (int)__float_as_uint(v);
  auto mx = [](int a, int b) { return (int)__float_as_uint(fmaxf(__uint_as_float((unsigned)a), __uint_as_float((unsigned)b))); };
  x = mx(x, __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true));   // row_shr:1
  x = mx(x, __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true));   // row_shr:2
  x = mx(x, __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true));   // row_shr:4
  x = mx(x, __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true));   // row_shr:8  -> lane 15 of each row
  x = mx(x, __builtin_amdgcn_update_dpp(x, x, 0x142, 0xA, 0xF, false));  // row_bcast:15 into rows 1, 3
  x = mx(x, __builtin_amdgcn_update_dpp(x, x, 0x143, 0xC, 0xF, false));  // row_bcast:31 into rows 2, 3 -> lane 63
  return __uint_as_float((unsigned)__builtin_amdgcn_readlane(x, 63));
}

// one segment: (value, first index) maximum under the threshold rule (use_thr) -- at most SL / 64 cells per lane
__device__ __forceinline__ void seg_scan(const float* spec, long long lo, long long hi, float abstol, float thr, bool use_thr,
                                         int lane, float& v, long long& vi) {
  for (long long base = lo; base < hi; base += 512) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = base + lane + 64 * u;
      x[u] = spec[i < hi ? i : hi - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = base + lane + 64 * u;
      float sv = x[u];
      if (use_thr && sv < thr) sv = abstol;
      if (i < hi && sv > v) {
        v = sv;
        vi = i;
      }
    }
  }
}

// exact bounds for every segment (+ the clip's global maximum): the first scan (use_thr = false), and the repair of
// last resort when a reseed keeps hitting stale bounds
__device__ __forceinline__ void seg_rebuild(const float* spec, long long n, const SegMax& G, float abstol, float thr,
                                            bool use_thr, int lane, float& best, long long& besti) {
  float bv = -1.0f;
  long long bi = n;
  for (int sg = 0; sg < G.S; ++sg) {
    const long long lo = sg * G.SL, hi = (lo + G.SL < n) ? lo + G.SL : n;
    float v = -1.0f;
    long long vi = n;
    seg_scan(spec, lo, hi, abstol, thr, use_thr, lane, v, vi);
    const float sm = wave_max_nonneg(fmaxf(v, 0.0f));
    if (lane == 0) G.m[sg] = sm;
    if (v > bv) {      // per lane: cells are visited in increasing index order, so `>` keeps the first index
      bv = v;
      bi = vi;
    }
  }
  wave_argmax(bv, bi);
  best = bv;
  besti = bi;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

__device__ __forceinline__ void seg_reseed(const float* spec, long long n, const SegMax& G, float abstol, float thr,
                                           int lane, float& max_val, long long& max_pos) {
  for (int tries = 0;; ++tries) {
    if (tries == 48) {      // many stale bounds in a row (e.g. the one reseed at the end of a dense clip): rebuild them all
      seg_rebuild(spec, n, G, abstol, thr, true, lane, max_val, max_pos);
      return;
    }
    float bv = -1.0f;
    long long bs = G.S;
    for (int sg = lane; sg < G.S; sg += 64) {
      const float x = G.m[sg];
      if (x > bv) {
        bv = x;
        bs = sg;
      }
    }
    wave_argmax(bv, bs);
    if (!(bv > abstol)) {   // nothing live anywhere: the caller's loop ends (any in-range position will do)
      max_val = abstol;
      max_pos = 0;
      return;
    }
    const long long lo = bs * G.SL, hi = (lo + G.SL < n) ? lo + G.SL : n;
    float tv = -1.0f;
    long long ti = n;
    seg_scan(spec, lo, hi, abstol, thr, true, lane, tv, ti);
    wave_argmax(tv, ti);
    if (tv == bv) {
      max_val = tv;
      max_pos = ti;
      return;
    }
    if (lane == 0) G.m[bs] = tv;   // stale-high bound repaired; try again
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
}

__global__ __launch_bounds__(64) void pghi_hgi_offline_kernel(HgiParams p) {
  const long long b = blockIdx.x;
  if (b >= p.B) return;
  const int lane = threadIdx.x;
  const int T = p.T, F = p.F;
  const long long n = (long long)T * F;
  float* spec = p.spec + b * n;
  const float* tg = p.tgradw + b * n;
  const float* fg = p.fgradw + b * n;
  float* phase = p.phase + b * n;
  HeapItem* heap = p.heap + b * (n + 2);
  int* order = p.order ? p.order + b * n : nullptr;
  const float abstol = p.abstol;

  for (long long i = lane; i < n; i += 64) phase[i] = 0.0f;  // dgt.py:170

  float max_val;
  long long max_pos;
  clip_argmax(spec, n, abstol, 0.f, false, lane, max_val, max_pos);  // :173-174
  const float thr = max_val * p.tol;                                   // :177-178
  long long npops = 0;
  int hn = 0;
  if (lane == 0) {
    heap[0].key = -max_val;  // :175
    heap[0].idx = (int)max_pos;
    spec[max_pos] = abstol;  // :176
  }
  hn = 1;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  while (max_val > abstol) {  // :179
    if (lane == 0) {
      while (hn > 0) {  // :180
        const HeapItem it = h_pop(heap, hn);
        if (order) order[npops] = it.idx;
        ++npops;
        const int c = it.idx;
        const int col = c / F;      // frame
        const int row = c - col * F;  // bin
        const float pc = phase[c];
        if (col < T - 1) {  // :188-194
          const float s = spec[c + F];
          if (live(s, abstol, thr)) {
            phase[c + F] = pc + (fg[c] + fg[c + F]) / 2.0f;
            h_push(heap, hn, -s, c + F);
            spec[c + F] = abstol;
          }
        }
        if (col > 0) {  // :195-201
          const float s = spec[c - F];
          if (live(s, abstol, thr)) {
            phase[c - F] = pc - (fg[c] + fg[c - F]) / 2.0f;
            h_push(heap, hn, -s, c - F);
            spec[c - F] = abstol;
          }
        }
        if (row < F - 1) {  // :202-208
          const float s = spec[c + 1];
          if (live(s, abstol, thr)) {
            phase[c + 1] = pc + (tg[c] + tg[c + 1]) / 2.0f;
            h_push(heap, hn, -s, c + 1);
            spec[c + 1] = abstol;
          }
        }
        if (row > 0) {  // :209-215
          const float s = spec[c - 1];
          if (live(s, abstol, thr)) {
            phase[c - 1] = pc - (tg[c] + tg[c - 1]) / 2.0f;
            h_push(heap, hn, -s, c - 1);
            spec[c - 1] = abstol;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __threadfence_block();
    // :216-219 reseed from the global max of what is left (lane-parallel scan)
    clip_argmax(spec, n, abstol, thr, true, lane, max_val, max_pos);
    if (lane == 0) {
      heap[0].key = -max_val;
      heap[0].idx = (int)max_pos;
      spec[max_pos] = abstol;
    }
    hn = 1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (p.npops && lane == 0) p.npops[b] = npops;
}

// K14 offline, wave-cooperative heap (pghi_heap.h): same binary heap, same sift rules, same pop order as the single-lane
// kernel above; lanes 0-3 handle the popped bin's next-frame / prev-frame / next-bin / prev-bin neighbours.
template <bool PROF>
__global__ __launch_bounds__(512) void pghi_hgi_offline_coop_kernel(HgiParams p) {
  // one wave per clip; 1, 2, 4 or 8 waves per workgroup (independent: no workgroup-level synchronisation).  A
  // workgroup's waves are spread evenly over the CU's four SIMDs, whereas 64-thread workgroups are placed by the
  // dispatcher as it sees fit -- and a SIMD that is handed one clip more than its neighbours finishes them all later:
  // the kernel's tail (4096 clips: 2.00 s as 4096 single-wave workgroups, 1.53 s as 512 eight-wave ones).
  // The wave number is uniform by construction; said explicitly (readfirstlane), the clip's base pointers, the heap
  // descriptor and the segment table live in scalar registers and every cell / heap address is base + 32-bit offset.
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long b = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= p.B) return;
  const int lane = threadIdx.x & 63;
  const int T = p.T, F = p.F;
  const long long n = (long long)T * F;
  float* spec = p.spec + b * n;
  const float* tg = p.tgradw + b * n;
  const float* fg = p.fgradw + b * n;
  float* phase = p.phase + b * n;
  extern __shared__ __attribute__((aligned(16))) u64 heap_top[];
  const size_t per_wave = (size_t)(p.heap_lds_cap + 1) + (size_t)(p.seg_cap + 1) / 2;     // u64 units: heap top, segment maxima
  u64* my_lds = heap_top + (size_t)wave * per_wave;
  const Heap H = {my_lds, reinterpret_cast<u64*>(p.heap + b * (n + 2)), p.heap_lds_cap};
  SegMax G;
  G.m = reinterpret_cast<float*>(my_lds + p.heap_lds_cap + 1);
  G.SL = 512 * ((n + 512LL * p.seg_cap - 1) / (512LL * p.seg_cap));
  if (G.SL < 512) G.SL = 512;
  G.S = (int)((n + G.SL - 1) / G.SL);
  const u64 anc_mask = chain_mask(lane);
  int* order = p.order ? p.order + b * n : nullptr;
  const float abstol = p.abstol;
  const float inv_F = 1.0f / (float)F;

  for (long long i = lane; i < n; i += 64) phase[i] = 0.0f;  // dgt.py:170

  float max_val;
  long long max_pos;
  seg_rebuild(spec, n, G, abstol, 0.f, false, lane, max_val, max_pos);  // :173-174 (+ the segment bounds)
  const float thr = max_val * p.tol;                                   // :177-178
  long long npops = 0;
  long long c_pop1 = 0, c_bubble = 0, c_sift = 0, c_nb = 0, c_push = 0, n_push = 0, s_depth = 0, hn_max = 0;
#define TICK() ((long long)__builtin_amdgcn_s_memtime())
  if (lane == 0) {
    H.store(0, pack_item(-max_val, (int)max_pos));  // :175
    spec[max_pos] = abstol;                         // :176
  }
  int hn = 1;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  while (max_val > abstol) {  // :179
    while (hn > 0) {          // :180
      hn = uni(hn);
      const long long t0 = PROF ? TICK() : 0;
      if (PROF) { s_depth += 31 - __clz((unsigned)hn | 1u); if (hn > hn_max) hn_max = hn; }
      // heappop, part 1: take the last entry off, read the root (heapq.py:51-56)
      const u64 top63 = H.top[lane >= 1 ? lane - 1 : 0];   // root + the first bubble round's subtree, one read
      const u64 last = H.load(hn - 1);     // usually deep in the global part: not needed before the leaf is known
      hn -= 1;
      int c;
      if (hn == 0) c = uni(item_idx(last));
      else c = __builtin_amdgcn_readlane(item_idx(top63), 1);   // the root always lives in LDS: no wait on `last`
      if (order && !PROF && lane == 0) order[npops] = c;
      ++npops;
      // frame / bin of c without an integer division (~25 dependent instructions on the pop's critical path):
      // float quotient, exact after one correction either way
      int col = (int)((float)c * inv_F);
      int row = c - col * F;
      if (row < 0) { row += F; col -= 1; }
      else if (row >= F) { row -= F; col += 1; }
      // request the neighbourhood now (lanes 0..3: next frame, previous frame, next bin, previous bin,
      // dgt.py:188-215); it does not depend on the heap repair below and arrives while that runs
      const int d = (lane == 0) ? F : (lane == 1) ? -F : (lane == 2) ? 1 : -1;
      const bool inb = (lane == 0) ? (col < T - 1) : (lane == 1) ? (col > 0) : (lane == 2) ? (row < F - 1)
                                                                                            : (lane == 3) && (row > 0);
      // Every lane loads (out-of-range neighbours and lanes >= 4 re-read bin c itself: the same cache lines), and
      // every loaded value is consumed outside any branch below.  A load the compiler has to treat as "maybe
      // still pending" at the loop's back edge makes it drain vmcnt at the top of the next pop -- which then
      // starts by sitting out the load of `last`, a deep heap entry, before it has issued anything else.
      const int nb = inb ? c + d : c;
      const float* gr = (lane < 2) ? fg : tg;
      const float s = fload(spec + nb);
      const float g_c = gr[c];
      const float g_n = gr[nb];
      const float pc = fload(phase + c);
      const long long t1 = PROF ? TICK() : 0;
      // heappop, part 2: bubble the smaller children up, drop `last` into the leaf, let it rise
      long long t2 = t1;                  // PROF: the clock between the bubble and the sift
      if (hn > 0) t2 = coop_pop_repair<PROF>(H, hn, last, top63, lane, anc_mask);
      const long long t3 = PROF ? TICK() : 0;
      const float half = (g_c + g_n) / 2.0f;
      const float new_phase = (lane & 1) ? pc - half : pc + half;
      const bool lv = inb && live(s, abstol, thr);     // inb is false on lanes >= 4
      if (lv) {
        phase[nb] = new_phase;
        spec[nb] = abstol;
      }
      const u64 lvmask = __ballot(lv);
      const long long t4 = PROF ? TICK() : 0;
      const u64 mine = pack_item(-s, nb);
      // heappush x (0..4), in lane order (heapq.py:45-48); batching the pushes was slower, profiles/r03_pghi_kernels.md
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if ((lvmask >> q) & 1ull) {
          const u64 item = readlane64(mine, q);
          coop_siftdown(H, hn, item, lane);
          ++hn;
          ++n_push;
        }
      }
      if (PROF) {
        const long long t5 = TICK();
        c_pop1 += t1 - t0; c_bubble += t2 - t1; c_sift += t3 - t2; c_nb += t4 - t3; c_push += t5 - t4;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // the scan below must not hit stale L1 lines
    // :216-219 reseed from the global max of what is left (lane-parallel scan)
    seg_reseed(spec, n, G, abstol, thr, lane, max_val, max_pos);
    if (lane == 0) {
      H.store(0, pack_item(-max_val, (int)max_pos));
      spec[max_pos] = abstol;
    }
    hn = 1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (p.npops && lane == 0) p.npops[b] = npops;
  if (PROF && order && lane == 0 && b == 0) {
    long long* o = reinterpret_cast<long long*>(order);
    o[0] = npops; o[1] = c_pop1; o[2] = c_bubble; o[3] = c_sift; o[4] = c_nb; o[5] = c_push; o[6] = n_push; o[7] = s_depth; o[8] = hn_max;
  }
#undef TICK
}

// ---------------------------------------------------------------------------
// K14 offline, winner-bit variant of the wave-cooperative heap (opt-in: ACIDS_PGHI_KERNEL=wbit; an experiment kept
// runnable, NOT the default -- measured slower, see the end of this comment).
//
// Same array-embedded binary heap, same sift rules, same pop order -- what changes is how the pop finds its
// bubble-up path.  Every internal node of the top 17 levels carries one "winner" bit -- 1 iff heapq.py:33 would
// take the right child: it exists and not (left.key < right.key) -- so the path root -> leaf of a pop is read off
// the bits by ~50 scalar instructions (three LDS words: levels 0-5, 6-11, 12-16) BEFORE any heap entry is loaded.
// All entries the pop needs -- per level: the child that moves up, the grandchild that becomes its new value, the
// sibling it is compared with for the new bit -- are then requested in ONE parallel round (lane k = level k),
// where the cooperative kernel above resolves five levels per dependent round.  A push is one round too
// (ancestors and their siblings by index).  The bits are derived data, kept exact by these rules:
//   * a pop rewrites the bits of the nodes on its path above the slot `last` ends up in;
//   * a push rewrites the bits of the ancestors whose chain child changed (those it passed, plus one);
//   * a bit left pointing at a right child that was since taken off the end of the heap is recognised when the
//     path is read (the position equals the heap's size) and sends the path to the left sibling, a leaf;
// every bit is thus written when its node first gets a child and whenever a child's key changes (model-checked
// against CPython's heapq with heavily tied keys before it was written in HIP).  Levels below 17 (heaps beyond
// 262 143 entries) continue with plain child compares, one dependent round per level.
// Outcome (profiles/r02b_pghi_kernels.md, 1024 dense clips): 2 global round trips per pop instead of ~2.3, but 477
// instructions per pop against 360 -- and with one wave per SIMD a pop costs ~4.7 cycles per instruction whatever
// the memory does: 0.765 s against 0.706 s.  Requesting the first push's ancestors ahead of the pop's round made it
// slower still (the register allocator reuses the prefetch registers, which drains vmcnt early).
// ---------------------------------------------------------------------------
constexpr int WB_LEVELS = 17;                    // winner bits for internal nodes at levels 0..16
constexpr int WB_T1 = 2, WB_T2 = 2 + 128;        // u32 word offsets of the tiers: [t0: 2][t1: 64 x 2][t2: 4096]
constexpr int WB_WORDS = 2 + 128 + 4096;

__device__ __forceinline__ u64 rfl64(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// winner bit of internal node `node` (level <= 16) <- bit.  Called by single lanes; lanes of one wave may hit the
// same word (LDS atomics).
__device__ __forceinline__ void wb_write(unsigned* wb, int node, bool bit) {
  const unsigned q = (unsigned)node + 1u;
  const int lv = 31 - __clz(q);
  const unsigned o = q - (1u << lv);
  const int base_lv = lv < 6 ? 0 : (lv < 12 ? 6 : 12);
  const int d = lv - base_lv;
  const unsigned j = o >> d;                                  // tier word (the ancestor at the tier's first level)
  const unsigned local = (1u << d) + (o & ((1u << d) - 1u));  // heap-order index inside the tier subtree, 1-based
  const unsigned widx = lv < 6 ? (local >> 5) : (lv < 12 ? WB_T1 + 2 * j + (local >> 5) : WB_T2 + j);
  const unsigned m = 1u << (local & 31);
  __hip_atomic_fetch_and(wb + widx, ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  if (bit) __hip_atomic_fetch_or(wb + widx, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// follow the bits from the root: returns the 17 choices, first level in the top bit (scalar unit)
__device__ __forceinline__ unsigned wb_follow(const unsigned* wb, int n) {
  u64 w = rfl64(*reinterpret_cast<const u64*>(wb));
  unsigned i = 1;
#pragma unroll
  for (int k = 0; k < 6; ++k) i = 2 * i + (unsigned)((w >> i) & 1ull);
  const unsigned j1 = i - 64;
  unsigned i2 = 1, i3 = 1, j2 = j1 << 6;
  if (n > 63) {
    w = rfl64(*reinterpret_cast<const u64*>(wb + WB_T1 + 2 * j1));
#pragma unroll
    for (int k = 0; k < 6; ++k) i2 = 2 * i2 + (unsigned)((w >> i2) & 1ull);
    j2 = (j1 << 6) | (i2 - 64);
    if (n > 4095) {
      const unsigned w2 = (unsigned)__builtin_amdgcn_readfirstlane((int)wb[WB_T2 + j2]);
#pragma unroll
      for (int k = 0; k < 5; ++k) i3 = 2 * i3 + ((w2 >> i3) & 1u);
      return (j2 << 5) | (i3 - 32);
    }
    return j2 << 5;
  }
  return j1 << 11;
}

// three (two) entries per lane in one round: LDS part unconditionally, global part under one uniform test.  The
// scheduling barriers keep the loads back to back: left alone, the scheduler slips the first load's select between
// them and the wait that select needs turns one round trip into three.
__device__ __forceinline__ void wb_load3(const Heap& H, int pa, bool va, int pb, bool vb, int pc, bool vc, u64 dflt,
                                         u64& a, u64& b, u64& c) {
  const bool ga = va && pa >= H.cap, gb = vb && pb >= H.cap, gc = vc && pc >= H.cap;
  a = H.top[(va && !ga) ? pa : 0];
  b = H.top[(vb && !gb) ? pb : 0];
  c = H.top[(vc && !gc) ? pc : 0];
  if (__ballot(ga || gb || gc)) {
    const u64* qa = H.rest + (ga ? pa : 0);
    const u64* qb = H.rest + (gb ? pb : 0);
    const u64* qc = H.rest + (gc ? pc : 0);
    __builtin_amdgcn_sched_barrier(0);
    const u64 xa = gload(qa);
    const u64 xb = gload(qb);
    const u64 xc = gload(qc);
    __builtin_amdgcn_sched_barrier(0);
    a = ga ? xa : a;
    b = gb ? xb : b;
    c = gc ? xc : c;
  }
  a = va ? a : dflt;
  b = vb ? b : dflt;
  c = vc ? c : dflt;
}
__device__ __forceinline__ void wb_load2(const Heap& H, int pa, bool va, int pb, bool vb, u64& a, u64& b) {
  const bool ga = va && pa >= H.cap, gb = vb && pb >= H.cap;
  a = H.top[(va && !ga) ? pa : 0];
  b = H.top[(vb && !gb) ? pb : 0];
  if (__ballot(ga || gb)) {
    const u64* qa = H.rest + (ga ? pa : 0);
    const u64* qb = H.rest + (gb ? pb : 0);
    __builtin_amdgcn_sched_barrier(0);
    const u64 xa = gload(qa);
    const u64 xb = gload(qb);
    __builtin_amdgcn_sched_barrier(0);
    a = ga ? xa : a;
    b = gb ? xb : b;
  }
}

// heappush (heapq.py:45-48, 9-21): `item` goes to position `pos` (= the heap's size) and rises; bits of the
// ancestors whose chain child changed are rewritten
__device__ __forceinline__ void wb_push(const Heap& H, unsigned* wb, int pos, u64 item, int lane) {
  const unsigned q = (unsigned)pos + 1u;
  const int depth = 31 - __clz(q);                // number of ancestors (<= 25)
  const int sh = lane < 31 ? lane : 30;
  const int my_dst = (int)(q >> sh) - 1;          // lane j: the chain node below ancestor j+1 (j = 0: pos itself)
  const int my_anc = (int)(q >> (sh + 1)) - 1;    // lane j: ancestor j+1
  const bool act = lane < depth;
  const int sibp = (my_dst & 1) ? my_dst + 1 : my_dst - 1;
  const bool sib_ok = act && sibp <= pos;         // only pos's own right sibling can be missing
  u64 anc, sb;
  wb_load2(H, my_anc, act, sibp, sib_ok, anc, sb);
  const bool rises = act && (item_key(item) < item_key(anc));
  const u64 mask = __ballot(rises);
  const int m = (mask == ~0ull) ? 64 : __builtin_ctzll(~mask);  // item passes ancestors 1 .. m
  if (lane <= m && lane <= depth) H.store(my_dst, lane == m ? item : anc);
  // ancestor j+1 (lane j <= min(m, depth-1)): its chain child my_dst now holds `anc` (j < m) or the item (j == m)
  const int anc_level = depth - 1 - lane;
  if (act && lane <= m && anc_level < WB_LEVELS) {
    const float nk = item_key(lane < m ? anc : item);
    const bool bit = (my_dst & 1) ? (sib_ok && !(nk < item_key(sb))) : !(item_key(sb) < nk);
    wb_write(wb, my_anc, bit);
  }
}

__global__ __launch_bounds__(512) void pghi_hgi_offline_wbit_kernel(HgiParams p) {
  const int wave = threadIdx.x >> 6;
  const long long b = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= p.B) return;
  const int lane = threadIdx.x & 63;
  const int T = p.T, F = p.F;
  const long long n = (long long)T * F;
  float* spec = p.spec + b * n;
  const float* tg = p.tgradw + b * n;
  const float* fg = p.fgradw + b * n;
  float* phase = p.phase + b * n;
  extern __shared__ __attribute__((aligned(16))) u64 heap_top[];
  const size_t per_wave = (size_t)(p.heap_lds_cap + 1) + (WB_WORDS + 1) / 2;      // u64 units
  u64* my_lds = heap_top + (size_t)wave * per_wave;
  const Heap H = {my_lds, reinterpret_cast<u64*>(p.heap + b * (n + 2)), p.heap_lds_cap};
  unsigned* wb = reinterpret_cast<unsigned*>(my_lds + p.heap_lds_cap + 1);
  int* order = p.order ? p.order + b * n : nullptr;
  const float abstol = p.abstol;
  const float inv_F = 1.0f / (float)F;
  const u64 kInf = (u64)0x7f800000u << 32;

  for (long long i = lane; i < n; i += 64) phase[i] = 0.0f;  // dgt.py:170

  float max_val;
  long long max_pos;
  clip_argmax(spec, n, abstol, 0.f, false, lane, max_val, max_pos);  // :173-174
  const float thr = max_val * p.tol;                                   // :177-178
  long long npops = 0;
  if (lane == 0) {
    H.store(0, pack_item(-max_val, (int)max_pos));  // :175
    spec[max_pos] = abstol;                         // :176
  }
  int hn = 1;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  while (max_val > abstol) {  // :179
    while (hn > 0) {          // :180
      hn = uni(hn);
      // heappop, part 1 (heapq.py:51-56): take the last entry off; the root is what is returned
      const int r = hn - 1;
      const u64 rootv = H.top[0];
      const u64 last = H.load(r);
      hn -= 1;
      const int c = (hn == 0) ? uni(item_idx(last)) : uni(item_idx(rootv));
      if (order && lane == 0) order[npops] = c;
      ++npops;
      int col = (int)((float)c * inv_F);
      int row = c - col * F;
      if (row < 0) { row += F; col -= 1; }
      else if (row >= F) { row -= F; col += 1; }
      // neighbourhood (lanes 0..3: next frame, previous frame, next bin, previous bin; dgt.py:188-215), requested now
      const int d = (lane == 0) ? F : (lane == 1) ? -F : (lane == 2) ? 1 : -1;
      const bool inb = (lane == 0) ? (col < T - 1) : (lane == 1) ? (col > 0) : (lane == 2) ? (row < F - 1)
                                                                                            : (lane == 3) && (row > 0);
      const int nb = inb ? c + d : c;
      const float* gr = (lane < 2) ? fg : tg;
      const float s = fload(spec + nb);
      const float g_c = gr[c];
      const float g_n = gr[nb];
      const float pc = fload(phase + c);

      if (hn > 0) {
        // heappop, part 2 (heapq.py:24-42): the path of smaller children from the root, read off the bits ...
        unsigned path = wb_follow(wb, hn);
        int plen = WB_LEVELS;                                   // levels described by `path`
        {
          int pos = (1 << WB_LEVELS) - 1 + (int)path;           // the level-17 node of the path
          // ... and, below level 17, by comparing the children (heaps beyond 2^18 - 1 entries only)
          while (pos < hn && 2 * pos + 1 < hn && plen < 31) {
            const int cl = 2 * pos + 1;
            const float kl = item_key(H.load(cl));
            const bool has_r = cl + 1 < hn;
            const float kr = has_r ? item_key(H.load(cl + 1)) : 0.f;
            const unsigned bsel = (has_r && !(kl < kr)) ? 1u : 0u;
            path = (path << 1) | (unsigned)uni((int)bsel);
            pos = cl + (int)(path & 1u);
            ++plen;
          }
        }
        // lane k = level k: p_k = (2^k - 1) + (first k choices)
        // A bit may still point at a right child that has since been taken off the end of the heap (position hn,
        // even): its left sibling hn - 1 is then the only child, and a leaf -- the path ends there.  (Nothing else
        // can be stale: the bit is rewritten as soon as position hn is filled again.)
        const int k1 = lane + 1, k2 = lane + 2;
        const int gone = (hn & 1) ? -1 : hn;
        int p0 = lane <= plen ? (1 << lane) - 1 + (int)(path >> (plen - lane)) : 0x7fffffff;
        int p1 = k1 <= plen ? (1 << k1) - 1 + (int)(path >> (plen - k1)) : 0x7fffffff;
        int p2 = k2 <= plen ? (1 << k2) - 1 + (int)(path >> (plen - k2)) : 0x7fffffff;
        p0 = p0 == gone ? hn - 1 : p0;
        p1 = p1 == gone ? hn - 1 : p1;
        p2 = p2 == gone ? hn - 1 : p2;
        const int L = __builtin_popcountll(__ballot(p0 < hn)) - 1;          // the path ends at level L (a prefix is valid)
        const bool v1 = p1 < hn, v2 = p2 < hn;
        const int sb1 = (p1 & 1) ? p1 + 1 : p1 - 1;                          // sibling of the child that moves up
        const bool vs = v1 && sb1 < hn;
        u64 X1, X2, S1;
        wb_load3(H, p1, v1, p2, v2, sb1, vs, kInf, X1, X2, S1);
        // `last` goes into the leaf p_L and rises while it is smaller than its parent (heapq.py:39-42): past the
        // entry that moved into p_{L-1} (the old p_L), p_{L-2}, ...  Levels below where it stops keep their entries.
        const u64 R = __ballot(v1 && item_key(last) < item_key(X1));          // bit k: passes the old entry of p_{k+1}
        const u64 Z = ~R & ((1ull << L) - 1ull);
        const int m = Z ? (L - 1) - (63 - __builtin_clzll(Z)) : L;
        const int Lp = L - m;                                                  // `last` ends up in p_{L'}
        if (lane < Lp) H.store(p0, X1);
        else if (lane == Lp) H.store(p0, last);
        if (lane < Lp && lane < WB_LEVELS) {
          const float nk = item_key(lane + 1 < Lp ? X2 : last);               // new entry of the chain child p_{k+1}
          const bool bit = (p1 & 1) ? (vs && !(nk < item_key(S1))) : !(item_key(S1) < nk);
          wb_write(wb, p0, bit);
        }
      }
      const float half = (g_c + g_n) / 2.0f;
      const float new_phase = (lane & 1) ? pc - half : pc + half;
      const bool lv = inb && live(s, abstol, thr);     // inb is false on lanes >= 4
      if (lv) {
        phase[nb] = new_phase;
        spec[nb] = abstol;
      }
      const u64 lvmask = __ballot(lv);
      const u64 mine = pack_item(-s, nb);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if ((lvmask >> q) & 1ull) {
          const u64 item = readlane64(mine, q);
          wb_push(H, wb, hn, item, lane);      // heappush (heapq.py:45-48)
          ++hn;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // the scan below must not hit stale L1 lines
    // :216-219 reseed from the global max of what is left (lane-parallel scan)
    clip_argmax(spec, n, abstol, thr, true, lane, max_val, max_pos);
    if (lane == 0) {
      H.store(0, pack_item(-max_val, (int)max_pos));
      spec[max_pos] = abstol;
    }
    hn = 1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (p.npops && lane == 0) p.npops[b] = npops;
}

// the heap integration proper: spec (B, T, F) is consumed (visited bins are overwritten), the gradients are read only
static int pghi_integrate_launch(float* spec, const float* tg, const float* fg, int64_t B, int T, int F, float tol, float abstol,
                                 float* phase, HeapItem* heap, int64_t* npops_or_null, int32_t* order_or_null, hipStream_t s) {
  static const int prof = [] { const char* e = dev_env("ACIDS_PGHI_PROF"); return (e && e[0] == '1') ? 1 : 0; }();   // dev builds only
  // LDS share of the heap: as much as fits while every clip of the batch can still be resident (160 KB per CU)
  const int cus = num_cus();
  const long long per_cu = (B + cus - 1) / cus;
  const int cap = per_cu <= 1 ? 16383 : per_cu <= 2 ? 8191 : per_cu <= 4 ? 4095 : per_cu <= 8 ? 2047 : per_cu <= 16 ? 1023 : 511;
  // segment maxima for the reseeds (cooperative kernel), behind the heap's top: as many as keep per_cu clips resident
  const int seg_cap = per_cu <= 4 ? 1024 : per_cu <= 8 ? 512 : 192;
  const size_t heap_lds = sizeof(u64) * ((size_t)(cap + 1) + (size_t)(seg_cap + 1) / 2);
  HgiParams h = {spec, tg, fg, phase, heap, (long long)B, T, F, abstol, tol, (long long*)npops_or_null, cap, seg_cap, prof,
                 order_or_null};
  // at_set_variant(AT_VARIANT_PGHI_KERNEL, 2) selects the single-lane reference kernel (debugging aid; identical results),
  // 1 the winner-bit variant (identical results; slower on every batch measured, see the comment above it and DESIGN.md
  // 3.4 -- kept selectable so that the parity tests and tools/fuzz_pghi.py can run it)
  const int pghi_kernel = variant(kVarPghiKernel);
  // waves per workgroup: as many (<= 8) as keep the workgroup's LDS within the CU's 160 KB (launch_waves)
  const int wpb = per_cu >= 8 ? 8 : per_cu >= 4 ? 4 : per_cu >= 2 ? 2 : 1;
  if (pghi_kernel == 2) {
    hipLaunchKernelGGL(pghi_hgi_offline_kernel, dim3((unsigned)B), dim3(64), 0, s, h);
    return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
  }
  if (pghi_kernel == 1 && !prof) {
    // winner-bit kernel: per clip 16.5 KB of bits + the heap's top levels in LDS; at most 8 clips resident per CU
    const int wcap = per_cu <= 4 ? 2047 : per_cu <= 6 ? 1023 : 255;
    h.heap_lds_cap = wcap;
    const size_t per_wave = sizeof(u64) * ((size_t)(wcap + 1) + (WB_WORDS + 1) / 2);
    return launch_waves(pghi_hgi_offline_wbit_kernel, B, wpb, per_wave, 512, s, h);
  }
  return launch_waves(prof ? pghi_hgi_offline_coop_kernel<true> : pghi_hgi_offline_coop_kernel<false>, B, wpb, heap_lds, 1024, s, h);
}

// the workspace of both entry points: spec | tg | fg (fp32, B n each) | heap (8-byte entries, n + 2 per clip, 16-byte aligned)
struct OfflineWorkspace {
  float *spec, *tg, *fg;
  HeapItem* heap;
};
static OfflineWorkspace carve_offline(void* workspace, int64_t B, size_t n) {
  OfflineWorkspace w;
  w.spec = (float*)workspace;
  w.tg = w.spec + (size_t)B * n;
  w.fg = w.tg + (size_t)B * n;
  w.heap = (HeapItem*)(((uintptr_t)(w.fg + (size_t)B * n) + 15) & ~(uintptr_t)15);
  return w;
}

}  // namespace at_hip

using namespace at_hip;

extern "C" {

int at_pghi_gradients(const float* mag, int64_t B, int T, int F, float gamma, int n_fft, int hop, float eps,
                      float* tgradw, float* fgradw, float* spec_or_null, void* stream) {
  if (B < 0 || T <= 0 || F <= 0 || n_fft <= 0 || hop <= 0) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!mag || !tgradw || !fgradw) return AT_EINVAL;
  GradParams p = {mag, spec_or_null, tgradw, fgradw, (long long)B, T, F, n_fft, hop, gamma, eps};
  hipLaunchKernelGGL(pghi_grad_offline_kernel, dim3(grid1d((long long)B * T * F)), dim3(256), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

size_t at_pghi_offline_workspace_bytes(int64_t B, int T, int F) {
  const size_t n = (size_t)T * (size_t)F;
  // spec + tgradw + fgradw (fp32) + heap (8 B entries, n + 2)
  return (size_t)B * (3 * n * sizeof(float) + (n + 2) * sizeof(HeapItem)) + 256;
}

int at_pghi_offline(const float* mag, int64_t B, int T, int F, float gamma, int n_fft, int hop, float tol, float abstol,
                    float* phase, void* workspace, size_t workspace_bytes, int64_t* npops_or_null,
                    int32_t* order_or_null, void* stream) {
  if (B < 0 || T <= 0 || F <= 0 || n_fft <= 0 || hop <= 0) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!mag || !phase) return AT_EINVAL;
  // heap positions are 32-bit and a bubble round addresses ((pos + 1) << 5) + 31; the frame / bin split of a bin
  // index goes through fp32: both hold up to 2^26 bins per clip (12 minutes of audio at n_fft 1024, hop 256)
  if ((long long)T * F > (1LL << 26) - 64) return AT_EUNSUPPORTED;
  if (!workspace || workspace_bytes < at_pghi_offline_workspace_bytes(B, T, F)) return AT_EWORKSPACE;
  const OfflineWorkspace w = carve_offline(workspace, B, (size_t)T * (size_t)F);
  hipStream_t s = (hipStream_t)stream;
  GradParams g = {mag, w.spec, w.tg, w.fg, (long long)B, T, F, n_fft, hop, gamma, abstol};
  hipLaunchKernelGGL(pghi_grad_offline_kernel, dim3(grid1d((long long)B * T * F)), dim3(256), 0, s, g);
  return pghi_integrate_launch(w.spec, w.tg, w.fg, B, T, F, tol, abstol, phase, w.heap, npops_or_null, order_or_null, s);
}

int at_pghi_integrate(const float* mag, const float* tgradw, const float* fgradw, int64_t B, int T, int F, float tol,
                      float abstol, float* phase, void* workspace, size_t workspace_bytes, int64_t* npops_or_null,
                      int32_t* order_or_null, void* stream) {
  if (B < 0 || T <= 0 || F <= 0) return AT_EINVAL;
  if (B == 0) return AT_OK;
  if (!mag || !tgradw || !fgradw || !phase) return AT_EINVAL;
  if ((long long)T * F > (1LL << 26) - 64) return AT_EUNSUPPORTED;
  if (!workspace || workspace_bytes < at_pghi_offline_workspace_bytes(B, T, F)) return AT_EWORKSPACE;
  const size_t n = (size_t)T * (size_t)F;
  const OfflineWorkspace w = carve_offline(workspace, B, n);   // the caller's gradients are used in place: tg / fg stay idle
  hipStream_t s = (hipStream_t)stream;
  // the integration marks visited bins in its own copy
  if (hipMemcpyAsync(w.spec, mag, sizeof(float) * (size_t)B * n, hipMemcpyDeviceToDevice, s) != hipSuccess) return AT_ELAUNCH;
  return pghi_integrate_launch(w.spec, tgradw, fgradw, B, T, F, tol, abstol, phase, w.heap, npops_or_null, order_or_null, s);
}

}  // extern "C"

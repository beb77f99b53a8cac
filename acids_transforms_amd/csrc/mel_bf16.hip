// mel_bf16.hip -- |X| -> mel filterbank as a dense bf16 MFMA GEMM (fp32 accumulate), fused contrast / normalise.
//
// BASELINE config 5's projection ("bf16 MFMA mel"): replaces  x.abs(); torch.matmul(mag, mel_bank); contrast;
// Normalize.forward  (reference transforms/spectral_repr.py:215-226) with both operands rounded to bf16
// (round-to-nearest-even) and products accumulated in fp32 on the matrix cores
// (v_mfma_f32_32x32x16_bf16).  It does NOT meet the 1e-5 parity bar of the fp32 paths (bf16 keeps 8
// significant bits: ~4e-3 relative) -- it is the opt-in `Magnitude(bank_dtype="bf16")` /
// StreamingDGTSession path; mel.hip / mel_banded.hip stay the default.
//
// Shape of the work: [rows x K] . [K x N], K = n_fft/2+1 (513), N = n_mels (128): 131 kflop and 4.1 KB of input
// per row -> HBM-bound by a factor of ~10 even at the bf16 MFMA rate, so the kernel is organised around the
// input stream, not around the MFMA pipe:
//   * 256-thread workgroup (4 waves, one per SIMD), persistent over 128-row tiles; wave w owns rows 32w..32w+31
//     of a tile and ALL (<= 128) output columns of the workgroup's column chunk: 4 accumulators of 32x32;
//   * the bank chunk, bf16, TRANSPOSED ([column][k], k contiguous) sits in LDS for the whole launch
//     (128 x 536 x 2 B = 134 KB; row stride 268 dwords = 4*67: the 16 lanes of a ds_read_b128 group hit 16
//     distinct 16-byte bank groups);
//   * A is streamed in 64-bin chunks: one coalesced 512-byte global load per row (8 B per lane, complex64),
//     |.| + cvt to bf16 in registers, parked in a wave-private 32 x 64 LDS slab (row stride 36 dwords, also
//     conflict-free for the fragment reads), read back as MFMA A fragments.  The next chunk's loads are issued
//     before the current chunk's MFMAs.  No workgroup barrier after the bank is loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acids_hip.h"
#include "mel_gemm.h"
#include "variants.h"

namespace at_hip {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BF_THREADS = 256;
constexpr int BF_TILE_ROWS = 128;       // per workgroup: 4 waves x 32 rows
constexpr int BF_CHUNK = 64;            // bins staged per step
constexpr int BF_AST = 72;              // A slab row stride in bf16 (144 B = 36 dwords)

struct MelBf16Params {
  const void* A;          // rows x K (complex64 or float32), row stride lda elements
  const __bf16* bank;     // packed image [n_pad][k_img], zeros in the padding
  float* out;
  const float* offset;
  const float* scale;
  long long rows, lda, ld_out;
  int K, N, k_img, n_pad;
  int a_kind, contrast;
  float eps;
  int kl;                 // LDS row stride of the bank in bf16 (k_img + 8)
  int nc;                 // columns per workgroup chunk (multiple of 32, <= 128)
  long long n_tiles;
};

__device__ __forceinline__ void wave_lds_sync() {
  // the slab is written and read by different lanes of the same wave: LDS operations of one wave complete in
  // order, what has to be pinned is the compiler's ordering
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one 64-bin chunk of the wave's 32 rows: issue the loads (8 B per lane for complex input, 4 B for real)
template <bool CPLX>
__device__ __forceinline__ void chunk_load(const MelBf16Params& p, long long row0, int k0, int lane, float2 (&regs)[32]) {
  const int k = k0 + lane;
  const int kc = k < p.K ? k : p.K - 1;            // clamped: unconditional loads (a conditional one drains vmcnt)
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    long long row = row0 + i;
    if (row >= p.rows) row = p.rows - 1;
    const long long at = row * p.lda + kc;
    if (CPLX) {
      regs[i] = reinterpret_cast<const float2*>(p.A)[at];
    } else {
      regs[i].x = reinterpret_cast<const float*>(p.A)[at];
    }
  }
}

template <bool CPLX>
__device__ __forceinline__ void chunk_park(const MelBf16Params& p, int k0, int lane, const float2 (&regs)[32], __bf16* slab) {
  const bool live = (k0 + lane) < p.K;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    float v;
    if (CPLX) {
      const float s2 = fmaf(regs[i].x, regs[i].x, regs[i].y * regs[i].y);
      v = (p.a_kind == A_COMPLEX_ABS2) ? s2 : __builtin_amdgcn_sqrtf(s2);
    } else {
      v = (p.a_kind == A_REAL_ABS) ? fabsf(regs[i].x) : regs[i].x;
    }
    slab[i * BF_AST + lane] = (__bf16)(live ? v : 0.0f);
  }
}

template <int NT, bool CPLX>
__global__ __launch_bounds__(BF_THREADS) void mel_bf16_kernel(MelBf16Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16* Bs = reinterpret_cast<__bf16*>(smem_raw);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __bf16* slab = Bs + (size_t)p.nc * p.kl + (size_t)wave * 32 * BF_AST;
  const int col0 = blockIdx.y * p.nc;               // first column of this workgroup's chunk

  // ---- bank chunk -> LDS, 16 bytes per thread per pass (image rows are 16-byte multiples) ----
  {
    const int pieces_per_row = p.k_img / 8;
    const int total = p.nc * pieces_per_row;
    for (int idx = threadIdx.x; idx < total; idx += BF_THREADS) {
      const int n = idx / pieces_per_row, q = idx - n * pieces_per_row;
      const int gn = col0 + n;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (gn < p.n_pad) v = *reinterpret_cast<const uint4*>(p.bank + (size_t)gn * p.k_img + q * 8);
      *reinterpret_cast<uint4*>(Bs + (size_t)n * p.kl + q * 8) = v;
    }
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  const int n_chunks = (p.k_img + BF_CHUNK - 1) / BF_CHUNK;
  float off = 0.f, sc = 1.f;
  const bool norm = p.offset != nullptr;
  if (norm) { off = *p.offset; sc = *p.scale; }

  for (long long tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
    const long long row0 = tile * BF_TILE_ROWS + wave * 32;
    if (row0 >= p.rows) continue;                   // uniform per wave; no barrier inside the loop
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    float2 regs[32];
    chunk_load<CPLX>(p, row0, 0, lane, regs);
    for (int c = 0; c < n_chunks; ++c) {
      const int k0 = c * BF_CHUNK;
      chunk_park<CPLX>(p, k0, lane, regs, slab);    // waits for the chunk's loads, frees the registers
      if (c + 1 < n_chunks) chunk_load<CPLX>(p, row0, k0 + BF_CHUNK, lane, regs);   // in flight during the MFMAs
      wave_lds_sync();
      const int steps = (p.k_img - k0) >= BF_CHUNK ? BF_CHUNK / 16 : (p.k_img - k0) / 16;
      for (int s = 0; s < steps; ++s) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(slab + r * BF_AST + s * 16 + 8 * h);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (size_t)(t * 32 + r) * p.kl + k0 + s * 16 + 8 * h);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
      wave_lds_sync();                              // the slab is rewritten by the next chunk
    }

    // ---- epilogue: C/D map of the 32x32 shape: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) ----
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = col0 + t * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const long long row = row0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row < p.rows && col < p.N) {
          float v = contrast_fwd(acc[t][e], p.contrast, p.eps);
          if (norm) v = (v - off) / sc;
          p.out[row * p.ld_out + col] = v;
        }
      }
    }
  }
}

// fp32 (K, N) bank -> the kernel's bf16 operand image [n_pad][k_img] (transposed, zero padded), RNE
__global__ void mel_bf16_pack_kernel(const float* __restrict__ bank, int K, int ldb, int N, int k_img, int n_pad,
                                     __bf16* __restrict__ img) {
  const long long total = (long long)n_pad * k_img;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i / k_img), k = (int)(i - (long long)n * k_img);
    const float v = (n < N && k < K) ? bank[(long long)k * ldb + n] : 0.0f;
    img[i] = (__bf16)v;
  }
}

static inline int bf_k_img(int K) { return (K + 15) / 16 * 16; }
static inline int bf_n_pad(int N) { return (N + 31) / 32 * 32; }

}  // namespace at_hip

using namespace at_hip;

extern "C" {

size_t at_mel_bf16_bank_bytes(int K, int N) {
  if (K <= 0 || N <= 0) return 0;
  return (size_t)bf_k_img(K) * (size_t)bf_n_pad(N) * 2;
}

int at_mel_bf16_pack_bank(const float* bank, int K, int ldb, int N, void* bank_bf16, void* stream) {
  if (!bank || !bank_bf16 || K <= 0 || N <= 0 || ldb < N) return AT_EINVAL;
  const int k_img = bf_k_img(K), n_pad = bf_n_pad(N);
  const long long total = (long long)k_img * n_pad;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(mel_bf16_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, bank, K, ldb, N, k_img, n_pad,
                     reinterpret_cast<__bf16*>(bank_bf16));
  return hipGetLastError() == hipSuccess ? AT_OK : AT_ELAUNCH;
}

int at_mel_project_bf16(const void* A, int a_kind, int64_t rows, int64_t lda, int K, const void* bank_bf16, int N,
                        int contrast, const float* offset, const float* scale, float eps, float* out, int64_t ld_out,
                        void* stream) {
  if (rows < 0 || K <= 0 || N <= 0 || lda < K || ld_out < N) return AT_EINVAL;
  if (a_kind < 0 || a_kind > 3 || contrast < 0 || contrast > 3) return AT_EINVAL;
  if ((offset == nullptr) != (scale == nullptr)) return AT_EINVAL;
  if (rows == 0) return AT_OK;
  if (!A || !bank_bf16 || !out) return AT_EINVAL;
  MelBf16Params p = {};
  p.A = A; p.bank = reinterpret_cast<const __bf16*>(bank_bf16); p.out = out; p.offset = offset; p.scale = scale;
  p.rows = rows; p.lda = lda; p.ld_out = ld_out;
  p.K = K; p.N = N; p.k_img = bf_k_img(K); p.n_pad = bf_n_pad(N);
  p.a_kind = a_kind; p.contrast = contrast; p.eps = eps;
  p.kl = p.k_img + 8;
  // columns per workgroup chunk: as many 32-column tiles (<= 4) as fit in LDS beside the four A slabs
  const size_t slabs = (size_t)4 * 32 * BF_AST * 2;
  const size_t lds_max = 160 * 1024;
  int nc = p.n_pad < 128 ? p.n_pad : 128;
  while (nc > 0 && (size_t)nc * p.kl * 2 + slabs > lds_max) nc -= 32;
  if (nc <= 0) return AT_EUNSUPPORTED;            // K too large for one 32-column tile (n_fft > 4096)
  p.nc = nc;
  p.n_tiles = (rows + BF_TILE_ROWS - 1) / BF_TILE_ROWS;
  const size_t lds = (size_t)nc * p.kl * 2 + slabs;
  const int nt = nc / 32;
  const bool cplx = a_kind < A_REAL;
  const void* fn = nullptr;
#define BF_PICK(NT_)                                                                               \
  fn = cplx ? reinterpret_cast<const void*>(&mel_bf16_kernel<NT_, true>)                           \
            : reinterpret_cast<const void*>(&mel_bf16_kernel<NT_, false>)
  switch (nt) {
    case 1: BF_PICK(1); break;
    case 2: BF_PICK(2); break;
    case 3: BF_PICK(3); break;
    default: BF_PICK(4); break;
  }
#undef BF_PICK
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      return AT_ELAUNCH;
    }
  }
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
  }
  const unsigned ychunks = (unsigned)((p.n_pad + nc - 1) / nc);
  long long gx = p.n_tiles < cus ? p.n_tiles : cus;   // one workgroup per CU (LDS-limited), persistent over tiles
  if (const long long forced = at_hip::forced_row_run(p.n_tiles)) gx = (p.n_tiles + forced - 1) / forced;   // AT_VARIANT_ROW_RUN
  dim3 grid((unsigned)gx, ychunks), block(BF_THREADS);
  void* args[] = {&p};
  if (hipLaunchKernel(fn, grid, block, args, lds, (hipStream_t)stream) != hipSuccess) {
    (void)hipGetLastError();
    return AT_ELAUNCH;
  }
  return AT_OK;
}

}  // extern "C"

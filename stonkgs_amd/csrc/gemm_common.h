// Argument block and helpers shared by the bf16 GEMM kernels (gemm_bf16.hip, gemm256.hip, gemm_w4.hip, gemm_a4.hip and the
// weight-gradient forms gemm_tn.hip, gemm_tn_a4.hip): device-side epilogues, waits and tile mapping first, the launchers'
// host-side helpers at the end. See stonk_gemm_nt_bf16 in include/stonk_hip.h for the meaning of each field.
#pragma once
#include "common.h"
#include "stonk_flags.h"

namespace stonk_gemm {

struct GemmArgs {
  const bf16* A;
  const bf16* B;
  void* C;
  const float* bias;
  const bf16* resid;
  bf16* aux;
  const int* m_dev;
  const int* k_dev;
  long lda, ldb, ldc, ldr, ldaux;
  int M, N, K;
  int flags;
  float alpha;
  int split_k;
  uint32_t drop_thr32;
  float drop_scale;
  uint32_t seed;      // already mixed (stonk_seed_mix)
};

// blocks b and b+8 share an XCD (round-robin dispatch): give each XCD a contiguous run of tiles so
// neighbouring tiles (same A row panel / same B column panel) hit the same L2. Bijective for any n.
__device__ __forceinline__ int xcd_remap(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7;
  const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + (b >> 3);
}

// raw s_barrier and counted waits (never __syncthreads, which would drain the loads in flight)
__device__ __forceinline__ void barrier() { __builtin_amdgcn_s_barrier(); }
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt is six bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// one work item of the persistent 256-row kernels whose K position is an element offset (gemm256.hip, gemm_w4.hip,
// gemm_tn_a4.hip; gemm_a4.hip counts K tiles and keeps its own)
struct Work {
  int m0, n0;       // tile origin
  long k_begin;     // element offset of the first K tile (TN: first token)
  int nk;           // K tiles in this work item
};

// Fused epilogue on 4 consecutive output columns n..n+3 of row m (values already scaled by alpha).
__device__ __forceinline__ f32x4 epilogue4(f32x4 v, const GemmArgs& p, int flags, int m, int n) {
  if (flags & STONK_EPI_BIAS) v += *(const f32x4*)(p.bias + n);
  if (flags & STONK_EPI_SAVE_PREACT) {
    const bool ag = (flags & STONK_EPI_AUX_GRAD) != 0;
    bf16x4 u = {(bf16)gelu_saved(v[0], ag), (bf16)gelu_saved(v[1], ag), (bf16)gelu_saved(v[2], ag),
                (bf16)gelu_saved(v[3], ag)};
    *(bf16x4*)(p.aux + (long)m * p.ldaux + n) = u;
  }
  if (flags & STONK_EPI_GELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
  }
  if (flags & STONK_EPI_GELU_BWD) {
    const bf16x4 u = *(const bf16x4*)(p.aux + (long)m * p.ldaux + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= gelu_factor((float)u[r], (flags & STONK_EPI_AUX_GRAD) != 0);
  }
  if (flags & STONK_EPI_DROPOUT) {
    const uint32_t rk = stonk_rowkey((uint32_t)m, p.seed), ck = stonk_colkey((uint32_t)n);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      v[r] = stonk_keep_key(rk, ck + (uint32_t)r * STONK_G_COL, p.drop_thr32) ? v[r] * p.drop_scale : 0.f;
  }
  if (flags & STONK_EPI_RESID) {
    const bf16x4 rr = *(const bf16x4*)(p.resid + (long)m * p.ldr + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += (float)rr[r];
  }
  return v;
}

// Fused epilogue on 8 consecutive output columns n..n+7 of row m (fp32 values already scaled by alpha): every side
// operand (bias, saved pre-activation, residual) is read / written as one 16- or 32-byte vector.
__device__ __forceinline__ void epilogue8(float (&v)[8], const GemmArgs& p, int flags, int m, int n) {
  if (flags & STONK_EPI_BIAS) {
    const f32x4 b0 = *(const f32x4*)(p.bias + n), b1 = *(const f32x4*)(p.bias + n + 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] += b0[r];
      v[4 + r] += b1[r];
    }
  }
  if (flags & STONK_EPI_SAVE_PREACT) {
    bf16x8 u;
#pragma unroll
    for (int r = 0; r < 8; ++r) u[r] = (bf16)gelu_saved(v[r], (flags & STONK_EPI_AUX_GRAD) != 0);
    *(bf16x8*)(p.aux + (long)m * p.ldaux + n) = u;
  }
  if (flags & STONK_EPI_GELU) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = gelu_erf(v[r]);
  }
  if (flags & STONK_EPI_GELU_BWD) {
    const bf16x8 u = *(const bf16x8*)(p.aux + (long)m * p.ldaux + n);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] *= gelu_factor((float)u[r], (flags & STONK_EPI_AUX_GRAD) != 0);
  }
  if (flags & STONK_EPI_DROPOUT) {
    const uint32_t rk = stonk_rowkey((uint32_t)m, p.seed), ck = stonk_colkey((uint32_t)n);
#pragma unroll
    for (int r = 0; r < 8; ++r)
      v[r] = stonk_keep_key(rk, ck + (uint32_t)r * STONK_G_COL, p.drop_thr32) ? v[r] * p.drop_scale : 0.f;
  }
  if (flags & STONK_EPI_RESID) {
    const bf16x8 rr = *(const bf16x8*)(p.resid + (long)m * p.ldr + n);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += (float)rr[r];
  }
}

// Side operands of one epilogue8 call, fetched AHEAD of their use (one round earlier) so that the global-load latency
// of the residual / saved pre-activation is not paid once per 16-row round.
struct SideOps {
  bf16x8 aux, res;
};
__device__ __forceinline__ void side_prefetch(SideOps& s, const GemmArgs& p, int flags, int m, int n, bool ok) {
  if (!ok) return;
  if (flags & STONK_EPI_GELU_BWD) s.aux = *(const bf16x8*)(p.aux + (long)m * p.ldaux + n);
  if (flags & STONK_EPI_RESID) s.res = *(const bf16x8*)(p.resid + (long)m * p.ldr + n);
}
// single-vector form for kernels that carry exactly one side operand (GELU' input OR residual)
__device__ __forceinline__ bf16x8 side_load1(const GemmArgs& p, int flags, int m, int n, bool ok) {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
  if (!ok) return z;
  if (flags & STONK_EPI_GELU_BWD) return *(const bf16x8*)(p.aux + (long)m * p.ldaux + n);
  return *(const bf16x8*)(p.resid + (long)m * p.ldr + n);
}
// epilogue8 with preloaded bias (8 columns of this lane, fixed for the whole tile) and side operands
__device__ __forceinline__ void epilogue8_pre(float (&v)[8], const GemmArgs& p, int flags, int m, int n, const f32x4& b0,
                                              const f32x4& b1, const SideOps& s) {
  if (flags & STONK_EPI_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] += b0[r];
      v[4 + r] += b1[r];
    }
  }
  if (flags & STONK_EPI_SAVE_PREACT) {
    bf16x8 u;
#pragma unroll
    for (int r = 0; r < 8; ++r) u[r] = (bf16)gelu_saved(v[r], (flags & STONK_EPI_AUX_GRAD) != 0);
    *(bf16x8*)(p.aux + (long)m * p.ldaux + n) = u;
  }
  if (flags & STONK_EPI_GELU) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = gelu_erf(v[r]);
  }
  if (flags & STONK_EPI_GELU_BWD) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] *= gelu_factor((float)s.aux[r], (flags & STONK_EPI_AUX_GRAD) != 0);
  }
  if (flags & STONK_EPI_DROPOUT) {
    const uint32_t rk = stonk_rowkey((uint32_t)m, p.seed), ck = stonk_colkey((uint32_t)n);
#pragma unroll
    for (int r = 0; r < 8; ++r)
      v[r] = stonk_keep_key(rk, ck + (uint32_t)r * STONK_G_COL, p.drop_thr32) ? v[r] * p.drop_scale : 0.f;
  }
  if (flags & STONK_EPI_RESID) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += (float)s.res[r];
  }
}

// ---------------------------------------------------------------- host side: what every launcher does
// Epilogue bits by their short names, for the launchers' switch (epi) blocks that name the compiled instances.
namespace epi_bits {
constexpr int B = STONK_EPI_BIAS, G = STONK_EPI_GELU, SV = STONK_EPI_SAVE_PREACT, GB = STONK_EPI_GELU_BWD,
              R = STONK_EPI_RESID, D = STONK_EPI_DROPOUT, AG = STONK_EPI_AUX_GRAD;
constexpr int MASK = B | G | SV | GB | R | D | AG;   // = 0x1FC: flags & MASK == 0 is the plain product
}  // namespace epi_bits

// CUs of the current device, asked once per process (one process per GPU); <= 0: the query failed, hipGetLastError() says why
inline int cu_count() {
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    n_cu = prop.multiProcessorCount;
  }
  return n_cu;
}

// Launch of a kernel whose dynamic LDS exceeds the default limit: the attribute is per function (and device), so the
// "already set" flag is per KERNEL - every instance of a kernel template has its own.
template <auto KERNEL, int LDS, typename Args>
int launch_with_lds(const Args& a, int grid, int block, hipStream_t st) {
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    attr_done = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), LDS, st, a);
  return stonk_launch_status();
}

// The four-wave kernels' 256 x (256 | 192) tiles (gemm_w4.hip, gemm_a4.hip). 192-wide instances exist for the epilogues of
// the N = 768 launches (none, bias, residual, bias + residual [+ dropout]) ...
inline bool epi_has_192(int e) {
  using namespace epi_bits;
  return e == 0 || e == B || e == R || e == (B | R) || e == (B | R | D);
}
// ... and are chosen (tile_n == 0 on entry) where they quantise better: time ~ rounds of the CUs x tile width (N = 768 at
// 32 768 rows: two full rounds instead of one and a half; at 16 384 rows one full round instead of 3/4). Returns the grid:
// one persistent workgroup per CU, or (items_per_wg > 0) work items / items_per_wg. k_shares: work items per output tile.
inline int tile_grid_256(const GemmArgs& a, bool has192, long k_shares, int items_per_wg, int n_cu, int& tile_n) {
  const long ntm = (a.M + 255) / 256;
  const long t256 = ntm * ((a.N + 255) / 256) * k_shares, t192 = ntm * (a.N / 192) * k_shares;
  if (tile_n == 0) {
    const long c256 = ((t256 + n_cu - 1) / n_cu) * 256, c192 = ((t192 + n_cu - 1) / n_cu) * 192;
    tile_n = (has192 && c192 < c256) ? 192 : 256;
  }
  const long tiles = tile_n == 192 ? t192 : t256;
  return (int)(items_per_wg > 0 ? (tiles + items_per_wg - 1) / items_per_wg : (tiles < n_cu ? tiles : n_cu));
}

}  // namespace stonk_gemm

// Argument block and helpers shared by the bf16 GEMM kernels (gemm_bf16.hip, gemm256.hip, gemm_w4.hip, gemm_a4.hip and the
// weight-gradient forms gemm_tn.hip, gemm_tn_a4.hip): device-side epilogues, waits and tile mapping first, the launchers'
// host-side helpers at the end. See stonk_gemm_nt_bf16 in include/stonk_hip.h for the meaning of each field.
#pragma once
#include <type_traits>

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

// Argument block of the grouped weight-gradient kernel (gemm_tn_a4_group.hip): problem i owns the block indices
// first[i] .. first[i] + items[i] - 1, one work item each (items[i] = its tiles x prob[i].split_k); first[] ascends.
struct TnGroupArgs {
  static constexpr int MAX = 4;
  GemmArgs prob[MAX];
  int first[MAX], items[MAX];
  int n;
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

// A capacity that a count in device memory may lower: min(cap, ceil(*dev / per)). Rows (m_dev) and tokens (k_dev) with
// per = 1, K tiles (k_dev) with per = 64. (all six kernels; gemm256.hip clamps its rows in its own text - with this helper
// its register allocation came out differently)
__device__ __forceinline__ int live_count(const int* dev, int cap, int per = 1) {
  if (dev) {
    const int d = (*dev + per - 1) / per;
    cap = d < cap ? d : cap;
  }
  return cap;
}

// Tile tt of ntm x ntn -> (row tile, column tile), walking the SHORTER dimension fastest, so that consecutive tiles share
// the operand panel of the longer one. (all six kernels)
struct TileRC {
  int rt, ct;
};
__device__ __forceinline__ TileRC tile_split(int tt, int ntm, int ntn) {
  if (ntm >= ntn) {
    const int rt = tt / ntn;
    return {rt, tt - rt * ntn};
  }
  const int ct = tt / ntm;
  return {tt - ct * ntm, ct};
}

// The next work item of this workgroup that has K tiles (k_dev may leave a K split empty): wi += G until get_work(wi, out)
// says there is none (false) or out.nk > 0. (gemm_tn_a4.hip, gemm_w4.hip's prefetch cursor; the other skip-empty loops of
// gemm256.hip and gemm_w4.hip compile to other instructions through it and keep their own text)
template <typename GetWork, typename W>
__device__ __forceinline__ bool next_live_work(GetWork&& get_work, int& wi, int G, W& out) {
  do {
    wi += G;
    if (!get_work(wi, out)) return false;
  } while (out.nk <= 0);
  return true;
}

// The element-wise stages of the fused epilogue on W consecutive output columns n..n+W-1 of row m (values already scaled
// by alpha), in their one order: bias, saved pre-activation (or GELU'; stored from here), GELU, GELU', dropout, residual.
// v: f32x4 or float[W]. Side operands: bias() = the W fp32 of the bias, aux() / res() = the W bf16 of the GELU' input /
// the residual, each asked for at its stage (a caller without prefetched ones loads them there). epilogue4 and
// epilogue8_pre are this chain; gemm_bf16.hip's constant-flag epilogue keeps the same stages in its own text (through the
// chain it needs two more VGPRs), and gemm_w4.hip / gemm_a4.hip do bias and GELU themselves and pass the rest here.
template <int W, typename V, typename Bias, typename Aux, typename Res>
__device__ __forceinline__ void epilogue_chain(V& v, const GemmArgs& p, int flags, int m, int n, Bias&& bias, Aux&& aux, Res&& res) {
  typedef bf16 bf16xW __attribute__((ext_vector_type(W)));
  if (flags & STONK_EPI_BIAS) {
    const auto b = bias();
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] += b[r];
  }
  if (flags & STONK_EPI_SAVE_PREACT) {
    bf16xW u;
#pragma unroll
    for (int r = 0; r < W; ++r) u[r] = (bf16)gelu_saved(v[r], (flags & STONK_EPI_AUX_GRAD) != 0);
    *(bf16xW*)(p.aux + (long)m * p.ldaux + n) = u;
  }
  if (flags & STONK_EPI_GELU) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = gelu_erf(v[r]);
  }
  if (flags & STONK_EPI_GELU_BWD) {
    const bf16xW u = aux();
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] *= gelu_factor((float)u[r], (flags & STONK_EPI_AUX_GRAD) != 0);
  }
  if (flags & STONK_EPI_DROPOUT) {
    const uint32_t rk = stonk_rowkey((uint32_t)m, p.seed), ck = stonk_colkey((uint32_t)n);
#pragma unroll
    for (int r = 0; r < W; ++r)
      v[r] = stonk_keep_key(rk, ck + (uint32_t)r * STONK_G_COL, p.drop_thr32) ? v[r] * p.drop_scale : 0.f;
  }
  if (flags & STONK_EPI_RESID) {
    const bf16xW rr = res();
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] += (float)rr[r];
  }
}

// Fused epilogue on 4 consecutive output columns n..n+3 of row m (values already scaled by alpha), side operands loaded here.
__device__ __forceinline__ f32x4 epilogue4(f32x4 v, const GemmArgs& p, int flags, int m, int n) {
  epilogue_chain<4>(v, p, flags, m, n, [&] { return *(const f32x4*)(p.bias + n); },
                    [&] { return *(const bf16x4*)(p.aux + (long)m * p.ldaux + n); },
                    [&] { return *(const bf16x4*)(p.resid + (long)m * p.ldr + n); });
  return v;
}

// Side operands (8 consecutive columns of one row) of one epilogue8_pre call, fetched AHEAD of their use (one round
// earlier) so that the global-load latency of the residual / saved pre-activation is not paid once per 16-row round.
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
// Fused epilogue on 8 consecutive output columns n..n+7 of row m (fp32 values already scaled by alpha), with preloaded
// bias (8 columns of this lane, fixed for the whole tile) and side operands
__device__ __forceinline__ void epilogue8_pre(float (&v)[8], const GemmArgs& p, int flags, int m, int n, const f32x4& b0,
                                              const f32x4& b1, const SideOps& s) {
  epilogue_chain<8>(v, p, flags, m, n, [&] { return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7); },
                    [&] { return s.aux; }, [&] { return s.res; });
}

// ---------------------------------------------------------------- host side: what every launcher does
// The epilogues (flags & epi_bits::MASK) that are compiled with constant flags are listed as types: a launcher asks its
// kernel's list whether there is an instance (has) and launches it through the same list (epi_dispatch), so the two cannot
// disagree.
template <int... E>
struct EpiList {
  static constexpr bool has(int epi) { return ((epi == E) || ...); }
};
// Epilogue bits by their short names, and the lists of compiled instances in them.
namespace epi_bits {
constexpr int B = STONK_EPI_BIAS, G = STONK_EPI_GELU, SV = STONK_EPI_SAVE_PREACT, GB = STONK_EPI_GELU_BWD,
              R = STONK_EPI_RESID, D = STONK_EPI_DROPOUT, AG = STONK_EPI_AUX_GRAD;
constexpr int MASK = B | G | SV | GB | R | D | AG;   // = 0x1FC: flags & MASK == 0 is the plain product
// the eight of the training step that every bf16 NT kernel has an instance of, and what a kernel has besides them
template <int... MORE>
using EpisCommon = EpiList<0, B, B | G | SV, GB, B | G | SV | AG, GB | AG, R, B | R, MORE...>;
using EpisStep = EpisCommon<B | G, B | R | D>;   // the step's ten: gemm_w4.hip, gemm_a4.hip
using EpisTile128 = EpisCommon<B | R | D>;       // gemm_bf16.hip
using EpisWave8 = EpisCommon<B | G>;             // gemm256.hip (bias + dropout + residual would spill there)
// the four-wave kernels' 256 x 192 tiles exist for the epilogues of the N = 768 launches
using Epis192 = EpiList<0, B, R, B | R, B | R | D>;
}  // namespace epi_bits

// f(std::integral_constant<int, epi>) for the member of the list that equals the run-time `epi`; `fallback` if there is none
template <int... E, typename F>
int epi_dispatch(EpiList<E...>, int epi, int fallback, F&& f) {
  int rc = fallback;
  (void)((epi == E && ((rc = f(std::integral_constant<int, E>{})), true)) || ...);
  return rc;
}

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

// The four-wave kernels' 256 x (256 | 192) tiles (gemm_w4.hip, gemm_a4.hip): where there is a 192-wide instance (has192:
// Epis192, N % 192 == 0) it is chosen (tile_n == 0 on entry) where it quantises better: time ~ rounds of the CUs x tile width (N = 768 at
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

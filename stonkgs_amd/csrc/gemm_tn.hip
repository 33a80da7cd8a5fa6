// Weight-gradient GEMM straight from row-major activations ("TN" form), bf16 MFMA, fp32 atomic accumulate:
//
//     dW[M', N'] += alpha * sum_t dY[t][m'] * X[t][n']          db[m'] += alpha * sum_t dY[t][m']
//
// dY = [T, M'] and X = [T, N'] are the tensors backward already holds ([token][feature], feature-contiguous); the
// contraction runs over the token index, i.e. over the ROW index of both operands. Instead of materialising dY^T and
// X^T for the NT kernel (two extra HBM passes per weight), the [64 tokens][128 features] tiles are DMA'd as they lie
// and the MFMA fragments (8 consecutive tokens of one feature per lane) are gathered by the hardware transpose read
// ds_read_b64_tr_b16 (two per fragment). Autograd's mm for nn.Linear weights/biases
// (hf:models/bert/modeling_bert.py:154-156,289,335,348,477; ref:stonkgs_model.py:70-71).
//
// Bias gradient for free: workgroups of the first column tile issue one extra MFMA per (feature tile, k-step) against
// an all-ones B fragment - column sums of dY on the matrix pipe, no second pass over dY.
//
// Tile 128x128 over 64-token K steps, 4 waves (2x2), 2 workgroups per CU, LDS-DMA double buffered as gemm_bf16.hip.
// LDS image: 256-byte rows (128 features), 16-byte chunk c of row r stored at c ^ (((r&3)<<2) | ((r>>2)&3))
// (conflict-free for the transposed reads); the swizzle is applied on the DMA source address.
#include <cstdlib>

#include "gemm_common.h"
#include "stonk_hip.h"   // (StonkTnProblem)

// persistent 256x256 variant (gemm256.hip, TN = true)
int stonk_gemm256_tn_launch(const stonk_gemm::GemmArgs& a, hipStream_t st);
int stonk_gemm_tn_a4_launch(const stonk_gemm::GemmArgs& a, hipStream_t st);
int stonk_gemm_tn_a4_store_launch(const stonk_gemm::GemmArgs& a, hipStream_t st);   // gemm_tn_a4_store.hip
int stonk_gemm_tn_a4_store_sumsq_launch(const stonk_gemm::GemmArgs& a, hipStream_t st);   // gemm_tn_a4_store_sumsq.hip (a.aux = the slots)
int stonk_gemm_tn_a4_group_launch(const stonk_gemm::TnGroupArgs& g, int grid, hipStream_t st);   // gemm_tn_a4_group.hip

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BK * 256;          // 16 KiB: 64 token rows x 128 features
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int TN_LDS = 2 * STAGE_BYTES;       // 64 KiB

using stonk_gemm::live_count;
using stonk_gemm::tile_split;
using stonk_gemm::xcd_remap;

struct TnArgs {
  const bf16* A;   // dY [T, M']
  const bf16* B;   // X  [T, N']
  float* C;        // dW [M', N'] fp32, accumulated
  float* bias;     // db [M'] fp32, accumulated (nullable)
  const int* k_dev;
  long lda, ldb, ldc;
  int M, N, K;     // M', N', token count (capacity)
  float alpha;
  int split_k;
  float* tile_sumsq;   // (gemm_tn_store_sumsq_kernel only) one slot per output tile, row_tile * col_tiles + col_tile
};

__device__ __forceinline__ int row_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// STORE: the launch has ONE K split, so every output element has exactly one producer - the epilogue writes acc * alpha
// (and the bias sums) with plain stores instead of adding them into a zeroed buffer, and a launch whose device-side token
// count leaves no K tile still defines every element (zeros).
// SUMSQ (with STORE): the workgroup also leaves the sum of the squares of the 128 x 128 values it stored in its tile's slot, in
// a fixed order - a lane's values in epilogue order (a tree per 16-row block, the blocks one after the other), the wave
// butterfly, the four waves in index order - so that the gradient-norm pass need not read them back. The accumulator is
// born after the K loop.
template <bool STORE, bool SUMSQ>
__device__ __forceinline__ void gemm_tn_body(const TnArgs& p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  const int K = live_count(p.k_dev, p.K);
  const int nk_total = (K + BK - 1) / BK;   // rows in [K, roundup) must read as zero (caller guarantees)
  const int ntm = p.M / BM, ntn = p.N / BN;
  const int nk_per = (nk_total + p.split_k - 1) / p.split_k;
  const int per_split = ntm * ntn;
  const int total = per_split * p.split_k;
  const int t = ((int)gridDim.x == total) ? xcd_remap(blockIdx.x, total) : blockIdx.x;
  const int ks = t / per_split;
  const int tt = t - ks * per_split;
  const stonk_gemm::TileRC rc = tile_split(tt, ntm, ntn);
  const int rt = rc.rt, ct = rc.ct;
  const int m0 = rt * BM, n0 = ct * BN;
  int nk = nk_total - ks * nk_per;
  nk = nk < nk_per ? nk : nk_per;
  if (!STORE && nk <= 0) return;
  const long tok_begin = (long)ks * nk_per * BK;
  const bool want_bias = p.bias != nullptr && ct == 0;

  // ---- DMA sources: a wave moves 16 token rows of each operand per K step (4 + 4 pieces of 4 rows x 256 B)
  const bf16* ga[4];
  const bf16* gb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 4 + (lane >> 4);     // token row inside the K step
    const int c = (lane & 15) ^ row_swz(r);             // logical chunk for physical slot (lane & 15)
    ga[i] = p.A + (tok_begin + r) * p.lda + m0 + c * 8;
    gb[i] = p.B + (tok_begin + r) * p.ldb + n0 + c * 8;
  }
  auto stage = [&](int kt, int buf) {
    char* sa = smem + buf * STAGE_BYTES + wave * 4096;
    char* sb = sa + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ga[i] + (long)kt * BK * p.lda),
                                       (__attribute__((address_space(3))) void*)(sa + i * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gb[i] + (long)kt * BK * p.ldb),
                                       (__attribute__((address_space(3))) void*)(sb + i * 1024), 16, 0, 0);
    }
  };

  // ---- transposed fragment offsets: lane (group g = lane>>4, q = (lane&15)>>2, pq = lane&3) addresses token row
  // 8g + 4*hi + q, features f0 + 4*pq .. +3 of the 16-feature tile; it receives feature f0 + (lane&15), 4 tokens.
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
  int offa[2][4], offb[2][4];
#pragma unroll
  for (int hi = 0; hi < 2; ++hi) {
    const int row = 8 * g + 4 * hi + q;                 // + 32 per k-step: swizzle unchanged (32 = 0 mod 16 rows)
    const int sw = row_swz(row);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ca = wm * 64 + i * 16 + 4 * pq, cb = wn * 64 + i * 16 + 4 * pq;
      offa[hi][i] = row * 256 + (((ca >> 3) ^ sw) << 4) + ((ca & 7) << 1);
      offb[hi][i] = row * 256 + (((cb >> 3) ^ sw) << 4) + ((cb & 7) << 1);
    }
  }

  f32x4 acc[4][4], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.0f;

  auto compute = [&](int buf) {
    const char* sa = smem + buf * STAGE_BYTES;
    const char* sb = sa + TILE_BYTES;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x4 alo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sa + s * 8192 + offa[0][i]));
        const bf16x4 ahi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sa + s * 8192 + offa[1][i]));
        a[i] = (bf16x8){alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
        const bf16x4 blo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sb + s * 8192 + offb[0][i]));
        const bf16x4 bhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(sb + s * 8192 + offb[1][i]));
        b[i] = (bf16x8){blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        if (want_bias && wn == 0) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], ones, accb[i], 0, 0, 0);
      }
    }
  };

  if (!STORE || nk > 0) stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
    compute(kt & 1);
  }

  // ---- epilogue: acc[i][j][r] = dW[m0 + wm*64 + i*16 + (lane>>4)*4 + r][n0 + wn*64 + j*16 + (lane&15)]
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float sq[4][4];   // (SUMSQ: added up as a tree per 16-row block, the four blocks one after the other)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + (lane & 15);
        if constexpr (STORE) p.C[(long)m * p.ldc + n] = acc[i][j][r] * p.alpha;
        else atomicAdd(p.C + (long)m * p.ldc + n, acc[i][j][r] * p.alpha);
        if constexpr (SUMSQ) {
          const float v = acc[i][j][r] * p.alpha;
          sq[r][j] = v * v;
        }
      }
      if (want_bias && wn == 0 && (lane & 15) == 0) {
        if constexpr (STORE) p.bias[m] = accb[i][r] * p.alpha;
        else atomicAdd(p.bias + m, accb[i][r] * p.alpha);
      }
    }
    if constexpr (SUMSQ) {
      float sr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sr[r] = (sq[r][0] + sq[r][1]) + (sq[r][2] + sq[r][3]);
      ss += (sr[0] + sr[1]) + (sr[2] + sr[3]);
    }
  }
  if constexpr (SUMSQ) {
    float* part = (float*)smem;   // (the operand images are dead once every wave is past its last K step)
    ss = wave_sum(ss);
    __syncthreads();
    if (lane == 0) part[wave] = ss;
    __syncthreads();
    if (tid == 0) p.tile_sumsq[rt * ntn + ct] = ((part[0] + part[1]) + part[2]) + part[3];
  }
}

template <bool STORE>
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(const TnArgs p) {
  gemm_tn_body<STORE, false>(p);
}
__global__ __launch_bounds__(256, 2) void gemm_tn_store_sumsq_kernel(const TnArgs p) { gemm_tn_body<true, true>(p); }

}  // namespace

// shared body of stonk_gemm_tn_bf16 (atomic accumulate) and stonk_gemm_tn_bf16_store (one K split, plain stores)
// Output tiles of the kernel a store launch is routed to (256 x 256 for split_k <= 0, else 128 x 128)
static long gemm_tn_store_tiles(int M, int N, int split_k) {
  return split_k <= 0 ? (long)((M + 255) / 256) * ((N + 255) / 256) : (long)(M / BM) * (N / BN);
}

// What the 256x256 kernels ask of a shape beyond the common checks (split_k <= 0 and the grouped entry)
static int tn_a4_shape_status(int64_t lda, int64_t ldb, int64_t ldc, int M, int N) {
  STONK_CHECK_ARG(M >= 256 && N >= 256, STONK_ESHAPE);
  // (operands are addressed per 64-token K tile: 64 rows of either operand must stay inside 32-bit byte offsets)
  STONK_CHECK_ARG(lda % 64 == 0 && ldb % 64 == 0 && lda < (1L << 23) && ldb < (1L << 23), STONK_ESHAPE);
  // (the four-wave kernel addresses dW through a buffer resource: a byte range of M * ldc * 4, 32-bit byte offsets, and a
  // column past N' pushed out of that range - a row stride below N' would let it land in the next row instead)
  STONK_CHECK_ARG(ldc >= N && (long)M * ldc * 4 < (1L << 31), STONK_ESHAPE);
  return STONK_OK;
}

// `tile_sumsq` (store only, nullable): n_slots floats for the per-tile sums of squares - the launch then takes the kernels
// that leave them
static int gemm_tn_route(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW, int64_t ldc, float* dbias,
                         int M, int N, int K, float alpha, int split_k, const int* k_dev, void* stream, bool store,
                         float* tile_sumsq = nullptr, int64_t n_slots = 0, bool dry = false) {
  STONK_CHECK_ARG(dY && X && dW, STONK_EINVAL);
  STONK_CHECK_ARG(M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0, STONK_ESHAPE);
  STONK_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)dY % 16 == 0 && (uintptr_t)X % 16 == 0, STONK_EALIGN);
  if (store) {
    // (the 256x256 kernel addresses dW through a buffer resource with 32-bit byte offsets and a byte range of M * ldc * 4)
    STONK_CHECK_ARG(ldc >= N && (long)M * ldc * 4 < (1L << 31), STONK_ESHAPE);
    STONK_CHECK_ARG((uintptr_t)dW % 4 == 0 && (uintptr_t)dbias % 4 == 0, STONK_EALIGN);
  }
  // split_k <= 0: the 256x256 kernels with an automatic split, work items = tiles x splits aimed at one full round of the
  // CUs. 0 (and -2 .. -15): the written-out four-wave kernel (gemm_tn_a4.hip) on all CUs. -16 .. -1024: the same kernel
  // limited to -split_k CUs' worth of workgroups - for launches that run on a second stream beside other work: a persistent
  // one-workgroup-per-CU kernel that takes every CU stalls the other stream until its workgroups retire (the step is 1.5 ms
  // faster with the weight gradients on 160 of the 256 CUs). -1: the older eight-wave 256x256 TN form of gemm256.hip.
  if (split_k <= 0) {
    if (const int rc = tn_a4_shape_status(lda, ldb, ldc, M, N)) return rc;
    STONK_CHECK_ARG(split_k >= -1024, STONK_ESHAPE);
    stonk_gemm::GemmArgs g = {};
    g.A = (const bf16*)dY; g.B = (const bf16*)X; g.C = dW; g.bias = dbias; g.k_dev = k_dev;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.alpha = alpha;
    const int nk = (K + BK - 1) / BK;
    const long tiles = (long)((M + 255) / 256) * ((N + 255) / 256);
    const long cus = split_k <= -16 ? -split_k : 256;
    long sk = tiles >= cus ? 1 : cus / tiles;   // floor: tiles x splits must not spill into a second, mostly empty round
    if (sk > nk / 8) sk = nk / 8 > 0 ? nk / 8 : 1;
    g.split_k = (int)sk;
    g.flags = (int)cus;   // grid cap
    if (store) {
      STONK_CHECK_ARG(sk == 1 && split_k != -1, STONK_ESHAPE);
      // (this kernel shares the bias sums out over the column tiles: one producer per element only with a single one)
      STONK_CHECK_ARG(!dbias || N <= 256, STONK_ESHAPE);
      if (dry) return STONK_OK;
      if (!tile_sumsq) return stonk_gemm_tn_a4_store_launch(g, (hipStream_t)stream);
      STONK_CHECK_ARG(n_slots >= gemm_tn_store_tiles(M, N, split_k), STONK_EINVAL);
      g.aux = (bf16*)tile_sumsq;
      return stonk_gemm_tn_a4_store_sumsq_launch(g, (hipStream_t)stream);
    }
    return split_k == -1 ? stonk_gemm256_tn_launch(g, (hipStream_t)stream) : stonk_gemm_tn_a4_launch(g, (hipStream_t)stream);
  }
  TnArgs a;
  a.A = (const bf16*)dY; a.B = (const bf16*)X; a.C = dW; a.bias = dbias; a.k_dev = k_dev;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.alpha = alpha;
  const int nk = (K + BK - 1) / BK;
  a.split_k = split_k < nk ? split_k : nk;
  const long tiles = (long)(M / BM) * (N / BN) * a.split_k;
  a.tile_sumsq = tile_sumsq;
  if (store) {
    STONK_CHECK_ARG(a.split_k == 1, STONK_ESHAPE);
    if (dry) return STONK_OK;
    if (!tile_sumsq) return stonk_gemm::launch_with_lds<gemm_tn_kernel<true>, TN_LDS>(a, (int)tiles, 256, (hipStream_t)stream);
    STONK_CHECK_ARG(n_slots >= tiles, STONK_EINVAL);
    return stonk_gemm::launch_with_lds<gemm_tn_store_sumsq_kernel, TN_LDS>(a, (int)tiles, 256, (hipStream_t)stream);
  }
  return stonk_gemm::launch_with_lds<gemm_tn_kernel<false>, TN_LDS>(a, (int)tiles, 256, (hipStream_t)stream);
}

extern "C" int stonk_gemm_tn_bf16(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW, int64_t ldc,
                                  float* dbias, int M, int N, int K, float alpha, int split_k, const int* k_dev,
                                  void* stream) {
  return gemm_tn_route(dY, lda, X, ldb, dW, ldc, dbias, M, N, K, alpha, split_k, k_dev, stream, false);
}

// Up to four accumulating launches of the four-wave kernel as ONE (gemm_tn_a4_group.hip): weight gradients whose operands
// are ready at about the same time share the CU share, so each needs fewer K splits to fill it - fewer float atomics per
// output element, fewer K-loop prologues, one launch. One common split: the largest sk with sum(tiles) * sk <= cap and
// sk <= K tiles / 8 of every problem (the single launches' rule), applied to each problem's own K, so that the workgroups
// of a launch finish together. One work item per workgroup: a group that does not fit the cap unsplit is refused
// (STONK_ESHAPE) and the caller launches its members one by one.
extern "C" int stonk_gemm_tn_bf16_group(const StonkTnProblem* problems, int n, int cu_cap, void* stream) {
  using stonk_gemm::TnGroupArgs;
  STONK_CHECK_ARG(problems && n > 0 && cu_cap >= 0, STONK_EINVAL);
  STONK_CHECK_ARG(n <= TnGroupArgs::MAX && cu_cap <= 1024, STONK_ESHAPE);
  TnGroupArgs g = {};
  long tiles_all = 0, sk = 1L << 30;
  for (int i = 0; i < n; ++i) {
    const StonkTnProblem& q = problems[i];
    STONK_CHECK_ARG(q.dY && q.X && q.dW, STONK_EINVAL);
    STONK_CHECK_ARG(q.M > 0 && q.N > 0 && q.K > 0 && q.M % 256 == 0 && q.N % 256 == 0, STONK_ESHAPE);
    STONK_CHECK_ARG(q.lda % 8 == 0 && q.ldb % 8 == 0, STONK_EALIGN);
    STONK_CHECK_ARG((uintptr_t)q.dY % 16 == 0 && (uintptr_t)q.X % 16 == 0, STONK_EALIGN);
    STONK_CHECK_ARG((uintptr_t)q.dW % 4 == 0 && (uintptr_t)q.dbias % 4 == 0, STONK_EALIGN);
    if (const int rc = tn_a4_shape_status(q.lda, q.ldb, q.ldc, q.M, q.N)) return rc;
    stonk_gemm::GemmArgs& a = g.prob[i];
    a.A = (const bf16*)q.dY; a.B = (const bf16*)q.X; a.C = q.dW; a.bias = q.dbias; a.k_dev = q.k_dev;
    a.lda = q.lda; a.ldb = q.ldb; a.ldc = q.ldc; a.M = q.M; a.N = q.N; a.K = q.K; a.alpha = q.alpha;
    tiles_all += (long)(q.M / 256) * (q.N / 256);
    const long by_k = ((q.K + BK - 1) / BK) / 8;
    sk = by_k < sk ? by_k : sk;
  }
  long cap = cu_cap;
  if (cap == 0) {   // (a cap from the caller needs no device: more workgroups than CUs are late, not wrong)
    cap = stonk_gemm::cu_count();
    if (cap <= 0) return (int)hipGetLastError();
  }
  STONK_CHECK_ARG(tiles_all <= cap, STONK_ESHAPE);
  sk = sk < cap / tiles_all ? sk : cap / tiles_all;
  sk = sk > 0 ? sk : 1;
  int at = 0;
  for (int i = 0; i < n; ++i) {
    g.prob[i].split_k = (int)sk;
    g.items[i] = (int)((long)(g.prob[i].M / 256) * (g.prob[i].N / 256) * sk);
    g.first[i] = at;
    at += i + 1 < n ? (g.items[i] + 7) & ~7 : g.items[i];   // (the next problem starts on a multiple of 8: XCD 0)
  }
  g.n = n;
  return stonk_gemm_tn_a4_group_launch(g, at, (hipStream_t)stream);
}

// dW = alpha * dY^T . X, db = alpha * colsum(dY): the same kernels with a store epilogue. Only for a launch the routing
// above leaves UNSPLIT (split_k == 1, or an automatic split that comes out as 1): anything else is refused with
// STONK_ESHAPE and the caller accumulates with stonk_gemm_tn_bf16 into a zeroed buffer as before.
extern "C" int stonk_gemm_tn_bf16_store(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW, int64_t ldc,
                                        float* dbias, int M, int N, int K, float alpha, int split_k, const int* k_dev,
                                        void* stream) {
  return gemm_tn_route(dY, lda, X, ldb, dW, ldc, dbias, M, N, K, alpha, split_k, k_dev, stream, true);
}

// stonk_gemm_tn_bf16_store that also writes, for every output tile of the kernel it routes to (256 x 256 for split_k <= 0,
// else 128 x 128), the sum of the squares of the values it stored: tile_sumsq[row_tile * col_tiles + col_tile]. Every slot is
// written by every launch (zeros when the device-side token count leaves no K tile), in a fixed order of summation.
extern "C" int stonk_gemm_tn_bf16_store_sumsq(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW,
                                              int64_t ldc, float* dbias, int M, int N, int K, float alpha, int split_k,
                                              const int* k_dev, float* tile_sumsq, int64_t n_slots, void* stream) {
  STONK_CHECK_ARG(tile_sumsq && n_slots >= 0, STONK_EINVAL);
  STONK_CHECK_ARG((uintptr_t)tile_sumsq % 4 == 0, STONK_EALIGN);
  return gemm_tn_route(dY, lda, X, ldb, dW, ldc, dbias, M, N, K, alpha, split_k, k_dev, stream, true, tile_sumsq, n_slots);
}

// Slots a stonk_gemm_tn_bf16_store_sumsq launch of this shape writes, or the (negative) status with which the store entry
// refuses the shape. Nothing is launched; operands are taken as present, aligned and dense (lda = M, ldb = ldc = N).
extern "C" int64_t stonk_gemm_tn_store_tiles(int M, int N, int K, int split_k) {
  static const int dummy = 0;   // (any aligned non-null address: a dry run reads nothing)
  const void* q = (const void*)(((uintptr_t)&dummy + 4096) & ~(uintptr_t)15);
  const int rc = gemm_tn_route(q, M, q, N, (float*)q, N, nullptr, M, N, K, 1.f, split_k, nullptr, nullptr, true, nullptr, 0, true);
  return rc != STONK_OK ? rc : gemm_tn_store_tiles(M, N, split_k);
}

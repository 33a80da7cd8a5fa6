// Weight gradient on the written-out four-wave loop (gemm_a4.hip's pipeline; the K loop is generated text,
// tools/gen_gemm_a4.py -> gemm_a4_loop.inc, STONK_TN_A4_*):
//   C[M', N'] (fp32) += alpha * sum_t A[t][m] * B[t][n]        A = dY [T, M'], B = X [T, N'], both row-major by token
//   bias[m]          += alpha * sum_t A[t][m]
// stonk_gemm_tn_bf16 with split_k == 0 / <= -16 lands here (gemm_tn.hip has the contract).
//
// What carries over from the NT kernel: 256 x 256 tiles, four waves (one per SIMD, 128 x 128 wave tiles),
// v_mfma_f32_16x16x32_bf16 into a[0:255], operands by LDS-DMA two K tiles ahead and across work items, two barriers per
// K tile, every wait "all but this K tile's own pieces". What is specific to the contraction running over ROWS:
//  * a K tile = 64 tokens x 512 B per operand; a 1-KiB piece = two token rows = eight full 128-byte lines; rows sit 512 B
//    apart in LDS (every row on the same banks), so the sixteen 32-byte feature-block segments of a row are XOR-permuted by
//    f(row) = (row & 3) | ((row >> 3) & 1) << 2 - applied to the SOURCE address, the image stays lane-linear;
//  * fragments by ds_read_b64_tr_b16 pairs (4 token rows x 16 features per 16-lane group): the half-wave's eight rows fall
//    into eight different 32-byte bank slots; one per-lane address per feature block, the rest immediates;
//  * srcA = the dY fragment, so a lane holds one output COLUMN: after one v_permlane16_swap per register pair a register
//    covers two rows x 32 consecutive columns = two 128-byte segments, the shape float atomics run at full rate with - no
//    LDS slab;
//  * bias gradient: one extra MFMA per dY block against an all-ones operand on every ntn-th K tile, into VGPR accumulators;
//  * tokens past the (device-side) count are out of the buffers' range and arrive as zeros; the cursors carry 64-bit
//    byte counts (the entity decoder's dlogits are 5.7 GB).
//
// STONK_TN_A4_STORE = 1 (gemm_tn_a4_store.hip includes this file with it): the same kernel for launches with ONE K split,
// where every output element has exactly one producer. The epilogue stores acc * alpha in the same two-rows x 128-byte
// shape instead of adding it into a zeroed buffer, the bias sums are stored too (the launcher admits a bias only with ONE
// column tile, where the bias duty below puts every K tile on that tile), and a device-side token count that leaves no K
// tile makes every work item store zeros.
//
// STONK_TN_A4_STORE = 2 (gemm_tn_a4_store_sumsq.hip): the store kernel that also leaves, per output tile, the sum of the
// squares of what it stored (slot row_tile * col_tiles + col_tile of `aux`, here a float array): the gradient-norm pass
// need not read these values back. The order of the sum is fixed - a lane's values in epilogue order (a tree over the 32
// values of a row block, the eight blocks one after the other), the wave butterfly, the four waves in index order - so a
// slot is a function of the inputs alone, whatever the grid. The accumulator is born after the K loop (one VGPR of the
// epilogue); the waves meet at one raw barrier per tile behind an LDS word each (16 bytes past the operand images), with
// no wait for the stores or the next item's operand loads in flight.
//
// STONK_TN_A4_GROUP = 1 (gemm_tn_a4_group.hip): the accumulating kernel for up to four problems in ONE launch
// (stonk_gemm_tn_bf16_group). The argument block is a table of problems; a workgroup finds the problem its block index
// falls into and is, from there on, workgroup `bid` of a launch of that problem alone on a grid of that problem's own
// work items (tiles x the common K split): the same tile_split, XCD runs, even K-tile counts and bias duty. One work item
// per workgroup - the launcher refuses anything else - so no workgroup walks from one problem into another (the K loop
// prefetches the next item's first K tiles with THIS item's leading dimensions).
#include "gemm_common.h"
#ifndef STONK_TN_A4_STORE
#define STONK_TN_A4_STORE 0
#endif
#ifndef STONK_TN_A4_GROUP
#define STONK_TN_A4_GROUP 0
#endif
#if STONK_TN_A4_GROUP
#define STONK_TN_A4_KERNEL gemm_tn_a4_group_kernel
#define STONK_TN_A4_LAUNCH stonk_gemm_tn_a4_group_launch
#elif STONK_TN_A4_STORE == 2
#define STONK_TN_A4_KERNEL gemm_tn_a4_store_sumsq_kernel
#define STONK_TN_A4_LAUNCH stonk_gemm_tn_a4_store_sumsq_launch
#elif STONK_TN_A4_STORE
#define STONK_TN_A4_KERNEL gemm_tn_a4_store_kernel
#define STONK_TN_A4_LAUNCH stonk_gemm_tn_a4_store_launch
#else
#define STONK_TN_A4_KERNEL gemm_tn_a4_kernel
#define STONK_TN_A4_LAUNCH stonk_gemm_tn_a4_launch
#endif
#ifndef STONK_A4_LOOP_INC
#define STONK_A4_LOOP_INC "gemm_a4_loop.inc"
#endif
#include STONK_A4_LOOP_INC

using namespace stonk_gemm;

namespace {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int IMG_BYTES = BK * 512;            // one operand of one K tile: 64 token rows x 512 B = 32 KiB
constexpr int IMG_LDS = 4 * IMG_BYTES;         // two stages x (A image + B image)
constexpr int LDS_BYTES = IMG_LDS + (STONK_TN_A4_STORE == 2 ? 16 : 0);   // (+ the four waves' partial sums of squares)

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct Cursor {     // where an operand stream stands: buffer words + bytes left from the base to the end of the live tokens
  i32x4 srd;
  int rem_lo, rem_hi;
};

#if STONK_TN_A4_GROUP
__global__ __launch_bounds__(256, 1) void STONK_TN_A4_KERNEL(const TnGroupArgs g) {
  // (first[] ascends; block indices between a problem's last item and the next problem's first are padding: the launcher
  // starts every problem on a multiple of 8, so that block index and `bid` name the same XCD)
  int pi = 0;
#pragma unroll
  for (int i = 1; i < TnGroupArgs::MAX; ++i) pi = (i < g.n && (int)blockIdx.x >= g.first[i]) ? i : pi;
  const GemmArgs& p = g.prob[pi];
  const int bid = (int)blockIdx.x - g.first[pi];
  const int G = g.items[pi];
  if (bid >= G) return;
#define STONK_TN_A4_BID bid
#else
__global__ __launch_bounds__(256, 1) void STONK_TN_A4_KERNEL(const GemmArgs p) {
#define STONK_TN_A4_BID blockIdx.x
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  const int M = p.M, N = p.N;
  const int Kact = live_count(p.k_dev, p.K);
  const int ntm = (M + BM - 1) / BM, ntn = (N + BN - 1) / BN;
  const int nk_total = (Kact + BK - 1) / BK;
  int nk_per = (nk_total + p.split_k - 1) / p.split_k;
  nk_per += nk_per & 1;
  const int per_split = ntm * ntn;
  const int total = per_split * p.split_k;
#if !STONK_TN_A4_GROUP
  const int G = gridDim.x;
#endif
#if STONK_TN_A4_STORE
  if (nk_total == 0) {   // (one K split: every work item is empty) each output tile is defined as zeros, row by row
    const int ldc0 = (int)p.ldc;
    for (int w = blockIdx.x; w < total; w += G) {
      const int rt = ntm >= ntn ? w / ntn : w % ntm, ct = ntm >= ntn ? w % ntn : w / ntm;
      const int n = ct * BN + tid;
      for (int r = 0; r < BM; ++r) {
        const int m = rt * BM + r;
        if (m < M && n < N) ((float*)p.C)[(long)m * ldc0 + n] = 0.f;
      }
      if (p.bias && ct == 0 && rt * BM + tid < M) ((float*)p.bias)[rt * BM + tid] = 0.f;
#if STONK_TN_A4_STORE == 2
      if (tid == 0) ((float*)p.aux)[rt * ntn + ct] = 0.f;
#endif
    }
    return;
  }
#endif

  auto get_work = [&](int w, Work& o) -> bool {
    if (w >= total) return false;
    int idx = w;
    {   // any grid size: the workgroups of one XCD (blockIdx & 7) take one contiguous run of items per round
      const int r = w / G, b = w - r * G;
      const int x = b & 7, base = G >> 3, rem = G & 7;
      const int cand = r * G + x * base + (x < rem ? x : rem) + (b >> 3);
      if ((r + 1) * G <= total) idx = cand;
    }
    const int ks = idx / per_split;
    const int tt = idx - ks * per_split;
    const TileRC t = tile_split(tt, ntm, ntn);
    o.m0 = t.rt * BM;
    o.n0 = t.ct * BN;
    o.k_begin = (long)ks * nk_per * BK;
    int nk = nk_total - ks * nk_per;
    nk = nk < nk_per ? nk : nk_per;
    o.nk = nk <= 0 ? 0 : nk + (nk & 1);   // (even; tokens past the end read as zeros)
    return true;
  };

  // ---- LDS-DMA sources: piece q of this wave = token rows 16 wave + 2 q, + 1 of the K tile (two rows x 512 B); a lane moves
  // 16 bytes: row lane >> 5, PHYSICAL 16-byte chunk lane & 31 of the image row = 32-byte segment (lane & 31) >> 1, i.e.
  // LOGICAL segment ((lane & 31) >> 1) ^ f(row)
  const int lda2 = (int)p.lda * 2, ldb2 = (int)p.ldb * 2;
  int voffA[8], voffB[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = 16 * wave + 2 * q + (lane >> 5);
    const int f = (row & 3) | (((row >> 3) & 1) << 2);
    const int c = (((((lane & 31) >> 1) ^ f) << 1) | (lane & 1)) << 4;
    voffA[q] = row * lda2 + c;
    voffB[q] = row * ldb2 + c;
  }
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int m0a = (int)lds0 + wave * 8192;
  const int m0b = (int)lds0 + 2 * IMG_BYTES + wave * 8192;
  // ---- transposed fragment reads: lane (g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3) addresses token row
  // 32 h + 8 g + 4 hi + q, features 4 pq .. + 3 of the 16-feature block; it receives feature lane & 15, four tokens
  int taA[8], taB[8];
  {
    const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
    const int f = q | ((g & 1) << 2);
    const int rowb = (8 * g + q) * 512 + pq * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      taA[i] = (int)lds0 + rowb + ((8 * wr + (i ^ f)) << 5);
      taB[i] = (int)lds0 + 2 * IMG_BYTES + rowb + ((8 * wc + (i ^ f)) << 5);
    }
  }
  const u32x4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};   // eight bf16 ones

  auto cursor_of = [&](const Work& w, Cursor& a, Cursor& b) {
    const unsigned long pa = (unsigned long)p.A + (unsigned long)((w.k_begin * p.lda + w.m0) * 2);
    const unsigned long pb = (unsigned long)p.B + (unsigned long)((w.k_begin * p.ldb + w.n0) * 2);
    const long ra = ((long)Kact - w.k_begin) * lda2 - (long)w.m0 * 2, rb = ((long)Kact - w.k_begin) * ldb2 - (long)w.n0 * 2;
    auto clamp = [](long r) -> int { return (int)(unsigned)(r < 0 ? 0 : (r > 0xFFFFF000L ? 0xFFFFF000L : r)); };
    a.srd = (i32x4){(int)(unsigned)pa, (int)((pa >> 32) & 0xffff), clamp(ra), 0x00020000};
    b.srd = (i32x4){(int)(unsigned)pb, (int)((pb >> 32) & 0xffff), clamp(rb), 0x00020000};
    a.rem_lo = (int)(unsigned)ra;
    a.rem_hi = (int)(ra >> 32);
    b.rem_lo = (int)(unsigned)rb;
    b.rem_hi = (int)(rb >> 32);
  };

  Work cw, nw;
  int cwi = STONK_TN_A4_BID;
  if (!get_work(cwi, cw)) return;
  if (cw.nk <= 0 && !next_live_work(get_work, cwi, G, cw)) return;   // (k_dev may leave a K split empty)
  Cursor ca, cb;
  cursor_of(cw, ca, cb);
  const int stepa = BK * lda2, stepb = BK * ldb2;

#define STONK_TN_A4_DMA_OPERANDS \
  STONK_A4_VOFF_IN(voffA, voffB), [m0a] "s"(m0a), [m0b] "s"(m0b), [stepa] "s"(stepa), [stepb] "s"(stepb)

  // K tiles 0 and 1 of the first work item
  asm volatile(STONK_TN_A4_PROLOGUE
               : "+{s[36:39]}"(ca.srd), "+{s[40:43]}"(cb.srd), [ralo] "+s"(ca.rem_lo), [rahi] "+s"(ca.rem_hi),
                 [rblo] "+s"(cb.rem_lo), [rbhi] "+s"(cb.rem_hi)
               : STONK_TN_A4_DMA_OPERANDS
               : "m0", "scc", "s48", "memory");

  const bool want_bias = p.bias != nullptr;
  const int r16 = lane & 15, qq = lane >> 4;

  for (;;) {
    int nwi = cwi;
    const bool more = next_live_work(get_work, nwi, G, nw);
    Cursor na, nb;
    cursor_of(more ? nw : cw, na, nb);   // (no next item: the cursor re-reads this item's first K tiles, never consumed)
    f32x16 acc[16];
    f32x4 bacc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int rem = cw.nk >> 1;
    // bias duty: column tile ct sums dY over the K tiles kt = ct (mod ntn) of its items (every workgroup carries 1/ntn of it)
    const int ct = cw.n0 / BN;
    const int kt0 = (int)(cw.k_begin / BK);
    int bph = want_bias ? ((kt0 - ct) % ntn + ntn) % ntn : 1;
    const int ntn_s = want_bias ? ntn : 0x7fffffff;   // (without a bias the phase never returns to 0)
    asm volatile(STONK_TN_A4_TILE
                 : STONK_A4_ACC_OUT_16(acc),
                   "+{s[36:39]}"(ca.srd), "+{s[40:43]}"(cb.srd), [ralo] "+s"(ca.rem_lo), [rahi] "+s"(ca.rem_hi),
                   [rblo] "+s"(cb.rem_lo), [rbhi] "+s"(cb.rem_hi), [rem] "+s"(rem), [bph] "+s"(bph),
                   [bacc0] "+v"(bacc[0]), [bacc1] "+v"(bacc[1]), [bacc2] "+v"(bacc[2]), [bacc3] "+v"(bacc[3]),
                   [bacc4] "+v"(bacc[4]), [bacc5] "+v"(bacc[5]), [bacc6] "+v"(bacc[6]), [bacc7] "+v"(bacc[7])
                 : STONK_TN_A4_DMA_OPERANDS, [taA0] "v"(taA[0]), [taA1] "v"(taA[1]), [taA2] "v"(taA[2]), [taA3] "v"(taA[3]),
                   [taA4] "v"(taA[4]), [taA5] "v"(taA[5]), [taA6] "v"(taA[6]), [taA7] "v"(taA[7]), [taB0] "v"(taB[0]),
                   [taB1] "v"(taB[1]), [taB2] "v"(taB[2]), [taB3] "v"(taB[3]), [taB4] "v"(taB[4]), [taB5] "v"(taB[5]),
                   [taB6] "v"(taB[6]), [taB7] "v"(taB[7]), [ones] "v"(ones), [ntn] "s"(ntn_s),
                   [nal] "s"(na.srd[0]), [nah] "s"(na.srd[1]), [nralo] "s"(na.rem_lo), [nrahi] "s"(na.rem_hi),
                   [nbl] "s"(nb.srd[0]), [nbh] "s"(nb.srd[1]), [nrblo] "s"(nb.rem_lo), [nrbhi] "s"(nb.rem_hi)
                 : "m0", "scc", "s48", "memory", STONK_A4_FRAG_CLOBBERS);

    // ---- epilogue: accumulator block (i, j) = a[4 (8 i + j) ..]: lane (n = lane & 15, qq) holds rows 16 i + 4 qq + e, column
    // 16 j + n. A v_permlane16_swap of the blocks (i, 2 jp) = x and (i, 2 jp + 1) = y leaves, per register e,
    //   x: rows 16 i + 8 (lane >> 5) + e,     columns 32 jp + (lane & 31)
    //   y: rows 16 i + 8 (lane >> 5) + 4 + e, columns 32 jp + (lane & 31)
    // i.e. one atomic wave-instruction = two rows x 128 contiguous bytes.
    // Buffer atomics: a row past M' falls off the end of the buffer, a column past N' is pushed out of its range - no
    // predicate, no branch, 32-bit offsets (M' ldc * 4 < 2^31: the launcher checks).
    const int wm0 = cw.m0 + wr * 128, wn0 = cw.n0 + wc * 128;
    const int ldc_b = (int)p.ldc * 4;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, M * ldc_b, 0x00020000);
    const __amdgpu_buffer_rsrc_t rBias = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, want_bias ? M * 4 : 0, 0x00020000);
    int coff[4];
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
      const int n = wn0 + 32 * jp + (lane & 31);
      coff[jp] = n * 4 + (n < N ? 0 : 0x40000000);
    }
#if STONK_TN_A4_STORE == 2
    float ss = 0.f;   // this lane's share of the tile's sum of squares: values that are stored (row < M', column < N') only
#endif
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float xs[4][4], ys[4][4];
#pragma unroll
      for (int jp = 0; jp < 4; ++jp) {
        const int bx = 8 * i + 2 * jp, by = bx + 1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xs[jp][e] = acc[bx >> 2][4 * (bx & 3) + e];
          ys[jp][e] = acc[by >> 2][4 * (by & 3) + e];
        }
      }
      asm volatile(STONK_A4_SWAP_4(xs, ys));
      const int mrow = wm0 + 16 * i + 8 * (lane >> 5);
#if STONK_TN_A4_STORE == 2
      float sq[4][4];   // (added up as a tree per row block, the eight row blocks one after the other: a short chain)
#endif
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ro = (mrow + e) * ldc_b, ro4 = (mrow + 4 + e) * ldc_b;
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
#if STONK_TN_A4_STORE == 2
          const float vx = xs[jp][e] * p.alpha, vy = ys[jp][e] * p.alpha;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vx), rC, ro + coff[jp], 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vy), rC, ro4 + coff[jp], 0, 0);
          const bool col_in = coff[jp] < 0x40000000;
          sq[e][jp] = ((col_in && mrow + e < M) ? vx * vx : 0.f) + ((col_in && mrow + 4 + e < M) ? vy * vy : 0.f);
#elif STONK_TN_A4_STORE
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xs[jp][e] * p.alpha), rC, ro + coff[jp], 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ys[jp][e] * p.alpha), rC, ro4 + coff[jp], 0, 0);
#else
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(xs[jp][e] * p.alpha, rC, ro + coff[jp], 0, 0);
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(ys[jp][e] * p.alpha, rC, ro4 + coff[jp], 0, 0);
#endif
        }
      }
#if STONK_TN_A4_STORE == 2
      {
        float se[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) se[e] = (sq[e][0] + sq[e][1]) + (sq[e][2] + sq[e][3]);
        ss += (se[0] + se[1]) + (se[2] + se[3]);
      }
#endif
      // bias gradient of this block's 16 features: every column of the extra accumulator holds the same sums
#if STONK_TN_A4_STORE
      if (want_bias && wc == 0 && ct == 0) {
        const int boff = r16 == 0 ? 0 : 0x40000000;   // (one lane per row stores)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(bacc[i][e] * p.alpha), rBias, (wm0 + 16 * i + 4 * qq + e) * 4 + boff, 0, 0);
      }
#else
      if (want_bias && wc == 0) {
        const int boff = r16 == 0 ? 0 : 0x40000000;   // (one lane per row adds)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(bacc[i][e] * p.alpha, rBias, (wm0 + 16 * i + 4 * qq + e) * 4 + boff, 0, 0);
      }
#endif
    }
#if STONK_TN_A4_STORE == 2
    {
      // (the previous tile's reader of these four words is two barriers or more behind: every K loop has them)
      volatile float* part = (volatile float*)(smem + IMG_LDS);
      ss = wave_sum(ss);
      if (lane == 0) part[wave] = ss;
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (tid == 0) ((float*)p.aux)[(cw.m0 / BM) * ntn + cw.n0 / BN] = ((part[0] + part[1]) + part[2]) + part[3];
    }
#endif
    if (!more) break;
    cwi = nwi;
    cw = nw;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef STONK_TN_A4_DMA_OPERANDS
#undef STONK_TN_A4_BID
}

}  // namespace

#if STONK_TN_A4_GROUP
// the grouped form; g.first / g.items / every split_k already chosen (stonk_gemm_tn_bf16_group), grid = blocks in all
int STONK_TN_A4_LAUNCH(const TnGroupArgs& g, int grid, hipStream_t st) {
  return launch_with_lds<STONK_TN_A4_KERNEL, LDS_BYTES>(g, grid, 256, st);
}
#else
// weight-gradient form on the written-out loop; a.split_k already chosen, a.flags = grid cap in CUs (stonk_gemm_tn_bf16)
int STONK_TN_A4_LAUNCH(const GemmArgs& a, hipStream_t st) {
  const int n_cu = cu_count();
  if (n_cu <= 0) return (int)hipGetLastError();
  const long tiles = (long)((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * a.split_k;
  const int cap = (a.flags > 0 && a.flags < n_cu) ? a.flags : n_cu;
  const int grid = (int)(tiles < cap ? tiles : cap);
  return launch_with_lds<STONK_TN_A4_KERNEL, LDS_BYTES>(a, grid, 256, st);
}
#endif

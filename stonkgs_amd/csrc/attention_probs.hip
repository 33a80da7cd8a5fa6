// Attention probabilities written out: P = softmax(Q K^T * scale + key mask) as fp32 [B, NH, S, S] (HuggingFace's
// `attentions` layout) and / or the per-row probability mass on the two key halves (text / entities), fp32 [B, NH, S, 2].
// Forward-only, no dropout, padded layout only; a separate kernel from the flash-style ones of attention.hip, which never
// hold the S x S scores and are not touched by this file.
//
// Replaces hf:models/bert/modeling_bert.py :111-136 as far as `attention_probs`.
//
// Semantics (those of the forward kernel, attention.hip):
//  * a masked key (attention_mask == 0) gets probability exactly 0.0 - its raw score is NEG_MASK = -2^100, entered as the
//    MFMA accumulator's initial value: the products are absorbed, as the reference's finfo.min absorbs them, and the
//    exponential of the difference to any live maximum is 0;
//  * padded positions AS QUERIES still get a row (the reference masks keys only);
//  * a sequence with NO unmasked key attends uniformly, P = 1/S: every score is exactly NEG_MASK, NEG_MASK * scale is
//    exact, fma(s, scale, -max) is exactly 0 for every key and the row sum is exactly S. No special case.
// The kernel takes no log-sum-exp from the forward (which cannot express the last case) and is self-contained, in two
// passes over the key tiles: pass 1 finds every query row's maximum and sum, pass 2 recomputes the scores and stores
// exp2(s - max) / sum. The recomputation is free: the launch is bound by its B * NH * S^2 * 4 bytes of stores.
//
// Orientation: S^T = K . Q^T with v_mfma_f32_16x16x32_bf16 - A = 16 keys x 32 dims (ds_read_b128 rows of the K tile in
// LDS), B = Q^T (the wave's 16 queries, registers for the whole kernel; both operands are contiguous along the head
// dimension, so no transposing read is needed). A lane then holds, for query (lane & 15), the four consecutive keys
// 4 (lane >> 4) .. + 3 of every 16-key subtile: the statistics are per-lane scalars merged across the four lane groups
// once, after pass 1. For the stores a wave's [16 queries][64 keys] tile goes through LDS and comes back row-major: every
// lane writes 16 contiguous bytes and every store instruction covers four query rows x 256 contiguous bytes (whole
// 128-byte lines). `modal_mass` is summed per lane over the tiles of each half in tile order and merged across the lane
// groups by two xor shuffles: no atomics, bitwise reproducible.
#include "common.h"
#include "attn_tiles.h"   // the K tile image and its swizzle, the score-bias constants, the XCD map

namespace {

constexpr int QB = 128;       // queries per workgroup: 4 waves x 2 groups of 16
constexpr int PLD = TK + 4;   // floats per row of a wave's probability tile (272 bytes: 16 rows two-way at worst)

struct ProbsArgs {
  const bf16* q;
  const bf16* k;
  long ld;
  const long* mask;   // [B,S] or null
  float* probs;       // [B,NH,S,S] or null
  float* modal;       // [B,NH,S,2] or null
  int NH, S, half;
  float scale;
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// orders a wave's LDS writes against its own later reads of other lanes' data (and the reverse): the wave runs in lockstep
// and the LDS serves a wave in order, so only the compiler has to be held
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup -> (query block, head, sequence) through xcd_linear(): every XCD takes one contiguous run of the linear
// order, so the S/128 blocks of a head read its K through one L2.
template <bool STORE_P>
__global__ __launch_bounds__(256, 2) void attn_probs_kernel(const ProbsArgs p) {
  __shared__ __attribute__((aligned(16))) char kt_lds[2 * TILEB];
  __shared__ __attribute__((aligned(16))) float p_lds[4][16 * PLD];
  extern __shared__ __attribute__((aligned(16))) float kbias[];   // [S] (dynamic: the launcher sizes it)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;   // MFMA column (query) / row group (keys 4g .. 4g+3 of a 16-key subtile)
  const int S = p.S, nxb = S / QB;
  const int l = xcd_linear(blockIdx.x, gridDim.x);
  const int xb = l % nxb, bh = l / nxb;     // bh = b * NH + h
  const int b = bh / p.NH, h = bh - b * p.NH;
  const long tok0 = (long)b * S;
  const int q0 = xb * QB + wave * 32;
  const float sc2 = p.scale * LOG2E;

  // the additive bias of every key of the sequence, once
  for (int key = tid; key < S; key += 256) kbias[key] = (p.mask == nullptr || p.mask[tok0 + key] != 0) ? 0.f : NEG_MASK;

  // B operand: Q^T of the wave's two groups of 16 queries - lane (c, g) holds Q[q][32 ks + 8 g .. + 7]
  bf16x8 qf[2][2];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const bf16* qrow = p.q + (tok0 + q0 + 16 * qg + c) * p.ld + h * HD;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qg][ks] = *(const bf16x8*)(qrow + 32 * ks + 8 * g);
  }

  // K tiles: 64 rows x 128 bytes = 512 16-byte chunks over 256 threads, fetched one tile ahead
  const bf16* kbase = p.k + tok0 * p.ld + h * HD;
  const int ntiles = S / TK, nit = 2 * ntiles;
  Stage2 stage;
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int id = tid + 256 * i;
      stage.c[i] = *(const bf16x8*)(kbase + (long)(kt * TK + (id >> 3)) * p.ld + (id & 7) * 8);
    }
  };
  auto store_tile = [&](int buf) { stage_store(stage, kt_lds + buf * TILEB, tid); };
  load_tile(0);
  store_tile(0);
  __syncthreads();   // (also publishes kbias)

  float m[2] = {NEG_INIT, NEG_INIT}, sum[2] = {0.f, 0.f}, inv[2] = {0.f, 0.f};   // m in scaled log2 units
  float mass[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float* pw = p_lds[wave];
  float* prow = p.probs + ((long)bh * S + q0) * S;   // 64-bit base of the wave's rows; offsets below stay under S * 32

  for (int it = 0; it < nit; ++it) {   // pass 1: tiles 0 .. ntiles-1, pass 2: the same tiles again
    const int kt = it < ntiles ? it : it - ntiles;
    const char* Ks = kt_lds + (it & 1) * TILEB;
    if (it + 1 < nit) load_tile(it + 1 < ntiles ? it + 1 : it + 1 - ntiles);
    if (it == ntiles) {   // between the passes: merge the statistics of the four lane groups (all lanes of a row agree)
#pragma unroll
      for (int qg = 0; qg < 2; ++qg) {
        float mm = fmaxf(m[qg], __shfl_xor(m[qg], 16, 64));
        mm = fmaxf(mm, __shfl_xor(mm, 32, 64));
        float s = sum[qg] * __builtin_amdgcn_exp2f(m[qg] - mm);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        m[qg] = mm;
        inv[qg] = 1.f / s;
      }
    }
    // A operand: the tile's four 16-key subtiles - lane (c, g) holds K[16 t + c][32 ks + 8 g .. + 7]
    bf16x8 kf[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[t][ks] = *(const bf16x8*)(Ks + tile_off(16 * t + c, 32 * ks + 8 * g));
    f32x4 kb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) kb[t] = *(const f32x4*)(kbias + kt * TK + 16 * t + 4 * g);

#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      // S^T[key][query] (+ key bias through the accumulator), raw units: s[t][j] = key 16 t + 4 g + j, query c
      f32x4 s[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[t] = kb[t];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) s[t] = mfma16(kf[t][ks], qf[qg][ks], s[t]);
      }
      if (it < ntiles) {   // pass 1: this lane's running maximum and sum
        float tmax = s[0][0];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) tmax = fmaxf(tmax, s[t][j]);
        const float m_new = fmaxf(m[qg], tmax * sc2);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) rs += __builtin_amdgcn_exp2f(fmaf(s[t][j], sc2, -m_new));
        sum[qg] = sum[qg] * __builtin_amdgcn_exp2f(m[qg] - m_new) + rs;
        m[qg] = m_new;
      } else {             // pass 2: the probabilities
        // (the mass is summed BEFORE the normalisation: additions only, so that nothing here can be contracted into an
        // fma in one instantiation and not in the other - the two output modes give bitwise the same mass)
        float ms = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s[t][j] = __builtin_amdgcn_exp2f(fmaf(s[t][j], sc2, -m[qg]));
            ms += s[t][j];
          }
        if (kt * TK < p.half) mass[qg][0] += ms;   // (half is a multiple of the tile: a tile lies in one half)
        else mass[qg][1] += ms;
        if (STORE_P) {
          wave_lds_sync();   // the previous round's reads are done
#pragma unroll
          for (int t = 0; t < 4; ++t) *(f32x4*)(pw + c * PLD + 16 * t + 4 * g) = s[t] * inv[qg];
          wave_lds_sync();
          // row-major again: lane (c, g) takes keys 4c .. 4c+3 of rows g, g+4, g+8, g+12 - 4 rows x 256 bytes per store
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = g + 4 * i;
            const f32x4 v = *(const f32x4*)(pw + row * PLD + 4 * c);
            __builtin_nontemporal_store(v, (f32x4*)(prow + (16 * qg + row) * S + kt * TK + 4 * c));
          }
        }
      }
    }
    if (it + 1 < nit) store_tile((it + 1) & 1);
    __syncthreads();
  }

  if (p.modal) {
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      float a = mass[qg][0], e = mass[qg][1];
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      e += __shfl_xor(e, 16, 64);
      e += __shfl_xor(e, 32, 64);
      if (g == 0) *(f32x2*)(p.modal + ((long)bh * S + q0 + 16 * qg + c) * 2) = (f32x2){a * inv[qg], e * inv[qg]};
    }
  }
}

}  // namespace

extern "C" int stonk_attention_probs(const void* q, const void* k, int64_t ld, const int64_t* attention_mask, float* probs,
                                     float* modal_mass, int B, int NH, int S, int D, int half, float scale, void* stream) {
  STONK_CHECK_ARG(q && k, STONK_EINVAL);
  STONK_CHECK_ARG(probs || modal_mass, STONK_EINVAL);
  STONK_CHECK_ARG(D == HD, STONK_ESHAPE);
  STONK_CHECK_ARG(B >= 0 && NH > 0 && S >= 128 && S % 128 == 0 && S <= 4096, STONK_ESHAPE);
  STONK_CHECK_ARG(half > 0 && half < S && half % 64 == 0, STONK_EINVAL);
  STONK_CHECK_ARG(scale > 0.f, STONK_EINVAL);   // (the row maximum is taken on the raw scores)
  STONK_CHECK_ARG(ld >= HD && ld % 8 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)probs % 16 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)modal_mass % 8 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((long)B * NH * (S / QB) < (1L << 31), STONK_ESHAPE);   // the grid's linear index
  if (B == 0) return STONK_OK;
  ProbsArgs a = {};
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.ld = ld; a.mask = (const long*)attention_mask;
  a.probs = probs; a.modal = modal_mass; a.NH = NH; a.S = S; a.half = half; a.scale = scale;
  const dim3 grid((unsigned)((long)B * NH * (S / QB))), block(256);
  const size_t kb = (size_t)S * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (probs) hipLaunchKernelGGL((attn_probs_kernel<true>), grid, block, kb, st, a);
  else hipLaunchKernelGGL((attn_probs_kernel<false>), grid, block, kb, st, a);
  return stonk_launch_status();
}

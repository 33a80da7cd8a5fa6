// Device helpers shared by the row-wise kernel sources (norm.hip, loss.hip, topk.hip): the 8-element piece loads of the
// sweeps and copies, and a wave's row held in registers in the two layouts the LayerNorm kernels use. What is also of use
// outside this family lives in common.h.
#pragma once
#include "common.h"

// ---- one 8-element piece of a row ----------------------------------------------------------------------------------------
// as eight floats (fp32: two 16-byte loads; fp16: one)
__device__ __forceinline__ void load8(const float* x, float (&v)[8]) {
  const f32x4 a = *(const f32x4*)x, b = *(const f32x4*)(x + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}
__device__ __forceinline__ void load8(const _Float16* x, float (&v)[8]) {
  const f16x8 a = *(const f16x8*)x;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
}
// as the bf16x8 a row of bf16 stores (a bf16 source is copied, an fp32 source rounded)
__device__ __forceinline__ bf16x8 load8_bf16(const bf16* x) { return *(const bf16x8*)x; }
__device__ __forceinline__ bf16x8 load8_bf16(const float* x) {
  const f32x4 a = *(const f32x4*)x, b = *(const f32x4*)(x + 4);
  return (bf16x8){(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}

// ---- chunk layout: lane l of the wave that owns a row holds its 8-element chunks l, l + 64, ... (any H % 8 == 0) ----------
template <int CPL>
struct RowRegs {
  float v[CPL][8];
};

// r = row; chunks past the row's end read as zero
template <int CPL>
__device__ __forceinline__ void load_row(const bf16* row, int nch, int lane, RowRegs<CPL>& r) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const bf16x8 x = *(const bf16x8*)(row + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) r.v[i][j] = (float)x[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r.v[i][j] = 0.f;
    }
  }
}
// the same from an fp32 row, or with ADD: r += row
template <bool ADD = false, int CPL>
__device__ __forceinline__ void load_row(const float* row, int nch, int lane, RowRegs<CPL>& r) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const f32x4 a = *(const f32x4*)(row + c * 8);
      const f32x4 b = *(const f32x4*)(row + c * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r.v[i][j] = ADD ? r.v[i][j] + a[j] : a[j];
        r.v[i][4 + j] = ADD ? r.v[i][4 + j] + b[j] : b[j];
      }
    } else if (!ADD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r.v[i][j] = 0.f;
    }
  }
}
template <int CPL>
__device__ __forceinline__ void store_bf16_row(bf16* row, int nch, int lane, const RowRegs<CPL>& r) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)r.v[i][j];
      *(bf16x8*)(row + c * 8) = o;
    }
  }
}

// ---- lane layout for H = 64 * EPL: every lane owns EPL columns for the whole launch - one 16-byte piece per 512 columns
// plus an 8-byte piece when EPL % 8 == 4 - so per-column values (gamma, dropout column keys) can stay in registers ------------
template <int EPL>
struct LaneRow {
  static_assert(EPL % 4 == 0 && EPL >= 4, "lane layout: 4-element granules");
  static constexpr int H = EPL * 64, NQ = EPL / 8;
  static constexpr bool TAIL = (EPL & 4) != 0;
  static constexpr int NQ8 = NQ > 0 ? NQ : 1;   // a row as loaded: bf16x8 p8[NQ8] and bf16x4 p4

  // the column of a lane's element e, as a function of e. `lane` is captured BY REFERENCE: pass a named variable that
  // outlives the lambda (the kernel's `const int lane`), never a temporary. (A lambda the kernel keeps, as it kept one of
  // its own before: as a plain function of (lane, e) one forward instance loads gamma / beta in other pieces)
  static __device__ __forceinline__ auto col_of(const int& lane) {
    return [&lane](int e) { return e < NQ * 8 ? (e >> 3) * 512 + lane * 8 + (e & 7) : NQ * 512 + lane * 4 + (e & 3); };
  }
  // piece q of the row (q == NQ: the 8-byte tail), requested and not waited for
  static __device__ __forceinline__ void load_piece(const bf16* row, int lane, int q, bf16x8 (&p8)[NQ8], bf16x4& p4) {
    if (q < NQ) p8[q] = *(const bf16x8*)(row + q * 512 + lane * 8);
    else p4 = *(const bf16x4*)(row + NQ * 512 + lane * 4);
  }
  static __device__ __forceinline__ float at(const bf16x8 (&p8)[NQ8], const bf16x4& p4, int e) {
    return e < NQ * 8 ? (float)p8[e >> 3][e & 7] : (float)p4[e & 3];
  }
  static __device__ __forceinline__ void store(bf16* row, int lane, const float (&v)[EPL]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)v[q * 8 + j];
      *(bf16x8*)(row + q * 512 + lane * 8) = o;
    }
    if (TAIL) {
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)v[NQ * 8 + j];
      *(bf16x4*)(row + NQ * 512 + lane * 4) = o;
    }
  }
};

// a wave's sum by DPP adds + v_readlane: the result is wave-uniform (in SGPRs). All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_sum_uniform(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror
  v += dpp_mov<0x140>(v);   // row_mirror: every lane of a 16-lane row now holds the row's sum
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

// ---- LayerNorm of a row held in the chunk layout (norm.hip's generic kernels and embedding front-ends, bigbird_rowwise.hip) ----
// two-pass (mean, then centred variance) statistics in fp32, as torch's native_layer_norm computes them
template <int CPL>
__device__ __forceinline__ void row_stats(const RowRegs<CPL>& r, int nch, int lane, int H, float eps, float& mean,
                                          float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += r.v[i][j];
  mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = r.v[i][j] - mean;
        q += d * d;
      }
    }
  }
  const float var = wave_sum(q) / (float)H;
  rstd = rsqrtf(var + eps);
}

// y = (x - mean) * rstd * gamma + beta, optional inverted dropout on y
template <int CPL>
__device__ __forceinline__ void normalize_store(RowRegs<CPL>& r, int nch, int lane, float mean, float rstd,
                                                const float* gamma, const float* beta, bf16* yrow, long row_idx, int H,
                                                bool drop, uint32_t thr32, float dscale, uint32_t seed) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const f32x4 g0 = *(const f32x4*)(gamma + c * 8), g1 = *(const f32x4*)(gamma + c * 8 + 4);
      const f32x4 b0 = *(const f32x4*)(beta + c * 8), b1 = *(const f32x4*)(beta + c * 8 + 4);
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = j < 4 ? g0[j] : g1[j - 4];
        const float b = j < 4 ? b0[j] : b1[j - 4];
        float y = (r.v[i][j] - mean) * rstd * g + b;
        if (drop) y = stonk_keep((uint32_t)row_idx, (uint32_t)(c * 8 + j), seed, thr32) ? y * dscale : 0.f;
        o[j] = (bf16)y;
      }
      *(bf16x8*)(yrow + c * 8) = o;
    }
  }
}

// Tile helpers shared by the dense attention kernels (attention.hip), the block-sparse ones (bigbird_attention.hip) and
// the written-out probabilities (attention_probs.hip): the [64][64] bf16 LDS tile image and its swizzle, the MFMA
// fragments read from it, the register-staged tile loads, the packed fp32 / bf16 arithmetic, the score-bias constants, the
// accumulator conversions and row stores, the XCD map and the delta row sum. Each including file gets its own (internal)
// copy. A helper is used only where the kernel compiles to the instructions of its written-out form
// (profiles/refactor_attention_sources.md lists, per helper, the kernels that keep their own lines for that reason).
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int HD = 64;        // head dim
constexpr int TK = 64;        // rows per LDS tile
constexpr int ROWB = 128;     // bytes per tile row
constexpr int TILEB = TK * ROWB;
constexpr int STAGEB = 2 * TILEB + 2 * TK * 4;   // two [64][64] bf16 tiles + two rows of 64 floats
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
// Additive key-padding bias in RAW score units, entered as the MFMA accumulator's initial value. A power of two: the
// products are absorbed (every masked score is exactly NEG_MASK, as the reference's finfo.min absorbs them) and
// NEG_MASK * scale is exact, so exp2(fma(s, scale, -max)) is exactly 1 for a row whose keys are all masked.
constexpr float NEG_MASK = -0x1p100f;
// Keys past the end of a packed sequence (the rest of its last 64-key tile: their K rows arrive as zeros) sit strictly
// BELOW the masked ones: when every real key is masked, the row maximum is NEG_MASK and the real keys' exp2 is 1 - theirs
// must still be 0, or a sequence of n rows would attend uniformly over 64 ceil(n / 64) keys.
constexpr float NEG_PAST = -0x1p101f;
constexpr float NEG_INIT = -0x1p120f;

// 16-byte chunk swizzle of a 128-byte tile row. Rows 2t and 2t+1 sit in opposite bank halves and share a swizzle; the
// swizzle is a bit rotation of t so that (a) 16 consecutive rows reading one logical chunk (ds_read_b128 fragments) hit
// 16 different bank groups and (b) rows r and r+2 of a transposed 4-row x 64-byte read (ds_read_b64_tr_b16) fall into
// different chunk halves - with the plain (row >> 1) & 7 they collided two ways (SQ_LDS_BANK_CONFLICT 20 % of LDS cycles).
__device__ __forceinline__ int swz(int row) {
  const int t = (row >> 1) & 7;
  return ((t & 1) << 2) | (t >> 1);
}
// byte offset of element (row, col) inside a [64][64] bf16 tile image
__device__ __forceinline__ int tile_off(int row, int col) {
  return row * ROWB + ((((col >> 3) ^ swz(row)) << 4) | ((col & 7) << 1));
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// Maximum of a 32x32 MFMA accumulator tile's 16 registers (and a running value) in eight v_max3_f32. fmaxf on MFMA
// results would make the compiler canonicalise every input first (one more VALU op per element), hence the asm - but the
// hazard recogniser does not see asm operands, so the statement carries its own wait for the MFMA that produced its
// inputs (an XDL write needs up to 19 wait states before a VALU read of the same registers).
__device__ __forceinline__ float max16_mfma(const f32x16& a) {
  float d;
  asm("s_nop 15\n\ts_nop 3\n\t"
      "v_max3_f32 %0, %1, %2, %3\n\t"
      "v_max3_f32 %0, %0, %4, %5\n\t"
      "v_max3_f32 %0, %0, %6, %7\n\t"
      "v_max3_f32 %0, %0, %8, %9\n\t"
      "v_max3_f32 %0, %0, %10, %11\n\t"
      "v_max3_f32 %0, %0, %12, %13\n\t"
      "v_max3_f32 %0, %0, %14, %15\n\t"
      "v_max3_f32 %0, %0, %16, %16"
      : "=&v"(d)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
        "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]));
  return d;
}
// same, folded into a running maximum (the compiler orders the two tiles' MFMAs freely, so this one waits as well)
__device__ __forceinline__ float max16_chain(float t, const f32x16& a) {
  float d;
  asm("s_nop 15\n\ts_nop 3\n\t"
      "v_max3_f32 %0, %17, %1, %2\n\t"
      "v_max3_f32 %0, %0, %3, %4\n\t"
      "v_max3_f32 %0, %0, %5, %6\n\t"
      "v_max3_f32 %0, %0, %7, %8\n\t"
      "v_max3_f32 %0, %0, %9, %10\n\t"
      "v_max3_f32 %0, %0, %11, %12\n\t"
      "v_max3_f32 %0, %0, %13, %14\n\t"
      "v_max3_f32 %0, %0, %15, %16"
      : "=&v"(d)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
        "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]), "v"(t));
  return d;
}

// Packed fp32 arithmetic (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: two floats per issue slot) and the packed
// conversion (one v_cvt_pk_bf16_f32 per pair; element-wise casts into a bf16 vector cost a conversion AND a v_perm each).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ bf16x8 pack8(const float* e) {
  union {
    bf16x8 v;
    bf16x2 h[4];
  } u;
#pragma unroll
  for (int j = 0; j < 4; ++j) u.h[j] = __builtin_convertvector((f32x2){e[2 * j], e[2 * j + 1]}, bf16x2);
  return u.v;
}

// A/B fragment of a 32x32x16 MFMA read by rows: lane (r, hh) gets tile[row0 + r][16*st + 8*hh .. +7]
__device__ __forceinline__ bf16x8 row_frag(const char* tile, int row0, int st, int r, int hh) {
  return *(const bf16x8*)(tile + tile_off(row0 + r, 16 * st + 8 * hh));
}

// Transposed A fragment: lane (r = column c0 + (lane & 31), hh) gets tile[row0 + 8*(j>>2) + 4*hh + (j&3)][col]
// for j = 0..7: exactly the k order of an accumulator tile reused as B operand (guide section 3).
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int row0, int c0, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int col = c0 + 16 * (g & 1) + 4 * (i & 3);
  const int row = row0 + 4 * (g >> 1) + (i >> 2);
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(tile + tile_off(row, col)));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(tile + tile_off(row + 8, col)));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// stage a [64][64] bf16 tile: 512 16-byte chunks over 256 threads
struct Stage2 {
  bf16x8 c[2];
};
// rows row0 .. row0+63 of the sequence that starts at `base`, through a buffer that begins at the tile's first row and
// ends with the sequence's last one: rows past it arrive as ZEROS - finite values the callers mask out (a packed
// sequence's length need not be a multiple of the tile). The descriptor is scalar arithmetic per tile and the per-thread
// offsets (TileOff) are two loop-invariant registers per row stride: with per-thread 64-bit addresses the compiler
// rebuilt row * ld for every load of every tile - 13 v_lshl_add_u64, 8 v_mul_lo_u32 and 4 v_mad_u64_u32 per tile, a fifth
// of the forward kernel's vector instructions (tools/isa_mix.py).
struct TileOff {
  int o[2];
};
__device__ __forceinline__ TileOff tile_voff(long ld, int tid) {
  TileOff t;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    t.o[i] = (id >> 3) * (int)(ld * 2) + (id & 7) * 16;
  }
  return t;
}
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
__device__ __forceinline__ void stage_load(Stage2& s, const bf16* base, long ld, int row0, int n, const TileOff& vo) {
#ifdef STONK_ATTN_ABLATE_LOADS   // timing experiment (tools/attn_probe.py): every tile re-reads the sequence's first - cache hits
  row0 = 0;
#endif
  row0 = __builtin_amdgcn_readfirstlane(row0);
  const int rows = n - row0 < TK ? n - row0 : TK;   // >= 1: the caller only asks for tiles that start inside the sequence
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(base + (long)row0 * ld), 0, (rows - 1) * (int)(ld * 2) + ROWB, 0x00020000);
#pragma unroll
  for (int i = 0; i < 2; ++i) s.c[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, vo.o[i], 0, 0));
}
__device__ __forceinline__ void stage_store(const Stage2& s, char* tile, int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    *(bf16x8*)(tile + tile_off(id >> 3, (id & 7) * 8)) = s.c[i];
  }
}

#ifdef STONK_ATTN_ABLATE_BARRIER   // timing experiment: the waves of a workgroup run free (races: garbage results)
#define TILE_BARRIER() __builtin_amdgcn_sched_barrier(0)
#else
#define TILE_BARRIER() __syncthreads()
#endif

// A zeroed accumulator, and the score accumulator's initial value: the bias of this lane's 16 keys (Mb: the 32 keys of its
// MFMA tile), zeros without a mask
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
template <bool HAS_MASK>
__device__ __forceinline__ f32x16 score_bias(const float* Mb, int hh) {
  f32x16 s;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 mb = {0.f, 0.f, 0.f, 0.f};
    if (HAS_MASK) mb = *(const f32x4*)(Mb + 8 * g + 4 * hh);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[4 * g + j] = mb[j];
  }
  return s;
}

// registers 8 ks .. 8 ks + 7 of an accumulator tile as the B operand of the next MFMA
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& s, int ks) {
  float e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = s[8 * ks + j];
  return pack8(e);
}

// A lane's output row: val(dt, i) = the final value of register i of its accumulator for columns 32 dt .. + 31, as bf16
template <class F>
__device__ __forceinline__ void store_row(bf16* row, int hh, F val) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 v = {(bf16)val(dt, 4 * g), (bf16)val(dt, 4 * g + 1), (bf16)val(dt, 4 * g + 2), (bf16)val(dt, 4 * g + 3)};
      *(bf16x4*)(row + dt * 32 + 8 * g + 4 * hh) = v;
    }
}

// Workgroups are dispatched round-robin over the 8 XCDs: the place of workgroup `lin` of n in an order where every XCD
// takes one contiguous run (a bijection of [0, n)), so that neighbours in that order share an L2
__device__ __forceinline__ int xcd_linear(int lin, int n) {
  const int q = n >> 3, rm = n & 7, x = lin & 7;
  return ((x < rm) ? x * (q + 1) : rm * (q + 1) + (x - rm) * q) + (lin >> 3);
}

// delta = rowsum(dO * O) of one 64-column row, in the dQ kernel's order - its lane pair (r, hh) sums the 8-column chunks
// 2 st + hh, st = 0..3, then adds the two halves - so that every producer of delta gives bitwise the same
__device__ __forceinline__ float delta_row(const bf16* drow, const bf16* orow) {
  float half[2] = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bf16x8 d = *(const bf16x8*)(drow + 8 * c), o = *(const bf16x8*)(orow + 8 * c);
#pragma unroll
    for (int j = 0; j < 8; ++j) half[c & 1] += (float)o[j] * (float)d[j];
  }
  return half[0] + half[1];
}

// host side: a runtime flag as a template argument - f gets std::true_type or std::false_type
template <class F>
void with_flag(bool on, F f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace

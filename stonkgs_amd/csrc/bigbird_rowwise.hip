// The row-wise kernels only the BigBird encoder needs (stonkgs_amd/bigbird_encoder.py): gelu_new, and BigBird's embeddings
// on given inputs_embeds with their backward's last step (further down).
//
// gelu_new, BigBird's hidden_act (hf:activations.py NewGELUActivation, the tanh form), forward and backward as bf16
// elementwise passes: the GEMM epilogues know the erf form only (STONK_EPI_GELU / _GELU_BWD), so the BigBird encoder runs
// its FFN-up GEMM with the bias alone, keeps the bf16 pre-activation u, and these kernels follow.
//
//   g  = 0.5 u (1 + tanh(a)),  a = c (u + k u^3),  c = sqrt(2 / pi),  k = 0.044715
//   du = dg [0.5 (1 + t) + 0.5 u (1 - t^2) c (1 + 3 k u^2)],  t = tanh(a)
//
// Both are evaluated through s = 0.5 (1 + t) = 1 / (1 + exp(-2a)), the logistic function of 2a:
//   g  = u s                       (relative accuracy kept on the negative side, where 1 + t cancels)
//   du = dg [s + u s (1 - s) 2c (1 + 3 k u^2)]        (1 - t^2 = 4 s (1 - s), 1 - s = E s with E = exp(-2a))
// For every finite bf16 u: u^3 may overflow to +-inf, then a = +-inf (u and u^3 have one sign: no inf - inf), E = 0 or
// inf and s = 1 or 0 exactly - g = u or -0. The derivative's second term would be (1 - t^2) * inf = 0 * inf there, so it
// is DROPPED once |2a| >= 87 (where fp32's exp(87) is still finite and 1 - t^2 < 4e-38: |u| > 7.5, the term is below 1e-34
// and t has long rounded to +-1); the first term s alone is then the derivative, 1 or 0 to fp32. Below that threshold
// |u| < 7.6 and every factor is finite.
#include "rowwise.h"

namespace {

constexpr float GN_2C = 1.5957691216057308f;   // 2 sqrt(2 / pi)
constexpr float GN_K = 0.044715f;
constexpr float GN_SAT = 87.f;

// z = 2a
__device__ __forceinline__ float gn_arg(float u) { return GN_2C * (u + GN_K * u * u * u); }

__device__ __forceinline__ float gelu_new_val(float u) {
  const float s = __builtin_amdgcn_rcpf(1.f + __expf(-gn_arg(u)));
  return u * s;
}
__device__ __forceinline__ float gelu_new_grad(float u) {
  const float z = gn_arg(u);
  const float E = __expf(-z);
  const float s = __builtin_amdgcn_rcpf(1.f + E);
  if (!(fabsf(z) < GN_SAT)) return s;
  return s + u * (s * (E * s)) * (GN_2C * (1.f + 3.f * GN_K * u * u));
}

__global__ __launch_bounds__(256) void gelu_new_fwd_kernel(const bf16* __restrict__ u, bf16* __restrict__ g, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const bf16x8 a = *(const bf16x8*)(u + 8 * i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)gelu_new_val((float)a[j]);
    *(bf16x8*)(g + 8 * i) = o;
  }
}

// (dg and du carry no __restrict__: the encoder runs this in place, du == dg - a thread reads its 8 elements, then writes them)
__global__ __launch_bounds__(256) void gelu_new_bwd_kernel(const bf16* dg, const bf16* __restrict__ u, bf16* du, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const bf16x8 a = *(const bf16x8*)(dg + 8 * i), b = *(const bf16x8*)(u + 8 * i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)a[j] * gelu_new_grad((float)b[j]));
    *(bf16x8*)(du + 8 * i) = o;
  }
}

constexpr long GN_GRID_CAP = 4096;   // workgroups of a launch: one trip covers GN_GRID_CAP * 256 * 8 elements

// BigBird's embeddings on given inputs_embeds (hf:models/big_bird/modeling_big_bird.py BigBirdEmbeddings :120-128):
// LayerNorm(dropout(inputs_embeds + token_type + position)) - the dropout BEFORE the LayerNorm, the opposite of BERT's
// order, so neither joint_embed_ln_kernel nor the LN_DROPOUT form of the LayerNorm (norm.hip) can express it. The dropped
// sum is what the LayerNorm reads: sum_out keeps it (bf16) for the backward, the statistics come from the fp32 values as
// in joint_embed_ln_kernel (row_stats / normalize_store: rowwise.h). The mask is the element form of the generator,
// (row, column) = (output row, column), as at the LN_DROPOUT site. A token type outside [0, type_rows) reads row 0 (the
// launcher has no error word: the host checks).
template <int CPL>
__global__ __launch_bounds__(256) void embeds_ln_kernel(
    const float* __restrict__ inputs_embeds, long ld_in, const long* __restrict__ token_type_ids,
    const float* __restrict__ pos_emb, const float* __restrict__ type_emb, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16* __restrict__ sum_out, bf16* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, long rows, int S, int H, int type_rows, float eps, bool drop, uint32_t thr32, float dscale,
    uint32_t seed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = H >> 3;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const int s = (int)(row % S);
    long tt = token_type_ids ? token_type_ids[row] : 0;
    if (tt < 0 || tt >= type_rows) tt = 0;
    RowRegs<CPL> r;
    load_row(inputs_embeds + row * ld_in, nch, lane, r);
    load_row<true>(type_emb + tt * H, nch, lane, r);
    load_row<true>(pos_emb + (long)s * H, nch, lane, r);
    if (drop) {
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int c = lane + 64 * i;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          r.v[i][j] = stonk_keep((uint32_t)row, (uint32_t)(c * 8 + j), seed, thr32) ? r.v[i][j] * dscale : 0.f;
      }
    }
    store_bf16_row<CPL>(sum_out + row * H, nch, lane, r);
    float mean, rstd;
    row_stats<CPL>(r, nch, lane, H, eps, mean, rstd);
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
    normalize_store<CPL>(r, nch, lane, mean, rstd, gamma, beta, y + row * H, row, H, false, 0u, 1.f, 0u);
  }
}

// The end of that front-end's backward: dsum = d(LayerNorm input) from stonk_layernorm_bwd; the mask is regenerated and
// g = keep ? dsum / (1 - p) : 0 goes out twice - fp32 as d(inputs_embeds), bf16 as what stonk_embed_grad sums into the
// position and token-type gradients. One thread per 8-column piece.
__global__ __launch_bounds__(256) void embeds_ln_bwd_finish_kernel(const bf16* __restrict__ dsum, long ld,
                                                                   float* __restrict__ d_in, long ld_out,
                                                                   bf16* __restrict__ dx_masked, long rows, int H, bool drop,
                                                                   uint32_t thr32, float dscale, uint32_t seed) {
  const int nch = H >> 3;
  const long pieces = rows * nch;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (long)gridDim.x * 256) {
    const long row = i / nch;
    const int c = (int)(i - row * nch);
    const bf16x8 d = *(const bf16x8*)(dsum + row * ld + c * 8);
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      g[j] = (float)d[j];
      if (drop) g[j] = stonk_keep((uint32_t)row, (uint32_t)(c * 8 + j), seed, thr32) ? g[j] * dscale : 0.f;
    }
    float* o = d_in + row * ld_out + c * 8;
    *(f32x4*)o = (f32x4){g[0], g[1], g[2], g[3]};
    *(f32x4*)(o + 4) = (f32x4){g[4], g[5], g[6], g[7]};
    bf16x8 m;
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = (bf16)g[j];
    *(bf16x8*)(dx_masked + row * H + c * 8) = m;
  }
}

}  // namespace

extern "C" int stonk_embeds_ln_fwd(const float* inputs_embeds, int64_t ld_in, const int64_t* token_type_ids,
                                   const float* pos_emb, const float* type_emb, const float* gamma, const float* beta,
                                   void* sum_out, void* y, float* mean, float* rstd, int B, int S, int H, int type_rows,
                                   float eps, float drop_p, uint32_t seed, void* stream) {
  STONK_CHECK_ARG(inputs_embeds && pos_emb && type_emb && gamma && beta && sum_out && y && mean && rstd, STONK_EINVAL);
  STONK_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, STONK_EINVAL);
  STONK_CHECK_ARG(B >= 0 && S > 0 && H > 0 && H % 8 == 0 && H <= 1024 && ld_in >= H && type_rows > 0, STONK_ESHAPE);
  STONK_CHECK_ARG((long)B * S < (1L << 31), STONK_ESHAPE);   // (the generator's row index has 32 bits)
  STONK_CHECK_ARG(ld_in % 4 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)inputs_embeds % 16 == 0 && (uintptr_t)pos_emb % 16 == 0 && (uintptr_t)type_emb % 16 == 0 &&
                      (uintptr_t)gamma % 16 == 0 && (uintptr_t)beta % 16 == 0 && (uintptr_t)sum_out % 16 == 0 &&
                      (uintptr_t)y % 16 == 0,
                  STONK_EALIGN);
  if (B == 0) return STONK_OK;
  const long rows = (long)B * S;
  const StonkDrop d = stonk_drop(drop_p, seed);
  // (H <= 1024: two 8-element chunks per lane; the grid of the row-wise kernels that take four rows a workgroup)
  hipLaunchKernelGGL((embeds_ln_kernel<2>), dim3(grid_cap(rows, 4, 2048)), dim3(256), 0, (hipStream_t)stream, inputs_embeds,
                     (long)ld_in, (const long*)token_type_ids, pos_emb, type_emb, gamma, beta, (bf16*)sum_out, (bf16*)y, mean,
                     rstd, rows, S, H, type_rows, eps, drop_p > 0.f, d.thr32, d.scale, d.seed);
  return stonk_launch_status();
}

extern "C" int stonk_embeds_ln_bwd_finish(const void* dsum, int64_t ld, float* d_inputs_embeds, int64_t ld_out,
                                          void* dx_masked, int64_t n_rows, int H, float drop_p, uint32_t seed,
                                          void* stream) {
  STONK_CHECK_ARG(dsum && d_inputs_embeds && dx_masked, STONK_EINVAL);
  STONK_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, STONK_EINVAL);
  STONK_CHECK_ARG(n_rows >= 0 && n_rows < (1L << 31) && H > 0 && H % 8 == 0 && H <= 1024 && ld >= H && ld_out >= H,
                  STONK_ESHAPE);
  STONK_CHECK_ARG(ld % 8 == 0 && ld_out % 4 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)dsum % 16 == 0 && (uintptr_t)d_inputs_embeds % 16 == 0 && (uintptr_t)dx_masked % 16 == 0,
                  STONK_EALIGN);
  if (n_rows == 0) return STONK_OK;
  const StonkDrop d = stonk_drop(drop_p, seed);
  hipLaunchKernelGGL(embeds_ln_bwd_finish_kernel, dim3(grid_cap((long)n_rows * (H >> 3), 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, (const bf16*)dsum, (long)ld, d_inputs_embeds, (long)ld_out, (bf16*)dx_masked,
                     (long)n_rows, H, drop_p > 0.f, d.thr32, d.scale, d.seed);
  return stonk_launch_status();
}

extern "C" int stonk_gelu_new_fwd_bf16(const void* u, void* g, int64_t n, void* stream) {
  STONK_CHECK_ARG(u && g && n >= 0 && n % 8 == 0, STONK_EINVAL);
  STONK_CHECK_ARG((uintptr_t)u % 16 == 0 && (uintptr_t)g % 16 == 0, STONK_EALIGN);
  if (n == 0) return STONK_OK;
  const long n8 = n / 8;
  hipLaunchKernelGGL(gelu_new_fwd_kernel, dim3(grid_cap(n8, 256, GN_GRID_CAP)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)u, (bf16*)g, n8);
  return stonk_launch_status();
}

extern "C" int stonk_gelu_new_bwd_bf16(const void* dg, const void* u, void* du, int64_t n, void* stream) {
  STONK_CHECK_ARG(dg && u && du && n >= 0 && n % 8 == 0, STONK_EINVAL);
  STONK_CHECK_ARG((uintptr_t)dg % 16 == 0 && (uintptr_t)u % 16 == 0 && (uintptr_t)du % 16 == 0, STONK_EALIGN);
  if (n == 0) return STONK_OK;
  const long n8 = n / 8;
  hipLaunchKernelGGL(gelu_new_bwd_kernel, dim3(grid_cap(n8, 256, GN_GRID_CAP)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)dg, (const bf16*)u, (bf16*)du, n8);
  return stonk_launch_status();
}

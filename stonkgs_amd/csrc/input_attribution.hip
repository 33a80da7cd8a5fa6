// Input attributions: per position, the gradient of a prediction with respect to the position's input embedding, reduced
// to saliency |dF/dx_p| and gradient x input <dF/dx_p, x_p> - and, on request, the gradient itself in fp32.
//
// The reference has no call for this. The nearest thing is autograd with respect to the `inputs_embeds` of
// ref:src/stonkgs/models/stonkgs_model.py:193-210 (the concatenation of the frozen backbone's output and the gathered
// entity rows that is handed to `self.bert`), which a reference user reaches only by patching `forward`: the tensor is
// built inside it from ids. Here the hand-written backward already produces d F / d(embedding sum) - `dsum`, the input
// gradient of the embeddings LayerNorm, and the sum is inputs_embeds + position + token-type, so with dropout off that IS
// d F / d inputs_embeds - and this kernel pairs it with the rows the forward's embedding kernel read
// (stonk_joint_embed_ln_fwd): text_hidden for the text half, kg_table[input_ids] for the entity half.
//
// One wavefront per padded position, four positions per workgroup; a lane reads 16-byte pieces of the bf16 gradient row
// and the matching bf16 / fp32 pieces of x, accumulates both sums in fp32 and the wave reduces them with xor shuffles
// (wave_sum), as the row-wise kernels of norm.hip do. No atomics, no workspace: the same input gives the same bits.
// In the packed layout (row_of_pos of stonk_unpad_plan) a dropped position has no row: nothing ever read it, its gradient
// is exactly 0, and all three outputs are written as 0 without a load. An entity id outside the table reads no memory
// either: x counts as 0 (the forward has already raised bit 0 of its error word for it).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void input_attribution_kernel(
    const bf16* __restrict__ dsum, long ld, const long* __restrict__ input_ids, const bf16* __restrict__ text_hidden,
    const float* __restrict__ kg_table, long kg_rows, const int* __restrict__ row_of_pos, float scale,
    float* __restrict__ grad_x_input, float* __restrict__ grad_norm, float* __restrict__ grad_out, long ld_out, long npos,
    int S, int half, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = H >> 3;
  for (long p = (long)blockIdx.x * 4 + wave; p < npos; p += (long)gridDim.x * 4) {
    const long r = row_of_pos ? (long)row_of_pos[p] : p;
    float* go = grad_out ? grad_out + p * ld_out : nullptr;
    if (r < 0) {   // dropped by the row plan: exactly zero
      if (go) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int c = lane; c < nch; c += 64) {
          *(f32x4*)(go + c * 8) = z;
          *(f32x4*)(go + c * 8 + 4) = z;
        }
      }
      if (lane == 0) {
        if (grad_x_input) grad_x_input[p] = 0.f;
        if (grad_norm) grad_norm[p] = 0.f;
      }
      continue;
    }
    const long b = p / S;
    const int s = (int)(p - b * S);
    const bf16* xt = nullptr;    // (wave-uniform: a position lies in one half)
    const float* xk = nullptr;
    if (s < half) {
      xt = text_hidden + (b * half + s) * H;
    } else {
      const long id = input_ids[p];
      if (id >= 0 && id < kg_rows) xk = kg_table + id * H;
    }
    const bf16* g_row = dsum + r * ld;
    float dot = 0.f, sq = 0.f;
    for (int c = lane; c < nch; c += 64) {
      const bf16x8 gv = *(const bf16x8*)(g_row + c * 8);
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        g[j] = scale * (float)gv[j];
        sq += g[j] * g[j];
      }
      if (xt) {
        const bf16x8 xv = *(const bf16x8*)(xt + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += g[j] * (float)xv[j];
      } else if (xk) {
        const f32x4 a = *(const f32x4*)(xk + c * 8);
        const f32x4 d = *(const f32x4*)(xk + c * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) dot += g[j] * a[j] + g[4 + j] * d[j];
      }
      if (go) {
        const f32x4 o0 = {g[0], g[1], g[2], g[3]}, o1 = {g[4], g[5], g[6], g[7]};
        *(f32x4*)(go + c * 8) = o0;
        *(f32x4*)(go + c * 8 + 4) = o1;
      }
    }
    dot = wave_sum(dot);
    sq = wave_sum(sq);
    if (lane == 0) {
      if (grad_x_input) grad_x_input[p] = dot;
      if (grad_norm) grad_norm[p] = sqrtf(sq);
    }
  }
}

}  // namespace

extern "C" int stonk_input_attribution(const void* dsum, int64_t ld, const int64_t* input_ids, const void* text_hidden,
                                       const float* kg_table, int64_t kg_rows, const int* row_of_pos, float scale,
                                       float* grad_x_input, float* grad_norm, float* grad_out, int64_t ld_out, int B,
                                       int S, int half, int H, void* stream) {
  STONK_CHECK_ARG(dsum && input_ids && text_hidden && kg_table && (grad_x_input || grad_norm), STONK_EINVAL);
  STONK_CHECK_ARG(B >= 0 && S > 0 && H > 0 && H % 8 == 0 && H <= 4096 && half >= 0 && half <= S && kg_rows > 0 && ld >= H,
                  STONK_ESHAPE);
  STONK_CHECK_ARG(!grad_out || ld_out >= H, STONK_ESHAPE);
  STONK_CHECK_ARG((uintptr_t)dsum % 16 == 0 && (uintptr_t)text_hidden % 16 == 0 && (uintptr_t)kg_table % 16 == 0 &&
                      ld % 8 == 0,
                  STONK_EALIGN);
  STONK_CHECK_ARG(!grad_out || ((uintptr_t)grad_out % 16 == 0 && ld_out % 4 == 0), STONK_EALIGN);
  if (B == 0) return STONK_OK;
  const long npos = (long)B * S;
  const long g = (npos + 3) / 4;
  hipLaunchKernelGGL(input_attribution_kernel, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)dsum, (long)ld, (const long*)input_ids, (const bf16*)text_hidden, kg_table,
                     (long)kg_rows, row_of_pos, scale, grad_x_input, grad_norm, grad_out, (long)ld_out, npos, S, half, H);
  return stonk_launch_status();
}

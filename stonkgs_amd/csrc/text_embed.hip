// Text-only BERT (the NLP baseline, ref:src/stonkgs/models/nlp_baseline_model.py): the one kernel STonKGs itself never
// needed - the gradient of a TRAINABLE word-embedding lookup. (The forward is stonk_joint_embed_ln_fwd with half = 0 and
// the fp32 word table in the place of the entity table: csrc/norm.hip.)
//
// d(word_embeddings)[id, :] += d(embedding sum)[row of position p, :] for every position p whose token is id - the
// backward of nn.Embedding(V, H, padding_idx) as BertEmbeddings uses it (hf:models/bert/modeling_bert.py:98-108): the
// padding row never receives a gradient.
//
// One wavefront per position. A lane reads 8 consecutive bf16 of the source row (16 bytes), the wave turns the 512
// columns it holds through a 1 KiB slice of LDS, and every atomic wave-instruction then adds 64 consecutive floats = 256
// contiguous bytes of ONE destination row (the shape global float atomics run at full rate in; one lane per row is an
// order of magnitude slower). The adds are no-return global_atomic_add_f32: the sum stays in fp32, its last bits depend
// on the arrival order - as the split-K weight gradients' already do.
#include "common.h"

namespace {

constexpr int WEG_WAVES = 4;      // wavefronts (= positions in flight) per workgroup
constexpr int WEG_CHUNK = 512;    // columns a wave holds at a time: 64 lanes x 8 bf16

__global__ __launch_bounds__(64 * WEG_WAVES) void word_embed_grad_kernel(
    const bf16* __restrict__ dsum, long ld, const long* __restrict__ input_ids, const int* __restrict__ row_of_pos,
    float* __restrict__ dword, long ld_w, long vocab, int padding_idx, long n_pos, int H, int* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) bf16 turn[WEG_WAVES][WEG_CHUNK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bf16* mine = turn[wave];   // this wave's slice: written and read by this wave alone (LDS operations of one wave are in order)
  for (long p = (long)blockIdx.x * WEG_WAVES + wave; p < n_pos; p += (long)gridDim.x * WEG_WAVES) {
    const long r = row_of_pos ? (long)row_of_pos[p] : p;   // packed layout: a dropped position has no row
    if (r < 0) continue;
    const long id = input_ids[p];
    if (id == padding_idx) continue;                        // (padding_idx = -1: no padding row)
    if (id < 0 || id >= vocab) {                            // torch's embedding raises IndexError; nothing is touched
      if (lane == 0) atomicOr(err, 1);
      continue;
    }
    const bf16* src = dsum + r * ld;
    float* dst = dword + id * ld_w;
    for (int c0 = 0; c0 < H; c0 += WEG_CHUNK) {
      const int c = c0 + 8 * lane;
      if (c < H) *(bf16x8*)(mine + 8 * lane) = *(const bf16x8*)(src + c);   // (H % 8 == 0: whole vectors)
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < WEG_CHUNK / 64; ++j) {
        const int col = c0 + 64 * j + lane;
        if (col < H) atomicAdd(dst + col, (float)mine[64 * j + lane]);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace

extern "C" int stonk_word_embed_grad(const void* dsum, int64_t ld, const int64_t* input_ids, const int* row_of_pos,
                                     float* dword, int64_t ld_w, int64_t vocab, int padding_idx, int B, int S, int H,
                                     int* err_flag, void* stream) {
  STONK_CHECK_ARG(dsum && input_ids && dword && err_flag, STONK_EINVAL);
  STONK_CHECK_ARG(B >= 0 && S > 0 && H > 0 && H % 8 == 0 && H <= 4096 && ld >= H && ld_w >= H && vocab > 0 &&
                      padding_idx < vocab && (long)B * S < (1L << 31),
                  STONK_ESHAPE);
  STONK_CHECK_ARG((uintptr_t)dsum % 16 == 0 && ld % 8 == 0 && (uintptr_t)dword % 4 == 0, STONK_EALIGN);
  if (B == 0) return STONK_OK;
  const long n_pos = (long)B * S;
  hipLaunchKernelGGL(word_embed_grad_kernel, dim3(grid_cap(n_pos, WEG_WAVES, 8192)), dim3(64 * WEG_WAVES), 0,
                     (hipStream_t)stream, (const bf16*)dsum, (long)ld, (const long*)input_ids, row_of_pos, dword, (long)ld_w,
                     (long)vocab, padding_idx, n_pos, H, err_flag);
  return stonk_launch_status();
}

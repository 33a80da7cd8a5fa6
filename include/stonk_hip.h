/* stonk_hip.h - C ABI of libstonk_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the STonKGs
 * pre-training hot path (STonKGsForPreTraining forward / backward / optimizer step).
 *
 * The reference (stonkgs v0.1.6-dev) has no FFI of its own: its hot path is a Python nn.Module whose
 * arithmetic is issued by HuggingFace `modeling_bert` into torch ATen. This header is therefore the
 * boundary a maintainer would bind (ctypes) to replace those ATen calls; every entry
 * cites the reference / HF site it replaces ("ref:" = /root/reference, "hf:" = transformers).
 *
 * Conventions:
 *  - plain pointers and sizes only; all pointers are DEVICE addresses unless stated; bf16 = 16-bit brain
 *    float stored as uint16_t; "ld*" are row strides in ELEMENTS;
 *  - every launcher is asynchronous on `stream` (a hipStream_t passed as void*), allocates nothing, keeps no
 *    global state (a launcher that needs scratch memory takes a caller workspace and has a `*_workspace_floats` query),
 *    never throws; it returns 0 on success, <0 for a rejected argument (STONK_E*), >0 for a
 *    hipError_t raised by the launch;
 *  - dropout masks are regenerated from (seed, element index) by a counter-based hash, never stored.
 */
#ifndef STONK_HIP_H
#define STONK_HIP_H
#include <stdint.h>
#include "../stonkgs_amd/csrc/stonk_flags.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STONK_OK 0
#define STONK_EINVAL (-1) /* null pointer / inconsistent argument */
#define STONK_ESHAPE (-2) /* unsupported shape */
#define STONK_EALIGN (-3) /* pointer or stride not aligned as required */

int stonk_abi_version(void);

/* C[M,N] = epilogue(alpha * A[M,K] . B[N,K]^T), A/B bf16, fp32 accumulate on MFMA. N % 128 == 0, K % 64 == 0.
 * `flags`: STONK_EPI_* (output type, bias, GELU, residual, saved pre-activation, GELU', dropout). STONK_EPI_AUX_GRAD
 * modifies the two users of `aux`: SAVE_PREACT (next to GELU) then stores gelu'(pre-activation) and GELU_BWD multiplies
 * by `aux` as is - the training step uses the pair, so the erf/exp of GELU' are evaluated once, in the forward epilogue.
 * m_dev / k_dev (nullable): effective M / K read from device memory at run time (label-sparse decoders).
 * `kernel`: STONK_GEMM_AUTO (the launcher picks one of its kernels from shape and epilogue), an explicit
 * STONK_GEMM_TILE128 / _WAVE8 / _WAVE4 / _WAVE4_192 / _ASM4 / _ASM4_192 (an explicit kernel that cannot take the arguments
 * is refused with STONK_ESHAPE; stonk_flags.h says what each takes), or STONK_GEMM_DISPATCHED / _DISPATCHED2: AUTO's choice without a persistent grid (one / two work items per
 * workgroup), for launches that run while another stream - a collective - holds CUs.
 * Replaces torch addmm/mm of hf:models/bert/modeling_bert.py:154-156 (Q,K,V), :289-293 (attn out), :334-337
 * (FFN up + GELU), :347-351 (FFN down), :476-480 (head transform); ref:src/stonkgs/models/stonkgs_model.py:70-71
 * (text / entity decoders) and their autograd backward. */
int stonk_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                       int flags, const float* bias, const void* resid, int64_t ldr, void* aux, int64_t ldaux,
                       float alpha, int split_k, const int* m_dev, const int* k_dev, float drop_p, uint32_t seed,
                       int kernel, void* stream);

/* Weight / bias gradient straight from row-major activations: dW[M',N'] += alpha * dY[T,M']^T . X[T,N'],
 * db[M'] += alpha * colsum(dY) (nullable). M', N' % 128 == 0; rows of dY / X in [k, roundup64(k)) must read as zero when
 * the token count k (<= K) comes from k_dev (the 256x256 kernels range-check tokens themselves). split_k >= 1: 128x128
 * tiles with that many K splits; split_k == 0: the four-wave 256x256 kernel (M', N' >= 256, lda / ldb % 64 == 0) with an
 * automatic split over all CUs; split_k <= -16: the same kernel held to -split_k CUs' worth of workgroups (launches on
 * a second stream beside other work); split_k == -1: the older eight-wave 256x256 form.
 * Autograd's weight/bias gradients of every nn.Linear on the path. */
int stonk_gemm_tn_bf16(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW, int64_t ldc, float* dbias,
                       int M, int N, int K, float alpha, int split_k, const int* k_dev, void* stream);
/* Up to 4 accumulating weight-gradient launches of the four-wave 256x256 kernel as ONE launch: gradients whose operands are
 * ready together share the CUs, so each is split over fewer K shares (fewer float atomics per element of dW). `problems` is
 * a HOST array of n descriptors (fields as the arguments of stonk_gemm_tn_bf16; read before the call returns). Per problem:
 * M', N' % 256 == 0, lda / ldb % 64 == 0, ldc >= N', M' * ldc * 4 < 2^31, else STONK_ESHAPE. cu_cap: the CUs' worth of
 * workgroups the launch may take (1 .. 1024; 0 = every CU of the device). One K split for all: the largest with
 * sum(tiles) * split <= cu_cap and split <= (K tiles of a problem) / 8 for every problem. n > 4, or more 256x256 tiles in
 * all than cu_cap: STONK_ESHAPE - launch the members one by one. The result differs from n stonk_gemm_tn_bf16 launches only
 * in the order of the fp32 additions. */
typedef struct StonkTnProblem {
  const void* dY; int64_t lda;
  const void* X; int64_t ldb;
  float* dW; int64_t ldc;
  float* dbias;
  const int* k_dev;
  int M, N, K;
  float alpha;
} StonkTnProblem;
int stonk_gemm_tn_bf16_group(const StonkTnProblem* problems, int n, int cu_cap, void* stream);
/* The same product STORED: dW = alpha * dY^T . X, db = alpha * colsum(dY) - whatever dW / db held before is overwritten,
 * and every element is defined even when *k_dev == 0 (zeros). Only for a launch that stonk_gemm_tn_bf16's routing leaves
 * with ONE K split (split_k == 1, or a split_k <= 0 whose automatic split comes out as 1; not -1): one producer per
 * element, so the result equals the accumulating form into zeros bit for bit. Anything else returns STONK_ESHAPE. Also
 * required: ldc >= N' and M' * ldc * 4 < 2^31 (32-bit byte offsets of the 256x256 kernel's stores), and with split_k <= 0
 * a bias only when N' <= 256 (that kernel shares the bias sums out over its column tiles), else STONK_ESHAPE. */
int stonk_gemm_tn_bf16_store(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW, int64_t ldc, float* dbias,
                             int M, int N, int K, float alpha, int split_k, const int* k_dev, void* stream);
/* stonk_gemm_tn_bf16_store (same routing, same refusals) that also leaves, for every output tile of the kernel it routes
 * to - 256x256 with split_k <= 0, else 128x128 - the sum of the squares of the values it stored (after the multiplication
 * by alpha; rows >= M' and columns >= N' of an edge tile are not stored and not counted):
 * tile_sumsq[row_tile * col_tiles + col_tile]. Every slot is written by every launch, zeros when *k_dev leaves no K tile: the
 * caller zeroes nothing. The order of summation inside a tile is fixed, so a slot depends on the inputs alone - not on the
 * grid, not on the launch. n_slots < the tile count: STONK_EINVAL. A gradient-norm pass takes the slots as the `extra` of
 * stonk_sumsq_f32_plus instead of reading dW back.
 * stonk_gemm_tn_store_tiles: that tile count for a shape and split_k, or the (negative) status with which the store entry
 * refuses the shape; nothing is launched. */
int stonk_gemm_tn_bf16_store_sumsq(const void* dY, int64_t lda, const void* X, int64_t ldb, float* dW, int64_t ldc,
                                   float* dbias, int M, int N, int K, float alpha, int split_k, const int* k_dev,
                                   float* tile_sumsq, int64_t n_slots, void* stream);
int64_t stonk_gemm_tn_store_tiles(int M, int N, int K, int split_k);

/* y = dropout(LayerNorm(x)); x,y bf16 [rows,H]; gamma/beta fp32; mean/rstd fp32 [rows] saved for backward.
 * Replaces nn.LayerNorm(eps=1e-12) + nn.Dropout at hf:modeling_bert.py:106-107, :291-292, :349-350, :479. */
int stonk_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                        int64_t rows, int H, float eps, int flags, float drop_p, uint32_t seed, void* stream);

/* dx = LayerNorm'(dy) (dy first masked by the forward's output dropout when STONK_LN_DROPOUT);
 * dx_drop (nullable) = dropout-masked copy of dx for the branch that went through nn.Dropout before the residual
 * add; dgamma/dbeta (fp32, nullable) are ACCUMULATED - through per-workgroup partials when a workspace of
 * >= 1024 * 2 * H floats is passed (nullable: falls back to atomics). Autograd backward of the sites above.
 * stonk_layernorm_bwd_workspace_floats(rows, H) is the size to pass (the only launcher that takes a workspace). */
int64_t stonk_layernorm_bwd_workspace_floats(int64_t rows, int H);
int stonk_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                        void* dx, void* dx_drop, float* dgamma, float* dbeta, int64_t rows, int H, int flags,
                        float drop_p_in, uint32_t seed_in, float drop_p_out, uint32_t seed_out, float* partial_ws,
                        int64_t ws_floats, void* stream);
/* With STONK_LN_DEFER_REDUCE in `flags` (workspace required) stonk_layernorm_bwd leaves the per-workgroup dgamma / dbeta
 * partial sums in `partial_ws`; this adds them into dgamma / dbeta - same `rows` and `H` as that call - on any stream
 * ordered after it. The training step runs it on its weight-gradient stream: only the optimizer waits for these two
 * vectors (autograd accumulates them at the same point: hf:modeling_bert.py:107 / :292 / :350 / :479 backward). */
int stonk_layernorm_bwd_reduce(const float* partial_ws, int64_t rows, int H, float* dgamma, float* dbeta, void* stream);

/* inputs_embeds + position + token-type embeddings -> LayerNorm -> dropout, in one pass:
 *   row (b,s<half)  = text_hidden[b*half+s]          (frozen LM backbone output, bf16)
 *   row (b,s>=half) = kg_table[input_ids[b,s]]       (fp32 node2vec table; ids 100/102/103 = LM special vectors)
 * Replaces the Python gather loop, torch.stack/cat and the CPU fp32 round trip of
 * ref:src/stonkgs/models/stonkgs_model.py:182-200 plus BertEmbeddings hf:modeling_bert.py:98-108.
 * An id outside [0, kg_rows) sets bit 0 of *err_flag (the reference raises KeyError at :185).
 * pos_of_row (nullable) / n_rows: the PACKED layout of stonk_unpad_plan - output row i (i < n_rows) is padded position
 * pos_of_row[i]; rows whose entry is -1 (the tail up to n_rows) are written as zeros with mean 0, rstd 1. */
int stonk_joint_embed_ln_fwd(const int64_t* input_ids, const int64_t* token_type_ids, const void* text_hidden,
                             const float* kg_table, const float* pos_emb, const float* type_emb, const float* gamma,
                             const float* beta, void* sum_out, void* y, float* mean, float* rstd, int B, int S,
                             int half, int H, int64_t kg_rows, int type_rows, float eps, int flags, float drop_p,
                             uint32_t seed, int* err_flag, const int* pos_of_row, int64_t n_rows, void* stream);

/* Frozen LM backbone embeddings: word_emb[input_ids[:, :S]] + pos + type[0] -> LayerNorm -> dropout.
 * Replaces BertEmbeddings of `self.lm_backbone(input_ids[:, :half])`, ref:stonkgs_model.py:178. */
int stonk_text_embed_ln_fwd(const int64_t* input_ids, int64_t ld_ids, const float* word_emb, const float* pos_emb,
                            const float* type_emb, const float* gamma, const float* beta, void* y, int B, int S, int H,
                            int64_t vocab, float eps, int flags, float drop_p, uint32_t seed, int* err_flag,
                            void* stream);

/* d(position_embeddings) and d(token_type_embeddings) from d(embedding sum) (bf16 [B*S,H]); accumulates.
 * row_of_pos (nullable): packed layout - dx row of padded position p is row_of_pos[p], -1 = dropped (no gradient).
 * token_type_ids (nullable: every position is type 0). type_rows is 1 or 2 - with 1, row 1 of dtype is not touched; more
 * type rows are refused (STONK_ESHAPE): the kernel keeps sums for rows 0 and 1 only. H % 8 == 0, H <= 1024. */
int stonk_embed_grad(const void* dx, const int64_t* token_type_ids, float* dpos, float* dtype, int B, int S, int H,
                     int type_rows, const int* row_of_pos, void* stream);

/* BigBird's embeddings on given inputs_embeds: y = LayerNorm(dropout(inputs_embeds + token_type + position)) - the dropout
 * BEFORE the LayerNorm (BERT's order is the opposite). Replaces hf:models/big_bird/modeling_big_bird.py BigBirdEmbeddings
 * :120-128 with inputs_embeds given and rescale_embeddings off. inputs_embeds fp32 [B*S, ld_in]; token_type_ids int64 [B,S]
 * or NULL (every position type 0; the launcher has no error word: an id outside [0, type_rows) reads row 0, the caller
 * checks); pos_emb fp32 [>= S, H], type_emb fp32 [type_rows, H]. sum_out bf16 [B*S, H]: the LayerNorm's input AFTER the
 * dropout (what stonk_layernorm_bwd takes as x); y bf16 [B*S, H]; mean / rstd fp32 [B*S], from the fp32 values. The mask is
 * the element form of the generator at (row, column) = (output row, column), scale 1 / (1 - drop_p), as at the
 * STONK_LN_DROPOUT site; drop_p == 0 keeps everything.
 * Refused: a null pointer other than token_type_ids, drop_p outside [0, 1) (STONK_EINVAL); B < 0, S <= 0, H <= 0, H % 8,
 * H > 1024, ld_in < H, type_rows <= 0, B * S >= 2^31 (STONK_ESHAPE); ld_in % 4, inputs_embeds / pos_emb / type_emb / gamma /
 * beta / sum_out / y not 16-byte aligned (STONK_EALIGN). B == 0 returns STONK_OK. */
int stonk_embeds_ln_fwd(const float* inputs_embeds, int64_t ld_in, const int64_t* token_type_ids, const float* pos_emb,
                        const float* type_emb, const float* gamma, const float* beta, void* sum_out, void* y, float* mean,
                        float* rstd, int B, int S, int H, int type_rows, float eps, float drop_p, uint32_t seed, void* stream);
/* The end of its backward (the backward of :127, nn.Dropout, and of the two adds): dsum bf16 [n_rows, ld] = d(sum_out) from
 * stonk_layernorm_bwd; the mask of (drop_p, seed) is regenerated and g = keep ? dsum / (1 - drop_p) : 0 is written twice:
 * d_inputs_embeds fp32 [n_rows, ld_out] and dx_masked bf16 [n_rows, H], which stonk_embed_grad turns into the position and
 * token-type gradients. Refused: a null pointer, drop_p outside [0, 1) (STONK_EINVAL); n_rows < 0 or >= 2^31, H <= 0, H % 8,
 * H > 1024, ld < H, ld_out < H (STONK_ESHAPE); ld % 8, ld_out % 4, a pointer not 16-byte aligned (STONK_EALIGN).
 * n_rows == 0 returns STONK_OK. */
int stonk_embeds_ln_bwd_finish(const void* dsum, int64_t ld, float* d_inputs_embeds, int64_t ld_out, void* dx_masked,
                               int64_t n_rows, int H, float drop_p, uint32_t seed, void* stream);

/* Gradient of a TRAINABLE word-embedding lookup (csrc/text_embed.hip): the text-only BERT of
 * ref:src/stonkgs/models/nlp_baseline_model.py:171-173 trains `bert.embeddings.word_embeddings.weight`, which STonKGs
 * leaves dead. Replaces the backward of nn.Embedding(V, H, padding_idx) in BertEmbeddings, hf:models/bert/modeling_bert.py:98-108
 * (torch's embedding_dense_backward). dsum: bf16 [rows, H] with row stride ld - the input gradient of the embeddings LayerNorm
 * (what the backward of stonk_joint_embed_ln_fwd produces). For padded position p = b*S + s: r = row_of_pos ? row_of_pos[p] : p
 * (row_of_pos nullable: the packed layout of stonk_unpad_plan); r < 0 (dropped) and input_ids[p] == padding_idx (-1 = no padding
 * row) contribute nothing; an id outside [0, vocab) sets bit 0 of *err_flag and touches no memory; otherwise
 * dword[id, :] += float(dsum[r, :]) (fp32 [vocab, H] with row stride ld_w). ACCUMULATES (gradient accumulation; the optimizer
 * zeroes the buffer). One wavefront per position, 16-byte loads, no-return fp32 atomics of 256 contiguous bytes per
 * wave-instruction: the sum's last bits depend on the arrival order. Refused before any launch: dsum / input_ids / dword /
 * err_flag null (STONK_EINVAL); H % 8, H > 4096, ld < H, ld_w < H, vocab <= 0, padding_idx >= vocab, S <= 0, B * S >= 2^31
 * (STONK_ESHAPE); dsum not 16-byte aligned, ld % 8, dword not 4-byte aligned (STONK_EALIGN). B == 0 returns STONK_OK. */
int stonk_word_embed_grad(const void* dsum, int64_t ld, const int64_t* input_ids, const int* row_of_pos, float* dword,
                          int64_t ld_w, int64_t vocab, int padding_idx, int B, int S, int H, int* err_flag, void* stream);

/* Input attributions from d F / d(embedding sum) (csrc/input_attribution.hip). The reference has no call for this: the
 * nearest is autograd with respect to the `inputs_embeds` of ref:src/stonkgs/models/stonkgs_model.py:193-210, which a
 * reference user reaches only by patching `forward` (the tensor is built inside it from ids). dsum: bf16 [rows, H] with row
 * stride ld - the input gradient of the embeddings LayerNorm; with dropout off it equals d F / d inputs_embeds, the sum being
 * inputs_embeds + position + token-type. For padded position p = b*S + s: r = row_of_pos ? row_of_pos[p] : p (row_of_pos
 * nullable: the packed layout of stonk_unpad_plan); r < 0 (dropped: nothing read the position) writes exactly 0 to all three
 * outputs; otherwise g = scale * float(dsum[r,:]), x = text_hidden[b*half + s,:] (bf16) for s < half, else
 * kg_table[input_ids[b,s],:] (fp32), and grad_x_input[p] = sum_h g_h x_h, grad_norm[p] = sqrt(sum_h g_h^2) (fp32 [B*S] each,
 * at least one non-null), grad_out[p,:] = g (nullable, fp32 [B*S, H] with row stride ld_out, padded layout). An entity id
 * outside [0, kg_rows) reads no memory and counts as x = 0 (stonk_joint_embed_ln_fwd has set bit 0 of its error word).
 * fp32 accumulation, one wavefront per position, no atomics, no workspace: bitwise repeatable. Refused before any launch:
 * a null required pointer or both scalar outputs null (STONK_EINVAL); H % 8, H > 4096, half outside [0, S], kg_rows <= 0,
 * ld < H, ld_out < H with grad_out (STONK_ESHAPE); dsum / text_hidden / kg_table / grad_out not 16-byte aligned, ld % 8 or
 * ld_out % 4 (STONK_EALIGN). B == 0 returns STONK_OK. */
int stonk_input_attribution(const void* dsum, int64_t ld, const int64_t* input_ids, const void* text_hidden,
                            const float* kg_table, int64_t kg_rows, const int* row_of_pos, float scale,
                            float* grad_x_input, float* grad_norm, float* grad_out, int64_t ld_out, int B, int S, int half,
                            int H, void* stream);

/* Row plan of the unpadded trainable encoder. A padded text position is never a key, and its output is read only if it
 * carries a label (the reference labels 15 % of the PADDED half, ref:src/stonkgs/data/indra_for_pretraining.py:33-77) or
 * is position 0 (the pooler's input): every other padded row can be dropped without changing a loss term or a gradient
 * of ref:src/stonkgs/models/stonkgs_model.py:204-245. Kept: attention_mask != 0, s == 0, text_labels[b,s] != -100
 * (s < half), ent_labels[b,s-half] != -100 (labels nullable); a sequence WITHOUT any unmasked key keeps all S positions
 * (the reference then attends uniformly over them). Outputs (int32 unless stated, device): row_of_pos [B*S] (-1 =
 * dropped), pos_of_row [B*S] (-1 past the total), seq_offsets [B+1] ([B] = total; the `seq_offsets` of
 * stonk_attention_*), row_mask int64 [B*S] (attention_mask per packed row, 0 past the total).
 * Optionally (all three or none) the READ rows - the packed rows whose last-layer output something reads (labelled
 * positions: the decoders; position 0: the pooler), on which alone the last layer's row-wise feed-forward block, the pooler
 * and the head transform need to run: read_rows [B*S] (packed row of the j-th read row, -1 past their count),
 * read_of_pos [B*S] (index into read_rows of a padded position, or -1), read_offsets [B+1] ([B] = their count;
 * read_rows[read_offsets[b]] is position 0 of sequence b). workspace: device ints, stonk_unpad_workspace_ints(B) of them
 * (= 3 B; it need not be zeroed). `half` is an argument of its own, 0 <= half <= S: a text label is read iff s < half, an
 * entity label iff half <= s < 2 half (both label arrays are [B, half]); positions from 2 half on are kept by their mask
 * word alone, and with half == 0 (the text-only baseline) neither label pointer is read. Any mask word != 0 is live;
 * row_mask carries the raw word. A sequence's packed rows are its read rows in position order, then its other kept rows
 * in position order.
 * Refused before any launch, in this order: attention_mask / row_of_pos / pos_of_row / seq_offsets / row_mask / workspace
 * null, or some but not all of the three read outputs given (STONK_EINVAL); B < 0, S <= 0, half < 0, half > S,
 * B S >= 2^31 (STONK_ESHAPE); ws_ints < 3 B (STONK_EINVAL). B == 0 returns STONK_OK. */
int64_t stonk_unpad_workspace_ints(int B);
int stonk_unpad_plan(const int64_t* attention_mask, const int64_t* text_labels, const int64_t* ent_labels, int B, int S,
                     int half, int* row_of_pos, int* pos_of_row, int* seq_offsets, int64_t* row_mask, int* read_rows,
                     int* read_of_pos, int* read_offsets, int* workspace, int64_t ws_ints, void* stream);

/* Fused attention, head_dim 64, S % 128 == 0, S <= 4096: out = dropout(softmax(q k^T * scale + mask)) v.
 * q/k/v: column slices of the [T, 3H] projection (row stride ld), head h at columns h*64..; attention_mask int64
 * [B,S] (0 = masked key) or NULL; lse fp32 [B,NH,S]. Replaces hf:modeling_bert.py:188-203 (eager :111-136).
 * A masked key has probability exactly 0 and gets exactly zero dk / dv - unless NO key of a sequence is unmasked: the
 * sequence then attends uniformly over its own rows, P = 1/n with n = S (padded) or the sequence's length (packed), as
 * the eager path does once finfo.min has absorbed every score; forward and backward agree on that at every S, dq / dk /
 * dv are those of the formulas with that P, and the sequence's lse entries are finite, about -2^100 * scale, and
 * meaningless.
 * PACKED layout (seq_offsets != NULL, int32 [B+1], device): sequence b is rows seq_offsets[b] .. seq_offsets[b+1]-1 of
 * q/k/v/out (any length <= S, no alignment), attention_mask is then REQUIRED and holds one word per packed ROW; lse (and
 * delta_ws) keep the [B,NH,S] layout. What the trainable encoder runs on once the rows that nothing reads - padding that
 * is neither a live key nor a labelled position - are dropped (stonk_unpad_plan); rows outside every sequence are never
 * read or written. q_offsets (nullable, int32 [B+1], packed layout only): sequence b's QUERIES are its first
 * q_offsets[b+1] - q_offsets[b] rows (its keys: all of them) - out / lse / dq are written for those rows only, dk / dv
 * receive their contributions only. The last encoder layer's form: stonk_unpad_plan puts a sequence's read rows first. */
int stonk_attention_fwd(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask,
                        const int* seq_offsets, const int* q_offsets, void* out, int64_t ldo, float* lse, int B, int NH,
                        int S, int D, float scale, float drop_p, uint32_t seed, void* stream);
/* Backward of the above (recomputes P from lse; no atomics). delta_ws: fp32 [B,NH,S] scratch. With q_offsets, dq rows
 * past a sequence's queries are NOT written (zero them if something reads them) and dout rows past them must be finite. */
int stonk_attention_bwd(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask,
                        const int* seq_offsets, const int* q_offsets, const void* out, int64_t ldo, const void* dout,
                        int64_t lddo,
                        const float* lse, float* delta_ws, void* dq, void* dk, int64_t ldd, void* dv, int B, int NH,
                        int S, int D, float scale, float drop_p, uint32_t seed, void* stream);

/* The same in separately launched parts (`phases`: STONK_ATTN_BWD_DELTA | _DQ | _DKV), so that the dQ and the dK / dV
 * kernels - independent once delta = rowsum(dO * O) exists - can be put on two streams: run DELTA first, order the DKV
 * call's stream after it, then DQ and DKV in any order or side by side. phases = STONK_ATTN_BWD_ALL is stonk_attention_bwd. */
int stonk_attention_bwd_phases(int phases, const void* q, const void* k, const void* v, int64_t ld,
                               const int64_t* attention_mask, const int* seq_offsets, const int* q_offsets, const void* out,
                               int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta_ws, void* dq,
                               void* dk, int64_t ldd, void* dv, int B, int NH, int S, int D, float scale, float drop_p,
                               uint32_t seed, void* stream);

/* Block-sparse (BigBird) attention, head_dim 64, block size 64, padded layout only, no dropout (csrc/bigbird_attention.hip).
 * Replaces hf:models/big_bird/modeling_big_bird.py:295-744 (BigBirdBlockSparseAttention.bigbird_block_sparse_attention)
 * on every query row whose own mask is 1; a masked position as a query still gets a row, by the rule below.
 * q/k/v: column slices of the [B*S, 3H] projection (row stride ld >= 3 NH 64), head h at columns h*64..; attention_mask
 * int64 [B,S] (0 = masked key) or NULL; out bf16 [B*S, ldo]; lse fp32 [B,NH,S]. nb = S / 64 blocks per sequence.
 * LISTS (device int32): key_blocks / key_mult [NH, nb, nb], key_count [NH, nb] - the first key_count[h][i] entries (j, m)
 * of row (h, i) are the key blocks the queries of block i of head h attend to and their multiplicities. The 64 queries of
 * a block take ONE softmax over the keys of the listed blocks, a key of an entry (j, m) counting m times (HuggingFace
 * concatenates the gathered blocks and does not remove duplicates): l += m sum exp, O += m P V, lse includes the m.
 * stonkgs_amd/bigbird_attention.py builds BigBird's lists (global, window and random blocks) and their inverses.
 * A masked key has probability exactly 0 and gets exactly zero dk / dv - unless ALL listed keys of a query block are
 * masked: its rows then attend uniformly over the listed keys, weighted by multiplicity (the dense kernels' rule, per
 * block; forward and backward agree, the block's lse entries are finite, about -2^100 * scale, and meaningless).
 * The launcher cannot read the lists: a count outside [0, nb] (the list counts as empty), an entry outside [0, nb) or a
 * multiplicity <= 0 (the entry is skipped) touches no memory through the bad value and sets bit 0 of *err_flag; a block
 * without a valid entry writes zeros. Each list array must hold the full [NH, nb, nb] / [NH, nb] extent.
 * Refused before any launch: q / k / v / a list / out / lse / err_flag null, scale <= 0 (STONK_EINVAL); D != 64, S % 64,
 * S < 320, S > 4096, NH <= 0, B < 0, ld < 3 NH 64, ldo < NH 64 (STONK_ESHAPE); ld % 8, ldo % 4, q / k / v not 16-byte
 * aligned, out not 8-byte aligned (STONK_EALIGN). B == 0 returns STONK_OK. */
int stonk_block_sparse_attention_fwd(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask,
                                     const int* key_blocks, const int* key_mult, const int* key_count, void* out, int64_t ldo,
                                     float* lse, int B, int NH, int S, int D, float scale, int* err_flag, void* stream);
/* Backward of the above: recomputes P from lse, three launches (row statistics, dq, dk / dv), no atomics, bitwise
 * repeatable. query_blocks / query_mult [NH, nb, nb], query_count [NH, nb]: the INVERSE lists - for key block j of head h
 * the query blocks that list it, with the multiplicity they list it with (the same multiset of pairs as the forward
 * lists; they fall under the same checks and the same err_flag bit). delta_ws: fp32 [2, B, NH, S] scratch (rowsum(dO * O),
 * then -lse in log2 units). dq / dk / dv: bf16, row stride ldd >= NH 64, every row of every sequence is written.
 * Refused as the forward, plus: a null inverse list / out / dout / lse / delta_ws / dq / dk / dv (STONK_EINVAL); lddo or
 * ldd < NH 64 (STONK_ESHAPE); ldo % 8, lddo % 8, ldd % 4, out / dout not 16-byte or dq / dk / dv not 8-byte aligned
 * (STONK_EALIGN). */
int stonk_block_sparse_attention_bwd(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask,
                                     const int* key_blocks, const int* key_mult, const int* key_count, const int* query_blocks,
                                     const int* query_mult, const int* query_count, const void* out, int64_t ldo,
                                     const void* dout, int64_t lddo, const float* lse, float* delta_ws, void* dq, void* dk,
                                     int64_t ldd, void* dv, int B, int NH, int S, int D, float scale, int* err_flag,
                                     void* stream);
/* The two entries above with `flags` (the entries above ARE these with flags = 0, bit for bit). One flag,
 * STONK_BSA_ZERO_MASKED_QUERIES: HuggingFace's rule for a masked QUERY. Replaces `context_layer = context_layer * from_mask`,
 * hf:models/big_bird/modeling_big_bird.py:617, and its backward - with the flag these entries replace :295-744 on EVERY row.
 * With the flag and a non-null attention_mask, for a position whose own mask word is 0:
 *   forward   its `out` row is exact zeros for every head (its lse entry is written as without the flag, finite);
 *   backward  its dout counts as zero: its dq row is exact zeros, it adds nothing to any dk / dv, its delta (delta_ws) is 0;
 *             a live row's dq is the flag-less run's, bit for bit.
 * A sequence without any live key therefore gets all-zero out, dq, dk and dv. The mask word is applied inside the kernels
 * (on the packed bits of the forward's final store; to delta and to the dO fragments and tiles in the backward, whose
 * arithmetic then yields the zeros by itself): no extra pass over [B*S, H], no atomics, bitwise repeatable. With a null attention_mask the flag changes nothing.
 * Refused as the entries above, plus: a bit of `flags` other than STONK_BSA_ZERO_MASKED_QUERIES (STONK_EINVAL).
 * B == 0 returns STONK_OK. */
int stonk_block_sparse_attention_fwd_ex(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask,
                                        const int* key_blocks, const int* key_mult, const int* key_count, void* out,
                                        int64_t ldo, float* lse, int B, int NH, int S, int D, float scale, int* err_flag,
                                        int flags, void* stream);
int stonk_block_sparse_attention_bwd_ex(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask,
                                        const int* key_blocks, const int* key_mult, const int* key_count,
                                        const int* query_blocks, const int* query_mult, const int* query_count, const void* out,
                                        int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta_ws, void* dq,
                                        void* dk, int64_t ldd, void* dv, int B, int NH, int S, int D, float scale,
                                        int* err_flag, int flags, void* stream);

/* P = softmax(q k^T * scale + key mask), written out. Forward-only, no dropout, PADDED layout only (csrc/attention_probs.hip).
 * q/k: column slices of the [B*S, 3H] projection (row stride ld), head h at columns h*64.. ; attention_mask int64 [B,S]
 * (0 = masked key) or NULL. probs (nullable): fp32 [B, NH, S, S], contiguous (HF `attentions` layout), 16-byte aligned.
 * modal_mass (nullable): fp32 [B, NH, S, 2]: per query row the probability mass on keys [0, half) and [half, S).
 * At least one of probs / modal_mass; probs == NULL skips the S x S stores. D == 64, S % 128 == 0, 128 <= S <= 4096,
 * 0 < half < S, half % 64 == 0, scale > 0. The forward kernel's semantics: a masked key gets exactly 0.0, masked positions
 * as queries still get a row, a sequence without any unmasked key attends uniformly (1/S). Two passes over the keys, no
 * lse input, no atomics (bitwise reproducible). Replaces hf:modeling_bert.py:111-136 as far as `attention_probs`. */
int stonk_attention_probs(const void* q, const void* k, int64_t ld, const int64_t* attention_mask, float* probs,
                          float* modal_mass, int B, int NH, int S, int D, int half, float scale, void* stream);

/* out[c][r] = in[r][c] (bf16). Rows >= *rows_dev (nullable) read as zero; colsum (nullable, fp32) += column sums
 * of `in` (bias gradients). Feeds wgrad operands to stonk_gemm_nt_bf16. */
int stonk_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int cols,
                         float* colsum, const int* rows_dev, void* stream);
int stonk_transpose_f32_to_bf16(const float* in, void* out, int64_t rows, int cols, int64_t ld_out, void* stream);
/* n bf16 transposes in ONE launch (the W^T copies of every weight after an optimizer step). desc_dev: device array of n
 * 56-byte entries {const void* in; void* out; int64 ld_in, ld_out, rows; int32 cols, first_tile, col_tiles, pad}, sorted
 * by first_tile; an entry covers ceil(rows/64) * col_tiles tiles of 64x64 (col_tiles = ceil(cols/64)), total_tiles = the
 * sum; cols % 8 == 0, ld_out >= roundup64(rows), rows past `rows` are written as zeros up to the tile edge. */
int stonk_transpose_bf16_batched(const void* desc_dev, int n, int total_tiles, void* stream);
int stonk_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);

/* On-device dynamic masking: ids_in [B,S] -> ids_out [B,S] + text / entity labels [B,half]. Per half,
 * exactly k_* positions (the reference uses int(half * 0.15)) chosen uniformly without replacement - padding included,
 * as the reference masks the padded sequence; 80 % -> mask_id, 10 % kept, 10 % uniform id in [0, vocab_*-1]; labels =
 * original id there, -100 elsewhere. Counter-based random stream (seed, row, half, position), restated bit for bit by
 * oracle/masking_oracle.py. Replaces ref:src/stonkgs/data/indra_for_pretraining.py:33-77 (replace_mlm_tokens), whose
 * own Mersenne-Twister draws stay reproducible on the host path (stonkgs_amd/data.py). Ids, labels and mask_id are
 * int64 words and pass through unchanged whatever their size; a random id is below vocab_* < 2^32. One workgroup per
 * (row, half) holds the half's keys in LDS: half <= 8192.
 * Refused before any launch, in this order: a null pointer (STONK_EINVAL); B < 0, half <= 0, S != 2 half, half > 8192
 * (STONK_ESHAPE); vocab_* <= 0 or >= 2^32 (STONK_EINVAL); k_* < 0 or > half (STONK_EINVAL). B == 0 returns STONK_OK. */
int stonk_mlm_mask(const int64_t* ids_in, int64_t* ids_out, int64_t* text_labels, int64_t* ent_labels, int B, int S,
                   int half, int64_t vocab_text, int64_t vocab_ent, int64_t mask_id, int k_text, int k_ent, uint32_t seed,
                   void* stream);

/* On-device row assembly: text_ids / text_attention [B,half] (already padded), source / target [B] node indices into
 * walks [n_nodes, walk_len] (2 * walk_len + 2 == half) -> ids_out / attention_out / type_out [B,S], nsp_out [B]. Entity
 * half = walks[source] [SEP] walks[target] [SEP]; with probability negative_rate a row takes the entity half of another
 * row of the batch and NSP label 1 (the reference appends 25 % such rows offline: the same 1 in 5). A node index outside
 * the table - of the row itself or of a negative's partner row - sets bit 0 of *err_flag (the reference raises KeyError)
 * and writes 0 at every entity position it feeds; the [SEP]s and every other element are written as usual. Replaces
 * ref:src/stonkgs/data/indra_for_pretraining.py:190-239 (row assembly) and :80-126 (negative NSP samples).
 * negative_rate is a FLOAT: row b is a negative iff B > 1 and its 32-bit draw is below
 * (uint32)((double)negative_rate * 2^32 + 0.5) - for 0.2f that is 858993472, not the 858993459 of the double 0.2; a
 * restatement must round the rate to float32 first. A negative's partner is drawn uniformly from [0, B); a row that
 * draws itself takes (b + 1) % B.
 * Refused before any launch, in this order: a null pointer (STONK_EINVAL); B < 0, half <= 0, S != 2 half,
 * 2 walk_len + 2 != half, n_nodes <= 0 (STONK_ESHAPE); negative_rate < 0 or >= 1 as a float (STONK_EINVAL). B == 0
 * returns STONK_OK. */
int stonk_assemble_rows(const int64_t* text_ids, const int64_t* text_attention, const int64_t* source,
                        const int64_t* target, const int64_t* walks, int64_t n_nodes, int walk_len, int64_t* ids_out,
                        int64_t* attention_out, int64_t* type_out, int64_t* nsp_out, int B, int S, int half,
                        int64_t sep_id, float negative_rate, uint32_t seed, int* err_flag, void* stream);

/* Labelled-row compaction for the MLM / ELM heads (labels != -100), count kept on the device.
 * rows_out[i] = b*S + offset + pos of the i-th labelled position - or, with row_of_pos (nullable; packed layout of
 * stonk_unpad_plan), that position's packed row. Semantics of nn.CrossEntropyLoss(ignore_index=-100) at
 * ref:stonkgs_model.py:229-240. */
int stonk_label_compact(const int64_t* labels, int64_t n, int half, int S, int offset, int* rows_out, int* targets_out,
                        int* count_out, const int* row_of_pos, void* stream);
int stonk_gather_rows_bf16(const void* src, int64_t ld_src, const int* rows, const int* count_dev, void* dst,
                           int64_t ld_dst, int cols, int64_t cap, void* stream);
int stonk_scatter_rows_bf16(const void* src, int64_t ld_src, const int* rows, const int* count_dev, void* dst,
                            int64_t ld_dst, int cols, void* stream);
int stonk_scatter_rows_f32_to_bf16(const float* src, int64_t ld_src, const int* rows, const int* count_dev, void* dst,
                                   int64_t ld_dst, int cols, void* stream);

/* Per labelled row: loss_sum += logsumexp(logits[row,:ncols]) - logits[row,target];
 * dlogits (bf16, nullable, cap_rows rows allocated) = (softmax - onehot) * grad_scale / count, rows
 * [count, roundup64(count)) zeroed. Bit 3 of *err_flag: target out of range. The sum is built in a fixed order (one share
 * per workgroup, added in double by the last workgroup to finish, then ONE addition to *loss_sum): the same bits on every
 * launch. The shares live in the library (16 sets used in turn): at most 16 of these launches may be in flight at once. */
int stonk_softmax_xent_fwd_bwd(const float* logits, int64_t ld, int ncols, int npad, const int* targets,
                               const int* count_dev, float* loss_sum, void* dlogits, int64_t ld_d, float grad_scale,
                               int cap_rows, int* err_flag, void* stream);

/* The same on fp16 logits (stonk_gemm_nt_bf16 with STONK_EPI_OUT_F16): 6 bytes of HBM traffic per logit instead of 10 -
 * the training step's label-sparse decoders use this pair; all arithmetic stays fp32. ld % 8 == 0. */
int stonk_softmax_xent_f16_fwd_bwd(const void* logits_f16, int64_t ld, int ncols, int npad, const int* targets,
                                   const int* count_dev, float* loss_sum, void* dlogits, int64_t ld_d, float grad_scale,
                                   int cap_rows, int* err_flag, void* stream);

/* Evaluation / masked prediction on the same label-sparse logits (the reference has no counterpart: it ranks a dense
 * [B,S,V] tensor in torch, which does not exist here). For every row r < min(*count_dev, cap_rows) - read on the device,
 * rows at or past it are not written - over the columns [0, ncols) only ([ncols, ld) is the decoder GEMM's padding and
 * influences nothing), in the total order "larger value first, lower column first among equal values":
 *   top_idx[r,0..k) / top_val[r,0..k): the k first columns and their RAW logits as fp32 (not log-probabilities);
 *   lse[r] = log sum exp over the valid columns (fp32, maximum subtracted);
 *   rank[r] = number of valid columns ordered before targets[r] (zero-based: columns with a larger value, plus columns
 *   with an equal value and a lower index); tgt_logit[r] = the target's logit.
 * targets nullable (then rank / tgt_logit are not touched and may be null; otherwise both are required). A target outside
 * [0, ncols) cannot be refused by the launcher (it lives on the device) and the entry takes no error word: that row gets
 * rank -1 and tgt_logit NaN, nothing is read out of bounds, and stonk_softmax_xent_* on the same targets - which the
 * engine runs first - sets bit 3 of its error word. 1 <= k <= 16 and k <= ncols, else STONK_ESHAPE; a null required
 * pointer or ld < ncols: STONK_EINVAL; both before any launch. Each logit is read once; no workspace, no atomics, the
 * same input gives the same bits. Rows that are 16-byte aligned (pointer and ld) are read in 16-byte pieces. */
int stonk_row_topk_f32(const float* logits, int64_t ld, int ncols, const int* targets, const int* count_dev, int cap_rows,
                       int k, float* top_val, int* top_idx, float* lse, int* rank, float* tgt_logit, void* stream);
int stonk_row_topk_f16(const void* logits_f16, int64_t ld, int ncols, const int* targets, const int* count_dev,
                       int cap_rows, int k, float* top_val, int* top_idx, float* lse, int* rank, float* tgt_logit,
                       void* stream);
/* NSP loss (ref:stonkgs_model.py:241-243): loss_sum_cnt[0] += sum, [1] += number of labels. */
int stonk_nsp_xent_fwd_bwd(const float* logits, const int64_t* labels, int B, int C, float* loss_sum_cnt, float* dlogits,
                           float grad_scale, int* err_flag, void* stream);
/* loss_out[0..3] = total, text MLM, entity MLM, NSP (ref:stonkgs_model.py:245). */
int stonk_loss_finalize(const float* text_sum, const int* text_cnt, const float* ent_sum, const int* ent_cnt,
                        const float* nsp_sum_cnt, float* loss_out, void* stream);

/* BertPooler / NSP classifier on fp32 master weights (hf:modeling_bert.py:457-463, :523-527). */
int stonk_small_linear_fwd(const void* x, int64_t ldx, const float* W, const float* bias, float* y, int M, int N, int K,
                           int act, void* stream);
int stonk_small_linear_bwd(const float* dy, const float* y, const void* x, int64_t ldx, const float* W, float* dW,
                           float* db, float* dx_f32, void* dx_bf16_accum, int64_t ld_dxb, int M, int N, int K, int act,
                           void* stream);

/* Classification head plumbing (ref:src/stonkgs/models/stonkgs_finetuning.py:310-330): dropout on the pooled fp32
 * vector (replayable from the seed), and *out = *num / *den for the mean of a device-side loss sum. */
int stonk_dropout_f32(const float* x, float* y, int64_t n, float p, uint32_t seed, void* stream);
int stonk_ratio_f32(const float* num, const float* den, float* out, void* stream);
/* The classification head's other two losses (ref:stonkgs_finetuning.py:328-338): `mode` = STONK_LOSS_MSE (regression,
 * nn.MSELoss), STONK_LOSS_MSE_BROADCAST (num_labels = 1 with 1-D labels: torch broadcasts [B,1] against [B] to [B,B], and
 * so does this), STONK_LOSS_BCE (multi-label, nn.BCEWithLogitsLoss). logits / targets fp32 [B,C] ([B] targets for the
 * broadcast mode); *loss_out = the mean; dlogits (nullable) = d(loss * grad_scale)/d(logits). */
int stonk_elementwise_loss_fwd_bwd(const float* logits, const float* targets, int B, int C, int mode, float* loss_out,
                                   float* dlogits, float grad_scale, void* stream);

/* du = dg * gelu'(u), bf16 elementwise (backward of hf:modeling_bert.py:478, the head transform's activation). */
int stonk_gelu_bwd_bf16(const void* dg, const void* u, void* du, int64_t n, void* stream);

/* gelu_new, BigBird's hidden_act (csrc/bigbird_rowwise.hip), bf16 elementwise, fp32 arithmetic, 16-byte vectors:
 *   g  = 0.5 u (1 + tanh(c (u + 0.044715 u^3))),  c = sqrt(2 / pi)
 *   du = dg [0.5 (1 + t) + 0.5 u (1 - t^2) c (1 + 3 * 0.044715 u^2)]
 * Replaces hf:activations.py NewGELUActivation as BigBirdIntermediate applies it (hf:models/big_bird/modeling_big_bird.py
 * BigBirdIntermediate.forward) and its backward: the GEMM epilogues carry the erf form only, so the BigBird encoder's FFN-up
 * GEMM runs with STONK_EPI_BIAS, writes the bf16 pre-activation u, and these follow (backward: the plain dgrad GEMM, then
 * _bwd, which may run in place, du == dg). Finite for EVERY finite bf16 u, +-bf16-max included: the derivative's second term
 * is dropped once |2 c (u + 0.044715 u^3)| >= 87, where 1 - t^2 < 4e-38 and u (1 + 3 k u^2) may overflow.
 * Refused: a null pointer, n < 0, n % 8 (STONK_EINVAL); a pointer not 16-byte aligned (STONK_EALIGN). n == 0 returns STONK_OK. */
int stonk_gelu_new_fwd_bf16(const void* u, void* g, int64_t n, void* stream);
int stonk_gelu_new_bwd_bf16(const void* dg, const void* u, void* du, int64_t n, void* stream);

/* Optimizer step pieces (hf:trainer.py:1780-1796 as driven by ref:src/stonkgs/models/stonkgs_pretraining.py:171-223):
 * *out_accum += sum(x^2), summed in a fixed order (bitwise repeatable: data-parallel replicas rely on it) through a caller
 * workspace of stonk_sumsq_workspace_floats() floats - zero it once after allocating it; the kernel leaves it ready for
 * the next launch; concurrent launches (different streams) need different workspaces;
 * fused clip_grad_norm_(max_grad_norm) + AdamW + bf16 weight refresh + grad zeroing. */
int64_t stonk_sumsq_workspace_floats(void);
int stonk_sumsq_f32(const float* x, int64_t n, float* out_accum, float* workspace, int64_t ws_floats, void* stream);
/* stonk_sumsq_f32 that also adds n_extra ready-made sums (device floats; nullable with n_extra == 0): the block that
 * finishes last adds them to its total in index order, behind the partial sums of x - one fixed order, no launch of its
 * own: 64 consecutive runs of ceil(n_extra / 64) extras are each summed element by element and the run sums are added to
 * the total one after the other, all in fp64, rounded to fp32 once at the end. Without extras: stonk_sumsq_f32, bit for
 * bit. */
int stonk_sumsq_f32_plus(const float* x, int64_t n, float* out_accum, float* workspace, int64_t ws_floats,
                         const float* extra, int64_t n_extra, void* stream);
/* stonk_adamw_step works on any piece of the flat buffers (pointers into p / g / p_bf16 at the piece, m / v wherever the
 * caller keeps that piece's state: an optimizer sharded over data-parallel ranks updates its 1/world of every gradient
 * bucket). decay_spans (nullable, device): n_spans sorted [lo, hi) element ranges of the WHOLE flat buffer that receive
 * the decoupled weight decay (HF Trainer decays weights, not biases / LayerNorm); span_base = the piece's offset in the
 * flat buffer (% 4 == 0). Without a table, weight_decay applies to every element. */
int stonk_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float bias_corr1, float bias_corr2, const float* gnorm_sq_dev,
                     float max_grad_norm, float grad_scale, const int64_t* decay_spans, int n_spans, int64_t span_base,
                     void* stream);
/* The step over the WHOLE flat buffers (n elements, n % 4 == 0) that also writes the bf16 W^T copies, so that no
 * stonk_transpose_bf16_batched pass follows it. Bit-identical to stonk_adamw_step (span_base 0) followed by that pass.
 * tile_desc_dev: device array of n_desc 56-byte entries {int64 off; void* wt; int64 ld_out, rows, prows; int32 cols,
 * first_tile, col_tiles, pad} sorted by first_tile - a 2-D weight of prows x cols elements at `off` in the flat buffers
 * (rows <= prows: the logical rows; pad rows are updated but reach the W^T copy as zeros), wt = its [cols, ld_out] copy;
 * an entry covers ceil(prows/64) * col_tiles tiles of 64x64 (col_tiles = ceil(cols/64)), total_tiles = the sum.
 * flat_spans_dev: device array of n_flat int64 triples {lo, hi, first_chunk} sorted by first_chunk - every other piece of
 * [0, n), updated 1024 elements per workgroup (an entry covers ceil((hi - lo)/1024) chunks, total_chunks = the sum).
 * The caller guarantees what a launcher cannot read from device tables: the two tables cover [0, n) exactly once; off, lo,
 * hi % 4 == 0; cols % 8 == 0; wt 16-byte aligned, ld_out % 8 == 0, ld_out >= roundup64(rows).
 * keep_grad_spans (nullable, device): n_keep sorted [lo, hi) ranges whose gradient is left as it is instead of zeroed
 * (the next step's stonk_gemm_tn_bf16_store overwrites them). decay_spans as for stonk_adamw_step. Tables 8-byte aligned. */
int stonk_adamw_step_tiled(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                           const float* gnorm_sq_dev, float max_grad_norm, float grad_scale, const int64_t* decay_spans,
                           int n_spans, const int64_t* keep_grad_spans, int n_keep, const void* tile_desc_dev, int n_desc,
                           int total_tiles, const int64_t* flat_spans_dev, int n_flat, int total_chunks, void* stream);
int stonk_scale_f32(float* x, int64_t n, float s, void* stream);

/* ---- node2vec (csrc/node2vec.hip): the stage that makes the model's knowledge-graph inputs - the random walks and the
 * entity table - from an edge list. Replaces ref:src/stonkgs/models/node2vec.py:270-370 (run_node2vec: nodevectors' CPU
 * walks, gensim's word2vec threads); stonkgs_amd/node2vec.py is the host side. The header comment of the source file
 * states the random-number formula and both algorithms exactly; tests/test_node2vec_cpu.py restates them in numpy.
 *
 * stonk_random_walks: rows [walk_lo, walk_hi) of walks (int32 [W, L], row stride ld) are written, nothing else.
 * CSR graph: rowptr int64 [N+1], col int32 [nnz], every adjacency list sorted ascending. starts (nullable): int32 [W],
 * walk w starts at starts[w]; NULL: at w % N; a start outside [0, N) gives a row of -1. thr_*: 24-bit acceptance
 * thresholds (<= 2^24) of the three classes of a candidate next node - the previous node, a common neighbour of the
 * previous node, anything else; all equal: a first-order (uniform) walk. Every draw is a pure function of (seed, w, step,
 * attempt, which): the rows do not depend on how [0, W) is cut into calls. Rejection sampling, at most 32 attempts a step.
 * Refused before any launch: rowptr / col / walks null (STONK_EINVAL); L < 1, walk_lo < 0, walk_hi < walk_lo, ld < L, N < 1,
 * a threshold above 2^24 (STONK_ESHAPE); rowptr not 8-byte, col / starts / walks not 4-byte aligned (STONK_EALIGN).
 * walk_lo == walk_hi returns STONK_OK without a launch. */
int stonk_random_walks(const int64_t* rowptr, const int32_t* col, int64_t N, const int32_t* starts, int64_t walk_lo,
                       int64_t walk_hi, int L, uint32_t thr_return, uint32_t thr_common, uint32_t thr_other, uint32_t seed,
                       int32_t* walks, int64_t ld, void* stream);
/* stonk_sgns_step: skip-gram with negative sampling over the groups (walk w, position t), w in [walk_lo, walk_hi), t in
 * [pos_lo, pos_hi), of `walks` (as above). W_in / W_out: fp32 [N, D], contiguous, D % 64 == 0, D <= 1024. Per group: a
 * reduced window b in [1, window], contexts walk[w][t-b .. t+b] without t, `negatives` noise nodes from the alias table
 * (alias_thr uint32 [N], alias_idx int32 [N]: a hashed draw picks a slot, slot s is kept iff a second draw < alias_thr[s],
 * else alias_idx[s]) shared by the group's contexts, a noise node equal to the centre skipped. Mini-batch semantics inside a
 * group (every gradient scale from the rows as read first), every update a device-scope float atomic add; rows read inside a
 * launch may be stale with respect to other groups of the same launch - the caller cuts an epoch into many launches and
 * passes each its own lr. loss_sum_cnt (nullable): [0] += sum of -log sigmoid terms, [1] += their number.
 * Refused before any launch: walks / W_in / W_out null, an alias array null with negatives > 0 (STONK_EINVAL); D % 64,
 * D > 1024, window < 1, negatives < 0, L < 1, ld < L, N < 1, an inverted range, positions outside [0, L], 2 * window context
 * rows of D floats beyond 64 KiB of LDS (STONK_ESHAPE); W_in / W_out not 16-byte, the others not 4-byte aligned
 * (STONK_EALIGN). An empty range returns STONK_OK without a launch. */
int stonk_sgns_step(const int32_t* walks, int64_t ld, int L, int64_t walk_lo, int64_t walk_hi, int pos_lo, int pos_hi,
                    float* W_in, float* W_out, int64_t N, int D, int window, int negatives, const uint32_t* alias_thr,
                    const int32_t* alias_idx, float lr, uint32_t seed, float* loss_sum_cnt, void* stream);

/* ---- Link-prediction score of a node2vec table (csrc/link_prediction.hip): how good a table is, and the figure the
 * hyper-parameter search maximises. Replaces the device-worthy parts of ref:src/stonkgs/models/node2vec.py:34-71
 * (run_link_prediction): stellargraph's negative sampling behind EdgeSplitter(kg).train_test_split() (:50), the [n, D]
 * Hadamard feature matrix (:56-58) and every pass scikit-learn's LogisticRegression.fit / predict makes over it (:66-68).
 * stonkgs_amd/link_prediction.py is the host side; tests/test_link_prediction_cpu.py restates both kernels in numpy.
 *
 * stonk_sample_non_edges: rows [sample_lo, sample_hi) of out (int32 [S, 2]) are written, nothing else. CSR graph as for
 * stonk_random_walks, symmetric (both directions of every edge present), N nodes. Sample i draws up to 64 ordered pairs
 * (u, v), uniform over [0, N)^2, and takes the first with u != v and v not adjacent to u; if all 64 are rejected the row is
 * (-1, -1) and *failures (int32, device; the caller zeroes it) grows by one. Row i is a pure function of (seed, i): it does
 * not depend on how [0, S) is cut into calls. DUPLICATES ARE ALLOWED: two samples may name the same pair (the reference's
 * sampler removes duplicates; at the densities this is used at a repeat is rare, and the classifier does not care).
 * Refused before any launch: rowptr / col / out / failures null (STONK_EINVAL); N < 1, sample_lo < 0, sample_hi < sample_lo,
 * sample_hi >= 2^30 (STONK_ESHAPE); rowptr not 8-byte, the others not 4-byte aligned (STONK_EALIGN). An empty range returns
 * STONK_OK without a launch. */
int stonk_sample_non_edges(const int64_t* rowptr, const int32_t* col, int64_t N, int64_t sample_lo, int64_t sample_hi,
                           uint32_t seed, int32_t* out, int32_t* failures, void* stream);
/* stonk_linkpred_lossgrad: one evaluation of the logistic model on Hadamard features, nothing of size [n, D] materialised.
 * emb fp32 [N, D], row stride ld >= D, D % 64 == 0, 64 <= D <= 1024; pairs int32 [n, 2]; y fp32 [n] (0 or 1); w fp32 [D].
 * Example e: x = emb[pairs[e][0]] * emb[pairs[e][1]] (elementwise), z = <x, w> + b, loss = softplus(z) - y z,
 * g = sigmoid(z) - y. Outputs, each skipped when null (at least one is needed): scores fp32 [n] = z; partials fp32
 * [G, D + 2], G = stonk_linkpred_partial_rows(), row r = workgroup r's [sum g x (D floats), sum g, sum loss] - the caller
 * sums the G rows (in fp64). Every row of partials is written by every launch. With partials null y may be null too: the
 * forward pass of decision_function / predict. An example with a node id outside [0, N) contributes nothing and gets the
 * score NaN. No float atomics; which wavefront adds which example in which order depends on (n, G) alone, and a
 * workgroup's wavefronts are added in a fixed order: two calls on equal inputs give bit-equal outputs (a line search
 * compares values of neighbouring points). A sub-range of examples is a call with offset pairs / y / scores pointers.
 * Refused before any launch: emb / pairs / w null, scores and partials both null, partials without y (STONK_EINVAL);
 * D % 64, D < 64, D > 1024, ld < D, ld >= 2^31, N < 1, N >= 2^31, n < 0 (STONK_ESHAPE); pairs not 8-byte, the others not
 * 4-byte aligned (STONK_EALIGN). n == 0 returns STONK_OK without a launch (partials is then left as it is). */
int64_t stonk_linkpred_partial_rows(void);
int stonk_linkpred_lossgrad(const float* emb, int64_t ld, int64_t N, int D, const int32_t* pairs, const float* y, int64_t n,
                            const float* w, float b, float* scores, float* partials, void* stream);

/* ---- KG baseline (csrc/kg_baseline.hip): the knowledge-graph-only classifier every STonKGs fine-tuning result is
 * compared against, ref:src/stonkgs/models/kg_baseline_model.py. Replaces the [n, L, D] float64 host array of its datasets
 * (:186, :249) by one gather-and-max pass, and its lightning training loop (batch 8, 100 epochs: 10^6 optimizer steps per
 * fold) by a kernel that walks many steps with the model on chip, all folds side by side. stonkgs_amd/kg_baseline_model.py
 * is the host side; tests/test_kg_baseline_cpu.py restates the dropout rule and the step.
 *
 * stonk_walk_maxpool: pooled[e, d] = max_t table[ids[e, t], d]. ids int32 [n, L], row stride ld_ids >= L, L >= 1; table fp32
 * [N, D], row stride ld_table; pooled fp32 [n, D], row stride ld_pooled; D % 64 == 0, 64 <= D <= 1024. Id -1 is the
 * reference's null vector (:155): a row of zeros that takes part in the maximum. Any other id outside [0, N) makes that
 * example's row NaN and adds one (per example) to *errors (int32, device; the caller zeroes it). The maximum is exact: for a
 * finite table the result is bit-identical to torch.max(x, dim=1).values. A NaN in the table is NOT propagated as torch
 * does (the hardware maximum drops a NaN operand). A sub-range of examples is a call with offset ids / pooled pointers.
 * Refused before any launch: a null pointer (STONK_EINVAL); D, L, the strides, N < 1 or >= 2^31, n < 0 or >= 2^31
 * (STONK_ESHAPE); table / pooled not 16-byte aligned, ld_table % 4, ld_pooled % 4, ids / errors not 4-byte aligned
 * (STONK_EALIGN). n == 0 returns STONK_OK without a launch. */
int stonk_walk_maxpool(const int32_t* ids, int64_t ld_ids, int64_t n, int L, const float* table, int64_t ld_table, int64_t N,
                       int D, float* pooled, int64_t ld_pooled, int32_t* errors, void* stream);
/* stonk_kgb_train_steps: R independent runs (cross-validation folds), one workgroup each, every run walking its own span of
 * consecutive optimizer steps of  dropout(p) -> linear [C, D] -> softmax -> CrossEntropyLoss(weight, "mean") ON THE
 * PROBABILITIES (the reference's quirk, :93-110: a second log-softmax is taken over the softmax output; the gradient goes
 * back through both) -> torch.optim.AdamW (decoupled weight decay, bias corrections by the global step number, no clipping,
 * no schedule).
 * PER-RUN LAYOUT, run r = 0 .. R - 1, all on the device: order int32, row r at order + r * ld_order, `batch` example indices
 * per step, -1 pads a ragged batch; n_steps int32 [R]; first_step int32 [R], the global index of the span's first step (the
 * step that uses Adam's t = 1 has index 0); class_weights fp32 [R, C]; W, mW, vW fp32 [R, C, D]; b, mb, vb fp32 [R, C]; loss
 * fp32, row r at loss + r * ld_loss, one value per step of the span; errors int32 [R]. Shared: pooled fp32 [n, D] with row
 * stride ld_pooled, labels int32 [n], the scalars (AdamW's are fp64, as torch keeps them: 1 - beta taken from an fp32 beta
 * would be off by 1e-5 of itself). Run r executes min(n_steps[r], n_steps_max) steps; n_steps_max (host) is
 * what the launcher checks against the cap stonk_kgb_max_steps() and against ld_order / ld_loss.
 * W, b and the moments are read at the start of the launch, stay in registers / LDS between the steps and are written back
 * at its end. The dropout keep decision is a pure function of (seed, run, global step, row in batch, feature) and the bias
 * corrections of the global step, so cutting a span into several launches changes no bit. Every reduction has a fixed
 * order, there are no float atomics: equal inputs give equal bits. The only synchronisation is the workgroup barrier.
 * An order entry outside [-1, n) or a label outside [0, C): the row contributes nothing (as if padded) and errors[r] is set
 * to 1 (the caller zeroes it). A step without a single valid row reports the loss 0 / 0 and updates nothing.
 * Refused before any launch, there is no fallback: a null pointer, p outside [0, 1), a beta outside [0, 1), lr < 0
 * (STONK_EINVAL); C outside [2, 16], batch outside [1, 64], D % 64, D outside [64, 1024], n_steps_max above the cap,
 * ld_order < n_steps_max * batch, ld_loss < n_steps_max, ld_pooled < D, n < 1 (STONK_ESHAPE); a pointer not 4-byte aligned
 * (STONK_EALIGN). R == 0 or n_steps_max == 0 returns STONK_OK without a launch. */
int64_t stonk_kgb_max_steps(void);
int stonk_kgb_train_steps(const float* pooled, int64_t ld_pooled, int64_t n, int D, const int32_t* labels, int C, int R,
                          const int32_t* order, int64_t ld_order, int batch, const int32_t* n_steps, const int32_t* first_step,
                          int n_steps_max, const float* class_weights, float* W, float* b, float* mW, float* vW, float* mb,
                          float* vb, float* loss, int64_t ld_loss, int32_t* errors, double lr, double beta1, double beta2,
                          double eps, double weight_decay, float p, uint32_t seed, void* stream);
/* stonk_kgb_predict: eval mode (no dropout). Example j = idx[j] (int32 [k], indices into pooled): probs fp32 [k, C] =
 * softmax(pooled[idx[j]] W^T + b), pred int32 [k] = the arg-max of the probabilities, the LOWEST index on a tie (what
 * torch.argmax returns for a first maximum). An index outside [0, n): the row of probs is NaN, pred -1, *errors grows by one.
 * Refusals as for stonk_kgb_train_steps; k == 0 returns STONK_OK without a launch. */
int stonk_kgb_predict(const float* pooled, int64_t ld_pooled, int64_t n, int D, const int32_t* idx, int64_t k, const float* W,
                      const float* b, int C, float* probs, int32_t* pred, int32_t* errors, void* stream);

/* ---- TransE (csrc/transe.hip): trains and ranks the table that ref:src/stonkgs/constants.py:70 names
 * transe_embeddings_best_model.tsv and ref:src/stonkgs/models/kg_baseline_model.py:208-267 reads (the reference does not
 * produce it; its authors used PyKEEN outside the package). stonkgs_amd/transe.py is the host side; the source file's
 * header states the algorithm and the random-number formula, tests/test_transe_cpu.py restates both in numpy.
 * Shared: ent fp32 [N_e, D], rel fp32 [N_r, D], contiguous, 16-byte aligned; D % 64 == 0, 64 <= D <= 1024; norm 1 or 2.
 *
 * stonk_transe_step: one slice of a margin-ranking pass with plain SGD, one wavefront per group g in [g_lo, g_hi). The
 * group's triple is triples[order ? order[g] : g] (triples int32 [n, 3] of (head, relation, tail); order nullable int32
 * [n]); `negatives` corrupted triples per group - each replaces the head or the tail by a uniform entity, a replacement
 * equal to what it replaces is skipped - drawn as pure functions of (seed, g, epoch, j). Loss: sum over the terms of
 * max(0, margin + ||h + r - t|| - ||h' + r - t'||), the norm itself for norm 2. Mini-batch semantics inside a group, one
 * device-scope float atomic add of -lr * grad per destination row; rows read inside a launch may be stale with respect to
 * other groups of the same launch - the caller cuts an epoch into many launches. A triple with an id outside its table (or
 * an order entry outside [0, n)) is skipped. loss_sum_cnt (nullable float [2]): [0] += the loss, [1] += the number of
 * non-skipped terms.
 * Refused before any launch: ent / rel / triples null, norm not 1 or 2 (STONK_EINVAL); D off the rule, negatives < 1,
 * negatives * (D + 1) floats beyond 64 KiB of LDS, N_e or N_r < 1, N_e / N_r / n >= 2^31, g_lo < 0, g_hi < g_lo, g_hi > n
 * (STONK_ESHAPE); ent / rel not 16-byte, the others not 4-byte aligned (STONK_EALIGN). g_lo == g_hi returns STONK_OK
 * without a launch. */
int stonk_transe_step(float* ent, float* rel, int64_t N_e, int64_t N_r, int D, const int32_t* triples, int64_t n,
                      const int32_t* order, int64_t g_lo, int64_t g_hi, int negatives, int norm, float margin, float lr,
                      uint32_t seed, uint32_t epoch, float* loss_sum_cnt, void* stream);
/* stonk_rows_l2_normalize: rows [row_lo, row_hi) of table (fp32, row stride ld >= D floats) become row / ||row||_2; a row
 * with norm < 1e-12 is left as it is; nothing outside the range is written.
 * Refused: table null (STONK_EINVAL); D off the rule, ld < D, ld >= 2^31, row_lo < 0, row_hi < row_lo, row_hi >= 2^31
 * (STONK_ESHAPE); table not 16-byte aligned (STONK_EALIGN). An empty range returns STONK_OK without a launch. */
int stonk_rows_l2_normalize(float* table, int64_t ld, int64_t row_lo, int64_t row_hi, int D, void* stream);
/* stonk_transe_rank: queries int32 [Q, 3]; side 0 ranks the tail (v = h + r, true entity t), side 1 the head (v = t - r,
 * true entity h). dist(c) = ||v - ent[c]||_1 (norm 1) or the SQUARED L2 distance (norm 2). less / equal (int32 [Q]): the
 * number of candidates with dist < / == the true entity's; every distance, the true one's included, goes through one
 * instruction sequence, so equal >= 1 when the true entity is a candidate. Candidates: all of [0, N_e) when cand_ptr is
 * null, else cand[cand_ptr[q] .. cand_ptr[q+1]) (cand_ptr int64 [Q+1], cand int32 [n_cand]; a range is clipped to
 * [0, n_cand], an id outside [0, N_e) is ignored). A query with an id out of range gets less = equal = -1. No [Q, N_e]
 * matrix exists: a workgroup keeps 16 query vectors in LDS and reads each entity row once per 16 queries.
 * Refused: ent / rel / queries / less / equal null, cand null with cand_ptr given and n_cand > 0, norm not 1 or 2, side not
 * 0 or 1 (STONK_EINVAL); D off the rule, N_e or N_r < 1 or >= 2^31, Q < 0 or >= 2^31, n_cand < 0 (STONK_ESHAPE); ent / rel
 * not 16-byte, cand_ptr not 8-byte, the others not 4-byte aligned (STONK_EALIGN). Q == 0 returns STONK_OK without a launch. */
int stonk_transe_rank(const float* ent, const float* rel, int64_t N_e, int64_t N_r, int D, int norm, const int32_t* queries,
                      int64_t Q, int side, const int64_t* cand_ptr, const int32_t* cand, int64_t n_cand, int32_t* less,
                      int32_t* equal, void* stream);

/* ---- Data-parallel gradient exchange (csrc/comm.hip): RCCL collectives on a stream the LIBRARY owns, handed over by
 * events. Replaces torch DistributedDataParallel's bucketed all-reduce, which the reference gets from HF Trainer when it
 * is launched distributed (ref:src/stonkgs/models/stonkgs_pretraining.py:215-223), and - reduce-scatter / all-gather -
 * DeepSpeed ZeRO-2's exchange when `deepspeed=True` (:174-175).
 *
 *   stonk_comm_unique_id   rank 0 fills 128 bytes (an ncclUniqueId); the CALLER carries them to the other ranks (a file,
 *                          a socket, torch's store - the library opens no connection of its own for that);
 *   stonk_comm_init        one communicator per process (one process per GPU): RCCL over xGMI inside a node; creates the
 *                          communicator's stream and two events. `*comm_out` is an opaque handle;
 *   stonk_comm_*_async     `buf` / `send` / `recv` are device pointers, `n` counts ELEMENTS, dtype 0 = fp32, 1 = bf16, the
 *                          reduction is a sum (the mean is the optimizer's grad_scale). The collective is ordered behind
 *                          everything `after_stream` has enqueued at the call (event hand-off: the producer stream does
 *                          not wait, the host does not block) and runs on the communicator's stream. allreduce: in place.
 *                          reduce_scatter: send holds world * recv_n elements, recv (which may be the rank's own slice of
 *                          send) receives the sum of slice `rank`; allgather: recv holds world * send_n elements (send
 *                          may be the rank's own slice of recv);
 *   stonk_comm_wait        `stream` waits (on the device) for every collective issued so far; no host synchronisation;
 *   stonk_comm_stream      the communicator's hipStream_t (for a profiler range, or to order caller work behind it);
 *   stonk_comm_destroy     drains the stream, destroys communicator, stream and events.
 * Return codes as everywhere (0, STONK_E*, a hipError_t); an RCCL failure r is reported as 10000 + r. RCCL itself is
 * resolved at run time: without it these entry points return STONK_EINVAL and the rest of the library is unaffected. */
int stonk_comm_unique_id(void* id_out_128_bytes);
int stonk_comm_init(void** comm_out, int world, int rank, const void* unique_id_128_bytes, int device);
int stonk_comm_allreduce_async(void* comm, void* buf, int64_t n, int dtype, void* after_stream);
int stonk_comm_reduce_scatter_async(void* comm, const void* send, void* recv, int64_t recv_n, int dtype, void* after_stream);
int stonk_comm_allgather_async(void* comm, const void* send, void* recv, int64_t send_n, int dtype, void* after_stream);
int stonk_comm_wait(void* comm, void* stream);
void* stonk_comm_stream(void* comm);
int stonk_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* STONK_HIP_H */

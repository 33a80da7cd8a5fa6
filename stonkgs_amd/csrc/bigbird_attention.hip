// Block-sparse (BigBird) attention, head_dim 64, block size 64, bf16 MFMA, fp32 softmax: forward and backward driven by
// per-(head, block) LISTS instead of the dense kernels' walk over every key tile (attention.hip, whose tile helpers these
// kernels share through attn_tiles.h).
//
// Replaces hf:models/big_bird/modeling_big_bird.py BigBirdBlockSparseAttention.bigbird_block_sparse_attention :295-744 for
// the query rows whose own mask is 1: the queries of block i take ONE softmax over the concatenation of the key blocks
// that HuggingFace gathers for them (global first / last block, the sliding window, the random blocks). A block gathered
// m times counts m times - duplicates are not removed, they add - which a list entry (j, m) expresses as
//     l += m sum exp(s - max)      O += m P V      dS = m P (dP - delta)      dV += m P^T dO,
// so the softmax is over at most nb entries however often a block repeats (the eval-mode plan repeats block 0 four times).
// No dropout (HuggingFace's block-sparse path applies none to the probabilities).
//
// Three backward kernels, no atomics, bitwise repeatable: bb_prep (delta = rowsum(dO o O) and -lse in log2 units),
// bb_bwd_dq (the forward's lists) and bb_bwd_dkv (the INVERSE lists: for key block j the query blocks that list it).
//
// A workgroup is one 64-row block of one head: four waves as (32-row half) x (32-key half of every 64-key tile). The two
// key halves keep their own running maximum, sum and accumulator and are merged through LDS at the end (forward); the
// backward kernels add their two partial sums the same way. Blocks 0 and nb-1 read nb tiles where the others read 5 to 8
// (and are read by every query block in dK/dV): bb_block() puts those workgroups first in the launch order.
//
// Masked keys enter as in the dense kernels: NEG_MASK through the MFMA accumulator, probability exactly 0. A block whose
// listed keys are ALL masked attends uniformly over them, weighted by multiplicity (every score is exactly NEG_MASK, every
// exp2 exactly 1); its lse, about NEG_MASK * scale, cannot carry log(64 L), so the backward recognises such a block by
// that lse (bb_degenerate) and rebuilds P = 1 / (64 L) from a zero score scale, L = the list's total multiplicity.
//
// The lists live in device memory, where the launcher cannot check them: a count outside [0, nb] (the list then counts as
// empty), an entry outside [0, nb) or a multiplicity <= 0 (the entry is skipped) sets bit 0 of *err_flag and reads nothing
// through the bad value. A block with no valid entry writes zeros.
//
// STONK_BSA_ZERO_MASKED_QUERIES (the _ex entries, with a mask): HuggingFace ends with context_layer * from_mask (:617), so
// the context row of a query whose OWN mask word is 0 is exactly zero and no gradient passes through it. The kernels' ZQ
// instances apply the row's mask word where the row leaves or enters them: the forward at its final store (the lse is
// written as without the flag), bb_prep to delta, bb_bwd_dq to its dO fragment and delta, bb_bwd_dkv to the
// rows of every dO tile as it is staged (delta arrives zeroed from bb_prep) - a masked row then has dP = 0 and delta = 0,
// hence dS = P (0 - 0) = 0 and P^T dO = 0 exactly: nothing reaches dK / dV, and no pass over [B*S, H] is added. The
// instances without ZQ are the kernels as they were. The ZQ instances are compiled in a translation unit of their own,
// bigbird_attention_zq.hip, which includes this file with STONK_BB_ZQ_UNIT defined (as gemm_tn_a4_store.hip includes
// gemm_tn_a4.hip): this object keeps the kernels it had, and the two objects meet in stonk_bb::launch_zq_*.
#include "common.h"
#include "attn_tiles.h"
#include "stonk_flags.h"

namespace {

constexpr int MAXNB = 64;                                 // blocks per sequence (S <= 4096)
constexpr int BB_LDS = 2 * STAGEB + 2 * MAXNB * 4 + 16;   // two stages, the compacted list (block, multiplicity), its length

struct BbArgs {
  const bf16* q;
  const bf16* k;
  const bf16* v;
  long ld;            // row stride (elements) of q/k/v
  const long* mask;   // [B,S] or null
  const int* kb;      // forward lists: key blocks of (head, query block) [NH, nb, nb], ...
  const int* km;      //   ... their multiplicities [NH, nb, nb]
  const int* kc;      //   ... and the lists' lengths [NH, nb]
  const int* qb;      // inverse lists (dK/dV): query blocks of (head, key block), multiplicities, lengths
  const int* qm;
  const int* qc;
  bf16* out;          // fwd: context [T, ldo]; bwd: the forward's context (read)
  long ldo;
  float* lse;         // [B, NH, S] natural-log LSE of the scaled+masked scores over the listed keys (multiplicity included)
  const bf16* dout;   // [T, lddo]
  long lddo;
  float* ws;          // [2, B, NH, S]: delta = rowsum(dO * O), then -lse in log2 units (bb_prep_kernel writes both)
  bf16* dq;
  bf16* dk;
  bf16* dv;
  long ldd;           // row stride of dq/dk/dv
  int B, NH, S, nb;
  float scale;
  int* err;
  int zq;             // bb_prep: delta = 0 for a row whose mask word is 0 (the other kernels take ZQ as a template argument)
};

// Workgroup -> (block, head, sequence). The 2 B NH workgroups of blocks 0 and nb-1 - nb tiles each, against 5 to 8 - take
// the first places of the launch order, so that they start first and the short ones fill in behind them. Of the rest every
// XCD (workgroups go round-robin over the 8 XCDs) takes one contiguous run of the (sequence, head, block) order: a head's
// blocks, which share its K and V (or Q and dO), share an L2.
struct BbBlock { int i, h, b; };
__device__ __forceinline__ BbBlock bb_block(int nb, int NH) {
  const int lin = blockIdx.x;
  const int pairs = gridDim.x / nb;   // B * NH
  int pair, i;
  if (lin < 2 * pairs) {
    pair = lin >> 1;
    i = (lin & 1) ? nb - 1 : 0;
  } else {
    const int rr = lin - 2 * pairs, n = pairs * (nb - 2);
    const int q = n >> 3, rm = n & 7, x = rr & 7;
    const int l = ((x < rm) ? x * (q + 1) : rm * (q + 1) + (x - rm) * q) + (rr >> 3);   // (a bijection of [0, n))
    pair = l / (nb - 2);
    i = 1 + l % (nb - 2);
  }
  BbBlock o;
  o.i = i;
  o.h = pair % NH;
  o.b = pair / NH;
  return o;
}

__device__ __forceinline__ bool bb_entry_ok(int j, int m, int nb) { return j >= 0 && j < nb && m > 0; }

// The list of (head h, block i), read by the first wave (nb <= 64: one entry per lane), its valid entries compacted in
// order into LDS: lj[] the blocks, lm[] the multiplicities, *ln their number (returned). Contains one barrier.
__device__ __forceinline__ int bb_list(const int* blocks, const int* mult, const int* count, int h, int i, int nb, int* lj,
                                       int* lm, int* ln, int* err, int tid) {
  if (tid < 64) {
    const long row = (long)h * nb + i;
    int cnt = count[row];
    bool bad = cnt < 0 || cnt > nb;
    if (bad) cnt = 0;
    const bool have = tid < cnt;   // (tid < cnt <= nb: inside the row of nb entries)
    int j = 0, m = 0;
    if (have) {
      j = blocks[row * nb + tid];
      m = mult[row * nb + tid];
    }
    const bool ok = have && bb_entry_ok(j, m, nb);
    bad |= have && !ok;
    const uint64_t okb = __ballot(ok);
    if (ok) {
      const int pos = __popcll(okb & ((1ull << tid) - 1));
      lj[pos] = j;
      lm[pos] = m;
    }
    const uint64_t badb = __ballot(bad);
    if (tid == 0) {
      *ln = __popcll(okb);
      if (badb != 0) atomicOr(err, 1);
    }
  }
  __syncthreads();
  return *ln;
}

// "Every listed key of this row's block is masked": the forward's lse is then NEG_MASK * scale (+ log(64 L), absorbed);
// a row with a live key has |lse| of the size of its scores, 2^70 times smaller for any data bf16 products can reach.
__device__ __forceinline__ bool bb_degenerate(float lse, float scale) { return lse < 0.5f * NEG_MASK * scale; }

// ------------------------------------------------------------------ forward
template <bool HAS_MASK, bool ZQ>
__global__ __launch_bounds__(256, 2) void bb_fwd_kernel(const BbArgs p) {
  __shared__ __attribute__((aligned(16))) char lds[BB_LDS];
  int* lj = (int*)(lds + 2 * STAGEB);
  int* lm = lj + MAXNB;
  int* ln = lm + MAXNB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int qh = wave & 1, kh = wave >> 1;   // this wave: query rows 32 qh .. + 31 of the block, keys 32 kh .. + 31 of every tile
  const BbBlock blk = bb_block(p.nb, p.NH);
  const int b = blk.b, h = blk.h;
  const int S = p.S;
  const long tok0 = (long)b * S;
  const int q0 = blk.i * TK + qh * 32;
  const float sc2 = p.scale * LOG2E;
  const int nlist = bb_list(p.kb, p.km, p.kc, h, blk.i, p.nb, lj, lm, ln, p.err, tid);

  bf16x8 qf[4];
  {
    const bf16* qrow = p.q + (tok0 + q0 + r) * p.ld + h * HD;
#pragma unroll
    for (int st = 0; st < 4; ++st) qf[st] = *(const bf16x8*)(qrow + 16 * st + 8 * hh);
  }
  f32x16 o[2] = {zero16(), zero16()};
  float m = NEG_INIT, l = 0.f;   // m in scaled log2 units

  const bf16* kbase = p.k + tok0 * p.ld + h * HD;
  const bf16* vbase = p.v + tok0 * p.ld + h * HD;
  Stage2 sk, sv;
  long mreg = 1;   // the mask word of key `tid` of the tile in flight (threads 0..63): converted when the tile is stored
  const TileOff vo = tile_voff(p.ld, tid);
  auto load_tile = [&](int j) {
    stage_load(sk, kbase, p.ld, j * TK, S, vo);
    stage_load(sv, vbase, p.ld, j * TK, S, vo);
    if (HAS_MASK && tid < TK) mreg = p.mask[tok0 + j * TK + tid];
  };
  auto store_tile = [&](int buf) {
    char* base = lds + buf * STAGEB;
    stage_store(sk, base, tid);
    stage_store(sv, base + TILEB, tid);
    if (HAS_MASK && tid < TK) ((float*)(base + 2 * TILEB))[tid] = mreg != 0 ? 0.f : NEG_MASK;
  };
  if (nlist > 0) {
    load_tile(lj[0]);
    store_tile(0);
    __syncthreads();
  }
  for (int it = 0; it < nlist; ++it) {   // the listed key blocks, in list order
    const char* Ks = lds + (it & 1) * STAGEB;
    const char* Vs = Ks + TILEB;
    const float* Mb = (const float*)(Ks + 2 * TILEB) + kh * 32;   // the tile's key bias
    const bool more = it + 1 < nlist;
    if (more) load_tile(lj[it + 1]);
    const float mu = (float)lm[it];
    // S^T = K . Q^T (+ key bias through the accumulator) for this wave's 32 keys of the tile, raw units
    f32x16 s = score_bias<HAS_MASK>(Mb, hh);
#pragma unroll
    for (int st = 0; st < 4; ++st) s = mfma32(row_frag(Ks, kh * 32, st, r, hh), qf[st], s);
    float tmax = max16_mfma(s);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax * sc2);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    const float negm = -m_new;
    f32x2 rs2 = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const f32x2 a = pk_fma((f32x2){s[i], s[i + 1]}, (f32x2){sc2, sc2}, (f32x2){negm, negm});
      const f32x2 e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
      s[i] = e[0];
      s[i + 1] = e[1];
      rs2 += e;
    }
    float rs = rs2[0] + rs2[1];
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + mu * rs;
    if (!__all(alpha == 1.f)) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        o[0][i] *= alpha;
        o[1][i] *= alpha;
      }
    }
    if (mu != 1.f) {   // (workgroup-uniform) the block counts mu times: m P goes into P . V
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] *= mu;
    }
    // O^T += V^T . (m P)^T
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pf = acc_frag(s, ks);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) o[dt] = mfma32(tr_frag(Vs, kh * 32 + 16 * ks, dt * 32, lane), pf, o[dt]);
    }
    if (more) store_tile((it + 1) & 1);
    TILE_BARRIER();
  }
  // merge the two key halves: the waves of the second hand (m, l, O) to those of the first through the (now free) stages
  float* xw = (float*)lds + qh * (34 * 64) + lane;   // [qh][34][64 lanes]
  if (kh == 1) {
    xw[0] = m;
    xw[64] = l;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) xw[(2 + dt * 16 + i) * 64] = o[dt][i];
  }
  __syncthreads();
  if (kh == 1) return;
  const float m1 = xw[0], l1 = xw[64];
  const float mf = fmaxf(m, m1);
  const float a0 = __builtin_amdgcn_exp2f(m - mf), a1 = __builtin_amdgcn_exp2f(m1 - mf);
  l = l * a0 + l1 * a1;
  const float inv = l > 0.f ? 1.f / l : 0.f;   // (l == 0: a block without a valid list entry writes zeros)
  unsigned long live_bits = ~0ul;   // ZQ: all ones for a live query, zero for a masked one (the row's own mask word)
  if (ZQ) live_bits = p.mask[tok0 + q0 + r] != 0 ? ~0ul : 0ul;
  bf16* orow = p.out + (tok0 + q0 + r) * p.ldo + h * HD;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = (o[dt][4 * g + j] * a0 + xw[(2 + dt * 16 + 4 * g + j) * 64] * a1) * inv;
      bf16x4 v = {(bf16)e[0], (bf16)e[1], (bf16)e[2], (bf16)e[3]};
      // (the mask word goes onto the packed BITS: a select on the floats changes how the compiler vectorises and contracts the
      // line above, and a live row's last bit with it - the flag must not be visible in a live row)
      if (ZQ) v = __builtin_bit_cast(bf16x4, __builtin_bit_cast(unsigned long, v) & live_bits);
      *(bf16x4*)(orow + dt * 32 + 8 * g + 4 * hh) = v;
    }
  if (hh == 0) p.lse[(long)(b * p.NH + h) * S + q0 + r] = l > 0.f ? (mf + __builtin_amdgcn_logf(l)) * LN2 : 0.f;
}

// ------------------------------------------------------------------ backward: per-row statistics
// delta = rowsum(dO * O) (delta_row: the one summation order of every producer of delta) and -lse in log2 units - for a row whose listed keys
// are all masked -log2(64 L) instead, L = the total multiplicity of its block's list (see the head of the file).
#ifndef STONK_BB_ZQ_UNIT
__global__ __launch_bounds__(128) void bb_prep_kernel(const BbArgs p) {
  const long rows = (long)p.B * p.NH * p.S;
  const long idx = (long)blockIdx.x * 128 + threadIdx.x;
  if (idx >= rows) return;
  const int S = p.S, nb = p.nb;
  const int qrow = (int)(idx % S);
  const long bh = idx / S;
  const int h = (int)(bh % p.NH);
  const long tok = (bh / p.NH) * S + qrow;
  float delta = delta_row(p.dout + tok * p.lddo + h * HD, p.out + tok * p.ldo + h * HD);
  if (p.zq && p.mask[tok] == 0) delta = 0.f;   // (a masked query's dO counts as zero)
  p.ws[idx] = delta;
  const float lse = p.lse[idx];
  float nls = -lse * LOG2E;
  if (bb_degenerate(lse, p.scale)) {
    const long row = (long)h * nb + qrow / TK;
    int cnt = p.kc[row];
    if (cnt < 0 || cnt > nb) cnt = 0;
    int L = 0;
    for (int e = 0; e < cnt; ++e) {
      const int j = p.kb[row * nb + e], m = p.km[row * nb + e];
      if (bb_entry_ok(j, m, nb)) L += m;
    }
    nls = L > 0 ? -__builtin_amdgcn_logf((float)(TK * L)) : 0.f;   // (v_log_f32 is log2)
  }
  p.ws[rows + idx] = nls;
}
#endif

// ------------------------------------------------------------------ backward: dQ (query on the lane)
template <bool HAS_MASK, bool ZQ>
__global__ __launch_bounds__(256, 2) void bb_bwd_dq_kernel(const BbArgs p) {
  __shared__ __attribute__((aligned(16))) char lds[BB_LDS];
  int* lj = (int*)(lds + 2 * STAGEB);
  int* lm = lj + MAXNB;
  int* ln = lm + MAXNB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int qh = wave & 1, kh = wave >> 1;
  const BbBlock blk = bb_block(p.nb, p.NH);
  const int b = blk.b, h = blk.h;
  const int S = p.S;
  const long tok0 = (long)b * S;
  const int q0 = blk.i * TK + qh * 32;
  const int nlist = bb_list(p.kb, p.km, p.kc, h, blk.i, p.nb, lj, lm, ln, p.err, tid);

  bf16x8 qf[4], dof[4];
  {
    const bf16* qrow = p.q + (tok0 + q0 + r) * p.ld + h * HD;
    const bf16* drow = p.dout + (tok0 + q0 + r) * p.lddo + h * HD;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      qf[st] = *(const bf16x8*)(qrow + 16 * st + 8 * hh);
      dof[st] = *(const bf16x8*)(drow + 16 * st + 8 * hh);
    }
  }
  const long stat = (long)(b * p.NH + h) * S + q0 + r;
  const long rows = (long)p.B * p.NH * S;
  float dlt = p.ws[stat];
  const float nlse2 = p.ws[rows + stat];
  if (ZQ) {   // a masked query: dO and delta count as zero, so dS = m P (0 - 0) is +0 for every key (P is finite) and the
              // accumulators stay +0: the row is stored as exact zeros by the lines every row takes
    if (p.mask[tok0 + q0 + r] == 0) {
      dlt = 0.f;
#pragma unroll
      for (int st = 0; st < 4; ++st) dof[st] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const float sc2 = bb_degenerate(p.lse[stat], p.scale) ? 0.f : p.scale * LOG2E;   // (a zero score scale: P = 2^nlse2 for every key)
  f32x16 dq[2] = {zero16(), zero16()};

  const bf16* kbase = p.k + tok0 * p.ld + h * HD;
  const bf16* vbase = p.v + tok0 * p.ld + h * HD;
  Stage2 sk, sv;
  long mreg = 1;
  const TileOff vo = tile_voff(p.ld, tid);
  auto load_tile = [&](int j) {
    stage_load(sk, kbase, p.ld, j * TK, S, vo);
    stage_load(sv, vbase, p.ld, j * TK, S, vo);
    if (HAS_MASK && tid < TK) mreg = p.mask[tok0 + j * TK + tid];
  };
  auto store_tile = [&](int buf) {
    char* base = lds + buf * STAGEB;
    stage_store(sk, base, tid);
    stage_store(sv, base + TILEB, tid);
    if (HAS_MASK && tid < TK) ((float*)(base + 2 * TILEB))[tid] = mreg != 0 ? 0.f : NEG_MASK;
  };
  if (nlist > 0) {
    load_tile(lj[0]);
    store_tile(0);
    __syncthreads();
  }
  for (int it = 0; it < nlist; ++it) {
    const char* Ks = lds + (it & 1) * STAGEB;
    const char* Vs = Ks + TILEB;
    const float* Mb = (const float*)(Ks + 2 * TILEB) + kh * 32;
    const bool more = it + 1 < nlist;
    if (more) load_tile(lj[it + 1]);
    const float mu = (float)lm[it];
    f32x16 s = score_bias<HAS_MASK>(Mb, hh), dp = zero16();
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      s = mfma32(row_frag(Ks, kh * 32, st, r, hh), qf[st], s);      // S^T[k][q] (+ key bias)
      dp = mfma32(row_frag(Vs, kh * 32, st, r, hh), dof[st], dp);   // dP^T[k][q] = sum_d V[k][d] dO[q][d]
    }
    const f32x2 mu2 = {mu, mu};
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const f32x2 a = pk_fma((f32x2){s[i], s[i + 1]}, (f32x2){sc2, sc2}, (f32x2){nlse2, nlse2});
      const f32x2 pr = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
      const f32x2 ds = mu2 * pr * ((f32x2){dp[i], dp[i + 1]} - (f32x2){dlt, dlt});   // dS^T = m P (dP - delta)
      s[i] = ds[0];
      s[i + 1] = ds[1];
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 dsf = acc_frag(s, ks);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) dq[dt] = mfma32(tr_frag(Ks, kh * 32 + 16 * ks, dt * 32, lane), dsf, dq[dt]);
    }
    if (more) store_tile((it + 1) & 1);
    TILE_BARRIER();
  }
  // the two key halves' partial sums, added through the (now free) stages
  float* xw = (float*)lds + qh * (32 * 64) + lane;   // [qh][32][64 lanes]
  if (kh == 1) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) xw[(dt * 16 + i) * 64] = dq[dt][i];
  }
  __syncthreads();
  if (kh == 1) return;
  store_row(p.dq + (tok0 + q0 + r) * p.ldd + h * HD, hh,
            [&](int dt, int i) { return (dq[dt][i] + xw[(dt * 16 + i) * 64]) * p.scale; });
}

// ------------------------------------------------------------------ backward: dK, dV (key on the lane)
// Workgroup = key block j; the tile loop walks the INVERSE list of (head, j): the query blocks that list j, with the
// multiplicity they list it with. Waves: (32-key half) x (32-row half of every query tile).
template <bool HAS_MASK, bool ZQ>
__global__ __launch_bounds__(256, 2) void bb_bwd_dkv_kernel(const BbArgs p) {
  __shared__ __attribute__((aligned(16))) char lds[BB_LDS];
  int* lj = (int*)(lds + 2 * STAGEB);
  int* lm = lj + MAXNB;
  int* ln = lm + MAXNB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int kh = wave & 1, qs = wave >> 1;   // this wave: keys 32 kh .. + 31 of the block, rows 32 qs .. + 31 of every query tile
  const BbBlock blk = bb_block(p.nb, p.NH);
  const int b = blk.b, h = blk.h;
  const int S = p.S;
  const long tok0 = (long)b * S;
  const int k0 = blk.i * TK + kh * 32;
  const int nlist = bb_list(p.qb, p.qm, p.qc, h, blk.i, p.nb, lj, lm, ln, p.err, tid);

  bf16x8 kf[4], vf[4];
  {
    const bf16* krow = p.k + (tok0 + k0 + r) * p.ld + h * HD;
    const bf16* vrow = p.v + (tok0 + k0 + r) * p.ld + h * HD;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      kf[st] = *(const bf16x8*)(krow + 16 * st + 8 * hh);
      vf[st] = *(const bf16x8*)(vrow + 16 * st + 8 * hh);
    }
  }
  float mb = 0.f;
  if (HAS_MASK) mb = p.mask[tok0 + k0 + r] != 0 ? 0.f : NEG_MASK;
  // a wave whose 32 keys are all masked has P = 0 for every query tile but the degenerate ones: it skips the others'
  // arithmetic (its accumulators stay exactly zero) and only helps to stage the tiles
  const bool wave_live = !HAS_MASK || __ballot(mb == 0.f) != 0;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) dk[0][i] = dk[1][i] = dv[0][i] = dv[1][i] = 0.f;

  const bf16* qbase = p.q + tok0 * p.ld + h * HD;
  const bf16* dbase = p.dout + tok0 * p.lddo + h * HD;
  const long statbase = (long)(b * p.NH + h) * S;
  const long rows = (long)p.B * p.NH * S;
  Stage2 sq, sd;
  // row statistics of a tile: threads 0..63 carry -lse (log2 units), 64..127 delta (negated when the tile is stored)
  float sreg = 0.f;
  float lse_nx = 0.f;   // the lse of the first row of the tile in flight: whether its block is a degenerate one
  const float* sptr = tid < TK ? p.ws + rows + statbase + tid : p.ws + statbase + (tid & (TK - 1));
  const TileOff voq = tile_voff(p.ld, tid), vod = tile_voff(p.lddo, tid);
  long qm[2] = {1, 1};   // ZQ: the mask words of the two query rows whose dO chunks this thread stages (tid / 8, + 32)
  auto load_tile = [&](int i) {
    stage_load(sq, qbase, p.ld, i * TK, S, voq);
    stage_load(sd, dbase, p.lddo, i * TK, S, vod);
    if (ZQ) {
      qm[0] = p.mask[tok0 + i * TK + (tid >> 3)];
      qm[1] = p.mask[tok0 + i * TK + 32 + (tid >> 3)];
    }
    if (tid < 2 * TK) sreg = sptr[i * TK];
    lse_nx = p.lse[statbase + i * TK];
  };
  auto store_tile = [&](int buf) {
    char* base = lds + buf * STAGEB;
    stage_store(sq, base, tid);
    if (ZQ) {   // a masked query's dO row is staged as zeros (its delta is zero in the workspace: bb_prep)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        if (qm[c] == 0) sd.c[c] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
    stage_store(sd, base + TILEB, tid);
    if (tid < 2 * TK) ((float*)(base + 2 * TILEB))[tid] = tid < TK ? sreg : -sreg;
  };
  float lse_cur = 0.f;
  if (nlist > 0) {
    load_tile(lj[0]);
    store_tile(0);
    lse_cur = lse_nx;
    __syncthreads();
  }
  for (int it = 0; it < nlist; ++it) {
    const char* Qs = lds + (it & 1) * STAGEB;
    const char* Ds = Qs + TILEB;
    const float* Ls = (const float*)(Qs + 2 * TILEB) + qs * 32;
    const float* Dl = Ls + TK;
    const bool more = it + 1 < nlist;
    const bool degen = bb_degenerate(lse_cur, p.scale);
    if (more) load_tile(lj[it + 1]);
    const float mu = (float)lm[it];
    if (wave_live || degen) {
      const float sc2 = degen ? 0.f : p.scale * LOG2E;
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = mb;
        dp[i] = 0.f;
      }
      // (operands requested a phase ahead of the MFMAs that use them and held there: see attn_bwd_dkv_kernel)
      bf16x8 qa[4], da[4];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        qa[st] = row_frag(Qs, qs * 32, st, r, hh);
        da[st] = row_frag(Ds, qs * 32, st, r, hh);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        s = mfma32(qa[st], kf[st], s);    // S[q][k] (+ key bias)
        dp = mfma32(da[st], vf[st], dp);  // dP[q][k] = sum_d dO[q][d] V[k][d]
      }
      bf16x8 td[2][2], tq[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          td[ks][dt] = tr_frag(Ds, qs * 32 + 16 * ks, dt * 32, lane);
          tq[ks][dt] = tr_frag(Qs, qs * 32 + 16 * ks, dt * 32, lane);
        }
      __builtin_amdgcn_sched_barrier(0);
      const f32x2 mu2 = {mu, mu};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 nls = *(const f32x4*)(Ls + 8 * g + 4 * hh);
        const f32x4 dl = *(const f32x4*)(Dl + 8 * g + 4 * hh);   // -delta
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
          const int i = 4 * g + j;
          const f32x2 a = pk_fma((f32x2){s[i], s[i + 1]}, (f32x2){sc2, sc2}, (f32x2){nls[j], nls[j + 1]});
          const f32x2 pr = mu2 * (f32x2){__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};   // m P
          const f32x2 ds = pr * ((f32x2){dp[i], dp[i + 1]} + (f32x2){dl[j], dl[j + 1]});                  // dS = m P (dP - delta)
          s[i] = pr[0];
          s[i + 1] = pr[1];
          dp[i] = ds[0];
          dp[i + 1] = ds[1];
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pf = acc_frag(s, ks), dsf = acc_frag(dp, ks);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mfma32(td[ks][dt], pf, dv[dt]);   // dV^T += dO^T . (m P)
          dk[dt] = mfma32(tq[ks][dt], dsf, dk[dt]);  // dK^T += Q^T . dS
        }
      }
    }
    if (more) store_tile((it + 1) & 1);
    lse_cur = lse_nx;
    TILE_BARRIER();
  }
  // the two query halves' partial sums, added through the (now free) stages
  float* xw = (float*)lds + kh * (64 * 64) + lane;   // [kh][64][64 lanes]
  if (qs == 1) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        xw[(dt * 16 + i) * 64] = dk[dt][i];
        xw[(32 + dt * 16 + i) * 64] = dv[dt][i];
      }
  }
  __syncthreads();
  if (qs == 1) return;
  bf16* krow = p.dk + (tok0 + k0 + r) * p.ldd + h * HD;
  bf16* vrow = p.dv + (tok0 + k0 + r) * p.ldd + h * HD;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float e[4], f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = (dk[dt][4 * g + j] + xw[(dt * 16 + 4 * g + j) * 64]) * p.scale;
        f[j] = dv[dt][4 * g + j] + xw[(32 + dt * 16 + 4 * g + j) * 64];
      }
      bf16x4 a = {(bf16)e[0], (bf16)e[1], (bf16)e[2], (bf16)e[3]};
      bf16x4 c = {(bf16)f[0], (bf16)f[1], (bf16)f[2], (bf16)f[3]};
      *(bf16x4*)(krow + dt * 32 + 8 * g + 4 * hh) = a;
      *(bf16x4*)(vrow + dt * 32 + 8 * g + 4 * hh) = c;
    }
}

static_assert(2 * 64 * 64 * 4 <= 2 * STAGEB, "the dK/dV partial sums fit the two stages");

#ifdef STONK_BB_ZQ_UNIT
}  // namespace

// The ZQ instances' launches, called from bigbird_attention.hip's _ex entries (which have checked every argument): `args` is
// that unit's BbArgs - the same struct, compiled from the same text.
namespace stonk_bb {
void launch_zq_fwd(const void* args, unsigned grid, void* stream) {
  const BbArgs a = *(const BbArgs*)args;
  hipLaunchKernelGGL((bb_fwd_kernel<true, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
}
void launch_zq_bwd(const void* args, unsigned grid, void* stream) {
  const BbArgs a = *(const BbArgs*)args;
  hipLaunchKernelGGL((bb_bwd_dq_kernel<true, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL((bb_bwd_dkv_kernel<true, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
}
}  // namespace stonk_bb
#else
int bb_check_common(const void* q, const void* k, const void* v, int64_t ld, const int* blocks, const int* mult,
                    const int* count, int* err_flag, int B, int NH, int S, int D, float scale) {
  STONK_CHECK_ARG(q && k && v && blocks && mult && count && err_flag, STONK_EINVAL);
  STONK_CHECK_ARG(D == HD, STONK_ESHAPE);
  // (64-row blocks; BigBird's row kinds need nb >= 5; one list entry per lane of a wave: nb <= 64)
  STONK_CHECK_ARG(B >= 0 && NH > 0 && S % TK == 0 && S >= 5 * TK && S <= MAXNB * TK, STONK_ESHAPE);
  STONK_CHECK_ARG(ld >= 3L * NH * HD, STONK_ESHAPE);   // q/k/v: column slices of one [B*S, 3H] projection
  STONK_CHECK_ARG((long)B * NH * (S / TK) < (1L << 31), STONK_ESHAPE);   // one workgroup per (sequence, head, block)
  STONK_CHECK_ARG(ld % 8 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)v % 16 == 0, STONK_EALIGN);
  STONK_CHECK_ARG(scale > 0.f, STONK_EINVAL);
  return STONK_OK;
}

// the fields that the forward and the backward fill alike
BbArgs bb_args(const void* q, const void* k, const void* v, int64_t ld, const int64_t* attention_mask, const int* key_blocks,
               const int* key_mult, const int* key_count, const void* out, int64_t ldo, const float* lse, int B, int NH, int S,
               float scale, int* err_flag) {
  BbArgs a = {};
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.ld = ld;
  a.mask = (const long*)attention_mask; a.kb = key_blocks; a.km = key_mult; a.kc = key_count;
  a.out = (bf16*)out; a.ldo = ldo; a.lse = (float*)lse;
  a.B = B; a.NH = NH; a.S = S; a.nb = S / TK; a.scale = scale; a.err = err_flag;
  return a;
}

}  // namespace

namespace stonk_bb {   // bigbird_attention_zq.hip
void launch_zq_fwd(const void* args, unsigned grid, void* stream);
void launch_zq_bwd(const void* args, unsigned grid, void* stream);
}  // namespace stonk_bb

extern "C" int stonk_block_sparse_attention_fwd_ex(const void* q, const void* k, const void* v, int64_t ld,
                                                   const int64_t* attention_mask, const int* key_blocks,
                                                   const int* key_mult, const int* key_count, void* out, int64_t ldo,
                                                   float* lse, int B, int NH, int S, int D, float scale, int* err_flag,
                                                   int flags, void* stream) {
  STONK_CHECK_ARG((flags & ~STONK_BSA_ZERO_MASKED_QUERIES) == 0, STONK_EINVAL);
  int rc = bb_check_common(q, k, v, ld, key_blocks, key_mult, key_count, err_flag, B, NH, S, D, scale);
  if (rc) return rc;
  STONK_CHECK_ARG(out && lse, STONK_EINVAL);
  STONK_CHECK_ARG(ldo >= (long)NH * HD, STONK_ESHAPE);
  STONK_CHECK_ARG(ldo % 4 == 0 && (uintptr_t)out % 8 == 0, STONK_EALIGN);
  if (B == 0) return STONK_OK;
  const BbArgs a = bb_args(q, k, v, ld, attention_mask, key_blocks, key_mult, key_count, out, ldo, lse, B, NH, S, scale, err_flag);
  const dim3 grid(B * NH * a.nb), block(256);
  hipStream_t st = (hipStream_t)stream;
  const bool zq = (flags & STONK_BSA_ZERO_MASKED_QUERIES) && attention_mask;   // (without a mask every query is live)
  if (zq) stonk_bb::launch_zq_fwd(&a, grid.x, stream);
  else with_flag(attention_mask != nullptr, [&](auto hm) { hipLaunchKernelGGL((bb_fwd_kernel<hm(), false>), grid, block, 0, st, a); });
  return stonk_launch_status();
}

extern "C" int stonk_block_sparse_attention_fwd(const void* q, const void* k, const void* v, int64_t ld,
                                                const int64_t* attention_mask, const int* key_blocks, const int* key_mult,
                                                const int* key_count, void* out, int64_t ldo, float* lse, int B, int NH,
                                                int S, int D, float scale, int* err_flag, void* stream) {
  return stonk_block_sparse_attention_fwd_ex(q, k, v, ld, attention_mask, key_blocks, key_mult, key_count, out, ldo, lse, B,
                                             NH, S, D, scale, err_flag, 0, stream);
}

extern "C" int stonk_block_sparse_attention_bwd_ex(const void* q, const void* k, const void* v, int64_t ld,
                                                   const int64_t* attention_mask, const int* key_blocks,
                                                   const int* key_mult, const int* key_count, const int* query_blocks,
                                                   const int* query_mult, const int* query_count, const void* out,
                                                   int64_t ldo, const void* dout, int64_t lddo, const float* lse,
                                                   float* delta_ws, void* dq, void* dk, int64_t ldd, void* dv, int B, int NH,
                                                   int S, int D, float scale, int* err_flag, int flags, void* stream) {
  STONK_CHECK_ARG((flags & ~STONK_BSA_ZERO_MASKED_QUERIES) == 0, STONK_EINVAL);
  int rc = bb_check_common(q, k, v, ld, key_blocks, key_mult, key_count, err_flag, B, NH, S, D, scale);
  if (rc) return rc;
  STONK_CHECK_ARG(query_blocks && query_mult && query_count && out && dout && lse && delta_ws && dq && dk && dv, STONK_EINVAL);
  STONK_CHECK_ARG(ldo >= (long)NH * HD && lddo >= (long)NH * HD && ldd >= (long)NH * HD, STONK_ESHAPE);
  STONK_CHECK_ARG(ldo % 8 == 0 && lddo % 8 == 0 && ldd % 4 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)dout % 16 == 0, STONK_EALIGN);
  STONK_CHECK_ARG((uintptr_t)dq % 8 == 0 && (uintptr_t)dk % 8 == 0 && (uintptr_t)dv % 8 == 0, STONK_EALIGN);
  if (B == 0) return STONK_OK;
  BbArgs a = bb_args(q, k, v, ld, attention_mask, key_blocks, key_mult, key_count, out, ldo, lse, B, NH, S, scale, err_flag);
  a.qb = query_blocks; a.qm = query_mult; a.qc = query_count;
  a.dout = (const bf16*)dout; a.lddo = lddo; a.ws = delta_ws;
  a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.ldd = ldd;
  const dim3 grid(B * NH * a.nb), block(256);
  const long rows = (long)B * NH * S;
  hipStream_t st = (hipStream_t)stream;
  const bool zq = (flags & STONK_BSA_ZERO_MASKED_QUERIES) && attention_mask;
  a.zq = zq;
  hipLaunchKernelGGL(bb_prep_kernel, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, st, a);
  if (zq) {
    stonk_bb::launch_zq_bwd(&a, grid.x, stream);
  } else {
    with_flag(attention_mask != nullptr, [&](auto hm) {
      hipLaunchKernelGGL((bb_bwd_dq_kernel<hm(), false>), grid, block, 0, st, a);
      hipLaunchKernelGGL((bb_bwd_dkv_kernel<hm(), false>), grid, block, 0, st, a);
    });
  }
  return stonk_launch_status();
}

extern "C" int stonk_block_sparse_attention_bwd(const void* q, const void* k, const void* v, int64_t ld,
                                                const int64_t* attention_mask, const int* key_blocks, const int* key_mult,
                                                const int* key_count, const int* query_blocks, const int* query_mult,
                                                const int* query_count, const void* out, int64_t ldo, const void* dout,
                                                int64_t lddo, const float* lse, float* delta_ws, void* dq, void* dk,
                                                int64_t ldd, void* dv, int B, int NH, int S, int D, float scale,
                                                int* err_flag, void* stream) {
  return stonk_block_sparse_attention_bwd_ex(q, k, v, ld, attention_mask, key_blocks, key_mult, key_count, query_blocks,
                                             query_mult, query_count, out, ldo, dout, lddo, lse, delta_ws, dq, dk, ldd, dv, B,
                                             NH, S, D, scale, err_flag, 0, stream);
}
#endif  // STONK_BB_ZQ_UNIT

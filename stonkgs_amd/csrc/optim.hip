// HBM-bound elementwise / layout kernels of the optimizer step (K16 in SURVEY.md section 2.3):
// global grad-norm, fused clip + AdamW + bf16 weight refresh + grad zeroing over ONE flat fp32 buffer,
// and the tiled transposes that feed the NT GEMM (wgrad operands, W^T copies for dgrad).
//
// Semantics follow what the reference's driver calls (ref:src/stonkgs/models/stonkgs_pretraining.py:171-223):
// hf:trainer.py:1780-1796 -> clip_grad_norm_(max_norm=1.0) then torch.optim.AdamW(betas=(0.9,0.999),
// eps=1e-8, weight_decay=0.0).step(), then model.zero_grad().
#include "common.h"
#include "stonk_flags.h"

namespace {

// Sum of squares in a FIXED order: every block leaves its partial sum in a slot, the last block to finish (ticket) adds
// the slots up in index order. With one atomicAdd per block the result depended on arrival order in its last bits - and
// with it the clip coefficient and every parameter update, so data-parallel ranks holding identical summed gradients
// drifted apart by an ulp per step (found with tools/dp_check.py). Slots and ticket live in a CALLER workspace
// (stonk_sumsq_workspace_floats(): SUMSQ_MAX_BLOCKS slots + the ticket word, zeroed once by the caller; the kernel
// leaves the ticket at zero), so launches on different streams with different workspaces do not meet.
// Grid cap = number of partial-sum slots. Fewer, longer-running workgroups stream better: alone on 974 MB (tools/sumsq_probe.py,
// us) 256 blocks 181, 384: 179, 512: 193, 768: 213, 1024: 279 (3.5 TB/s - the round-3 value), 2048: 376, 4096: 569.
#ifndef STONK_SUMSQ_BLOCKS
#define STONK_SUMSQ_BLOCKS 256
#endif
constexpr int SUMSQ_MAX_BLOCKS = STONK_SUMSQ_BLOCKS;

// `extra` (nullable, stonk_sumsq_f32_plus): n_extra sums of squares somebody else has taken already (the per-tile sums a
// store-mode weight gradient leaves, stonk_gemm_tn_bf16_store_sumsq). The last block adds them to its total in index order,
// behind the partial slots - still one fixed order, and no launch of its own on the serial path: the extras are cut into 64
// consecutive runs of ceil(n_extra / 64), lane r of the first wave adds run r up element by element, and the 64 run sums
// are added to the total one after the other. All of it in fp64, rounded to fp32 once at the end: in fp32, a thousand
// small addends each rounded at the size of the running total left the norm 6e-6 off (90 ulp; the full pass is within
// one). (One thread adding all 3 414 slots of the flagship's decoders one by one was a dependent chain of 35 us.)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, long n, float* __restrict__ out,
                                                    float* __restrict__ g_sumsq_part, unsigned* __restrict__ ticket,
                                                    const float* __restrict__ extra, long n_extra) {
  float acc = 0.f;
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  // four 16-byte loads requested before the first is used (a pure read of 974 MB: with one load in flight per thread it ran
  // at 3.4 TB/s); the summation order stays a function of (n, grid) alone - the same bits on every launch and rank
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const f32x4 v0 = *(const f32x4*)(x + 4 * i), v1 = *(const f32x4*)(x + 4 * (i + stride)),
                v2 = *(const f32x4*)(x + 4 * (i + 2 * stride)), v3 = *(const f32x4*)(x + 4 * (i + 3 * stride));
    acc += v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2] + v0[3] * v0[3];
    acc += v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2] + v1[3] * v1[3];
    acc += v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2] + v2[3] * v2[3];
    acc += v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2] + v3[3] * v3[3];
  }
  for (; i < n4; i += stride) {
    const f32x4 v = *(const f32x4*)(x + 4 * i);
    acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) acc += x[i] * x[i];
  acc = wave_sum(acc);
  __shared__ float part[4];
  __shared__ bool last;
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(&g_sumsq_part[blockIdx.x], part[0] + part[1] + part[2] + part[3], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();   // the slot is visible device-wide before the ticket is taken
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == gridDim.x - 1);
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  float tot = 0.f;   // 256 threads: strided slots, then a fixed tree - the same order on every launch and every rank
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256)
    tot += __hip_atomic_load(&g_sumsq_part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tot = wave_sum(tot);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = tot;
  __syncthreads();
  tot = (part[0] + part[1]) + (part[2] + part[3]);
  if (n_extra > 0) {   // (a kernel argument: uniform)
    __shared__ double run[64];
    if (threadIdx.x < 64) {
      const long per = (n_extra + 63) >> 6, lo = threadIdx.x * per, hi = lo + per < n_extra ? lo + per : n_extra;
      double a = 0.0;
      for (long i = lo; i < hi; ++i) a += (double)extra[i];
      run[threadIdx.x] = a;
    }
    __syncthreads();
    double wide = tot;
    for (int r = 0; r < 64; ++r) wide += run[r];
    tot = (float)wide;
  }
  if (threadIdx.x == 0) {
    atomicAdd(out, tot);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
  }
}

// One pass over the flat buffers: p, g, m, v read; p, m, v, bf16(p) written; g zeroed - 34 bytes per parameter, each touched
// once per step (8.3 GB at 243 M parameters: nothing a cache could keep). HBM-bound. Round 4 (tools/adamw_ab.py, 243 M
// elements, one box): 1, 2 or 4 groups requested per thread before the first use, default or non-temporal accesses -
// 4.30 / 4.41 / 4.27 TB/s and 4.25 / 4.39 / 4.40: the mix of four read and five write streams runs at 4.3-4.4 TB/s whatever
// a thread keeps in flight (a plain copy reaches 6.3 on this chip). Two groups, default policy.
//
// The training step with replicated optimizer state runs the TILED form further down (stonk_adamw_step_tiled) instead:
// + 2 bytes for the W^T tile, - 4 where the gradient is not zeroed (the two decoders, 156.8 M parameters, whose next
// gradient is stored rather than accumulated) - 36 bytes per parameter for a dgrad weight, 32 for the decoders, 33.4 on
// average over the flagship's 243 M: 8.13 GB, and no separate transpose pass (profiles/optimizer_boundary.md).
#ifndef STONK_ADAMW_UNROLL
#define STONK_ADAMW_UNROLL 2
#endif
#ifndef STONK_ADAMW_NT
#define STONK_ADAMW_NT 0
#endif
#ifndef STONK_ADAMW_BLOCKS
// grid cap. Alone on 243 M elements (ADAMW_AB=blocks tools/adamw_ab.py, us): 256 blocks 1516, 512: 1588, 1024: 1715, 4096: 1735 -
// but IN THE STEP 256 blocks cost +1.6 ms (27.9-28.4 against 26.3-26.7 ms, tools/ab_libs.sh): the kernel runs on the optimizer
// stream beside the next step's first launches, and 256 long-lived workgroups are placed once, on whatever CUs are free at
// that moment, where 4096 short ones follow the CUs as they come free. (The gradient-norm pass before it does gain from
// its 256 blocks in the step: -0.15 ms.)
#define STONK_ADAMW_BLOCKS 4096
#endif
template <typename T>
__device__ __forceinline__ T stream_load(const T* q) {
#if STONK_ADAMW_NT
  return __builtin_nontemporal_load(q);
#else
  return *q;
#endif
}
template <typename T>
__device__ __forceinline__ void stream_store(T* q, const T& x) {
#if STONK_ADAMW_NT
  __builtin_nontemporal_store(x, q);
#else
  *q = x;
#endif
}
// true when element e lies inside one of the n sorted [lo, hi) spans (bisection: last span whose start <= e)
__device__ __forceinline__ bool in_spans(const long* __restrict__ spans, int n, long e) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (spans[2 * mid] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo != 0 && e < spans[2 * (lo - 1) + 1];
}
// the last of the n entries of a table sorted by first(i) whose first(i) <= bid: the entry that owns workgroup `bid` of a
// launch whose grid is the sum of the entries' workgroup counts (first(0) = 0)
template <typename B, typename F>
__device__ __forceinline__ int last_entry_at_or_below(int n, B bid, F first) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(mid) <= bid) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The scalars every AdamW kernel derives once per thread, and the update of one group of four elements: ONE definition,
// so that the flat kernel, its span form and the tiled kernel produce the same bits from the same inputs.
struct AdamwConsts {
  float coef, step, inv_sqrt_bc2;
};
__device__ __forceinline__ AdamwConsts adamw_consts(float lr, float bc1, float bc2, const float* __restrict__ gnorm_sq,
                                                    float max_norm, float grad_scale) {
  AdamwConsts c;
  c.coef = grad_scale;
  if (gnorm_sq && max_norm > 0.f) {
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
    const float total = sqrtf(*gnorm_sq) * grad_scale;
    const float cc = max_norm / (total + 1e-6f);
    c.coef *= cc < 1.f ? cc : 1.f;
  }
  c.step = lr / bc1;
  c.inv_sqrt_bc2 = rsqrtf(bc2);
  return c;
}
// decoupled weight decay: everywhere (no table), or on the elements inside one of the sorted [lo, hi) spans of the
// flat buffer (HF Trainer's grouping: weights yes, biases and LayerNorm no). Tensors start at multiples of 256
// elements, so the four elements of a group share the answer.
__device__ __forceinline__ float adamw_keep(float lr, float wd, const long* __restrict__ decay_spans, int n_spans, long e) {
  float keep = 1.f - lr * wd;
  if (decay_spans && wd != 0.f && !in_spans(decay_spans, n_spans, e)) keep = 1.f;
  return keep;
}
// (Left to -ffp-contract=fast, as the flat kernel always was: which multiply-adds the compiler fuses decides the last bit,
// and spelling the fusion out by hand did not reproduce the bits the flat kernel has produced so far - tried: m' as
// fma(1 - b1, g, b1 m), v' as fma(b2, v, (1 - b2) g g), as its instruction stream reads - so the expression stays as it
// was and tests/test_optim_tiled_gpu.py holds the three kernels to each other bit for bit on every build.)
__device__ __forceinline__ bf16x4 adamw_update4(f32x4& pp, const f32x4& gg, f32x4& mm, f32x4& vv, const AdamwConsts& c,
                                                float keep, float b1, float b2, float eps) {
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gr = gg[j] * c.coef;
    float w = pp[j] * keep;
    mm[j] = b1 * mm[j] + (1.f - b1) * gr;
    vv[j] = b2 * vv[j] + (1.f - b2) * gr * gr;
    const float denom = sqrtf(vv[j]) * c.inv_sqrt_bc2 + eps;
    w -= c.step * (mm[j] / denom);
    pp[j] = w;
    o[j] = (bf16)w;
  }
  return o;
}

// `keep_grad` (nullable): sorted [lo, hi) spans of the flat buffer whose gradient is NOT zeroed - the next step's weight
// gradient overwrites them (store-mode epilogue of the unsplit decoder gradients), so the 4 bytes per parameter of
// zeroing would be written for nothing.
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16* __restrict__ pb, long n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2,
                                                    const float* __restrict__ gnorm_sq, float max_norm,
                                                    float grad_scale, const long* __restrict__ decay_spans,
                                                    int n_spans, long span_base, const long* __restrict__ keep_grad,
                                                    int n_keep) {
  constexpr int U = STONK_ADAMW_UNROLL;
  const AdamwConsts c = adamw_consts(lr, bc1, bc2, gnorm_sq, max_norm, grad_scale);
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * 256;
  for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += stride * U) {
    f32x4 pp[U], gg[U], mm[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i < n4) {
        pp[u] = stream_load((const f32x4*)(p + 4 * i));
        gg[u] = stream_load((const f32x4*)(g + 4 * i));
        mm[u] = stream_load((const f32x4*)(m + 4 * i));
        vv[u] = stream_load((const f32x4*)(v + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i >= n4) break;
      const float keep = adamw_keep(lr, wd, decay_spans, n_spans, span_base + 4 * i);
      const bf16x4 o = adamw_update4(pp[u], gg[u], mm[u], vv[u], c, keep, b1, b2, eps);
      stream_store((f32x4*)(p + 4 * i), pp[u]);
      stream_store((f32x4*)(m + 4 * i), mm[u]);
      stream_store((f32x4*)(v + 4 * i), vv[u]);
      if (!(keep_grad && in_spans(keep_grad, n_keep, span_base + 4 * i)))
        stream_store((f32x4*)(g + 4 * i), (f32x4){0.f, 0.f, 0.f, 0.f});
      if (pb) *(bf16x4*)(pb + 4 * i) = o;   // (read again by the next forward: default policy)
    }
  }
}

// The flat update over a device-side list of spans in ONE launch (what the tiled kernel below leaves: biases, LayerNorm,
// embeddings, pooler, NSP head and the alignment gaps between tensors - about fifty pieces, 1.2 M elements): `spans` =
// n entries {lo, hi, first_chunk} sorted by first_chunk, a workgroup takes one chunk of 1024 elements of one span.
constexpr int ADAMW_CHUNK = 1024;
__global__ __launch_bounds__(256) void adamw_spans_kernel(float* __restrict__ p, float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          bf16* __restrict__ pb, const long* __restrict__ spans, int n,
                                                          float lr, float b1, float b2, float eps, float wd, float bc1,
                                                          float bc2, const float* __restrict__ gnorm_sq, float max_norm,
                                                          float grad_scale, const long* __restrict__ decay_spans,
                                                          int n_spans, const long* __restrict__ keep_grad, int n_keep) {
  const long bid = blockIdx.x;
  const int lo = last_entry_at_or_below(n, bid, [&](int i) { return spans[3 * i + 2]; });
  const long e = spans[3 * lo] + (bid - spans[3 * lo + 2]) * ADAMW_CHUNK + 4 * threadIdx.x;
  if (e >= spans[3 * lo + 1]) return;
  const AdamwConsts c = adamw_consts(lr, bc1, bc2, gnorm_sq, max_norm, grad_scale);
  f32x4 pp = *(const f32x4*)(p + e), gg = *(const f32x4*)(g + e), mm = *(const f32x4*)(m + e), vv = *(const f32x4*)(v + e);
  const float keep = adamw_keep(lr, wd, decay_spans, n_spans, e);
  const bf16x4 o = adamw_update4(pp, gg, mm, vv, c, keep, b1, b2, eps);
  *(f32x4*)(p + e) = pp;
  *(f32x4*)(m + e) = mm;
  *(f32x4*)(v + e) = vv;
  if (!(keep_grad && in_spans(keep_grad, n_keep, e))) *(f32x4*)(g + e) = (f32x4){0.f, 0.f, 0.f, 0.f};
  *(bf16x4*)(pb + e) = o;
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, long n, float s) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] *= s;
}

__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ x, bf16* __restrict__ y, long n) {
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = *(const f32x4*)(x + 4 * i);
    *(bf16x4*)(y + 4 * i) = (bf16x4){(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) y[i] = (bf16)x[i];
}

// 64x64 tile transpose through LDS. SrcT = bf16 or float; output bf16. Rows at or past *rows_dev read as zero
// (label-sparse decoder operands); optional column sums of the source (bias gradients) via atomics.
constexpr int TT = 64;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
__device__ __forceinline__ unsigned short bf16_bits(float f) {
  const bf16 b = (bf16)f;
  unsigned short u;
  __builtin_memcpy(&u, &b, 2);
  return u;
}
__device__ __forceinline__ float bits_to_float(unsigned short u) {
  return __uint_as_float(((unsigned)u) << 16);
}
// The store half of a 64x64 tile transpose: thread t writes out row c0 + (t >> 2), sixteen source rows (r0 + 16 (t & 3) ...)
// = 32 contiguous bytes, from the tile in LDS. For the threads whose out row exists: if (c0 + (t >> 2) < cols) at the call
// (with the test in here the compiler lays the branch out differently).
__device__ __forceinline__ void store_tile_transposed(const unsigned short (&tile)[TT][TT + 2], bf16* out, long ld_out, long r0,
                                                      int c0, int t) {
  const int oc = t >> 2, rb = (t & 3) * 16;
  u16x8 o0, o1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o0[j] = tile[rb + j][oc];
    o1[j] = tile[rb + 8 + j][oc];
  }
  bf16* dst = out + (long)(c0 + oc) * ld_out + r0 + rb;
  *(u16x8*)dst = o0;
  *(u16x8*)(dst + 8) = o1;
}

template <typename SrcT>
__global__ __launch_bounds__(256) void transpose_kernel(const SrcT* __restrict__ in, long ld_in, bf16* __restrict__ out,
                                                        long ld_out, long rows, int cols, float* __restrict__ colsum,
                                                        const int* __restrict__ rows_dev) {
  __shared__ unsigned short tile[TT][TT + 2];
  long live = rows;
  if (rows_dev) {
    const long rd = *rows_dev;
    live = rd < rows ? rd : rows;
  }
  // only tiles up to the 64-row round-up of the live count are ever consumed; blocks walk them with stride gridDim.y
  const long live_tiles = (live + TT - 1) / TT;
  const int t = threadIdx.x;
  const int c0 = blockIdx.x * TT;
  for (long rt = blockIdx.y; rt < live_tiles; rt += gridDim.y) {
    const long r0 = rt * TT;
    // load: thread -> (row = t >> 3 (+32), 8 columns)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int rr = (t >> 3) + 32 * pass;
      const int cc = (t & 7) * 8;
      const long r = r0 + rr;
      unsigned short vals[8];
      if (r < live && c0 + cc < cols) {
        if constexpr (sizeof(SrcT) == 2) {
          const u16x8 v = *(const u16x8*)(in + r * ld_in + c0 + cc);
#pragma unroll
          for (int j = 0; j < 8; ++j) vals[j] = v[j];
        } else {
          const f32x4 a = *(const f32x4*)(in + r * ld_in + c0 + cc);
          const f32x4 b = *(const f32x4*)(in + r * ld_in + c0 + cc + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            vals[j] = bf16_bits(a[j]);
            vals[4 + j] = bf16_bits(b[j]);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = 0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[rr][cc + j] = vals[j];
    }
    __syncthreads();
    if (c0 + (t >> 2) < cols) store_tile_transposed(tile, out, ld_out, r0, c0, t);
    if (colsum && t < TT && c0 + t < cols) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < TT; ++r) s += bits_to_float(tile[r][t]);
      atomicAdd(colsum + c0 + t, s);
    }
    __syncthreads();
  }
}

// Batched form of the bf16 transpose: ONE launch refreshes every W^T copy of the model (57 tensors per optimizer step; as
// separate launches they were 1.2 ms of mostly launch gaps and small grids on the optimizer stream). `desc` is a
// device-side table of n entries {in, out, ld_in, ld_out, rows, cols, first_tile, tiles_per_row}; the grid is the total
// number of 64x64 tiles and a workgroup finds its entry by bisection on first_tile.
struct TransposeDesc {
  const bf16* in;
  bf16* out;
  long ld_in, ld_out, rows;
  int cols, first_tile, col_tiles, pad;
};
__global__ __launch_bounds__(256) void transpose_batched_kernel(const TransposeDesc* __restrict__ desc, int n) {
  __shared__ unsigned short tile[TT][TT + 2];
  const int bid = blockIdx.x;
  const int lo = last_entry_at_or_below(n, bid, [&](int i) { return desc[i].first_tile; });
  const TransposeDesc d = desc[lo];
  const int tl = bid - d.first_tile;
  const long r0 = (long)(tl / d.col_tiles) * TT;
  const int c0 = (tl % d.col_tiles) * TT;
  const int t = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int rr = (t >> 3) + 32 * pass, cc = (t & 7) * 8;
    const long r = r0 + rr;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < d.rows && c0 + cc < d.cols) v = *(const u16x8*)(d.in + r * d.ld_in + c0 + cc);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[rr][cc + j] = v[j];
  }
  __syncthreads();
  if (c0 + (t >> 2) < d.cols) store_tile_transposed(tile, d.out, d.ld_out, r0, c0, t);
}

// AdamW over the 2-D weights that have a W^T copy, one 64x64 tile per workgroup: the update of adamw_kernel (the same
// adamw_update4 on the same four-element groups, so the same bits), the row-major bf16 mirror, and - through LDS - the
// transposed bf16 tile straight into the W^T copy. The separate batched transpose re-read the mirror the optimizer had
// written microseconds before (0.49 GB in, 0.49 GB out, a launch of its own on the serial path); here the transposed tile
// costs its 2 bytes per parameter of writes only. `desc` = n entries sorted by first_tile; an entry covers
// ceil(prows / 64) * col_tiles tiles. prows >= rows are the rows the flat buffers hold (the decoders' pad rows): all of
// them are updated, rows at or past `rows` reach the W^T copy as zeros up to the tile edge and row tiles past
// roundup64(rows) do not touch it - exactly what transpose_batched_kernel writes.
struct AdamwTileDesc {
  long off;   // first element of the tensor in the flat buffers
  bf16* wt;
  long ld_out, rows, prows;
  int cols, first_tile, col_tiles, pad;
};
__global__ __launch_bounds__(256) void adamw_tiled_kernel(float* __restrict__ p, float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          bf16* __restrict__ pb, const AdamwTileDesc* __restrict__ desc,
                                                          int n, float lr, float b1, float b2, float eps, float wd,
                                                          float bc1, float bc2, const float* __restrict__ gnorm_sq,
                                                          float max_norm, float grad_scale,
                                                          const long* __restrict__ decay_spans, int n_spans,
                                                          const long* __restrict__ keep_grad, int n_keep) {
  __shared__ unsigned short tile[TT][TT + 2];
  const int bid = blockIdx.x;
  const int lo = last_entry_at_or_below(n, bid, [&](int i) { return desc[i].first_tile; });
  const AdamwTileDesc d = desc[lo];
  const int tl = bid - d.first_tile;
  const long r0 = (long)(tl / d.col_tiles) * TT;
  const int c0 = (tl % d.col_tiles) * TT;
  const int t = threadIdx.x;
  const int cc = (t & 15) * 4;   // 16 threads = one 256-byte row segment, 16 rows per pass
  const bool col_live = c0 + cc < d.cols;
  const AdamwConsts c = adamw_consts(lr, bc1, bc2, gnorm_sq, max_norm, grad_scale);
  // (one group of four per trip and NOT unrolled: the compiler then emits for adamw_update4 the instruction sequence it
  // emits in the flat kernels - unrolled, it paired operations across the trips differently and single results differed in
  // their last bit; the bitwise test guards this. 59 000 short workgroups keep enough loads in flight without a thread
  // queueing its own)
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int rr = (t >> 4) + 16 * pass;
    const long r = r0 + rr;
    unsigned short bits[4] = {0, 0, 0, 0};
    if (col_live && r < d.prows) {
      const long e = d.off + r * d.cols + c0 + cc;
      f32x4 pp = *(const f32x4*)(p + e), gg = *(const f32x4*)(g + e), mm = *(const f32x4*)(m + e), vv = *(const f32x4*)(v + e);
      const float keep = adamw_keep(lr, wd, decay_spans, n_spans, e);
      const bf16x4 o = adamw_update4(pp, gg, mm, vv, c, keep, b1, b2, eps);
      *(f32x4*)(p + e) = pp;
      *(f32x4*)(m + e) = mm;
      *(f32x4*)(v + e) = vv;
      if (!(keep_grad && in_spans(keep_grad, n_keep, e))) *(f32x4*)(g + e) = (f32x4){0.f, 0.f, 0.f, 0.f};
      *(bf16x4*)(pb + e) = o;
      if (r < d.rows) __builtin_memcpy(bits, &o, 8);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[rr][cc + j] = bits[j];
  }
  if (r0 >= d.rows) return;   // (pad rows past the W^T copy's last tile; uniform over the workgroup)
  __syncthreads();
  if (c0 + (t >> 2) < d.cols) store_tile_transposed(tile, d.wt, d.ld_out, r0, c0, t);
}

// grid of the elementwise kernels: a thread takes four elements at a time; at most 4096 workgroups, or `cap` if that is fewer
inline unsigned ew_grid(long n, long cap = 4096) { return grid_cap(n / 4, 256, cap < 4096 ? cap : 4096); }

// One launch of transpose_kernel<SrcT> after the checks the two entry points share. With `rows_dev` the live row count is
// unknown on the host: the grid is bounded at 64 row tiles and the workgroups stride.
template <typename SrcT>
int transpose_launch(const SrcT* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int cols, float* colsum,
                     const int* rows_dev, void* stream) {
  STONK_CHECK_ARG(in && out && rows >= 0 && cols > 0, STONK_EINVAL);
  STONK_CHECK_ARG(cols % 8 == 0 && ld_in % 8 == 0 && ld_out % 8 == 0, STONK_EALIGN);
  STONK_CHECK_ARG(ld_out >= ((rows + TT - 1) / TT) * TT, STONK_ESHAPE);
  if (rows == 0) return STONK_OK;
  const dim3 grid((cols + TT - 1) / TT, grid_cap(rows, TT, rows_dev ? 64 : 65535));
  hipLaunchKernelGGL((transpose_kernel<SrcT>), grid, dim3(256), 0, (hipStream_t)stream, in, (long)ld_in, (bf16*)out,
                     (long)ld_out, (long)rows, cols, colsum, rows_dev);
  return stonk_launch_status();
}

}  // namespace

extern "C" int64_t stonk_sumsq_workspace_floats(void) { return SUMSQ_MAX_BLOCKS + 1; }

// *out_accum += sum(x^2) + extra[0] + extra[1] + ... (stonk_sumsq_f32: no extras; then an empty x launches nothing)
extern "C" int stonk_sumsq_f32_plus(const float* x, int64_t n, float* out_accum, float* workspace, int64_t ws_floats,
                                    const float* extra, int64_t n_extra, void* stream) {
  STONK_CHECK_ARG(x && out_accum && workspace && n >= 0, STONK_EINVAL);
  STONK_CHECK_ARG(n_extra >= 0 && (extra || n_extra == 0), STONK_EINVAL);
  STONK_CHECK_ARG(ws_floats >= SUMSQ_MAX_BLOCKS + 1, STONK_EINVAL);
  STONK_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)workspace % 4 == 0 && (uintptr_t)extra % 4 == 0, STONK_EALIGN);
  if (n == 0 && n_extra == 0) return STONK_OK;
  hipLaunchKernelGGL(sumsq_kernel, dim3(ew_grid(n, SUMSQ_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, (long)n,
                     out_accum, workspace, (unsigned*)(workspace + SUMSQ_MAX_BLOCKS), extra, (long)n_extra);
  return stonk_launch_status();
}

extern "C" int stonk_sumsq_f32(const float* x, int64_t n, float* out_accum, float* workspace, int64_t ws_floats,
                               void* stream) {
  return stonk_sumsq_f32_plus(x, n, out_accum, workspace, ws_floats, nullptr, 0, stream);
}

extern "C" int stonk_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                                const float* gnorm_sq_dev, float max_grad_norm, float grad_scale,
                                const int64_t* decay_spans, int n_spans, int64_t span_base, void* stream) {
  STONK_CHECK_ARG(p && g && m && v && n >= 0 && n % 4 == 0, STONK_EINVAL);
  STONK_CHECK_ARG(n_spans >= 0 && (decay_spans || n_spans == 0) && span_base >= 0 && span_base % 4 == 0, STONK_EINVAL);
  STONK_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0, STONK_EALIGN);
  STONK_CHECK_ARG(bias_corr1 > 0.f && bias_corr2 > 0.f, STONK_EINVAL);
  if (n == 0) return STONK_OK;
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_grid(n, STONK_ADAMW_BLOCKS)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     (bf16*)p_bf16, (long)n, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, gnorm_sq_dev,
                     max_grad_norm, grad_scale, (const long*)decay_spans, n_spans, (long)span_base, (const long*)nullptr, 0);
  return stonk_launch_status();
}

// The optimizer step of the WHOLE flat buffers with the W^T copies written in the same pass: adamw_tiled_kernel over the
// tensors of `tile_desc_dev`, adamw_spans_kernel over `flat_spans_dev` = everything else. The tables are device memory the
// launcher cannot read: the caller guarantees that the two cover [0, n) exactly once, that offsets and span ends are
// multiples of 4, cols % 8 == 0, W^T copies 16-byte aligned with ld_out % 8 == 0 and ld_out >= roundup64(rows).
extern "C" int stonk_adamw_step_tiled(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                                      float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                                      float bias_corr2, const float* gnorm_sq_dev, float max_grad_norm, float grad_scale,
                                      const int64_t* decay_spans, int n_spans, const int64_t* keep_grad_spans, int n_keep,
                                      const void* tile_desc_dev, int n_desc, int total_tiles,
                                      const int64_t* flat_spans_dev, int n_flat, int total_chunks, void* stream) {
  STONK_CHECK_ARG(p && g && m && v && p_bf16 && n >= 0 && n % 4 == 0, STONK_EINVAL);
  STONK_CHECK_ARG(n_spans >= 0 && (decay_spans || n_spans == 0) && n_keep >= 0 && (keep_grad_spans || n_keep == 0),
                  STONK_EINVAL);
  STONK_CHECK_ARG(tile_desc_dev && n_desc > 0 && total_tiles > 0, STONK_EINVAL);
  STONK_CHECK_ARG(n_flat >= 0 && total_chunks >= 0 && (n_flat == 0) == (total_chunks == 0) && (flat_spans_dev || n_flat == 0),
                  STONK_EINVAL);
  STONK_CHECK_ARG(bias_corr1 > 0.f && bias_corr2 > 0.f, STONK_EINVAL);
  STONK_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0 && (uintptr_t)p_bf16 % 8 == 0,
                  STONK_EALIGN);
  STONK_CHECK_ARG(((uintptr_t)tile_desc_dev | (uintptr_t)flat_spans_dev | (uintptr_t)decay_spans |
                   (uintptr_t)keep_grad_spans) % 8 == 0, STONK_EALIGN);
  if (n == 0) return STONK_OK;
  hipLaunchKernelGGL(adamw_tiled_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16*)p_bf16,
                     (const AdamwTileDesc*)tile_desc_dev, n_desc, lr, beta1, beta2, eps, weight_decay, bias_corr1,
                     bias_corr2, gnorm_sq_dev, max_grad_norm, grad_scale, (const long*)decay_spans, n_spans,
                     (const long*)keep_grad_spans, n_keep);
  if (n_flat > 0)
    hipLaunchKernelGGL(adamw_spans_kernel, dim3(total_chunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       (bf16*)p_bf16, (const long*)flat_spans_dev, n_flat, lr, beta1, beta2, eps, weight_decay,
                       bias_corr1, bias_corr2, gnorm_sq_dev, max_grad_norm, grad_scale, (const long*)decay_spans, n_spans,
                       (const long*)keep_grad_spans, n_keep);
  return stonk_launch_status();
}

extern "C" int stonk_scale_f32(float* x, int64_t n, float s, void* stream) {
  STONK_CHECK_ARG(x && n >= 0, STONK_EINVAL);
  if (n == 0) return STONK_OK;
  hipLaunchKernelGGL(scale_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, (long)n, s);
  return stonk_launch_status();
}

extern "C" int stonk_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream) {
  STONK_CHECK_ARG(x && y && n >= 0, STONK_EINVAL);
  STONK_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)y % 8 == 0, STONK_EALIGN);
  if (n == 0) return STONK_OK;
  hipLaunchKernelGGL(cast_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, (bf16*)y, (long)n);
  return stonk_launch_status();
}

// out[c][r] = in[r][c] for r < rows (rows >= *rows_dev read as zero), c < cols. out needs ld_out >= roundup(rows, 64).
extern "C" int stonk_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int cols,
                                    float* colsum, const int* rows_dev, void* stream) {
  return transpose_launch((const bf16*)in, ld_in, out, ld_out, rows, cols, colsum, rows_dev, stream);
}

extern "C" int stonk_transpose_bf16_batched(const void* desc_dev, int n, int total_tiles, void* stream) {
  STONK_CHECK_ARG(desc_dev && n > 0 && total_tiles > 0, STONK_EINVAL);
  STONK_CHECK_ARG((uintptr_t)desc_dev % 8 == 0, STONK_EALIGN);
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream,
                     (const TransposeDesc*)desc_dev, n);
  return stonk_launch_status();
}

// bf16 W^T copy of a dense fp32 [rows, cols] master weight: out[c][r] = bf16(in[r][c])
extern "C" int stonk_transpose_f32_to_bf16(const float* in, void* out, int64_t rows, int cols, int64_t ld_out,
                                           void* stream) {
  return transpose_launch(in, cols, out, ld_out, rows, cols, (float*)nullptr, (const int*)nullptr, stream);   // (dense: ld_in = cols)
}

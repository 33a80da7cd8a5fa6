// The knowledge-graph-only baseline of ref:src/stonkgs/models/kg_baseline_model.py: the walks of a triple's two entities are
// looked up in a node2vec (or TransE) table, max-pooled per dimension, and a dropout + linear + softmax classifier is trained
// on the pooled vectors by AdamW, five cross-validation folds at a time. stonkgs_amd/kg_baseline_model.py is the host side;
// tests/test_kg_baseline_cpu.py restates the dropout rule and one optimizer step in numpy / torch.
//
// POOLING (stonk_walk_maxpool). One wavefront per example; a lane holds 16-byte chunks {j * 64 + lane} of a table row
// (every load instruction covers 1 KiB of the row), D / 4 chunks in all, so at D 64 only lanes 0 .. 15 carry data. Two
// register sets take turns as in link_prediction.hip: the id two rows ahead is requested first, then the next row, then
// the current row is folded into the running maximum with the next one in flight. A position past the end re-reads the
// last row (a maximum does not mind), so the loop is straight-line code and the loads can be counted. Id -1 is the
// reference's null vector: a row of zeros that takes part in the maximum (row 0 is read in its place and discarded).
// v_max_f32 drops a NaN operand, so a NaN in the table is NOT propagated the way torch.max does; for a finite table the
// result is bit-identical to torch.max(x, dim=1).values.
//
// TRAINING (stonk_kgb_train_steps). One workgroup of 256 threads per run (fold), blockIdx.x = run; a launch walks up to
// STONK_KGB_MAX_STEPS consecutive optimizer steps of every run with the whole model on chip.
//   ON-CHIP LAYOUT. Thread t owns the feature columns d = t + 256 k, k = 0 .. 3 (D <= 1024), of EVERY class: W[c][d],
//   m[c][d], v[c][d] (3 x 16 x 4 floats at C 16, D 1024) and the step's gradient (16 x 4 doubles, see below) live in its
//   registers: 320 of them at that shape, so the kernel is compiled for one wavefront per SIMD and uses the whole
//   512-register file (no scratch). Why columns and not rows: the weight
//   gradient dW[c][d] = sum_i g[i][c] h[i][d] and the AdamW update then need nothing from another thread - a column owner
//   reads its own h[i][d] and the B x C numbers g, which sit in LDS - so the only cross-thread reduction of a step is the
//   forward dot product z[i][c], B x C numbers: one butterfly per row within each wavefront that carries all classes and
//   halves them from stage to stage (kgb_reduce_classes), then the four wavefronts' partial sums
//   are added in the order 0, 1, 2, 3 by the thread that owns row i. The bias, its moments and its gradient are thread
//   c's; a copy of b is kept in LDS for the forward pass.
//   A STEP. (A) threads i < batch publish row i's example index, label and class weight (validated) in LDS; (B) rows are
//   taken eight at a time: all loads of a chunk are issued together, dropout is applied, and every class's partial dot
//   product is reduced; (C) thread i finishes row i: z, q = softmax(z), r = softmax(q) - the reference hands PROBABILITIES
//   to CrossEntropyLoss, which takes a second log-softmax - the weighted loss term, and the gradient through both
//   softmaxes, dz[i][c], to LDS; (D) every thread accumulates its columns' gradient over the rows in the order 0 .. B - 1
//   and applies torch.optim.AdamW's update (decoupled decay first, then the moments, bias corrections by the global step
//   number). THE GRADIENT IS FORMED IN FP64 - dot products, both softmaxes, dz and the sums over the rows - and rounded to
//   fp32 once, where AdamW takes it: on its first steps AdamW's update is lr * g / (|g| + eps), and for a gradient element
//   that nearly cancels (|g| of the order of eps = 1e-8, sums of terms near 1e-3) an fp32 summation error of 1e-10 moves
//   the weight by 1e-7, twenty times its rounding. Parameters and moments are fp32, as torch's.
//   Four __syncthreads per step, no other synchronisation, no float atomics: equal inputs give equal bits.
//   With batch <= 8 the rows read in (B) stay in registers for (D); larger batches re-read them (they are in L2).
//   The order entries and labels of the next two steps are requested a step ahead, so that their latency is not paid in
//   line.
//   DROPOUT. stepkey = H( H(mix(seed) + run) ^ (global step * 0x9E3779B1) ) (n2v_key of graph_common.h over stonk_seed_mix),
//   keep(i, d) = stonk_keep(row = i, col = d, stepkey, thr32) of common.h: a pure function of (seed, run, global step, row
//   in batch, feature). Kept values are multiplied by 1 / (1 - p).
//   BIAS CORRECTIONS. beta^t by repeated squaring in fp64 - a function of t alone, so cutting a span elsewhere changes no
//   bit - then step_size = lr / (1 - beta1^t) and sqrt(1 - beta2^t) are rounded to fp32 as torch does with its scalars.
//
// PREDICTION (stonk_kgb_predict). Eval mode: one wavefront per example, a lane holds elements {j * 64 + lane} of the pooled
// row, W is read from global memory (it is 64 KiB at most and stays in cache). The arg-max is taken over the
// probabilities; the LOWEST index wins a tie, as torch.argmax does on a first maximum.
#include <math.h>

#include "graph_common.h"

// Longest span of steps one launch may walk, chosen so that the longest launch (D 1024, C 16, batch 64) stays below
// 100 ms on a shared machine. profiles/kg_baseline.md holds the measured time per step at that shape and the arithmetic.
#define STONK_KGB_MAX_STEPS 256
#define STONK_KGB_THREADS 256
#define STONK_KGB_COLS 4        // feature columns per thread: 4 x 256 = D up to 1024
#define STONK_KGB_MAX_BATCH 64
#define STONK_KGB_MAX_CLASSES 16
#define STONK_KGB_CHUNK 8       // rows whose loads are in flight together

namespace {

// ------------------------------------------------------------------------------------------------------------ pooling
__device__ __forceinline__ int pool_id(const int* __restrict__ row, int t, int L) { return row[t < L ? t : L - 1]; }

template <int NV>
__device__ __forceinline__ void pool_load(const float* __restrict__ table, long ld, int id, int N, int lane, int D4,
                                          f32x4 (&r)[NV]) {
  const f32x4* p = (const f32x4*)(table + (long)((unsigned)id < (unsigned)N ? id : 0) * ld);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = j * 64 + lane;
    r[j] = p[c < D4 ? c : 0];   // (a lane without a chunk re-reads chunk 0 and never stores)
  }
}

template <int NV>
__device__ __forceinline__ void pool_fold(int id, int N, const f32x4 (&r)[NV], f32x4 (&acc)[NV], bool& bad) {
  const bool ok = (unsigned)id < (unsigned)N;
  bad |= id < -1 || id >= N;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[j][q] = fmaxf(acc[j][q], ok ? r[j][q] : 0.f);
}

template <int NV>
__global__ __launch_bounds__(256) void walk_maxpool_kernel(const int* __restrict__ ids, long ld_ids, long n, int L,
                                                           const float* __restrict__ table, long ld_table, int N, int D4,
                                                           float* __restrict__ pooled, long ld_pooled,
                                                           int* __restrict__ errors) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n) return;
  const int* row = ids + e * ld_ids;
  f32x4 acc[NV], ra[NV], rb[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  int idA = pool_id(row, 0, L), idB = pool_id(row, 1, L);
  __builtin_amdgcn_sched_barrier(0);   // (the id loads stay ahead of the row loads)
  pool_load<NV>(table, ld_table, idA, N, lane, D4, ra);
  for (int t = 0;;) {
    const int idC = pool_id(row, t + 2, L);
    __builtin_amdgcn_sched_barrier(0);
    pool_load<NV>(table, ld_table, idB, N, lane, D4, rb);
    __builtin_amdgcn_sched_barrier(0);
    pool_fold<NV>(idA, N, ra, acc, bad);
    if (++t >= L) break;
    const int idD = pool_id(row, t + 2, L);
    __builtin_amdgcn_sched_barrier(0);
    pool_load<NV>(table, ld_table, idC, N, lane, D4, ra);
    __builtin_amdgcn_sched_barrier(0);
    pool_fold<NV>(idB, N, rb, acc, bad);
    if (++t >= L) break;
    idA = idC;
    idB = idD;
  }
  f32x4* out = (f32x4*)(pooled + e * ld_pooled);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = j * 64 + lane;
    if (c < D4) out[c] = bad ? f32x4{NAN, NAN, NAN, NAN} : acc[j];
  }
  if (bad && lane == 0) atomicAdd(errors, 1);
}

// ------------------------------------------------------------------------------------------------------------ training
struct KgbTrain {
  const float* pooled;
  long ld_pooled, n;
  const int* labels;
  const int* order;
  long ld_order;
  const int* n_steps;
  const int* first_step;
  const float* class_weights;
  float *W, *b, *mW, *vW, *mb, *vb, *loss;
  long ld_loss;
  int* errors;
  int D, C, batch, n_steps_max;
  double lr, beta1, beta2;                       // (fp64 as torch's Python scalars: 1 - 0.999f is off by 1.3e-5 of itself)
  float beta2_f, one_minus_beta1, one_minus_beta2, decay, eps, drop_scale;
  uint32_t seedkey, thr32;
};

// The wavefront's sums of CM values per lane, all classes in one butterfly: in stage s the lanes with bit (5 - s) clear keep
// the lower half of the values still held and hand the upper half to their partner, and the other way round, so the number
// of shuffles halves with every stage (CM - 1 in all, then log2(64 / CM) on the one value left, instead of 6 CM; the caller takes eight classes at a time at most). Returns
// the total of class `lane / (64 / CM)`, the same in the 64 / CM lanes of that group. A fixed order of additions.
// (rank_reduce32 of transe.hip is the same algorithm in fp32 over 32 values.)
template <int CM>
__device__ __forceinline__ double kgb_reduce_classes(double (&v)[CM], int lane) {
  int o = 32;
#pragma unroll
  for (int half = CM / 2; half >= 1; half >>= 1, o >>= 1) {
    const bool upper = (lane & o) != 0;
#pragma unroll
    for (int j = 0; j < half; ++j) {
      const double send = upper ? v[j] : v[j + half];
      const double keep = upper ? v[j + half] : v[j];
      v[j] = keep + __shfl_xor(send, o, 64);
    }
  }
  double t = v[0];
#pragma unroll
  for (; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

__device__ __forceinline__ double kgb_ipow(double x, uint32_t t) {   // x^t by squaring: a function of (x, t) alone
  double r = 1.0;
  for (; t; t >>= 1) {
    if (t & 1u) r *= x;
    x *= x;
  }
  return r;
}

// torch.optim.AdamW, one element: decoupled decay, the moments, the bias-corrected update
__device__ __forceinline__ void kgb_adamw(float& p, float& m, float& v, float g, const KgbTrain& a, float step_size,
                                          float bc2_sqrt) {
  p *= a.decay;
  m += (g - m) * a.one_minus_beta1;
  v = v * a.beta2_f + a.one_minus_beta2 * g * g;
  p -= step_size * (m / (sqrtf(v) / bc2_sqrt + a.eps));
}

template <int CM>
__device__ __forceinline__ void kgb_load_chunk(const KgbTrain& a, const int* s_idx, int i0, int tid, uint32_t stepkey,
                                               float (&h)[STONK_KGB_CHUNK][STONK_KGB_COLS]) {
  // every load is issued whatever the data says (a padded or refused row reads row 0 and is zeroed afterwards)
#pragma unroll
  for (int r = 0; r < STONK_KGB_CHUNK; ++r) {
    const int i = i0 + r;
    const int idx = i < a.batch ? s_idx[i] : -1;
    const float* x = a.pooled + (long)(idx >= 0 ? idx : 0) * a.ld_pooled;
#pragma unroll
    for (int k = 0; k < STONK_KGB_COLS; ++k) {
      const int d = tid + k * STONK_KGB_THREADS;
      h[r][k] = x[d < a.D ? d : 0];
    }
  }
#pragma unroll
  for (int r = 0; r < STONK_KGB_CHUNK; ++r) {
    const int i = i0 + r;
    const bool live = i < a.batch && s_idx[i] >= 0;
    const uint32_t rowkey = stonk_rowkey((uint32_t)i, stepkey);
#pragma unroll
    for (int k = 0; k < STONK_KGB_COLS; ++k) {
      const int d = tid + k * STONK_KGB_THREADS;
      const bool keep = live && d < a.D && stonk_keep_key(rowkey, stonk_colkey((uint32_t)d), a.thr32);
      h[r][k] = keep ? h[r][k] * a.drop_scale : 0.f;
    }
  }
}

template <int CM>
__global__ __launch_bounds__(STONK_KGB_THREADS) void kgb_train_kernel(const KgbTrain a) {
  __shared__ double s_zp[4][STONK_KGB_MAX_BATCH][CM + 1];
  __shared__ double s_gz[STONK_KGB_MAX_BATCH][CM];
  __shared__ double s_wy[STONK_KGB_MAX_BATCH], s_num[STONK_KGB_MAX_BATCH];
  __shared__ float s_b[STONK_KGB_MAX_CLASSES], s_cw[STONK_KGB_MAX_CLASSES];
  __shared__ int s_idx[STONK_KGB_MAX_BATCH], s_y[STONK_KGB_MAX_BATCH], s_err;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, run = blockIdx.x;
  const int C = a.C, D = a.D, batch = a.batch;
  int ns = a.n_steps[run];
  ns = ns < a.n_steps_max ? ns : a.n_steps_max;
  ns = ns < STONK_KGB_MAX_STEPS ? ns : STONK_KGB_MAX_STEPS;
  const uint32_t step0 = (uint32_t)a.first_step[run];
  const long pbase = (long)run * C * D;

  float w[STONK_KGB_COLS][CM], m[STONK_KGB_COLS][CM], v[STONK_KGB_COLS][CM];
#pragma unroll
  for (int k = 0; k < STONK_KGB_COLS; ++k) {
    const int d = tid + k * STONK_KGB_THREADS;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const bool have = d < D && c < C;
      const long o = pbase + (long)(have ? c : 0) * D + (have ? d : 0);
      w[k][c] = have ? a.W[o] : 0.f;
      m[k][c] = have ? a.mW[o] : 0.f;
      v[k][c] = have ? a.vW[o] : 0.f;
    }
  }
  float bias = 0.f, bias_m = 0.f, bias_v = 0.f;
  if (tid < C) {
    bias = a.b[run * C + tid];
    bias_m = a.mb[run * C + tid];
    bias_v = a.vb[run * C + tid];
    s_b[tid] = bias;
    s_cw[tid] = a.class_weights[run * C + tid];
  }
  if (tid == 0) s_err = 0;

  // the order entries of steps 0 and 1 and the labels of step 0 (thread i < batch: row i)
  const int* order = a.order + (long)run * a.ld_order;
  int o_cur = -1, y_cur = 0, o_next = -1;
  if (tid < batch) {
    if (ns > 0) o_cur = order[tid];
    if (ns > 1) o_next = order[batch + tid];
    y_cur = a.labels[(unsigned long)o_cur < (unsigned long)a.n ? o_cur : 0];
  }
  __syncthreads();

  float h[STONK_KGB_CHUNK][STONK_KGB_COLS];
  for (int s = 0; s < ns; ++s) {
    const uint32_t gstep = step0 + (uint32_t)s;
    const uint32_t stepkey = n2v_key(a.seedkey, (uint32_t)run, gstep);
    // ---- (A) the batch's rows: index, label, class weight; the loads of the steps after this one
    if (tid < batch) {
      const bool in_range = (unsigned long)o_cur < (unsigned long)a.n;
      const bool ok = in_range && (unsigned)y_cur < (unsigned)C;
      if (!ok && o_cur != -1) s_err = 1;
      s_idx[tid] = ok ? o_cur : -1;
      s_y[tid] = ok ? y_cur : 0;
      s_wy[tid] = ok ? (double)s_cw[ok ? y_cur : 0] : 0.0;
      o_cur = o_next;
      y_cur = a.labels[(unsigned long)o_cur < (unsigned long)a.n ? o_cur : 0];
      o_next = s + 2 < ns ? order[(long)(s + 2) * batch + tid] : -1;
    }
    __syncthreads();
    // ---- (B) forward: partial dot products of every (row, class), reduced within the wavefront
    for (int i0 = 0; i0 < batch; i0 += STONK_KGB_CHUNK) {
      kgb_load_chunk<CM>(a, s_idx, i0, tid, stepkey, h);
#pragma unroll
      for (int r = 0; r < STONK_KGB_CHUNK; ++r) {
        if (i0 + r < batch) {
          constexpr int G = CM < 8 ? CM : CM == 8 ? 8 : 4;   // classes per butterfly: at CM 16 the file is full, 8 at once spill
#pragma unroll
          for (int c0 = 0; c0 < CM; c0 += G) {
            if (c0 < C) {
              double part[G];
#pragma unroll
              for (int c = 0; c < G; ++c) {   // (the rows of W past C are zeros)
                part[c] = 0.0;
#pragma unroll
                for (int k = 0; k < STONK_KGB_COLS; ++k) part[c] += (double)h[r][k] * (double)w[k][c0 + c];
              }
              const double total = kgb_reduce_classes<G>(part, lane);
              const int cls = c0 + lane / (64 / G);
              if (lane % (64 / G) == 0 && cls < C) s_zp[wv][i0 + r][cls] = total;
            }
          }
        }
      }
    }
    __syncthreads();
    // ---- (C) row i: both softmaxes, the loss term, the gradient with respect to z
    if (tid < batch) {
      const double wy = s_wy[tid];
      double wsum = 0.0;
      for (int j = 0; j < batch; ++j) wsum += s_wy[j];
      double z[CM], q[CM], dq[CM];
      double mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        z[c] = c < C ? ((s_zp[0][tid][c] + s_zp[1][tid][c]) + s_zp[2][tid][c]) + s_zp[3][tid][c] + (double)s_b[c] : -INFINITY;
        mx = fmax(mx, z[c]);
      }
      double sum = 0.0;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        q[c] = c < C ? exp(z[c] - mx) : 0.0;
        sum += q[c];
      }
      double mx2 = 0.0, qy = 0.0;
      const int y = s_y[tid];
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        q[c] = q[c] / sum;
        mx2 = fmax(mx2, q[c]);
        qy = c == y ? q[c] : qy;
      }
      double sum2 = 0.0;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        dq[c] = c < C ? exp(q[c] - mx2) : 0.0;   // (for now: the second softmax's numerator)
        sum2 += dq[c];
      }
      const double nll = -((qy - mx2) - log(sum2));
      const double scale = wsum > 0.0 ? wy / wsum : 0.0;
      double dot = 0.0;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        dq[c] = scale * (dq[c] / sum2 - (c == y ? 1.0 : 0.0));
        dot += dq[c] * q[c];
      }
      const bool live = s_idx[tid] >= 0;
#pragma unroll
      for (int c = 0; c < CM; ++c) s_gz[tid][c] = live && c < C ? q[c] * (dq[c] - dot) : 0.0;
      s_num[tid] = live ? wy * nll : 0.0;
    }
    if (batch > STONK_KGB_CHUNK) kgb_load_chunk<CM>(a, s_idx, 0, tid, stepkey, h);   // (in flight across the barrier)
    __syncthreads();
    // ---- (D) gradient of the owned columns over the rows in order, loss, AdamW
    double wsum = 0.0, num = 0.0;
    for (int j = 0; j < batch; ++j) {
      wsum += s_wy[j];
      num += s_num[j];
    }
    if (tid == 0) a.loss[(long)run * a.ld_loss + s] = (float)(num / wsum);   // (no valid row: 0 / 0, as torch; nothing is updated)
    if (wsum > 0.0) {
      double g[STONK_KGB_COLS][CM];
#pragma unroll
      for (int k = 0; k < STONK_KGB_COLS; ++k)
#pragma unroll
        for (int c = 0; c < CM; ++c) g[k][c] = 0.0;
      for (int i0 = 0; i0 < batch; i0 += STONK_KGB_CHUNK) {
        if (i0 > 0) kgb_load_chunk<CM>(a, s_idx, i0, tid, stepkey, h);
#pragma unroll
        for (int r = 0; r < STONK_KGB_CHUNK; ++r) {
          if (i0 + r < batch) {
#pragma unroll
            for (int c = 0; c < CM; ++c) {
              const double gz = s_gz[i0 + r][c];
#pragma unroll
              for (int k = 0; k < STONK_KGB_COLS; ++k) g[k][c] += gz * (double)h[r][k];
            }
          }
        }
      }
      const uint32_t t = gstep + 1u;
      const double bc1 = 1.0 - kgb_ipow(a.beta1, t), bc2 = 1.0 - kgb_ipow(a.beta2, t);
      const float step_size = (float)(a.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
#pragma unroll
      for (int k = 0; k < STONK_KGB_COLS; ++k) {
        if (tid + k * STONK_KGB_THREADS < D) {
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (c < C) kgb_adamw(w[k][c], m[k][c], v[k][c], (float)g[k][c], a, step_size, bc2_sqrt);
        }
      }
      if (tid < C) {
        double gb = 0.0;
        for (int j = 0; j < batch; ++j) gb += s_gz[j][tid];
        kgb_adamw(bias, bias_m, bias_v, (float)gb, a, step_size, bc2_sqrt);
      }
    }
    __syncthreads();   // (everyone has read this step's rows and b before either is replaced)
    if (tid < C) s_b[tid] = bias;
  }

#pragma unroll
  for (int k = 0; k < STONK_KGB_COLS; ++k) {
    const int d = tid + k * STONK_KGB_THREADS;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (d < D && c < C) {
        const long o = pbase + (long)c * D + d;
        a.W[o] = w[k][c];
        a.mW[o] = m[k][c];
        a.vW[o] = v[k][c];
      }
    }
  }
  if (tid < C) {
    a.b[run * C + tid] = bias;
    a.mb[run * C + tid] = bias_m;
    a.vb[run * C + tid] = bias_v;
  }
  __syncthreads();
  if (tid == 0 && s_err) a.errors[run] = 1;
}

// ---------------------------------------------------------------------------------------------------------- prediction
__global__ __launch_bounds__(256) void kgb_predict_kernel(const float* __restrict__ pooled, long ld_pooled, long n, int D,
                                                          const int* __restrict__ idx, long k, const float* __restrict__ W,
                                                          const float* __restrict__ b, int C, float* __restrict__ probs,
                                                          int* __restrict__ pred, int* __restrict__ errors) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= k) return;
  const int id = idx[e];
  const bool ok = (unsigned long)id < (unsigned long)n;
  const float* x = pooled + (long)(ok ? id : 0) * ld_pooled;
  float xr[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int d = j * 64 + lane;
    xr[j] = d < D ? x[d] : 0.f;
  }
  float z[STONK_KGB_MAX_CLASSES];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < STONK_KGB_MAX_CLASSES; ++c) {
    float part = 0.f;
    if (c < C) {
      const float* wr = W + (long)c * D;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int d = j * 64 + lane;
        part += d < D ? xr[j] * wr[d] : 0.f;
      }
    }
    z[c] = c < C ? wave_sum(part) + b[c] : -INFINITY;
    mx = fmaxf(mx, z[c]);
  }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < STONK_KGB_MAX_CLASSES; ++c) {
    z[c] = c < C ? expf(z[c] - mx) : 0.f;
    sum += z[c];
  }
  float best = -1.f;
  int arg = -1;
#pragma unroll
  for (int c = 0; c < STONK_KGB_MAX_CLASSES; ++c) {
    z[c] = z[c] / sum;
    if (c < C && z[c] > best) {   // (strictly greater: the lowest index keeps a tie)
      best = z[c];
      arg = c;
    }
  }
#pragma unroll
  for (int c = 0; c < STONK_KGB_MAX_CLASSES; ++c)
    if (lane == c && c < C) probs[e * C + c] = ok ? z[c] : NAN;
  if (lane == 0) {
    pred[e] = ok ? arg : -1;
    if (!ok) atomicAdd(errors, 1);
  }
}

}  // namespace

extern "C" int stonk_walk_maxpool(const int32_t* ids, int64_t ld_ids, int64_t n, int L, const float* table, int64_t ld_table,
                                  int64_t N, int D, float* pooled, int64_t ld_pooled, int32_t* errors, void* stream) {
  STONK_CHECK_ARG(ids && table && pooled && errors, STONK_EINVAL);
  STONK_CHECK_ARG(graph_dim_ok(D) && L >= 1 && ld_ids >= L && ld_table >= D && ld_pooled >= D && N >= 1 && n >= 0 &&
                      fits_i32(N, n, ld_table, ld_ids, ld_pooled),
                  STONK_ESHAPE);   // (row offsets are 64-bit products of two values below 2^31)
  STONK_CHECK_ARG(aligned_to(4, ids, errors) && aligned_to(16, table, pooled) && ld_table % 4 == 0 && ld_pooled % 4 == 0,
                  STONK_EALIGN);
  if (n == 0) return STONK_OK;
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define STONK_POOL_CASE(NV)                                                                                             \
  case NV:                                                                                                              \
    hipLaunchKernelGGL(walk_maxpool_kernel<NV>, grid, block, 0, s, ids, (long)ld_ids, (long)n, L, table, (long)ld_table, \
                       (int)N, D / 4, pooled, (long)ld_pooled, errors);                                                 \
    break;
  switch ((D + 255) / 256) { STONK_POOL_CASE(1) STONK_POOL_CASE(2) STONK_POOL_CASE(3) STONK_POOL_CASE(4) }
#undef STONK_POOL_CASE
  return stonk_launch_status();
}

extern "C" int64_t stonk_kgb_max_steps(void) { return STONK_KGB_MAX_STEPS; }

extern "C" int stonk_kgb_train_steps(const float* pooled, int64_t ld_pooled, int64_t n, int D, const int32_t* labels, int C,
                                     int R, const int32_t* order, int64_t ld_order, int batch, const int32_t* n_steps,
                                     const int32_t* first_step, int n_steps_max, const float* class_weights, float* W,
                                     float* b, float* mW, float* vW, float* mb, float* vb, float* loss, int64_t ld_loss,
                                     int32_t* errors, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, float p, uint32_t seed, void* stream) {
  STONK_CHECK_ARG(pooled && labels && order && n_steps && first_step && class_weights && W && b && mW && vW && mb && vb &&
                      loss && errors,
                  STONK_EINVAL);
  STONK_CHECK_ARG(p >= 0.f && p < 1.f && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0. &&
                      weight_decay >= 0.,
                  STONK_EINVAL);
  STONK_CHECK_ARG(C >= 2 && C <= STONK_KGB_MAX_CLASSES && batch >= 1 && batch <= STONK_KGB_MAX_BATCH &&
                      graph_dim_ok(D) && R >= 0 && R <= 65535 && n >= 1 && ld_pooled >= D && fits_i32(n, ld_pooled) &&
                      n_steps_max >= 0 && n_steps_max <= STONK_KGB_MAX_STEPS &&
                      ld_order >= (int64_t)n_steps_max * batch && ld_loss >= n_steps_max,
                  STONK_ESHAPE);
  STONK_CHECK_ARG(aligned_to(4, pooled, labels, order, n_steps, first_step, class_weights, W, b, mW, vW, mb, vb, loss, errors),
                  STONK_EALIGN);
  if (R == 0 || n_steps_max == 0) return STONK_OK;
  KgbTrain a;
  a.pooled = pooled, a.ld_pooled = (long)ld_pooled, a.n = (long)n, a.labels = labels, a.order = order;
  a.ld_order = (long)ld_order, a.n_steps = n_steps, a.first_step = first_step, a.class_weights = class_weights;
  a.W = W, a.b = b, a.mW = mW, a.vW = vW, a.mb = mb, a.vb = vb, a.loss = loss, a.ld_loss = (long)ld_loss, a.errors = errors;
  a.D = D, a.C = C, a.batch = batch, a.n_steps_max = n_steps_max;
  a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = (float)eps;
  a.beta2_f = (float)beta2, a.one_minus_beta1 = (float)(1.0 - beta1), a.one_minus_beta2 = (float)(1.0 - beta2);
  a.decay = (float)(1.0 - lr * weight_decay);
  a.drop_scale = 1.f / (1.f - p), a.seedkey = stonk_seed_mix(seed), a.thr32 = stonk_drop_thr32(p);
  const dim3 grid((unsigned)R), block(STONK_KGB_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (C <= 2) hipLaunchKernelGGL(kgb_train_kernel<2>, grid, block, 0, s, a);
  else if (C <= 4) hipLaunchKernelGGL(kgb_train_kernel<4>, grid, block, 0, s, a);
  else if (C <= 8) hipLaunchKernelGGL(kgb_train_kernel<8>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(kgb_train_kernel<16>, grid, block, 0, s, a);
  return stonk_launch_status();
}

extern "C" int stonk_kgb_predict(const float* pooled, int64_t ld_pooled, int64_t n, int D, const int32_t* idx, int64_t k,
                                 const float* W, const float* b, int C, float* probs, int32_t* pred, int32_t* errors,
                                 void* stream) {
  STONK_CHECK_ARG(pooled && idx && W && b && probs && pred && errors, STONK_EINVAL);
  STONK_CHECK_ARG(C >= 2 && C <= STONK_KGB_MAX_CLASSES && graph_dim_ok(D) && n >= 1 && ld_pooled >= D && k >= 0 &&
                      fits_i32(n, ld_pooled, k),
                  STONK_ESHAPE);
  STONK_CHECK_ARG(aligned_to(4, pooled, idx, W, b, probs, pred, errors), STONK_EALIGN);
  if (k == 0) return STONK_OK;
  hipLaunchKernelGGL(kgb_predict_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pooled,
                     (long)ld_pooled, (long)n, D, idx, (long)k, W, b, C, probs, pred, errors);
  return stonk_launch_status();
}

// Row-wise top-k + log-sum-exp + rank of the target over the label-sparse decoder logits (evaluation and masked
// prediction: stonk_row_topk_f32 / _f16). What training keeps of these rows is one loss sum (loss.hip); evaluation wants,
// per labelled row, the k best classes, the row's log-sum-exp and where the target stands - without a dense logits tensor.
//
// One workgroup of 256 threads takes one row at a time (grid-stride over the rows below the device-side count) and reads
// each logit ONCE, in the 16-byte pieces of loss.hip's sweep (four pieces per thread in flight). In that one sweep
//   * (max, sum-exp) are kept online in fp32, as the cross-entropy kernel keeps them;
//   * the rank of the target is counted: its logit is fetched first (one wave-uniform load), then every column adds
//     (v > target) + (v == target && column < target's);
//   * every lane keeps its own best k columns in registers as sorted 64-bit keys. A key is the logit's bits made
//     monotonic (high word) over 0x7fffffff - column (low word): unsigned key order IS the stated total order - larger
//     value first, lower column first among equal values - and keys are unique, so nothing below depends on the order in
//     which lanes or waves are visited. A value enters the sorted insert only when it reaches the lane's k-th value, or the
//     wave's best k-th value (any lane's k-th value is a lower bound of the row's k-th).
// The merge: every wave selects its k best keys by k rounds of a wave-wide maximum (cross-lane shuffles, the owner pops),
// the four waves' candidates meet in LDS and wave 0 selects the row's k best from them the same way. No atomics, no
// workspace; the same input gives the same bits.
#include "rowwise.h"

namespace {

__device__ __forceinline__ uint32_t f2ord(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
// (v + 0.0f: -0.0 becomes +0.0 - the two compare equal and must tie on the column)
__device__ __forceinline__ unsigned long long make_key(float v, int c) {
  return ((unsigned long long)f2ord(v + 0.0f) << 32) | (uint32_t)(0x7fffffff - c);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
    const unsigned long long y = ((unsigned long long)hi << 32) | lo;
    x = y > x ? y : x;
  }
  return x;
}
// the lane's sorted list: keys[0] the best; 0 = empty (below every real key). KC >= k slots; the k-th decides what enters.
template <int KC> struct LaneTop {
  unsigned long long keys[KC];
  float kth;   // value of the k-th key (-inf while the list holds fewer than k)
  int k;
  __device__ __forceinline__ void init(int k_) {
    k = k_;
    kth = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < KC; ++j) keys[j] = 0ull;
  }
  __device__ __forceinline__ unsigned long long kth_key() const {
    unsigned long long r = 0ull;
#pragma unroll
    for (int j = 0; j < KC; ++j) r = (j == k - 1) ? keys[j] : r;
    return r;
  }
  __device__ __forceinline__ void offer(float v, int c) {   // (called for v >= the threshold only)
    const unsigned long long key = make_key(v, c);
    if (key > kth_key()) {
      keys[KC - 1] = key;   // (replaces the weakest slot: at or below the k-th)
#pragma unroll
      for (int j = KC - 1; j > 0; --j) {
        const unsigned long long a = keys[j - 1], b = keys[j];
        const bool sw = b > a;
        keys[j - 1] = sw ? b : a;
        keys[j] = sw ? a : b;
      }
      const unsigned long long kk = kth_key();
      kth = kk ? ord2f((uint32_t)(kk >> 32)) : -__builtin_inff();
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < KC; ++j) keys[j] = keys[j + 1];
    keys[KC - 1] = 0ull;
  }
};

template <typename LT, int KC>
__global__ __launch_bounds__(256) void row_topk_kernel(const LT* __restrict__ logits, long ld, int ncols,
                                                       const int* __restrict__ targets, const int* __restrict__ count,
                                                       int cap_rows, int k, float* __restrict__ top_val,
                                                       int* __restrict__ top_idx, float* __restrict__ lse_out,
                                                       int* __restrict__ rank_out, float* __restrict__ tgt_out, int vec) {
  __shared__ float red_m[4], red_s[4];
  __shared__ int red_r[4];
  __shared__ unsigned long long cand[4][16];
  int cnt = *count;
  cnt = cnt < cap_rows ? cnt : cap_rows;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int row = blockIdx.x; row < cnt; row += gridDim.x) {
    const LT* x = logits + (long)row * ld;
    // the target's logit first: the rank count then rides in the sweep. A target outside [0, ncols) reads nothing:
    // its rank is -1 and its logit NaN (every comparison against NaN is false)
    int tgt = targets ? targets[row] : -1;
    const bool have_tgt = targets && tgt >= 0 && tgt < ncols;
    tgt = have_tgt ? tgt : -1;
    const float T = have_tgt ? (float)x[tgt] : __builtin_nanf("");
    int before = 0;   // columns ordered before the target
    float m = -3.0e38f, s = 0.f;
    LaneTop<KC> top;
    top.init(k);
    float thr = -__builtin_inff();
    const int n8 = vec ? (ncols >> 3) : 0;
    for (int i0 = 0; i0 < n8; i0 += 1024) {
      float v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 256 * u + t;
        if (i < n8) {
          load8(x + 8 * (long)i, v[u]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[u][j] = -__builtin_inff();
        }
      }
      float vm = v[0][0];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) vm = fmaxf(vm, v[u][j]);
      if (vm > m) {
        s *= __expf(m - vm);
        m = vm;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += __expf(v[u][j] - m);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 256 * u + t;
        if (i < n8) {   // (a piece past the row's end is no column)
          const int c0 = 8 * i;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float a = v[u][j];
            before += (a > T) + ((a == T) & (c0 + j < tgt));
            if (a >= thr) top.offer(a, c0 + j);
          }
        }
      }
      thr = wave_max(top.kth);   // (>= the lane's own k-th value)
    }
    for (int i = (n8 << 3) + t; i < ncols; i += 256) {   // the row's end - or all of a row that cannot be read in pieces
      const float a = (float)x[i];
      if (a > m) {
        s *= __expf(m - a);
        m = a;
      }
      s += __expf(a - m);
      before += (a > T) + ((a == T) & (i < tgt));
      if (a >= top.kth) top.offer(a, i);
    }
    // (max, sum-exp) and the rank count: across the wave, then across the four waves
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
      const float mn = fmaxf(m, m2);
      s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
      m = mn;
    }
    before = wave_sum_i(before);
    // the wave's k best keys: k rounds of a wave-wide maximum; the lane that owns the winner pops it
    for (int r = 0; r < k; ++r) {
      const unsigned long long head = top.keys[0];
      const unsigned long long best = wave_max_u64(head);
      if (head == best && best != 0ull) top.pop();
      if (lane == 0) cand[w][r] = best;
    }
    if (lane == 0) {
      red_m[w] = m;
      red_s[w] = s;
      red_r[w] = before;
    }
    __syncthreads();
    if (w == 0) {
      // 4 x k candidates, one per lane; the row's k best in order, result r kept by lane r for one store per output
      unsigned long long mine = (lane & 15) < k ? cand[lane >> 4][lane & 15] : 0ull;
      float out_v = 0.f;
      int out_i = 0;
      for (int r = 0; r < k; ++r) {
        const unsigned long long best = wave_max_u64(mine);
        if (mine == best) mine = 0ull;
        if (lane == r) {
          out_v = ord2f((uint32_t)(best >> 32));
          out_i = 0x7fffffff - (int)(uint32_t)best;
        }
      }
      if (lane < k) {
        top_val[(long)row * k + lane] = out_v;
        top_idx[(long)row * k + lane] = out_i;
      }
      if (lane == 0) {
        const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        float S = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) S += red_s[j] * __expf(red_m[j] - M);
        lse_out[row] = M + __logf(S);
        if (targets) {
          rank_out[row] = have_tgt ? red_r[0] + red_r[1] + red_r[2] + red_r[3] : -1;
          tgt_out[row] = T;
        }
      }
    }
    __syncthreads();   // (the next row overwrites cand / red_*)
  }
}

template <typename LT>
int launch_row_topk(const LT* logits, int64_t ld, int ncols, const int* targets, const int* count_dev, int cap_rows, int k,
                    float* top_val, int* top_idx, float* lse, int* rank, float* tgt_logit, void* stream) {
  STONK_CHECK_ARG(logits && count_dev && top_val && top_idx && lse && cap_rows >= 0, STONK_EINVAL);
  STONK_CHECK_ARG(!targets || (rank && tgt_logit), STONK_EINVAL);
  STONK_CHECK_ARG(ncols > 0 && k >= 1 && k <= 16 && k <= ncols, STONK_ESHAPE);
  STONK_CHECK_ARG(ld >= ncols, STONK_EINVAL);
  if (cap_rows == 0) return STONK_OK;
  // 16-byte pieces need 16-byte aligned rows; anything else is swept element by element (same results)
  constexpr int per16 = 16 / (int)sizeof(LT);
  const int vec = (uintptr_t)logits % 16 == 0 && ld % per16 == 0;
  const dim3 grid(grid_cap(cap_rows, 1, 2048)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define STONK_TOPK_LAUNCH(KC)                                                                                          \
  hipLaunchKernelGGL((row_topk_kernel<LT, KC>), grid, block, 0, st, logits, (long)ld, ncols, targets, count_dev, cap_rows, \
                     k, top_val, top_idx, lse, rank, tgt_logit, vec)
  if (k == 1) STONK_TOPK_LAUNCH(1);
  else if (k <= 4) STONK_TOPK_LAUNCH(4);
  else if (k <= 8) STONK_TOPK_LAUNCH(8);
  else if (k <= 12) STONK_TOPK_LAUNCH(12);
  else STONK_TOPK_LAUNCH(16);
#undef STONK_TOPK_LAUNCH
  return stonk_launch_status();
}

}  // namespace

extern "C" int stonk_row_topk_f32(const float* logits, int64_t ld, int ncols, const int* targets, const int* count_dev,
                                  int cap_rows, int k, float* top_val, int* top_idx, float* lse, int* rank,
                                  float* tgt_logit, void* stream) {
  return launch_row_topk<float>(logits, ld, ncols, targets, count_dev, cap_rows, k, top_val, top_idx, lse, rank, tgt_logit,
                                stream);
}

extern "C" int stonk_row_topk_f16(const void* logits_f16, int64_t ld, int ncols, const int* targets, const int* count_dev,
                                  int cap_rows, int k, float* top_val, int* top_idx, float* lse, int* rank,
                                  float* tgt_logit, void* stream) {
  return launch_row_topk<_Float16>((const _Float16*)logits_f16, ld, ncols, targets, count_dev, cap_rows, k, top_val,
                                   top_idx, lse, rank, tgt_logit, stream);
}

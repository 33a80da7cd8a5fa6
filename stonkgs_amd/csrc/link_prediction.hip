// Link-prediction score of a node2vec table: negative (non-edge) sampling, and one evaluation of a logistic model on the
// Hadamard product of two table rows. Replaces what ref:src/stonkgs/models/node2vec.py::run_link_prediction gets from
// stellargraph's EdgeSplitter (negatives) and from scikit-learn's LogisticRegression over a materialised [n, D] feature
// matrix; stonkgs_amd/link_prediction.py is the host side (edge sampling, the split, L-BFGS, the AUC).
//
// RANDOMNESS: draw(w, t, a, c) of graph_common.h, salt GRAPH_SALT_NONEDGE: w = i the sample, t = 0, a the attempt, c = 0
// for u and 1 for v.
//
// NEGATIVES (stonk_sample_non_edges). Sample i, attempts a = 0 .. 63: u = mulhi(draw(i,a,0), N), v = mulhi(draw(i,a,1), N);
// the first attempt with u != v and v not in adj(u) (binary search in u's sorted list; the CSR is symmetric, so one
// direction decides) is written to out[i] = (u, v). After STONK_NONEDGE_ATTEMPTS rejections out[i] = (-1, -1) and the failure
// counter grows by one (an int atomic add). One lane per sample; a pure function of (seed, i). Two samples may be equal:
// negatives are drawn with replacement.
//
// LOSS AND GRADIENT (stonk_linkpred_lossgrad). Example e = (u, v, y): x = emb[u] * emb[v] (elementwise), z = <x, w> + b,
// loss = softplus(z) - y z, g = sigmoid(z) - y. Nothing of size [n, D] exists: a wavefront gathers the two rows of one
// example at a time, a lane holding elements {i * 64 + lane} of a row (every load covers 256 contiguous bytes), with w and
// the D / 64 gradient accumulators in registers; the dot product goes through wave_sum. The rows of the wave's next
// example and the ids of the one after it are requested before the current example is reduced: the kernel is bound by
// gather latency and HBM, not by arithmetic.
// DETERMINISM. The grid is always STONK_LINKPRED_ROWS workgroups of four wavefronts; wavefront q of the grid takes examples
// q, q + 4 G, q + 8 G, ... in that order, so which wave adds what, and in which order, depends on (n, G) alone. A
// workgroup's waves 1 .. 3 put their sums into LDS, wave 0 adds them in the order 0, 1, 2, 3 and stores row blockIdx of
// `partials`: [sum g x (D floats), sum g, sum loss]. No float atomic anywhere: two calls on equal inputs give equal bits.
// Every row of partials is written by every launch (a workgroup without examples writes zeros).
// An example with a node id outside [0, N) adds nothing and gets the score NaN (row 0 is read in its place and discarded).
#include <math.h>

#include "graph_common.h"

#define STONK_NONEDGE_ATTEMPTS 64
// workgroups = rows of `partials`: four per CU on 256 CUs. NOT tuned: up to D 640 all 16 wavefronts of a CU are resident
// (at most 128 VGPRs); at D 768 (131 VGPRs) and above three per SIMD fit, so the grid runs in one round and a third.
#define STONK_LINKPRED_ROWS 1024
#define STONK_LINKPRED_WAVES 4

namespace {

__global__ __launch_bounds__(256) void non_edge_kernel(const long* __restrict__ rowptr, const int* __restrict__ col, int N,
                                                       long lo, long hi, uint32_t seedkey, int* __restrict__ out,
                                                       int* __restrict__ failures) {
  const long i = lo + (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hi) return;
  const uint32_t key = n2v_key(seedkey, (uint32_t)i, 0u);
  int u = -1, v = -1;
  for (int a = 0; a < STONK_NONEDGE_ATTEMPTS; ++a) {
    const int cu = (int)n2v_mulhi(n2v_draw(key, a, 0), (uint32_t)N);
    const int cv = (int)n2v_mulhi(n2v_draw(key, a, 1), (uint32_t)N);
    if (cu == cv) continue;
    const long end = rowptr[cu + 1], l = csr_lower_bound(col, rowptr[cu], end, cv);
    if (l < end && col[l] == cv) continue;
    u = cu;
    v = cv;
    break;
  }
  out[2 * i] = u;
  out[2 * i + 1] = v;
  if (u < 0) atomicAdd(failures, 1);
}

struct LinkpredSums {
  float g, loss;
};

// The loop below is straight-line code on purpose: every load is issued whatever the data says (an example past the end
// re-reads the last pair, a node id outside [0, N) reads row 0, and the result is masked afterwards). With branches around
// loads the compiler cannot count how many are in flight and falls back to waiting for all of them before every use,
// which serialises the gather.
struct LinkpredExample {
  int2 id;
  float label;
  bool ok;
};

template <bool GRAD>
__device__ __forceinline__ LinkpredExample linkpred_example(const int2* __restrict__ pairs, const float* __restrict__ y,
                                                            long i, long n, int N) {
  const long j = i < n ? i : n - 1;
  LinkpredExample ex;
  ex.id = pairs[j];
  ex.label = GRAD ? y[j] : 0.f;
  ex.ok = (unsigned)ex.id.x < (unsigned)N && (unsigned)ex.id.y < (unsigned)N;
  return ex;
}

template <int NF>
__device__ __forceinline__ void linkpred_load(const float* __restrict__ emb, long ld, const LinkpredExample& ex, int lane,
                                              float (&ru)[NF], float (&rv)[NF]) {
  const float* pu = emb + (long)(ex.ok ? ex.id.x : 0) * ld + lane;
  const float* pv = emb + (long)(ex.ok ? ex.id.y : 0) * ld + lane;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    ru[i] = pu[i * 64];
    rv[i] = pv[i * 64];
  }
}

template <int NF, bool GRAD, bool SCORES>
__device__ __forceinline__ void linkpred_reduce(const LinkpredExample& ex, const float (&ru)[NF], const float (&rv)[NF],
                                                const float (&wr)[NF], float (&acc)[NF], LinkpredSums& sums, float b, long e,
                                                int lane, float* __restrict__ scores) {
  float x[NF], dot = 0.f;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    x[i] = ru[i] * rv[i];
    dot += x[i] * wr[i];
  }
  const float z = wave_sum(dot) + b;
  if (SCORES && lane == 0) scores[e] = ex.ok ? z : NAN;
  if (GRAD) {
    const float g = ex.ok ? 1.f / (1.f + expf(-z)) - ex.label : 0.f;
    sums.g += g;
    sums.loss += ex.ok ? softplus(z) - ex.label * z : 0.f;
#pragma unroll
    for (int i = 0; i < NF; ++i) acc[i] += g * x[i];
  }
}

template <int NF, bool GRAD, bool SCORES>
__global__ __launch_bounds__(64 * STONK_LINKPRED_WAVES) void linkpred_kernel(
    const float* __restrict__ emb, long ld, int N, const int2* __restrict__ pairs, const float* __restrict__ y,
    const float* __restrict__ w, float b, long n, float* __restrict__ scores, float* __restrict__ partials) {
  constexpr int D = NF * 64;
  __shared__ float red[STONK_LINKPRED_WAVES - 1][D + 2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long stride = (long)gridDim.x * STONK_LINKPRED_WAVES;
  float wr[NF], acc[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    wr[i] = w[i * 64 + lane];
    acc[i] = 0.f;
  }
  LinkpredSums sums = {0.f, 0.f};

  // Two register sets, A and B, take turns (no copy between them: a copy would wait for the load it copies). In each half
  // step the ids two examples ahead are requested FIRST, then the rows of the next example (its ids were requested a half
  // step earlier, before the rows now in flight: loads return in order, so waiting for those ids leaves the rows alone),
  // then the current example is reduced with the next one's rows in flight.
  long e = (long)blockIdx.x * STONK_LINKPRED_WAVES + wv;
  if (e < n) {
    float au[NF], av[NF], bu[NF], bv[NF];
    LinkpredExample exA = linkpred_example<GRAD>(pairs, y, e, n, N);
    LinkpredExample exB = linkpred_example<GRAD>(pairs, y, e + stride, n, N);
    __builtin_amdgcn_sched_barrier(0);   // (the instruction scheduler may not sink the id loads below the row loads)
    linkpred_load<NF>(emb, ld, exA, lane, au, av);
    while (true) {
      const LinkpredExample exC = linkpred_example<GRAD>(pairs, y, e + 2 * stride, n, N);
      __builtin_amdgcn_sched_barrier(0);
      linkpred_load<NF>(emb, ld, exB, lane, bu, bv);
      __builtin_amdgcn_sched_barrier(0);   // (nor pull the reduction, which waits for older loads, above these)
      linkpred_reduce<NF, GRAD, SCORES>(exA, au, av, wr, acc, sums, b, e, lane, scores);
      e += stride;
      if (e >= n) break;
      const LinkpredExample exD = linkpred_example<GRAD>(pairs, y, e + 2 * stride, n, N);
      __builtin_amdgcn_sched_barrier(0);
      linkpred_load<NF>(emb, ld, exC, lane, au, av);
      __builtin_amdgcn_sched_barrier(0);
      linkpred_reduce<NF, GRAD, SCORES>(exB, bu, bv, wr, acc, sums, b, e, lane, scores);
      e += stride;
      if (e >= n) break;
      exA = exC;
      exB = exD;
    }
  }
  float sum_g = sums.g, sum_loss = sums.loss;
  if (!GRAD) return;
  // the workgroup's four waves meet once: a fixed order of addition
  if (wv > 0) {
#pragma unroll
    for (int i = 0; i < NF; ++i) red[wv - 1][i * 64 + lane] = acc[i];
    if (lane == 0) {
      red[wv - 1][D] = sum_g;
      red[wv - 1][D + 1] = sum_loss;
    }
  }
  __syncthreads();
  if (wv == 0) {
    float* row = partials + (long)blockIdx.x * (D + 2);
    for (int q = 0; q < STONK_LINKPRED_WAVES - 1; ++q) {
#pragma unroll
      for (int i = 0; i < NF; ++i) acc[i] += red[q][i * 64 + lane];
      sum_g += red[q][D];
      sum_loss += red[q][D + 1];
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) row[i * 64 + lane] = acc[i];
    if (lane == 0) {
      row[D] = sum_g;
      row[D + 1] = sum_loss;
    }
  }
}

template <int NF>
void launch_linkpred(hipStream_t stream, const float* emb, long ld, int N, const int2* pairs, const float* y, const float* w,
                     float b, long n, float* scores, float* partials) {
  const dim3 grid(STONK_LINKPRED_ROWS), block(64 * STONK_LINKPRED_WAVES);
  if (partials && scores)
    hipLaunchKernelGGL((linkpred_kernel<NF, true, true>), grid, block, 0, stream, emb, ld, N, pairs, y, w, b, n, scores, partials);
  else if (partials)
    hipLaunchKernelGGL((linkpred_kernel<NF, true, false>), grid, block, 0, stream, emb, ld, N, pairs, y, w, b, n, scores, partials);
  else
    hipLaunchKernelGGL((linkpred_kernel<NF, false, true>), grid, block, 0, stream, emb, ld, N, pairs, y, w, b, n, scores, partials);
}

}  // namespace

extern "C" int stonk_sample_non_edges(const int64_t* rowptr, const int32_t* col, int64_t N, int64_t sample_lo,
                                      int64_t sample_hi, uint32_t seed, int32_t* out, int32_t* failures, void* stream) {
  STONK_CHECK_ARG(rowptr && col && out && failures, STONK_EINVAL);
  STONK_CHECK_ARG(N >= 1 && fits_i32(N) && sample_lo >= 0 && sample_hi >= sample_lo && sample_hi <= 0x3fffffffLL,
                  STONK_ESHAPE);   // (2 i + 1 stays an int32-sized element index; i is hashed as 32 bits)
  STONK_CHECK_ARG(aligned_to(8, rowptr) && aligned_to(4, col, out, failures), STONK_EALIGN);
  if (sample_hi == sample_lo) return STONK_OK;
  const int64_t blocks = (sample_hi - sample_lo + 255) / 256;
  hipLaunchKernelGGL(non_edge_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const long*)rowptr, col,
                     (int)N, (long)sample_lo, (long)sample_hi, stonk_hash32(seed ^ GRAPH_SALT_NONEDGE), out, failures);
  return stonk_launch_status();
}

extern "C" int64_t stonk_linkpred_partial_rows(void) { return STONK_LINKPRED_ROWS; }

extern "C" int stonk_linkpred_lossgrad(const float* emb, int64_t ld, int64_t N, int D, const int32_t* pairs, const float* y,
                                       int64_t n, const float* w, float b, float* scores, float* partials, void* stream) {
  STONK_CHECK_ARG(emb && pairs && w && (scores || partials) && (!partials || y), STONK_EINVAL);
  STONK_CHECK_ARG(graph_dim_ok(D) && ld >= D && N >= 1 && fits_i32(N) && n >= 0 && n <= 0x3fffffffffffLL,
                  STONK_ESHAPE);   // (row offsets are 64-bit: id < 2^31 times ld; N * ld needs no bound of its own)
  STONK_CHECK_ARG(fits_i32(ld), STONK_ESHAPE);
  STONK_CHECK_ARG(aligned_to(8, pairs) && aligned_to(4, emb, y, w, scores, partials), STONK_EALIGN);
  if (n == 0) return STONK_OK;
  hipStream_t s = (hipStream_t)stream;
#define STONK_LP_CASE(NF)                                                                                       \
  case NF:                                                                                                      \
    launch_linkpred<NF>(s, emb, (long)ld, (int)N, (const int2*)pairs, y, w, b, (long)n, scores, partials); \
    break;
  switch (D / 64) {
    STONK_LP_CASE(1) STONK_LP_CASE(2) STONK_LP_CASE(3) STONK_LP_CASE(4) STONK_LP_CASE(5) STONK_LP_CASE(6) STONK_LP_CASE(7)
    STONK_LP_CASE(8) STONK_LP_CASE(9) STONK_LP_CASE(10) STONK_LP_CASE(11) STONK_LP_CASE(12) STONK_LP_CASE(13)
    STONK_LP_CASE(14) STONK_LP_CASE(15) STONK_LP_CASE(16)
  }
#undef STONK_LP_CASE
  return stonk_launch_status();
}

// TransE on the GPU (Bordes et al. 2013): one slice of a margin-ranking SGD pass over a triple list, the entity constraint
// (rows to unit L2 norm), and rank evaluation without a [Q, N_e] score matrix. Produces the table that
// ref:src/stonkgs/constants.py:70 names transe_embeddings_best_model.tsv (the reference's authors made theirs with PyKEEN,
// outside the package); stonkgs_amd/transe.py is the host side, tests/test_transe_cpu.py restates (a) and (c) in numpy.
//
// Tables: ent fp32 [N_e, D], rel fp32 [N_r, D], contiguous; D % 64 == 0, 64 <= D <= 1024 (graph_dim_ok). Rows are held
// as graph_common.h lays them out; norms go through wave_sum.
//
// RANDOMNESS: draw(w, t, a, c) of graph_common.h, salt GRAPH_SALT_TRANSE: w = g, the GROUP index (not the triple it
// names), t the epoch, a = j the negative; written draw(j, c) below.
//
// (a) STEP (stonk_transe_step). One wavefront per group g in [g_lo, g_hi); its triple (h, r, t) = triples[order ? order[g]
// : g]. An order entry outside [0, n), or an id outside its table, skips the group. Negative j in [0, K):
//     tail-replaced iff draw(j, 1) >> 31, else head-replaced;   e_j = mulhi(draw(j, 0), N_e);
//     e_j equal to the entity it replaces: skipped, adds nothing to the count; two equal negatives each contribute.
//   x_p = (h + r) - t;  x_j = (h + r) - e_j (tail) or (e_j + r) - t (head), in this order in fp32.
//   d(x) = sum |x_i| (norm 1) or sqrt(sum x_i^2) (norm 2: the norm itself, not its square).
//   a_j = margin + d(x_p) - d(x_j); the term is active iff a_j > 0; the group's loss is the sum of the active a_j.
//   G(x) = sign(x) with sign(0) = 0 (norm 1);  x / ||x||, and 0 where ||x|| < 1e-12 (norm 2).  A = number of active terms.
//     dh =  A G(x_p) - sum over active tail-replaced j of G(x_j)
//     dt = -A G(x_p) + sum over active head-replaced j of G(x_j)
//     dr =  A G(x_p) - sum over active j of G(x_j)
//     the replacement row gets -G(x_j) where it replaced a head, +G(x_j) where it replaced a tail.
//   Mini-batch semantics inside a group: every quantity above comes from the rows as first read - the group's G(x_j)
//   wait in LDS (each lane reads back only what it wrote: no barrier) until the last row has been read. Then each
//   destination gets ONE device-scope float atomic add of -lr * grad: one each for h, r and t (summed in registers), one
//   per active replacement. A group with A == 0 issues no add. Rows are read with plain loads; staleness with respect to
//   other groups of the same launch is accepted and ends at the launch boundary (node2vec.hip's header gives the
//   reasoning), which is why the host cuts an epoch into many launches.
//   loss_sum_cnt[0] += the loss, [1] += the number of non-skipped terms (one pair of adds per wavefront).
//
// (b) NORMALISE (stonk_rows_l2_normalize). Rows [row_lo, row_hi), row stride ld: row /= ||row||_2; a row with norm < 1e-12
// is left as it is. One wavefront per row, the row in registers between its one read and its one write.
//
// (c) RANK (stonk_transe_rank). Query (h, r, t), side 0: v = h + r, true entity t; side 1: v = t - r, true entity h.
// dist(c) = sum_i |v_i - ent[c]_i| (norm 1) or sum_i (v_i - ent[c]_i)^2 (norm 2: the SQUARED distance - monotone with the
// norm, no square root). less[q] / equal[q] = number of candidates c with dist(c) < / == dist(true). Candidates: all of
// [0, N_e), or the list cand[cand_ptr[q] .. cand_ptr[q+1]) (ids outside [0, N_e) ignored). A query with an id out of range
// gets less = equal = -1.
//   A workgroup (4 wavefronts) keeps the v of 16 queries in LDS (64 KiB at D 1024) and sweeps the candidates: a wavefront
//   holds TWO entity rows in registers (the next pair's are requested before this pair's arithmetic begins) and
//   accumulates, per lane, the 32 partial distances of the 16 queries to them, so an entity row comes from memory once per
//   16 queries and a v element from LDS once per two candidates. One halving butterfly (rank_reduce32) then sums all 32
//   across the lanes: 32 shuffles instead of 192. The true entity's distance is computed by the
//   SAME loop body in a first sweep whose candidates are the tile's true entities - one instruction sequence for every
//   distance, and a sum that does not depend on the slot a candidate sits in, so bit-equal rows give bit-equal distances
//   and equal >= 1 whenever the true entity is a candidate. Few query tiles: the candidate range is split over blockIdx.y
//   and the counts meet by integer atomics.
#include "graph_common.h"

#define RANK_QT 16
#define RANK_WAVES 4

namespace {

template <int NORM>
__device__ __forceinline__ float transe_norm(const float (&x)[16], int nf) {
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < nf) a += NORM == 1 ? fabsf(x[i]) : x[i] * x[i];
  a = wave_sum(a);
  return NORM == 1 ? a : sqrtf(a);
}

// G(x) element: sign(x) / x over its norm (0 below 1e-12)
template <int NORM>
__device__ __forceinline__ float transe_g(float x, float nrm) {
  if (NORM == 1) return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  return nrm < 1e-12f ? 0.f : x / nrm;
}

template <int NORM>
__global__ __launch_bounds__(64) void transe_step_kernel(float* ent, float* rel, int N_e, int N_r, int D,
                                                         const int* __restrict__ triples, long n,
                                                         const int* __restrict__ order, long g_lo, long g_hi, int K,
                                                         float margin, float lr, uint32_t seedkey, uint32_t epoch,
                                                         float* loss_sum_cnt) {
  extern __shared__ float smem[];
  const int lane = threadIdx.x, nf = D >> 6;
  float* gneg = smem;                      // [K][D]: the add of an ACTIVE term's replacement row; a lane's own elements
  int* nid = (int*)(smem + (long)K * D);   // [K]: the replacement entity of an active term, else -1 (wave-uniform words:
  float loss_sum = 0.f, loss_cnt = 0.f;    //      every lane writes the same word and reads back what it wrote itself)
  for (long g = g_lo + blockIdx.x; g < g_hi; g += gridDim.x) {
    const long tri = order ? (long)order[g] : g;
    if (tri < 0 || tri >= n) continue;
    const int h = triples[tri * 3], r = triples[tri * 3 + 1], t = triples[tri * 3 + 2];
    if ((unsigned)h >= (unsigned)N_e || (unsigned)t >= (unsigned)N_e || (unsigned)r >= (unsigned)N_r) continue;
    const uint32_t key = n2v_key(seedkey, (uint32_t)g, epoch);
    float* hrow = ent + (long)h * D + lane;
    float* rrow = rel + (long)r * D + lane;
    float* trow = ent + (long)t * D + lane;
    float hv[16], rv[16], tv[16], gp[16];  // the rows as first read; x_p, then G(x_p)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      hv[i] = i < nf ? hrow[i * 64] : 0.f;
      rv[i] = i < nf ? rrow[i * 64] : 0.f;
      tv[i] = i < nf ? trow[i * 64] : 0.f;
      gp[i] = (hv[i] + rv[i]) - tv[i];
    }
    const float dp = transe_norm<NORM>(gp, nf);
#pragma unroll
    for (int i = 0; i < 16; ++i) gp[i] = transe_g<NORM>(gp[i], dp);
    float st[16], sh[16];                  // sums of G(x_j) over the active tail-replaced / head-replaced terms
#pragma unroll
    for (int i = 0; i < 16; ++i) st[i] = sh[i] = 0.f;
    int A = 0;
    for (int j = 0; j < K; ++j) {
      const bool tail = n2v_draw(key, j, 1) >> 31;
      const int e = (int)n2v_mulhi(n2v_draw(key, j, 0), (uint32_t)N_e);
      nid[j] = -1;
      if (e == (tail ? t : h)) continue;
      loss_cnt += 1.f;
      const float* erow = ent + (long)e * D + lane;
      float xj[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float ev = i < nf ? erow[i * 64] : 0.f;
        xj[i] = tail ? (hv[i] + rv[i]) - ev : (ev + rv[i]) - tv[i];
      }
      const float dj = transe_norm<NORM>(xj, nf);
      const float a = margin + dp - dj;
      if (!(a > 0.f)) continue;
      loss_sum += a;
      ++A;
      nid[j] = e;
      float* dst = gneg + (long)j * D + lane;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i < nf) {
          const float gj = transe_g<NORM>(xj[i], dj);
          if (tail) st[i] += gj; else sh[i] += gj;
          dst[i * 64] = tail ? -lr * gj : lr * gj;     // -lr * (+G) where it replaced a tail, -lr * (-G) a head
        }
      }
    }
    if (!A) continue;
    // every row of the group has been read: now the adds, one per destination
    const float fa = (float)A;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < nf) atomicAdd(hrow + i * 64, -lr * (fa * gp[i] - st[i]));
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < nf) atomicAdd(rrow + i * 64, -lr * ((fa * gp[i] - st[i]) - sh[i]));
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < nf) atomicAdd(trow + i * 64, -lr * (sh[i] - fa * gp[i]));
    for (int j = 0; j < K; ++j) {
      const int e = nid[j];
      if (e < 0) continue;
      float* dst = ent + (long)e * D + lane;
      const float* src = gneg + (long)j * D + lane;
      for (int i = 0; i < nf; ++i) atomicAdd(dst + i * 64, src[i * 64]);
    }
  }
  wave_loss_flush(loss_sum_cnt, lane, loss_sum, loss_cnt);
}

__global__ __launch_bounds__(64) void rows_l2_normalize_kernel(float* table, long ld, long row_lo, long row_hi, int D) {
  const int lane = threadIdx.x, nf = D >> 6;
  for (long row = row_lo + blockIdx.x; row < row_hi; row += gridDim.x) {
    float* p = table + row * ld + lane;
    float x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = i < nf ? p[i * 64] : 0.f;
    const float nrm = transe_norm<2>(x, nf);
    if (nrm < 1e-12f) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < nf) p[i * 64] = x[i] / nrm;
  }
}

// One butterfly for the 32 partial sums a wavefront holds per lane (16 queries x 2 candidates): at every stage a lane keeps
// one half of its values and hands the other half to its partner, so 16 + 8 + 4 + 2 + 1 + 1 = 32 shuffles do what 32
// separate butterflies would do in 192. Lane L ends with the full sum of value L >> 1. The additions a value goes through
// are those of wave_sum - pairs (l, l ^ 32), then (l, l ^ 16), ... - whichever slot it sat in: the result does not depend
// on the slot, bit for bit. (kgb_reduce_classes of kg_baseline.hip is the same algorithm in fp64 over CM values; one template
// for both changed kgb_train_kernel's code: profiles/refactor_graph_sources.md, section 2.)
__device__ __forceinline__ float rank_reduce32(float (&a)[2 * RANK_QT], int lane) {
#pragma unroll
  for (int st = 0; st < 5; ++st) {
    const int o = 32 >> st, n = 16 >> st;
    const bool upper = lane & o;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i < n) {
        float lo = a[i], hi = a[i + n];
        // (opaque to the optimiser: left to itself it rewrites the select of two values as a[lane-dependent index] and
        // lowers that to a chain of 32 compares and selects - two thousand selects a call instead of 62)
        asm volatile("" : "+v"(lo), "+v"(hi));
        const float send = upper ? lo : hi, keep = upper ? hi : lo;
        a[i] = keep + __shfl_xor(send, o, 64);
      }
    }
  }
  return a[0] + __shfl_xor(a[0], 1, 64);
}

template <int NORM>
__device__ __forceinline__ void rank_acc(float& a, float y) {
  a = NORM == 1 ? a + fabsf(y) : fmaf(y, y, a);
}

__host__ __device__ inline long rank_lds_bytes(int D) {
  return ((long)RANK_QT * D + RANK_QT + RANK_QT + RANK_QT * 2) * 4;
}

template <int NORM>
__global__ __launch_bounds__(64 * RANK_WAVES) void transe_rank_kernel(const float* __restrict__ ent,
                                                                      const float* __restrict__ rel, int N_e, int N_r, int D,
                                                                      const int* __restrict__ queries, long Q, int side,
                                                                      const long* __restrict__ cand_ptr,
                                                                      const int* __restrict__ cand, long n_cand,
                                                                      int* less, int* equal) {
  extern __shared__ float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nf = D >> 6;
  float* v = smem;                                    // [QT][D]
  float* dtrue = v + (long)RANK_QT * D;               // [QT]
  int* tid = (int*)(dtrue + RANK_QT);                 // [QT]: the true entity, -1: an invalid (or absent) query
  int* cnt = tid + RANK_QT;                           // [QT][2]: less, equal of the tile's queries
  if (threadIdx.x < 2 * RANK_QT) cnt[threadIdx.x] = 0;
  const long q0 = (long)blockIdx.x * RANK_QT;
  const int ntile = Q - q0 < RANK_QT ? (int)(Q - q0) : RANK_QT;
  for (int q = wave; q < RANK_QT; q += RANK_WAVES) {
    int h = -1, r = -1, t = -1;
    if (q < ntile) {
      const int* tr = queries + (q0 + q) * 3;
      h = tr[0], r = tr[1], t = tr[2];
    }
    const bool ok = (unsigned)h < (unsigned)N_e && (unsigned)t < (unsigned)N_e && (unsigned)r < (unsigned)N_r;
    if (lane == 0) {
      tid[q] = ok ? (side ? h : t) : -1;
      dtrue[q] = 0.f;
    }
    const float* a = ent + (long)(ok ? (side ? t : h) : 0) * D + lane;
    const float* b = rel + (long)(ok ? r : 0) * D + lane;
    for (int i = 0; i < nf; ++i) v[(long)q * D + i * 64 + lane] = ok ? (side ? a[i * 64] - b[i * 64] : a[i * 64] + b[i * 64]) : 0.f;
  }
  __syncthreads();
  // sweep 0: the tile's true entities (their distances are stored); then the candidates (counted): all of a slice of
  // [0, N_e) for the whole tile, or query by query the query's own list
  const long c_lo = (long)N_e * blockIdx.y / gridDim.y, c_hi = (long)N_e * (blockIdx.y + 1) / gridDim.y;
  const int nsweep = 1 + (cand_ptr ? ntile : 1);
  int n_less = 0, n_equal = 0;                        // lanes 4 q and 4 q + 2 count for query q
  for (int s = 0; s < nsweep; ++s) {
    long base = 0, count = ntile;
    int q_lo = 0, q_hi = ntile;
    if (s > 0 && !cand_ptr) {
      base = c_lo, count = c_hi - c_lo;
    } else if (s > 0) {
      q_lo = s - 1, q_hi = s;
      long lo = cand_ptr[q0 + q_lo], hi = cand_ptr[q0 + q_lo + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > n_cand ? n_cand : hi;
      base = lo, count = hi > lo ? hi - lo : 0;
    }
    // the ids of candidate pair k, and its two rows into registers (an id outside [0, N_e): row 0 is read and not counted)
    auto pair_ids = [&](long k, int& id0, int& id1) {
      id1 = -1;
      if (s == 0) {
        id0 = tid[k];
        if (k + 1 < count) id1 = tid[k + 1];
      } else if (!cand_ptr) {
        id0 = (int)(base + k);
        if (k + 1 < count) id1 = (int)(base + k + 1);
      } else {
        id0 = cand[base + k];
        if (k + 1 < count) id1 = cand[base + k + 1];
      }
    };
    auto load_rows = [&](int id0, int id1, float (&r0)[16], float (&r1)[16]) {
      const float* p0 = ent + (long)((unsigned)id0 < (unsigned)N_e ? id0 : 0) * D + lane;
      const float* p1 = ent + (long)((unsigned)id1 < (unsigned)N_e ? id1 : 0) * D + lane;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        r0[i] = i < nf ? p0[i * 64] : 0.f;
        r1[i] = i < nf ? p1[i * 64] : 0.f;
      }
    };
    long k = 2 * wave;
    int id0 = -1, id1 = -1;
    float e0[16], e1[16];
    if (k < count) {
      pair_ids(k, id0, id1);
      load_rows(id0, id1, e0, e1);
    }
    while (k < count) {
      // the NEXT pair's rows are requested before this pair's arithmetic: one memory latency per pair, hidden behind it
      const long kn = k + 2 * RANK_WAVES;
      int nid0 = -1, nid1 = -1;
      float n0[16], n1[16];
      if (kn < count) {
        pair_ids(kn, nid0, nid1);
        load_rows(nid0, nid1, n0, n1);
      }
      const bool ok0 = (unsigned)id0 < (unsigned)N_e, ok1 = (unsigned)id1 < (unsigned)N_e;
      if (ok0 || ok1) {
        // all 16 queries of the tile against the two rows (a list sweep counts for its own query only)
        float acc[2 * RANK_QT];
#pragma unroll
        for (int j = 0; j < 2 * RANK_QT; ++j) acc[j] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (i >= nf) break;                          // (a branch, wave-uniform: an `if` around the body becomes 32 selects)
          const float* vi = v + i * 64 + lane;
#pragma unroll
          for (int q = 0; q < RANK_QT; ++q) {
            const float x = vi[(long)q * D];
            rank_acc<NORM>(acc[2 * q], x - e0[i]);
            rank_acc<NORM>(acc[2 * q + 1], x - e1[i]);
          }
        }
        const float d = rank_reduce32(acc, lane);      // this lane: query lane >> 2, the first or the second row
        const int q = lane >> 2, second = (lane >> 1) & 1;
        const bool live = !(lane & 1) && (second ? ok1 : ok0);
        if (s == 0) {
          if (live && q == k + second) dtrue[q] = d;
        } else {
          const bool mine = live && q >= q_lo && q < q_hi && tid[q] >= 0;
          const float dt = dtrue[q];
          n_less += mine && d < dt;
          n_equal += mine && d == dt;
        }
      }
      if (kn < count) {
#pragma unroll
        for (int i = 0; i < 16; ++i) e0[i] = n0[i], e1[i] = n1[i];
      }
      id0 = nid0, id1 = nid1, k = kn;
    }
    if (s == 0) __syncthreads();
  }
  if (n_less) atomicAdd(cnt + (lane >> 2) * 2, n_less);          // (LDS; eight lanes of the workgroup per query)
  if (n_equal) atomicAdd(cnt + (lane >> 2) * 2 + 1, n_equal);
  __syncthreads();
  if (threadIdx.x < ntile) {
    const int q = threadIdx.x;
    const int a = cnt[q * 2], b = cnt[q * 2 + 1];
    if (tid[q] < 0) {
      if (blockIdx.y == 0) less[q0 + q] = equal[q0 + q] = -1;
    } else {                                          // (the launcher zeroed both arrays)
      if (a) atomicAdd(less + q0 + q, a);
      if (b) atomicAdd(equal + q0 + q, b);
    }
  }
}

}  // namespace

extern "C" int stonk_transe_step(float* ent, float* rel, int64_t N_e, int64_t N_r, int D, const int32_t* triples, int64_t n,
                                 const int32_t* order, int64_t g_lo, int64_t g_hi, int negatives, int norm, float margin,
                                 float lr, uint32_t seed, uint32_t epoch, float* loss_sum_cnt, void* stream) {
  STONK_CHECK_ARG(ent && rel && triples, STONK_EINVAL);
  STONK_CHECK_ARG(norm == 1 || norm == 2, STONK_EINVAL);
  STONK_CHECK_ARG(graph_dim_ok(D) && negatives >= 1 && N_e >= 1 && N_r >= 1 && n >= 0 && fits_i32(N_e, N_r, n),
                  STONK_ESHAPE);
  STONK_CHECK_ARG(g_lo >= 0 && g_hi >= g_lo && g_hi <= n, STONK_ESHAPE);
  STONK_CHECK_ARG((long)negatives * (D + 1) * 4 <= 65536, STONK_ESHAPE);   // a group's G(x_j) wait in LDS
  STONK_CHECK_ARG(aligned_to(16, ent, rel) && aligned_to(4, triples, order, loss_sum_cnt), STONK_EALIGN);
  if (g_hi == g_lo) return STONK_OK;
  const int64_t ngroups = g_hi - g_lo;
  const int64_t blocks = ngroups < 4096 ? ngroups : 4096;   // wavefronts stride over the groups: 16 per CU
  const size_t lds = (size_t)negatives * (D + 1) * 4;
  auto kern = norm == 1 ? transe_step_kernel<1> : transe_step_kernel<2>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), lds, (hipStream_t)stream, ent, rel, (int)N_e, (int)N_r, D, triples,
                     (long)n, order, (long)g_lo, (long)g_hi, negatives, margin, lr, stonk_hash32(seed ^ GRAPH_SALT_TRANSE), epoch,
                     loss_sum_cnt);
  return stonk_launch_status();
}

extern "C" int stonk_rows_l2_normalize(float* table, int64_t ld, int64_t row_lo, int64_t row_hi, int D, void* stream) {
  STONK_CHECK_ARG(table, STONK_EINVAL);
  STONK_CHECK_ARG(graph_dim_ok(D) && ld >= D && row_lo >= 0 && row_hi >= row_lo && fits_i32(ld, row_hi), STONK_ESHAPE);
  STONK_CHECK_ARG(aligned_to(16, table), STONK_EALIGN);
  if (row_hi == row_lo) return STONK_OK;
  const int64_t rows = row_hi - row_lo;
  const int64_t blocks = rows < 8192 ? rows : 8192;
  hipLaunchKernelGGL(rows_l2_normalize_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, table, (long)ld,
                     (long)row_lo, (long)row_hi, D);
  return stonk_launch_status();
}

extern "C" int stonk_transe_rank(const float* ent, const float* rel, int64_t N_e, int64_t N_r, int D, int norm,
                                 const int32_t* queries, int64_t Q, int side, const int64_t* cand_ptr, const int32_t* cand,
                                 int64_t n_cand, int32_t* less, int32_t* equal, void* stream) {
  STONK_CHECK_ARG(ent && rel && queries && less && equal && (!cand_ptr || cand || n_cand == 0), STONK_EINVAL);
  STONK_CHECK_ARG((norm == 1 || norm == 2) && (side == 0 || side == 1), STONK_EINVAL);
  STONK_CHECK_ARG(graph_dim_ok(D) && N_e >= 1 && N_r >= 1 && Q >= 0 && fits_i32(N_e, N_r, Q) && n_cand >= 0, STONK_ESHAPE);
  STONK_CHECK_ARG(aligned_to(16, ent, rel) && aligned_to(8, cand_ptr) && aligned_to(4, queries, cand, less, equal),
                  STONK_EALIGN);
  if (Q == 0) return STONK_OK;
  const int64_t tiles = (Q + RANK_QT - 1) / RANK_QT;
  int64_t split = 1;
  if (!cand_ptr) {   // few query tiles: cut the candidates too, so that there are about 2048 workgroups
    split = (2048 + tiles - 1) / tiles;
    const int64_t most = (N_e + 63) / 64;
    split = split > most ? most : split;
    split = split > 1024 ? 1024 : (split < 1 ? 1 : split);
  }
  hipError_t e = hipMemsetAsync(less, 0, (size_t)Q * 4, (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(equal, 0, (size_t)Q * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  auto kern = norm == 1 ? transe_rank_kernel<1> : transe_rank_kernel<2>;
  if (rank_lds_bytes(D) > 65536) {   // D 1024: 16 query vectors are 64 KiB, the tile's bookkeeping comes on top
    e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rank_lds_bytes(D));
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)split), dim3(64 * RANK_WAVES), (size_t)rank_lds_bytes(D),
                     (hipStream_t)stream, ent, rel, (int)N_e, (int)N_r, D, queries, (long)Q, side, (const long*)cand_ptr, cand,
                     (long)n_cand, less, equal);
  return stonk_launch_status();
}

// node2vec on the GPU: second-order random walks over a CSR graph, and one slice of a skip-gram-with-negative-sampling
// (SGNS) pass over those walks. Replaces what ref:src/stonkgs/models/node2vec.py::run_node2vec gets from `nodevectors`
// (numba walks on CPU threads) and `gensim` (word2vec "hogwild" threads); stonkgs_amd/node2vec.py is the host side.
//
// RANDOMNESS: draw(w, t, a, c) of graph_common.h, salts GRAPH_SALT_WALKS and GRAPH_SALT_SGNS: w the walk, t the step
// (walks) or position (SGNS), a the attempt (walks) or the negative's number + 1 (SGNS), c which of an attempt's two draws.
//
// WALKS (stonk_random_walks). walk[w][0] = starts ? starts[w] : w % N. Step t >= 1 from cur = walk[w][t-1]
// (prev = walk[w][t-2]), deg = rowptr[cur+1] - rowptr[cur]:
//   * deg == 0: walk[w][t] = cur (the walk stays);
//   * first order (t == 1, or the three thresholds are equal): walk[w][t] = col[rowptr[cur] + mulhi(draw(w,t,0,0), deg)];
//   * second order: rejection sampling, at most STONK_WALK_ATTEMPTS = 32 attempts a = 0, 1, ...:
//       cand = col[rowptr[cur] + mulhi(draw(w,t,a,0), deg)];
//       class = cand == prev ? RETURN : cand in adj(prev) (binary search in prev's sorted list) ? COMMON : OTHER;
//       accept iff (draw(w,t,a,1) >> 8) < thr[class]   (24-bit integer compare: a CPU restatement is bit-exact);
//     after 32 rejections the last candidate is taken - no unbounded spin.
// A start outside [0, N) gives a row of -1 and reads nothing. One lane per walk (the kernel is latency-bound: dependent
// lookups); a wavefront keeps 32 steps of its 64 walks in an LDS tile and writes the tile out two rows per store
// instruction, each row a contiguous 128-byte segment - not one strided dword store per step.
//
// SGNS (stonk_sgns_step). One wavefront per group (walk w, position t); centre c = walk[w][t]:
//   * reduced window b = 1 + draw(w,t,0,0) % window; contexts = walk[w][u], u in [t-b, t+b] \ {t}, inside [0, L);
//   * targets = c (label 1) and K negatives (label 0) shared by all contexts of the group: negative j takes
//     slot = mulhi(draw(w,t,j+1,0), N) and n = draw(w,t,j+1,1) < alias_thr[slot] ? slot : alias_idx[slot]; n == c is skipped;
//   * mini-batch semantics: every g(u, j) = (label_j - sigmoid(<W_in[ctx_u], W_out[tgt_j]>)) * lr is computed from the
//     rows as read BEFORE the group adds anything; then W_in[ctx_u] += sum_j g(u,j) W_out[tgt_j] (one add per context
//     occurrence) and W_out[tgt_j] += sum_u g(u,j) W_in[ctx_u] (one add per target occurrence: the sum over the group's
//     contexts is formed in registers). Repeated nodes - a walk a-b-a, two equal negatives - each contribute their add.
//   * rows are held as graph_common.h lays them out; dot products go through wave_sum. The context rows wait in LDS (each
//     lane reads back only what it wrote: no barrier), the target rows are read again for the context sums - BEFORE any
//     add into W_out is issued.
//   * every update is a device-scope float atomic add (global_atomic_add_f32, executed at the memory side: no add is lost
//     with adders on all eight XCDs). Rows are read with PLAIN loads: per-XCD L2s are not coherent, so an L1-bypassing
//     (sc1) load could not promise a fresh row either; staleness ends at the launch boundary, which is why the host cuts an
//     epoch into many launches (node2vec). Plain loads keep the second read of a target row an L1 hit.
//   * a node id outside [0, N) in `walks` (the -1 rows above) is skipped: as centre the group, as context the pair.
#include "graph_common.h"

#define STONK_WALK_ATTEMPTS 32
#define STONK_WALK_CHUNK 32

namespace {

__global__ __launch_bounds__(64) void random_walk_kernel(const long* __restrict__ rowptr, const int* __restrict__ col, int N,
                                                         const int* __restrict__ starts, long walk_lo, long walk_hi, int L,
                                                         uint32_t thr_ret, uint32_t thr_com, uint32_t thr_oth,
                                                         uint32_t seedkey, int* __restrict__ out, long ld) {
  __shared__ int tile[64 * (STONK_WALK_CHUNK + 1)];   // [walk of the wave][step of the chunk], padded against bank conflicts
  const int lane = threadIdx.x;
  const long wbase = walk_lo + (long)blockIdx.x * 64;
  const long w = wbase + lane;
  int cur = -1, prev = -1;
  if (w < walk_hi) {
    cur = starts ? starts[w] : (int)(w % N);
    if ((unsigned)cur >= (unsigned)N) cur = -1;
  }
  const bool first_order = thr_ret == thr_com && thr_com == thr_oth;
  for (int t0 = 0; t0 < L; t0 += STONK_WALK_CHUNK) {
    const int nc = L - t0 < STONK_WALK_CHUNK ? L - t0 : STONK_WALK_CHUNK;
    for (int j = 0; j < nc; ++j) {
      const int t = t0 + j;
      if (t > 0 && cur >= 0) {
        const long lo = rowptr[cur];
        const uint32_t deg = (uint32_t)(rowptr[cur + 1] - lo);
        int next = cur;
        if (deg) {
          const uint32_t key = n2v_key(seedkey, (uint32_t)w, (uint32_t)t);
          if (first_order || t == 1) {
            next = col[lo + n2v_mulhi(n2v_draw(key, 0, 0), deg)];
          } else {
            const long plo = rowptr[prev], phi = rowptr[prev + 1];
            for (int a = 0; a < STONK_WALK_ATTEMPTS; ++a) {
              next = col[lo + n2v_mulhi(n2v_draw(key, a, 0), deg)];
              uint32_t thr = thr_ret;
              if (next != prev) {
                const long l = csr_lower_bound(col, plo, phi, next);
                thr = (l < phi && col[l] == next) ? thr_com : thr_oth;
              }
              if ((n2v_draw(key, a, 1) >> 8) < thr) break;
            }
          }
        }
        prev = cur;
        cur = next;
      }
      tile[lane * (STONK_WALK_CHUNK + 1) + j] = cur;
    }
    __syncthreads();
    const int c = lane & 31;
    for (int r = lane >> 5; r < 64; r += 2)   // two rows per store instruction, 128 contiguous bytes each
      if (c < nc && wbase + r < walk_hi) out[(wbase + r) * ld + t0 + c] = tile[r * (STONK_WALK_CHUNK + 1) + c];
    __syncthreads();
  }
}

// dynamic LDS of a group's wavefront, in floats / ints: context rows, the g(u, j) table, context and target ids
__host__ __device__ inline long sgns_lds_bytes(int D, int window, int K) {
  const long nctx = 2L * window;
  return (nctx * D + nctx * (K + 1) + nctx + (K + 1)) * 4;
}

__global__ __launch_bounds__(64) void sgns_kernel(const int* __restrict__ walks, long ld, int L, long walk_lo, int pos_lo,
                                                  int npos, long ngroups, float* W_in, float* W_out, int N, int D, int window,
                                                  int K, const uint32_t* __restrict__ alias_thr,
                                                  const int* __restrict__ alias_idx, float lr, uint32_t seedkey,
                                                  float* loss_sum_cnt) {
  extern __shared__ float smem[];
  const int lane = threadIdx.x, nf = D >> 6, maxctx = 2 * window, T = K + 1;
  float* ctx = smem;                          // [maxctx][D]: element i * 64 + lane of a row belongs to this lane alone
  float* gs = ctx + (long)maxctx * D;         // [maxctx][T]   (wave-uniform values: every lane writes the same word and
  int* cid = (int*)(gs + maxctx * T);         // [maxctx]       reads back what it wrote itself)
  int* tid = cid + maxctx;                    // [T]
  float loss_sum = 0.f, loss_cnt = 0.f;
  for (long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long w = walk_lo + g / npos;
    const int t = pos_lo + (int)(g % npos);
    const int* row = walks + w * ld;
    const int c = row[t];
    if ((unsigned)c >= (unsigned)N) continue;
    const uint32_t key = n2v_key(seedkey, (uint32_t)w, (uint32_t)t);
    const int b = 1 + (int)(n2v_draw(key, 0, 0) % (uint32_t)window);
    int nctx = 0;
    const int u_lo = t - b < 0 ? 0 : t - b, u_hi = t + b > L - 1 ? L - 1 : t + b;
    for (int u = u_lo; u <= u_hi; ++u) {
      if (u == t) continue;
      const int x = row[u];
      if ((unsigned)x >= (unsigned)N) continue;
      cid[nctx] = x;
      const float* src = W_in + (long)x * D + lane;
      float* dst = ctx + (long)nctx * D + lane;
      for (int i = 0; i < nf; ++i) dst[i * 64] = src[i * 64];
      ++nctx;
    }
    if (!nctx) continue;
    int ntgt = 1;
    tid[0] = c;
    for (int j = 0; j < K; ++j) {
      const uint32_t slot = n2v_mulhi(n2v_draw(key, j + 1, 0), (uint32_t)N);
      const int n = n2v_draw(key, j + 1, 1) < alias_thr[slot] ? (int)slot : alias_idx[slot];
      if (n == c || (unsigned)n >= (unsigned)N) continue;
      tid[ntgt++] = n;
    }
    // every g(u, j), from the rows as they are before this group adds anything
    for (int j = 0; j < ntgt; ++j) {
      const float* trow = W_out + (long)tid[j] * D + lane;
      float tr[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) tr[i] = i < nf ? trow[i * 64] : 0.f;
      for (int u = 0; u < nctx; ++u) {
        const float* crow = ctx + (long)u * D + lane;
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (i < nf) dot += tr[i] * crow[i * 64];
        dot = wave_sum(dot);
        const float f = 1.f / (1.f + expf(-dot));
        gs[u * T + j] = ((j == 0 ? 1.f : 0.f) - f) * lr;
        loss_sum += softplus(j == 0 ? -dot : dot);
        loss_cnt += 1.f;
      }
    }
    // W_in[ctx_u] += sum_j g(u, j) W_out[tgt_j]: W_out is read again here, before any add into it is issued
    for (int u = 0; u < nctx; ++u) {
      float acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      for (int j = 0; j < ntgt; ++j) {
        const float gg = gs[u * T + j];
        const float* trow = W_out + (long)tid[j] * D + lane;
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (i < nf) acc[i] += gg * trow[i * 64];
      }
      float* dst = W_in + (long)cid[u] * D + lane;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < nf) atomicAdd(dst + i * 64, acc[i]);
    }
    // W_out[tgt_j] += sum_u g(u, j) W_in[ctx_u], the context rows as read at the top (LDS)
    for (int j = 0; j < ntgt; ++j) {
      float acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      for (int u = 0; u < nctx; ++u) {
        const float gg = gs[u * T + j];
        const float* crow = ctx + (long)u * D + lane;
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (i < nf) acc[i] += gg * crow[i * 64];
      }
      float* dst = W_out + (long)tid[j] * D + lane;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < nf) atomicAdd(dst + i * 64, acc[i]);
    }
  }
  wave_loss_flush(loss_sum_cnt, lane, loss_sum, loss_cnt);
}

}  // namespace

extern "C" int stonk_random_walks(const int64_t* rowptr, const int32_t* col, int64_t N, const int32_t* starts,
                                  int64_t walk_lo, int64_t walk_hi, int L, uint32_t thr_return, uint32_t thr_common,
                                  uint32_t thr_other, uint32_t seed, int32_t* walks, int64_t ld, void* stream) {
  STONK_CHECK_ARG(rowptr && col && walks, STONK_EINVAL);
  STONK_CHECK_ARG(L >= 1 && walk_lo >= 0 && walk_hi >= walk_lo && ld >= L && N >= 1 && fits_i32(N), STONK_ESHAPE);
  STONK_CHECK_ARG(thr_return <= (1u << 24) && thr_common <= (1u << 24) && thr_other <= (1u << 24), STONK_ESHAPE);
  STONK_CHECK_ARG(aligned_to(8, rowptr) && aligned_to(4, col, starts, walks), STONK_EALIGN);
  if (walk_hi == walk_lo) return STONK_OK;
  const int64_t blocks = (walk_hi - walk_lo + 63) / 64;
  STONK_CHECK_ARG(fits_i32(blocks), STONK_ESHAPE);
  hipLaunchKernelGGL(random_walk_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, (const long*)rowptr, col,
                     (int)N, starts, (long)walk_lo, (long)walk_hi, L, thr_return, thr_common, thr_other,
                     stonk_hash32(seed ^ GRAPH_SALT_WALKS), walks, (long)ld);
  return stonk_launch_status();
}

extern "C" int stonk_sgns_step(const int32_t* walks, int64_t ld, int L, int64_t walk_lo, int64_t walk_hi, int pos_lo,
                               int pos_hi, float* W_in, float* W_out, int64_t N, int D, int window, int negatives,
                               const uint32_t* alias_thr, const int32_t* alias_idx, float lr, uint32_t seed,
                               float* loss_sum_cnt, void* stream) {
  STONK_CHECK_ARG(walks && W_in && W_out && (negatives <= 0 || (alias_thr && alias_idx)), STONK_EINVAL);
  STONK_CHECK_ARG(graph_dim_ok(D) && window >= 1 && negatives >= 0 && L >= 1 && ld >= L && N >= 1 && fits_i32(N),
                  STONK_ESHAPE);
  STONK_CHECK_ARG(walk_lo >= 0 && walk_hi >= walk_lo && pos_lo >= 0 && pos_hi >= pos_lo && pos_hi <= L, STONK_ESHAPE);
  STONK_CHECK_ARG((long)window <= 4096 && (long)negatives <= 4096 && sgns_lds_bytes(D, window, negatives) <= 65536,
                  STONK_ESHAPE);   // a group's context rows wait in LDS
  STONK_CHECK_ARG(aligned_to(16, W_in, W_out) && aligned_to(4, walks, alias_thr, alias_idx, loss_sum_cnt), STONK_EALIGN);
  if (walk_hi == walk_lo || pos_hi == pos_lo) return STONK_OK;
  const int npos = pos_hi - pos_lo;
  const int64_t ngroups = (walk_hi - walk_lo) * npos;
  const int64_t blocks = ngroups < 4096 ? ngroups : 4096;   // wavefronts stride over the groups: 16 per CU
  hipLaunchKernelGGL(sgns_kernel, dim3((unsigned)blocks), dim3(64), (size_t)sgns_lds_bytes(D, window, negatives),
                     (hipStream_t)stream, walks, (long)ld, L, (long)walk_lo, pos_lo, npos, (long)ngroups, W_in, W_out, (int)N,
                     D, window, negatives, alias_thr, alias_idx, lr, stonk_hash32(seed ^ GRAPH_SALT_SGNS), loss_sum_cnt);
  return stonk_launch_status();
}

// What the graph-side sources share (node2vec.hip, link_prediction.hip, kg_baseline.hip, transe.hip): the counter-based
// draws, the row-per-wavefront idiom, and the launchers' argument predicates.
//
// RANDOMNESS. Every draw is a pure function of (seed, w, t, attempt a, which c) - no state, so a result does not depend on
// launch geometry or on how a range is cut into calls. With H = stonk_hash32 (common.h) and 32-bit wrap-around arithmetic:
//     seedkey       = H(seed ^ SALT)                          one GRAPH_SALT_* per kernel, below
//     key(w, t)     = H( H(seedkey + w) ^ (t * 0x9E3779B1) )
//     draw(w,t,a,c) = H( key(w, t) + (2 a + c + 1) * 0x85EBCA77 )
// and mulhi(r, n) = (r * n) >> 32 (64-bit product) maps a draw onto [0, n). Each .hip header says what w, t, a and c are in
// its kernel; the numpy restatements in tests/test_node2vec_cpu.py are bit-exact against this.
#pragma once
#include "common.h"

constexpr uint32_t GRAPH_SALT_WALKS = 0x6E327677u, GRAPH_SALT_SGNS = 0x6E327367u, GRAPH_SALT_NONEDGE = 0x6E326E65u,
                   GRAPH_SALT_TRANSE = 0x74724573u;

__host__ __device__ inline uint32_t n2v_key(uint32_t seedkey, uint32_t w, uint32_t t) {
  return stonk_hash32(stonk_hash32(seedkey + w) ^ (t * 0x9E3779B1u));
}
__host__ __device__ inline uint32_t n2v_draw(uint32_t key, uint32_t attempt, uint32_t which) {
  return stonk_hash32(key + (2u * attempt + which + 1u) * 0x85EBCA77u);
}
__host__ __device__ inline uint32_t n2v_mulhi(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// A ROW IN REGISTERS. A lane holds elements {i * 64 + lane} of a row of D = 64 nf floats, nf <= 16, so every load and every
// atomic wave-instruction covers 256 contiguous bytes. The kernels spell the `i < nf` / `i * 64` walk out where they use
// it: as shared functions it changed every kernel's code (profiles/refactor_graph_sources.md, section 2).

// the first position of col[lo .. hi), an ascending adjacency list of a CSR graph, whose entry is not below x (x is in
// the list iff that position is inside it and holds x)
__device__ __forceinline__ long csr_lower_bound(const int* __restrict__ col, long lo, long hi, int x) {
  long l = lo, h = hi;
  while (l < h) {
    const long m = (l + h) >> 1;
    if (col[m] < x) l = m + 1; else h = m;
  }
  return l;
}

// a wavefront's loss and term count of a whole launch: one pair of adds per wavefront, not per group
__device__ __forceinline__ void wave_loss_flush(float* loss_sum_cnt, int lane, float loss_sum, float loss_cnt) {
  if (loss_sum_cnt && lane == 0 && loss_cnt > 0.f) {
    atomicAdd(loss_sum_cnt, loss_sum);
    atomicAdd(loss_sum_cnt + 1, loss_cnt);
  }
}

// launcher predicates (host)
static inline bool graph_dim_ok(int D) { return D >= 64 && D % 64 == 0 && D <= 1024; }
template <class... T>
static inline bool fits_i32(T... v) { return ((v <= 0x7fffffffLL) && ...); }
template <class... P>
static inline bool aligned_to(uintptr_t bytes, P... p) { return (((uintptr_t)p % bytes == 0) && ...); }   // (null: aligned)

// What node2vec.hip and link_prediction.hip share: the counter-based draws (node2vec.hip's header states the formula; the
// numpy restatements in tests/test_node2vec_cpu.py are bit-exact against it) and the stable softplus.
#pragma once
#include "common.h"

__host__ __device__ inline uint32_t n2v_key(uint32_t seedkey, uint32_t w, uint32_t t) {
  return stonk_hash32(stonk_hash32(seedkey + w) ^ (t * 0x9E3779B1u));
}
__host__ __device__ inline uint32_t n2v_draw(uint32_t key, uint32_t attempt, uint32_t which) {
  return stonk_hash32(key + (2u * attempt + which + 1u) * 0x85EBCA77u);
}
__host__ __device__ inline uint32_t n2v_mulhi(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// The host decisions of the graph-side launchers (node2vec.hip, link_prediction.hip, kg_baseline.hip, transe.hip), recorded
// without a GPU: the four files are compiled --cuda-host-only and linked with this program, which stands in for the HIP
// entry points they use. Every extern "C" launcher is fed seeded random argument tuples - a valid tuple with some fields
// replaced by values at and around the launchers' bounds - and one line per call is printed: the status, or what the launch
// would have been (kernel symbol, grid, workgroup, dynamic LDS bytes; memsets and function attributes before it). Two trees
// that print the same bytes refuse the same tuples with the same status and launch the same kernels in the same geometry.
// Nothing is dereferenced and nothing runs on a device: the pointers are made-up addresses.
//   tools/graph_launch_recorder.sh TREE OUT     builds the program from TREE's sources into OUT (see there)
//   OUT [tuples per launcher, default 20000]    prints the record
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "stonk_hip.h"

// ------------------------------------------------------------------------------------------------ the stand-ins
// host stub -> device symbol (the objects register their kernels from static constructors, possibly before this file's)
static std::map<const void*, std::string>& kernels() {
  static std::map<const void*, std::string> m;
  return m;
}
static const char* kernel_name(const void* f) {
  const auto it = kernels().find(f);
  return it == kernels().end() ? "?" : it->second.c_str();
}
static struct {
  dim3 grid, block;
  size_t lds;
  hipStream_t stream;
} g_config;

extern "C" void** __hipRegisterFatBinary(const void*) {
  static void* handle;
  return &handle;
}
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, void*, void*, void*, void*,
                                      int*) {
  kernels()[host] = name;
}
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
  g_config = {grid, block, lds, stream};
  return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  *grid = g_config.grid, *block = g_config.block, *lds = g_config.lds, *stream = g_config.stream;
  return hipSuccess;
}
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t) {
  printf(" launch %s grid %u %u %u block %u %u %u lds %zu", kernel_name(f), g.x, g.y, g.z, b.x, b.y, b.z, lds);
  return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) {
  printf(" memset %p %d %zu", p, v, bytes);
  return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute attr, int value) {
  printf(" attribute %s %d %d", kernel_name(f), (int)attr, value);
  return hipSuccess;
}

// ------------------------------------------------------------------------------------------------ argument values
static uint64_t g_state;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
static bool edge() { return rnd() % 100 < 12; }   // a field leaves its valid value with this chance
template <class T, size_t N>
static T pick(const T (&v)[N]) { return v[rnd() % N]; }

static const int kDims[] = {0, -64, 1, 63, 64, 65, 127, 128, 129, 192, 768, 960, 1023, 1024, 1025, 1088, 2048};
static const int64_t kCounts[] = {-1, 0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536,
                                  0x3fffffffLL, 0x40000000LL, 0x7ffffffeLL, 0x7fffffffLL, 0x80000000LL, 0x80000001LL,
                                  0x3fffffffffffLL, 0x400000000000LL};
static int dim() { return edge() ? pick(kDims) : 64 * (int)(1 + below(16)); }
static int64_t count(int64_t most = 100000) { return edge() ? pick(kCounts) : 1 + below(most); }
static int small(int64_t lo, int64_t hi) {   // [lo, hi] or one step outside it, or far outside (hi >= lo; 64-bit inside)
  static const int far[] = {-1, 0, 4096, 4097, 65535, 65536, 0x7fffffff};
  return edge() ? pick(far) : (int)(rnd() % 100 < 10 ? (rnd() & 1 ? lo - 1 : hi + 1) : lo + below(hi - lo + 1));
}
// a made-up device address: aligned to 256 bytes, or null, or off by 1, 2, 4, 8 bytes
template <class T>
static T* ptr(bool may_be_null = false) {
  static const int off[] = {1, 2, 4, 8, 12};
  uintptr_t p = 0x7f0000000000ull + (uintptr_t)below(1 << 20) * 256;
  if (edge()) p = rnd() % 3 == 0 ? 0 : p + pick(off);
  if (may_be_null && rnd() % 3 == 0) p = 0;
  return (T*)p;
}
static void* stream() { return (void*)0x5000; }

#define RECORD(name, ...)              \
  do {                                 \
    printf("%s %d:", #name, i);        \
    const int st = name(__VA_ARGS__);  \
    printf(" status %d\n", st);        \
  } while (0)

int main(int argc, char** argv) {
  const int tuples = argc > 1 ? atoi(argv[1]) : 20000;
  printf("stonk_linkpred_partial_rows %" PRId64 "\nstonk_kgb_max_steps %" PRId64 "\n", stonk_linkpred_partial_rows(),
         stonk_kgb_max_steps());
  g_state = 1;
  for (int i = 0; i < tuples; ++i) {
    const int L = small(1, 200);
    const int64_t lo = count(1000), hi = rnd() % 10 ? lo + count(1 << 20) - 1 : count();
    const uint32_t thr = rnd() % 8 ? (uint32_t)below((1 << 24) + 1) : (1u << 24) + 1;
    RECORD(stonk_random_walks, ptr<int64_t>(), ptr<int32_t>(), count(), ptr<int32_t>(true), lo, hi, L,
           rnd() % 8 ? (uint32_t)below((1 << 24) + 1) : thr, thr, rnd() % 3 ? thr : (uint32_t)below(1 << 24), (uint32_t)rnd(),
           ptr<int32_t>(), rnd() % 8 ? L + below(9) : L - 1, stream());
  }
  g_state = 2;
  for (int i = 0; i < tuples; ++i) {
    // window and negatives on both sides of the LDS limit: (2 w D + 2 w (K + 1) + 2 w + K + 1) * 4 <= 65536
    const int D = dim(), L = small(1, 200), Dv = D > 0 ? D : 64;
    const int window = rnd() % 3 ? small(1, 10) : (int)(8192 / Dv) + (int)below(5) - 2;
    const int K = rnd() % 4 ? small(0, 20) : small(0, 400);
    const int64_t lo = count(1000), hi = rnd() % 10 ? lo + count(50000) - 1 : count();
    const int plo = small(0, L > 0 ? L : 1), phi = rnd() % 10 ? (int)(plo + below(L > plo ? (int64_t)L - plo + 1 : 1)) : small(0, 300);
    const bool no_alias = K <= 0 && rnd() % 2;
    RECORD(stonk_sgns_step, ptr<int32_t>(), rnd() % 8 ? L + below(9) : L - 1, L, lo, hi, plo, phi, ptr<float>(), ptr<float>(),
           count(), D, window, K, no_alias ? nullptr : ptr<uint32_t>(), no_alias ? nullptr : ptr<int32_t>(), 0.025f,
           (uint32_t)rnd(), ptr<float>(true), stream());
  }
  g_state = 3;
  for (int i = 0; i < tuples; ++i) {
    const int64_t lo = count(1000), hi = rnd() % 10 ? lo + count(1 << 22) - 1 : count();
    RECORD(stonk_sample_non_edges, ptr<int64_t>(), ptr<int32_t>(), count(), lo, hi, (uint32_t)rnd(), ptr<int32_t>(),
           ptr<int32_t>(), stream());
  }
  g_state = 4;
  for (int i = 0; i < tuples; ++i) {
    const int D = dim();
    float* scores = ptr<float>(true);
    float* partials = ptr<float>(true);
    RECORD(stonk_linkpred_lossgrad, ptr<float>(), rnd() % 8 ? D + 4 * below(20) : (rnd() & 1 ? D - 1 : count()), count(), D,
           ptr<int32_t>(), ptr<float>(rnd() % 4 == 0), count(), ptr<float>(), 0.1f, scores, partials, stream());
  }
  g_state = 5;
  for (int i = 0; i < tuples; ++i) {
    const int D = dim(), L = small(1, 300);
    auto ld = [&](int least, int step) { return rnd() % 8 ? least + step * below(20) : (rnd() & 1 ? least - 1 : count()); };
    RECORD(stonk_walk_maxpool, ptr<int32_t>(), ld(L, 1), count(), L, ptr<float>(), ld(D, rnd() % 6 ? 4 : 1), count(), D,
           ptr<float>(), ld(D, rnd() % 6 ? 4 : 1), ptr<int32_t>(), stream());
  }
  g_state = 6;
  for (int i = 0; i < tuples; ++i) {
    const int D = dim(), C = small(2, 16), batch = small(1, 64), R = rnd() % 8 ? small(0, 8) : small(65534, 65535);
    const int steps = small(0, 256);
    auto prob = [&] { return rnd() % 12 ? (double)below(1000) / 1000 : (rnd() & 1 ? 1.0 : -0.5); };
    RECORD(stonk_kgb_train_steps, ptr<float>(), rnd() % 8 ? D + below(80) : (rnd() & 1 ? D - 1 : count()), count(), D,
           ptr<int32_t>(), C, R, ptr<int32_t>(), rnd() % 8 ? (int64_t)steps * batch + below(9) : (int64_t)steps * batch - 1, batch,
           ptr<int32_t>(), ptr<int32_t>(), steps, ptr<float>(), ptr<float>(), ptr<float>(), ptr<float>(), ptr<float>(),
           ptr<float>(), ptr<float>(), ptr<float>(), rnd() % 8 ? steps + below(9) : steps - 1, ptr<int32_t>(),
           rnd() % 12 ? 1e-3 : -1e-3, prob(), prob(), rnd() % 12 ? 1e-8 : -1.0, rnd() % 12 ? 0.01 : -0.01, (float)prob(),
           (uint32_t)rnd(), stream());
  }
  g_state = 7;
  for (int i = 0; i < tuples; ++i) {
    const int D = dim();
    RECORD(stonk_kgb_predict, ptr<float>(), rnd() % 8 ? D + below(80) : (rnd() & 1 ? D - 1 : count()), count(), D,
           ptr<int32_t>(), count(), ptr<float>(), ptr<float>(), small(2, 16), ptr<float>(), ptr<int32_t>(), ptr<int32_t>(),
           stream());
  }
  g_state = 8;
  for (int i = 0; i < tuples; ++i) {
    // negatives on both sides of the LDS limit: K (D + 1) * 4 <= 65536
    const int D = dim(), Dv = D > 0 ? D : 64;
    const int K = rnd() % 3 ? small(1, 8) : 16384 / (Dv + 1) + (int)below(5) - 2;
    const int64_t n = count(), lo = count(1000), hi = rnd() % 10 ? lo + count(50000) - 1 : count();
    RECORD(stonk_transe_step, ptr<float>(), ptr<float>(), count(), count(), D, ptr<int32_t>(), rnd() % 4 ? hi + below(100) : n,
           ptr<int32_t>(true), lo, hi, K, small(1, 2), 1.0f, 0.01f, (uint32_t)rnd(), (uint32_t)below(100), ptr<float>(true),
           stream());
  }
  g_state = 9;
  for (int i = 0; i < tuples; ++i) {
    const int D = dim();
    const int64_t lo = count(1000), hi = rnd() % 10 ? lo + count(20000) - 1 : count();
    RECORD(stonk_rows_l2_normalize, ptr<float>(), rnd() % 8 ? D + below(80) : (rnd() & 1 ? D - 1 : count()), lo, hi, D, stream());
  }
  g_state = 10;
  for (int i = 0; i < tuples; ++i) {
    const int D = rnd() % 4 ? dim() : 1024;   // D 1024: the dynamic-LDS attribute
    const bool lists = rnd() % 2;
    const int64_t n_cand = lists ? count() : 0;
    RECORD(stonk_transe_rank, ptr<float>(), ptr<float>(), count(2000000), count(), D, small(1, 2), ptr<int32_t>(), count(),
           small(0, 1), lists ? ptr<int64_t>() : nullptr, lists ? ptr<int32_t>(rnd() % 8 == 0) : nullptr, n_cand, ptr<int32_t>(),
           ptr<int32_t>(), stream());
  }
  return 0;
}

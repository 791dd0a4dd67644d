// What the host twins of the tiled passes share (scann_peaks.cpp, scann_mst.cpp, scann_silhouette.cpp; host only): the 8 x 8 block of
// distance chains of scann_knn_distsq on a pool transposed in blocks of eight rows, and how a pass is dealt to threads.  The including
// file is compiled with floating-point contraction off (#pragma clang fp contract(off) before its includes).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>

#include "scann_prim.h"

namespace scann {

typedef float v8 __attribute__((vector_size(32)));

// The pool in blocks of eight rows, each block transposed to [dim][8], so that one vector holds column j of eight rows; the rows behind
// the last repeat it (their results are never read)
inline std::vector<float> transpose8(const float* rows, int64_t n, int64_t dim) {
  std::vector<float> t((size_t)((n + 7) / 8 * 8 * dim));
  for (int64_t r = 0; r < (n + 7) / 8 * 8; ++r) {
    const float* src = rows + std::min(r, n - 1) * dim;
    float* dst = t.data() + (r / 8) * 8 * dim + r % 8;
    for (int64_t j = 0; j < dim; ++j) dst[8 * j] = src[j];
  }
  return t;
}

// dist2 of eight queries to the eight rows of a transposed block, the chain of scann_knn_distsq with the query first: 64 independent
// chains, each with its columns ascending; out[u][l] = dist2(x[u], row l of the block).  Inlined into a plain caller and into one
// compiled for AVX2 and FMA (host_fast): one instruction per eight chains there instead of a libm call per chain; fmaf is correctly
// rounded either way, so the bits are the same
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpsabi"
__attribute__((always_inline)) inline void dist2_8x8(const float* const* x, const float* block, int64_t d, v8* out) {
  v8 a[8];
  for (int u = 0; u < 8; ++u) a[u] = v8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t j = 0; j < d; ++j) {
    v8 r;
    __builtin_memcpy(&r, block + 8 * j, sizeof(r));
    for (int u = 0; u < 8; ++u) {
      const v8 t = x[u][j] - r;
      a[u] = __builtin_elementwise_fma(t, t, a[u]);
    }
  }
  for (int u = 0; u < 8; ++u) out[u] = a[u];
}
#pragma clang diagnostic pop

inline bool host_fast() { return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma"); }

// Threads of a pass over `items` queries against c.n rows of c.dim columns, dealt in groups of eight queries: as many as the caller
// asks for (threads > 0), else one for a small pass and at most 16; never more than there are groups
template <class Twin>
int64_t twin_threads(const Twin& c, int64_t items, int64_t threads = 0) {
  const double work = (double)items * (double)c.n * (double)c.dim;
  const int64_t nt = threads > 0 ? threads : work < 4e6 ? 1 : std::min<int64_t>(16, (int64_t)std::thread::hardware_concurrency());
  return std::max<int64_t>(1, std::min<int64_t>(nt, (items + 7) / 8));
}

// fn(c, k, nt) on thread k of nt takes the groups k, k + nt, ...; every query's result is its own
template <class Twin>
void twin_run(void (*fn)(const Twin&, int64_t, int64_t), const Twin& c, int64_t items, int64_t threads = 0) {
  if (items <= 0) return;
  const int64_t nt = twin_threads(c, items, threads);
  if (nt == 1) return fn(c, 0, 1);
  std::vector<std::thread> pool;
  for (int64_t k = 0; k < nt; ++k) pool.emplace_back(fn, std::cref(c), k, nt);
  for (auto& th : pool) th.join();
}

}  // namespace scann

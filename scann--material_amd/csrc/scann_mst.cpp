// The exact minimum spanning tree of a latent-space index, the host half (include/scann_hip.h): scann_index_mst around the kernels of
// scann_mst.hip -- the loop over the Boruvka rounds and the final sort of the edges --, and the twin scann_mst_host (the kernels' bits:
// the distance chain of scann_knn_distsq, the weight and the orders of scann_mst.h), threaded over the rows for the distances.  Every
// floating-point expression here is evaluated as written, each operation rounded to nearest: the file is compiled with floating-point
// contraction off.
#pragma clang fp contract(off)

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <thread>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_mst.h"
#include "scann_runtime.h"
#include "scann_twin.h"

using namespace scann;

namespace {

// ceil(log2(n)) for n >= 1
int ceil_log2(int64_t n) {
  int l = 0;
  while (((int64_t)1 << l) < n) ++l;
  return l;
}

// the first bad entry of core2 (NaN or negative), or -1
int64_t bad_core(const float* core2, int64_t n) {
  for (int64_t i = 0; core2 && i < n; ++i)
    if (!(core2[i] >= 0.f)) return i;
  return -1;
}

// the tree's edges, found in any order, into the order of the definition
void sort_edges(int64_t n_edges, const int32_t* ea, const int32_t* eb, const float* ew, int32_t* a, int32_t* b, float* w) {
  std::vector<int64_t> order((size_t)n_edges);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return mst_before(ew[x], ea[x], eb[x], ew[y], ea[y], eb[y]); });
  for (int64_t e = 0; e < n_edges; ++e) a[e] = ea[order[(size_t)e]], b[e] = eb[order[(size_t)e]], w[e] = ew[order[(size_t)e]];
}

// The twin's search.  A row keeps the first MST_KEEP rows of other components under (w, position), found by one exact pass over the pool.
// Components only merge, so an entry that has joined the row's component never leaves it again: later rounds walk the list from `head`,
// and the first entry of another component is the row's first such row in the whole pool (everything outside a full list comes behind
// its last entry).  Only a row whose full list is used up is searched again.
constexpr int MST_KEEP = 8;

struct Twin {
  const float* rows;   // [n][dim] the pool ...
  const float* rows8;  // ... and its transposed blocks
  int64_t n, dim;
  const float* core;    // [n]
  const int32_t* comp;  // [n] -1: not eligible
  const int32_t* todo;  // the rows to search
  int64_t n_todo;
  float* lw;            // [n][MST_KEEP] the lists
  int32_t* lr;
  int32_t* cnt;         // [n] entries of the list
  int32_t* head;        // [n] entries known to lie in the row's component
};

// the groups of eight rows of todo first, first + step, ...
__attribute__((always_inline)) inline void twin_groups(const Twin& c, int64_t first, int64_t step) {
  for (int64_t g0 = 8 * first; g0 < c.n_todo; g0 += 8 * step) {
    const float* x[8];
    int64_t row[8];
    int32_t lab[8];
    bool one = true;  // the eight rows carry one label
    for (int u = 0; u < 8; ++u) {
      row[u] = c.todo[std::min(g0 + u, c.n_todo - 1)];
      x[u] = c.rows + row[u] * c.dim;
      lab[u] = c.comp[row[u]];
      one = one && lab[u] == lab[0];
    }
    const int m_u = (int)std::min<int64_t>(8, c.n_todo - g0);
    for (int u = 0; u < m_u; ++u) c.cnt[row[u]] = 0, c.head[row[u]] = 0;
    for (int64_t j0 = 0; j0 < c.n; j0 += 8) {
      const int m = (int)std::min<int64_t>(8, c.n - j0);
      if (one) {  // the skip rule of the kernel, on this scale
        bool same = true;
        for (int l = 0; l < m; ++l) same = same && c.comp[j0 + l] == lab[0];
        if (same) continue;
      }
      v8 d[8];
      dist2_8x8(x, c.rows8 + j0 * c.dim, c.dim, d);
      for (int u = 0; u < m_u; ++u) {
        const int64_t i = row[u];
        float* lw = c.lw + i * MST_KEEP;
        int32_t* lr = c.lr + i * MST_KEEP;
        for (int l = 0; l < m; ++l) {
          const int64_t j = j0 + l;
          if (c.comp[j] < 0 || c.comp[j] == lab[u]) continue;
          const float w = mst_weight(d[u][l], c.core[i], c.core[j]);
          int k = c.cnt[i];
          if (k == MST_KEEP) {
            if (!mst_row_before(w, (int32_t)j, lw[MST_KEEP - 1], lr[MST_KEEP - 1])) continue;  // behind the list's last entry
            --k;
          } else {
            c.cnt[i] = k + 1;
          }
          for (; k > 0 && mst_row_before(w, (int32_t)j, lw[k - 1], lr[k - 1]); --k) lw[k] = lw[k - 1], lr[k] = lr[k - 1];
          lw[k] = w, lr[k] = (int32_t)j;
        }
      }
    }
  }
}

// the same loops where the host has AVX2 and a fused multiply-add instruction: one instruction per eight chains instead of a libm call
// per chain; fmaf is correctly rounded either way, so the bits are the same
void search_plain(const Twin& c, int64_t first, int64_t step) { twin_groups(c, first, step); }
__attribute__((target("avx2,fma"))) void search_fma(const Twin& c, int64_t first, int64_t step) { twin_groups(c, first, step); }

// the record of the calling thread's last scann_index_mst, for scann_mst_last_rounds
struct RoundLog {
  int32_t n = 0;
  int32_t components[40];
  double seconds[40];
  int64_t skipped[40];
  int64_t tiles = 0;
};
thread_local RoundLog g_log;

}  // namespace

extern "C" {

int scann_mst_host(const float* rows, int64_t n, int64_t dim, const float* core2, int64_t* n_edges, int32_t* a, int32_t* b, float* w) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || !n_edges || (n > 0 && !rows) || (n > 1 && (!a || !b || !w)) || bad_core(core2, n) >= 0)
    return SCANN_ERR_INVALID;
  *n_edges = 0;
  if (n == 0) return SCANN_OK;
  std::vector<int32_t> comp((size_t)n);
  int64_t n_comp = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bool ok = finite_row(rows + i * dim, dim);
    comp[(size_t)i] = ok ? (int32_t)i : -1;
    n_comp += ok;
  }
  if (n_comp <= 1) return SCANN_OK;
  const int max_rounds = ceil_log2(n_comp) + 1;
  const std::vector<float> rows8 = transpose8(rows, n, dim);
  const std::vector<float> zeros(core2 ? 0 : (size_t)n, 0.f);
  std::vector<float> lw((size_t)n * MST_KEEP), bw((size_t)n), ew((size_t)n);
  std::vector<int32_t> lr((size_t)n * MST_KEEP), cnt((size_t)n, MST_KEEP), head((size_t)n, MST_KEEP), todo, blo((size_t)n), bhi((size_t)n),
      up((size_t)n), ea((size_t)n), eb((size_t)n);
  todo.reserve((size_t)n);
  int64_t m = 0;
  Twin c{rows, rows8.data(), n, dim, core2 ? core2 : zeros.data(), comp.data(), nullptr, 0, lw.data(), lr.data(), cnt.data(), head.data()};
  for (int round = 0; n_comp > 1; ++round) {
    if (round >= max_rounds) return SCANN_ERR_UNSUPPORTED;  // cannot happen: every round at least halves the components
    // every row's first row of another component
    todo.clear();
    for (int64_t i = 0; i < n; ++i) {
      if (comp[(size_t)i] < 0) continue;
      int32_t& hd = head[(size_t)i];
      while (hd < cnt[(size_t)i] && comp[(size_t)lr[(size_t)(i * MST_KEEP + hd)]] == comp[(size_t)i]) ++hd;
      if (hd == cnt[(size_t)i] && cnt[(size_t)i] == MST_KEEP) todo.push_back((int32_t)i);
    }
    c.todo = todo.data(), c.n_todo = (int64_t)todo.size();
    twin_run(host_fast() ? search_fma : search_plain, c, c.n_todo);
    // every component's first edge under (w, min, max); labels are positions of rows
    std::fill(blo.begin(), blo.end(), -1);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t l = comp[(size_t)i];
      if (l < 0 || head[(size_t)i] >= cnt[(size_t)i]) continue;
      const size_t e = (size_t)(i * MST_KEEP + head[(size_t)i]);
      const int32_t lo = std::min((int32_t)i, lr[e]), hi = std::max((int32_t)i, lr[e]);
      if (blo[(size_t)l] < 0 || mst_before(lw[e], lo, hi, bw[(size_t)l], blo[(size_t)l], bhi[(size_t)l])) bw[(size_t)l] = lw[e], blo[(size_t)l] = lo, bhi[(size_t)l] = hi;
    }
    for (int64_t l = 0; l < n; ++l) {
      up[(size_t)l] = (int32_t)l;
      if (comp[(size_t)l] != l || blo[(size_t)l] < 0) continue;
      const int32_t lo = blo[(size_t)l], hi = bhi[(size_t)l], l2 = comp[(size_t)lo] == l ? comp[(size_t)hi] : comp[(size_t)lo];
      const bool same = blo[(size_t)l2] == lo && bhi[(size_t)l2] == hi;  // the component across picked this edge too
      if (same && l > l2) {
        up[(size_t)l] = l2;  // the smaller label is the root and appends the edge
        continue;
      }
      if (!same) up[(size_t)l] = l2;
      ea[(size_t)m] = lo, eb[(size_t)m] = hi, ew[(size_t)m] = bw[(size_t)l];
      ++m;
    }
    int64_t left = 0;
    for (int64_t i = 0; i < n; ++i) {
      int32_t l = comp[(size_t)i];
      if (l < 0) continue;
      for (int64_t guard = 0; up[(size_t)l] != l && guard < n; ++guard) l = up[(size_t)l];
      comp[(size_t)i] = l;
    }
    for (int64_t i = 0; i < n; ++i) left += comp[(size_t)i] == i;
    if (left >= n_comp) return SCANN_ERR_UNSUPPORTED;  // cannot happen
    n_comp = left;
  }
  sort_edges(m, ea.data(), eb.data(), ew.data(), a, b, w);
  *n_edges = m;
  return SCANN_OK;
}

int scann_index_mst(scann_handle_t* h, scann_index_t* pool, const float* core2, int64_t* n_edges, int32_t* a, int32_t* b, float* w, int32_t* rounds) {
  const std::string who = "scann_index_mst: ";
  if (const int r = check_pool(h, pool, "scann_index_mst")) return r;
  if (!n_edges) return fail(h, SCANN_ERR_INVALID, who + "n_edges is null");
  const int64_t N = pool->n;
  if (N > SCANN_MST_MAX_ROWS)
    return fail(h, SCANN_ERR_UNSUPPORTED, who + "the pool has " + std::to_string(N) + " rows, above SCANN_MST_MAX_ROWS = " + std::to_string(SCANN_MST_MAX_ROWS));
  if (N > 1 && !a) return fail(h, SCANN_ERR_INVALID, who + "a is null");
  if (N > 1 && !b) return fail(h, SCANN_ERR_INVALID, who + "b is null");
  if (N > 1 && !w) return fail(h, SCANN_ERR_INVALID, who + "w is null");
  if (const int64_t bad = bad_core(core2, N); bad >= 0)
    return fail(h, SCANN_ERR_INVALID, who + "core2[" + std::to_string(bad) + "] is " + (core2[bad] != core2[bad] ? "NaN" : "negative"));
  g_log.n = 0;
  if (N == 0) {
    *n_edges = 0;
    if (rounds) *rounds = 0;
    return SCANN_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  MstArgs t{};
  t.n_total = (int32_t)N; t.chunk_rows = pool->chunk_rows; t.stride = pool->stride;
  peaks_geometry(N, N, &t.rows_per_range, &t.n_range);
  // one workspace for the call
  MstStep c{};
  c.n = (int32_t)N;
  float *d_core, *out_w;
  int32_t* out_p;
  CallWs ws;
  ws.take(c.comp, (size_t)N); ws.take(d_core, (size_t)N); ws.take(out_w, (size_t)N); ws.take(out_p, (size_t)N); ws.take(c.hi, (size_t)N);
  ws.take(c.ptr[0], (size_t)N); ws.take(c.ptr[1], (size_t)N); ws.take(c.edge_a, (size_t)N); ws.take(c.edge_b, (size_t)N); ws.take(c.edge_w, (size_t)N);
  ws.take(c.key, (size_t)N); ws.take(t.part_w, (size_t)N * t.n_range); ws.take(t.part_p, (size_t)N * t.n_range); ws.take(t.rows, (size_t)n_chunk);
  ws.take(c.counters, 64);  // [0] edges, [1] components, [2] tiles skipped
  HIPCHK(h, ws.alloc());
  int32_t* const d_comp = c.comp;
  c.best_w = out_w; c.best_p = out_p;
  t.comp = d_comp; t.core2 = d_core;
  t.skipped = reinterpret_cast<unsigned int*>(c.counters + 2);
  int32_t counters[3] = {0, 0, 0};
  hipError_t e = ws.upload_rows(pool, n_chunk, t.rows, nullptr, s);
  if (e == hipSuccess) e = hipMemsetAsync(c.counters, 0, 256, s);
  if (e == hipSuccess) e = core2 ? hipMemcpyAsync(d_core, core2, (size_t)N * 4, hipMemcpyHostToDevice, s) : hipMemsetAsync(d_core, 0, (size_t)N * 4, s);
  if (e == hipSuccess) e = launch_mst_eligible(t, d_comp, c.counters, s);
  if (e == hipSuccess) e = hipMemcpyAsync(counters, c.counters, 12, hipMemcpyDeviceToHost, s);
  hipError_t e_sync = hipStreamSynchronize(s);
  int64_t n_comp = counters[1];
  const int max_rounds = ceil_log2(std::max<int64_t>(n_comp, 1)) + 1;
  int n_round = 0;
  const char* internal = nullptr;
  g_log.tiles = (int64_t)((N + TILE_TQ - 1) / TILE_TQ) * ((N + TILE_TR - 1) / TILE_TR);
  while (e == hipSuccess && e_sync == hipSuccess && n_comp > 1) {  // at most max_rounds passes: every exit below is reached without a wait in a kernel
    if (n_round >= max_rounds) {
      internal = "more rounds than ceil(log2 n) + 1 would be needed";
      break;
    }
    const auto t0 = std::chrono::steady_clock::now();
    e = launch_mst_tile(t, s);
    if (e == hipSuccess) e = launch_knn_merge(t.part_w, t.part_p, (int)N, t.n_range, 1, out_w, out_p, s);  // the first under (w, position)
    if (e == hipSuccess) e = launch_mst_step(c, ceil_log2(n_comp), s);
    if (e == hipSuccess) e = hipMemcpyAsync(counters, c.counters, 12, hipMemcpyDeviceToHost, s);  // the round's one read-back
    e_sync = hipStreamSynchronize(s);
    if (e != hipSuccess || e_sync != hipSuccess) break;
    g_log.components[n_round] = (int32_t)n_comp;
    g_log.seconds[n_round] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    g_log.skipped[n_round] = (int64_t)(uint32_t)counters[2] - (n_round ? std::accumulate(g_log.skipped, g_log.skipped + n_round, (int64_t)0) : 0);
    g_log.n = ++n_round;
    if (counters[1] >= n_comp) {
      internal = "a round did not reduce the number of components";
      break;
    }
    n_comp = counters[1];
  }
  const int64_t m = counters[0];
  std::vector<int32_t> ea((size_t)std::max<int64_t>(m, 0)), eb(ea.size());
  std::vector<float> ew(ea.size());
  const bool good = e == hipSuccess && e_sync == hipSuccess && !internal && m >= 0 && m <= N - 1;
  if (good && m > 0) {
    e = hipMemcpyAsync(ea.data(), c.edge_a, (size_t)m * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(eb.data(), c.edge_b, (size_t)m * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ew.data(), c.edge_w, (size_t)m * 4, hipMemcpyDeviceToHost, s);
    e_sync = hipStreamSynchronize(s);
  }
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  if (internal) return fail(h, SCANN_ERR_UNSUPPORTED, who + "internal error: " + internal);
  if (!good) return fail(h, SCANN_ERR_UNSUPPORTED, who + "internal error: " + std::to_string(m) + " edges for " + std::to_string(N) + " rows");
  sort_edges(m, ea.data(), eb.data(), ew.data(), a, b, w);
  *n_edges = m;
  if (rounds) *rounds = n_round;
  return SCANN_OK;
}

int scann_mst_last_rounds(int32_t cap, int32_t* components, double* seconds, int64_t* skipped, int64_t* tiles) {
  const int32_t n = std::min(g_log.n, std::max(cap, 0));
  for (int32_t r = 0; r < n; ++r) {
    if (components) components[r] = g_log.components[r];
    if (seconds) seconds[r] = g_log.seconds[r];
    if (skipped) skipped[r] = g_log.skipped[r];
  }
  if (tiles) *tiles = g_log.tiles;
  return g_log.n;
}

}  // extern "C"

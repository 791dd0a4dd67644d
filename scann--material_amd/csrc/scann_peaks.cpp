// Density-peak clustering and kernel density of a latent-space index, the host half (include/scann_hip.h): scann_index_density,
// scann_index_peaks and scann_index_density_batch around the kernels of scann_peaks.hip, and the twins scann_density_host and
// scann_peaks_host (the kernels' bits: the distance chain of scann_knn_distsq, the term of scann_peaks.h, integer sums), threaded over the
// queries.  Every floating-point expression here is evaluated as written, each operation rounded to nearest: the file is compiled with
// floating-point contraction off.
#pragma clang fp contract(off)

#include <cmath>
#include <thread>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_peaks.h"
#include "scann_runtime.h"
#include "scann_twin.h"

using namespace scann;

namespace {

struct Twin {
  const float* rows;   // [n][dim] the pool ...
  const float* rows8;  // ... and its transposed blocks
  int64_t n, dim;
  const float* q;      // [nq][dim] the queries
  int64_t nq;
  const int32_t* skip;  // [nq] or null
  bool self;            // the queries are the pool's rows: position i is left out of query i's sum
  float gamma;
  int64_t* sums;
  int32_t* parent;
  float* delta2;
};

// the groups of eight queries first, first + step, ...: their sums (pass 0) or, from the finished sums of the self-join, their parents
// (pass 1: the rows of a block come in position order, so among equal distances the earlier row stays)
template <int PASS>
__attribute__((always_inline)) inline void twin_groups(const Twin& c, int64_t first, int64_t step) {
  for (int64_t i0 = 8 * first; i0 < c.nq; i0 += 8 * step) {
    const float* x[8];
    bool ok[8];
    int64_t leave[8], s[8];
    for (int u = 0; u < 8; ++u) {
      const int64_t i = std::min(i0 + u, c.nq - 1);
      x[u] = c.q + i * c.dim;
      ok[u] = i0 + u < c.nq && (PASS == 0 ? finite_row(x[u], c.dim) : c.sums[i] >= 0);
      leave[u] = c.self ? i : c.skip ? c.skip[i] : -1;
      s[u] = 0;
      if (PASS == 1 && i0 + u < c.nq) c.parent[i] = -1, c.delta2[i] = __builtin_inff();
    }
    for (int64_t j0 = 0; j0 < c.n; j0 += 8) {
      v8 d[8];
      dist2_8x8(x, c.rows8 + j0 * c.dim, c.dim, d);
      const int m = (int)std::min<int64_t>(8, c.n - j0);
      for (int u = 0; u < 8; ++u) {
        if (!ok[u]) continue;
        const int64_t i = i0 + u;
        for (int l = 0; l < m; ++l) {
          const int64_t j = j0 + l;
          const float dl = d[u][l];
          if (PASS == 0) {
            if (j != leave[u]) s[u] += peaks_term(dl, c.gamma);
          } else if (dl == dl && peaks_above(c.sums[j], (int32_t)j, c.sums[i], (int32_t)i) && (c.parent[i] < 0 || dl < c.delta2[i])) {
            c.parent[i] = (int32_t)j, c.delta2[i] = dl;  // a NaN distance never qualifies
          }
        }
      }
    }
    for (int u = 0; PASS == 0 && u < 8 && i0 + u < c.nq; ++u) c.sums[i0 + u] = ok[u] ? s[u] : -1;
  }
}

// the same loops where the host has AVX2 and a fused multiply-add instruction: one instruction per eight chains instead of a libm call
// per chain; fmaf is correctly rounded either way, so the bits are the same
void density_plain(const Twin& c, int64_t first, int64_t step) { twin_groups<0>(c, first, step); }
__attribute__((target("avx2,fma"))) void density_fma(const Twin& c, int64_t first, int64_t step) { twin_groups<0>(c, first, step); }
void parent_plain(const Twin& c, int64_t first, int64_t step) { twin_groups<1>(c, first, step); }
__attribute__((target("avx2,fma"))) void parent_fma(const Twin& c, int64_t first, int64_t step) { twin_groups<1>(c, first, step); }

// Enqueued on s: the sums of nq queries -- dq, device rows of the pool's stride, or null: the pool's own rows -- against the pool, left in
// d_sums [nq]; tab: the device copy of the pool's chunk table
hipError_t enqueue_density(const scann_index* pool, const float* const* tab, const float* dq, const int32_t* dskip, int64_t nq, float gamma,
                           unsigned long long* d_sums, hipStream_t s) {
  PeaksArgs a{};
  a.rows = tab;
  a.n_total = (int32_t)pool->n; a.chunk_rows = pool->chunk_rows; a.stride = pool->stride;
  a.q = dq; a.skip = dskip; a.nq = (int32_t)nq; a.gamma = gamma; a.sums = d_sums;
  peaks_geometry(pool->n, nq, &a.rows_per_range, &a.n_range);
  hipError_t e = hipMemsetAsync(d_sums, 0, (size_t)nq * 8, s);
  if (e == hipSuccess) e = launch_peaks_density(a, s);
  if (e == hipSuccess) e = launch_peaks_finish(a, s);
  return e;
}

// nq queries of the pool's width at q -- host rows (kind = hipMemcpyHostToDevice) or device rows -- staged padded to the stride, their
// sums against the pool downloaded to sums; one wait
int density_staged(scann_handle* h, scann_index* pool, const float* q, hipMemcpyKind kind, const int32_t* skip, int64_t nq, float gamma, hipStream_t s,
                   int64_t* sums) {
  const int n_chunk = (int)((pool->n + pool->chunk_rows - 1) / pool->chunk_rows);
  CallWs ws;
  RowStage st;
  int32_t* d_skip;
  unsigned long long* d_sums;
  const float* const* d_rows;
  st.take(ws, nq, pool->dim, pool->dim, pool->stride, kind);
  ws.take(d_skip, (size_t)nq); ws.take(d_sums, (size_t)nq); ws.take(d_rows, (size_t)std::max(n_chunk, 1));
  HIPCHK(h, ws.alloc());
  hipError_t e = st.stage_rows(q, s);
  if (e == hipSuccess && skip) e = hipMemcpyAsync(d_skip, skip, (size_t)nq * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, n_chunk, d_rows, nullptr, s);
  if (e == hipSuccess) e = enqueue_density(pool, d_rows, st.rows(q), skip ? d_skip : nullptr, nq, gamma, d_sums, s);
  if (e == hipSuccess) e = hipMemcpyAsync(sums, d_sums, (size_t)nq * 8, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  return SCANN_OK;
}

}  // namespace

extern "C" {

int scann_density_host(const float* rows, int64_t n, int64_t dim, const float* q, int64_t nq, const int32_t* skip_pos, float gamma, int64_t* sums) {
  if (n < 0 || n > (int64_t)0x7fffffff || nq < 0 || nq > (int64_t)0x7fffffff || dim < 1 || bad_gamma(gamma) || (n > 0 && !rows) ||
      (nq > 0 && (!q || !sums)))
    return SCANN_ERR_INVALID;
  if (nq == 0) return SCANN_OK;
  if (n == 0) {
    for (int64_t i = 0; i < nq; ++i) sums[i] = finite_row(q + i * dim, dim) ? 0 : -1;
    return SCANN_OK;
  }
  const std::vector<float> rows8 = transpose8(rows, n, dim);
  Twin c{rows, rows8.data(), n, dim, q, nq, skip_pos, false, gamma, sums, nullptr, nullptr};
  twin_run(host_fast() ? density_fma : density_plain, c, nq);
  return SCANN_OK;
}

int scann_peaks_host(const float* rows, int64_t n, int64_t dim, float gamma, int64_t* sums, int32_t* parent, float* delta2) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || bad_gamma(gamma) || (n > 0 && (!rows || !sums || !parent || !delta2))) return SCANN_ERR_INVALID;
  if (n == 0) return SCANN_OK;
  const std::vector<float> rows8 = transpose8(rows, n, dim);
  Twin c{rows, rows8.data(), n, dim, rows, n, nullptr, true, gamma, sums, parent, delta2};
  twin_run(host_fast() ? density_fma : density_plain, c, n);
  twin_run(host_fast() ? parent_fma : parent_plain, c, n);
  return SCANN_OK;
}

int scann_index_density(scann_handle_t* h, scann_index_t* pool, const float* q, int64_t nq, const int32_t* skip_pos, float gamma, int64_t* sums) {
  const std::string w = "scann_index_density: ";
  if (const int r = check_pool(h, pool, "scann_index_density")) return r;
  if (nq < 0 || nq > (int64_t)0x7fffffff - 1024) return fail(h, SCANN_ERR_INVALID, w + "nq " + std::to_string(nq) + " outside 0 .. 2^31 - 1025");
  if (nq > 0 && !q) return fail(h, SCANN_ERR_INVALID, w + "q is null");
  if (nq > 0 && !sums) return fail(h, SCANN_ERR_INVALID, w + "sums is null");
  if (bad_gamma(gamma)) return fail(h, SCANN_ERR_INVALID, w + "gamma must be finite and > 0");
  if (const int r = check_pool_rows(h, pool, "scann_index_density", (int64_t)0x7fffffff - 1024)) return r;
  if (nq == 0) return SCANN_OK;
  if (pool->n == 0) {
    for (int64_t i = 0; i < nq; ++i) sums[i] = finite_row(q + i * pool->dim, pool->dim) ? 0 : -1;
    return SCANN_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  return density_staged(h, pool, q, hipMemcpyHostToDevice, skip_pos, nq, gamma, h->streams[0], sums);
}

int scann_index_peaks(scann_handle_t* h, scann_index_t* pool, float gamma, int64_t* sums, int32_t* parent, float* delta2) {
  const std::string w = "scann_index_peaks: ";
  if (const int r = check_pool(h, pool, "scann_index_peaks")) return r;
  if (bad_gamma(gamma)) return fail(h, SCANN_ERR_INVALID, w + "gamma must be finite and > 0");
  const int64_t N = pool->n;
  if (const int r = check_pool_rows(h, pool, "scann_index_peaks", (int64_t)0x7fffffff - 1024)) return r;
  if (N > 0 && !sums) return fail(h, SCANN_ERR_INVALID, w + "sums is null");
  if (N > 0 && !parent) return fail(h, SCANN_ERR_INVALID, w + "parent is null");
  if (N > 0 && !delta2) return fail(h, SCANN_ERR_INVALID, w + "delta2 is null");
  if (N == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  PeaksArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = pool->stride;
  a.nq = (int32_t)N; a.gamma = gamma;
  peaks_geometry(N, N, &a.rows_per_range, &a.n_range);
  // one workspace for the call: the sums, the ranges' partial results, the merged results, the chunk table
  CallWs ws;
  float* out_d;
  int32_t* out_p;
  ws.take(a.sums, (size_t)N); ws.take(a.part_d, (size_t)N * a.n_range); ws.take(a.part_p, (size_t)N * a.n_range); ws.take(out_d, (size_t)N);
  ws.take(out_p, (size_t)N); ws.take(a.rows, (size_t)n_chunk);
  HIPCHK(h, ws.alloc());
  std::vector<int64_t> sums_h((size_t)N);  // (the outputs change only if the call succeeds)
  std::vector<int32_t> parent_h((size_t)N);
  std::vector<float> delta_h((size_t)N);
  hipError_t e = ws.upload_rows(pool, n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess) e = enqueue_density(pool, a.rows, nullptr, nullptr, N, gamma, a.sums, s);
  if (e == hipSuccess) e = launch_peaks_parent(a, s);
  if (e == hipSuccess) e = launch_knn_merge(a.part_d, a.part_p, (int)N, a.n_range, 1, out_d, out_p, s);  // the first under (dist2, position)
  if (e == hipSuccess) e = hipMemcpyAsync(sums_h.data(), a.sums, (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(parent_h.data(), out_p, (size_t)N * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(delta_h.data(), out_d, (size_t)N * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  std::copy(sums_h.begin(), sums_h.end(), sums);
  std::copy(parent_h.begin(), parent_h.end(), parent);
  std::copy(delta_h.begin(), delta_h.end(), delta2);
  return SCANN_OK;
}

int scann_index_density_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, float gamma, float* y, float* ga, int64_t* sums) {
  const std::string w = "scann_index_density_batch: ";
  if (!h || !idx || !db) return fail(h, SCANN_ERR_INVALID, w + "null argument");
  if (idx->h != h) return fail(h, SCANN_ERR_INVALID, w + "the index belongs to another handle");
  if (const int r = check_level(h, idx, level, "scann_index_density_batch")) return r;
  if (bad_gamma(gamma)) return fail(h, SCANN_ERR_INVALID, w + "gamma must be finite and > 0");
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int64_t nq = atom ? db->n_atom : db->n_struct;
  if (nq <= 0) return fail(h, SCANN_ERR_INVALID, w + "an empty batch");
  if (!sums) return fail(h, SCANN_ERR_INVALID, w + "sums is null");
  if (idx->n > (int64_t)0x7fffffff - 1024) return fail(h, SCANN_ERR_UNSUPPORTED, w + "the index has too many rows");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, w + "weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  // the level's rows are the queries where the forward left them
  return density_staged(h, idx, atom ? db->out_z : db->out_bf, hipMemcpyDeviceToDevice, nullptr, nq, gamma, h->streams[db->last_slot], sums);
}

}  // extern "C"

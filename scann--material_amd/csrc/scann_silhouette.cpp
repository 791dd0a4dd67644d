// Silhouette of a labelled latent-space index, the host half (include/scann_hip.h): scann_index_silhouette around the kernels of
// scann_silhouette.hip, and the twin scann_silhouette_host (the kernels' bits: the distance chain of scann_knn_distsq, the term of
// scann_silhouette.h, integer sums, the fp64 finish), threaded over the queries.  Every floating-point expression here is evaluated as
// written, each operation rounded to nearest: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <thread>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_runtime.h"
#include "scann_twin.h"
#include "scann_silhouette.h"

using namespace scann;

namespace {

struct Twin {
  const float* rows;    // [n][dim] the pool ...
  const float* rows8;   // ... and its transposed blocks
  int64_t n, dim;
  const int32_t* labels;      // [n]
  const unsigned char* cnt;   // [n] the row counts
  int32_t C;
  const int32_t* qpos;  // [nq] or null: all rows
  int64_t nq;
  bool squared;
  int32_t shift;
  float scale;
  const int64_t* counts;
  double *a, *b;
  int32_t* other;
  int64_t* sums;        // [nq][C] or null
  std::atomic<int>* bad;
};

// a, b, other of a counting query with label ci from its sums: the finish of the definition
void finish_query(const int64_t* S, const int64_t* counts, int32_t C, int32_t shift, int32_t ci, double* a, double* b, int32_t* other) {
  *a = counts[ci] <= 1 ? 0.0 : std::ldexp((double)S[ci], -shift) / (double)(counts[ci] - 1);
  double best = 0.0;
  int32_t bc = -1;
  for (int32_t c = 0; c < C; ++c) {
    if (c == ci || counts[c] <= 0) continue;
    const double m = std::ldexp((double)S[c], -shift) / (double)counts[c];
    if (bc < 0 || m < best) best = m, bc = c;
  }
  *b = bc < 0 ? std::numeric_limits<double>::quiet_NaN() : best;
  *other = bc;
}

// the groups of eight queries first, first + step, ...
__attribute__((always_inline)) inline void twin_groups(const Twin& c, int64_t first, int64_t step) {
  std::vector<int64_t> S((size_t)8 * c.C);
  bool bad = false;
  for (int64_t i0 = 8 * first; i0 < c.nq; i0 += 8 * step) {
    const float* x[8];
    int64_t pos[8];
    bool ok[8];
    for (int u = 0; u < 8; ++u) {
      const int64_t i = std::min(i0 + u, c.nq - 1);
      pos[u] = c.qpos ? c.qpos[i] : i;
      x[u] = c.rows + pos[u] * c.dim;
      ok[u] = i0 + u < c.nq && c.cnt[pos[u]];
    }
    std::fill(S.begin(), S.end(), 0);
    for (int64_t j0 = 0; j0 < c.n; j0 += 8) {
      v8 d[8];
      dist2_8x8(x, c.rows8 + j0 * c.dim, c.dim, d);
      const int m = (int)std::min<int64_t>(8, c.n - j0);
      for (int u = 0; u < 8; ++u) {
        if (!ok[u]) continue;
        for (int l = 0; l < m; ++l) {
          const int64_t j = j0 + l;
          if (!c.cnt[j] || j == pos[u]) continue;
          const float f = sil_scaled(d[u][l], c.squared, c.scale);
          bad |= sil_out_of_range(f);
          S[(size_t)u * c.C + c.labels[j]] += (int64_t)sil_round(f);
        }
      }
    }
    for (int u = 0; u < 8 && i0 + u < c.nq; ++u) {
      const int64_t i = i0 + u;
      if (ok[u]) {
        finish_query(S.data() + (size_t)u * c.C, c.counts, c.C, c.shift, c.labels[pos[u]], c.a + i, c.b + i, c.other + i);
      } else {
        c.a[i] = c.b[i] = std::numeric_limits<double>::quiet_NaN();
        c.other[i] = -1;
      }
      if (c.sums)
        for (int32_t k = 0; k < c.C; ++k) c.sums[i * c.C + k] = ok[u] ? S[(size_t)u * c.C + k] : -1;
    }
  }
  if (bad) c.bad->store(1);
}

// the same loops where the host has AVX2 and a fused multiply-add instruction; fmaf is correctly rounded either way: the same bits
void groups_plain(const Twin& c, int64_t first, int64_t step) { twin_groups(c, first, step); }
__attribute__((target("avx2,fma"))) void groups_fma(const Twin& c, int64_t first, int64_t step) { twin_groups(c, first, step); }

// What both routes check before any work, in the order of the header; empty: fine
std::string bad_arguments(int64_t n, const int32_t* labels, int32_t C, const int32_t* qpos, int64_t nq, int32_t shift, const int64_t* counts,
                          const double* a, const double* b, const int32_t* other) {
  if (C < 1 || C > SCANN_KMEANS_MAX_K) return "C " + std::to_string(C) + " outside 1 .. " + std::to_string(SCANN_KMEANS_MAX_K);
  if (shift < -126 || shift > 126) return "shift " + std::to_string(shift) + " outside -126 .. 126";
  if (!counts) return "counts is null";
  if (n > 0 && !labels) return "labels is null";
  if (qpos && (nq < 0 || nq > (int64_t)0x7fffffff - 1024)) return "nq " + std::to_string(nq) + " outside 0 .. 2^31 - 1025";
  const int64_t m = qpos ? nq : n;
  if (m > 0 && !a) return "a is null";
  if (m > 0 && !b) return "b is null";
  if (m > 0 && !other) return "other is null";
  for (int64_t p = 0; p < n; ++p)
    if (labels[p] < -1 || labels[p] >= C)
      return "labels[" + std::to_string(p) + "] = " + std::to_string(labels[p]) + " outside -1 .. " + std::to_string(C - 1);
  for (int64_t i = 0; qpos && i < nq; ++i)
    if (qpos[i] < 0 || qpos[i] >= n)
      return "qpos[" + std::to_string(i) + "] = " + std::to_string(qpos[i]) + " outside 0 .. " + std::to_string(n - 1);
  return "";
}

}  // namespace

extern "C" {

int scann_silhouette_host(const float* rows, int64_t n, int64_t dim, const int32_t* labels, int32_t C, const int32_t* qpos, int64_t nq,
                          int32_t squared, int32_t shift, int32_t threads, int64_t* counts, double* a, double* b, int32_t* other, int64_t* sums) {
  if (n < 0 || n > (int64_t)0x7fffffff - 1024 || dim < 1 || (n > 0 && !rows) || threads < 0 ||
      !bad_arguments(n, labels, C, qpos, nq, shift, counts, a, b, other).empty())
    return SCANN_ERR_INVALID;
  std::fill(counts, counts + C, 0);
  if (n == 0) return SCANN_OK;
  std::vector<unsigned char> cnt((size_t)n);
  for (int64_t p = 0; p < n; ++p) {
    cnt[(size_t)p] = labels[p] >= 0 && finite_row(rows + p * dim, dim);
    if (cnt[(size_t)p]) ++counts[labels[p]];
  }
  const int64_t m = qpos ? nq : n;
  if (m == 0) return SCANN_OK;
  const std::vector<float> rows8 = transpose8(rows, n, dim);
  std::atomic<int> bad{0};
  Twin c{rows, rows8.data(), n, dim, labels, cnt.data(), C, qpos, m, squared != 0, shift, std::ldexp(1.0f, shift), counts, a, b, other, sums, &bad};
  twin_run(host_fast() ? groups_fma : groups_plain, c, m, threads);
  return bad.load() ? SCANN_ERR_RANGE : SCANN_OK;
}

int scann_index_silhouette(scann_handle_t* h, scann_index_t* pool, const int32_t* labels, int32_t C, const int32_t* qpos, int64_t nq,
                           int32_t squared, int32_t shift, int64_t* counts, double* a, double* b, int32_t* other, int64_t* sums) {
  const std::string w = "scann_index_silhouette: ";
  if (const int r = check_pool(h, pool, "scann_index_silhouette")) return r;
  const int64_t N = pool->n;
  if (const int r = check_pool_rows(h, pool, "scann_index_silhouette", (int64_t)0x7fffffff - 1024)) return r;
  const std::string why = bad_arguments(N, labels, C, qpos, nq, shift, counts, a, b, other);
  if (!why.empty()) return fail(h, SCANN_ERR_INVALID, w + why);
  const int64_t M = qpos ? nq : N;
  if (N == 0) {
    std::fill(counts, counts + C, 0);
    return SCANN_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);

  // 1. which rows are eligible: the rows stay on the device, one byte per row comes back
  std::vector<unsigned char> cnt((size_t)N);
  {
    const float* const* d_rows;
    unsigned char* d_elig;
    CallWs ws;
    ws.take(d_rows, (size_t)n_chunk); ws.take(d_elig, (size_t)N);
    HIPCHK(h, ws.alloc());
    hipError_t e = ws.upload_rows(pool, n_chunk, d_rows, nullptr, s);
    if (e == hipSuccess) e = launch_sil_eligible(d_rows, (int32_t)N, pool->chunk_rows, pool->stride, d_elig, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_elig, (size_t)N, hipMemcpyDeviceToHost, s);
    const hipError_t e_sync = hipStreamSynchronize(s);
    ws.release();
    HIPCHK(h, e);
    HIPCHK(h, e_sync);
  }
  // 2. the counts, and the permutation: the counting positions by (label, position), every cluster padded to whole tiles
  std::vector<int64_t> counts_h((size_t)C, 0);
  for (int64_t p = 0; p < N; ++p) {
    cnt[(size_t)p] = cnt[(size_t)p] && labels[p] >= 0;
    if (cnt[(size_t)p]) ++counts_h[(size_t)labels[p]];
  }
  std::vector<int64_t> first((size_t)C + 1, 0);
  for (int32_t c = 0; c < C; ++c) first[(size_t)c + 1] = first[(size_t)c] + (counts_h[(size_t)c] + TILE_TR - 1) / TILE_TR * TILE_TR;
  const int64_t n_perm = first[(size_t)C];
  if (n_perm > (int64_t)0x7fffffff - 1024) return fail(h, SCANN_ERR_UNSUPPORTED, w + "the padded clusters have too many rows");
  std::vector<int32_t> perm((size_t)n_perm, -1), tile_label((size_t)(n_perm / TILE_TR));
  {
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (int64_t p = 0; p < N; ++p)
      if (cnt[(size_t)p]) perm[(size_t)at[(size_t)labels[p]]++] = (int32_t)p;
    for (int32_t c = 0; c < C; ++c)
      for (int64_t tl = first[(size_t)c] / TILE_TR; tl < first[(size_t)c + 1] / TILE_TR; ++tl) tile_label[(size_t)tl] = c;
  }
  std::vector<int32_t> qp((size_t)M), ql((size_t)M);
  for (int64_t i = 0; i < M; ++i) {
    const int64_t p = qpos ? qpos[i] : i;
    qp[(size_t)i] = cnt[(size_t)p] ? (int32_t)p : -1;
    ql[(size_t)i] = cnt[(size_t)p] ? labels[p] : -1;
  }
  // 3. the queries in slices whose table stays within 512 MiB; everything of the call is enqueued, then one wait
  const int64_t slice = std::max<int64_t>(TILE_TQ, std::min<int64_t>(((int64_t)512 << 20) / (8 * (int64_t)C) / TILE_TQ * TILE_TQ, (M + TILE_TQ - 1) / TILE_TQ * TILE_TQ));
  SilArgs all{};  // the regions of the whole call; a slice's arguments start from a copy
  all.chunk_rows = pool->chunk_rows; all.stride = pool->stride; all.n_perm = (int32_t)n_perm;
  all.squared = squared != 0; all.shift = shift; all.C = C; all.scale = std::ldexp(1.0f, shift);
  const size_t n_q = (size_t)std::max<int64_t>(M, 1);
  CallWs ws;
  ws.take(all.rows, (size_t)n_chunk); ws.take(all.perm, (size_t)std::max<int64_t>(n_perm, 1)); ws.take(all.tile_label, tile_label.size() + 1);
  ws.take(all.counts, (size_t)C); ws.take(all.qpos, n_q); ws.take(all.qlabel, n_q); ws.take(all.other, n_q); ws.take(all.a, n_q); ws.take(all.b, n_q);
  ws.take(all.table, (size_t)slice * C); ws.take(all.flag, 64);
  HIPCHK(h, ws.alloc());
  unsigned long long* const d_table = all.table;
  std::vector<double> a_h((size_t)M), b_h((size_t)M);  // (the outputs change only if the call succeeds)
  std::vector<int32_t> other_h((size_t)M);
  unsigned int flag_h = 0;
  hipError_t e = ws.upload_rows(pool, n_chunk, all.rows, nullptr, s);
  if (e == hipSuccess && n_perm) e = hipMemcpyAsync(writable(all.perm), perm.data(), (size_t)n_perm * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n_perm) e = hipMemcpyAsync(writable(all.tile_label), tile_label.data(), tile_label.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(all.counts), counts_h.data(), (size_t)C * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && M) e = hipMemcpyAsync(writable(all.qpos), qp.data(), (size_t)M * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && M) e = hipMemcpyAsync(writable(all.qlabel), ql.data(), (size_t)M * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(all.flag, 0, 4, s);
  for (int64_t q0 = 0; q0 < M && e == hipSuccess; q0 += slice) {
    const int64_t m = std::min(slice, M - q0);
    SilArgs k = all;
    k.qpos += q0; k.qlabel += q0; k.a += q0; k.b += q0; k.other += q0;
    k.nq = (int32_t)m;
    peaks_geometry(n_perm, m, &k.rows_per_range, &k.n_range);
    e = hipMemsetAsync(d_table, 0, (size_t)m * C * 8, s);
    if (e == hipSuccess) e = launch_sil_tiles(k, s);
    if (e == hipSuccess) e = launch_sil_finish(k, s);
    if (e == hipSuccess && sums) e = hipMemcpyAsync(sums + q0 * C, d_table, (size_t)m * C * 8, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess && M) e = hipMemcpyAsync(a_h.data(), all.a, (size_t)M * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && M) e = hipMemcpyAsync(b_h.data(), all.b, (size_t)M * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && M) e = hipMemcpyAsync(other_h.data(), all.other, (size_t)M * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&flag_h, all.flag, 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  if (flag_h)
    return fail(h, SCANN_ERR_RANGE, w + "a term is not finite or above 2^31 at shift " + std::to_string(shift) + ": lower the shift");
  std::copy(counts_h.begin(), counts_h.end(), counts);
  std::copy(a_h.begin(), a_h.end(), a);
  std::copy(b_h.begin(), b_h.end(), b);
  std::copy(other_h.begin(), other_h.end(), other);
  if (sums)
    for (int64_t i = 0; i < M; ++i)
      if (qp[(size_t)i] < 0) std::fill(sums + i * C, sums + (i + 1) * C, (int64_t)-1);
  return SCANN_OK;
}

}  // extern "C"

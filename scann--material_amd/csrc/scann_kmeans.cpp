// k-means clustering of a latent-space index, the host half (include/scann_hip.h): scann_index_kmeans around the kernels of
// scann_kmeans.hip and the host twin scann_kmeans_host (the distance chain of scann_knn_distsq, integer sums).
#include "scann_call.h"
#include "scann_kmeans.h"
#include "scann_knn.h"
#include "scann_runtime.h"

using namespace scann;

extern "C" {

int64_t scann_kmeans_host(const float* rows, int64_t n, int64_t dim, int32_t k, const float* init, int32_t max_iter, int64_t stop_changed,
                          int32_t* labels, float* dist2, float* centres, int64_t* sizes, int32_t* converged) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || k < 1 || k > SCANN_KMEANS_MAX_K || !init || max_iter < 0 || stop_changed < 0 || !centres ||
      (n > 0 && (!rows || !labels)))
    return SCANN_ERR_INVALID;
  for (int64_t i = 0; i < (int64_t)k * dim; ++i)
    if (!std::isfinite(init[i])) return SCANN_ERR_INVALID;
  std::copy(init, init + (int64_t)k * dim, centres);
  std::vector<char> elig((size_t)n, 1);
  std::vector<int> ex((size_t)dim, 0);
  {
    std::vector<float> mx((size_t)dim, 0.f);
    for (int64_t p = 0; p < n; ++p) {
      elig[(size_t)p] = finite_row(rows + p * dim, dim);
      for (int64_t j = 0; j < dim && elig[(size_t)p]; ++j) mx[(size_t)j] = std::max(mx[(size_t)j], std::fabs(rows[p * dim + j]));
    }
    for (int64_t j = 0; j < dim; ++j) ex[(size_t)j] = frexp_exponent(mx[(size_t)j]);  // the scale of the update's integer sums
  }
  std::vector<int32_t> lab((size_t)n, -1);
  std::vector<float> d2((size_t)n, __builtin_inff()), tmp((size_t)k);
  std::vector<int64_t> sum((size_t)k * dim), cnt((size_t)k);
  int32_t t = 0;
  bool conv = false;
  for (;; ++t) {
    int64_t changed = 0;
    for (int64_t p = 0; p < n; ++p) {
      if (!elig[(size_t)p]) continue;
      dist2_to_rows(rows + p * dim, centres, k, dim, tmp.data());  // the row first
      int32_t best = -1;
      for (int32_t c = 0; c < k; ++c)  // dist2 ascending, index ascending; a NaN distance never qualifies
        if (tmp[(size_t)c] == tmp[(size_t)c] && (best < 0 || tmp[(size_t)c] < tmp[(size_t)best])) best = c;
      changed += best != lab[(size_t)p];
      lab[(size_t)p] = best;
      d2[(size_t)p] = best < 0 ? __builtin_inff() : tmp[(size_t)best];
    }
    conv = changed <= stop_changed;
    if (conv || t == max_iter) break;
    std::fill(sum.begin(), sum.end(), 0);
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int64_t p = 0; p < n; ++p) {
      const int32_t c = lab[(size_t)p];
      if (c < 0) continue;
      ++cnt[(size_t)c];
      for (int64_t j = 0; j < dim; ++j) sum[(size_t)c * dim + j] += std::llrint(std::ldexp((double)rows[p * dim + j], 30 - ex[(size_t)j]));
    }
    for (int32_t c = 0; c < k; ++c)
      for (int64_t j = 0; j < dim && cnt[(size_t)c] > 0; ++j)
        centres[(int64_t)c * dim + j] = (float)std::ldexp((double)sum[(size_t)c * dim + j] / (double)cnt[(size_t)c], ex[(size_t)j] - 30);
  }
  if (n > 0) std::copy(lab.begin(), lab.end(), labels);
  if (dist2 && n > 0) std::copy(d2.begin(), d2.end(), dist2);
  if (sizes) {
    std::fill(sizes, sizes + k, 0);
    for (int64_t p = 0; p < n; ++p)
      if (lab[(size_t)p] >= 0) ++sizes[lab[(size_t)p]];
  }
  if (converged) *converged = conv ? 1 : 0;
  return t;
}

int64_t scann_index_kmeans(scann_handle_t* h, scann_index_t* pool, int32_t k, const float* init, const int32_t* init_pos, int32_t max_iter,
                           int64_t stop_changed, int32_t* labels, float* dist2, float* centres, int64_t* sizes, int32_t* converged) {
  if (const int r = check_pool(h, pool, "scann_index_kmeans")) return r;
  if (k < 1 || k > SCANN_KMEANS_MAX_K)
    return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: k " + std::to_string(k) + " outside 1 .. " + std::to_string(SCANN_KMEANS_MAX_K));
  if ((init != nullptr) == (init_pos != nullptr))
    return fail(h, SCANN_ERR_INVALID, std::string("scann_index_kmeans: exactly one of init and init_pos must be given, got ") + (init ? "both" : "neither"));
  if (max_iter < 0) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: max_iter " + std::to_string(max_iter) + " is negative");
  if (stop_changed < 0) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: stop_changed " + std::to_string(stop_changed) + " is negative");
  if (!labels) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: labels is null");
  if (!centres) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: centres is null");
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride;
  if (const int r = check_pool_rows(h, pool, "scann_index_kmeans", (int64_t)0x7fffffff - 1024)) return r;
  for (int64_t i = 0; init && i < (int64_t)k * dim; ++i)
    if (!std::isfinite(init[i]))
      return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: init holds a non-finite value (centre " + std::to_string(i / dim) + ", column " +
                                            std::to_string(i % dim) + ")");
  for (int32_t c = 0; init_pos && c < k; ++c)
    if (init_pos[c] < 0 || init_pos[c] >= N)
      return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: init_pos[" + std::to_string(c) + "] = " + std::to_string(init_pos[c]) + " outside the pool's " +
                                            std::to_string(N) + " rows");
  if (N == 0) {  // (init: init_pos has nothing to point at)
    std::copy(init, init + (int64_t)k * dim, centres);
    if (sizes) std::fill(sizes, sizes + k, 0);
    if (converged) *converged = 1;
    return 0;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  KmArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride; a.dim = dim; a.k = k;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  a.tiles_per_chunk = (pool->chunk_rows + KM_TP - 1) / KM_TP;
  a.n_tile = a.n_chunk * a.tiles_per_chunk;
  a.max_iter = max_iter; a.stop_changed = stop_changed;
  // one workspace for the call.  First what the memset clears: the state, the column maxima, the counts, the sums; then the centres,
  // the initial positions, the chunk table, labels, dist2 and the eligibility bytes
  CallWs ws;
  int32_t* d_pos;
  ws.take(a.st, 1); ws.take(a.colmax, (size_t)stride); ws.take(a.counts, (size_t)k); ws.take(a.sums, (size_t)k * stride);
  ws.take(a.centres, (size_t)k * stride);
  const size_t zeroed = ws.bytes();  // (the centres' padding columns are zero)
  ws.take(d_pos, (size_t)k); ws.take(a.rows, (size_t)a.n_chunk); ws.take(a.labels, (size_t)N); ws.take(a.dist2, (size_t)N); ws.take(a.elig, (size_t)N);
  HIPCHK(h, ws.alloc());
  a.init_pos = init_pos ? d_pos : nullptr;
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, a.n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess && init) e = hipMemcpy2DAsync(a.centres, (size_t)stride * 4, init, (size_t)dim * 4, (size_t)dim * 4, (size_t)k, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && init_pos) e = hipMemcpyAsync(d_pos, init_pos, (size_t)k * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_kmeans_prepare(a, s);
  if (e == hipSuccess) e = launch_kmeans_gather(a, s);  // (init_pos: the centres never leave the device)
  // every round is enqueued at once: whether the loop has ended travels from launch to launch through device memory.  (The state holds
  // KM_ROUNDS counters: a longer run waits after that many rounds and clears them.)
  KmState st{};
  for (int64_t t0 = 0; t0 <= max_iter && e == hipSuccess; t0 += KM_ROUNDS) {
    if (t0 > 0) e = hipMemsetAsync(reinterpret_cast<char*>(a.st) + offsetof(KmState, changed), 0, sizeof(st.changed), s);
    for (int64_t t = t0; t <= max_iter && t < t0 + KM_ROUNDS && e == hipSuccess; ++t) e = launch_kmeans_round(a, (int)t, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(KmState), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (st.done) break;
  }
  const bool ok = e == hipSuccess && st.done && !st.bad_init;
  if (ok) e = hipMemcpyAsync(labels, a.labels, (size_t)N * 4, hipMemcpyDeviceToHost, s);
  if (ok && e == hipSuccess && dist2) e = hipMemcpyAsync(dist2, a.dist2, (size_t)N * 4, hipMemcpyDeviceToHost, s);
  if (ok && e == hipSuccess)
    e = hipMemcpy2DAsync(centres, (size_t)dim * 4, a.centres, (size_t)stride * 4, (size_t)dim * 4, (size_t)k, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  if (st.bad_init) {
    const int32_t c = k - st.bad_init;
    return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: init_pos[" + std::to_string(c) + "] = " + std::to_string(init_pos[c]) +
                                          " names a row with a non-finite component");
  }
  if (!st.done) return fail(h, SCANN_ERR_HIP, "scann_index_kmeans: the loop did not end");
  if (sizes) {
    std::fill(sizes, sizes + k, 0);
    for (int64_t p = 0; p < N; ++p)
      if (labels[p] >= 0) ++sizes[labels[p]];
  }
  if (converged) *converged = st.converged;
  return st.n_iter;
}

}  // extern "C"

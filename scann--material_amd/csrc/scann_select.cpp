// Greedy k-center selection from a latent-space index, the host half (include/scann_hip.h): scann_index_select around the kernels of
// scann_select.hip and the host twin scann_kcenter_host (the distance chain of scann_knn_distsq).
#include "scann_call.h"
#include "scann_knn.h"
#include "scann_runtime.h"
#include "scann_select.h"

using namespace scann;

namespace {

// the places of a selection's outputs from `from` on: no pick
void select_tail(int64_t from, int64_t m, int32_t* pos, int64_t* ids, int32_t* atoms, float* radius2) {
  for (int64_t i = from; i < m; ++i) {
    pos[i] = -1;
    if (ids) ids[i] = -1;
    if (atoms) atoms[i] = -1;
    if (radius2) radius2[i] = __builtin_inff();
  }
}

}  // namespace

extern "C" {

int64_t scann_kcenter_host(const float* rows, int64_t n, const float* ref, int64_t nr, int64_t dim, int64_t m, float stop_dist2, int32_t* pos,
                           float* radius2) {
  if (n < 0 || nr < 0 || dim < 1 || m < 1 || stop_dist2 != stop_dist2 || !pos || (n > 0 && !rows) || (nr > 0 && !ref) || n > (int64_t)0x7fffffff)
    return SCANN_ERR_INVALID;
  select_tail(0, m, pos, nullptr, nullptr, radius2);
  if (n == 0) return 0;
  std::vector<float> mind((size_t)n, __builtin_inff()), tmp((size_t)std::max(n, nr));
  std::vector<char> live((size_t)n);
  for (int64_t p = 0; p < n; ++p) live[(size_t)p] = finite_row(rows + p * dim, dim);
  for (int64_t p = 0; p < n && nr > 0; ++p) {
    if (!live[(size_t)p]) continue;
    dist2_to_rows(rows + p * dim, ref, nr, dim, tmp.data());
    for (int64_t r = 0; r < nr; ++r)  // a NaN distance never counts
      if (tmp[(size_t)r] < mind[(size_t)p]) mind[(size_t)p] = tmp[(size_t)r];
  }
  int64_t cnt = 0;
  while (cnt < m) {
    int64_t best = -1;
    for (int64_t p = 0; p < n; ++p)  // mind descending, position ascending
      if (live[(size_t)p] && (best < 0 || mind[(size_t)p] > mind[(size_t)best])) best = p;
    if (best < 0 || (stop_dist2 > 0.f && mind[(size_t)best] < stop_dist2)) break;
    pos[cnt] = (int32_t)best;
    if (radius2) radius2[cnt] = mind[(size_t)best];
    live[(size_t)best] = 0;
    if (++cnt == m) break;
    dist2_to_rows(rows + best * dim, rows, n, dim, tmp.data());
    for (int64_t p = 0; p < n; ++p)
      if (live[(size_t)p] && tmp[(size_t)p] < mind[(size_t)p]) mind[(size_t)p] = tmp[(size_t)p];
  }
  return cnt;
}

int64_t scann_index_select(scann_handle_t* h, scann_index_t* pool, scann_index_t* reference, int64_t m, float stop_dist2, int32_t* pos, int64_t* ids,
                           int32_t* atoms, float* radius2) {
  if (const int r = check_pool(h, pool, "scann_index_select")) return r;
  if (reference == pool) return fail(h, SCANN_ERR_INVALID, "scann_index_select: the reference is the pool itself");
  if (reference && reference->h != h) return fail(h, SCANN_ERR_INVALID, "scann_index_select: the reference belongs to another handle");
  if (reference && reference->dim != pool->dim)
    return fail(h, SCANN_ERR_INVALID, "scann_index_select: the pool holds rows of " + std::to_string(pool->dim) + " columns, the reference of " +
                                          std::to_string(reference->dim));
  if (m < 1) return fail(h, SCANN_ERR_INVALID, "scann_index_select: m " + std::to_string(m) + " is not >= 1");
  if (stop_dist2 != stop_dist2) return fail(h, SCANN_ERR_INVALID, "scann_index_select: stop_dist2 is NaN");
  if (!pos) return fail(h, SCANN_ERR_INVALID, "scann_index_select: pos is null");
  const int64_t N = pool->n;
  if (const int r = check_pool_rows(h, pool, "scann_index_select", (int64_t)0x7fffffff - 2 * KC_LANES)) return r;
  select_tail(0, m, pos, ids, atoms, radius2);
  if (N == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  KcArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = pool->stride;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  a.tiles_per_chunk = (pool->chunk_rows + KC_LANES - 1) / KC_LANES;
  a.n_tile = a.n_chunk * a.tiles_per_chunk;
  a.n_pick = (int32_t)std::min<int64_t>(m, N);
  a.stop = stop_dist2;
  const int groups = std::min(a.n_tile, KC_MAX_GROUPS);
  // one workspace for the call: the state (first: it is what the memset clears), mind, the picks, the candidates, the chunk table, live
  CallWs ws;
  ws.take(a.st, 1); ws.take(a.mind, (size_t)N); ws.take(a.out_pos, (size_t)a.n_pick); ws.take(a.out_r2, (size_t)a.n_pick);
  ws.take(a.part, (size_t)groups); ws.take(a.rows, (size_t)a.n_chunk); ws.take(a.live, (size_t)N);
  HIPCHK(h, ws.alloc());
  const bool has_ref = reference && reference->n > 0;
  int r = SCANN_OK;
  hipError_t e = hipMemsetAsync(a.st, 0, sizeof(KcState), s);
  if (e == hipSuccess) e = ws.upload_rows(pool, a.n_chunk, a.rows, nullptr, s);
  // the initial mind: the k = 1 query of the pool's own rows, chunk by chunk where they lie, against the reference
  for (int c = 0; c < a.n_chunk && has_ref && e == hipSuccess && !r; ++c)
    r = search(h, reference, pool->rows_of((size_t)c), nullptr, std::min<int64_t>(pool->chunk_rows, N - (int64_t)c * pool->chunk_rows), 1, s, nullptr,
               nullptr, nullptr, nullptr, a.mind + (size_t)c * pool->chunk_rows);
  if (e == hipSuccess && !r) e = launch_kcenter_prepare(a, has_ref, s);
  // every pick is enqueued at once: a pick reads its predecessor's position, and whether the selection has ended, from device memory
  for (int i = 0; i < a.n_pick && e == hipSuccess && !r; ++i) e = launch_kcenter_step(a, groups, s);
  KcState st{};
  std::vector<int32_t> pos_h((size_t)a.n_pick);
  std::vector<float> r2_h((size_t)a.n_pick);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(pos_h.data(), a.out_pos, (size_t)a.n_pick * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(r2_h.data(), a.out_r2, (size_t)a.n_pick * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(&st, a.st, sizeof(KcState), hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  if (r) return r;
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  const int64_t cnt = std::min<int64_t>(std::max<int32_t>(st.count, 0), a.n_pick);
  for (int64_t i = 0; i < cnt; ++i) {
    const int32_t p = pos_h[(size_t)i];
    pos[i] = p;
    if (ids) ids[i] = pool->ids[(size_t)p];
    if (atoms) atoms[i] = pool->atoms[(size_t)p];
    if (radius2) radius2[i] = r2_h[(size_t)i];
  }
  return cnt;
}

}  // extern "C"

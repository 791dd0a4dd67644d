// Prototypes and criticisms of a latent-space index (MMD-critic), the host half (include/scann_hip.h): scann_index_prototypes and
// scann_index_criticisms around the kernels of scann_proto.hip and the self-join of scann_peaks.hip, and the twins scann_prototypes_host
// and scann_criticisms_host (the kernels' bits: the distance chain of scann_knn_distsq, the term of scann_peaks.h, integer sums and
// scores), threaded over the rows.
#include <thread>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_proto.h"
#include "scann_runtime.h"
#include "scann_twin.h"

using namespace scann;

namespace {

// fn(lo, hi) over the rows [0, n) cut into one range per thread; every row's result is its own
template <class F>
void over_rows(int64_t n, int64_t dim, const F& fn) {
  const double work = (double)n * (double)dim;
  const int64_t nt = std::max<int64_t>(1, std::min<int64_t>({(int64_t)(work < 4e6 ? 1 : 16), (int64_t)std::thread::hardware_concurrency(), (n + 1023) / 1024}));
  if (nt == 1) return fn((int64_t)0, n);
  const int64_t per = (n + nt - 1) / nt;
  std::vector<std::thread> pool;
  for (int64_t k = 0; k < nt; ++k) pool.emplace_back([&fn, k, per, n] { fn(std::min(k * per, n), std::min((k + 1) * per, n)); });
  for (auto& th : pool) th.join();
}

// term[i] = t(i, pick) for every row i with use[i] != 0 (0 elsewhere); tmp [n]
void column_terms(const float* rows, int64_t n, int64_t dim, int64_t pick, float gamma, const uint8_t* use, float* tmp, int32_t* term) {
  over_rows(n, dim, [&](int64_t lo, int64_t hi) {
    dist2_to_rows(rows + pick * dim, rows + lo * dim, hi - lo, dim, tmp + lo);
    for (int64_t i = lo; i < hi; ++i) term[i] = use[i] ? peaks_term(tmp[i], gamma) : 0;
  });
}

// the places of a selection's outputs from `from` on: no pick
void proto_tail(int64_t from, int64_t m, int32_t* pos, int64_t* ids, int32_t* atoms, int64_t* score, int64_t* b_at_pick) {
  for (int64_t i = from; i < m; ++i) {
    pos[i] = -1;
    if (ids) ids[i] = -1;
    if (atoms) atoms[i] = -1;
    if (score) score[i] = 0;
    if (b_at_pick) b_at_pick[i] = 0;
  }
}

// the first weight outside 0 .. 2^31, or -1
int64_t bad_weight(const int64_t* weight, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (weight[i] < 0 || weight[i] > PT_MAX_WEIGHT) return i;
  return -1;
}

ProtoArgs proto_args(const scann_index* pool, int64_t picks, float gamma) {
  ProtoArgs a{};
  a.n_total = (int32_t)pool->n; a.chunk_rows = pool->chunk_rows; a.stride = pool->stride;
  a.n_chunk = (int)((pool->n + pool->chunk_rows - 1) / pool->chunk_rows);
  a.tiles_per_chunk = (pool->chunk_rows + PT_LANES - 1) / PT_LANES;
  a.n_tile = a.n_chunk * a.tiles_per_chunk;
  a.n_pick = (int32_t)std::min<int64_t>(picks, pool->n);
  a.gamma = gamma;
  return a;
}

}  // namespace

extern "C" {

int64_t scann_prototypes_host(const float* rows, int64_t n, int64_t dim, int64_t m, float gamma, int32_t* pos, int64_t* score, int64_t* b_at_pick,
                              int64_t* A, int64_t* B) {
  if (n < 0 || n > (int64_t)0x7fffffff - 1024 || dim < 1 || m < 1 || bad_gamma(gamma) || !pos || (n > 0 && !rows)) return SCANN_ERR_INVALID;
  if ((__int128)n * m > PT_RANGE) return SCANN_ERR_INVALID;
  proto_tail(0, m, pos, nullptr, nullptr, score, b_at_pick);
  if (n == 0) return 0;
  // A: the sums of the rows as queries of their own pool, nothing left out: t(i, i) = 2^30 is part of them
  std::vector<int64_t> a((size_t)n), b((size_t)n, 0);
  if (const int r = scann_density_host(rows, n, dim, rows, n, nullptr, gamma, a.data())) return r;
  std::vector<uint8_t> live((size_t)n), elig((size_t)n);
  int64_t n_el = 0;
  for (int64_t i = 0; i < n; ++i) n_el += elig[(size_t)i] = live[(size_t)i] = a[(size_t)i] >= 0;
  std::vector<float> tmp((size_t)n);
  std::vector<int32_t> term((size_t)n);
  int64_t cnt = 0;
  while (cnt < m) {
    int64_t best = -1, bs = 0;
    for (int64_t i = 0; i < n; ++i) {  // score descending, position ascending
      if (!live[(size_t)i]) continue;
      const int64_t s = (cnt + 1) * a[(size_t)i] - n_el * b[(size_t)i];
      if (best < 0 || s > bs) best = i, bs = s;
    }
    if (best < 0) break;
    pos[cnt] = (int32_t)best;
    if (score) score[cnt] = bs;
    if (b_at_pick) b_at_pick[cnt] = b[(size_t)best];
    live[(size_t)best] = 0;
    ++cnt;
    column_terms(rows, n, dim, best, gamma, elig.data(), tmp.data(), term.data());  // the last pick's column is folded as well
    for (int64_t i = 0; i < n; ++i) b[(size_t)i] += term[(size_t)i];
  }
  if (A) std::copy(a.begin(), a.end(), A);
  if (B) std::copy(b.begin(), b.end(), B);
  return cnt;
}

int64_t scann_criticisms_host(const float* rows, int64_t n, int64_t dim, const int64_t* weight, const int32_t* exclude, int64_t n_exclude, int64_t c,
                              float gamma, int32_t* pos, int64_t* score) {
  if (n < 0 || n > (int64_t)0x7fffffff - 1024 || dim < 1 || c < 1 || bad_gamma(gamma) || !pos || (n > 0 && (!rows || !weight)) || n_exclude < 0 ||
      (n_exclude > 0 && !exclude))
    return SCANN_ERR_INVALID;
  if (bad_weight(weight, n) >= 0) return SCANN_ERR_INVALID;
  for (int64_t i = 0; i < n_exclude; ++i)
    if (exclude[i] < 0 || exclude[i] >= n) return SCANN_ERR_INVALID;
  proto_tail(0, c, pos, nullptr, nullptr, score, nullptr);
  if (n == 0) return 0;
  std::vector<uint8_t> live((size_t)n);
  for (int64_t i = 0; i < n; ++i) live[(size_t)i] = weight[i] > 0 && finite_row(rows + i * dim, dim);
  for (int64_t i = 0; i < n_exclude; ++i) live[(size_t)exclude[i]] = 0;
  std::vector<float> tmp((size_t)n);
  std::vector<int32_t> term((size_t)n), cmax((size_t)n, 0);
  int64_t cnt = 0;
  while (cnt < c) {
    int64_t best = -1, bs = 0;
    for (int64_t i = 0; i < n; ++i) {  // score descending, position ascending
      if (!live[(size_t)i]) continue;
      const int64_t s = weight[i] * (PT_ONE - cmax[(size_t)i]);
      if (best < 0 || s > bs) best = i, bs = s;
    }
    if (best < 0 || bs <= 0) break;
    pos[cnt] = (int32_t)best;
    if (score) score[cnt] = bs;
    live[(size_t)best] = 0;
    if (++cnt == c) break;
    column_terms(rows, n, dim, best, gamma, live.data(), tmp.data(), term.data());
    for (int64_t i = 0; i < n; ++i) cmax[(size_t)i] = std::max(cmax[(size_t)i], term[(size_t)i]);
  }
  return cnt;
}

int64_t scann_index_prototypes(scann_handle_t* h, scann_index_t* pool, int64_t m, float gamma, int32_t* pos, int64_t* ids, int32_t* atoms,
                               int64_t* score, int64_t* b_at_pick, int64_t* A, int64_t* B) {
  const std::string w = "scann_index_prototypes: ";
  if (const int r = check_pool(h, pool, "scann_index_prototypes")) return r;
  if (m < 1) return fail(h, SCANN_ERR_INVALID, w + "m " + std::to_string(m) + " is not >= 1");
  if (bad_gamma(gamma)) return fail(h, SCANN_ERR_INVALID, w + "gamma must be finite and > 0");
  if (!pos) return fail(h, SCANN_ERR_INVALID, w + "pos is null");
  const int64_t N = pool->n;
  if (const int r = check_pool_rows(h, pool, "scann_index_prototypes", (int64_t)0x7fffffff - 1024)) return r;
  if ((__int128)N * m > PT_RANGE)
    return fail(h, SCANN_ERR_INVALID, w + "the pool's " + std::to_string(N) + " rows times m " + std::to_string(m) + " pass 2^32: a score would leave int64");
  proto_tail(0, m, pos, ids, atoms, score, b_at_pick);
  if (N == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  ProtoArgs a = proto_args(pool, m, gamma);
  const int groups = std::min(a.n_tile, PT_MAX_GROUPS);
  // one workspace for the call: the state and B (first: they are what the memset clears), A, live, the candidates, the picks, the chunk table
  CallWs ws;
  ws.take(a.st, 1); ws.take(a.B, (size_t)N);
  const size_t zeroed = ws.bytes();
  ws.take(a.A, (size_t)N); ws.take(a.live, (size_t)N); ws.take(a.part_v, (size_t)groups); ws.take(a.part_p, (size_t)groups);
  ws.take(a.out_pos, (size_t)a.n_pick); ws.take(a.out_score, (size_t)a.n_pick); ws.take(a.rows, (size_t)a.n_chunk);
  HIPCHK(h, ws.alloc());
  // A: the self-join of the density pass, device to device (S_i over j != i, -1 for an ineligible row), then + t(i, i)
  PeaksArgs pa{};
  pa.rows = a.rows; pa.n_total = a.n_total; pa.chunk_rows = a.chunk_rows; pa.stride = a.stride;
  pa.nq = a.n_total; pa.gamma = gamma; pa.sums = reinterpret_cast<unsigned long long*>(a.A);
  peaks_geometry(N, N, &pa.rows_per_range, &pa.n_range);
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = hipMemsetAsync(a.A, 0, (size_t)N * 8, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, a.n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess) e = launch_peaks_density(pa, s);
  if (e == hipSuccess) e = launch_peaks_finish(pa, s);
  if (e == hipSuccess) e = launch_proto_prepare(a, s);
  // every pick is enqueued at once: a pick reads its predecessor's position, and whether the selection has ended, from device memory;
  // the launch behind the last pick only folds its column
  for (int i = 0; i <= a.n_pick && e == hipSuccess; ++i) e = launch_proto_step(a, false, groups, s);
  ProtoState st{};
  std::vector<int32_t> pos_h((size_t)a.n_pick);
  std::vector<int64_t> score_h((size_t)a.n_pick), A_h((size_t)N), B_h(B ? (size_t)N : 0);
  if (e == hipSuccess) e = hipMemcpyAsync(pos_h.data(), a.out_pos, (size_t)a.n_pick * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(score_h.data(), a.out_score, (size_t)a.n_pick * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(A_h.data(), a.A, (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && B) e = hipMemcpyAsync(B_h.data(), a.B, (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(ProtoState), hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  const int64_t cnt = std::min<int64_t>(std::max<int32_t>(st.count, 0), a.n_pick);
  for (int64_t i = 0; i < cnt; ++i) {
    const int32_t p = pos_h[(size_t)i];
    pos[i] = p;
    if (ids) ids[i] = pool->ids[(size_t)p];
    if (atoms) atoms[i] = pool->atoms[(size_t)p];
    if (score) score[i] = score_h[(size_t)i];
    // score = (i + 1) A_p - n B_p with n >= 1: B_p as it stood at the pick, exactly
    if (b_at_pick) b_at_pick[i] = ((i + 1) * A_h[(size_t)p] - score_h[(size_t)i]) / st.n;
  }
  if (A) std::copy(A_h.begin(), A_h.end(), A);
  if (B) std::copy(B_h.begin(), B_h.end(), B);
  return cnt;
}

int64_t scann_index_criticisms(scann_handle_t* h, scann_index_t* pool, const int64_t* weight, const int32_t* exclude, int64_t n_exclude, int64_t c,
                               float gamma, int32_t* pos, int64_t* ids, int32_t* atoms, int64_t* score) {
  const std::string w = "scann_index_criticisms: ";
  if (const int r = check_pool(h, pool, "scann_index_criticisms")) return r;
  if (c < 1) return fail(h, SCANN_ERR_INVALID, w + "c " + std::to_string(c) + " is not >= 1");
  if (bad_gamma(gamma)) return fail(h, SCANN_ERR_INVALID, w + "gamma must be finite and > 0");
  if (!pos) return fail(h, SCANN_ERR_INVALID, w + "pos is null");
  const int64_t N = pool->n;
  if (const int r = check_pool_rows(h, pool, "scann_index_criticisms", (int64_t)0x7fffffff - 1024)) return r;
  if (N > 0 && !weight) return fail(h, SCANN_ERR_INVALID, w + "weight is null");
  if (n_exclude < 0 || n_exclude > (int64_t)0x7fffffff) return fail(h, SCANN_ERR_INVALID, w + "n_exclude " + std::to_string(n_exclude) + " outside 0 .. 2^31 - 1");
  if (n_exclude > 0 && !exclude) return fail(h, SCANN_ERR_INVALID, w + "exclude is null");
  if (const int64_t i = bad_weight(weight, N); i >= 0)
    return fail(h, SCANN_ERR_INVALID, w + "weight[" + std::to_string(i) + "] = " + std::to_string(weight[i]) + " outside 0 .. 2^31");
  for (int64_t i = 0; i < n_exclude; ++i)
    if (exclude[i] < 0 || exclude[i] >= N)
      return fail(h, SCANN_ERR_INVALID, w + "exclude[" + std::to_string(i) + "] = " + std::to_string(exclude[i]) + " outside the pool's " + std::to_string(N) + " rows");
  proto_tail(0, c, pos, ids, atoms, score, nullptr);
  if (N == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  ProtoArgs a = proto_args(pool, c, gamma);
  const int groups = std::min(a.n_tile, PT_MAX_GROUPS);
  // one workspace for the call: the state and Cmax (first: they are what the memset clears), the weights, live, the candidates, the
  // picks, the excluded positions, the chunk table
  CallWs ws;
  int32_t* d_ex;
  ws.take(a.st, 1); ws.take(a.cmax, (size_t)N);
  const size_t zeroed = ws.bytes();
  ws.take(a.A, (size_t)N); ws.take(a.live, (size_t)N); ws.take(a.part_v, (size_t)groups); ws.take(a.part_p, (size_t)groups);
  ws.take(a.out_pos, (size_t)a.n_pick); ws.take(a.out_score, (size_t)a.n_pick); ws.take(d_ex, (size_t)n_exclude); ws.take(a.rows, (size_t)a.n_chunk);
  HIPCHK(h, ws.alloc());
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, a.n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess) e = hipMemcpyAsync(a.A, weight, (size_t)N * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n_exclude > 0) e = hipMemcpyAsync(d_ex, exclude, (size_t)n_exclude * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_crit_prepare(a, d_ex, (int32_t)n_exclude, s);
  for (int i = 0; i < a.n_pick && e == hipSuccess; ++i) e = launch_proto_step(a, true, groups, s);
  ProtoState st{};
  std::vector<int32_t> pos_h((size_t)a.n_pick);
  std::vector<int64_t> score_h((size_t)a.n_pick);
  if (e == hipSuccess) e = hipMemcpyAsync(pos_h.data(), a.out_pos, (size_t)a.n_pick * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(score_h.data(), a.out_score, (size_t)a.n_pick * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(ProtoState), hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  const int64_t cnt = std::min<int64_t>(std::max<int32_t>(st.count, 0), a.n_pick);
  for (int64_t i = 0; i < cnt; ++i) {
    const int32_t p = pos_h[(size_t)i];
    pos[i] = p;
    if (ids) ids[i] = pool->ids[(size_t)p];
    if (atoms) atoms[i] = pool->atoms[(size_t)p];
    if (score) score[i] = score_h[(size_t)i];
  }
  return cnt;
}

}  // extern "C"

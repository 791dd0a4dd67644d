// Exact neighbour ranks of a latent-space index, the host half (include/scann_hip.h): scann_index_ranks around the kernels of
// scann_ranks.hip, and the twin scann_ranks_host (the kernels' bits: the distance chain of scann_knn_distsq, the key order and the bin
// search of scann_ranks.h, integer counts), threaded over the queries.  Every floating-point expression here is evaluated as written,
// each operation rounded to nearest: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <limits>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_runtime.h"
#include "scann_twin.h"
#include "scann_silhouette.h"
#include "scann_ranks.h"

using namespace scann;

namespace {

static_assert(RANKS_MP == SCANN_RANKS_MAX_PROBES && RANKS_SLICE == SCANN_RANKS_SLICE, "the header's constants");

struct Twin {
  const float* rows;    // [n][dim] the pool ...
  const float* rows8;   // ... and its transposed blocks
  int64_t n, dim;
  const unsigned char* elig;  // [n]
  const int32_t* qpos;  // [nq] or null: all rows
  int64_t nq;
  const int32_t* probe; // [nq][m]
  int32_t m;
  int32_t* rank;        // [nq][m]
  float* dist2;         // [nq][m] or null
};

// the chain of scann_knn_distsq, q first
inline float chain(const float* q, const float* r, int64_t d) {
  float acc = 0.f;
  for (int64_t j = 0; j < d; ++j) {
    const float t = q[j] - r[j];
    acc = std::fmaf(t, t, acc);
  }
  return acc;
}

// One query's sorted thresholds: the keys of its probes that have a rank, ascending, behind them (+inf, RANKS_NO_POS)
struct Thresholds {
  float d[RANKS_MP];
  int32_t p[RANKS_MP];
  int32_t slot_probe[RANKS_MP];  // >= m: none
  float dmax;                    // -1: no probe has a rank
  uint32_t hist[RANKS_MP];
};

void thresholds_of(const Twin& c, int64_t i, int64_t pos, bool q_ok, Thresholds* th) {
  float d[RANKS_MP];
  int32_t p[RANKS_MP];
  th->dmax = -1.f;
  for (int32_t k = 0; k < RANKS_MP; ++k) {
    const int32_t pr = k < c.m ? c.probe[i * c.m + k] : -1;
    const bool has = q_ok && pr >= 0 && pr != pos && c.elig[pr];
    d[k] = has ? chain(c.rows + pos * c.dim, c.rows + (int64_t)pr * c.dim, c.dim) : std::numeric_limits<float>::infinity();
    p[k] = has ? pr : RANKS_NO_POS;
    if (has) th->dmax = std::max(th->dmax, d[k]);
  }
  for (int32_t k = 0; k < RANKS_MP; ++k) {  // the slot: the keys before this one, equal keys in probe order
    int32_t slot = 0;
    for (int32_t o = 0; o < RANKS_MP; ++o) {
      const bool same = d[o] == d[k] && p[o] == p[k];
      slot += same ? o < k : ranks_key_le(d[o], p[o], d[k], p[k]);
    }
    th->d[slot] = d[k], th->p[slot] = p[k], th->slot_probe[slot] = k;
  }
  std::fill(th->hist, th->hist + RANKS_MP, 0u);
}

// the groups of eight queries first, first + step, ...
__attribute__((always_inline)) inline void twin_groups(const Twin& c, int64_t first, int64_t step) {
  std::vector<Thresholds> th(8);
  for (int64_t i0 = 8 * first; i0 < c.nq; i0 += 8 * step) {
    const float* x[8];
    int64_t pos[8];
    for (int u = 0; u < 8; ++u) {
      const int64_t i = std::min(i0 + u, c.nq - 1);
      pos[u] = c.qpos ? c.qpos[i] : i;
      x[u] = c.rows + pos[u] * c.dim;
      thresholds_of(c, i, pos[u], i0 + u < c.nq && c.elig[pos[u]], &th[(size_t)u]);
    }
    for (int64_t j0 = 0; j0 < c.n; j0 += 8) {
      v8 d[8];
      dist2_8x8(x, c.rows8 + j0 * c.dim, c.dim, d);
      const int m = (int)std::min<int64_t>(8, c.n - j0);
      for (int u = 0; u < 8; ++u) {
        Thresholds& t = th[(size_t)u];
        for (int l = 0; l < m; ++l) {
          const int64_t j = j0 + l;
          if (!(d[u][l] <= t.dmax) || !c.elig[j] || j == pos[u]) continue;  // above every threshold: the row counts nowhere
          const int bin = ranks_bin<RANKS_MP>(t.d, 1, t.p, d[u][l], (int32_t)j);
          if (bin < RANKS_MP) ++t.hist[bin];
        }
      }
    }
    for (int u = 0; u < 8 && i0 + u < c.nq; ++u) {
      const Thresholds& t = th[(size_t)u];
      uint32_t below = 0;
      for (int32_t s = 0; s < RANKS_MP; ++s) {
        below += t.hist[s];
        const int32_t k = t.slot_probe[s];
        if (k >= c.m) continue;
        const bool has = t.p[s] != RANKS_NO_POS;
        c.rank[(i0 + u) * c.m + k] = has ? (int32_t)below : -1;
        if (c.dist2) c.dist2[(i0 + u) * c.m + k] = has ? t.d[s] : std::numeric_limits<float>::infinity();
      }
    }
  }
}

// the same loops where the host has AVX2 and a fused multiply-add instruction; fmaf is correctly rounded either way: the same bits
void groups_plain(const Twin& c, int64_t first, int64_t step) { twin_groups(c, first, step); }
__attribute__((target("avx2,fma"))) void groups_fma(const Twin& c, int64_t first, int64_t step) { twin_groups(c, first, step); }

// What both routes check before any work, in the order of the header; empty: fine
std::string bad_arguments(int64_t n, const int32_t* qpos, int64_t nq, const int32_t* probe, int32_t m, const int32_t* rank) {
  if (m < 1 || m > SCANN_RANKS_MAX_PROBES) return "m " + std::to_string(m) + " outside 1 .. " + std::to_string(SCANN_RANKS_MAX_PROBES);
  if (qpos && (nq < 0 || nq > (int64_t)0x7fffffff - 1024)) return "nq " + std::to_string(nq) + " outside 0 .. 2^31 - 1025";
  const int64_t M = qpos ? nq : n;
  if (M > 0 && !probe) return "probe is null";
  if (M > 0 && !rank) return "rank is null";
  for (int64_t i = 0; qpos && i < nq; ++i)
    if (qpos[i] < 0 || qpos[i] >= n)
      return "qpos[" + std::to_string(i) + "] = " + std::to_string(qpos[i]) + " outside 0 .. " + std::to_string(n - 1);
  for (int64_t e = 0; e < M * m; ++e)
    if (probe[e] < -1 || probe[e] >= n)
      return "probe[" + std::to_string(e) + "] = " + std::to_string(probe[e]) + " outside -1 .. " + std::to_string(n - 1);
  return "";
}

}  // namespace

extern "C" {

int scann_ranks_host(const float* rows, int64_t n, int64_t dim, const int32_t* qpos, int64_t nq, const int32_t* probe, int32_t m,
                     int32_t threads, int32_t* rank, float* dist2) {
  if (n < 0 || n > (int64_t)0x7fffffff - 1024 || dim < 1 || (n > 0 && !rows) || threads < 0 || !bad_arguments(n, qpos, nq, probe, m, rank).empty())
    return SCANN_ERR_INVALID;
  const int64_t M = qpos ? nq : n;
  if (n == 0 || M == 0) return SCANN_OK;
  std::vector<unsigned char> elig((size_t)n);
  for (int64_t p = 0; p < n; ++p) elig[(size_t)p] = finite_row(rows + p * dim, dim);
  const std::vector<float> rows8 = transpose8(rows, n, dim);
  const Twin c{rows, rows8.data(), n, dim, elig.data(), qpos, M, probe, m, rank, dist2};
  twin_run(host_fast() ? groups_fma : groups_plain, c, M, threads);
  return SCANN_OK;
}

int scann_index_ranks(scann_handle_t* h, scann_index_t* pool, const int32_t* qpos, int64_t nq, const int32_t* probe, int32_t m, int32_t* rank,
                      float* dist2) {
  const std::string w = "scann_index_ranks: ";
  if (const int r = check_pool(h, pool, "scann_index_ranks")) return r;
  const int64_t N = pool->n;
  if (const int r = check_pool_rows(h, pool, "scann_index_ranks", (int64_t)0x7fffffff - 1024)) return r;
  const std::string why = bad_arguments(N, qpos, nq, probe, m, rank);
  if (!why.empty()) return fail(h, SCANN_ERR_INVALID, w + why);
  const int64_t M = qpos ? nq : N;
  if (N == 0 || M == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  std::vector<int32_t> all_pos;
  if (!qpos) {
    all_pos.resize((size_t)N);
    for (int64_t p = 0; p < N; ++p) all_pos[(size_t)p] = (int32_t)p;
    qpos = all_pos.data();
  }
  // the queries in slices of RANKS_SLICE; everything of the call is enqueued, then one wait.  The regions the memset clears come first
  const int64_t slice = std::min<int64_t>(RANKS_SLICE, M);
  RanksArgs all{};  // the regions of the whole call; a slice's arguments start from a copy
  all.n_total = (int32_t)N; all.chunk_rows = pool->chunk_rows; all.stride = pool->stride; all.m = m;
  unsigned char* d_elig;
  CallWs ws;
  ws.take(all.table, (size_t)slice * RANKS_MP);
  const size_t zeroed = ws.bytes();
  ws.take(all.rows, (size_t)n_chunk); ws.take(d_elig, (size_t)N);
  ws.take(all.qpos, (size_t)M); ws.take(all.probe, (size_t)M * m); ws.take(all.rank, (size_t)M * m); ws.take(all.dist2, (size_t)M * m);
  ws.take(all.qleave, (size_t)slice); ws.take(all.qmax, (size_t)slice);
  ws.take(all.thr_d, (size_t)slice * RANKS_MP); ws.take(all.thr_p, (size_t)slice * RANKS_MP); ws.take(all.slot_probe, (size_t)slice * RANKS_MP);
  HIPCHK(h, ws.alloc());
  all.elig = d_elig;
  std::vector<int32_t> rank_h((size_t)M * m);  // (the outputs change only if the call succeeds)
  std::vector<float> dist2_h(dist2 ? (size_t)M * m : 0);
  hipError_t e = ws.upload_rows(pool, n_chunk, all.rows, nullptr, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(all.qpos), qpos, (size_t)M * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(all.probe), probe, (size_t)M * m * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_sil_eligible(all.rows, (int32_t)N, pool->chunk_rows, pool->stride, d_elig, s);
  for (int64_t q0 = 0; q0 < M && e == hipSuccess; q0 += slice) {
    const int64_t nqs = std::min(slice, M - q0);
    RanksArgs k = all;
    k.qpos += q0; k.probe += q0 * m; k.rank += q0 * m; k.dist2 += q0 * m;
    k.nq = (int32_t)nqs;
    peaks_geometry(N, nqs, &k.rows_per_range, &k.n_range);
    if (k.rows_per_range > RANKS_RANGE_ROWS) {  // (a full slice against 262144 rows or more: more ranges than the geometry asks for)
      k.rows_per_range = RANKS_RANGE_ROWS;
      k.n_range = (int32_t)((N + RANKS_RANGE_ROWS - 1) / RANKS_RANGE_ROWS);
    }
    e = hipMemsetAsync(all.table, 0, zeroed, s);
    if (e == hipSuccess) e = launch_ranks_prepare(k, s);
    if (e == hipSuccess) e = launch_ranks_tiles(k, s);
    if (e == hipSuccess) e = launch_ranks_finish(k, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rank_h.data(), all.rank, (size_t)M * m * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && dist2) e = hipMemcpyAsync(dist2_h.data(), all.dist2, (size_t)M * m * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  std::copy(rank_h.begin(), rank_h.end(), rank);
  if (dist2) std::copy(dist2_h.begin(), dist2_h.end(), dist2);
  return SCANN_OK;
}

}  // extern "C"

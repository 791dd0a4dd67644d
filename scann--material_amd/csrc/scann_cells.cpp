// An index's partition into cells and the search that skips cells out of reach, the host half (include/scann_hip.h:
// scann_index_partition): the layout of a partition (shared by the device build and the host twin scann_cells_host), the build around
// scann_index_select and scann_index_kmeans, the read-back, the bound as a C function and the pruned route of scann::search().
#include "scann_cells.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "scann_call.h"
#include "scann_runtime.h"
#include "scann_search.h"

using namespace scann;

static_assert(CELLS_MAX == SCANN_KMEANS_MAX_K, "a partition has at most as many cells as k-means has centres");

namespace scann {

void cells_layout(const int32_t* labels, const float* dist2, int64_t n, int32_t C, CellLayout& out) {
  std::vector<int32_t> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  auto cell_of = [&](int32_t p) { return labels[p] < 0 ? C : labels[p]; };
  sort_by_cell(order.data(), order.data() + n, C, cell_of, dist2);
  out.C = C;
  out.perm.clear(); out.lo.clear(); out.hi.clear();
  out.first_tile.assign((size_t)C + 2, 0);
  size_t at = 0;
  for (int32_t c = 0; c <= C; ++c) {  // c == C: the loose segment
    out.first_tile[(size_t)c] = (int32_t)(out.perm.size() / TILE_TR);
    size_t end = at;
    while (end < (size_t)n && cell_of(order[end]) == c) ++end;
    for (size_t t0 = at; t0 < end; t0 += TILE_TR) {
      const size_t t1 = std::min(end, t0 + TILE_TR);
      for (size_t i = t0; i < t0 + TILE_TR; ++i) out.perm.push_back(i < t1 ? order[i] : -1);
      out.lo.push_back(c < C ? dist2[order[t0]] : 0.f);
      out.hi.push_back(c < C ? dist2[order[t1 - 1]] : __builtin_inff());
    }
    at = end;
  }
  out.first_tile[(size_t)C + 1] = (int32_t)(out.perm.size() / TILE_TR);
}

void cells_drop(scann_index* ix) {
  CellPart* p = ix->part;
  if (!p) return;
  for (char* c : p->chunks) cached_free(c);
  cached_free(p->meta);
  delete p;
  ix->part = nullptr;
}

}  // namespace scann

namespace {

// info [4]: cells in use, tiles, pad entries, rows of the largest cell
void layout_info(const CellLayout& lay, const int32_t* labels, int64_t n, int64_t* info) {
  if (!info) return;
  std::vector<int64_t> size((size_t)lay.C + 1, 0);
  for (int64_t p = 0; p < n; ++p)
    if (labels[p] >= 0) ++size[(size_t)labels[p]];
  info[0] = lay.C;
  info[1] = (int64_t)lay.lo.size();
  info[2] = (int64_t)lay.perm.size() - n;
  info[3] = *std::max_element(size.begin(), size.end());
}

void layout_out(const CellLayout& lay, const float* centres_h, int64_t dim, float* centres, int32_t* perm, int32_t* first_tile, float* lo, float* hi) {
  if (centres) std::copy(centres_h, centres_h + (size_t)lay.C * dim, centres);
  if (perm) std::copy(lay.perm.begin(), lay.perm.end(), perm);
  if (first_tile) std::copy(lay.first_tile.begin(), lay.first_tile.end(), first_tile);
  if (lo) std::copy(lay.lo.begin(), lay.lo.end(), lo);
  if (hi) std::copy(lay.hi.begin(), lay.hi.end(), hi);
}

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// the share of a pass's (group, tile) pairs above which the full kernel answers it at this k; +inf: never
double fallback_share(int k, int tiles) {
  if (k > (tiles >= CELL_FALLBACK_BIG ? CELL_FALLBACK_K : CELL_FALLBACK_K_SMALL)) return __builtin_inf();
  const char* v = std::getenv("SCANN_CELLS_FALLBACK");
  if (!v || !*v) return CELL_FALLBACK_SHARE;
  if (!std::strcmp(v, "off")) return __builtin_inf();
  char* end = nullptr;
  const double x = std::strtod(v, &end);
  return end != v && x >= 0.0 ? x : CELL_FALLBACK_SHARE;
}

// rank [C]: the place of every cell on a walk through the centres that starts at cell 0 and always goes on to the nearest centre not
// yet seen (the lower index among equals).  Cell numbers come from farthest-point picks, so neighbours in number lie far apart; queries
// ordered by the rank of their nearest cell put neighbouring cells into one group of 128.  Only the order of the queries depends on it.
void cells_walk(const float* centres, int32_t C, int32_t dim, std::vector<int32_t>& rank) {
  rank.assign((size_t)C, 0);
  std::vector<char> seen((size_t)C, 0);
  std::vector<float> d((size_t)C);
  for (int32_t at = 0, i = 0; i < C; ++i) {
    rank[(size_t)at] = i;
    seen[(size_t)at] = 1;
    dist2_to_rows(centres + (size_t)at * dim, centres, C, dim, d.data());
    int32_t next = -1;
    for (int32_t c = 0; c < C; ++c)
      if (!seen[(size_t)c] && (next < 0 || d[(size_t)c] < d[(size_t)next])) next = c;
    if (next < 0) break;
    at = next;
  }
}

}  // namespace

int scann::cells_search(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2,
                        int64_t* ids, int32_t* atoms, int32_t* pos, float* dev_d) {
  const CellPart& P = *ix->part;
  const int T = P.n_tile, C = P.lay.C;
  const int64_t g = std::min<int64_t>(nq, 1024);
  const int G = (int)((g + TILE_TQ - 1) / TILE_TQ);
  const int W = std::max(1, std::min(CELL_LISTS, T));
  const int64_t full_tiles = SearchStats::full_tiles(ix);
  CellSearchArgs a = cells_args(P);
  a.k = k; a.n_list = W;
  CallWs ws;
  float *out_d, *tau_d;
  int32_t *out_p, *tau_p, *d_qperm;
  ws.take(a.D, (size_t)g * std::max(C, 1)); ws.take(a.key_cell, (size_t)g); ws.take(a.key_d, (size_t)g); ws.take(d_qperm, (size_t)G * TILE_TQ);
  ws.take(a.seed_flag, (size_t)G * T); ws.take(a.list, (size_t)2 * G * T); ws.take(a.count, (size_t)2 * G);
  ws.take(tau_d, (size_t)g * k); ws.take(tau_p, (size_t)g * k); ws.take(out_d, (size_t)g * k); ws.take(out_p, (size_t)g * k);
  ws.take(a.part_d, (size_t)g * 2 * W * k); ws.take(a.part_p, (size_t)g * 2 * W * k);
  HIPCHK(h, ws.alloc());
  a.qperm = d_qperm; a.tau = tau_d;
  std::vector<int32_t> pos_h(dev_d ? 0 : (size_t)g * k), count((size_t)2 * G);
  PassOrder order;
  SearchStats st;
  const double share = fallback_share(k, T);
  hipError_t e = hipSuccess;
  for (int64_t q0 = 0; q0 < nq && e == hipSuccess; q0 += g) {
    const int m = (int)std::min<int64_t>(g, nq - q0), n_group = (m + TILE_TQ - 1) / TILE_TQ;
    a.q = dq + (size_t)q0 * P.stride; a.qid = dqid ? dqid + q0 : nullptr; a.nq = m; a.n_group = n_group;
    e = cells_pass_order(a, P.cell_rank, order, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.seed_flag, 0, (size_t)n_group * T, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.part_p, 0xff, (size_t)m * 2 * W * k * 4, s);  // position -1: a list that has ended
    if (e == hipSuccess) e = launch_cells_plan(a, 0, s);
    if (e == hipSuccess) e = launch_cells_list(a, 0, s);
    if (e == hipSuccess) e = launch_knn_merge(a.part_d, a.part_p, m, 2 * W, k, tau_d, tau_p, s);
    if (e == hipSuccess) e = launch_cells_plan(a, 1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(count.data(), a.count, (size_t)2 * n_group * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the plan decides the route of the pass)
    if (e != hipSuccess) break;
    int64_t seeds = 0, kept = 0;
    for (int i = 0; i < n_group; ++i) seeds += count[(size_t)i], kept += count[(size_t)i] + count[(size_t)n_group + i];
    if ((double)kept > share * (double)n_group * (double)T) {
      // the plan keeps too much: the full kernel answers this pass (its seeds were visited, and count as that)
      const size_t o = (size_t)q0 * k;
      if (const int r = search_full(h, ix, a.q, a.qid, m, k, s, dev_d ? nullptr : dist2 + o, ids ? ids + o : nullptr, atoms ? atoms + o : nullptr,
                                    pos ? pos + o : nullptr, dev_d ? dev_d + o : nullptr)) {
        ws.release();
        return r;
      }
      st.pass(n_group, full_tiles, seeds, seeds + (int64_t)n_group * full_tiles);
      continue;
    }
    st.pass(n_group, full_tiles, seeds, kept);
    e = launch_cells_list(a, 1, s);
    if (e == hipSuccess) e = launch_knn_merge(a.part_d, a.part_p, m, 2 * W, k, dev_d ? dev_d + (size_t)q0 * k : out_d, out_p, s);
    if (e == hipSuccess && !dev_d) e = hipMemcpyAsync(dist2 + (size_t)q0 * k, out_d, (size_t)m * k * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !dev_d) e = hipMemcpyAsync(pos_h.data(), out_p, (size_t)m * k * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) break;
    const size_t o = (size_t)q0 * k;
    if (!dev_d) name_positions(ix, pos_h.data(), (size_t)m * k, pos ? pos + o : nullptr, ids ? ids + o : nullptr, atoms ? atoms + o : nullptr);
  }
  if (e != hipSuccess) (void)hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  st.write(ix);
  return SCANN_OK;
}

extern "C" {

double scann_cell_bound(float D, float lo, float hi) { return cell_bound(D, lo, hi); }

int64_t scann_cells_capacity(int64_t n, int32_t cells) { return n < 0 || cells < 0 ? SCANN_ERR_INVALID : n / TILE_TR + cells + 1; }

int scann_cells_host(const float* rows, int64_t n, int64_t dim, int32_t cells, int32_t max_iter, int64_t* info, float* centres, int32_t* perm,
                     int32_t* first_tile, float* lo, float* hi) {
  if (n < 1 || n > (int64_t)0x7fffffff || dim < 1 || !rows || cells < 1 || cells > SCANN_KMEANS_MAX_K || max_iter < 0) return SCANN_ERR_INVALID;
  const int64_t want = std::min<int64_t>(cells, n);
  std::vector<int32_t> picks((size_t)want), labels((size_t)n, -1);
  std::vector<float> d2((size_t)n, __builtin_inff());
  const int64_t C = scann_kcenter_host(rows, n, nullptr, 0, dim, want, 0.f, picks.data(), nullptr);
  if (C < 0) return (int)C;
  std::vector<float> init((size_t)C * dim), cen((size_t)C * dim);
  if (C > 0) {
    for (int64_t c = 0; c < C; ++c) std::copy(rows + (int64_t)picks[(size_t)c] * dim, rows + ((int64_t)picks[(size_t)c] + 1) * dim, init.begin() + c * dim);
    const int64_t r = scann_kmeans_host(rows, n, dim, (int32_t)C, init.data(), max_iter, 0, labels.data(), d2.data(), cen.data(), nullptr, nullptr);
    if (r < 0) return (int)r;
  }
  CellLayout lay;
  cells_layout(labels.data(), d2.data(), n, (int32_t)C, lay);
  layout_info(lay, labels.data(), n, info);
  layout_out(lay, cen.data(), dim, centres, perm, first_tile, lo, hi);
  return SCANN_OK;
}

int scann_index_partition(scann_handle_t* h, scann_index_t* ix, int32_t cells, int32_t max_iter, int64_t* info) {
  if (const int r = check_index(h, ix, "scann_index_partition")) return r;
  if (cells < 0 || cells > SCANN_KMEANS_MAX_K)
    return fail(h, SCANN_ERR_INVALID, "scann_index_partition: cells " + std::to_string(cells) + " outside 0 .. " + std::to_string(SCANN_KMEANS_MAX_K));
  if (max_iter < 0) return fail(h, SCANN_ERR_INVALID, "scann_index_partition: max_iter " + std::to_string(max_iter) + " is negative");
  HIPCHK(h, hipSetDevice(h->device));
  cells_drop(ix);  // (every call is synchronous: nothing reads the copy now)
  if (info) std::fill(info, info + 4, 0);
  const int64_t N = ix->n;
  if (cells == 0 || N == 0) return SCANN_OK;
  if (const int r = check_pool_rows(h, ix, "scann_index_partition", (int64_t)0x7fffffff - (int64_t)TILE_TR * (SCANN_KMEANS_MAX_K + 2))) return r;
  const int64_t want = std::min<int64_t>(cells, N);
  std::vector<int32_t> picks((size_t)want), labels((size_t)N, -1);
  std::vector<float> d2((size_t)N, __builtin_inff());
  const int64_t C = scann_index_select(h, ix, nullptr, want, 0.f, picks.data(), nullptr, nullptr, nullptr);
  if (C < 0) return (int)C;
  CellPart* P = new CellPart();
  P->cells_arg = cells; P->max_iter = max_iter; P->dim = ix->dim; P->stride = ix->stride; P->chunk_rows = ix->chunk_rows;
  P->centres.assign((size_t)C * ix->dim, 0.f);
  if (C > 0) {
    const int64_t r = scann_index_kmeans(h, ix, (int32_t)C, nullptr, picks.data(), max_iter, 0, labels.data(), d2.data(), P->centres.data(), nullptr, nullptr);
    if (r < 0) {
      delete P;
      return (int)r;
    }
  }
  cells_layout(labels.data(), d2.data(), N, (int32_t)C, P->lay);
  cells_walk(P->centres.data(), (int32_t)C, ix->dim, P->cell_rank);
  const CellLayout& lay = P->lay;
  const int T = (int)lay.lo.size();
  P->n_tile = T;
  P->n_cell_tile = lay.first_tile[(size_t)C];
  const int64_t n_perm = (int64_t)T * TILE_TR;
  const int n_chunk = (int)((n_perm + P->chunk_rows - 1) / P->chunk_rows), n_src = (int)((N + ix->chunk_rows - 1) / ix->chunk_rows);
  hipStream_t s = h->streams[0];
  ix->part = P;  // (from here on cells_drop frees what has been allocated)
  hipError_t e = hipSuccess;
  for (int c = 0; c < n_chunk && e == hipSuccess; ++c) {
    char* p = nullptr;
    e = cached_malloc((void**)&p, P->chunk_bytes());
    if (e == hipSuccess) P->chunks.push_back(p);
  }
  // the meta block: centres, the tiles' cells, the cells' first tiles, lo, hi, their roots, the full flags, the three chunk tables
  size_t at = 0;
  auto region = [&](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
  const size_t o_cen = region((size_t)std::max<int64_t>(C, 1) * P->stride * 4), o_tc = region((size_t)T * 4), o_ft = region(((size_t)C + 2) * 4),
               o_lo = region((size_t)T * 4), o_hi = region((size_t)T * 4), o_rlo = region((size_t)T * 8), o_rhi = region((size_t)T * 8),
               o_full = region((size_t)T), o_tab = region((size_t)n_chunk * 24);
  if (e == hipSuccess) e = cached_malloc((void**)&P->meta, at);
  if (e != hipSuccess) {
    cells_drop(ix);
    HIPCHK(h, e);
  }
  P->d_centres = reinterpret_cast<float*>(P->meta + o_cen); P->d_tile_cell = reinterpret_cast<int32_t*>(P->meta + o_tc);
  P->d_first_tile = reinterpret_cast<int32_t*>(P->meta + o_ft); P->d_lo = reinterpret_cast<float*>(P->meta + o_lo);
  P->d_hi = reinterpret_cast<float*>(P->meta + o_hi); P->d_rlo = reinterpret_cast<double*>(P->meta + o_rlo);
  P->d_rhi = reinterpret_cast<double*>(P->meta + o_rhi); P->d_full = reinterpret_cast<unsigned char*>(P->meta + o_full);
  void** d_tab = reinterpret_cast<void**>(P->meta + o_tab);
  P->d_rows = reinterpret_cast<const float* const*>(d_tab); P->d_ids = reinterpret_cast<const int64_t* const*>(d_tab + n_chunk);
  P->d_pos = reinterpret_cast<const int32_t* const*>(d_tab + 2 * n_chunk);
  std::vector<void*> tab((size_t)3 * n_chunk);
  for (int c = 0; c < n_chunk; ++c) tab[(size_t)c] = P->rows_of((size_t)c), tab[(size_t)n_chunk + c] = P->ids_of((size_t)c), tab[(size_t)2 * n_chunk + c] = P->pos_of((size_t)c);
  std::vector<int32_t> tile_cell((size_t)T, -1);
  std::vector<unsigned char> full((size_t)T, 0);
  for (int32_t c = 0; c < C; ++c)
    for (int t = lay.first_tile[(size_t)c]; t < lay.first_tile[(size_t)c + 1]; ++t) tile_cell[(size_t)t] = c;
  for (int t = 0; t < T; ++t) full[(size_t)t] = lay.perm[(size_t)t * TILE_TR + TILE_TR - 1] >= 0;
  CallWs ws;
  CellGatherArgs ga{};
  int32_t* d_perm;
  ws.take(d_perm, (size_t)n_perm); ws.take(ga.src_rows, (size_t)n_src); ws.take(ga.src_ids, (size_t)n_src);
  e = ws.alloc();
  ga.dst_rows = reinterpret_cast<float* const*>(d_tab); ga.dst_ids = reinterpret_cast<int64_t* const*>(d_tab + n_chunk);
  ga.dst_pos = reinterpret_cast<int32_t* const*>(d_tab + 2 * n_chunk);
  ga.perm = d_perm; ga.n_perm = (int32_t)n_perm; ga.chunk_rows = P->chunk_rows; ga.stride = P->stride;
  if (e == hipSuccess) e = hipMemsetAsync(P->d_centres, 0, (size_t)std::max<int64_t>(C, 1) * P->stride * 4, s);  // (the padding columns are zero)
  if (e == hipSuccess && C > 0)
    e = hipMemcpy2DAsync(P->d_centres, (size_t)P->stride * 4, P->centres.data(), (size_t)P->dim * 4, (size_t)P->dim * 4, (size_t)C, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(P->d_tile_cell, tile_cell.data(), (size_t)T * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(P->d_first_tile, lay.first_tile.data(), ((size_t)C + 2) * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(P->d_lo, lay.lo.data(), (size_t)T * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(P->d_hi, lay.hi.data(), (size_t)T * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(P->d_full, full.data(), (size_t)T, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tab, tab.data(), (size_t)3 * n_chunk * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_perm, lay.perm.data(), (size_t)n_perm * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = ws.upload_rows(ix, n_src, ga.src_rows, ga.src_ids, s);
  if (e == hipSuccess) e = launch_cells_gather(ga, s);
  if (e == hipSuccess) e = launch_cells_roots(P->d_lo, P->d_hi, P->d_rlo, P->d_rhi, T, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  if (e != hipSuccess || e_sync != hipSuccess) cells_drop(ix);
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  layout_info(lay, labels.data(), N, P->info);
  if (info) std::copy(P->info, P->info + 4, info);
  return SCANN_OK;
}

int scann_index_cells_read(scann_handle_t* h, scann_index_t* ix, int64_t* info, float* centres, int32_t* perm, int32_t* first_tile, float* lo,
                           float* hi) {
  if (const int r = check_index(h, ix, "scann_index_cells_read")) return r;
  if (info) std::fill(info, info + 4, 0);
  if (!ix->part) return SCANN_OK;  // no partition: info says 0 cells, 0 tiles
  const CellPart& P = *ix->part;
  if (info) std::copy(P.info, P.info + 4, info);
  // the permutation as the device holds it: the copy's positions, read back
  if (perm) {
    HIPCHK(h, hipSetDevice(h->device));
    for (size_t c = 0; c < P.chunks.size(); ++c) {
      const int64_t r0 = (int64_t)c * P.chunk_rows, m = std::min<int64_t>(P.chunk_rows, (int64_t)P.lay.perm.size() - r0);
      HIPCHK(h, hipMemcpy(perm + r0, P.pos_of(c), (size_t)m * 4, hipMemcpyDeviceToHost));
    }
  }
  layout_out(P.lay, P.centres.data(), P.dim, centres, nullptr, first_tile, lo, hi);
  return SCANN_OK;
}

int scann_index_partition_args(const scann_index_t* ix, int32_t* cells, int32_t* max_iter) {
  if (!ix) return SCANN_ERR_INVALID;
  if (cells) *cells = ix->part ? ix->part->cells_arg : 0;
  if (max_iter) *max_iter = ix->part ? ix->part->max_iter : 0;
  return SCANN_OK;
}

int scann_index_search_stats(const scann_index_t* ix, int64_t* out) {
  if (!ix || !out) return SCANN_ERR_INVALID;
  std::copy(ix->stats, ix->stats + 4, out);
  return SCANN_OK;
}

int scann_index_query_rows(scann_handle_t* h, scann_index_t* ix, int64_t first, int64_t n, int32_t k, float* dist2, int64_t* ids, int32_t* atoms,
                           int32_t* pos) {
  if (const int r = check_index(h, ix, "scann_index_query_rows")) return r;
  if (const int r = check_k(h, k, "scann_index_query_rows")) return r;
  if (first < 0 || n <= 0 || first + n > ix->n)
    return fail(h, SCANN_ERR_INVALID, "scann_index_query_rows: rows " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " + std::to_string(ix->n));
  if (n > (int64_t)0x7fffffff / SCANN_KNN_MAX_K) return fail(h, SCANN_ERR_INVALID, "scann_index_query_rows: too many queries in one call");
  if (!dist2) return fail(h, SCANN_ERR_INVALID, "scann_index_query_rows: dist2 is null");
  HIPCHK(h, hipSetDevice(h->device));
  SearchStats st;
  // the queries where they lie, chunk by chunk: rows of the index are padded as queries are
  if (const int r = row_runs(ix, first, n, [&](size_t c, int64_t r0, int64_t m, int64_t done) {
        const int r = search(h, ix, ix->rows_of(c) + (size_t)r0 * ix->stride, nullptr, m, k, h->streams[0], dist2 + (size_t)done * k,
                             ids ? ids + (size_t)done * k : nullptr, atoms ? atoms + (size_t)done * k : nullptr, pos ? pos + (size_t)done * k : nullptr);
        st.add(ix->stats);
        return r;
      }))
    return r;
  st.write(ix);
  return SCANN_OK;
}

}  // extern "C"

// What the searches over a latent-space index share on the host (header only): the walk over a window of rows chunk by chunk
// (row_runs), the staging of query rows with their ids (staged_queries) and of a batch's rows at a level (staged_batch_queries), the
// partition's fields of CellSearchArgs (cells_args), the order of a partitioned pass's queries (sort_by_cell, query_order,
// cells_pass_order), the naming of positions (name_positions) and what scann_index_search_stats reports (SearchStats).
// scann_knn.cpp (every row), scann_cells.cpp (the cells in reach) and scann_within.cpp (the radius search) are written in these pieces;
// a new search over the index is, too.  The pure pieces call nothing, so the stand-alone check programs reach them without a device.
#pragma once
#include <algorithm>
#include <numeric>

#include "scann_call.h"
#include "scann_cells.h"

namespace scann {

// f(chunk, first row in the chunk, rows, rows done so far) for the rows [first, first + n) of ix, chunk by chunk; f returns a status
// and the first that is not 0 ends the walk and is returned
template <class F>
int row_runs(const scann_index* ix, int64_t first, int64_t n, F f) {
  for (int64_t done = 0; done < n;) {
    const int64_t at = first + done, r0 = at % ix->chunk_rows, m = std::min<int64_t>(n - done, ix->chunk_rows - r0);
    if (const int r = f((size_t)(at / ix->chunk_rows), r0, m, done)) return r;
    done += m;
  }
  return SCANN_OK;
}

// nq queries of the index's width at q -- host rows (kind = hipMemcpyHostToDevice) or device rows -- and their ids (host [nq], or null)
// staged in one block of the cache: the rows padded to the stride, then the ids.  Device rows whose width is the stride stay where they
// lie.  body(rows, ids on the device or null) runs the search on stream s, synchronously, and returns its status
template <class F>
int staged_queries(scann_handle* h, const scann_index* ix, const float* q, hipMemcpyKind kind, const int64_t* qid, int64_t nq, hipStream_t s, F body) {
  CallWs ws;
  RowStage st;
  int64_t* d_qid;
  st.take(ws, nq, ix->dim, ix->dim, ix->stride, kind);
  ws.take(d_qid, qid ? (size_t)nq : 0);
  HIPCHK(h, ws.alloc());
  hipError_t e = st.stage_rows(q, s);
  if (e == hipSuccess && qid) e = hipMemcpyAsync(d_qid, qid, (size_t)nq * 8, hipMemcpyHostToDevice, s);
  int r = SCANN_OK;
  if (e == hipSuccess) r = body(st.rows(q), qid ? d_qid : nullptr);
  else (void)hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  return r;
}

// What scann_index_query_batch and scann_index_within_batch do once their arguments have passed: the forward of the batch with the
// level's output, then the level's rows staged as the queries where the forward left them, under the structures' ids (query_ids [n_struct]
// or null), on the stream of the batch's slot.  who: the entry point's name
template <class F>
int staged_batch_queries(scann_handle* h, const scann_index* ix, scann_dbatch* db, int32_t level, const int64_t* query_ids, float* y, float* ga,
                         const char* who, F body) {
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, std::string(who) + ": weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  const bool atom = level == SCANN_OUT_AFTER_LC;
  std::vector<int64_t> qid;
  if (query_ids)
    if (const int r = expand_ids(h, db, atom, query_ids, 0, qid, nullptr)) return r;
  return staged_queries(h, ix, atom ? db->out_z : db->out_bf, hipMemcpyDeviceToDevice, query_ids ? qid.data() : nullptr, atom ? db->n_atom : db->n_struct,
                        h->streams[db->last_slot], body);
}

// the fields of a partition; a pass adds its own: k, n_list, radius2, the queries and the workspace regions
inline CellSearchArgs cells_args(const CellPart& P) {
  CellSearchArgs a{};
  a.rows = P.d_rows; a.ids = P.d_ids; a.pos = P.d_pos; a.centres = P.d_centres; a.tile_cell = P.d_tile_cell; a.first_tile = P.d_first_tile;
  a.rlo = P.d_rlo; a.rhi = P.d_rhi; a.full = P.d_full;
  a.C = P.lay.C; a.n_tile = P.n_tile; a.n_cell_tile = P.n_cell_tile; a.chunk_rows = P.chunk_rows; a.stride = P.stride;
  return a;
}

// The order of a partition, of its rows and of the queries of a pass alike: by cell (C: none, last), within a cell by d ascending, then
// by place
template <class Cell>
void sort_by_cell(int32_t* begin, int32_t* end, int32_t C, Cell cell_of, const float* d) {
  std::sort(begin, end, [&](int32_t x, int32_t y) {
    const int32_t cx = cell_of(x), cy = cell_of(y);
    if (cx != cy) return cx < cy;
    if (cx < C && d[x] != d[y]) return d[x] < d[y];
    return x < y;
  });
}

// qperm [m rounded up to whole groups of 128]: the m queries of a pass by (place of the nearest cell on the walk through the centres,
// distance to its centre, place), those without a cell (key_cell -1) last, then -1.  A group of 128 then looks at the same cells
inline void query_order(const int32_t* key_cell, const float* key_d, const int32_t* cell_rank, int32_t C, int32_t m, int32_t* qperm) {
  std::fill(qperm + m, qperm + (m + TILE_TQ - 1) / TILE_TQ * TILE_TQ, -1);
  std::iota(qperm, qperm + m, 0);
  sort_by_cell(qperm, qperm + m, C, [&](int32_t x) { return key_cell[x] < 0 ? C : cell_rank[key_cell[x]]; }, key_d);
}

// How a pass over a partition begins, enqueued on s with one wait: the centre distances of a's queries, their nearest cells brought to
// the host, and the order of the queries into a.qperm (a workspace region).  o: the host side, which stays until the pass has been waited for
struct PassOrder {
  std::vector<int32_t> key_cell, qperm;
  std::vector<float> key_d;
};
inline hipError_t cells_pass_order(const CellSearchArgs& a, const std::vector<int32_t>& cell_rank, PassOrder& o, hipStream_t s) {
  const size_t m = (size_t)a.nq, padded = (size_t)a.n_group * TILE_TQ;
  o.key_cell.resize(m); o.key_d.resize(m); o.qperm.resize(padded);
  hipError_t e = launch_cells_centre(a, s);
  if (e == hipSuccess) e = hipMemcpyAsync(o.key_cell.data(), a.key_cell, m * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(o.key_d.data(), a.key_d, m * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  query_order(o.key_cell.data(), o.key_d.data(), cell_rank.data(), a.C, a.nq, o.qperm.data());
  return hipMemcpyAsync(writable(a.qperm), o.qperm.data(), padded * 4, hipMemcpyHostToDevice, s);
}

// n positions of ix as the calls report them: the position, the row's id, its atom; -1 for a position of -1.  Every output may be null
inline void name_positions(const scann_index* ix, const int32_t* p, size_t n, int32_t* pos, int64_t* ids, int32_t* atoms) {
  for (size_t i = 0; i < n && (pos || ids || atoms); ++i) {
    if (pos) pos[i] = p[i];
    if (ids) ids[i] = p[i] < 0 ? -1 : ix->ids[(size_t)p[i]];
    if (atoms) atoms[i] = p[i] < 0 ? -1 : ix->atoms[(size_t)p[i]];
  }
}

// What scann_index_search_stats reports of a call, summed over its passes: the (group, tile) pairs a full search of the index's own
// chunks has, the seed tiles visited, the tiles visited in all, the groups of 128 queries
struct SearchStats {
  int64_t v[4] = {0, 0, 0, 0};
  // tiles of a full search.  A chunk holds whole tiles (chunk_rows is a multiple of TILE_TR: scann_index_create), so the chunks'
  // tiles add up to the tiles of n rows
  static int64_t full_tiles(const scann_index* ix) { return (ix->n + TILE_TR - 1) / TILE_TR; }
  static int64_t groups(int64_t m) { return (m + TILE_TQ - 1) / TILE_TQ; }
  void pass(int64_t n_group, int64_t tiles, int64_t seeds, int64_t visited) { v[0] += n_group * tiles, v[1] += seeds, v[2] += visited, v[3] += n_group; }
  void add(const int64_t* stats) { for (int i = 0; i < 4; ++i) v[i] += stats[i]; }  // a search's, into those of the call it was a part of
  void write(scann_index* ix) const { std::copy(v, v + 4, ix->stats); }
};

}  // namespace scann

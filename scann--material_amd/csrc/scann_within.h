// Internal declarations of the radius search over a latent-space index (scann_within.hip, scann_within.cpp); the C ABI and the
// definition are in include/scann_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_cells.h"

namespace scann {

constexpr int64_t WITHIN_MAX_CAP = (int64_t)1 << 30;  // entries a call returns at most (SCANN_WITHIN_MAX_CAP)
constexpr int WITHIN_RANGES = 1024;                   // workgroups per group of 128 queries at most, without a partition
constexpr int WITHIN_PASS = 1 << 17;                  // queries of one launch at most, without a partition

// One launch of within_tile_kernel: the hits of `nq` queries among the entries of a table of rows stored in chunks.  Workgroup (x, g) takes
// the x-th share of the tiles of group g, 128 queries:
//   without a list   the group's tiles are first(g) .. n_entries / 64 of the table in order, first(g) = 0, or with `upper` the first tile
//                    that holds a position above the group's least query position; entry e is position e
//   with a list      the tiles list[g][0 .. count[g]) of the cell-ordered copy; entry e is position pos[e], -1: a pad entry
// Slot i of group g is query qperm[128 g + i] of the launch (qperm null: query 128 g + i; -1: none).  Query i of the launch is query
// q_base + i of the call and, self_first >= 0, the row at position self_first + i.
struct WithinArgs {
  const float* const* rows;   // [n_chunk] -> [chunk_rows][stride], the padding columns zero
  const int64_t* const* ids;  // [n_chunk] -> [chunk_rows] (read with qid only)
  const int32_t* const* pos;  // [n_chunk] -> [chunk_rows], or null: an entry is its position
  int32_t n_entries, chunk_rows, stride;
  const float* q;       // [nq][stride], padded like the rows
  const int64_t* qid;   // [nq] or null: rows with this id are skipped
  int32_t nq, n_group, q_base, self_first, upper;
  const int32_t* qperm;  // [n_group * 128] or null
  const int32_t* list;   // [n_group][n_tile] or null
  const int32_t* count;  // [n_group]
  int32_t n_tile;
  float radius2;
  // the results: exact counts, and one record per hit as long as the records fit
  uint32_t* counts;            // [queries of the call]
  unsigned long long* cursor;  // records reserved so far (a reservation past cap writes nothing and still counts)
  long long cap;
  int32_t *rec_q, *rec_p;      // [cap] query of the call, position ...
  float* rec_d;                // ... and dist2
};
hipError_t launch_within_tile(const WithinArgs& a, int n_share, hipStream_t s);

// The order of the result, established on the host: the records of a call, in any order, into their queries' segments (first [nq + 1] is
// the exclusive prefix sum of counts), each segment sorted by (dist2, position).  Keys within a query are unique, so the result is too.
// Threaded over the queries, 16 threads at most.  dist2 / pos may be null
void within_finish(const int64_t* first, int64_t nq, const int32_t* rec_q, const int32_t* rec_p, const float* rec_d, int64_t total, float* dist2,
                   int32_t* pos);

}  // namespace scann

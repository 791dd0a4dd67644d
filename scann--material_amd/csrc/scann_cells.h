// Internal declarations of an index's partition into cells and of the nearest-row search that skips cells out of reach (scann_cells.hip,
// scann_cells.cpp); the C ABI and the definition are in include/scann_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "scann_knn.h"

namespace scann {

constexpr int CELLS_MAX = 1024;  // cells of a partition at most (SCANN_KMEANS_MAX_K)

// ---- the bound (include/scann_hip.h: scann_cell_bound), one function for the device and the host ----
// a = sqrt(D), r_lo = sqrt(lo), r_hi = sqrt(hi) as doubles; ok: D and hi are finite
constexpr double CELL_EPS = 1.0 / 4096.0;                       // 2^-12
constexpr double CELL_ABS = 1.0 / 18446744073709551616.0;       // 2^-64
__host__ __device__ inline double cell_bound_roots(double a, double r_lo, double r_hi, bool ok) {
  if (!ok) return 0.0;
  const double g1 = (1.0 - CELL_EPS) * a - (1.0 + CELL_EPS) * r_hi, g2 = (1.0 - CELL_EPS) * r_lo - (1.0 + CELL_EPS) * a;
  const double g = (g1 > g2 ? g1 : g2) - CELL_ABS;
  return g > 0.0 ? (1.0 - CELL_EPS) * (g * g) : 0.0;
}
// whether an fp32 value is finite, from its bits (no library call: the same on both sides)
__host__ __device__ inline bool cell_finite(float x) { return (x - x) == 0.f; }
__host__ __device__ inline double cell_bound(float D, float lo, float hi) {
  const bool ok = cell_finite(D) && cell_finite(hi) && D >= 0.f && lo >= 0.f && hi >= 0.f;
  return ok ? cell_bound_roots(sqrt((double)D), sqrt((double)lo), sqrt((double)hi), true) : 0.0;
}

// ---- the layout of a partition, built on the host from labels and dist2 (the device build and the host twin share it) ----
struct CellLayout {
  int32_t C = 0;                    // cells
  std::vector<int32_t> perm;        // [64 * tiles] original position, -1: a pad entry
  std::vector<int32_t> first_tile;  // [C + 2]: first tile of cell c; [C]: first loose tile; [C + 1]: tiles
  std::vector<float> lo, hi;        // [tiles]
};
// labels [n] in -1 .. C - 1, dist2 [n]: rows sorted by (label, dist2 ascending, position ascending), label -1 last, every cell and the
// loose segment padded to whole tiles of 64
void cells_layout(const int32_t* labels, const float* dist2, int64_t n, int32_t C, CellLayout& out);

// ---- the partition attached to an index (scann_index::part) ----
struct CellPart {
  int32_t cells_arg = 0, max_iter = 0;  // as asked for
  int32_t dim = 0, stride = 0, chunk_rows = 0;
  CellLayout lay;
  std::vector<float> centres;   // host [C * dim]
  int64_t info[4] = {0, 0, 0, 0};  // cells in use, tiles, pad entries, rows of the largest cell (scann_index_partition's info)
  std::vector<int32_t> cell_rank;  // host [C]: the cell's place on a nearest-neighbour walk through the centres (the order of the queries)
  int32_t n_tile = 0, n_cell_tile = 0;  // tiles in all; tiles that belong to a cell (the loose ones lie behind them)
  // device: chunks of the handle's cache, each rows [chunk_rows][stride] fp32, ids [chunk_rows] int64, pos [chunk_rows] int32
  std::vector<char*> chunks;
  // device: one block (meta) that holds everything below
  char* meta = nullptr;
  float* d_centres = nullptr;
  int32_t* d_tile_cell = nullptr;   // [n_tile] cell of a tile, -1: loose
  int32_t* d_first_tile = nullptr;  // [C + 2]
  float *d_lo = nullptr, *d_hi = nullptr;  // [n_tile]
  double *d_rlo = nullptr, *d_rhi = nullptr;  // [n_tile] their square roots
  unsigned char* d_full = nullptr;  // [n_tile] 1: 64 real rows
  const float* const* d_rows = nullptr;  // [n_chunk] chunk tables
  const int64_t* const* d_ids = nullptr;
  const int32_t* const* d_pos = nullptr;
  float* rows_of(size_t c) const { return reinterpret_cast<float*>(chunks[c]); }
  int64_t* ids_of(size_t c) const { return reinterpret_cast<int64_t*>(chunks[c] + (size_t)chunk_rows * stride * 4); }
  int32_t* pos_of(size_t c) const { return reinterpret_cast<int32_t*>(chunks[c] + (size_t)chunk_rows * stride * 4 + (size_t)chunk_rows * 8); }
  size_t chunk_bytes() const { return (size_t)chunk_rows * stride * 4 + (size_t)chunk_rows * 12; }
};

// the partition of ix, freed (its blocks go back to the cache); the caller has waited for the device
void cells_drop(scann_index* ix);
// scann::search() on a partitioned index: the same arguments, the same answer in every byte
int cells_search(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2, int64_t* ids,
                 int32_t* atoms, int32_t* pos, float* dev_d);

// The fall-back of cells_search (measured, profiles/cells_rate.txt): a pass of up to 1,024 queries whose plan keeps more than
// CELL_FALLBACK_SHARE of its (group, tile) pairs is answered by the full kernel if k <= 3, or k <= 7 on a copy of at least
// CELL_FALLBACK_BIG tiles (about a million rows).  Where the list route visits every tile it loses to the full kernel up to k = 7 and
// wins from k = 8 on, because its second pass drops a distance above tau_q after one compare; but falling back costs the plan and the
// seed pass, which a small index gets back only at the smallest k (131,072 rows: k = 1 3.18 -> 2.69 ms, k = 5 3.25 -> 3.49 ms;
// 2.4 M rows: k = 5 45.5 -> 39.4 ms).  No size between 131,072 and 2.4 M rows was measured; the limit lies in that gap.
// Environment SCANN_CELLS_FALLBACK: another share, or "off" (tools/cells_rate.py measures the route itself that way).
constexpr double CELL_FALLBACK_SHARE = 0.5;
constexpr int CELL_FALLBACK_K_SMALL = 3, CELL_FALLBACK_K = 7;
constexpr int CELL_FALLBACK_BIG = 16384;

// ---- kernels (scann_cells.hip) ----
constexpr int CELL_LISTS = 128;  // at most as many workgroups of cells_list_kernel per group of 128 queries and pass

// the permuted copy: entry e of the cell order <- row perm[e] of the index (pad: a zero row, id 0, position -1)
struct CellGatherArgs {
  const float* const* src_rows;  // the index's chunks
  const int64_t* const* src_ids;
  float* const* dst_rows;
  int64_t* const* dst_ids;
  int32_t* const* dst_pos;
  const int32_t* perm;  // [n_perm]
  int32_t n_perm, chunk_rows, stride;
};
hipError_t launch_cells_gather(const CellGatherArgs& a, hipStream_t s);
// r_lo, r_hi [n] = sqrt of lo, hi in fp64
hipError_t launch_cells_roots(const float* lo, const float* hi, double* rlo, double* rhi, int n, hipStream_t s);

struct CellSearchArgs {
  // the partition
  const float* const* rows;
  const int64_t* const* ids;
  const int32_t* const* pos;
  const float* centres;        // [C][stride]
  const int32_t* tile_cell;    // [n_tile]
  const int32_t* first_tile;   // [C + 2]
  const double *rlo, *rhi;     // [n_tile]
  const unsigned char* full;   // [n_tile]
  int32_t C, n_tile, n_cell_tile, chunk_rows, stride;
  // the pass: nq queries, slot i of the cell order of the queries is query qperm[i]
  const float* q;        // [nq][stride]
  const int64_t* qid;    // [nq] or null
  int32_t nq, k, n_group;
  float* D;              // [nq][C]  dist2(query, centre)
  int32_t* key_cell;     // [nq] nearest centre (-1: none) ...
  float* key_d;          // ... and its distance
  const int32_t* qperm;  // [n_group * 128], -1: no query
  unsigned char* seed_flag;  // [n_group][n_tile], cleared by the caller
  int32_t* list;         // [2][n_group][n_tile]: the seeds, then the survivors
  int32_t* count;        // [2][n_group]
  const float* tau;      // [nq][k] the seed pass's merged lists (tau = the last place)
  float radius2;         // plan pass 2 (a radius search): the threshold of every query
  float* part_d;         // [nq][2 * n_list][k]
  int32_t* part_p;
  int32_t n_list;
};
size_t cells_list_lds_bytes(int k);
hipError_t launch_cells_centre(const CellSearchArgs& a, hipStream_t s);   // D, key_cell, key_d
hipError_t launch_cells_plan(const CellSearchArgs& a, int pass, hipStream_t s);  // pass 0: seeds; 1: survivors; 2: a radius search's survivors
hipError_t launch_cells_list(const CellSearchArgs& a, int pass, hipStream_t s);

}  // namespace scann

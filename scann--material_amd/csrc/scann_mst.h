// Internal declarations of the exact minimum spanning tree of a latent-space index (scann_mst.hip; the host half and the twin are in
// scann_mst.cpp); the C ABI is include/scann_hip.h: scann_index_mst, scann_mst_host.  The weight, the edge order and the per-row rule
// below are the one place that forms them: the twin and the kernels include it.
//
// Why Boruvka rounds give the unique tree.  The edge order (w, min, max) is a strict total order, so the minimum spanning tree is unique.
// In a round every component picks its first outgoing edge; by the cut property that edge is in the tree.  The picked edges close no
// cycle: along a cycle of components every pick would have to come strictly before the next one in the order, all the way round.
//
// The per-row rule.  For a fixed row q the edge order restricted to the edges at q is the order (w, r) of the other end r: the rows
// r < q give edges (w, r, q), the rows r > q edges (w, q, r), and for equal w every edge of the first kind comes before every one of the
// second (r < q = min), within the first kind min = r ascends and within the second max = r ascends.  So a walk over the positions in
// ascending order that replaces the incumbent only on a strictly smaller w finds the row's first edge.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_peaks.h"

namespace scann {

// w(i, j) = max(dist2(i, j), core2[i], core2[j]); none of the three is a NaN, so the max is exact and has no order
__host__ __device__ inline float mst_weight(float dist2, float ci, float cj) {
  float w = dist2;
  if (ci > w) w = ci;
  if (cj > w) w = cj;
  return w;
}

// edge (w1, lo1, hi1) comes before edge (w2, lo2, hi2): the edge order
__host__ __device__ inline bool mst_before(float w1, int32_t lo1, int32_t hi1, float w2, int32_t lo2, int32_t hi2) {
  return w1 < w2 || (w1 == w2 && (lo1 < lo2 || (lo1 == lo2 && hi1 < hi2)));
}

// the per-row rule: the other end (w, r) comes before the incumbent (bw, br) of the same row
__host__ __device__ inline bool mst_row_before(float w, int32_t r, float bw, int32_t br) { return w < bw || (w == bw && r < br); }

// One round's search: for every row the first row of another component under (w, position).  The tiling is that of peaks_tile_kernel
// (the tile of scann_tile.h): workgroup (x, y) takes queries [128 x, 128 x + 128) and positions [y * rows_per_range, (y + 1) * rows_per_range).
struct MstArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, stride;
  int32_t rows_per_range, n_range;
  const int32_t* comp;       // [n] the component's label of a row, -1 for a row that is not eligible
  const float* core2;        // [n] (zeros without core distances)
  float* part_w;             // [n][n_range] the range's first row of another component under (w, position) ...
  int32_t* part_p;           // ... and its position; (+inf, -1) where the range has none
  unsigned int* skipped;     // [1] or null: the tiles whose arithmetic was skipped are counted here (the rate tool)
};
// the device state of the component step, all [n] unless said otherwise
struct MstStep {
  int32_t n;
  int32_t* comp;                   // in/out
  const float* best_w;             // the merged search result of every row ...
  const int32_t* best_p;           // ... -1: none
  unsigned long long* key;         // per label: the least (bits of w) << 32 | min(q, r) of the component's rows
  int32_t* hi;                     // per label: the least max(q, r) among the rows that attain key
  int32_t* ptr[2];                 // per label: the label across the component's first edge; double-buffered for the jumps
  int32_t* edge_a;                 // [n - 1] the edges of the tree, in no order
  int32_t* edge_b;
  float* edge_w;
  int32_t* counters;               // [0] the edges so far, [1] the components after this round
};
hipError_t launch_mst_eligible(const MstArgs& a, int32_t* comp, int32_t* counters, hipStream_t s);  // comp[i] = i or -1; counters[1] = the eligible rows
hipError_t launch_mst_tile(const MstArgs& a, hipStream_t s);
// the component step behind the merged search: `jumps` pointer-jumping launches; leaves the new labels in comp and their number in counters[1]
hipError_t launch_mst_step(const MstStep& c, int jumps, hipStream_t s);

}  // namespace scann

// Internal declarations of the density-peak clustering and the kernel density of a latent-space index (scann_peaks.hip; the host half and
// the twins are in scann_peaks.cpp); the C ABI is include/scann_hip.h: scann_index_density, scann_index_peaks, scann_index_density_batch,
// scann_density_host, scann_peaks_host.  The fixed-point term below is the one place that forms it: the twins and the kernel include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scann_rbf.h"
#include "scann_tile.h"

namespace scann {

// The weight term of a pair at distance dist2: t = round-to-nearest-even(2^30 w), w = scann_rbf_weight(dist2, gamma); 0 <= t <= 2^30, and
// 0 for a NaN distance (such a pair contributes nothing).  w is 0 or a normal number, so the scaling by 2^30 is exact.
__host__ __device__ inline int32_t peaks_term(float dist2, float gamma) {
  if (dist2 != dist2) return 0;
  return (int32_t)rintf(ldexpf(rbf_weight(dist2, gamma), 30));
}

// row j with the sum sj is above row i with the sum si (the density order)
__host__ __device__ inline bool peaks_above(long long sj, int32_t j, long long si, int32_t i) { return sj > si || (sj == si && j < i); }

constexpr int PK_LANES = TILE_LANES;  // lanes of every kernel of the density, spanning-tree and silhouette passes (the tile: scann_tile.h)
constexpr int PK_BLOCKS = 4096;       // about as many workgroups per launch as this

// One launch of a tile kernel: nq queries against positions 0 .. n_total - 1 of a pool stored in chunks of `chunk_rows` rows.  Workgroup
// (x, y) takes queries [128 x, 128 x + 128) and positions [y * rows_per_range, (y + 1) * rows_per_range): ranges are cut by position, so
// the pool's chunking does not enter the result.  q null: the queries are the pool's own rows, query i the row at position i, and
// position i is left out of query i's sum (the self-join).
struct PeaksArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, stride;
  const float* q;            // [nq][stride], padded like the rows, or null
  const int32_t* skip;       // [nq] or null: position skip[i] >= 0 is left out of query i's sum (density with q only)
  int32_t nq, rows_per_range, n_range;
  float gamma;
  unsigned long long* sums;  // [nq] int64.  density: cleared before the launch, every workgroup adds its range's part
                             //              parent: the finished sums of the pool's rows, read
  float* part_d;             // parent: [nq][n_range] the range's first row above the query under (dist2, position) ...
  int32_t* part_p;           // ... and its position; (+inf, -1) where the range has none
};
// how a pass over n rows by nq queries is cut into ranges (rows_per_range a multiple of 64)
void peaks_geometry(int64_t n, int64_t nq, int32_t* rows_per_range, int32_t* n_range);
hipError_t launch_peaks_density(const PeaksArgs& a, hipStream_t s);
// sums[i] = -1 for every query with a non-finite component (after launch_peaks_density, on the same stream)
hipError_t launch_peaks_finish(const PeaksArgs& a, hipStream_t s);
hipError_t launch_peaks_parent(const PeaksArgs& a, hipStream_t s);

}  // namespace scann

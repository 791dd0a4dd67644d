// Internal declarations of the k-means clustering over a latent-space index (scann_kmeans.hip; the host half is in scann_kmeans.cpp); the
// C ABI is include/scann_hip.h: scann_index_kmeans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_tile.h"

namespace scann {

constexpr int KM_LANES = TILE_LANES;      // lanes of every workgroup
constexpr int KM_TP = TILE_TQ;      // pool rows of a tile of kmeans_assign_kernel
constexpr int KM_TC = TILE_TR;      // centres per block of that kernel: a lane owns 8 rows x 4 centres
constexpr int KM_SLAB = TILE_SLAB;      // columns per LDS slab
constexpr int KM_MAX_GROUPS = 768;  // workgroups of an assignment at most (three fit a CU at its 138 registers): the tiles are dealt evenly, workgroup g walks tiles g, g + G, ...
constexpr int KM_ROUNDS = 256;      // rounds whose `changed` counters the state holds: the host enqueues at most this many before it waits
constexpr int KM_SUM_LDS = 64 << 10;  // bytes of int64 sums a workgroup of kmeans_sum_kernel keeps in LDS: k x cols x 8
constexpr int KM_SUM_GROUPS = 1024;   // about as many workgroups in that kernel

// What the rounds hand to each other, in device memory (zeroed before the first launch).  The round number t is a launch argument:
// nothing here is written by a launch that another workgroup of the same launch reads with a different outcome.
struct KmState {
  int32_t done;       // the loop has ended (or an initial position named an ineligible row): every later launch returns at once
  int32_t n_iter;     // t of the last assignment
  int32_t converged;  // changed_t <= stop_changed
  int32_t bad_init;   // k - the first place of init_pos that names an ineligible row (0: none)
  uint32_t changed[KM_ROUNDS];  // [t % KM_ROUNDS] rows whose label changed in round t
};

// One clustering.  Tile i holds rows [128 (i % tiles_per_chunk), + 128) of chunk i / tiles_per_chunk; position = chunk * chunk_rows + row.
struct KmArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, n_chunk, stride, dim;
  int32_t tiles_per_chunk, n_tile;
  int32_t k;
  float* centres;            // [k][stride], columns dim .. stride-1 zero
  uint8_t* elig;             // [n_total] 1: every component finite
  int32_t* labels;           // [n_total]
  float* dist2;              // [n_total]
  uint32_t* colmax;          // [stride] bit pattern of the largest |x| of the column over the eligible rows
  unsigned long long* sums;  // [k][stride] two's-complement int64 sums of q over the rows of a cluster (zero between rounds)
  uint32_t* counts;          // [k] rows of a cluster (zero between rounds)
  const int32_t* init_pos;   // [k] or null
  KmState* st;
  int32_t max_iter;
  int64_t stop_changed;
};

// elig, labels = -1, dist2 = +inf, colmax (zero before)
hipError_t launch_kmeans_prepare(const KmArgs& a, hipStream_t s);
// centres = the rows at init_pos; an ineligible one ends the call through the state
hipError_t launch_kmeans_gather(const KmArgs& a, hipStream_t s);
// round t: the assignment A(C_t) with the count of changed rows; the sums and counts of U unless the loop ends here; the end of the
// loop, or C_{t+1} and zeroed sums
hipError_t launch_kmeans_round(const KmArgs& a, int t, hipStream_t s);

}  // namespace scann

// Internal declarations of the greedy k-center selection over a latent-space index (scann_select.hip; the host half is in scann_select.cpp);
// the C ABI is include/scann_hip.h: scann_index_select.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_prim.h"

namespace scann {

constexpr int KC_LANES = 256;        // lanes of a workgroup = pool rows of a tile: one lane owns one row's chain
constexpr int KC_SLAB = 32;          // columns per LDS slab
constexpr int KC_MAX_GROUPS = 1024;  // workgroups of one pick (four fit a CU); each walks every KC_MAX_GROUPS-th tile

// What one pick hands to the next, in device memory (zeroed before the first launch)
struct KcState {
  uint32_t ticket;  // workgroups of the running launch that have left their candidate; the last one resets it
  int32_t count;    // picks made
  int32_t done;     // nothing eligible is left, or the next radius fell below stop_dist2: every later launch returns at once
  int32_t cur1;     // position of the latest pick + 1 (0: none yet): the centre the next launch folds into mind
};

// One selection.  Tile i holds rows [256 (i % tiles_per_chunk), + 256) of chunk i / tiles_per_chunk; position = chunk * chunk_rows + row.
struct KcArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, n_chunk, stride;
  int32_t tiles_per_chunk, n_tile;
  float* mind;               // [n_total] least dist2 to the reference and the picks so far
  uint8_t* live;             // [n_total] 1: every component finite and not picked yet
  unsigned long long* part;  // [workgroups] a workgroup's first row under (mind descending, position ascending): mind's bits << 32 | position
  KcState* st;
  int32_t* out_pos;          // [n_pick]
  float* out_r2;             // [n_pick]
  int32_t n_pick;
  float stop;                // stop_dist2 (<= 0: none)
};

// live[p] = row p is finite in every column; mind[p] = +inf unless `has_init` (then mind already holds the distances to the reference)
hipError_t launch_kcenter_prepare(const KcArgs& a, bool has_init, hipStream_t s);
// one pick: fold the latest centre into mind (none before the first pick), then take the first live row under the total order
hipError_t launch_kcenter_step(const KcArgs& a, int groups, hipStream_t s);

}  // namespace scann

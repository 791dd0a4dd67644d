// Internal declarations of the prototypes and criticisms of a latent-space index (MMD-critic; scann_proto.hip, the host half and the
// twins are in scann_proto.cpp); the C ABI is include/scann_hip.h: scann_index_prototypes, scann_index_criticisms, scann_prototypes_host,
// scann_criticisms_host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_peaks.h"

namespace scann {

constexpr int PT_LANES = 256;        // lanes of a workgroup = pool rows of a tile: one lane owns one row's chain
constexpr int PT_SLAB = 32;          // columns per LDS slab
constexpr int PT_MAX_GROUPS = 1024;  // workgroups of one pick (four fit a CU); each walks every PT_MAX_GROUPS-th tile

constexpr long long PT_ONE = 1ll << 30;            // t(i, i): the term at distance 0
constexpr long long PT_RANGE = 1ll << 32;          // N * m may not pass it: |score| <= N m 2^30 <= 2^62
constexpr long long PT_MAX_WEIGHT = 1ll << 31;     // a criticism weight lies in 0 .. 2^31: score <= 2^61

// what a row still is to a selection (ProtoArgs::live)
constexpr uint8_t PT_OUT = 0;     // never picked, never folded: a non-finite row; criticisms: also an excluded row or one of weight 0
constexpr uint8_t PT_LIVE = 1;    // can be picked
constexpr uint8_t PT_PICKED = 2;  // picked; prototypes: its B still takes every later column

// What one pick hands to the next, in device memory (zeroed before the first launch)
struct ProtoState {
  uint32_t ticket;  // workgroups of the running launch that have left their candidate; the last one resets it
  int32_t count;    // picks made
  int32_t done;     // nothing that can be picked is left: every later launch returns at once
  int32_t cur1;     // position of the latest pick + 1 (0: none yet): the column the next launch folds
  long long n;      // prototypes: eligible rows (proto_prepare_kernel counts them)
};

// One selection.  Tile i holds rows [256 (i % tiles_per_chunk), + 256) of chunk i / tiles_per_chunk; position = chunk * chunk_rows + row.
struct ProtoArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, n_chunk, stride;
  int32_t tiles_per_chunk, n_tile;
  float gamma;
  long long* A;         // [n_total] prototypes: A_i, -1 for an ineligible row; criticisms: the weights
  long long* B;         // [n_total] prototypes: the sum of the folded columns
  int32_t* cmax;        // [n_total] criticisms: the largest term to a pick so far
  uint8_t* live;        // [n_total] PT_OUT / PT_LIVE / PT_PICKED
  long long* part_v;    // [workgroups] a workgroup's first row under (score descending, position ascending): its score ...
  int32_t* part_p;      // ... and its position (-1: none)
  ProtoState* st;
  int32_t* out_pos;     // [n_pick]
  long long* out_score;  // [n_pick]
  int32_t n_pick;
};

// prototypes, after the self-join left S in A: A += 2^30 and live = PT_LIVE for the eligible rows (S >= 0), st->n = their number
hipError_t launch_proto_prepare(const ProtoArgs& a, hipStream_t s);
// criticisms: live = PT_LIVE for the finite rows of weight > 0, then PT_OUT for the n_ex positions at ex
hipError_t launch_crit_prepare(const ProtoArgs& a, const int32_t* ex, int32_t n_ex, hipStream_t s);
// one pick: fold the latest pick's column (none before the first pick), then take the first live row under the total order; crit: the
// fold is a max into cmax and the selection ends at a score <= 0, else the fold is a sum into B and a launch that finds n_pick picks made
// only folds
hipError_t launch_proto_step(const ProtoArgs& a, bool crit, int groups, hipStream_t s);

}  // namespace scann

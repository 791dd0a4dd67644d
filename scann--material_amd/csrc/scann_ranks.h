// Internal declarations of the exact neighbour ranks of a latent-space index (scann_ranks.hip; the host half and the twin are in
// scann_ranks.cpp); the C ABI is include/scann_hip.h: scann_index_ranks, scann_ranks_host.  The key comparison below is the one place
// that orders two keys: the twin and the kernels include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scann_peaks.h"

namespace scann {

// The search's total order on the rows seen from one query: dist2 ascending, then position ascending.  key (da, pa) <= key (db, pb).
// No key of an eligible pair has a NaN distance; +inf is an ordinary value.
__host__ __device__ inline bool ranks_key_le(float da, int32_t pa, float db, int32_t pb) { return da < db || (da == db && pa <= pb); }
// the position of a threshold that no probe owns: with dist2 +inf it lies behind every key of a row (positions stay below 2^31 - 1024)
constexpr int32_t RANKS_NO_POS = 0x7fffffff;

// How many of the N sorted thresholds (d[s * ld], p[s]), s = 0 .. N - 1, N a power of two, are <= the key (dist2, pos): the bin of a
// pair, 0 .. N.  A threshold's position is read only where its distance equals the pair's.
template <int N>
__host__ __device__ inline int ranks_bin(const float* d, int ld, const int32_t* p, float dist2, int32_t pos) {
  int lo = 0;  // the thresholds before lo are <= the key
#pragma unroll
  for (int half = N / 2; half >= 1; half >>= 1) {
    const int s = lo + half - 1;
    const float ds = d[s * ld];
    if (ds < dist2 || (ds == dist2 && p[s] <= pos)) lo += half;  // ranks_key_le, the position read on a tie only
  }
  const float ds = d[lo * ld];  // lo <= N - 1 here: the halves add up to N - 1
  if (ds < dist2 || (ds == dist2 && p[lo] <= pos)) lo += 1;
  return lo;
}

constexpr int RANKS_MP = 32;            // thresholds per query in the tables (SCANN_RANKS_MAX_PROBES), a power of two
constexpr int RANKS_RANGE_ROWS = 65472; // a workgroup's range has at most so many rows: its histogram counts in 16 bits (1023 tiles)
constexpr int64_t RANKS_SLICE = 262144; // queries per slice (SCANN_RANKS_SLICE): the four tables of a slice stay within 128 MiB

// One slice of a call: nq queries, rows of the pool by position, against positions 0 .. n_total - 1 of a pool stored in chunks of
// `chunk_rows` rows.  Workgroup (x, y) of the tile kernel takes queries [128 x, 128 x + 128) and positions [y * rows_per_range,
// (y + 1) * rows_per_range).
struct RanksArgs {
  const float* const* rows;   // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, stride;
  const unsigned char* elig;  // [n_total] 1: every component of the row is finite (launch_sil_eligible)
  const int32_t* qpos;        // [nq] the query's position
  const int32_t* probe;       // [nq][m] positions, -1: unused
  int32_t nq, m, rows_per_range, n_range;
  // prepare -> tiles -> finish
  int32_t* qleave;            // [nq] the query's position if it is eligible and has a probe with a rank, else -1: it gets nothing
  float* qmax;                // [nq] the largest distance among its thresholds with a rank
  float* thr_d;               // [nq][32] the probes' keys sorted ascending, behind them (+inf, RANKS_NO_POS) ...
  int32_t* thr_p;             // ... a probe without a rank has such a key too
  int32_t* slot_probe;        // [nq][32] which probe the sorted slot belongs to (>= m: none)
  unsigned int* table;        // [nq][32] cleared before the launch: bin b = the rows with exactly b thresholds <= their key
  int32_t* rank;              // [nq][m] the result
  float* dist2;               // [nq][m]
};
hipError_t launch_ranks_prepare(const RanksArgs& a, hipStream_t s);
hipError_t launch_ranks_tiles(const RanksArgs& a, hipStream_t s);
hipError_t launch_ranks_finish(const RanksArgs& a, hipStream_t s);

}  // namespace scann

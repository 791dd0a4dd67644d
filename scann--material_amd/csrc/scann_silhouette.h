// Internal declarations of the silhouette of a labelled latent-space index (scann_silhouette.hip; the host half and the twin are in
// scann_silhouette.cpp); the C ABI is include/scann_hip.h: scann_index_silhouette, scann_silhouette_host.  The fixed-point term below is
// the one place that forms it: the twin and the kernel include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scann_peaks.h"

namespace scann {

// The term of a pair at distance dist2: e = dist2 or its correctly rounded square root, f = e * 2^shift with scale = 2^shift (a normal
// fp32 number for -126 <= shift <= 126), t = round-to-nearest-even(f).  e * scale is ldexpf(e, shift): both are the one correct rounding
// of the exact product, gradual underflow included.  The term is out of range where e is not finite or t > 2^31, which is where f is not
// <= 2^31 (an infinite product of a finite e has t > 2^31); sil_round is then 2^31, and the call's result is an error anyway.
__host__ __device__ inline float sil_scaled(float dist2, bool squared, float scale) { return (squared ? dist2 : sqrtf(dist2)) * scale; }
__host__ __device__ inline bool sil_out_of_range(float f) { return !(f <= 2147483648.f); }
__host__ __device__ inline uint32_t sil_round(float f) { return (uint32_t)rintf(fminf(f, 2147483648.f)); }
// f is never negative, so its bit pattern orders it, +inf and NaN last: the kernel keeps the largest pattern of its terms
constexpr uint32_t SIL_LIMIT_BITS = 0x4f000000u;  // 2^31

// One launch of sil_tile_kernel: nq queries against the counting rows of a pool stored in chunks of `chunk_rows` rows, through a
// permutation.  perm [n_perm] lists the counting positions sorted by (label, position), every cluster padded with -1 to whole 64-row
// tiles, so a tile belongs to one cluster: tile_label [n_perm / 64].  Workgroup (x, y) takes queries [128 x, 128 x + 128) and the
// permutation entries [y * rows_per_range, (y + 1) * rows_per_range).
struct SilArgs {
  const float* const* rows;   // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t chunk_rows, stride;
  const int32_t* perm;        // [n_perm], n_perm a multiple of 64
  const int32_t* tile_label;  // [n_perm / 64]
  int32_t n_perm;
  const int32_t* qpos;        // [nq] the query's position, which its sums leave out; -1: the query does not count and gets nothing
  const int32_t* qlabel;      // [nq] its label, -1 where it does not count (the finish)
  int32_t nq, rows_per_range, n_range;
  int32_t squared, shift, C;
  float scale;                // 2^shift
  unsigned long long* table;  // [nq][C] int64, cleared before the launch: every workgroup adds its range's part per cluster
  const long long* counts;    // [C]
  unsigned int* flag;         // set to 1 where a term is out of range
  double *a, *b;              // [nq] the finish
  int32_t* other;             // [nq]
};
hipError_t launch_sil_tiles(const SilArgs& a, hipStream_t s);
// a, b, other of the nq queries from the finished table and the counts (after launch_sil_tiles, on the same stream)
hipError_t launch_sil_finish(const SilArgs& a, hipStream_t s);
// ok[p] = 1 where all components of the row at position p are finite, else 0
hipError_t launch_sil_eligible(const float* const* rows, int32_t n_total, int32_t chunk_rows, int32_t stride, unsigned char* ok, hipStream_t s);

}  // namespace scann

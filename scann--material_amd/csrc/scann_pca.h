// Internal declarations of the principal-component map of a latent-space index (scann_pca.hip; the host half, the twins and the
// eigen-decomposition are in scann_pca.cpp); the C ABI is include/scann_hip.h: scann_index_moments, scann_index_project, scann_project_batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_tile.h"

namespace scann {

constexpr int PCA_LANES = TILE_LANES;    // lanes of every workgroup
constexpr int PCA_BLK = 64;          // columns of a block of pca_scatter_kernel: a workgroup owns one 64 x 64 block of T, a lane 4 x 4 of it
constexpr int PCA_ROWS = 32;         // rows per LDS slab of that kernel
constexpr int PCA_GROUPS = 1024;     // about as many workgroups in the sum, maximum and scatter passes
constexpr int PCA_TP = TILE_TQ;      // rows of a tile of pca_project_kernel
constexpr int PCA_TC = TILE_TR;      // components per block of that kernel: a lane owns 8 rows x 4 components
constexpr int PCA_SLAB = TILE_SLAB;    // columns per LDS slab of that kernel
constexpr int PCA_MAX_GROUPS = 768;  // workgroups of a projection at most: the tiles are dealt evenly

// What the passes of the moments hand to each other, in device memory (zeroed before the first launch)
struct PcaState {
  uint32_t n;  // eligible rows
};

// The moments of one index.  position = chunk * chunk_rows + row.
struct PcaArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, n_chunk, stride, dim;
  PcaState* st;
  uint8_t* elig;             // [n_total] 1: every component finite
  uint32_t* colmax;          // [stride] bit pattern of the largest |x| of the column over the eligible rows
  unsigned long long* sums;  // [stride] S_j, two's-complement int64
  float* mean;               // [stride]
  uint32_t* cenmax;          // [stride] bit pattern of the largest |x - mean| of the column over the eligible rows
  unsigned long long* T;     // [stride][stride] the blocks (I, J), I <= J, of the scatter
  unsigned long long* R;     // [stride]
  double* cov;               // [dim][dim]
  int32_t* col_exp;          // [dim] f_j
  const uint8_t* mask;       // [n_total] or null: a row with mask 0 is not eligible whatever it holds (scann_index_fit_moments: its targets)
};

// elig, n, colmax; S; mean; cenmax; T and R; cov and col_exp -- six launches on one stream, nothing waits in between
hipError_t launch_pca_moments(const PcaArgs& a, hipStream_t s);

// One projection: rows [first, first + n) of a chunked block of rows (a single chunk for the rows of a batch)
struct PcaProjArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t first, n, chunk_rows, stride, dim;
  const float* mean;         // [stride], the padding zero
  const float* comp;         // [m][stride], the padding zero
  const float* scale;        // [m]
  int32_t m;
  float* coords;             // [n][m]
  float* md2;                // [n] or null
  float* dist2;              // [n] or null
};
hipError_t launch_pca_project(const PcaProjArgs& a, hipStream_t s);

}  // namespace scann

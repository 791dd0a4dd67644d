// Internal declarations of the Gaussian landmark features of a latent-space index (scann_rbf.hip; the host half and the twin are in
// scann_rbf.cpp); the C ABI is include/scann_hip.h: scann_rbf_weight, scann_index_rbf_features, scann_rbf_features_host,
// scann_rbf_head_batch.  The weight chain below is the one place that holds its coefficients: the host twin and the kernel include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scann_tile.h"

namespace scann {

// c_j = the fp32 rounding of 2^(-1/2) (-ln 2)^j / j!, j = 0 .. 7: 2^(-1/2 - g) on g in [-1/2, 1/2)
#define SCANN_RBF_C0 0x1.6a09e6p-1f
#define SCANN_RBF_C1 -0x1.f5e466p-2f
#define SCANN_RBF_C2 0x1.5be298p-3f
#define SCANN_RBF_C3 -0x1.41839ep-5f
#define SCANN_RBF_C4 0x1.bdb696p-8f
#define SCANN_RBF_C5 -0x1.ee4fd2p-11f
#define SCANN_RBF_C6 0x1.c8d752p-14f
#define SCANN_RBF_C7 -0x1.69e51ep-17f

// 2^(-dist2 * gamma), the definition of scann_rbf_weight (include/scann_hip.h): every operation fp32 and rounded once, nothing
// contracted beyond the stated fmaf; the same body on the host and on the device.  u < 0 does not arise from a distance; there the
// exponent is bounded so that the conversion to int is defined on both sides (the result is then > 1, +inf from 2^128 on).
__host__ __device__ inline float rbf_weight(float dist2, float gamma) {
#pragma clang fp contract(off)
  const float u = dist2 * gamma;
  if (!(u < 126.f)) return u != u ? u : 0.f;  // NaN stays NaN; from 126 on (and at +inf) the weight is 0: no denormal result arises
  const float i = floorf(u);
  const float g = (u - i) - 0.5f;  // in [-0.5, 0.5)
  float p = SCANN_RBF_C7;
  p = fmaf(p, g, SCANN_RBF_C6);
  p = fmaf(p, g, SCANN_RBF_C5);
  p = fmaf(p, g, SCANN_RBF_C4);
  p = fmaf(p, g, SCANN_RBF_C3);
  p = fmaf(p, g, SCANN_RBF_C2);
  p = fmaf(p, g, SCANN_RBF_C1);
  p = fmaf(p, g, SCANN_RBF_C0);
  return ldexpf(p, i < -256.f ? 256 : -(int)i);
}

constexpr int RBF_LANES = TILE_LANES;  // lanes of rbf_feature_kernel
constexpr int RBF_TP = TILE_TQ;  // pool rows per tile
constexpr int RBF_TL = TILE_TR;  // landmarks per tile
constexpr int RBF_SLAB = TILE_SLAB;  // columns per LDS slab
constexpr int RBF_LD = RBF_TL + 4;  // floats per row of the feature tile in LDS: 16-byte aligned, rows four banks apart
// floats the slabs and the feature tile share: max(32 * (128 + 64) + 64, 128 * 68)
constexpr int RBF_UNION = RBF_TP * RBF_LD;

// One launch of rbf_feature_kernel: the features of positions 0 .. n_total - 1 of a pool stored in chunks of `chunk_rows` rows against m
// landmarks, written to rows of `out_stride` floats stored in chunks of `out_chunk_rows` rows.  Workgroup b takes the 128 positions from
// 128 (b / n_lt) and the 64 landmarks from 64 (b % n_lt), n_lt = ceil(m / 64): the tiles are cut by position, so neither table's
// chunking enters the result.  Columns m .. out_stride - 1 of a written row are set to zero.
struct RbfArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, stride;
  const float* lm;           // [m][stride] landmarks, padded like the rows
  int32_t m;
  float gamma;
  float* const* out;         // [n_out_chunk] -> [out_chunk_rows][out_stride]
  int32_t out_chunk_rows, out_stride;
};
hipError_t launch_rbf_features(const RbfArgs& a, hipStream_t s);

}  // namespace scann

// Internal declarations of the readout head fitted on a latent-space index (scann_head.hip; the host half and the twin are in
// scann_head.cpp); the C ABI is include/scann_hip.h: scann_index_fit_moments, scann_index_ridge_loo, scann_head_batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "scann_pca.h"

struct scann_handle;

namespace scann {

constexpr int HEAD_LANES = 256;   // lanes of every workgroup
constexpr int HEAD_KMAX = 16;     // SCANN_HEAD_MAX_TARGETS
constexpr int HEAD_LMAX = 32;     // SCANN_HEAD_MAX_LAMBDA
constexpr int HEAD_TILE = 128;    // rows of a tile of head_loo_kernel: the reduction block of the definition
constexpr int HEAD_COLS = 64;     // output columns (chains per row) of one pass of that kernel
constexpr int HEAD_SLAB = 32;     // components per LDS slab of that kernel
constexpr int HEAD_GROUPS = 1024; // about as many workgroups in the passes over the targets and in the cross scatter
constexpr int HEAD_XROWS = 64;    // rows per LDS slab of quantised targets in head_cross_kernel

// The target half of the augmented moments.  The X half (eligibility under the wider mask, n, mean, f, T, R, cov) is PcaArgs'.
struct HeadMomArgs {
  const float* t;             // [n_total][K] targets
  int32_t K;
  uint32_t* tmax;             // [16] bit pattern of the largest |t| of the column over the eligible rows
  unsigned long long* tsum;   // [16] S of the target columns
  float* tmean;               // [16]
  uint32_t* tcen;             // [16] bit pattern of the largest |t - mean|
  unsigned long long* Txt;    // [stride][16] sum of u_j * v_k
  unsigned long long* Ttt;    // [16][16]     sum of v_k * v_k'
  unsigned long long* Rt;     // [16]         sum of v_k
  double* cross;              // [dim + K][K] the covariance of every column of [rows | t] with target k
  int32_t* texp;              // [16] f of the target columns
};

// mask[p] = every target of row p finite (rows null), or that and every component of the row finite
hipError_t launch_head_mask(const float* const* rows, int32_t chunk_rows, int32_t stride, int32_t n_total, const float* t, int32_t K, uint8_t* mask,
                            hipStream_t s);
// behind launch_pca_moments(a) with a.mask set: the target columns' mean and f, the cross and target blocks of the scatter, their covariance
hipError_t launch_head_moments(const PcaArgs& a, const HeadMomArgs& m, hipStream_t s);

// One group of rows of the leave-one-out pass: positions [first, first + n) of the pool, first a multiple of HEAD_TILE; z holds their
// coordinates.  Tile g of the group writes part[(first / HEAD_TILE + g) * Q ..], Q = 3 L K + L + 1: sse, sae, sse_fit [L * K] each, dof [L], rows.
struct HeadLooArgs {
  int32_t first, n, m, L, K;
  const float* z;        // [n][m]
  const float* t;        // [n_total][K]
  const float* tmean;    // [K]
  const float* scale;    // [L][m]
  const float* coef;     // [L * K][m]
  float lev0;
  const uint8_t* elig;   // [n_total]
  const int32_t* resid_l;  // [K] or null
  float* resid;          // [n_total][K] or null (filled with NaN beforehand)
  double* part;
};
hipError_t launch_head_loo(const HeadLooArgs& a, hipStream_t s);
// out[q] = the partials of tiles 0 .. n_tile - 1 added in that order, q < Q
hipError_t launch_head_sum(const double* part, int32_t n_tile, int32_t Q, double* out, hipStream_t s);

// pred[p][k] = tmean[k] + w[p][k];  lev[p][k] = lev0 + the md2 chain of z[p] with scale[k]
struct HeadEvalArgs {
  int32_t n, m, K;
  const float* w;      // [n][K]
  const float* z;      // [n][m]
  const float* tmean;  // [K]
  const float* scale;  // [K][m]
  float lev0;
  float* pred;         // [n][K]
  float* lev;          // [n][K]
};
hipError_t launch_head_eval(const HeadEvalArgs& a, hipStream_t s);

// The evaluation of scann_head_batch, shared with scann_rbf_head_batch (scann_head.cpp).  check_head_eval: what is wrong with a head's
// host arguments over rows of `dim` columns, or an empty string.  head_eval_rows: pred / lev [nq * K] of the head on nq device rows,
// `pitch` floats apart (dim, or the stride dim rounded up to a multiple of 4 with zero padding), enqueued on s, downloaded and waited for.
std::string check_head_eval(int dim, const float* mean, const float* tmean, const float* weights, int32_t K, const float* components, int32_t m,
                            const float* scale, float lev0, const float* pred, const float* lev);
int head_eval_rows(scann_handle* h, hipStream_t s, const float* src, int pitch, int64_t nq, int dim, const float* mean, const float* tmean,
                   const float* weights, int32_t K, const float* components, int32_t m, const float* scale, float lev0, float* pred, float* lev);

}  // namespace scann

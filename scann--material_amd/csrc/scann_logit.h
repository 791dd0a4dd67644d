// Internal declarations of the classification head on a latent-space index (scann_logit.hip; the host half and the twin are in
// scann_logit.cpp); the C ABI is include/scann_hip.h: scann_index_logit_pass, scann_logit_pass_host, scann_logit_head_batch.  The softmax
// body below is the one place that defines a row's probabilities: the host twin and the kernels include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scann_rbf.h"

namespace scann {

constexpr int LOGIT_CMAX = 16;     // SCANN_LOGIT_MAX_CLASSES
constexpr int LOGIT_MMAX = 64;     // SCANN_LOGIT_MAX_MODELS
constexpr int LOGIT_LANES = TILE_LANES; // lanes of logit_pass_kernel
constexpr int LOGIT_BLOCK = TILE_TQ; // positions of a block: the innermost level of the summation tree of the definition
constexpr int LOGIT_SPAN = 32;     // blocks of a span, the middle level: one workgroup
constexpr int LOGIT_COLS = TILE_TR; // logit columns (model x class) of one launch
constexpr int LOGIT_GMAX = 32;     // models of one launch at most (64 columns / 2 classes)
constexpr int LOGIT_SLAB = TILE_SLAB; // components per LDS slab of the logit chains
constexpr int LOGIT_CHUNK = 64;    // components per LDS chunk of the gradient accumulation
constexpr int LOGIT_LD = LOGIT_COLS + 4;  // floats per row of the logit / residual tile and of the component chunk in LDS
#define SCANN_LOGIT_LOG2E 0x1.715476p+0f  // the fp32 rounding of log2(e): scann_rbf_weight(u, log2 e) = e^-u

// The softmax of one row's C logits, the definition of include/scann_hip.h: every operation fp32 and rounded once.  a[k] for k >= C is not
// read.  p[k] = w_k / S with w_k = 2^-((amax - a_k) log2 e) through the bit-defined chain of scann_rbf.h, S the sum of the w_k with k
// ascending, the division IEEE correctly rounded.  best: the lowest k whose logit no later one exceeds (a NaN logit exceeds nothing and
// nothing exceeds a NaN in place 0).  brier: the fmaf chain of (p_k - onehot_k)^2, k ascending.  The loops run over all 16 places under
// a k < C guard so that on the device the arrays stay in registers.
__host__ __device__ inline void logit_softmax(const float (&a)[LOGIT_CMAX], int C, int label, float (&p)[LOGIT_CMAX], float& brier, int& best) {
#pragma clang fp contract(off)
  float amax = a[0], abest = a[0];
  best = 0;
#pragma unroll
  for (int k = 1; k < LOGIT_CMAX; ++k)
    if (k < C) {
      amax = fmaxf(amax, a[k]);
      if (a[k] > abest) abest = a[k], best = k;
    }
  float S = 0.f;
#pragma unroll
  for (int k = 0; k < LOGIT_CMAX; ++k)
    if (k < C) {
      p[k] = rbf_weight(amax - a[k], SCANN_LOGIT_LOG2E);
      S = k == 0 ? p[0] : S + p[k];
    }
  float b = 0.f;
#pragma unroll
  for (int k = 0; k < LOGIT_CMAX; ++k)
    if (k < C) {
      p[k] = p[k] / S;
      const float e = p[k] - (k == label ? 1.f : 0.f);
      b = fmaf(e, e, b);
    }
  brier = b;
}

// One launch of logit_pass_kernel: `ncol` = n_model * C logit columns of models that all have C classes, over positions 0 .. n_total - 1
// of a pool stored in chunks of `chunk_rows` rows.  Workgroup s takes span s (positions 4096 s .. 4096 s + 4095), block by block, and
// adds every block's sums, in block order, to its own partials gpart[s][ncol][dim + 1] and spart[s][n_model][6], which the caller
// cleared; launch_logit_sum then adds the spans in order.  Column jj * C + k is class k of the launch's model jj.
struct LogitArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t n_total, chunk_rows, stride, dim;
  const int32_t* labels;     // [n_total]
  const float* mean;         // [stride], padding zero
  const float* u;            // [ncol][stride] the weights of the launch's columns, padding zero
  const float* u0;           // [ncol] their intercepts
  int32_t C, n_model, ncol;
  int32_t F;                 // folds, 0 or 2 .. 16
  int32_t fold[LOGIT_GMAX];  // the fold each model holds out, or -1
  int32_t prob_model[LOGIT_CMAX];  // per fold (place 0 with F = 0): the launch's model whose probabilities go to prob, or -1
  double* gpart;             // [n_span][ncol][dim + 1]
  double* spart;             // [n_span][n_model][6]: rows, hits, brier over the training rows, then over the held-out rows
  float* prob;               // [n_total][C] or null
  int64_t* n_used;           // [n_span] rows that count (written by every launch: the same values)
};
hipError_t launch_logit_pass(const LogitArgs& a, hipStream_t s);
// out[q * out_pitch .. + inner) for q < outer: part[s][q][0 .. inner) added over the spans in order (out_pitch >= inner)
hipError_t launch_logit_sum(const double* part, int32_t n_span, int32_t Q, double* out, hipStream_t s);
// every float of x[0 .. n) becomes the quiet NaN 0x7fc00000
hipError_t launch_logit_fill_nan(float* x, int64_t n, hipStream_t s);
// prob[p][k], p < n, of one model on device rows `pitch` floats apart: the logit chain of the definition and logit_softmax
hipError_t launch_logit_eval(const float* rows, int32_t pitch, int32_t n, int32_t dim, const float* mean, const float* u /* [C][dim + 1] */, int32_t C,
                             float* prob, hipStream_t s);

}  // namespace scann

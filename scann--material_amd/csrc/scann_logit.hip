// Classification head on a latent-space index (scann_index_logit_pass, include/scann_hip.h): for several softmax models at once, each
// model's log-likelihood gradient and score sums over the rows of an index, in the original coordinates.
//
// logit_pass_kernel: one workgroup of 256 lanes per span of 32 blocks of 128 positions, up to 64 logit columns (model x class) per launch.
// Per block:
//   A  the logit chains (fp32 fmaf, components ascending, from the intercept) on the tile and the slab pipeline of scann_tile.h, product
//      form: rows (minus the mean) are the tile's "queries", the weights its "rows", a lane owns 8 rows x 4 columns;  whether a row
//      has a non-finite component is found while it is staged.  The 128 x 64 logits go to an LDS tile.
//   B  one lane per (row, model): logit_softmax (scann_logit.h), the residuals onehot - p written over the logits (0 where the row does
//      not train the model), brier / hit / membership to LDS, the probabilities of the model that reports the row's fold to global.
//   D  one lane per quantity: the 64 intercept sums and the 6 score sums of every model, over the block's rows in position order (fp64).
//   C  the gradient, 64 components at a time: the rows are staged again (minus the mean; zero where the row does not count), a lane owns
//      4 columns x 4 components of fp64 accumulators and runs over the 128 rows in position order.
// A block's sums are added to the workgroup's own span partials in global memory (the same lane owns a quantity throughout, plain loads
// and stores); logit_sum_kernel adds the spans in order, one lane per quantity.  The tree -- block, span, spans -- is the definition's.
// No atomics on floating-point values, no scratch.
#pragma clang fp contract(off)

#include <algorithm>

#include "scann_logit.h"

namespace scann {

namespace {

constexpr int TILE = LOGIT_BLOCK * LOGIT_LD;      // floats of the logit tile, and of the area behind it

__global__ __launch_bounds__(LOGIT_LANES) void logit_pass_kernel(LogitArgs a) {
  __shared__ float4 logit_smem[2 * TILE / 4];
  __shared__ int bad[LOGIT_BLOCK], lab[LOGIT_BLOCK];
  __shared__ int n_count;
  float* tile = reinterpret_cast<float*>(logit_smem);  // [128][68] logits, then residuals
  float* area = tile + TILE;
  float* ps = area;                                    // A: the row slab ...
  float* ls = area + tile_slab_floats(LOGIT_BLOCK);    // A: ... and the weight slab (tile_stage)
  float* bri = area;                                   // B, D: [128][32] brier of (row, model)
  int* code = reinterpret_cast<int*>(area + LOGIT_BLOCK * LOGIT_GMAX);  // B, D: [128][32] 1 trains, 2 held out, 4 hit
  float* ych = area;                                   // C: [128][68] the chunk's components
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int stride = a.stride, dim = a.dim, C = a.C, ncol = a.ncol, n_model = a.n_model, F = a.F;
  const int span = (int)blockIdx.x;
  const size_t D1 = (size_t)dim + 1;
  double* gp = a.gpart + (size_t)span * ncol * D1;
  double* sp = a.spart + (size_t)span * n_model * 6;
  if (t == 0) n_count = 0;
  const float* lrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int item = (t + LOGIT_LANES * i) >> 3;
    lrow[i] = item < ncol ? a.u + (size_t)item * stride : nullptr;
  }
  float u0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) u0[j] = 4 * rg + j < ncol ? a.u0[4 * rg + j] : 0.f;
  const int n_slab = (dim + LOGIT_SLAB - 1) / LOGIT_SLAB;
  for (int b = 0; b < LOGIT_SPAN; ++b) {
    const int p0 = (span * LOGIT_SPAN + b) * LOGIT_BLOCK;
    if (p0 >= a.n_total) break;
    __syncthreads();  // the previous block's reads of the tile and the area are over
    if (t < LOGIT_BLOCK) {
      const bool in = p0 + t < a.n_total;
      bad[t] = in ? 0 : 1;
      lab[t] = in ? a.labels[p0 + t] : -1;
    }
    // ---- A: the logit chains.  A block may lie across two storage chunks
    const int pc0 = p0 / a.chunk_rows, poff = p0 - pc0 * a.chunk_rows;
    const float* prow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int item = (t + LOGIT_LANES * i) >> 3;
      int o = poff + item, c = pc0;
      if (o >= a.chunk_rows) o -= a.chunk_rows, ++c;
      prow[i] = p0 + item < a.n_total ? a.rows[c] + (size_t)o * stride : nullptr;
    }
    float4 gq[4], gr[2];
    float nf[4] = {0.f, 0.f, 0.f, 0.f};  // NaN once a staged piece of the lane's item i was not finite
    auto fetch = [&](int slab) {
      const int col = slab * LOGIT_SLAB + 4 * (t & 7);
      const float4 m4 = col < stride ? *reinterpret_cast<const float4*>(a.mean + col) : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 v = prow[i] && col < stride ? *reinterpret_cast<const float4*>(prow[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
        nf[i] += row_nonfinite(v);
        gq[i] = float4{v.x - m4.x, v.y - m4.y, v.z - m4.z, v.w - m4.w};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) gr[i] = lrow[i] && col < stride ? *reinterpret_cast<const float4*>(lrow[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
    };
    f2 acc[8][2];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j][0] = f2{u0[0], u0[1]}, acc[j][1] = f2{u0[2], u0[3]};
    fetch(0);
    for (int slab = 0; slab < n_slab; ++slab) {
      __syncthreads();  // the previous slab's reads are over
      tile_stage<LOGIT_LANES, 4, LOGIT_BLOCK>(ps, gq, t);
      tile_stage<LOGIT_LANES, 2, LOGIT_COLS>(ls, gr, t);
      __syncthreads();
      if (slab + 1 < n_slab) fetch(slab + 1);
      const int nc = min(LOGIT_SLAB, dim - slab * LOGIT_SLAB);  // the components that exist: a chain has no step for the padding
      tile_slab<TileForm::PROD>(ps, ls, qg, rg, acc, nc);
    }
    __syncthreads();  // every lane has read its last slab
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (nf[i] != nf[i]) bad[(t + LOGIT_LANES * i) >> 3] = 1;  // (the eight lanes of an item may all write: the same value)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = tile_query(qg, j);
      *reinterpret_cast<float4*>(tile + row * LOGIT_LD + 4 * rg) = float4{acc[j][0].x, acc[j][0].y, acc[j][1].x, acc[j][1].y};
    }
    __syncthreads();
    // ---- B: softmax, residuals, scores
    for (int item = t; item < LOGIT_BLOCK * n_model; item += LOGIT_LANES) {
      const int row = item & (LOGIT_BLOCK - 1), jj = item >> 7;
      const int label = lab[row], p = p0 + row;
      const bool counts = !bad[row] && label >= 0 && label < C;
      float* av = tile + row * LOGIT_LD + jj * C;
      float lg[LOGIT_CMAX], pv[LOGIT_CMAX], brier;
      int best;
#pragma unroll
      for (int k = 0; k < LOGIT_CMAX; ++k) lg[k] = k < C ? av[k] : 0.f;
      logit_softmax(lg, C, label, pv, brier, best);
      const int f = a.fold[jj], fp = F > 0 ? p % F : 0;
      const bool train = counts && (f < 0 || fp != f), held = counts && f >= 0 && fp == f;
#pragma unroll
      for (int k = 0; k < LOGIT_CMAX; ++k)
        if (k < C) av[k] = train ? (k == label ? 1.f : 0.f) - pv[k] : 0.f;
      bri[row * LOGIT_GMAX + jj] = brier;
      code[row * LOGIT_GMAX + jj] = (train ? 1 : 0) | (held ? 2 : 0) | (best == label ? 4 : 0);
      if (a.prob && counts && a.prob_model[fp] == jj) {
        float* dst = a.prob + (size_t)p * C;
#pragma unroll
        for (int k = 0; k < LOGIT_CMAX; ++k)
          if (k < C) dst[k] = pv[k];
      }
      if (jj == 0 && counts) atomicAdd(&n_count, 1);
    }
    __syncthreads();
    // ---- D: intercept and score sums, one lane per quantity, rows in position order
    if (t < LOGIT_COLS) {
      if (t < ncol) {
        double s = 0.0;
        for (int row = 0; row < LOGIT_BLOCK; ++row) s += (double)tile[row * LOGIT_LD + t];
        gp[(size_t)t * D1 + dim] += s;
      }
    } else if (t - LOGIT_COLS < 6 * n_model) {
      const int q = t - LOGIT_COLS, jj = q / 6, which = (q % 6) / 3, kind = q % 3;
      double s = 0.0;
      for (int row = 0; row < LOGIT_BLOCK; ++row) {
        const int c = code[row * LOGIT_GMAX + jj];
        if (!(c & (1 << which))) continue;
        s += kind == 0 ? 1.0 : kind == 1 ? ((c & 4) ? 1.0 : 0.0) : (double)bri[row * LOGIT_GMAX + jj];
      }
      sp[q] += s;
    }
    // ---- C: the gradient, 64 components at a time
    const int cg = t >> 4, pg = t & 15;
    for (int c0 = 0; c0 < dim; c0 += LOGIT_CHUNK) {
      __syncthreads();  // D's, or the previous chunk's, reads of the area are over
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = t + LOGIT_LANES * i, row = e >> 4, c4 = 4 * (e & 15), col = c0 + c4;
        float4 v{0.f, 0.f, 0.f, 0.f};
        if (!bad[row] && col < stride) {
          int o = poff + row, c = pc0;
          if (o >= a.chunk_rows) o -= a.chunk_rows, ++c;
          const float4 x = *reinterpret_cast<const float4*>(a.rows[c] + (size_t)o * stride + col);
          const float4 m4 = *reinterpret_cast<const float4*>(a.mean + col);
          v = float4{x.x - m4.x, x.y - m4.y, x.z - m4.z, x.w - m4.w};
        }
        *reinterpret_cast<float4*>(ych + row * LOGIT_LD + c4) = v;
      }
      __syncthreads();
      if (4 * cg >= ncol) continue;
      double g[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[i][j] = 0.0;
#pragma unroll 2
      for (int row = 0; row < LOGIT_BLOCK; ++row) {
        const float4 r4 = *reinterpret_cast<const float4*>(tile + row * LOGIT_LD + 4 * cg);
        const float4 y4 = *reinterpret_cast<const float4*>(ych + row * LOGIT_LD + 4 * pg);
        const double rd[4] = {(double)r4.x, (double)r4.y, (double)r4.z, (double)r4.w};
        const double yd[4] = {(double)y4.x, (double)y4.y, (double)y4.z, (double)y4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) g[i][j] = __builtin_fma(rd[i], yd[j], g[i][j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = 4 * cg + i, comp = c0 + 4 * pg + j;
          if (col < ncol && comp < dim) gp[(size_t)col * D1 + comp] += g[i][j];
        }
    }
  }
  __syncthreads();
  if (t == 0) a.n_used[span] = n_count;
}

__global__ __launch_bounds__(256) void logit_sum_kernel(const double* part, int n_span, int Q, double* out) {
  const int q = (int)(blockIdx.x * 256 + threadIdx.x);
  if (q >= Q) return;
  double s = 0.0;
  for (int i = 0; i < n_span; ++i) s += part[(size_t)i * Q + q];
  out[q] = s;
}

__global__ __launch_bounds__(256) void logit_fill_nan_kernel(float* x, long long n) {
  const float nan = __builtin_nanf("");
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) x[i] = nan;
}

__global__ __launch_bounds__(256) void logit_eval_kernel(const float* rows, int pitch, int n, int dim, const float* mean, const float* u, int C, float* prob) {
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= n) return;
  const float* x = rows + (size_t)p * pitch;
  float lg[LOGIT_CMAX], pv[LOGIT_CMAX], brier;
  int best;
#pragma unroll
  for (int k = 0; k < LOGIT_CMAX; ++k) {
    lg[k] = 0.f;
    if (k < C) {
      const float* w = u + (size_t)k * (dim + 1);
      float acc = w[dim];
      for (int j = 0; j < dim; ++j) acc = fmaf(x[j] - mean[j], w[j], acc);
      lg[k] = acc;
    }
  }
  logit_softmax(lg, C, -1, pv, brier, best);
#pragma unroll
  for (int k = 0; k < LOGIT_CMAX; ++k)
    if (k < C) prob[(size_t)p * C + k] = pv[k];
}

}  // namespace

hipError_t launch_logit_pass(const LogitArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.ncol <= 0) return hipSuccess;
  const unsigned n_span = (unsigned)(((int64_t)a.n_total + LOGIT_BLOCK * LOGIT_SPAN - 1) / (LOGIT_BLOCK * LOGIT_SPAN));
  hipLaunchKernelGGL(logit_pass_kernel, dim3(n_span), dim3(LOGIT_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_logit_sum(const double* part, int32_t n_span, int32_t Q, double* out, hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  hipLaunchKernelGGL(logit_sum_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, part, n_span, Q, out);
  return hipGetLastError();
}

hipError_t launch_logit_fill_nan(float* x, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(logit_fill_nan_kernel, dim3(grid), dim3(256), 0, s, x, (long long)n);
  return hipGetLastError();
}

hipError_t launch_logit_eval(const float* rows, int32_t pitch, int32_t n, int32_t dim, const float* mean, const float* u, int32_t C, float* prob,
                             hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(logit_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, pitch, n, dim, mean, u, C, prob);
  return hipGetLastError();
}

}  // namespace scann

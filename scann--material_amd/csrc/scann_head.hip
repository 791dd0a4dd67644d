// Readout head on a latent-space index (scann_index_fit_moments, scann_index_ridge_loo, scann_head_batch, include/scann_hip.h): ridge
// regression of K targets on the rows of an index, its regularisation chosen by exact leave-one-out residuals, bit-reproducible.
//   moments     the definition of scann_index_moments on the N x (dim + K) matrix [rows | t].  The X half -- eligibility under the wider
//               mask, n, mean, f, the X-X scatter and its covariance -- is launch_pca_moments with PcaArgs::mask = the finiteness of the
//               targets (head_mask_kernel).  The target columns are read from their own array:
//   head_tstat_kernel<0|1|2>  the column maxima of |t|, the 30-bit sums S, the column maxima of |t - mean| over the eligible rows: a lane
//                          keeps K values in registers over its rows, then one LDS and one global integer atomic per column.
//   head_tmean_kernel      the means of the target columns.
//   head_cross_kernel      the cross block: a lane owns one column j of X and K int64 accumulators of u_j * v_k; the quantised targets of
//                          64 rows at a time lie in LDS, read as broadcasts.  The workgroups of the first column block also sum the K x K
//                          block and R of the targets.  Integer sums: order-free, added with 64-bit integer atomics.
//   head_cross_finalise_kernel  the covariance of every column of [rows | t] with every target: the expression of pca_finalise_kernel.
//   leave-one-out   pca_project_kernel leaves the coordinates z [rows][m] of a group of rows in device memory; head_loo_kernel takes one
//               128-row tile -- the reduction block of the definition -- per workgroup.  A lane owns one row and the chains of 16 (leverages)
//               or 32 (predictions) of the 64 output columns of a pass; z and the [S | B] columns pass through LDS 32 components at a
//               time, the coefficients read as broadcasts.  Every chain is VALU fmaf over the components ascending, never split.  Behind the
//               chains every lane forms e and r of its row in registers; 64 lanes then add one column each over the tile's rows in row
//               order in fp64 and write the tile's partial.  head_sum_kernel adds the partials in tile order.
//   head_eval_kernel  pred = tmean + w and lev = lev0 + md2 behind the two projections of scann_head_batch.
// No float atomics, no scratch.
#include "scann_head.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace scann {

namespace {

constexpr int HEAD_ZS = HEAD_TILE + 1;           // floats per staged component of the z slab and per column of the other per-row tables
constexpr int HEAD_CS = HEAD_COLS + 4;           // floats per staged component of the coefficient slab
constexpr int HEAD_UNION = HEAD_COLS * HEAD_ZS;  // the slabs and the tile of residuals share this: 64 * 129 >= 32 * 129 + 32 * 68

// the eligibility scan (scann_prim.h) over the rows, where there are any, and the K targets of a row, its 8 lanes taking one in turn
__global__ __launch_bounds__(HEAD_LANES) void head_mask_kernel(const float* const* rows, int chunk_rows, int stride, int n_total, const float* t, int K,
                                                               uint8_t* mask) {
  eligible_scan(
      rows, chunk_rows, stride, n_total,
      [&](int p, int sub) {
        int bad = 0;
        for (int k = sub; k < K; k += 8) bad |= !f32_finite(t[(size_t)p * K + k]);
        return bad;
      },
      [&](int p, int bad) { mask[p] = bad ? 0 : 1; });
}

// MODE 0: tmax_k = max |t|; MODE 1: S_k += q(t, k); MODE 2: tcen_k = max |t - mean_k|; over the eligible rows, a lane one row at a time
template <int MODE>
__global__ __launch_bounds__(HEAD_LANES) void head_tstat_kernel(PcaArgs a, HeadMomArgs m) {
  __shared__ unsigned long long red[HEAD_KMAX];
  const int tid = threadIdx.x, K = m.K;
  if (tid < HEAD_KMAX) red[tid] = 0;
  __syncthreads();
  long long s[HEAD_KMAX];
  uint32_t mx[HEAD_KMAX];
  int sh[HEAD_KMAX];
  float mean[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) {
    s[k] = 0, mx[k] = 0;
    sh[k] = MODE == 1 && k < K ? 30 - f32_exponent(m.tmax[k]) : 0;
    mean[k] = MODE == 2 && k < K ? m.tmean[k] : 0.f;
  }
  for (int64_t p = (int64_t)blockIdx.x * HEAD_LANES + tid; p < a.n_total; p += (int64_t)gridDim.x * HEAD_LANES) {
    if (!a.elig[p]) continue;
    const float* tp = m.t + (size_t)p * K;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) {
      if (k >= K) continue;
      const float v = tp[k];
      if (MODE == 0) mx[k] = max(mx[k], __float_as_uint(v) & 0x7fffffffu);
      else if (MODE == 1) s[k] += (long long)(int)__builtin_rint(__builtin_ldexp((double)v, sh[k]));  // |q| <= 2^30
      else mx[k] = max(mx[k], __float_as_uint(v - mean[k]) & 0x7fffffffu);
    }
  }
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) {
    if (k >= K) continue;
    if (MODE == 1) {
      if (s[k]) atomicAdd(&red[k], (unsigned long long)s[k]);
    } else if (mx[k]) {
      atomicMax(reinterpret_cast<uint32_t*>(&red[k]), mx[k]);
    }
  }
  __syncthreads();
  if (tid < K) {
    if (MODE == 1) {
      if (red[tid]) atomicAdd(&m.tsum[tid], red[tid]);
    } else {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(&red[tid]);
      if (v) atomicMax(MODE == 0 ? &m.tmax[tid] : &m.tcen[tid], v);
    }
  }
}

__global__ __launch_bounds__(HEAD_LANES) void head_tmean_kernel(PcaArgs a, HeadMomArgs m) {
  const uint32_t n = a.st->n;
  const int k = threadIdx.x;
  if (k >= m.K) return;
  float mu = 0.f;
  if (n > 0) {
    const double q = (double)(long long)m.tsum[k] / (double)n;
    mu = (float)__builtin_ldexp(q, f32_exponent(m.tmax[k]) - 30);
  }
  m.tmean[k] = mu;
}

// workgroup (x, y): rows [x * rows_per_group, + rows_per_group), columns 256 y .. 256 y + 255 of X, one to a lane
__global__ __launch_bounds__(HEAD_LANES) void head_cross_kernel(PcaArgs a, HeadMomArgs m, int rows_per_group) {
  __shared__ int4 vs4[HEAD_XROWS * (HEAD_KMAX / 4)];  // [64][16] quantised targets; 0 for an ineligible row
  __shared__ int els[HEAD_XROWS];
  int* vs = reinterpret_cast<int*>(vs4);
  const uint32_t n = a.st->n;
  if (n < 2) return;  // (uniform)
  const int bits = sum_bits(n);
  const int tid = threadIdx.x, K = m.K;
  const int j = blockIdx.y * HEAD_LANES + tid;
  const bool inj = j < a.stride;
  const float meanj = inj ? a.mean[j] : 0.f;
  const int shj = bits - (inj ? f32_exponent(a.cenmax[j]) : 0);
  // staging: the lane quantises target tid & 15 of rows (tid >> 4) + 16 i of a slab
  const int sk = tid & 15, sr = tid >> 4;
  const float meant = sk < K ? m.tmean[sk] : 0.f;
  const int sht = bits - (sk < K ? f32_exponent(m.tcen[sk]) : 0);
  const bool first = blockIdx.y == 0;  // these workgroups also sum the K x K block (lane = (k1, k2)) and R of the targets
  long long acc[HEAD_KMAX], tt = 0, rt = 0;
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) acc[k] = 0;
  const int64_t p_begin = (int64_t)blockIdx.x * rows_per_group;
  const int64_t p_end = min((int64_t)a.n_total, p_begin + rows_per_group);
  for (int64_t p0 = p_begin; p0 < p_end; p0 += HEAD_XROWS) {
    __syncthreads();  // the previous slab's reads are over
#pragma unroll
    for (int i = 0; i < HEAD_XROWS / 16; ++i) {
      const int r = sr + 16 * i;
      const int64_t p = p0 + r;
      const int e = p < p_end ? a.elig[p] : 0;
      int v = 0;
      if (e && sk < K) v = (int)__builtin_rint(__builtin_ldexp((double)(m.t[(size_t)p * K + sk] - meant), sht));
      vs[r * HEAD_KMAX + sk] = v;
      if (sk == 0) els[r] = e;
    }
    __syncthreads();
    const int nr = (int)min((int64_t)HEAD_XROWS, p_end - p0);
#pragma unroll 4
    for (int r = 0; r < nr; ++r) {
      if (!els[r]) continue;  // (uniform)
      int u = 0;
      if (inj) u = (int)__builtin_rint(__builtin_ldexp((double)(tile_row(a.rows, (uint32_t)(p0 + r), (uint32_t)a.chunk_rows, a.stride)[j] - meanj), shj));
      const int4 v0 = vs4[r * 4], v1 = vs4[r * 4 + 1], v2 = vs4[r * 4 + 2], v3 = vs4[r * 4 + 3];
      const int v[HEAD_KMAX] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k) acc[k] += (long long)u * (long long)v[k];
      if (first) {
        const int vi = vs[r * HEAD_KMAX + sr], vj = vs[r * HEAD_KMAX + sk];
        tt += (long long)vi * (long long)vj;
        if (sr == 0) rt += vj;
      }
    }
  }
  if (inj) {
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k)
      if (k < K && acc[k]) atomicAdd(&m.Txt[(size_t)j * HEAD_KMAX + k], (unsigned long long)acc[k]);
  }
  if (first) {
    if (sr < K && sk < K && tt) atomicAdd(&m.Ttt[sr * HEAD_KMAX + sk], (unsigned long long)tt);
    if (sr == 0 && sk < K && rt) atomicAdd(&m.Rt[sk], (unsigned long long)rt);
  }
}

// one lane per (i, k): column i < dim + K of [rows | t] against target k
__global__ __launch_bounds__(HEAD_LANES) void head_cross_finalise_kernel(PcaArgs a, HeadMomArgs m) {
  const uint32_t n = a.st->n;
  if (n < 2) return;
  const int K = m.K, D = a.dim + K;
  const int64_t e = (int64_t)blockIdx.x * HEAD_LANES + threadIdx.x;
  const int i = (int)(e / K), k = (int)(e % K);
  if (i >= D) return;
  const int bits = sum_bits(n);
  const bool x = i < a.dim;
  const int fi = f32_exponent(x ? a.cenmax[i] : m.tcen[i - a.dim]), fk = f32_exponent(m.tcen[k]);
  const double T = (double)(long long)(x ? m.Txt[(size_t)i * HEAD_KMAX + k] : m.Ttt[(i - a.dim) * HEAD_KMAX + k]);
  const double Ri = (double)(long long)(x ? a.R[i] : m.Rt[i - a.dim]), Rk = (double)(long long)m.Rt[k];
  const double prod = Ri * Rk;
  const double corr = prod / (double)n;
  const double diff = T - corr;
  m.cross[(size_t)i * K + k] = __builtin_ldexp(diff / (double)(n - 1), fi + fk - 2 * bits);
  if (i == a.dim + k) m.texp[k] = fk;
}

// The chains of NC columns of a pass for the lane's row: columns col0 + half * NC + i of `coef` ([n_col][m]); A: the leverage chain
// acc = fmaf(t, t, acc), t = z * S rounded once; else the prediction chain acc = fmaf(z, B, acc); components ascending
template <bool A, int NC>
__device__ __forceinline__ void head_chains(const HeadLooArgs& a, const float* __restrict__ coef, int col0, int n_col, int r0, int nrow, float* zs,
                                            float* cf, float (&acc)[NC]) {
  const int tid = threadIdx.x, row = tid & (HEAD_TILE - 1), half = tid >> 7, m = a.m;
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = 0.f;
  for (int c0 = 0; c0 < m; c0 += HEAD_SLAB) {
    const int cn = min(HEAD_SLAB, m - c0);
    __syncthreads();  // the previous slab's reads, or the epilogue's reads of the shared block, are over
    for (int e = tid; e < HEAD_TILE * HEAD_SLAB; e += HEAD_LANES) {
      const int r = e >> 5, c = e & 31;
      zs[c * HEAD_ZS + r] = r < nrow && c < cn ? a.z[(size_t)(r0 + r) * m + c0 + c] : 0.f;
    }
    for (int e = tid; e < HEAD_COLS * HEAD_SLAB; e += HEAD_LANES) {
      const int j = e >> 5, c = e & 31;
      cf[c * HEAD_CS + j] = col0 + j < n_col && c < cn ? coef[(size_t)(col0 + j) * m + c0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 2
    for (int c = 0; c < cn; ++c) {
      const float zv = zs[c * HEAD_ZS + row];
      const float* w = cf + c * HEAD_CS + half * NC;
#pragma unroll
      for (int q = 0; q < NC / 4; ++q) {
        const float4 w4 = *reinterpret_cast<const float4*>(w + 4 * q);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (A) {
            const float t = __fmul_rn(zv, wv[i]);
            acc[4 * q + i] = __builtin_fmaf(t, t, acc[4 * q + i]);
          } else {
            acc[4 * q + i] = __builtin_fmaf(zv, wv[i], acc[4 * q + i]);
          }
        }
      }
    }
  }
}

// workgroup x: tile x of the group, rows [128 x, 128 x + 128) of it
__global__ __launch_bounds__(HEAD_LANES) void head_loo_kernel(HeadLooArgs a) {
  __shared__ float4 un4[HEAD_UNION / 4];
  __shared__ float levs[HEAD_LMAX * HEAD_ZS];  // [l][row]
  __shared__ float ds[HEAD_KMAX * HEAD_ZS];    // [k][row] t - tmean
  __shared__ int el[HEAD_TILE];
  float* un = reinterpret_cast<float*>(un4);
  float* zs = un;                          // [32][129] z slab, component-major
  float* cf = un + HEAD_SLAB * HEAD_ZS;    // [32][68] coefficient slab, component-major
  float* ps = un;                          // [64][129] e, then r, of the pass's columns
  const int tid = threadIdx.x, row = tid & (HEAD_TILE - 1), half = tid >> 7;
  const int L = a.L, K = a.K, LK = L * K, Q = 3 * LK + L + 1;
  const int r0 = blockIdx.x * HEAD_TILE, nrow = min(HEAD_TILE, a.n - r0);
  const int64_t pos0 = (int64_t)a.first + r0;
  double* part = a.part + (size_t)(a.first / HEAD_TILE + blockIdx.x) * Q;
  if (tid < HEAD_TILE) el[tid] = tid < nrow ? a.elig[pos0 + tid] : 0;
  for (int e = tid; e < HEAD_TILE * K; e += HEAD_LANES) {
    const int r = e / K, k = e - r * K;
    ds[k * HEAD_ZS + r] = r < nrow ? __fsub_rn(a.t[(size_t)(pos0 + r) * K + k], a.tmean[k]) : 0.f;
  }
  {
    float acc[16];
    head_chains<true, 16>(a, a.scale, 0, L, r0, nrow, zs, cf, acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int l = half * 16 + i;
      if (l < L) levs[l * HEAD_ZS + row] = __fadd_rn(a.lev0, acc[i]);
    }
  }
  __syncthreads();
  if (tid < L) {
    double s = 0.0;
    for (int r = 0; r < nrow; ++r)
      if (el[r]) s += (double)levs[tid * HEAD_ZS + r];
    part[3 * LK + tid] = s;
  } else if (tid == HEAD_COLS) {
    int c = 0;
    for (int r = 0; r < nrow; ++r) c += el[r];
    part[3 * LK + L] = (double)c;
  }
  const bool live = el[row] != 0;
  for (int col0 = 0; col0 < LK; col0 += HEAD_COLS) {
    float acc[32];
    head_chains<false, 32>(a, a.coef, col0, LK, r0, nrow, zs, cf, acc);
    const int o0 = col0 + half * 32;
    {
      int l = o0 / K, k = o0 - l * K;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        acc[i] = o0 + i < LK ? __fsub_rn(ds[k * HEAD_ZS + row], acc[i]) : 0.f;  // e
        if (++k == K) k = 0, ++l;
      }
    }
    __syncthreads();  // every lane is behind its chains: the slabs may go
#pragma unroll
    for (int i = 0; i < 32; ++i) ps[(half * 32 + i) * HEAD_ZS + row] = acc[i];
    __syncthreads();
    const int o = col0 + tid;
    if (tid < HEAD_COLS && o < LK) {
      double fit = 0.0;
      for (int r = 0; r < nrow; ++r) {
        if (!el[r]) continue;
        const double e = (double)ps[tid * HEAD_ZS + r];
        fit += e * e;
      }
      part[2 * LK + o] = fit;
    }
    __syncthreads();
    {
      int l = o0 / K, k = o0 - l * K;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        float rv = 0.f;
        if (o0 + i < LK) {
          const float lev = levs[l * HEAD_ZS + row];
          rv = lev < 1.f ? (float)((double)acc[i] / (1.0 - (double)lev)) : __builtin_inff();
          if (a.resid && live && a.resid_l[k] == l) a.resid[(size_t)(pos0 + row) * K + k] = rv;
        }
        ps[(half * 32 + i) * HEAD_ZS + row] = rv;
        if (++k == K) k = 0, ++l;
      }
    }
    __syncthreads();
    if (tid < HEAD_COLS && o < LK) {
      double sse = 0.0, sae = 0.0;
      for (int r = 0; r < nrow; ++r) {
        if (!el[r]) continue;
        const double rv = (double)ps[tid * HEAD_ZS + r];
        sse += rv * rv;
        sae += __builtin_fabs(rv);
      }
      part[o] = sse;
      part[LK + o] = sae;
    }
  }
}

// one lane per quantity: the tiles' partials added in tile order
__global__ __launch_bounds__(HEAD_LANES) void head_sum_kernel(const double* part, int n_tile, int Q, double* out) {
  const int q = blockIdx.x * HEAD_LANES + threadIdx.x;
  if (q >= Q) return;
  double s = 0.0;
  for (int g = 0; g < n_tile; ++g) s += part[(size_t)g * Q + q];
  out[q] = s;
}

// one lane per (row, target)
__global__ __launch_bounds__(HEAD_LANES) void head_eval_kernel(HeadEvalArgs a) {
  const int64_t e = (int64_t)blockIdx.x * HEAD_LANES + threadIdx.x;
  if (e >= (int64_t)a.n * a.K) return;
  const int64_t p = e / a.K;
  const int k = (int)(e - p * a.K);
  a.pred[e] = __fadd_rn(a.tmean[k], a.w[e]);
  const float* z = a.z + (size_t)p * a.m;
  const float* s = a.scale + (size_t)k * a.m;
  float acc = 0.f;
  for (int c = 0; c < a.m; ++c) {
    const float v = __fmul_rn(z[c], s[c]);
    acc = __builtin_fmaf(v, v, acc);
  }
  a.lev[e] = __fadd_rn(a.lev0, acc);
}

}  // namespace

hipError_t launch_head_mask(const float* const* rows, int32_t chunk_rows, int32_t stride, int32_t n_total, const float* t, int32_t K, uint8_t* mask,
                            hipStream_t s) {
  if (n_total <= 0) return hipSuccess;
  const int n_pass = (n_total + 31) / 32;
  hipLaunchKernelGGL(head_mask_kernel, dim3((unsigned)std::min(n_pass, 2048)), dim3(HEAD_LANES), 0, s, rows, chunk_rows, stride, n_total, t, K, mask);
  return hipGetLastError();
}

hipError_t launch_head_moments(const PcaArgs& a, const HeadMomArgs& m, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  const unsigned n_g = (unsigned)std::min<int64_t>(HEAD_GROUPS, ((int64_t)a.n_total + HEAD_LANES - 1) / HEAD_LANES);
  hipLaunchKernelGGL(head_tstat_kernel<0>, dim3(n_g), dim3(HEAD_LANES), 0, s, a, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(head_tstat_kernel<1>, dim3(n_g), dim3(HEAD_LANES), 0, s, a, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(head_tmean_kernel, dim3(1), dim3(HEAD_LANES), 0, s, a, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(head_tstat_kernel<2>, dim3(n_g), dim3(HEAD_LANES), 0, s, a, m);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int ny = (a.stride + HEAD_LANES - 1) / HEAD_LANES, want = std::max(1, HEAD_GROUPS / ny);
  const int64_t rpg = std::max<int64_t>(HEAD_XROWS, (((int64_t)a.n_total + want - 1) / want + HEAD_XROWS - 1) / HEAD_XROWS * HEAD_XROWS);
  const unsigned n_rg = (unsigned)(((int64_t)a.n_total + rpg - 1) / rpg);
  hipLaunchKernelGGL(head_cross_kernel, dim3(n_rg, (unsigned)ny), dim3(HEAD_LANES), 0, s, a, m, (int)rpg);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t n_el = (int64_t)(a.dim + m.K) * m.K;
  hipLaunchKernelGGL(head_cross_finalise_kernel, dim3((unsigned)((n_el + HEAD_LANES - 1) / HEAD_LANES)), dim3(HEAD_LANES), 0, s, a, m);
  return hipGetLastError();
}

hipError_t launch_head_loo(const HeadLooArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(head_loo_kernel, dim3((unsigned)((a.n + HEAD_TILE - 1) / HEAD_TILE)), dim3(HEAD_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_head_sum(const double* part, int32_t n_tile, int32_t Q, double* out, hipStream_t s) {
  hipLaunchKernelGGL(head_sum_kernel, dim3((unsigned)((Q + HEAD_LANES - 1) / HEAD_LANES)), dim3(HEAD_LANES), 0, s, part, n_tile, Q, out);
  return hipGetLastError();
}

hipError_t launch_head_eval(const HeadEvalArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int64_t n_el = (int64_t)a.n * a.K;
  hipLaunchKernelGGL(head_eval_kernel, dim3((unsigned)((n_el + HEAD_LANES - 1) / HEAD_LANES)), dim3(HEAD_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

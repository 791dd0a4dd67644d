// Principal-component map of a latent-space index (scann_index_moments, scann_index_project, scann_project_batch, include/scann_hip.h),
// bit-reproducible: mean and covariance depend on the index contents only, a projected row on the row and the projection only.
//   mean        mean_j = (float) ldexp((double) S_j / (double) n, e_j - 30): the k-means update with one cluster (scann_kmeans.hip);
//   scatter     T[i][j] = the int64 sum over the eligible rows of u_i * u_j,  u_j = llrint(ldexp((double)(x_j - mean_j), b - f_j)),
//               |u| <= 2^b, b = min(24, (62 - L) / 2) for n < 2^L: no partial sum reaches 2^62, so the sum is the same in any order and
//               neither the launch geometry nor the chunking enters it;  R_j = the sum of u_j;
//   covariance  fp64, one expression per (i, j) from T, R and n;
//   projection  z_c = the fp32 chain acc = fmaf(x[j] - mean[j], W[c][j], acc) over the columns ascending, the difference rounded once.
// The moments are six launches on one stream; the host waits once, behind the last:
//   pca_prepare_kernel     a row is eligible iff all its components are finite (and, with a mask, its mask byte is set: the targets of
//                          scann_index_fit_moments, scann_head.hip); their count; the column maxima of |x| over the eligible
//                          rows by integer max on the bit patterns (kmeans_prepare_kernel's pass).
//   pca_pass_kernel<0>     S_j: a lane owns 4 columns of every R-th row of its workgroup's range and sums q in registers; one LDS add
//                          and one global 64-bit integer atomic per column and workgroup.
//   pca_mean_kernel        the mean.
//   pca_pass_kernel<1>     the column maxima of |x - mean| (fp32, rounded once), the same pass with an integer max.
//   pca_scatter_kernel     the hot path: N * dim^2 / 2 exact 32 x 32 + 64-bit multiply-adds.  A workgroup owns one 64 x 64 block (I, J),
//                          I <= J, of the column-block pairs and a range of rows.  It quantises the rows on the fly (read fp32, subtract
//                          the mean, scale, round) into LDS slabs of int32, 32 rows at a time, the next slab's loads in flight
//                          meanwhile; a lane owns a 4 x 4 block of int64 accumulators in registers and adds it to T once, at the end,
//                          with 64-bit integer atomics.  R_j comes from the diagonal blocks (16 lanes of the first wave).
//   pca_finalise_kernel    the covariance, one lane per (i, j), i <= j, mirrored; f_j.
// The projection runs on the tile and the slab pipeline of scann_tile.h in the product form: a workgroup takes tiles of 128 rows (the
// tile's "queries") and walks the components 64 at a time (its "rows"); the centred value is formed once, where the row is
// fetched.  dist2 (the difference-form chain against the mean) rides along in the first
// component block, in the 16 lanes that own component group 0; pca_md2_kernel is a small pass over the coordinates, one lane per row.
// No float atomics, no scratch.
#include "scann_pca.h"

#include <algorithm>

namespace scann {

namespace {

// the eligibility scan with the column maxima (scann_prim.h); the barriers of eligible_scan_colmax also order the count
__global__ __launch_bounds__(PCA_LANES) void pca_prepare_kernel(PcaArgs a) {
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  eligible_scan_colmax<PCA_LANES>(
      a.rows, a.chunk_rows, a.stride, a.n_total, a.colmax, [&](int p, int) { return a.mask ? !a.mask[p] : 0; },
      [&](int p, int bad) {
        a.elig[p] = bad ? 0 : 1;
        if (!bad) atomicAdd(&cnt, 1u);
      });
  if (threadIdx.x == 0 && cnt) atomicAdd(&a.st->n, cnt);
}

// MODE 0: S_j += q(x, j); MODE 1: cenmax_j = max |x - mean_j|.  Workgroup x: rows [x * rows_per_group, + rows_per_group); lane t:
// columns 4 (t % cgs) .. + 3 of the rows t / cgs, + R, ... of the range, cgs = stride / 4 column groups, R = 256 / cgs rows to a pass
template <int MODE>
__global__ __launch_bounds__(PCA_LANES) void pca_pass_kernel(PcaArgs a, int rows_per_group) {
  __shared__ unsigned long long red[1024];
  const int t = threadIdx.x, cgs = a.stride >> 2, R = PCA_LANES / cgs, col = 4 * (t % cgs), rsub = t / cgs;
  for (int j = t; j < a.stride; j += PCA_LANES) red[j] = 0;
  __syncthreads();
  long long s[4] = {0, 0, 0, 0};
  uint32_t mx[4] = {0, 0, 0, 0};
  int sh[4];
  float mean[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sh[j] = 30 - f32_exponent(a.colmax[col + j]);
    mean[j] = MODE == 1 ? a.mean[col + j] : 0.f;
  }
  const int64_t p_end = min((int64_t)a.n_total, ((int64_t)blockIdx.x + 1) * rows_per_group);
  if (rsub < R) {
    for (int64_t p0 = (int64_t)blockIdx.x * rows_per_group + rsub; p0 < p_end; p0 += 4 * R) {
      int el[4];
      float4 x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t p = p0 + (int64_t)i * R;
        el[i] = p < p_end ? a.elig[p] : 0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (el[i]) x[i] = *reinterpret_cast<const float4*>(tile_row(a.rows, (uint32_t)(p0 + (int64_t)i * R), (uint32_t)a.chunk_rows, a.stride) + col);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!el[i]) continue;
        const float xv[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (MODE == 0) s[j] += (long long)(int)__builtin_rint(__builtin_ldexp((double)xv[j], sh[j]));  // |q| <= 2^30
          else mx[j] = max(mx[j], __float_as_uint(xv[j] - mean[j]) & 0x7fffffffu);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (MODE == 0) {
        if (s[j]) atomicAdd(&red[col + j], (unsigned long long)s[j]);
      } else if (mx[j]) {
        atomicMax(reinterpret_cast<uint32_t*>(&red[col + j]), mx[j]);
      }
    }
  }
  __syncthreads();
  for (int j = t; j < a.stride; j += PCA_LANES) {
    if (MODE == 0) {
      if (red[j]) atomicAdd(&a.sums[j], red[j]);
    } else {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(&red[j]);
      if (v) atomicMax(&a.cenmax[j], v);
    }
  }
}

__global__ __launch_bounds__(PCA_LANES) void pca_mean_kernel(PcaArgs a) {
  const uint32_t n = a.st->n;
  for (int j = threadIdx.x; j < a.stride; j += PCA_LANES) {
    float m = 0.f;
    if (n > 0) {
      const double q = (double)(long long)a.sums[j] / (double)n;  // both conversions and the division round to nearest
      m = (float)__builtin_ldexp(q, f32_exponent(a.colmax[j]) - 30);
    }
    a.mean[j] = m;
  }
}

// workgroup (x, y): rows [x * rows_per_group, + rows_per_group), block pair y = (I, J), I <= J, in row-major order of the upper triangle
__global__ __launch_bounds__(PCA_LANES) void pca_scatter_kernel(PcaArgs a, int rows_per_group) {
  __shared__ int4 sa[PCA_ROWS * (PCA_BLK / 4)], sb[PCA_ROWS * (PCA_BLK / 4)];
  const uint32_t n = a.st->n;
  if (n < 2) return;  // (uniform)
  const int bits = sum_bits(n);
  const int t = threadIdx.x, ti = t & 15, tj = t >> 4;
  const int stride = a.stride, nb = (stride + PCA_BLK - 1) / PCA_BLK;
  int I = 0, rem = blockIdx.y;
  while (rem >= nb - I) rem -= nb - I, ++I;
  const int J = I + rem;
  const bool diag = I == J;
  // staging: the lane quantises columns 4 (t & 15) .. + 3 of both blocks in rows t >> 4 and 16 + (t >> 4) of a slab
  const int colA = I * PCA_BLK + 4 * ti, colB = J * PCA_BLK + 4 * ti;
  const bool inA = colA < stride, inB = !diag && colB < stride;
  float meanA[4], meanB[4];
  int shA[4], shB[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    meanA[j] = inA ? a.mean[colA + j] : 0.f;
    shA[j] = bits - (inA ? f32_exponent(a.cenmax[colA + j]) : 0);
    meanB[j] = inB ? a.mean[colB + j] : 0.f;
    shB[j] = bits - (inB ? f32_exponent(a.cenmax[colB + j]) : 0);
  }
  const int64_t p_begin = (int64_t)blockIdx.x * rows_per_group;
  const int64_t p_end = min((int64_t)a.n_total, p_begin + rows_per_group);
  const int n_slab = (int)((p_end - p_begin + PCA_ROWS - 1) / PCA_ROWS);
  float4 gA[2], gB[2];
  int el[2];
  auto fetch = [&](int slab) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t p = p_begin + (int64_t)slab * PCA_ROWS + tj + 16 * i;
      el[i] = p < p_end ? a.elig[p] : 0;
      gA[i] = gB[i] = float4{0.f, 0.f, 0.f, 0.f};
      if (el[i]) {
        const float* row = tile_row(a.rows, (uint32_t)p, (uint32_t)a.chunk_rows, stride);
        if (inA) gA[i] = *reinterpret_cast<const float4*>(row + colA);
        if (inB) gB[i] = *reinterpret_cast<const float4*>(row + colB);
      }
    }
  };
  // exact scaling of the centred value (fp32, rounded once), then round to nearest even; |u| <= 2^24, so the conversion is one instruction
  auto quant = [](float4 x, const float* mean, const int* sh, bool on) {
    int4 u{0, 0, 0, 0};
    if (on) {
      u.x = (int)__builtin_rint(__builtin_ldexp((double)(x.x - mean[0]), sh[0]));
      u.y = (int)__builtin_rint(__builtin_ldexp((double)(x.y - mean[1]), sh[1]));
      u.z = (int)__builtin_rint(__builtin_ldexp((double)(x.z - mean[2]), sh[2]));
      u.w = (int)__builtin_rint(__builtin_ldexp((double)(x.w - mean[3]), sh[3]));
    }
    return u;
  };
  long long acc[4][4], racc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;
  const int4* pb = diag ? sa : sb;
  const bool sums_r = diag && tj == 0;  // (the first 16 lanes of the first wave)
  if (n_slab > 0) fetch(0);
  for (int slab = 0; slab < n_slab; ++slab) {
    __syncthreads();  // the previous slab's reads are over
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa[(tj + 16 * i) * (PCA_BLK / 4) + ti] = quant(gA[i], meanA, shA, el[i] && inA);
      if (!diag) sb[(tj + 16 * i) * (PCA_BLK / 4) + ti] = quant(gB[i], meanB, shB, el[i] && inB);
    }
    __syncthreads();
    if (slab + 1 < n_slab) fetch(slab + 1);
#pragma unroll 8
    for (int r = 0; r < PCA_ROWS; ++r) {
      const int4 av = sa[r * (PCA_BLK / 4) + ti], bv = pb[r * (PCA_BLK / 4) + tj];
      const int ai[4] = {av.x, av.y, av.z, av.w}, bj[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += (long long)ai[i] * (long long)bj[j];
      if (sums_r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) racc[i] += ai[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ci = I * PCA_BLK + 4 * ti + i;
    if (ci >= stride) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cj = J * PCA_BLK + 4 * tj + j;
      if (cj < stride && acc[i][j]) atomicAdd(&a.T[(size_t)ci * stride + cj], (unsigned long long)acc[i][j]);
    }
    if (sums_r && racc[i]) atomicAdd(&a.R[ci], (unsigned long long)racc[i]);
  }
}

// one lane per (i, j), i <= j < dim
__global__ __launch_bounds__(PCA_LANES) void pca_finalise_kernel(PcaArgs a) {
#pragma clang fp contract(off)
  const uint32_t n = a.st->n;
  if (n < 2) return;
  const int64_t e = (int64_t)blockIdx.x * PCA_LANES + threadIdx.x;
  const int i = (int)(e / a.dim), j = (int)(e % a.dim);
  if (i >= a.dim || i > j) return;
  const int bits = sum_bits(n);
  const int fi = f32_exponent(a.cenmax[i]), fj = f32_exponent(a.cenmax[j]);
  const double T = (double)(long long)a.T[(size_t)i * a.stride + j];
  const double Ri = (double)(long long)a.R[i], Rj = (double)(long long)a.R[j];
  const double prod = Ri * Rj;
  const double corr = prod / (double)n;
  const double diff = T - corr;
  const double c = __builtin_ldexp(diff / (double)(n - 1), fi + fj - 2 * bits);
  a.cov[(size_t)i * a.dim + j] = c;
  a.cov[(size_t)j * a.dim + i] = c;
  if (i == j) a.col_exp[i] = fi;
}

__global__ __launch_bounds__(PCA_LANES) void pca_project_kernel(PcaProjArgs a, int n_tile) {
  __shared__ float4 pca_smem[TILE_SLABS / 4];
  float* sm = reinterpret_cast<float*>(pca_smem);
  float* ps = sm;                             // the slab of centred rows ...
  float* cs = sm + tile_slab_floats(PCA_TP);  // ... and the component slab (tile_stage)
  const int t = threadIdx.x, pg = t & 15, cg = t >> 4;
  const int m = a.m, stride = a.stride;
  const int n_slab = (stride + PCA_SLAB - 1) / PCA_SLAB;
  const int n_step = ((m + PCA_TC - 1) / PCA_TC) * n_slab;  // (component block, slab) steps of a tile
  const float* __restrict__ comp = a.comp;
  const float* __restrict__ mean = a.mean;
  const bool want_d2 = a.dist2 != nullptr && t < 16;  // (component group 0: 16 lanes of the first wave)
  for (int tile = blockIdx.x; tile < n_tile; tile += gridDim.x) {
    const int r0 = tile * PCA_TP, nrow = min(PCA_TP, a.n - r0);
    // the lane stages rows (t >> 3) + 32 i of the tile
    const float* rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int item = (t >> 3) + 32 * i;
      rp[i] = item < nrow ? tile_row(a.rows, (uint32_t)((int64_t)a.first + r0 + item), (uint32_t)a.chunk_rows, stride) : nullptr;
    }
    // one step's slab in registers: 128 rows x 8 and 64 components x 8 float4 (four columns of one item each); items / columns beyond the
    // end are zero.  The rows are centred here: x - mean in fp32, rounded once.  Step s + 1 is fetched while step s is computed
    float4 gp[4], gc[2];
    auto fetch = [&](int step) {
      const int c0 = (step / n_slab) * PCA_TC, col = (step % n_slab) * PCA_SLAB + 4 * (t & 7);
      float4 mu{0.f, 0.f, 0.f, 0.f};
      if (col < stride) mu = *reinterpret_cast<const float4*>(mean + col);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gp[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (rp[i] && col < stride) {
          const float4 x = *reinterpret_cast<const float4*>(rp[i] + col);
          gp[i] = float4{x.x - mu.x, x.y - mu.y, x.z - mu.z, x.w - mu.w};
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int item = (t >> 3) + 32 * i;
        gc[i] = c0 + item < m && col < stride ? *reinterpret_cast<const float4*>(comp + (size_t)(c0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
        // the chains of the definition end at column dim - 1.  Behind it the centred value is +0, and with a component of -0 the product is
        // -0, which leaves every accumulator as it is, -0.0 included (with +0 an accumulator of -0.0 would become +0.0)
        if (col + 3 >= a.dim) {
          if (col >= a.dim) gc[i].x = -0.f;
          if (col + 1 >= a.dim) gc[i].y = -0.f;
          if (col + 2 >= a.dim) gc[i].z = -0.f;
          gc[i].w = -0.f;
        }
      }
    };
    f2 acc[8][2];
    float dacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f}, dacc[j] = 0.f;
    fetch(0);
    for (int step = 0; step < n_step; ++step) {
      __syncthreads();  // the previous slab's reads are over
      tile_stage<PCA_LANES, 4, PCA_TP>(ps, gp, t);
      tile_stage<PCA_LANES, 2, PCA_TC>(cs, gc, t);
      __syncthreads();
      if (step + 1 < n_step) fetch(step + 1);
      tile_slab<TileForm::PROD>(ps, cs, pg, cg, acc, PCA_SLAB);
      if (want_d2 && step < n_slab) {  // the first component block: the distance to the mean, the difference-form chain (the rows are centred)
#pragma unroll 4
        for (int c = 0; c < PCA_SLAB; ++c) {
          float pv[8];
          tile_queries(ps, c, pg, pv);
#pragma unroll
          for (int j = 0; j < 8; ++j) dacc[j] = __builtin_fmaf(pv[j], pv[j], dacc[j]);
        }
      }
      if (step % n_slab != n_slab - 1) continue;
      // the component block's last slab: the lane's 8 x 4 coordinates
      const int c0 = (step / n_slab) * PCA_TC + 4 * cg;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = tile_query(pg, j);
        if (row < nrow) {
          float* out = a.coords + (size_t)(r0 + row) * m;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c0 + i < m) out[c0 + i] = tile_at(acc, j, i);
          if (want_d2 && step < n_slab) a.dist2[r0 + row] = dacc[j];
        }
        acc[j][0] = acc[j][1] = f2{0.f, 0.f};
      }
    }
  }
}

// one lane per row: md2 = the chain over the components ascending of (z_c * s_c)^2, the product rounded once
__global__ __launch_bounds__(PCA_LANES) void pca_md2_kernel(PcaProjArgs a) {
  const int64_t p = (int64_t)blockIdx.x * PCA_LANES + threadIdx.x;
  if (p >= a.n) return;
  const float* z = a.coords + (size_t)p * a.m;
  float acc = 0.f;
  for (int c = 0; c < a.m; ++c) {
    const float v = __fmul_rn(z[c], a.scale[c]);
    acc = __builtin_fmaf(v, v, acc);
  }
  a.md2[p] = acc;
}

}  // namespace

hipError_t launch_pca_moments(const PcaArgs& a, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  const int n_pass = (a.n_total + 31) / 32;
  hipLaunchKernelGGL(pca_prepare_kernel, dim3((unsigned)std::min(n_pass, 2048)), dim3(PCA_LANES), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // whole steps of 4 passes of 256 / (stride / 4) rows, at least 4 of them to a workgroup
  const int pass = 4 * (PCA_LANES / (a.stride / 4));
  const int64_t rpg = std::max<int64_t>(4 * pass, (((int64_t)a.n_total + PCA_GROUPS - 1) / PCA_GROUPS + pass - 1) / pass * pass);
  const unsigned n_rg = (unsigned)(((int64_t)a.n_total + rpg - 1) / rpg);
  hipLaunchKernelGGL(pca_pass_kernel<0>, dim3(n_rg), dim3(PCA_LANES), 0, s, a, (int)rpg);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pca_mean_kernel, dim3(1), dim3(PCA_LANES), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pca_pass_kernel<1>, dim3(n_rg), dim3(PCA_LANES), 0, s, a, (int)rpg);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int nb = (a.stride + PCA_BLK - 1) / PCA_BLK, n_pair = nb * (nb + 1) / 2;
  const int want = std::max(1, PCA_GROUPS / n_pair);
  const int64_t spg = std::max<int64_t>(PCA_ROWS, (((int64_t)a.n_total + want - 1) / want + PCA_ROWS - 1) / PCA_ROWS * PCA_ROWS);
  const unsigned n_sg = (unsigned)(((int64_t)a.n_total + spg - 1) / spg);
  hipLaunchKernelGGL(pca_scatter_kernel, dim3(n_sg, (unsigned)n_pair), dim3(PCA_LANES), 0, s, a, (int)spg);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t n_el = (int64_t)a.dim * a.dim;
  hipLaunchKernelGGL(pca_finalise_kernel, dim3((unsigned)((n_el + PCA_LANES - 1) / PCA_LANES)), dim3(PCA_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pca_project(const PcaProjArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int n_tile = (a.n + PCA_TP - 1) / PCA_TP;
  // the tiles dealt evenly over at most PCA_MAX_GROUPS workgroups
  const int per = (n_tile + PCA_MAX_GROUPS - 1) / PCA_MAX_GROUPS, groups = (n_tile + per - 1) / per;
  hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)groups), dim3(PCA_LANES), 0, s, a, n_tile);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.md2) return e;
  hipLaunchKernelGGL(pca_md2_kernel, dim3((unsigned)((a.n + PCA_LANES - 1) / PCA_LANES)), dim3(PCA_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

// k-means (Lloyd's iteration) over a latent-space index (scann_index_kmeans, include/scann_hip.h), bit-reproducible: labels and centres
// depend on the index contents and the initial centres only.
//   assignment  label[p] = the first centre under the total order (dist2 ascending, centre index ascending), dist2 the chain of
//               scann_knn.hip:  acc_{j+1} = fmaf(P[p][j] - C[c][j], P[p][j] - C[c][j], acc_j), fp32, columns ascending;
//   update      C[c][j] = (float) ldexp((double) S[c][j] / (double) n_c, e_j - 30),  S[c][j] the int64 sum over the cluster's rows of
//               q(x, j) = llrint(ldexp((double) x, 30 - e_j)),  e_j the frexp exponent of the column's largest |x| over the eligible rows.
// The sum is an integer sum: it does not depend on the order of the adds, so neither on the launch geometry nor on the chunking.  Its
// error against the exact mean is at most 2^(e_j - 31) per component, 128 times finer than an fp32 ulp at the top of the column's range.
//
// kmeans_prepare_kernel (once): a row is eligible iff all its components are finite; labels = -1, dist2 = +inf; the column maxima of
// |x| over the eligible rows by integer max on the bit patterns (order-free), first in LDS, then one atomic per column and workgroup.
// kmeans_gather_kernel (init_pos only): the initial centres copied from the pool's rows on the device.
// A round t is three launches on one stream; the host enqueues every round and waits once.  t is a launch argument, everything else
// (done, changed_t) travels through device memory, and a launch after `done` returns at its first instruction:
//   kmeans_assign_kernel    the hot path, on the tile and the slab pipeline of scann_tile.h: a workgroup takes tiles of 128 pool rows
//                           (the tile's "queries": the rows are the many side here) and walks the centres 64 at a time (its "rows"); a
//                           lane's block is 8 rows x 4 centres.  A lane keeps the first centre under the order for each of
//                           its 8 rows over the centres it visits -- ascending, so a strict < keeps the lower index --, and the 16 lanes
//                           of a row are reduced once per tile by comparisons of (dist2, index).  The distance matrix is never written.
//                           It writes label / dist2 and counts the rows whose label changed: one integer add per workgroup.
//   kmeans_sum_kernel       the update's sums, as a pass of its own over the rows (4 bytes read per component): a workgroup takes a
//                           range of rows and a group of `cols` columns, k x cols int64 sums live in its LDS (ds_add_u64: a lane adds
//                           4 columns of a row, a wave 256 / cols rows, so two lanes meet only where two of those rows share a cluster;
//                           8 rows of 16 bytes are in flight per lane: at 2 workgroups per CU the loads' latency bounds it otherwise), and at the
//                           end it adds its non-zero sums to global memory with 64-bit integer atomics: workgroups x k x cols x 8
//                           bytes instead of N x dim x 8.  Returns at once in the round that ends the loop.
//   kmeans_finalise_kernel  one workgroup per centre: ends the loop (changed_t <= stop_changed or t == max_iter), or forms the new centre
//                           with an fp64 division, correctly rounded, and zeroes the sums and the count.
// No float atomics, no scratch.  Nothing is read within the launch that wrote it, except atomically added integers that the next
// launch reads: the stream orders the launches.
#include "scann_kmeans.h"

#include <algorithm>

namespace scann {

namespace {

constexpr int KM_ASSIGN_SMEM = TILE_SLABS + 4 * KM_TP * 2;  // floats of the two slabs, then per wave and row the wave's first centre (dist2, index)

__device__ __forceinline__ int km_slot(int t) { return t & (KM_ROUNDS - 1); }
// the loop ends with round t's assignment
__device__ __forceinline__ bool km_last_round(const KmArgs& a, int t, uint32_t changed) {
  return (int64_t)changed <= a.stop_changed || t >= a.max_iter;
}

// the eligibility scan with the column maxima (scann_prim.h)
__global__ __launch_bounds__(KM_LANES) void kmeans_prepare_kernel(KmArgs a) {
  eligible_scan_colmax<KM_LANES>(a.rows, a.chunk_rows, a.stride, a.n_total, a.colmax, NoExtra{}, [&](int p, int bad) {
    a.elig[p] = bad ? 0 : 1;
    a.labels[p] = -1;
    a.dist2[p] = __builtin_inff();
  });
}

// one workgroup per centre
__global__ __launch_bounds__(KM_LANES) void kmeans_gather_kernel(KmArgs a) {
  const int c = blockIdx.x, p = a.init_pos[c];
  if (!a.elig[p]) {  // (uniform)
    if (threadIdx.x == 0) {
      atomicMax(&a.st->bad_init, a.k - c);  // the first such place is k - bad_init
      a.st->done = 1;
    }
    return;
  }
  const float* row = tile_row(a.rows, p, a.chunk_rows, a.stride);
  for (int j = threadIdx.x; j < a.stride; j += KM_LANES) a.centres[(size_t)c * a.stride + j] = row[j];
}

// (d, l) before (e, m) in the total order; l < 0: no centre yet, behind every other.  The last line is dist_before (scann_prim.h)
// written out: behind the call hipcc compiles kmeans_assign_kernel's reduction to branches on the exec mask in place of selects, and at
// k = 256 a call of five rounds over 2.4 M rows then takes 1 % longer (profiles/primitives_refactor.txt, section 5)
__device__ __forceinline__ bool km_before(float d, int32_t l, float e, int32_t m) {
  if (l < 0) return false;
  if (m < 0) return true;
  return d < e || (d == e && l < m);
}

__global__ __launch_bounds__(KM_LANES) void kmeans_assign_kernel(KmArgs a, int round) {
  __shared__ float4 km_smem[KM_ASSIGN_SMEM / 4];
  if (a.st->done) return;  // (uniform)
  float* sm = reinterpret_cast<float*>(km_smem);
  float* ps = sm;                               // the row slab ...
  float* cs = sm + tile_slab_floats(KM_TP);     // ... and the centre slab (tile_stage)
  float* red_d = sm + TILE_SLABS;                // [4][128] the waves' first centres of the tile's rows ...
  int32_t* red_l = reinterpret_cast<int32_t*>(red_d + 4 * KM_TP);  // ... and their indices
  const int t = threadIdx.x, pg = t & 15, cg = t >> 4;
  const int k = a.k, stride = a.stride;
  const int n_slab = (stride + KM_SLAB - 1) / KM_SLAB;
  const int n_step = ((k + KM_TC - 1) / KM_TC) * n_slab;  // (centre block, slab) steps of a tile
  const float* __restrict__ centres = a.centres;
  int n_changed = 0;  // (lane 0's is the workgroup's)
  for (int tile = blockIdx.x; tile < a.n_tile; tile += gridDim.x) {
    const int chunk = tile / a.tiles_per_chunk, r0 = (tile % a.tiles_per_chunk) * KM_TP;
    const int nrow = min(a.chunk_rows, a.n_total - chunk * a.chunk_rows) - r0;  // <= 0: a tile behind the chunk's last row
    if (nrow <= 0) continue;  // (uniform)
    const float* __restrict__ rows = a.rows[chunk];
    // one step's slab in registers: 128 rows x 8 and 64 centres x 8 float4 (four columns of one item each); items / columns beyond the
    // end are zero.  Step s + 1 is fetched while step s is computed
    float4 gp[4], gc[2];
    auto fetch = [&](int step) {
      const int c0 = (step / n_slab) * KM_TC, col0 = (step % n_slab) * KM_SLAB;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = t + KM_LANES * i, item = e >> 3, col = col0 + 4 * (e & 7);
        gp[i] = item < nrow && col < stride ? *reinterpret_cast<const float4*>(rows + (size_t)(r0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = t + KM_LANES * i, item = e >> 3, col = col0 + 4 * (e & 7);
        gc[i] = c0 + item < k && col < stride ? *reinterpret_cast<const float4*>(centres + (size_t)(c0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
      }
    };
    f2 acc[8][2];
    float bd[8];
    int32_t bl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f}, bd[j] = __builtin_inff(), bl[j] = -1;
    fetch(0);
    for (int step = 0; step < n_step; ++step) {
      __syncthreads();  // the previous slab's reads (and the previous tile's reduction) are over
      tile_stage<KM_LANES, 4, KM_TP>(ps, gp, t);
      tile_stage<KM_LANES, 2, KM_TC>(cs, gc, t);
      __syncthreads();
      if (step + 1 < n_step) fetch(step + 1);
      tile_slab<TileForm::DIFF>(ps, cs, pg, cg, acc, KM_SLAB);  // the row first
      if (step % n_slab != n_slab - 1) continue;
      // the centre block's last slab: the lane's 4 centres, ascending, against the first so far of each of its 8 rows
      const int c0 = (step / n_slab) * KM_TC + 4 * cg;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = tile_at(acc, j, i);
          // a NaN distance never qualifies; the first centre that does is taken whatever its distance (+inf is ordered)
          if (c0 + i < k && d == d && (bl[j] < 0 || d < bd[j])) bd[j] = d, bl[j] = c0 + i;
        }
        acc[j][0] = acc[j][1] = f2{0.f, 0.f};
      }
    }
    // the 16 lanes of a row: 4 in each wave (lanes pg, pg + 16, pg + 32, pg + 48), then the 4 waves through LDS
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float od = __shfl_xor(bd[j], off);
        const int32_t ol = __shfl_xor(bl[j], off);
        if (km_before(od, ol, bd[j], bl[j])) bd[j] = od, bl[j] = ol;
      }
    }
    if ((t & 63) < 16) {
      const int w = t >> 6;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = tile_query(pg, j);
        red_d[w * KM_TP + r] = bd[j];
        red_l[w * KM_TP + r] = bl[j];
      }
    }
    __syncthreads();
    int moved = 0;
    if (t < KM_TP && t < nrow) {
      const int32_t p = chunk * a.chunk_rows + r0 + t;
      if (a.elig[p]) {
        float d = red_d[t];
        int32_t l = red_l[t];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const float od = red_d[w * KM_TP + t];
          const int32_t ol = red_l[w * KM_TP + t];
          if (km_before(od, ol, d, l)) d = od, l = ol;
        }
        moved = a.labels[p] != l;
        a.labels[p] = l;
        a.dist2[p] = l < 0 ? __builtin_inff() : d;
      }
    }
    n_changed += __syncthreads_count(moved);
  }
  if (t == 0 && n_changed) atomicAdd(&a.st->changed[km_slot(round)], (uint32_t)n_changed);
}

// workgroup (x, y): rows [x * rows_per_group, + rows_per_group), columns [y * cols, + cols); cols a power of two, 8 .. 128
__global__ __launch_bounds__(KM_LANES) void kmeans_sum_kernel(KmArgs a, int round, int cols, int rows_per_group) {
  extern __shared__ float4 km_dyn[];
  if (a.st->done || km_last_round(a, round, a.st->changed[km_slot(round)])) return;  // (uniform)
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(km_dyn);  // [k][cols]
  uint32_t* cnt = reinterpret_cast<uint32_t*>(acc + (size_t)a.k * cols);   // [k]
  // a lane takes 4 columns of a row (one 16-byte load); cols / 4 lanes to a row, R rows to a pass, 8 passes in flight
  const int lpr = cols >> 2, t = threadIdx.x, lc = 4 * (t & (lpr - 1)), rsub = t / lpr, R = KM_LANES / lpr;
  const int n_acc = a.k * cols;
  for (int i = t; i < n_acc; i += KM_LANES) acc[i] = 0;
  for (int i = t; i < a.k; i += KM_LANES) cnt[i] = 0;
  __syncthreads();
  const int col = blockIdx.y * cols + lc;  // (a multiple of 4, as the stride is)
  const bool in_col = col < a.stride, counts = blockIdx.y == 0 && lc == 0;
  int sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sh[j] = 30 - (in_col ? f32_exponent(a.colmax[col + j]) : 0);
  const int64_t p_end = min((int64_t)a.n_total, ((int64_t)blockIdx.x + 1) * rows_per_group);
  for (int64_t p0 = (int64_t)blockIdx.x * rows_per_group + rsub; p0 < p_end; p0 += 8 * R) {
    int32_t l[8];
    float4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t p = p0 + (int64_t)i * R;
      l[i] = p < p_end ? a.labels[p] : -1;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t p = p0 + (int64_t)i * R;
      x[i] = float4{0.f, 0.f, 0.f, 0.f};
      if (l[i] >= 0 && in_col) {
        x[i] = *reinterpret_cast<const float4*>(tile_row(a.rows, (uint32_t)p, (uint32_t)a.chunk_rows, a.stride) + col);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (l[i] < 0) continue;
      if (in_col) {
        const float xv[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
        unsigned long long* dst = acc + l[i] * cols + lc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // exact scaling, then round to nearest even; |q| <= 2^30, so the conversion is one instruction
          const int q = (int)__builtin_rint(__builtin_ldexp((double)xv[j], sh[j]));
          if (q) atomicAdd(dst + j, (unsigned long long)(long long)q);
        }
      }
      if (counts) atomicAdd(&cnt[l[i]], 1u);
    }
  }
  __syncthreads();
  for (int i = t; i < n_acc; i += KM_LANES) {
    const unsigned long long v = acc[i];
    const int j = blockIdx.y * cols + (i & (cols - 1));
    if (v && j < a.stride) atomicAdd(&a.sums[(size_t)(i / cols) * a.stride + j], v);
  }
  if (blockIdx.y == 0)
    for (int i = t; i < a.k; i += KM_LANES)
      if (cnt[i]) atomicAdd(&a.counts[i], cnt[i]);
}

// one workgroup per centre
__global__ __launch_bounds__(KM_LANES) void kmeans_finalise_kernel(KmArgs a, int round) {
  if (a.st->done) return;  // (uniform; the lane that sets it below is of a workgroup that returns there as every other does)
  const uint32_t changed = a.st->changed[km_slot(round)];
  if (km_last_round(a, round, changed)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.st->n_iter = round;
      a.st->converged = (int64_t)changed <= a.stop_changed;
      a.st->done = 1;
    }
    return;
  }
  const int c = blockIdx.x;
  const uint32_t n = a.counts[c];
  for (int j = threadIdx.x; j < a.stride; j += KM_LANES) {
    const size_t o = (size_t)c * a.stride + j;
    if (n > 0 && j < a.dim) {
      const double mean = (double)(long long)a.sums[o] / (double)n;  // both conversions and the division round to nearest
      a.centres[o] = (float)__builtin_ldexp(mean, f32_exponent(a.colmax[j]) - 30);
    }
    a.sums[o] = 0;
  }
  __syncthreads();  // every lane has read the count
  if (threadIdx.x == 0) a.counts[c] = 0;
}

// columns per workgroup of kmeans_sum_kernel: the largest power of two in 8 .. 128 whose k x cols int64 sums fit KM_SUM_LDS, not
// wider than the stride needs
int sum_cols(int k, int stride) {
  int cols = 128;
  while (cols > 8 && ((size_t)k * cols * 8 > (size_t)KM_SUM_LDS || cols / 2 >= stride)) cols >>= 1;
  return cols;
}

}  // namespace

hipError_t launch_kmeans_prepare(const KmArgs& a, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  const int n_pass = (a.n_total + 31) / 32;
  hipLaunchKernelGGL(kmeans_prepare_kernel, dim3((unsigned)std::min(n_pass, 2048)), dim3(KM_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_kmeans_gather(const KmArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || !a.init_pos) return hipSuccess;
  hipLaunchKernelGGL(kmeans_gather_kernel, dim3((unsigned)a.k), dim3(KM_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_kmeans_round(const KmArgs& a, int t, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  // the tiles dealt evenly over at most KM_MAX_GROUPS workgroups
  const int per = (a.n_tile + KM_MAX_GROUPS - 1) / KM_MAX_GROUPS, groups = (a.n_tile + per - 1) / per;
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)groups), dim3(KM_LANES), 0, s, a, t);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int cols = sum_cols(a.k, a.stride), n_cg = (a.stride + cols - 1) / cols;
  const int want = std::max(1, KM_SUM_GROUPS / n_cg);
  // whole steps of 8 passes of 4 KM_LANES / cols rows, at least 16 of them to a workgroup
  const int pass = 8 * (4 * KM_LANES / cols);
  const int64_t rpg = std::max<int64_t>(16 * pass, (((int64_t)a.n_total + want - 1) / want + pass - 1) / pass * pass);
  const int n_rg = (int)(((int64_t)a.n_total + rpg - 1) / rpg);
  const size_t lds = (size_t)a.k * cols * 8 + (size_t)a.k * 4;
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_sum_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kmeans_sum_kernel, dim3((unsigned)n_rg, (unsigned)n_cg), dim3(KM_LANES), lds, s, a, t, cols, (int)rpg);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kmeans_finalise_kernel, dim3((unsigned)a.k), dim3(KM_LANES), 0, s, a, t);
  return hipGetLastError();
}

}  // namespace scann

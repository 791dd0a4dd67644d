// Density-peak clustering and kernel density of a latent-space index (scann_index_density, scann_index_peaks, include/scann_hip.h):
//   t(x, r) = round-to-nearest-even(2^30 scann_rbf_weight(dist2(x, r), gamma)),   S(x) = the int64 sum of t over the pool rows that count,
//   parent_i = the first row under (dist2, position) among the rows above i in the density order (S descending, position ascending),
// dist2 the difference-form chain of scann_knn_distsq (fp32, columns ascending).
//
// peaks_tile_kernel<false> (density) and <true> (parent) run on the tile and the slab pipeline of scann_tile.h, 128 queries x 64 pool
// rows per tile.  A workgroup's rows are a range of positions, each row read from its own storage chunk; where a
// row lies is worked out once per tile, where a query lies once per workgroup.  The queries are rows of their own or, for the self-join,
// the pool's rows by position.
//   density  at a tile's last slab the lane turns its 32 distances into terms in registers (peaks_term: the weight body of scann_rbf.h)
//            and adds them into eight 64-bit accumulators, one per query of its block; rows behind the range's end and the position a
//            query leaves out add nothing.  At the end of the range the 16 lanes that share a query are added through LDS (over the
//            slabs) and lane q < 128 adds the range's part to the query's sum with one 64-bit integer atomic.  Integer sums have no
//            order, so the split into ranges and the order of the atomics do not enter the result.
//   parent   the k = 1 walk of knn_tile_kernel: the tile's 128 x 64 distances go to LDS (over the slabs) with the 64 rows' sums beside
//            them, and lane q < 128 walks its query's 64 distances in position order; a row qualifies if it is above the query, and among
//            equal distances the earlier stays.  The range's result is one (dist2, position) per query; knn_merge_kernel (k = 1) takes
//            the first under (dist2, position) over the ranges.  No atomics.
// peaks_finish_kernel marks the queries with a non-finite component (S = -1); such a row is never above an eligible one.
// No scratch; 32 KiB + 1 KiB of LDS and at most 124 VGPRs: four workgroups per CU.
#include "scann_peaks.h"

#include <algorithm>

namespace scann {

namespace {

template <bool PARENT>
__global__ __launch_bounds__(PK_LANES) void peaks_tile_kernel(PeaksArgs a) {
  __shared__ float4 peaks_smem[TILE_UNION / 4];
  __shared__ long long side[TILE_TQ];                  // density: [128] the position each query leaves out; parent: [64] the tile rows' sums
  float* sm = reinterpret_cast<float*>(peaks_smem);
  float* qs = sm;                                    // the query slab ...
  float* rs = sm + tile_slab_floats(TILE_TQ);        // ... and the row slab (tile_stage)
  float* tile = sm;                                  // parent:  [64][128] distances of the tile, over the slabs
  unsigned long long* red = reinterpret_cast<unsigned long long*>(peaks_smem);  // density: [16][128] the lanes' sums, over the slabs
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.x * TILE_TQ;
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const long long r_lo = (long long)blockIdx.y * a.rows_per_range, r_hi = r_lo + a.rows_per_range;
  const int r_begin = (int)(r_lo < a.n_total ? r_lo : a.n_total), r_end = (int)(r_hi < a.n_total ? r_hi : a.n_total);
  const bool self = a.q == nullptr;
  // the lane stages four float4 of queries per slab, always of the same items: their rows are found once
  const float* qp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qi = q0 + ((t + PK_LANES * i) >> 3);
    qp[i] = qi >= a.nq ? nullptr : self ? tile_row(a.rows, qi, chunk_rows, stride) : a.q + (size_t)qi * stride;
  }
  const bool owner = t < TILE_TQ && q0 + t < a.nq;  // lane t finishes query q0 + t
  long long my_s = -1;     // parent: the query's sum (negative: not eligible, nothing is above it) ...
  float bd = 0.f;          // ... and the first row above it so far
  int bp = -1;
  if (PARENT) {
    if (owner) my_s = (long long)a.sums[q0 + t];
  } else if (t < TILE_TQ) {
    side[t] = !owner ? -1 : self ? q0 + t : a.skip ? a.skip[q0 + t] : -1;
  }
  unsigned long long s64[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s64[j] = 0;
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = ((r_end - r_begin + TILE_TR - 1) / TILE_TR) * n_slab;  // (tile, slab) steps of this range
  float4 gq[4], gr[2];
  const float* rp[2] = {nullptr, nullptr};
  int f_slab = 0, f_tile0 = r_begin;  // the step the next fetch belongs to
  auto fetch = [&]() {
    if (f_slab == 0) {  // a new tile: every row from its own chunk, a range may lie across a chunk boundary
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int pos = f_tile0 + ((t + PK_LANES * i) >> 3);
        rp[i] = pos < r_end ? tile_row(a.rows, pos, chunk_rows, stride) : nullptr;
      }
    }
    const int col = f_slab * TILE_SLAB + 4 * (t & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) gq[i] = qp[i] && col < stride ? *reinterpret_cast<const float4*>(qp[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i) gr[i] = rp[i] && col < stride ? *reinterpret_cast<const float4*>(rp[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
    if (++f_slab == n_slab) f_slab = 0, f_tile0 += TILE_TR;
  };
  f2 acc[8][2];
  tile_clear(acc);
  int c_slab = 0, tile0 = r_begin;  // the step being computed
  if (n_step > 0) fetch();
  for (int step = 0; step < n_step; ++step) {
    __syncthreads();  // the previous slab's reads, or the previous tile's walk, are over
    tile_stage<PK_LANES, 4, TILE_TQ>(qs, gq, t);
    tile_stage<PK_LANES, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch();
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (++c_slab != n_slab) continue;
    c_slab = 0;
    // the tile's last slab
    if (!PARENT) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int leave = (int)side[tile_query(qg, j)];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int pos = tile0 + 4 * rg + i;
          const int32_t term = peaks_term(tile_at(acc, j, i), a.gamma);
          s64[j] += (unsigned long long)(pos < r_end && pos != leave ? term : 0);
        }
        acc[j][0] = acc[j][1] = f2{0.f, 0.f};
      }
    } else {
      __syncthreads();  // every lane has read its last slab
      tile_write<TILE_TQ>(tile, acc, qg, rg);
      tile_clear(acc);
      if (t < TILE_TR) side[t] = tile0 + t < r_end ? (long long)a.sums[tile0 + t] : -1;
      __syncthreads();
      if (owner && my_s >= 0) {
        const int n = min(TILE_TR, r_end - tile0), me = q0 + t;
        for (int r = 0; r < n; ++r) {  // positions ascending: among equal distances the earlier row stays
          const float d = tile[r * TILE_TQ + t];
          if (!(d == d) || !peaks_above(side[r], tile0 + r, my_s, me)) continue;  // a NaN distance never qualifies
          if (bp < 0 || d < bd) bd = d, bp = tile0 + r;
        }
      }
    }
    tile0 += TILE_TR;
  }
  if (PARENT) {
    if (owner) {
      const size_t o = (size_t)(q0 + t) * a.n_range + blockIdx.y;
      a.part_d[o] = bp < 0 ? __builtin_inff() : bd;
      a.part_p[o] = bp;
    }
  } else {
    __syncthreads();  // every lane has read its last slab
    tile_sums_write(red, s64, qg, rg);
    __syncthreads();
    if (owner) {
      unsigned long long total = 0;
#pragma unroll
      for (int g = 0; g < PK_LANES / 16; ++g) total += red[g * TILE_TQ + t];
      if (total) atomicAdd(a.sums + q0 + t, total);
    }
  }
}

__global__ __launch_bounds__(PK_LANES) void peaks_finish_kernel(PeaksArgs a) {
  const int qi = blockIdx.x * PK_LANES + threadIdx.x;
  if (qi >= a.nq) return;
  const float* row = a.q == nullptr ? tile_row(a.rows, qi, a.chunk_rows, a.stride) : a.q + (size_t)qi * a.stride;
  if (row_nonfinite(row, a.stride)) a.sums[qi] = ~0ull;  // -1
}

}  // namespace

void peaks_geometry(int64_t n, int64_t nq, int32_t* rows_per_range, int32_t* n_range) {
  const int64_t n_qt = std::max<int64_t>(1, (nq + TILE_TQ - 1) / TILE_TQ), tiles = std::max<int64_t>(1, (n + TILE_TR - 1) / TILE_TR);
  const int64_t want = std::min<int64_t>({(PK_BLOCKS + n_qt - 1) / n_qt, tiles, 65535});
  const int64_t per = (tiles + want - 1) / want;  // tiles per range
  *rows_per_range = (int32_t)(per * TILE_TR);
  *n_range = (int32_t)((tiles + per - 1) / per);
}

hipError_t launch_peaks_density(const PeaksArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(peaks_tile_kernel<false>, dim3((unsigned)((a.nq + TILE_TQ - 1) / TILE_TQ), (unsigned)a.n_range), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_peaks_finish(const PeaksArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(peaks_finish_kernel, dim3((unsigned)((a.nq + PK_LANES - 1) / PK_LANES)), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_peaks_parent(const PeaksArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(peaks_tile_kernel<true>, dim3((unsigned)((a.nq + TILE_TQ - 1) / TILE_TQ), (unsigned)a.n_range), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

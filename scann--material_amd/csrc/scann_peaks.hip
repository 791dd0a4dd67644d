// Density-peak clustering and kernel density of a latent-space index (scann_index_density, scann_index_peaks, include/scann_hip.h):
//   t(x, r) = round-to-nearest-even(2^30 scann_rbf_weight(dist2(x, r), gamma)),   S(x) = the int64 sum of t over the pool rows that count,
//   parent_i = the first row under (dist2, position) among the rows above i in the density order (S descending, position ascending),
// dist2 the difference-form chain of scann_knn_distsq (fp32, columns ascending; why VALU and why this form: the top of scann_knn.hip).
//
// peaks_tile_kernel<false> (density) and <true> (parent) share the arithmetic and the tiling of knn_tile_kernel: 256 lanes, 128 queries x
// 64 pool rows per tile, 32-column slabs through LDS, column-major ([column][item], every group of four columns shifted by four floats),
// the next slab fetched into registers while this one is computed, an 8 x 4 register block of independent chains per lane, two rows of
// one query per packed fp32 instruction.  A workgroup's rows are a range of positions, each row read from its own storage chunk; where a
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
// No scratch; 32 KiB + 1 KiB of LDS and at most 122 VGPRs: four workgroups per CU.
#include "scann_peaks.h"

#include <algorithm>

namespace scann {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

template <bool PARENT>
__global__ __launch_bounds__(PK_LANES) void peaks_tile_kernel(PeaksArgs a) {
  __shared__ float4 peaks_smem[PK_UNION / 4];
  __shared__ long long side[PK_TQ];                  // density: [128] the position each query leaves out; parent: [64] the tile rows' sums
  float* sm = reinterpret_cast<float*>(peaks_smem);
  float* qs = sm;                                    // [32][PK_QS] + 32  query slab, column-major
  float* rs = sm + PK_SLAB * PK_QS + PK_SLAB;        // [32][PK_RS] + 32  row slab, column-major
  float* tile = sm;                                  // parent:  [64][128] distances of the tile, over the slabs
  unsigned long long* red = reinterpret_cast<unsigned long long*>(peaks_smem);  // density: [16][128] the lanes' sums, over the slabs
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.x * PK_TQ;
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const long long r_lo = (long long)blockIdx.y * a.rows_per_range, r_hi = r_lo + a.rows_per_range;
  const int r_begin = (int)(r_lo < a.n_total ? r_lo : a.n_total), r_end = (int)(r_hi < a.n_total ? r_hi : a.n_total);
  const bool self = a.q == nullptr;
  // the lane stages four float4 of queries per slab, always of the same items: their rows are found once
  const float* qp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qi = q0 + ((t + PK_LANES * i) >> 3);
    qp[i] = nullptr;
    if (qi < a.nq) {
      if (self) {
        const int c = qi / chunk_rows;
        qp[i] = a.rows[c] + (size_t)(qi - c * chunk_rows) * stride;
      } else {
        qp[i] = a.q + (size_t)qi * stride;
      }
    }
  }
  const bool owner = t < PK_TQ && q0 + t < a.nq;  // lane t finishes query q0 + t
  long long my_s = -1;     // parent: the query's sum (negative: not eligible, nothing is above it) ...
  float bd = 0.f;          // ... and the first row above it so far
  int bp = -1;
  if (PARENT) {
    if (owner) my_s = (long long)a.sums[q0 + t];
  } else if (t < PK_TQ) {
    side[t] = !owner ? -1 : self ? q0 + t : a.skip ? a.skip[q0 + t] : -1;
  }
  unsigned long long s64[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s64[j] = 0;
  const int n_slab = (stride + PK_SLAB - 1) / PK_SLAB;
  const int n_step = ((r_end - r_begin + PK_TR - 1) / PK_TR) * n_slab;  // (tile, slab) steps of this range
  float4 gq[4], gr[2];
  const float* rp[2] = {nullptr, nullptr};
  int f_slab = 0, f_tile0 = r_begin;  // the step the next fetch belongs to
  auto fetch = [&]() {
    if (f_slab == 0) {  // a new tile: every row from its own chunk, a range may lie across a chunk boundary
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int pos = f_tile0 + ((t + PK_LANES * i) >> 3);
        rp[i] = nullptr;
        if (pos < r_end) {
          const int c = pos / chunk_rows;
          rp[i] = a.rows[c] + (size_t)(pos - c * chunk_rows) * stride;
        }
      }
    }
    const int col = f_slab * PK_SLAB + 4 * (t & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) gq[i] = qp[i] && col < stride ? *reinterpret_cast<const float4*>(qp[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i) gr[i] = rp[i] && col < stride ? *reinterpret_cast<const float4*>(rp[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
    if (++f_slab == n_slab) f_slab = 0, f_tile0 += PK_TR;
  };
  f2 acc[8][2];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f};
  int c_slab = 0, tile0 = r_begin;  // the step being computed
  if (n_step > 0) fetch();
  for (int step = 0; step < n_step; ++step) {
    __syncthreads();  // the previous slab's reads, or the previous tile's walk, are over
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + PK_LANES * i, item = e >> 3, c = 4 * (e & 7);
      float* d = qs + c * PK_QS + c + item;
      d[0] = gq[i].x; d[PK_QS] = gq[i].y; d[2 * PK_QS] = gq[i].z; d[3 * PK_QS] = gq[i].w;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = t + PK_LANES * i, item = e >> 3, c = 4 * (e & 7);
      float* d = rs + c * PK_RS + c + item;
      d[0] = gr[i].x; d[PK_RS] = gr[i].y; d[2 * PK_RS] = gr[i].z; d[3 * PK_RS] = gr[i].w;
    }
    __syncthreads();
    if (step + 1 < n_step) fetch();
#pragma unroll 4
    for (int c = 0; c < PK_SLAB; ++c) {  // columns ascending: every pair's chain in the order of the definition
      const int sh = c & ~3;
      const float4 qa = *reinterpret_cast<const float4*>(qs + c * PK_QS + sh + 4 * qg);       // queries 4 qg .. 4 qg + 3
      const float4 qb = *reinterpret_cast<const float4*>(qs + c * PK_QS + sh + 64 + 4 * qg);  // queries 64 + 4 qg .. 64 + 4 qg + 3
      const float4 r4 = *reinterpret_cast<const float4*>(rs + c * PK_RS + sh + 4 * rg);       // rows 4 rg .. 4 rg + 3
      const f2 r01{r4.x, r4.y}, r23{r4.z, r4.w};
      const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f2 qq{qv[j], qv[j]};
        const f2 d0 = qq - r01, d1 = qq - r23;  // rounded once; the explicit fma keeps the square and the sum one operation
        acc[j][0] = __builtin_elementwise_fma(d0, d0, acc[j][0]);
        acc[j][1] = __builtin_elementwise_fma(d1, d1, acc[j][1]);
      }
    }
    if (++c_slab != n_slab) continue;
    c_slab = 0;
    // the tile's last slab
    if (!PARENT) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int leave = (int)side[(j < 4 ? 0 : 60) + 4 * qg + j];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int pos = tile0 + 4 * rg + i;
          const float d = (i & 1) ? acc[j][i >> 1].y : acc[j][i >> 1].x;
          const int32_t term = peaks_term(d, a.gamma);
          s64[j] += (unsigned long long)(pos < r_end && pos != leave ? term : 0);
        }
        acc[j][0] = acc[j][1] = f2{0.f, 0.f};
      }
    } else {
      __syncthreads();  // every lane has read its last slab
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float* dst = tile + (4 * rg + i) * PK_TQ + 4 * qg;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (i & 1) ? acc[j][i >> 1].y : acc[j][i >> 1].x;
        *reinterpret_cast<float4*>(dst) = float4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<float4*>(dst + 64) = float4{v[4], v[5], v[6], v[7]};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f};
      if (t < PK_TR) side[t] = tile0 + t < r_end ? (long long)a.sums[tile0 + t] : -1;
      __syncthreads();
      if (owner && my_s >= 0) {
        const int n = min(PK_TR, r_end - tile0), me = q0 + t;
        for (int r = 0; r < n; ++r) {  // positions ascending: among equal distances the earlier row stays
          const float d = tile[r * PK_TQ + t];
          if (!(d == d) || !peaks_above(side[r], tile0 + r, my_s, me)) continue;  // a NaN distance never qualifies
          if (bp < 0 || d < bd) bd = d, bp = tile0 + r;
        }
      }
    }
    tile0 += PK_TR;
  }
  if (PARENT) {
    if (owner) {
      const size_t o = (size_t)(q0 + t) * a.n_range + blockIdx.y;
      a.part_d[o] = bp < 0 ? __builtin_inff() : bd;
      a.part_p[o] = bp;
    }
  } else {
    __syncthreads();  // every lane has read its last slab
#pragma unroll
    for (int j = 0; j < 8; ++j) red[rg * PK_TQ + (j < 4 ? 0 : 60) + 4 * qg + j] = s64[j];
    __syncthreads();
    if (owner) {
      unsigned long long total = 0;
#pragma unroll
      for (int g = 0; g < PK_LANES / 16; ++g) total += red[g * PK_TQ + t];
      if (total) atomicAdd(a.sums + q0 + t, total);
    }
  }
}

__global__ __launch_bounds__(PK_LANES) void peaks_finish_kernel(PeaksArgs a) {
  const int qi = blockIdx.x * PK_LANES + threadIdx.x;
  if (qi >= a.nq) return;
  const float* row;
  if (a.q == nullptr) {
    const int c = qi / a.chunk_rows;
    row = a.rows[c] + (size_t)(qi - c * a.chunk_rows) * a.stride;
  } else {
    row = a.q + (size_t)qi * a.stride;
  }
  float nf = 0.f;  // NaN once a component was not finite (x - x is 0 for a finite x only; the padding columns are zero)
  for (int c = 0; c < a.stride; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    nf += ((v.x - v.x) + (v.y - v.y)) + ((v.z - v.z) + (v.w - v.w));
  }
  if (nf != nf) a.sums[qi] = ~0ull;  // -1
}

}  // namespace

void peaks_geometry(int64_t n, int64_t nq, int32_t* rows_per_range, int32_t* n_range) {
  const int64_t n_qt = std::max<int64_t>(1, (nq + PK_TQ - 1) / PK_TQ), tiles = std::max<int64_t>(1, (n + PK_TR - 1) / PK_TR);
  const int64_t want = std::min<int64_t>({(PK_BLOCKS + n_qt - 1) / n_qt, tiles, 65535});
  const int64_t per = (tiles + want - 1) / want;  // tiles per range
  *rows_per_range = (int32_t)(per * PK_TR);
  *n_range = (int32_t)((tiles + per - 1) / per);
}

hipError_t launch_peaks_density(const PeaksArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(peaks_tile_kernel<false>, dim3((unsigned)((a.nq + PK_TQ - 1) / PK_TQ), (unsigned)a.n_range), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_peaks_finish(const PeaksArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(peaks_finish_kernel, dim3((unsigned)((a.nq + PK_LANES - 1) / PK_LANES)), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_peaks_parent(const PeaksArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(peaks_tile_kernel<true>, dim3((unsigned)((a.nq + PK_TQ - 1) / PK_TQ), (unsigned)a.n_range), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

// Silhouette of a labelled latent-space index (scann_index_silhouette, include/scann_hip.h):
//   t(i, j) = round-to-nearest-even(2^shift e),  e = dist2(row_i, row_j) or its correctly rounded square root,
//   S[i][c] = the int64 sum of t over the counting rows j != i with label c,
// dist2 the difference-form chain of scann_knn_distsq (fp32, columns ascending).
//
// sil_tile_kernel is peaks_tile_kernel<false> (scann_peaks.hip) with another reduction, on the tile and the slab pipeline of
// scann_tile.h, 128 queries x 64 rows per tile.  A query has C sums, up to 1024, which fit neither registers nor LDS; so the rows come through a
// permutation that the host builds: the counting positions sorted by (label, position), every cluster padded to whole 64-row tiles.  A
// tile then belongs to one cluster, the lane keeps the eight 64-bit accumulators of the density pass, and they are flushed when the
// next tile belongs to another cluster and at the end of the range: the 16 lanes that share a query are added through LDS (over the
// slabs) and lane q < 128 adds the part to table[query][cluster] with one 64-bit integer atomic.  Integer sums have no order, so the
// split into ranges, the permutation and the order of the atomics do not enter the result.  Pad entries (-1), the query's own position
// and queries that do not count add nothing and raise no flag.  A term out of range sets the flag word with an ordinary atomic.
// The queries are rows of the pool by position (qpos), each read from its own storage chunk, as the tile's rows are.
// sil_finish_kernel: one wave per query forms a, b and other from the table and the counts in fp64.
// No scratch; 32 KiB + 2 KiB of LDS: four workgroups per CU (the registers: profiles/silhouette_rate.txt).
#pragma clang fp contract(off)
#include "scann_silhouette.h"

namespace scann {

namespace {

template <bool SQUARED>
__global__ __launch_bounds__(PK_LANES) void sil_tile_kernel(SilArgs a) {
  __shared__ float4 sil_smem[TILE_UNION / 4];
  __shared__ int leave_s[TILE_TQ];                     // the position each query leaves out; -1: the query gets nothing
  __shared__ const float* qrow_s[TILE_TQ];             // where each query's row lies, null: none
  __shared__ int perm_s[2][TILE_TR];                   // the positions of a tile's rows, this tile's and the next one's
  float* sm = reinterpret_cast<float*>(sil_smem);
  float* qs = sm;                                    // the query slab ...
  float* rs = sm + tile_slab_floats(TILE_TQ);        // ... and the row slab (tile_stage)
  unsigned long long* red = reinterpret_cast<unsigned long long*>(sil_smem);  // [16][128] the lanes' sums, over the slabs
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.x * TILE_TQ;
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const long long r_lo = (long long)blockIdx.y * a.rows_per_range, r_hi = r_lo + a.rows_per_range;
  const int r_begin = (int)(r_lo < a.n_perm ? r_lo : a.n_perm), r_end = (int)(r_hi < a.n_perm ? r_hi : a.n_perm);  // multiples of 64
  // the lane stages four float4 of queries per slab, always of the same items: their rows are found once, and kept in LDS, not in
  // eight registers (the term stage needs them for the fourth workgroup per CU)
  const bool owner = t < TILE_TQ && q0 + t < a.nq;  // lane t finishes query q0 + t
  if (t < TILE_TQ) {
    const int pos = owner ? a.qpos[q0 + t] : -1;
    leave_s[t] = pos;
    qrow_s[t] = pos >= 0 ? tile_row(a.rows, pos, chunk_rows, stride) : nullptr;
  }
  __syncthreads();
  unsigned long long s64[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s64[j] = 0;
  uint32_t worst = 0;  // the largest bit pattern among the scaled terms that count
  const float scale = a.scale;
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = ((r_end - r_begin) / TILE_TR) * n_slab;  // (tile, slab) steps of this range
  float4 gq[4], gr[2];
  const float* rp[2] = {nullptr, nullptr};
  int f_slab = 0, f_tile0 = r_begin, f_par = 0;  // the step the next fetch belongs to, and its tile's half of perm_s
  auto fetch = [&]() {
    if (f_slab == 0) {  // a new tile: every row through the permutation, from its own chunk
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int pos = a.perm[f_tile0 + ((t + PK_LANES * i) >> 3)];  // f_tile0 + 63 < n_perm
        rp[i] = pos >= 0 ? tile_row(a.rows, pos, chunk_rows, stride) : nullptr;
        if ((t & 7) == 0) perm_s[f_par][(t + PK_LANES * i) >> 3] = pos;  // read two barriers later at the earliest
      }
      f_par ^= 1;
    }
    const int col = f_slab * TILE_SLAB + 4 * (t & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* qp = qrow_s[(t + PK_LANES * i) >> 3];
      gq[i] = qp && col < stride ? *reinterpret_cast<const float4*>(qp + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) gr[i] = rp[i] && col < stride ? *reinterpret_cast<const float4*>(rp[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
    if (++f_slab == n_slab) f_slab = 0, f_tile0 += TILE_TR;
  };
  f2 acc[8][2];
  tile_clear(acc);
  int c_slab = 0, tile0 = r_begin, par = 0;  // the step being computed
  if (n_step > 0) fetch();
  for (int step = 0; step < n_step; ++step) {
    __syncthreads();  // the previous slab's reads, or the previous flush, are over
    tile_stage<PK_LANES, 4, TILE_TQ>(qs, gq, t);
    tile_stage<PK_LANES, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch();
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (++c_slab != n_slab) continue;
    c_slab = 0;
    // the tile's last slab: the 32 distances become terms
    const int4 p4 = *reinterpret_cast<const int4*>(&perm_s[par][4 * rg]);  // the positions of the lane's four rows
    const int pp[4] = {p4.x, p4.y, p4.z, p4.w};
    par ^= 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int leave = leave_s[tile_query(qg, j)];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float f = sil_scaled(tile_at(acc, j, i), SQUARED, scale);
        const bool live = leave >= 0 && pp[i] >= 0 && pp[i] != leave;
        s64[j] += live ? sil_round(f) : 0u;
        worst = max(worst, live ? __float_as_uint(f) : 0u);
      }
      acc[j][0] = acc[j][1] = f2{0.f, 0.f};
      __builtin_amdgcn_sched_barrier(0);  // one query's four roots at a time: 32 interleaved ones cost the fourth workgroup per CU
    }
    const int tile = tile0 / TILE_TR, label = a.tile_label[tile];
    tile0 += TILE_TR;
    if (tile0 < r_end && a.tile_label[tile + 1] == label) continue;  // (the same for every lane)
    // the cluster ends here, or the range does: the sums go to the table
    __syncthreads();  // every lane has read its last slab
    tile_sums_write(red, s64, qg, rg);
#pragma unroll
    for (int j = 0; j < 8; ++j) s64[j] = 0;
    __syncthreads();
    if (owner) {
      unsigned long long total = 0;
#pragma unroll
      for (int g = 0; g < PK_LANES / 16; ++g) total += red[g * TILE_TQ + t];
      if (total) atomicAdd(a.table + (size_t)(q0 + t) * a.C + label, total);
    }
  }
  if (worst > SIL_LIMIT_BITS) atomicOr(a.flag, 1u);
}

// One wave per query: lane l takes the clusters l, l + 64, ...; the least (mean, cluster) over the lanes by exchange.
__global__ __launch_bounds__(PK_LANES) void sil_finish_kernel(SilArgs a) {
  const int qi = blockIdx.x * (PK_LANES / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (qi >= a.nq) return;  // (the whole wave)
  const int ci = a.qlabel[qi];
  const double nan = __builtin_nan("");
  if (ci < 0) {
    if (lane == 0) a.a[qi] = nan, a.b[qi] = nan, a.other[qi] = -1;
    return;
  }
  const unsigned long long* row = a.table + (size_t)qi * a.C;
  double best = 0.0;
  int bc = -1;
  for (int c = lane; c < a.C; c += 64) {
    const long long n = a.counts[c];
    if (c == ci || n <= 0) continue;
    const double m = ldexp((double)(long long)row[c], -a.shift) / (double)n;
    if (bc < 0 || m < best) best = m, bc = c;  // clusters ascending: among equal means the lower stays
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off, 64);
    const int oc = __shfl_xor(bc, off, 64);
    if (oc >= 0 && (bc < 0 || ob < best || (ob == best && oc < bc))) best = ob, bc = oc;
  }
  if (lane == 0) {
    const long long n = a.counts[ci];
    a.a[qi] = n <= 1 ? 0.0 : ldexp((double)(long long)row[ci], -a.shift) / (double)(n - 1);
    a.b[qi] = bc < 0 ? nan : best;
    a.other[qi] = bc;
  }
}

__global__ __launch_bounds__(PK_LANES) void sil_eligible_kernel(const float* const* rows, int n_total, int chunk_rows, int stride, unsigned char* ok) {
  const int p = blockIdx.x * PK_LANES + threadIdx.x;
  if (p >= n_total) return;
  ok[p] = row_nonfinite(tile_row(rows, p, chunk_rows, stride), stride) ? 0 : 1;
}

}  // namespace

hipError_t launch_sil_tiles(const SilArgs& a, hipStream_t s) {
  if (a.n_perm <= 0 || a.nq <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.nq + TILE_TQ - 1) / TILE_TQ), (unsigned)a.n_range);
  if (a.squared)
    hipLaunchKernelGGL(sil_tile_kernel<true>, grid, dim3(PK_LANES), 0, s, a);
  else
    hipLaunchKernelGGL(sil_tile_kernel<false>, grid, dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sil_finish(const SilArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  const int per = PK_LANES / 64;
  hipLaunchKernelGGL(sil_finish_kernel, dim3((unsigned)((a.nq + per - 1) / per)), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sil_eligible(const float* const* rows, int32_t n_total, int32_t chunk_rows, int32_t stride, unsigned char* ok, hipStream_t s) {
  if (n_total <= 0) return hipSuccess;
  hipLaunchKernelGGL(sil_eligible_kernel, dim3((unsigned)((n_total + PK_LANES - 1) / PK_LANES)), dim3(PK_LANES), 0, s, rows, n_total, chunk_rows, stride, ok);
  return hipGetLastError();
}

}  // namespace scann

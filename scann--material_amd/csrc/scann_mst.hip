// The exact minimum spanning tree of a latent-space index by Boruvka rounds (scann_index_mst, include/scann_hip.h):
//   w(i, j) = max(dist2(i, j), core2[i], core2[j]),  edges ordered by (w, min(i, j), max(i, j)),
// dist2 the difference-form chain of scann_knn_distsq.  The order is total, so the tree is unique (scann_mst.h has the argument and the
// per-row rule the walk rests on).  A round is
//   mst_tile_kernel   for every row the first row of ANOTHER component under (w, position): the tiling and the arithmetic of
//                     peaks_tile_kernel<true> (the tile and the slab pipeline of scann_tile.h, 128 queries x 64 pool rows, ranges cut
//                     by position, each row read from its own storage chunk), with the 64 rows' labels and
//                     core distances beside the distance tile in LDS.  One (w, position) per query and range; knn_merge_kernel (k = 1)
//                     takes the first over the ranges.  A tile whose 64 rows carry the one label that all 128 queries of the workgroup
//                     carry holds no qualifying pair: every wave finds that with one compare per lane and a ballot (all waves read the
//                     same 64 labels, so the flag is uniform across the workgroup), and the tile is neither fetched nor computed.
//   the component step  mst_pick_kernel: a 64-bit atomicMin per row on (bits of w) << 32 | min(q, r) of its component's label (w >= 0, so
//                     the bit pattern is monotone); mst_pick_hi_kernel: a 32-bit atomicMin of max(q, r) among the rows that attain it.
//                     Exactly one row of a component attains both (the edge has one end in the component); mst_link_kernel lets it point
//                     the component at the one across the edge and append the edge.  Two components that picked the same edge root at the
//                     smaller label, which alone appends it.  mst_jump_kernel doubles the pointers, a number of launches fixed by the
//                     host; mst_relabel_kernel writes the roots back as labels and counts them.
// No kernel waits on another workgroup, every loop bound is fixed at launch, atomics are order-free (min, and a counter whose order the
// host's final sort removes).  No scratch; 110 VGPRs and 33,536 bytes of LDS: four workgroups per CU.
#include "scann_mst.h"

#include <algorithm>

namespace scann {

namespace {

__global__ __launch_bounds__(PK_LANES) void mst_tile_kernel(MstArgs a) {
  __shared__ float4 mst_smem[TILE_UNION / 4];
  __shared__ int32_t s_comp[TILE_TR];                  // the tile rows' labels ...
  __shared__ float s_core[TILE_TR];                    // ... and core distances
  float* sm = reinterpret_cast<float*>(mst_smem);
  float* qs = sm;                                    // the query slab ...
  float* rs = sm + tile_slab_floats(TILE_TQ);        // ... and the row slab (tile_stage)
  float* tile = sm;                                  // [64][128] distances of the tile, over the slabs
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.x * TILE_TQ, nq = a.n_total;
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const long long r_lo = (long long)blockIdx.y * a.rows_per_range, r_hi = r_lo + a.rows_per_range;
  const int r_begin = (int)(r_lo < a.n_total ? r_lo : a.n_total), r_end = (int)(r_hi < a.n_total ? r_hi : a.n_total);
  // the lane stages four float4 of queries per slab, always of the same items: their rows are found once
  const float* qp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qi = q0 + ((t + PK_LANES * i) >> 3);
    qp[i] = qi < nq ? tile_row(a.rows, qi, chunk_rows, stride) : nullptr;
  }
  const bool owner = t < TILE_TQ && q0 + t < nq;  // lane t finishes query q0 + t
  const int my_c = owner ? a.comp[q0 + t] : -1;  // negative: not eligible, nothing qualifies
  const float my_core = owner ? a.core2[q0 + t] : 0.f;
  float bw = 0.f;  // the first row of another component so far
  int bp = -1;
  // the skip rule: do all queries of the workgroup carry one label?  (q0 < nq: the grid covers the queries)
  const int q_label = a.comp[q0];
  const bool q_one = __syncthreads_and(t >= TILE_TQ || q0 + t >= nq || a.comp[q0 + t] == q_label) != 0;
  unsigned int n_skipped = 0;
  // the first tile at or behind `from` with work in it (beyond the range: none): every wave looks at the same 64 labels
  auto seek = [&](int from) {
    int tl = from;
    if (!q_one) return tl;
    while (tl < r_end) {
      const int pos = tl + (t & 63);
      const bool same = pos >= r_end || a.comp[pos] == q_label;
      if (__ballot(same) != ~0ull) break;
      tl += TILE_TR;
      ++n_skipped;
    }
    return tl;
  };
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  float4 gq[4], gr[2];
  const float* rp[2] = {nullptr, nullptr};
  int f_slab = 0, f_tile0 = seek(r_begin);  // the step the next fetch belongs to
  int nxt = r_end;                          // the tile of the latest first-slab fetch
  auto fetch = [&]() {
    if (f_slab == 0) {  // a new tile: every row from its own chunk, a range may lie across a chunk boundary
      nxt = f_tile0;
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
    if (++f_slab == n_slab) f_slab = 0, f_tile0 = seek(f_tile0 + TILE_TR);
  };
  f2 acc[8][2];
  tile_clear(acc);
  int c_slab = 0, tile0 = f_tile0;  // the step being computed
  if (f_tile0 < r_end) fetch();
  while (tile0 < r_end) {
    __syncthreads();  // the previous slab's reads, or the previous tile's walk, are over
    tile_stage<PK_LANES, 4, TILE_TQ>(qs, gq, t);
    tile_stage<PK_LANES, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (f_tile0 < r_end) fetch();
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (++c_slab != n_slab) continue;
    c_slab = 0;
    // the tile's last slab
    __syncthreads();  // every lane has read its last slab
    tile_write<TILE_TQ>(tile, acc, qg, rg);
    tile_clear(acc);
    if (t < TILE_TR) {
      const bool in = tile0 + t < r_end;
      s_comp[t] = in ? a.comp[tile0 + t] : -1;
      s_core[t] = in ? a.core2[tile0 + t] : 0.f;
    }
    __syncthreads();
    if (owner && my_c >= 0) {
      const int n = min(TILE_TR, r_end - tile0);
      for (int r = 0; r < n; ++r) {  // positions ascending: among equal weights the earlier row stays (the per-row rule)
        const int c = s_comp[r];
        if (c < 0 || c == my_c) continue;
        const float w = mst_weight(tile[r * TILE_TQ + t], my_core, s_core[r]);
        if (bp < 0 || mst_row_before(w, tile0 + r, bw, bp)) bw = w, bp = tile0 + r;
      }
    }
    tile0 = nxt > tile0 ? nxt : r_end;  // the tile whose first slab is in flight, if there is one
  }
  if (owner) {
    const size_t o = (size_t)(q0 + t) * a.n_range + blockIdx.y;
    a.part_w[o] = bp < 0 ? __builtin_inff() : bw;
    a.part_p[o] = bp;
  }
  if (a.skipped && t == 0 && n_skipped) atomicAdd(a.skipped, n_skipped);
}

// comp[i] = i for a row whose components are all finite, -1 otherwise; counters[1] += the eligible rows
__global__ __launch_bounds__(PK_LANES) void mst_eligible_kernel(MstArgs a, int32_t* comp, int32_t* counters) {
  const int qi = blockIdx.x * PK_LANES + threadIdx.x;
  bool ok = false;
  if (qi < a.n_total) {
    ok = !row_nonfinite(tile_row(a.rows, qi, a.chunk_rows, a.stride), a.stride);
    comp[qi] = ok ? qi : -1;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counters + 1, (int32_t)__popcll(m));
}

__global__ __launch_bounds__(PK_LANES) void mst_clear_kernel(MstStep c) {
  const int i = blockIdx.x * PK_LANES + threadIdx.x;
  if (i == 0) c.counters[1] = 0;
  if (i >= c.n) return;
  c.key[i] = ~0ull;
  c.hi[i] = 0x7fffffff;
  c.ptr[0][i] = i;
}

// the row's candidate as the component step sees it: false if the row has none
__device__ inline bool mst_candidate(const MstStep& c, int i, int* label, int* other, unsigned long long* key, int* hi) {
  if (i >= c.n) return false;
  const int l = c.comp[i], p = c.best_p[i];
  if (l < 0 || p < 0) return false;
  *label = l;
  *other = p;
  *key = ((unsigned long long)__float_as_uint(c.best_w[i]) << 32) | (unsigned int)min(i, p);
  *hi = max(i, p);
  return true;
}

__global__ __launch_bounds__(PK_LANES) void mst_pick_kernel(MstStep c) {
  int l, p, hi;
  unsigned long long k;
  if (mst_candidate(c, blockIdx.x * PK_LANES + threadIdx.x, &l, &p, &k, &hi)) atomicMin(c.key + l, k);
}

__global__ __launch_bounds__(PK_LANES) void mst_pick_hi_kernel(MstStep c) {
  int l, p, hi;
  unsigned long long k;
  if (mst_candidate(c, blockIdx.x * PK_LANES + threadIdx.x, &l, &p, &k, &hi) && c.key[l] == k) atomicMin(c.hi + l, hi);
}

__global__ __launch_bounds__(PK_LANES) void mst_link_kernel(MstStep c) {
  const int i = blockIdx.x * PK_LANES + threadIdx.x;
  int l, p, hi;
  unsigned long long k;
  if (!mst_candidate(c, i, &l, &p, &k, &hi) || c.key[l] != k || c.hi[l] != hi) return;
  // the one row of component l that holds its first edge
  const int l2 = c.comp[p];
  const bool same = c.key[l2] == k && c.hi[l2] == hi;  // the component across picked this edge too
  if (same && l > l2) {
    c.ptr[0][l] = l2;  // the smaller label is the root and appends the edge
    return;
  }
  if (!same) c.ptr[0][l] = l2;
  const int e = atomicAdd(c.counters, 1);
  if (e < c.n - 1) {
    c.edge_a[e] = min(i, p);
    c.edge_b[e] = hi;
    c.edge_w[e] = c.best_w[i];
  }
}

__global__ __launch_bounds__(PK_LANES) void mst_jump_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * PK_LANES + threadIdx.x;
  if (i < n) out[i] = in[in[i]];
}

__global__ __launch_bounds__(PK_LANES) void mst_relabel_kernel(MstStep c, const int32_t* __restrict__ root) {
  const int i = blockIdx.x * PK_LANES + threadIdx.x;
  bool is_root = false;
  if (i < c.n) {
    const int l = c.comp[i];
    if (l >= 0) {
      const int r = root[l];
      c.comp[i] = r;
      is_root = r == i;  // a label is the position of one of the component's rows
    }
  }
  const unsigned long long m = __ballot(is_root);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(c.counters + 1, (int32_t)__popcll(m));
}

}  // namespace

hipError_t launch_mst_eligible(const MstArgs& a, int32_t* comp, int32_t* counters, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  hipLaunchKernelGGL(mst_eligible_kernel, dim3((unsigned)((a.n_total + PK_LANES - 1) / PK_LANES)), dim3(PK_LANES), 0, s, a, comp, counters);
  return hipGetLastError();
}

hipError_t launch_mst_tile(const MstArgs& a, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  hipLaunchKernelGGL(mst_tile_kernel, dim3((unsigned)((a.n_total + TILE_TQ - 1) / TILE_TQ), (unsigned)a.n_range), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mst_step(const MstStep& c, int jumps, hipStream_t s) {
  if (c.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((c.n + PK_LANES - 1) / PK_LANES)), block(PK_LANES);
  hipLaunchKernelGGL(mst_clear_kernel, grid, block, 0, s, c);
  hipLaunchKernelGGL(mst_pick_kernel, grid, block, 0, s, c);
  hipLaunchKernelGGL(mst_pick_hi_kernel, grid, block, 0, s, c);
  hipLaunchKernelGGL(mst_link_kernel, grid, block, 0, s, c);
  int cur = 0;
  for (int j = 0; j < jumps; ++j, cur ^= 1) hipLaunchKernelGGL(mst_jump_kernel, grid, block, 0, s, c.ptr[cur], c.ptr[cur ^ 1], c.n);
  hipLaunchKernelGGL(mst_relabel_kernel, grid, block, 0, s, c, c.ptr[cur]);
  return hipGetLastError();
}

}  // namespace scann

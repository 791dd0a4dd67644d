// The radius search over a latent-space index (include/scann_hip.h: scann_index_within): the kernel.
//
// within_tile_kernel: the tile and the slab pipeline of scann_tile.h, 128 queries against 64 entries at a time, the difference-form chain.
// What is its own is the epilogue.  After a tile's last slab every lane compares its 8 x 4 chain values with radius2 in registers and
// applies the position rules (pad entries, the query's own position, `upper`) there, the id rule only where a value passed; the
// workgroup votes through one LDS word whether the tile holds a hit at all.  A tile without one -- the common case -- has cost one
// compare per pair: no tile_write, no LDS walk, no global traffic.  A tile with hits adds to its queries' counts (LDS first, then one
// global integer add per query: order-free) and appends (query, position, dist2) records behind ONE reservation per workgroup and tile.
// The records arrive in no particular order; the host establishes the order of the result (within_finish).  Nothing depends on the
// chunking, the shares or the launch geometry.
#include "scann_within.h"

namespace scann {

namespace {

constexpr int KT = TILE_LANES;

// (the second bound holds the kernel to 128 VGPRs, four workgroups per CU as knn_tile_kernel has; left alone the compiler takes 167)
__global__ __launch_bounds__(KT, 4) void within_tile_kernel(WithinArgs a) {
  __shared__ float4 within_smem[TILE_SLABS / 4];
  __shared__ int32_t qsl[TILE_TQ];    // the group's queries, -1: none
  __shared__ uint32_t lcnt[TILE_TQ];  // a tile's hits per query
  __shared__ uint32_t ltot;           // ... and in all
  __shared__ unsigned long long lbase;
  __shared__ int32_t vote;            // the number of the last tile of this workgroup that held a hit
  float* qs = reinterpret_cast<float*>(within_smem);
  float* rs = qs + tile_slab_floats(TILE_TQ);
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int g = blockIdx.y, stride = a.stride;
  const bool upper = a.upper != 0, has_qid = a.qid != nullptr;
  int t_first = 0, cnt_all;
  if (a.list) cnt_all = a.count[g];
  else {
    const int T = (a.n_entries + TILE_TR - 1) / TILE_TR;
    // below the diagonal: tiles that lie wholly at or below the group's least query position hold no hit
    if (upper) t_first = min(T, (a.self_first + g * TILE_TQ + 1) / TILE_TR);
    cnt_all = T - t_first;
  }
  const int i_begin = (int)((long long)cnt_all * blockIdx.x / gridDim.x), i_end = (int)((long long)cnt_all * (blockIdx.x + 1) / gridDim.x);
  const int32_t* list = a.list ? a.list + (size_t)g * a.n_tile : nullptr;
  if (t < TILE_TQ) {
    const int q = a.qperm ? a.qperm[g * TILE_TQ + t] : g * TILE_TQ + t;
    qsl[t] = q < a.nq ? q : -1;
  }
  if (t == 0) vote = 0;
  __syncthreads();
  // the lane's eight queries: which exist, and the positions they hold in the table (-2: none)
  uint32_t valid = 0;
  int32_t qp[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int q = qsl[tile_query(qg, j)];
    valid |= (uint32_t)(q >= 0) << j;
    qp[j] = q >= 0 && a.self_first >= 0 ? a.self_first + q : -2;
  }
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = (i_end - i_begin) * n_slab;
  float4 gq[4], gr[2];
  auto fetch = [&](int step) {
    const int i = i_begin + step / n_slab, c0 = (step % n_slab) * TILE_SLAB;
    const int e0 = (list ? list[i] : t_first + i) * TILE_TR, ch = e0 / a.chunk_rows;  // (a chunk holds whole tiles)
    const float* rows = a.rows[ch] + (size_t)(e0 - ch * a.chunk_rows) * stride;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = t + KT * u, item = e >> 3, col = c0 + 4 * (e & 7);
      const int q = qsl[item];
      gq[u] = q >= 0 && col < stride ? *reinterpret_cast<const float4*>(a.q + (size_t)q * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = t + KT * u, item = e >> 3, col = c0 + 4 * (e & 7);
      gr[u] = e0 + item < a.n_entries && col < stride ? *reinterpret_cast<const float4*>(rows + (size_t)item * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  f2 acc[8][2];
  tile_clear(acc);
  if (n_step > 0) fetch(0);
  for (int step = 0; step < n_step; ++step) {
    __syncthreads();  // the previous slab's reads are over
    tile_stage<KT, 4, TILE_TQ>(qs, gq, t);
    tile_stage<KT, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch(step + 1);
    const bool last = step % n_slab == n_slab - 1;
    // the positions of the lane's four entries, asked for before the slab so that they have arrived behind it
    const int i_tile = i_begin + step / n_slab;
    const int e0 = (list ? list[i_tile] : t_first + i_tile) * TILE_TR, ch = e0 / a.chunk_rows, r0 = e0 - ch * a.chunk_rows + 4 * rg;
    int32_t p[4] = {-1, -1, -1, -1};
    if (last) {
      if (a.pos) {
        const int4 v = *reinterpret_cast<const int4*>(a.pos[ch] + r0);
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = e0 + 4 * rg + i < a.n_entries ? e0 + 4 * rg + i : -1;
      }
    }
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (!last) continue;
    // the tile's last slab: the compare, in registers.  NaN <= radius2 is false; +inf <= radius2 only at radius2 = +inf
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = ((valid >> j) & 1u) && tile_at(acc, j, i) <= a.radius2 && p[i] >= 0 && p[i] != qp[j] && (!upper || p[i] > qp[j]);
        mask |= (uint32_t)ok << (4 * j + i);
      }
    if (mask && has_qid) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!((mask >> (4 * j)) & 15u)) continue;
        const long long id = a.qid[qsl[tile_query(qg, j)]];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (((mask >> (4 * j + i)) & 1u) && a.ids[ch][r0 + i] == id) mask &= ~(1u << (4 * j + i));
      }
    }
    const int seq = step / n_slab + 1;
    if (mask) vote = seq;
    __syncthreads();
    if (vote != seq) {  // no hit in the tile
      tile_clear(acc);
      continue;
    }
    if (t < TILE_TQ) lcnt[t] = 0;
    if (t == 0) ltot = 0;
    __syncthreads();
    const uint32_t n_lane = __builtin_popcount(mask);
    uint32_t off = 0;
    if (n_lane) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t c = __builtin_popcount((mask >> (4 * j)) & 15u);
        if (c) atomicAdd(&lcnt[tile_query(qg, j)], c);
      }
      off = atomicAdd(&ltot, n_lane);
    }
    __syncthreads();
    if (t < TILE_TQ && lcnt[t]) atomicAdd(&a.counts[a.q_base + qsl[t]], lcnt[t]);
    if (t == 0) lbase = atomicAdd(a.cursor, (unsigned long long)ltot);  // one reservation for the tile
    __syncthreads();
    if (n_lane && lbase + ltot <= (unsigned long long)a.cap) {
      unsigned long long w = lbase + off;
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((mask >> (4 * j + i)) & 1u) {
            a.rec_q[w] = a.q_base + qsl[tile_query(qg, j)];
            a.rec_p[w] = p[i];
            a.rec_d[w] = tile_at(acc, j, i);
            ++w;
          }
    }
    tile_clear(acc);
  }
}

}  // namespace

hipError_t launch_within_tile(const WithinArgs& a, int n_share, hipStream_t s) {
  if (a.n_group <= 0 || n_share <= 0 || a.n_entries <= 0) return hipSuccess;
  hipLaunchKernelGGL(within_tile_kernel, dim3((unsigned)n_share, (unsigned)a.n_group), dim3(KT), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

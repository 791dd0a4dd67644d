// Exact neighbour ranks of a latent-space index (scann_index_ranks, include/scann_hip.h):
//   key of row l seen from query i = (dist2(row_i, row_l), l), ordered by dist2 ascending, then position ascending,
//   rank[i][p] = the number of eligible rows l != i whose key is strictly less than the key of probe[i][p],
// dist2 the difference-form chain of scann_knn_distsq (fp32, columns ascending).
//
// A query has up to 32 probes, and every pair of the self-join would have to be compared with all of them.  Instead the probes' keys are
// sorted per query once (ranks_prepare_kernel: one wave per query, lane p forms probe p's key with the chain and finds its sorted slot by
// counting the keys before it), and a pair only finds its BIN, the number of thresholds <= its key, and counts itself there:
//   rank of the sorted slot s = the rows in bins 0 .. s,
// since a row lies strictly below threshold s exactly when at most s thresholds are <= its key.  Rows in the last bin (above every
// threshold) count nowhere, and on a map worth scoring that is nearly every row: the lane keeps its eight queries' largest threshold
// distance in registers and drops such a pair after one compare.
//
// ranks_tile_kernel is sil_tile_kernel (scann_silhouette.hip) with another reduction, on the tile and the slab pipeline of scann_tile.h,
// 128 queries x 64 rows per tile, ranges cut by position.  Beside the slabs the workgroup keeps its queries' sorted threshold distances
// [32][128] and a histogram [16][128] of u32, two 16-bit bins to a word (a range has at most 65472 rows, so no bin overflows into its
// neighbour).  A pair that passes the compare finds its bin by a binary search over the threshold distances in LDS -- the thresholds'
// positions stay in global memory and are read only where a threshold's distance equals the pair's -- and does one LDS atomic add.  At the
// end of its range the workgroup adds its non-zero bins to the global table [nq][32] with integer atomics: integer sums have no order, so
// the split into ranges and the order of the atomics do not enter the result.  Ineligible rows, rows behind the range's end and the
// query's own position count nowhere; a query without a probe that has a rank is not even fetched.
// ranks_finish_kernel: one lane per query adds up the bins and scatters the ranks back to probe order.
// No scratch.  LDS: 24.25 KiB of slabs + 16 KiB of thresholds + 8 KiB of histogram + 1.5 KiB = 49.75 KiB, three workgroups per CU, not
// the four of the sibling kernels: a fourth would need the thresholds or the histogram in halves, i.e. two passes over all pairs wherever
// m > 16 (the map scores use m = 31), and one pass at three quarters of the occupancy is the cheaper of the two.
#pragma clang fp contract(off)
#include "scann_ranks.h"

namespace scann {

namespace {

constexpr int MP = RANKS_MP;

// One wave per query.  Lane p < m forms the key of probe p; the lanes m .. 31 hold keys of no probe.  Slot of lane p = the number of
// lanes whose key is before its own, equal keys in lane order: a permutation of 0 .. 31 with the probes that have a rank first.
__global__ __launch_bounds__(PK_LANES) void ranks_prepare_kernel(RanksArgs a) {
  const int qi = blockIdx.x * (PK_LANES / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (qi >= a.nq) return;  // (the whole wave)
  const int me = a.qpos[qi];
  const float* qrow = tile_row(a.rows, me, a.chunk_rows, a.stride);
  const bool q_ok = a.elig[me] != 0;
  const int pos = lane < a.m ? a.probe[(size_t)qi * a.m + lane] : -1;
  const bool has = q_ok && pos >= 0 && pos != me && a.elig[pos] != 0;
  float d = __builtin_inff();
  if (has) {
    const float* r = tile_row(a.rows, pos, a.chunk_rows, a.stride);
    float acc = 0.f;
    for (int c = 0; c < a.stride; c += 4) {  // (the padding columns are zero on both sides: they leave the chain as it is)
      const float4 x = *reinterpret_cast<const float4*>(qrow + c), y = *reinterpret_cast<const float4*>(r + c);
      float t;
      t = x.x - y.x; acc = fmaf(t, t, acc);
      t = x.y - y.y; acc = fmaf(t, t, acc);
      t = x.z - y.z; acc = fmaf(t, t, acc);
      t = x.w - y.w; acc = fmaf(t, t, acc);
    }
    d = acc;
  }
  const int kp = has ? pos : RANKS_NO_POS;
  int slot = 0;
  float dmax = -1.f;  // below every distance: a query without thresholds drops every pair
  for (int o = 0; o < MP; ++o) {
    const float od = __shfl(d, o, 64);
    const int op = __shfl(kp, o, 64);
    const bool before = od < d || (od == d && (op < kp || (op == kp && o < lane)));
    slot += before ? 1 : 0;
    if (op != RANKS_NO_POS) dmax = fmaxf(dmax, od);
  }
  if (lane < MP) {
    const size_t o = (size_t)qi * MP + slot;
    a.thr_d[o] = d;
    a.thr_p[o] = kp;
    a.slot_probe[o] = lane;
  }
  if (lane == 0) {
    a.qleave[qi] = dmax >= 0.f ? me : -1;
    a.qmax[qi] = dmax;
  }
}

__global__ __launch_bounds__(PK_LANES) void ranks_tile_kernel(RanksArgs a) {
  __shared__ float4 ranks_smem[TILE_SLABS / 4];
  __shared__ float thr_s[MP * TILE_TQ];                // [slot][query] the sorted threshold distances
  __shared__ unsigned int hist_s[MP / 2 * TILE_TQ];    // [bin / 2][query], bin b in the half word b & 1
  __shared__ int leave_s[TILE_TQ];                     // the position each query leaves out; -1: the query gets nothing
  __shared__ float qmax_s[TILE_TQ];
  __shared__ int perm_s[2][TILE_TR];                   // the positions of a tile's rows (-1: none), this tile's and the next one's
  float* sm = reinterpret_cast<float*>(ranks_smem);
  float* qs = sm;                                    // the query slab ...
  float* rs = sm + tile_slab_floats(TILE_TQ);        // ... and the row slab (tile_stage)
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.x * TILE_TQ;
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const long long r_lo = (long long)blockIdx.y * a.rows_per_range, r_hi = r_lo + a.rows_per_range;
  const int r_begin = (int)(r_lo < a.n_total ? r_lo : a.n_total), r_end = (int)(r_hi < a.n_total ? r_hi : a.n_total);
  if (t < TILE_TQ) {
    const bool in = q0 + t < a.nq;
    leave_s[t] = in ? a.qleave[q0 + t] : -1;
    qmax_s[t] = in ? a.qmax[q0 + t] : -1.f;
  }
  for (int e = t; e < MP * TILE_TQ; e += PK_LANES) {  // query e / 32, slot e % 32: the table is read along its rows
    const int q = e / MP, s = e % MP;
    thr_s[s * TILE_TQ + q] = q0 + q < a.nq ? a.thr_d[(size_t)(q0 + q) * MP + s] : __builtin_inff();
  }
  for (int e = t; e < MP / 2 * TILE_TQ; e += PK_LANES) hist_s[e] = 0u;
  __syncthreads();
  // the lane stages four float4 of queries per slab, always of the same items: their rows are found once
  const float* qp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pos = leave_s[(t + PK_LANES * i) >> 3];
    qp[i] = pos >= 0 ? tile_row(a.rows, pos, chunk_rows, stride) : nullptr;
  }
  float dmax[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dmax[j] = qmax_s[tile_query(qg, j)];
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = ((r_end - r_begin + TILE_TR - 1) / TILE_TR) * n_slab;  // (tile, slab) steps of this range
  float4 gq[4], gr[2];
  const float* rp[2] = {nullptr, nullptr};
  int f_slab = 0, f_tile0 = r_begin, f_par = 0;  // the step the next fetch belongs to, and its tile's half of perm_s
  auto fetch = [&]() {
    if (f_slab == 0) {  // a new tile: every eligible row from its own chunk
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = (t + PK_LANES * i) >> 3;
        int pos = f_tile0 + r;
        if (pos >= r_end || !a.elig[pos]) pos = -1;
        rp[i] = pos >= 0 ? tile_row(a.rows, pos, chunk_rows, stride) : nullptr;
        if ((t & 7) == 0) perm_s[f_par][r] = pos;  // read two barriers later at the earliest
      }
      f_par ^= 1;
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
  int c_slab = 0, par = 0;  // the step being computed
  if (n_step > 0) fetch();
  for (int step = 0; step < n_step; ++step) {
    __syncthreads();  // the previous slab's reads are over
    tile_stage<PK_LANES, 4, TILE_TQ>(qs, gq, t);
    tile_stage<PK_LANES, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch();
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (++c_slab != n_slab) continue;
    c_slab = 0;
    // the tile's last slab: the 32 distances find their bins
    const int4 p4 = *reinterpret_cast<const int4*>(&perm_s[par][4 * rg]);  // the positions of the lane's four rows
    const int pp[4] = {p4.x, p4.y, p4.z, p4.w};
    par ^= 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = tile_query(qg, j);
      const int leave = leave_s[q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = tile_at(acc, j, i);
        // (dmax is -1 for a query that gets nothing; both rows finite: d is no NaN)
        if (d <= dmax[j] && pp[i] >= 0 && pp[i] != leave) {
          const int bin = ranks_bin<MP>(thr_s + q, TILE_TQ, a.thr_p + (size_t)(q0 + q) * MP, d, pp[i]);
          if (bin < MP) atomicAdd(&hist_s[(bin >> 1) * TILE_TQ + q], 1u << (16 * (bin & 1)));
        }
      }
      acc[j][0] = acc[j][1] = f2{0.f, 0.f};
    }
  }
  __syncthreads();
  for (int e = t; e < MP / 2 * TILE_TQ; e += PK_LANES) {
    const unsigned int v = hist_s[e];
    const int q = e % TILE_TQ, b = 2 * (e / TILE_TQ);
    if (!v) continue;  // (a query behind the end has counted nothing)
    unsigned int* row = a.table + (size_t)(q0 + q) * MP + b;
    if (v & 0xffffu) atomicAdd(row, v & 0xffffu);
    if (v >> 16) atomicAdd(row + 1, v >> 16);
  }
}

__global__ __launch_bounds__(PK_LANES) void ranks_finish_kernel(RanksArgs a) {
  const int qi = blockIdx.x * PK_LANES + threadIdx.x;
  if (qi >= a.nq) return;
  const size_t o = (size_t)qi * MP;
  unsigned int below = 0;
  for (int s = 0; s < MP; ++s) {
    below += a.table[o + s];
    const int p = a.slot_probe[o + s];
    if (p >= a.m) continue;
    const bool has = a.thr_p[o + s] != RANKS_NO_POS;
    a.rank[(size_t)qi * a.m + p] = has ? (int32_t)below : -1;
    a.dist2[(size_t)qi * a.m + p] = has ? a.thr_d[o + s] : __builtin_inff();
  }
}

}  // namespace

hipError_t launch_ranks_prepare(const RanksArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  const int per = PK_LANES / 64;
  hipLaunchKernelGGL(ranks_prepare_kernel, dim3((unsigned)((a.nq + per - 1) / per)), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ranks_tiles(const RanksArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(ranks_tile_kernel, dim3((unsigned)((a.nq + TILE_TQ - 1) / TILE_TQ), (unsigned)a.n_range), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ranks_finish(const RanksArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(ranks_finish_kernel, dim3((unsigned)((a.nq + PK_LANES - 1) / PK_LANES)), dim3(PK_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

// The nearest-row search over an index partitioned into cells (include/scann_hip.h: scann_index_partition): the kernels.
//
// cells_gather_kernel builds the cell-ordered copy of the rows.  A search then runs, per pass of up to 1024 queries:
//   cells_centre_kernel   D[q][c] = dist2(query, centre), the chain of scann_knn_distsq with the query first, and per query its nearest
//                         centre (the host orders the queries by it, so that a group of 128 is coherent)
//   cells_plan_kernel 0   per group of 128 queries: every query's seed, the tile of least bound within its nearest cell (a tile of 64 real
//                         rows before a partial one), compacted into the group's seed list
//   cells_list_kernel       the tile body of knn_tile_kernel over a list of tiles of the copy; the merge of its lists gives tau_q
//   cells_plan_kernel 1   the survivors: every loose tile, and every other tile that is no seed and has bound <= tau_q for some q
//   cells_list_kernel       over the survivors, dropping distances above tau_q; knn_merge_kernel over both sets of lists
// In cell order a tile's rows are not in position order, so every insert and every rejection of the list kernel compares the pair
// (dist2, original position); pad entries (position -1) never enter a list.  No atomics; nothing depends on the launch geometry.
#include "scann_cells.h"

#include <algorithm>

namespace scann {

namespace {

constexpr int KT = TILE_LANES;

__global__ __launch_bounds__(256) void cells_gather_kernel(CellGatherArgs a) {
  const int per_row = a.stride / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.n_perm * per_row) return;
  const int e = (int)(i / per_row), c4 = (int)(i - (long long)e * per_row);
  const int p = a.perm[e];
  const int dc = e / a.chunk_rows, dr = e - dc * a.chunk_rows;
  float4 v{0.f, 0.f, 0.f, 0.f};
  if (p >= 0) v = *reinterpret_cast<const float4*>(tile_row(a.src_rows, p, a.chunk_rows, a.stride) + 4 * c4);
  *reinterpret_cast<float4*>(a.dst_rows[dc] + (size_t)dr * a.stride + 4 * c4) = v;
  if (c4 == 0) {
    a.dst_ids[dc][dr] = p >= 0 ? *tile_row(a.src_ids, p, a.chunk_rows, 1) : 0;
    a.dst_pos[dc][dr] = p;
  }
}

__global__ __launch_bounds__(256) void cells_roots_kernel(const float* __restrict__ lo, const float* __restrict__ hi, double* __restrict__ rlo,
                                                          double* __restrict__ rhi, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  rlo[i] = sqrt((double)lo[i]);
  rhi[i] = sqrt((double)hi[i]);  // (+inf stays +inf: a loose tile)
}

// 8 queries per workgroup in LDS, lane t takes centres t, t + 256, ...: one chain per (query, centre), columns ascending, query first
constexpr int CQ = 8;
__global__ __launch_bounds__(256) void cells_centre_kernel(CellSearchArgs a) {
  extern __shared__ float4 cells_smem[];
  float* qs = reinterpret_cast<float*>(cells_smem);  // [8][stride]
  float* bd = qs + CQ * a.stride;                    // [8][256] each lane's nearest centre of a query ...
  int32_t* bc = reinterpret_cast<int32_t*>(bd + CQ * 256);  // ... and which
  const int t = threadIdx.x, q0 = blockIdx.x * CQ, stride = a.stride;
  const int per_row = stride / 4;
  for (int e = t; e < CQ * per_row; e += 256) {
    const int i = e / per_row, c4 = e - i * per_row;
    reinterpret_cast<float4*>(qs)[e] = q0 + i < a.nq ? *reinterpret_cast<const float4*>(a.q + (size_t)(q0 + i) * stride + 4 * c4) : float4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  float best_d[CQ];
  int32_t best_c[CQ];
#pragma unroll
  for (int i = 0; i < CQ; ++i) best_d[i] = __builtin_inff(), best_c[i] = 0x7fffffff;
  for (int c = t; c < a.C; c += 256) {
    const float* z = a.centres + (size_t)c * stride;
    float acc[CQ];
#pragma unroll
    for (int i = 0; i < CQ; ++i) acc[i] = 0.f;
    for (int j = 0; j < stride; j += 4) {
      const float4 zv = *reinterpret_cast<const float4*>(z + j);
#pragma unroll
      for (int i = 0; i < CQ; ++i) {
        const float4 qv = *reinterpret_cast<const float4*>(qs + i * stride + j);
        const float d0 = qv.x - zv.x, d1 = qv.y - zv.y, d2 = qv.z - zv.z, d3 = qv.w - zv.w;
        acc[i] = __builtin_fmaf(d0, d0, acc[i]);
        acc[i] = __builtin_fmaf(d1, d1, acc[i]);
        acc[i] = __builtin_fmaf(d2, d2, acc[i]);
        acc[i] = __builtin_fmaf(d3, d3, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < CQ; ++i) {
      if (q0 + i < a.nq) a.D[(size_t)(q0 + i) * a.C + c] = acc[i];
      if (acc[i] == acc[i] && dist_before(acc[i], c, best_d[i], best_c[i])) best_d[i] = acc[i], best_c[i] = c;  // a NaN distance never qualifies
    }
  }
#pragma unroll
  for (int i = 0; i < CQ; ++i) bd[i * 256 + t] = best_d[i], bc[i * 256 + t] = best_c[i];
  __syncthreads();
  if (t < CQ && q0 + t < a.nq) {
    float d = __builtin_inff();
    int32_t c = 0x7fffffff;
    for (int l = 0; l < 256; ++l)
      if (dist_before(bd[t * 256 + l], bc[t * 256 + l], d, c)) d = bd[t * 256 + l], c = bc[t * 256 + l];
    a.key_cell[q0 + t] = c == 0x7fffffff ? -1 : c;
    a.key_d[q0 + t] = d;
  }
}

// One workgroup per group of 128 queries.  Flags of the group's tiles, then their ordered compaction into the pass's list.
// pass 2 is the plan of a radius search (scann_within.cpp): pass 1's survivors with every tau_q = a.radius2 and no seeds; its list and
// its count take the places of pass 0's.
__global__ __launch_bounds__(256) void cells_plan_kernel(CellSearchArgs a, int pass) {
  __shared__ float dmin[CELLS_MAX], dmax[CELLS_MAX];  // per cell over the group's queries: least and greatest D (pass 1)
  __shared__ unsigned char wild[CELLS_MAX];                 // a query of the group has a D that is not finite
  __shared__ float tau[TILE_TQ];
  __shared__ int32_t ql[TILE_TQ];
  __shared__ int32_t scan[256];
  __shared__ int32_t base;
  __shared__ float tau_max;
  const int t = threadIdx.x, g = blockIdx.x, T = a.n_tile, C = a.C;
  const bool radius = pass == 2;
  const int slot = radius ? 0 : pass;  // where the pass's list and count lie
  unsigned char* flag = radius ? nullptr : a.seed_flag + (size_t)g * T;
  if (t < TILE_TQ) {
    const int q = a.qperm[g * TILE_TQ + t];
    ql[t] = q;
    tau[t] = q < 0 || pass == 0 ? __builtin_inff() : radius ? a.radius2 : a.tau[(size_t)q * a.k + a.k - 1];
  }
  if (t == 0) base = 0;
  __syncthreads();
  if (pass == 0) {
    // the seed of query t: within its nearest cell the tile of least bound, a full tile before a partial one, then the earlier tile
    if (t < TILE_TQ && ql[t] >= 0) {
      const int c = a.key_cell[ql[t]];
      if (c >= 0) {
        const float D = a.key_d[ql[t]];
        const bool ok = cell_finite(D);
        const double ah = sqrt((double)D);
        double bb = 0.0;
        int bt = -1, bf = 0;
        for (int tt = a.first_tile[c]; tt < a.first_tile[c + 1]; ++tt) {
          const double b = cell_bound_roots(ah, a.rlo[tt], a.rhi[tt], ok && a.rhi[tt] < __builtin_inf());
          const int f = a.full[tt];
          if (bt < 0 || b < bb || (b == bb && f > bf)) bb = b, bt = tt, bf = f;
        }
        if (bt >= 0) flag[bt] = 1;
      }
    }
  } else {
    if (t == 0) {
      float m = 0.f;  // the greatest tau of the group (+inf where a query has fewer than k rows so far)
      for (int i = 0; i < TILE_TQ; ++i)
        if (ql[i] >= 0 && tau[i] > m) m = tau[i];
      tau_max = m;
    }
    for (int c = t; c < C; c += 256) {
      float lo = __builtin_inff(), hi = 0.f;
      bool w = false;
      for (int i = 0; i < TILE_TQ; ++i) {
        if (ql[i] < 0) continue;
        const float D = a.D[(size_t)ql[i] * C + c];
        if (!cell_finite(D)) w = true;
        else lo = fminf(lo, D), hi = fmaxf(hi, D);
      }
      dmin[c] = lo, dmax[c] = hi, wild[c] = w;
    }
  }
  __syncthreads();
  // the tiles in order, 256 at a time: this pass's flag of each, and the flagged ones appended to the list
  int32_t* list = a.list + ((size_t)slot * a.n_group + g) * T;
  for (int t0 = 0; t0 < T; t0 += 256) {
    const int tt = t0 + t;
    int f = 0;
    if (tt < T) {
      if (pass == 0) f = flag[tt];
      else if (!radius && flag[tt]) f = 0;  // a seed: visited already
      else if (tt >= a.n_cell_tile) f = 1;  // a loose tile is always visited
      else {
        const int c = a.tile_cell[tt];
        const double rlo = a.rlo[tt], rhi = a.rhi[tt];
        f = 1;
        // the whole group at once: every query's bound is at least the bound of (least a, greatest a), so above the greatest tau
        // no query of the group can need the tile
        if (!wild[c] && dmin[c] <= dmax[c]) {
          const double a_lo = sqrt((double)dmin[c]), a_hi = sqrt((double)dmax[c]);
          const double g1 = (1.0 - CELL_EPS) * a_lo - (1.0 + CELL_EPS) * rhi, g2 = (1.0 - CELL_EPS) * rlo - (1.0 + CELL_EPS) * a_hi;
          const double gg = (g1 > g2 ? g1 : g2) - CELL_ABS;
          if (rhi < __builtin_inf() && gg > 0.0 && (1.0 - CELL_EPS) * (gg * gg) > (double)tau_max) f = 0;
        }
        if (f) {  // query by query
          f = 0;
          for (int i = 0; i < TILE_TQ && !f; ++i) {
            if (ql[i] < 0) continue;
            const float D = a.D[(size_t)ql[i] * C + c];
            const double b = cell_bound_roots(sqrt((double)D), rlo, rhi, cell_finite(D) && rhi < __builtin_inf());
            if (!(b > (double)tau[i])) f = 1;
          }
        }
      }
    }
    // an inclusive scan of the 256 flags
    scan[t] = f;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int v = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    if (f) list[base + scan[t] - 1] = tt;
    __syncthreads();
    if (t == 255) base += scan[255];
    __syncthreads();
  }
  if (t == 0) a.count[slot * a.n_group + g] = base;
}

// knn_tile_kernel's tile body over a list of tiles of the cell-ordered copy: workgroup (x, g) takes the x-th share of group g's list
__global__ __launch_bounds__(KT) void cells_list_kernel(CellSearchArgs a, int pass) {
  extern __shared__ float4 cells_smem[];
  float* sm = reinterpret_cast<float*>(cells_smem);
  float* qs = sm;
  float* rs = sm + tile_slab_floats(TILE_TQ);
  float* tile = sm;
  float* ld = sm + TILE_UNION;                                             // [k][128] the k first so far under (dist2, position) ...
  int32_t* lp = reinterpret_cast<int32_t*>(ld + a.k * TILE_TQ);            // ... and their original positions
  long long* idt = reinterpret_cast<long long*>(lp + a.k * TILE_TQ);       // [64] ids of the tile's rows (qid only)
  int32_t* pt = reinterpret_cast<int32_t*>(idt + TILE_TR);                 // [64] original positions of the tile's rows, -1: a pad entry
  int32_t* qsl = pt + TILE_TR;                                             // [128] the group's queries
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int g = blockIdx.y, k = a.k, stride = a.stride;
  const int cnt_all = a.count[pass * a.n_group + g];
  const int i_begin = (int)((long long)cnt_all * blockIdx.x / gridDim.x), i_end = (int)((long long)cnt_all * (blockIdx.x + 1) / gridDim.x);
  const int32_t* list = a.list + ((size_t)pass * a.n_group + g) * a.n_tile;
  if (t < TILE_TQ) qsl[t] = a.qperm[g * TILE_TQ + t];
  __syncthreads();
  const int my_q = t < TILE_TQ ? qsl[t] : -1;
  const bool owner = my_q >= 0;
  const bool has_qid = a.qid != nullptr;
  const long long my_id = owner && has_qid ? a.qid[my_q] : 0;
  const float my_tau = owner && pass == 1 ? a.tau[(size_t)my_q * k + k - 1] : __builtin_inff();
  int cnt = 0;
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = (i_end - i_begin) * n_slab;
  float4 gq[4], gr[2];
  auto fetch = [&](int step) {
    const int tt = list[i_begin + step / n_slab], c0 = (step % n_slab) * TILE_SLAB;
    const int e0 = tt * TILE_TR, ch = e0 / a.chunk_rows;  // (a chunk holds whole tiles)
    const float* rows = a.rows[ch] + (size_t)(e0 - ch * a.chunk_rows) * stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + KT * i, item = e >> 3, col = c0 + 4 * (e & 7);
      const int q = qsl[item];
      gq[i] = q >= 0 && col < stride ? *reinterpret_cast<const float4*>(a.q + (size_t)q * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = t + KT * i, item = e >> 3, col = c0 + 4 * (e & 7);
      gr[i] = col < stride ? *reinterpret_cast<const float4*>(rows + (size_t)item * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  f2 acc[8][2];
  tile_clear(acc);
  if (n_step > 0) fetch(0);
  for (int step = 0; step < n_step; ++step) {
    __syncthreads();
    tile_stage<KT, 4, TILE_TQ>(qs, gq, t);
    tile_stage<KT, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch(step + 1);
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (step % n_slab != n_slab - 1) continue;
    __syncthreads();
    tile_write<TILE_TQ>(tile, acc, qg, rg);
    tile_clear(acc);
    if (t < TILE_TR) {
      const int e0 = list[i_begin + step / n_slab] * TILE_TR, ch = e0 / a.chunk_rows, r = e0 - ch * a.chunk_rows + t;
      pt[t] = a.pos[ch][r];
      if (has_qid) idt[t] = a.ids[ch][r];
    }
    __syncthreads();
    if (owner) {
      for (int r = 0; r < TILE_TR; ++r) {
        const int32_t p = pt[r];
        if (p < 0) continue;  // a pad entry
        const float d = tile[r * TILE_TQ + t];
        if (!(d == d)) continue;  // a NaN distance never qualifies
        if (has_qid && idt[r] == my_id) continue;
        if (d > my_tau) continue;  // k rows at most this far are known already; an equal distance stays
        if (cnt == k && !dist_before(d, p, ld[(k - 1) * TILE_TQ + t], lp[(k - 1) * TILE_TQ + t])) continue;
        int j = cnt < k ? cnt : k - 1;
        for (; j > 0 && dist_before(d, p, ld[(j - 1) * TILE_TQ + t], lp[(j - 1) * TILE_TQ + t]); --j) {
          ld[j * TILE_TQ + t] = ld[(j - 1) * TILE_TQ + t];
          lp[j * TILE_TQ + t] = lp[(j - 1) * TILE_TQ + t];
        }
        ld[j * TILE_TQ + t] = d;
        lp[j * TILE_TQ + t] = p;
        if (cnt < k) ++cnt;
      }
    }
  }
  if (owner) {
    const size_t o = ((size_t)my_q * (2 * a.n_list) + (size_t)pass * a.n_list + blockIdx.x) * k;
    for (int j = 0; j < k; ++j) {
      a.part_d[o + j] = j < cnt ? ld[j * TILE_TQ + t] : __builtin_inff();
      a.part_p[o + j] = j < cnt ? lp[j * TILE_TQ + t] : -1;
    }
  }
}

template <class K>
hipError_t allow_lds(K kernel, size_t lds) {
  if (lds <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

hipError_t launch_cells_gather(const CellGatherArgs& a, hipStream_t s) {
  const long long n = (long long)a.n_perm * (a.stride / 4);
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cells_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cells_roots(const float* lo, const float* hi, double* rlo, double* rhi, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cells_roots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lo, hi, rlo, rhi, n);
  return hipGetLastError();
}

size_t cells_list_lds_bytes(int k) { return (size_t)TILE_UNION * 4 + (size_t)k * TILE_TQ * 8 + TILE_TR * 8 + TILE_TR * 4 + TILE_TQ * 4; }

hipError_t launch_cells_centre(const CellSearchArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  const size_t lds = (size_t)CQ * a.stride * 4 + (size_t)CQ * 256 * 8;
  if (const hipError_t e = allow_lds(cells_centre_kernel, lds)) return e;
  hipLaunchKernelGGL(cells_centre_kernel, dim3((unsigned)((a.nq + CQ - 1) / CQ)), dim3(256), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_cells_plan(const CellSearchArgs& a, int pass, hipStream_t s) {
  if (a.n_group <= 0) return hipSuccess;
  hipLaunchKernelGGL(cells_plan_kernel, dim3((unsigned)a.n_group), dim3(256), 0, s, a, pass);
  return hipGetLastError();
}

hipError_t launch_cells_list(const CellSearchArgs& a, int pass, hipStream_t s) {
  if (a.n_group <= 0 || a.n_list <= 0) return hipSuccess;
  const size_t lds = cells_list_lds_bytes(a.k);
  if (const hipError_t e = allow_lds(cells_list_kernel, lds)) return e;
  hipLaunchKernelGGL(cells_list_kernel, dim3((unsigned)a.n_list, (unsigned)a.n_group), dim3(KT), lds, s, a, pass);
  return hipGetLastError();
}

}  // namespace scann

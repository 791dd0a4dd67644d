// Nearest rows of a latent-space index (scann_index_query, include/scann_hip.h): exact brute force in the difference form
//   dist2(q, r) = acc_D,  acc_0 = 0,  acc_{j+1} = fmaf(q[j] - r[j], q[j] - r[j], acc_j)        (fp32, columns ascending)
// and the k first rows under the total order (dist2 ascending, position ascending).
//
// knn_tile_kernel (one launch over all storage chunks): the tile and the slab pipeline of scann_tile.h, 128 queries against a contiguous
// range of index rows, 64 at a time.  After the last slab the 128 x 64 distances go to LDS, and lane q < 128 walks query q's 64 distances in position order
// against its sorted list of the k best so far ([place][query] in LDS: no register array is indexed, nothing spills).  At the end of
// the range the list is the range's partial result.  knn_merge_kernel: one wave per query pops the least head of the query's partial
// lists k times.  No atomics; every comparison is of (dist2, position), so the result is the same for any split into ranges.
#include "scann_knn.h"

#include <algorithm>

namespace scann {

namespace {

constexpr int KT = TILE_LANES;  // lanes of knn_tile_kernel

__global__ __launch_bounds__(KT) void knn_tile_kernel(KnnArgs a) {
  extern __shared__ float4 knn_smem[];
  float* sm = reinterpret_cast<float*>(knn_smem);
  float* qs = sm;                             // the query slab ...
  float* rs = sm + tile_slab_floats(TILE_TQ);  // ... and the row slab (tile_stage)
  float* tile = sm;                           // [64][128]     distances of the tile, over the slabs
  float* ld = sm + TILE_UNION;                 // [k][128]      per query: the k least distances so far, ascending ...
  int32_t* lp = reinterpret_cast<int32_t*>(ld + a.k * TILE_TQ);                   // ... and their positions
  long long* idt = reinterpret_cast<long long*>(lp + a.k * TILE_TQ);              // [64] ids of the tile's rows (qid only)
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.y * TILE_TQ;
  const int chunk = blockIdx.z, pos_base = chunk * a.chunk_rows;
  const int n_rows = min(a.chunk_rows, a.n_total - pos_base);  // rows of this chunk
  const float* __restrict__ rows = a.rows[chunk];
  const int r_begin = blockIdx.x * a.rows_per_range, r_end = min(n_rows, r_begin + a.rows_per_range);
  const int k = a.k, stride = a.stride;
  const bool owner = t < TILE_TQ && q0 + t < a.nq;  // lane t keeps the list of query q0 + t
  const bool has_qid = a.qid != nullptr;
  const long long my_id = owner && has_qid ? a.qid[q0 + t] : 0;
  int cnt = 0;
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = ((r_end - r_begin + TILE_TR - 1) / TILE_TR) * n_slab;  // (tile, slab) steps of this range
  // one step's slab in registers: 128 queries x 8 and 64 rows x 8 float4 (four columns of one item each); items / columns beyond the
  // end are zero.  Step s + 1 is fetched while step s is computed
  float4 gq[4], gr[2];
  auto fetch = [&](int step) {
    const int tile0 = r_begin + (step / n_slab) * TILE_TR, c0 = (step % n_slab) * TILE_SLAB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + KT * i, item = e >> 3, col = c0 + 4 * (e & 7);
      gq[i] = q0 + item < a.nq && col < stride ? *reinterpret_cast<const float4*>(a.q + (size_t)(q0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = t + KT * i, item = e >> 3, col = c0 + 4 * (e & 7);
      gr[i] = tile0 + item < r_end && col < stride ? *reinterpret_cast<const float4*>(rows + (size_t)(tile0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  f2 acc[8][2];
  tile_clear(acc);
  if (n_step > 0) fetch(0);
  for (int step = 0; step < n_step; ++step) {
    const int tile0 = r_begin + (step / n_slab) * TILE_TR;
    __syncthreads();  // the previous slab's reads, or the previous tile's walk, are over
    tile_stage<KT, 4, TILE_TQ>(qs, gq, t);
    tile_stage<KT, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch(step + 1);
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (step % n_slab != n_slab - 1) continue;
    // the tile's last slab: its 128 x 64 distances go to LDS and every query's list is brought up to date
    __syncthreads();  // every lane has read its last slab
    tile_write<TILE_TQ>(tile, acc, qg, rg);
    tile_clear(acc);
    if (has_qid && t < TILE_TR) idt[t] = tile0 + t < r_end ? a.ids[chunk][tile0 + t] : 0;
    __syncthreads();
    if (owner) {
      const int n = min(TILE_TR, r_end - tile0);
      for (int r = 0; r < n; ++r) {  // positions ascending: among equal distances the earlier row is already in the list
        const float d = tile[r * TILE_TQ + t];
        if (!(d == d)) continue;  // a NaN distance never qualifies
        if (has_qid && idt[r] == my_id) continue;
        if (cnt == k && !(d < ld[(k - 1) * TILE_TQ + t])) continue;
        int j = cnt < k ? cnt : k - 1;
        for (; j > 0 && ld[(j - 1) * TILE_TQ + t] > d; --j) {
          ld[j * TILE_TQ + t] = ld[(j - 1) * TILE_TQ + t];
          lp[j * TILE_TQ + t] = lp[(j - 1) * TILE_TQ + t];
        }
        ld[j * TILE_TQ + t] = d;
        lp[j * TILE_TQ + t] = pos_base + tile0 + r;
        if (cnt < k) ++cnt;
      }
    }
  }
  if (owner) {
    const size_t o = ((size_t)(q0 + t) * a.n_range + (size_t)chunk * gridDim.x + blockIdx.x) * k;
    for (int j = 0; j < k; ++j) {
      a.part_d[o + j] = j < cnt ? ld[j * TILE_TQ + t] : __builtin_inff();
      a.part_p[o + j] = j < cnt ? lp[j * TILE_TQ + t] : -1;
    }
  }
}

__global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ part_d, const int32_t* __restrict__ part_p, int n_range, int k,
                                                       float* __restrict__ out_d, int32_t* __restrict__ out_p) {
  extern __shared__ float4 knn_smem[];
  unsigned char* head = reinterpret_cast<unsigned char*>(knn_smem);  // [n_range] entries of each list already taken
  const int lane = threadIdx.x;
  const size_t q = blockIdx.x;
  for (int l = lane; l < n_range; l += 64) head[l] = 0;
  __syncthreads();
  constexpr int32_t NONE = 0x7fffffff;
  for (int o = 0; o < k; ++o) {
    float bd = __builtin_inff();
    int32_t bp = NONE, bl = -1;
    for (int l = lane; l < n_range; l += 64) {
      const int hd = head[l];
      if (hd >= k) continue;
      const size_t e = (q * n_range + l) * k + hd;
      const int32_t p = part_p[e];
      if (p < 0) continue;  // the list has ended
      const float d = part_d[e];
      if (dist_before(d, p, bd, bp)) bd = d, bp = p, bl = l;
    }
    float wd = bd;
    int32_t wp = bp;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float od = __shfl_xor(wd, off);
      const int32_t op = __shfl_xor(wp, off);
      if (dist_before(od, op, wd, wp)) wd = od, wp = op;
    }
    if (wp != NONE && bp == wp) ++head[bl];  // positions are unique: one lane advances one list
    if (lane == 0) {
      out_d[q * k + o] = wp == NONE ? __builtin_inff() : wd;
      out_p[q * k + o] = wp == NONE ? -1 : wp;
    }
    __syncthreads();
  }
}

}  // namespace

size_t knn_lds_bytes(int k) { return (size_t)TILE_UNION * 4 + (size_t)k * TILE_TQ * 8 + TILE_TR * 8; }

hipError_t launch_knn_tile(const KnnArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  const size_t lds = knn_lds_bytes(a.k);
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)(a.n_range / a.n_chunk), (unsigned)((a.nq + TILE_TQ - 1) / TILE_TQ), (unsigned)a.n_chunk);
  hipLaunchKernelGGL(knn_tile_kernel, grid, dim3(KT), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_knn_merge(const float* part_d, const int32_t* part_p, int nq, int n_range, int k, float* out_d, int32_t* out_p, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const size_t lds = std::max<size_t>((size_t)n_range, 16);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)nq), dim3(64), lds, s, part_d, part_p, n_range, k, out_d, out_p);
  return hipGetLastError();
}

}  // namespace scann

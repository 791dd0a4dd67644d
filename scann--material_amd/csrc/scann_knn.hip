// Nearest rows of a latent-space index (scann_index_query, include/scann_hip.h): exact brute force in the difference form
//   dist2(q, r) = acc_D,  acc_0 = 0,  acc_{j+1} = fmaf(q[j] - r[j], q[j] - r[j], acc_j)        (fp32, columns ascending)
// and the k first rows under the total order (dist2 ascending, position ascending).
//
// Why VALU and not the matrix pipe: the product form |q|^2 + |r|^2 - 2 q.r loses exactly the neighbours that matter (near-duplicates) to
// cancellation, and a pair's chain above has one fixed order, so its bits do not depend on the tiling.
//
// knn_tile_kernel (one launch over all storage chunks): a workgroup of 256 lanes takes 128 queries and a contiguous range of index rows.  Rows go through LDS 64 at a time in
// slabs of 32 columns (the next slab is fetched into registers while this one is computed), stored column-major ([column][item]) so
// that a lane reads its 8 queries and its 4 rows of one column with three conflict-free 16-byte LDS reads and owns an 8 x 4 register
// block of independent chains, two rows of one query per packed fp32 instruction.  After
// the last slab the 128 x 64 distances go to LDS (over the slabs), and lane q < 128 walks query q's 64 distances in position order
// against its sorted list of the k best so far ([place][query] in LDS: no register array is indexed, nothing spills).  At the end of
// the range the list is the range's partial result.  knn_merge_kernel: one wave per query pops the least head of the query's partial
// lists k times.  No atomics; every comparison is of (dist2, position), so the result is the same for any split into ranges.
#include "scann_knn.h"

#include <algorithm>

namespace scann {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int KT = 256;  // lanes of knn_tile_kernel

__global__ __launch_bounds__(KT) void knn_tile_kernel(KnnArgs a) {
  extern __shared__ float4 knn_smem[];
  float* sm = reinterpret_cast<float*>(knn_smem);
  float* qs = sm;                             // [32][KNN_QS] + 32  query slab, column-major
  float* rs = sm + KNN_SLAB * KNN_QS + KNN_SLAB;  // [32][KNN_RS] + 32  row slab, column-major
  float* tile = sm;                           // [64][128]     distances of the tile, over the slabs
  float* ld = sm + KNN_UNION;                 // [k][128]      per query: the k least distances so far, ascending ...
  int32_t* lp = reinterpret_cast<int32_t*>(ld + a.k * KNN_TQ);                   // ... and their positions
  long long* idt = reinterpret_cast<long long*>(lp + a.k * KNN_TQ);              // [64] ids of the tile's rows (qid only)
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int q0 = blockIdx.y * KNN_TQ;
  const int chunk = blockIdx.z, pos_base = chunk * a.chunk_rows;
  const int n_rows = min(a.chunk_rows, a.n_total - pos_base);  // rows of this chunk
  const float* __restrict__ rows = a.rows[chunk];
  const int r_begin = blockIdx.x * a.rows_per_range, r_end = min(n_rows, r_begin + a.rows_per_range);
  const int k = a.k, stride = a.stride;
  const bool owner = t < KNN_TQ && q0 + t < a.nq;  // lane t keeps the list of query q0 + t
  const bool has_qid = a.qid != nullptr;
  const long long my_id = owner && has_qid ? a.qid[q0 + t] : 0;
  int cnt = 0;
  const int n_slab = (stride + KNN_SLAB - 1) / KNN_SLAB;
  const int n_step = ((r_end - r_begin + KNN_TR - 1) / KNN_TR) * n_slab;  // (tile, slab) steps of this range
  // one step's slab in registers: 128 queries x 8 and 64 rows x 8 float4 (four columns of one item each); items / columns beyond the
  // end are zero.  Step s + 1 is fetched while step s is computed
  float4 gq[4], gr[2];
  auto fetch = [&](int step) {
    const int tile0 = r_begin + (step / n_slab) * KNN_TR, c0 = (step % n_slab) * KNN_SLAB;
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
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f};
  if (n_step > 0) fetch(0);
  for (int step = 0; step < n_step; ++step) {
    const int tile0 = r_begin + (step / n_slab) * KNN_TR;
    __syncthreads();  // the previous slab's reads, or the previous tile's walk, are over
    // column c of an item at [c * stride + (c / 4) * 4 + item]: the lanes of a wave hold 8 column groups of 8 items, and the shift per
    // column group spreads their stores over the banks; the 16-byte reads below stay aligned
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + KT * i, item = e >> 3, c = 4 * (e & 7);
      float* d = qs + c * KNN_QS + c + item;
      d[0] = gq[i].x; d[KNN_QS] = gq[i].y; d[2 * KNN_QS] = gq[i].z; d[3 * KNN_QS] = gq[i].w;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = t + KT * i, item = e >> 3, c = 4 * (e & 7);
      float* d = rs + c * KNN_RS + c + item;
      d[0] = gr[i].x; d[KNN_RS] = gr[i].y; d[2 * KNN_RS] = gr[i].z; d[3 * KNN_RS] = gr[i].w;
    }
    __syncthreads();
    if (step + 1 < n_step) fetch(step + 1);
#pragma unroll 4
    for (int c = 0; c < KNN_SLAB; ++c) {  // columns ascending: every pair's chain in the order of the definition
      const int sh = c & ~3;
      const float4 qa = *reinterpret_cast<const float4*>(qs + c * KNN_QS + sh + 4 * qg);       // queries 4 qg .. 4 qg + 3
      const float4 qb = *reinterpret_cast<const float4*>(qs + c * KNN_QS + sh + 64 + 4 * qg);  // queries 64 + 4 qg .. 64 + 4 qg + 3
      const float4 r4 = *reinterpret_cast<const float4*>(rs + c * KNN_RS + sh + 4 * rg);
      const f2 r01{r4.x, r4.y}, r23{r4.z, r4.w};
      const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f2 qq{qv[j], qv[j]};
        const f2 d0 = qq - r01, d1 = qq - r23;  // rounded once; the explicit fma below keeps the square and the sum one operation
        acc[j][0] = __builtin_elementwise_fma(d0, d0, acc[j][0]);
        acc[j][1] = __builtin_elementwise_fma(d1, d1, acc[j][1]);
      }
    }
    if (step % n_slab != n_slab - 1) continue;
    // the tile's last slab: its 128 x 64 distances go to LDS and every query's list is brought up to date
    __syncthreads();  // every lane has read its last slab
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* dst = tile + (4 * rg + i) * KNN_TQ + 4 * qg;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (i & 1) ? acc[j][i >> 1].y : acc[j][i >> 1].x;
      *reinterpret_cast<float4*>(dst) = float4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<float4*>(dst + 64) = float4{v[4], v[5], v[6], v[7]};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f};
    if (has_qid && t < KNN_TR) idt[t] = tile0 + t < r_end ? a.ids[chunk][tile0 + t] : 0;
    __syncthreads();
    if (owner) {
      const int n = min(KNN_TR, r_end - tile0);
      for (int r = 0; r < n; ++r) {  // positions ascending: among equal distances the earlier row is already in the list
        const float d = tile[r * KNN_TQ + t];
        if (!(d == d)) continue;  // a NaN distance never qualifies
        if (has_qid && idt[r] == my_id) continue;
        if (cnt == k && !(d < ld[(k - 1) * KNN_TQ + t])) continue;
        int j = cnt < k ? cnt : k - 1;
        for (; j > 0 && ld[(j - 1) * KNN_TQ + t] > d; --j) {
          ld[j * KNN_TQ + t] = ld[(j - 1) * KNN_TQ + t];
          lp[j * KNN_TQ + t] = lp[(j - 1) * KNN_TQ + t];
        }
        ld[j * KNN_TQ + t] = d;
        lp[j * KNN_TQ + t] = pos_base + tile0 + r;
        if (cnt < k) ++cnt;
      }
    }
  }
  if (owner) {
    const size_t o = ((size_t)(q0 + t) * a.n_range + (size_t)chunk * gridDim.x + blockIdx.x) * k;
    for (int j = 0; j < k; ++j) {
      a.part_d[o + j] = j < cnt ? ld[j * KNN_TQ + t] : __builtin_inff();
      a.part_p[o + j] = j < cnt ? lp[j * KNN_TQ + t] : -1;
    }
  }
}

// (d, p) before (e, q) in the total order
__device__ __forceinline__ bool knn_before(float d, int32_t p, float e, int32_t q) { return d < e || (d == e && p < q); }

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
      if (knn_before(d, p, bd, bp)) bd = d, bp = p, bl = l;
    }
    float wd = bd;
    int32_t wp = bp;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float od = __shfl_xor(wd, off);
      const int32_t op = __shfl_xor(wp, off);
      if (knn_before(od, op, wd, wp)) wd = od, wp = op;
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

size_t knn_lds_bytes(int k) { return (size_t)KNN_UNION * 4 + (size_t)k * KNN_TQ * 8 + KNN_TR * 8; }

hipError_t launch_knn_tile(const KnnArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.nq <= 0) return hipSuccess;
  const size_t lds = knn_lds_bytes(a.k);
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)(a.n_range / a.n_chunk), (unsigned)((a.nq + KNN_TQ - 1) / KNN_TQ), (unsigned)a.n_chunk);
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

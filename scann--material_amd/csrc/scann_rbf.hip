// Gaussian landmark features of a latent-space index (scann_index_rbf_features, include/scann_hip.h):
//   phi[p][c] = scann_rbf_weight(dist2(x_p, z_c), gamma),   dist2 the difference-form chain of scann_knn_distsq (fp32, columns ascending)
// written device to device as a feature matrix that the moment and leave-one-out kernels of the readout head read like any index.
//
// rbf_feature_kernel: the arithmetic and the tiling of knn_tile_kernel (scann_knn.hip).  A workgroup of 256 lanes takes 128 pool rows and
// 64 landmarks; both pass through LDS in slabs of 32 columns, column-major ([column][item], every group of four columns shifted by four
// floats), the next slab fetched into registers while this one is computed; a lane owns an 8 x 4 register block of independent chains, two
// landmarks of one row per packed fp32 instruction.  The landmarks (m x stride x 4 bytes) are re-read per row tile from L2.  Whether a
// row has a non-finite component is found while its columns are staged, once per row: such a row is NaN in all its features.  After the
// last slab the weight chain (scann_rbf.h) runs on the lane's 32 distances and the 128 x 64 features cross LDS (over the slabs) so that
// 16 lanes store one row's 256 bytes.  Tiles are cut by position, not by storage chunk.  No atomics, no scratch.
#include "scann_rbf.h"

namespace scann {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int PS = RBF_TP, LS = RBF_TL;  // floats per staged column of the row / landmark slab

// 0 where all four are finite, NaN otherwise (x - x is 0 for a finite x only)
__device__ __forceinline__ float rbf_nonfinite(const float4& v) { return ((v.x - v.x) + (v.y - v.y)) + ((v.z - v.z) + (v.w - v.w)); }

__global__ __launch_bounds__(RBF_LANES) void rbf_feature_kernel(RbfArgs a) {
  __shared__ float4 rbf_smem[(RBF_UNION + RBF_TP) / 4];
  float* sm = reinterpret_cast<float*>(rbf_smem);
  float* ps = sm;                               // [32][128] + 32  pool-row slab, column-major
  float* ls = sm + RBF_SLAB * PS + RBF_SLAB;    // [32][64] + 32   landmark slab, column-major
  float* tile = sm;                             // [128][68]       features of the tile, over the slabs
  int* bad = reinterpret_cast<int*>(sm + RBF_UNION);  // [128] the row has a non-finite component
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int n_lt = (a.m + RBF_TL - 1) / RBF_TL;
  const int l0 = (int)(blockIdx.x % (unsigned)n_lt) * RBF_TL, p0 = (int)(blockIdx.x / (unsigned)n_lt) * RBF_TP;
  const int stride = a.stride;
  // the lane stages four float4 of pool rows and two of landmarks per slab, always of the same items: their rows are found once.  A tile
  // may lie across two storage chunks
  const int pc0 = p0 / a.chunk_rows, poff = p0 - pc0 * a.chunk_rows;
  const float* prow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int item = (t + RBF_LANES * i) >> 3;
    int o = poff + item, c = pc0;
    if (o >= a.chunk_rows) o -= a.chunk_rows, ++c;
    prow[i] = p0 + item < a.n_total ? a.rows[c] + (size_t)o * stride : nullptr;
  }
  const float* lrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int item = (t + RBF_LANES * i) >> 3;
    lrow[i] = l0 + item < a.m ? a.lm + (size_t)(l0 + item) * stride : nullptr;
  }
  if (t < RBF_TP) bad[t] = 0;
  const int n_slab = (stride + RBF_SLAB - 1) / RBF_SLAB;
  float4 gq[4], gr[2];
  float nf[4] = {0.f, 0.f, 0.f, 0.f};  // NaN once a staged piece of the lane's item i was not finite
  auto fetch = [&](int slab) {
    const int col = slab * RBF_SLAB + 4 * (t & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gq[i] = prow[i] && col < stride ? *reinterpret_cast<const float4*>(prow[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
      nf[i] += rbf_nonfinite(gq[i]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) gr[i] = lrow[i] && col < stride ? *reinterpret_cast<const float4*>(lrow[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
  };
  f2 acc[8][2];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f};
  fetch(0);
  for (int slab = 0; slab < n_slab; ++slab) {
    __syncthreads();  // the previous slab's reads are over
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + RBF_LANES * i, item = e >> 3, c = 4 * (e & 7);
      float* d = ps + c * PS + c + item;
      d[0] = gq[i].x; d[PS] = gq[i].y; d[2 * PS] = gq[i].z; d[3 * PS] = gq[i].w;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = t + RBF_LANES * i, item = e >> 3, c = 4 * (e & 7);
      float* d = ls + c * LS + c + item;
      d[0] = gr[i].x; d[LS] = gr[i].y; d[2 * LS] = gr[i].z; d[3 * LS] = gr[i].w;
    }
    __syncthreads();
    if (slab + 1 < n_slab) fetch(slab + 1);
#pragma unroll 4
    for (int c = 0; c < RBF_SLAB; ++c) {  // columns ascending: every pair's chain in the order of the definition
      const int sh = c & ~3;
      const float4 qa = *reinterpret_cast<const float4*>(ps + c * PS + sh + 4 * qg);       // rows 4 qg .. 4 qg + 3
      const float4 qb = *reinterpret_cast<const float4*>(ps + c * PS + sh + 64 + 4 * qg);  // rows 64 + 4 qg .. 64 + 4 qg + 3
      const float4 r4 = *reinterpret_cast<const float4*>(ls + c * LS + sh + 4 * rg);       // landmarks 4 rg .. 4 rg + 3
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
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (nf[i] != nf[i]) bad[(t + RBF_LANES * i) >> 3] = 1;  // (the eight lanes of an item may all write: the same value)
  __syncthreads();  // every lane has read its last slab, and the rows' flags are complete
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = (j < 4 ? 0 : 60) + 4 * qg + j;
    const bool b = bad[row] != 0;
    float4 w;
    w.x = b ? nan : rbf_weight(acc[j][0].x, a.gamma);
    w.y = b ? nan : rbf_weight(acc[j][0].y, a.gamma);
    w.z = b ? nan : rbf_weight(acc[j][1].x, a.gamma);
    w.w = b ? nan : rbf_weight(acc[j][1].y, a.gamma);
    *reinterpret_cast<float4*>(tile + row * RBF_LD + 4 * rg) = w;
  }
  __syncthreads();
  // 16 lanes per row: a wave stores four whole 256-byte row segments per instruction
  const int oc0 = p0 / a.out_chunk_rows, ooff = p0 - oc0 * a.out_chunk_rows;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = t + RBF_LANES * i, row = e >> 4, c4 = 4 * (e & 15), col = l0 + c4;
    if (p0 + row >= a.n_total || col >= a.out_stride) continue;
    float4 v = *reinterpret_cast<const float4*>(tile + row * RBF_LD + c4);
    if (col + 3 >= a.m) {  // the padding columns of the last landmarks' float4 are zero
      if (col + 1 >= a.m) v.y = 0.f;
      if (col + 2 >= a.m) v.z = 0.f;
      v.w = 0.f;
    }
    int o = ooff + row, c = oc0;
    if (o >= a.out_chunk_rows) o -= a.out_chunk_rows, ++c;
    *reinterpret_cast<float4*>(a.out[c] + (size_t)o * a.out_stride + col) = v;
  }
}

}  // namespace

hipError_t launch_rbf_features(const RbfArgs& a, hipStream_t s) {
  if (a.n_total <= 0 || a.m <= 0) return hipSuccess;
  const unsigned n_lt = (unsigned)((a.m + RBF_TL - 1) / RBF_TL), n_pt = (unsigned)(((int64_t)a.n_total + RBF_TP - 1) / RBF_TP);
  hipLaunchKernelGGL(rbf_feature_kernel, dim3(n_lt * n_pt), dim3(RBF_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

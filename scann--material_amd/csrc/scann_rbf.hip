// Gaussian landmark features of a latent-space index (scann_index_rbf_features, include/scann_hip.h):
//   phi[p][c] = scann_rbf_weight(dist2(x_p, z_c), gamma),   dist2 the difference-form chain of scann_knn_distsq (fp32, columns ascending)
// written device to device as a feature matrix that the moment and leave-one-out kernels of the readout head read like any index.
//
// rbf_feature_kernel: the tile and the slab pipeline of scann_tile.h, difference form: 128 pool rows (the tile's "queries") against 64
// landmarks (its "rows").  The landmarks (m x stride x 4 bytes) are re-read per row tile from L2.  Whether a
// row has a non-finite component is found while its columns are staged, once per row: such a row is NaN in all its features.  After the
// last slab the weight chain (scann_rbf.h) runs on the lane's 32 distances and the 128 x 64 features cross LDS (over the slabs) so that
// 16 lanes store one row's 256 bytes.  Tiles are cut by position, not by storage chunk.  No atomics, no scratch.
#include "scann_rbf.h"

namespace scann {

namespace {

__global__ __launch_bounds__(RBF_LANES) void rbf_feature_kernel(RbfArgs a) {
  __shared__ float4 rbf_smem[(RBF_UNION + RBF_TP) / 4];
  float* sm = reinterpret_cast<float*>(rbf_smem);
  float* ps = sm;                               // the pool-row slab ...
  float* ls = sm + tile_slab_floats(RBF_TP);    // ... and the landmark slab (tile_stage)
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
      nf[i] += row_nonfinite(gq[i]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) gr[i] = lrow[i] && col < stride ? *reinterpret_cast<const float4*>(lrow[i] + col) : float4{0.f, 0.f, 0.f, 0.f};
  };
  f2 acc[8][2];
  tile_clear(acc);
  fetch(0);
  for (int slab = 0; slab < n_slab; ++slab) {
    __syncthreads();  // the previous slab's reads are over
    tile_stage<RBF_LANES, 4, RBF_TP>(ps, gq, t);
    tile_stage<RBF_LANES, 2, RBF_TL>(ls, gr, t);
    __syncthreads();
    if (slab + 1 < n_slab) fetch(slab + 1);
    tile_slab<TileForm::DIFF>(ps, ls, qg, rg, acc, RBF_SLAB);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (nf[i] != nf[i]) bad[(t + RBF_LANES * i) >> 3] = 1;  // (the eight lanes of an item may all write: the same value)
  __syncthreads();  // every lane has read its last slab, and the rows' flags are complete
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = tile_query(qg, j);
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

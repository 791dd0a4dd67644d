// The slab pipeline of the tiled passes over a latent-space index, once: the tile constants, the LDS layout of a staged slab, the inner
// column loop on a lane's register block and the ways a finished block leaves the registers.  The kernels that are built from it
// (knn_tile_kernel, match_tile_kernel, kmeans_assign_kernel, rbf_feature_kernel, logit_pass_kernel, pca_project_kernel,
// peaks_tile_kernel, mst_tile_kernel, sil_tile_kernel, ranks_tile_kernel) keep what is their own: what they fetch and by which rule, the step loop with
// its barriers, and the epilogue.
//
// The chain.  Every result of these passes is defined to the bit (include/scann_hip.h) by one fp32 chain per pair, columns ascending:
//   difference form  acc_{j+1} = fmaf(q[j] - r[j], q[j] - r[j], acc_j)   the difference rounded once, the square and the sum one operation
//   product form     acc_{j+1} = fmaf(q[j], r[j], acc_j)
// Why VALU and not the matrix pipe: the product form |q|^2 + |r|^2 - 2 q.r of a distance loses exactly the neighbours that matter
// (near-duplicates) to cancellation, and a chain has one fixed order, so its bits depend neither on the tiling nor on the launch
// geometry.  A chain is never split over lanes.
//
// The tile.  A workgroup of 256 lanes takes 128 items of one side ("queries": lane index qg = t & 15) and 64 of the other ("rows":
// rg = t >> 4).  Both pass through LDS in slabs of 32 columns; a lane fetches four float4 of queries and two of rows per slab into
// registers (float4 i of lane t: item (t + 256 i) >> 3, columns 4 (t & 7) .. + 3 of the slab; items and columns beyond the end are
// zero) while the previous slab is computed.  A slab lies column-major, [column][item], so that a lane reads its 8 queries (4 qg .. + 3
// and 64 + 4 qg .. + 3) and its 4 rows (4 rg .. + 3) of one column with three conflict-free 16-byte LDS reads; it owns an 8 x 4
// register block of independent chains, two rows of one query per packed fp32 instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_prim.h"

namespace scann {

constexpr int TILE_LANES = 256;  // lanes of a workgroup
constexpr int TILE_TQ = 128;     // queries per tile
constexpr int TILE_TR = 64;      // rows per tile
constexpr int TILE_SLAB = 32;    // columns per LDS slab
// floats of a slab whose staged columns are ld floats long: column c lies (c / 4) * 4 floats further (tile_stage)
constexpr int tile_slab_floats(int ld) { return TILE_SLAB * ld + TILE_SLAB; }
constexpr int TILE_SLABS = tile_slab_floats(TILE_TQ) + tile_slab_floats(TILE_TR);  // floats of the query slab and the row slab behind it
// floats the slabs share with what follows them: the 64 x 128 distance tile (tile_write) or the lanes' 16 x 128 64-bit sums (tile_sums_write)
constexpr int TILE_UNION = TILE_TR * TILE_TQ;
static_assert(TILE_SLABS <= TILE_UNION, "the slabs lie under the tile");

typedef float f2 __attribute__((ext_vector_type(2)));

// The LDS store of one staged slab: g[i] holds columns 4 (e & 7) .. + 3 of item e >> 3, e = t + LANES i.  Column c of an item goes to
// [c * LD + (c / 4) * 4 + item]: the lanes of a wave hold 8 column groups of 8 items, and the shift per column group spreads their
// stores over the banks; the 16-byte reads of tile_slab stay aligned.
template <int LANES, int N, int LD>
__device__ __forceinline__ void tile_stage(float* slab, const float4 (&g)[N], int t) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = t + LANES * i, item = e >> 3, c = 4 * (e & 7);
    float* d = slab + c * LD + c + item;
    d[0] = g[i].x; d[LD] = g[i].y; d[2 * LD] = g[i].z; d[3 * LD] = g[i].w;
  }
}

// column c of the lane's 8 queries
__device__ __forceinline__ void tile_queries(const float* qs, int c, int qg, float (&qv)[8]) {
  const float* p = qs + c * TILE_TQ + (c & ~3) + 4 * qg;
  const float4 qa = *reinterpret_cast<const float4*>(p), qb = *reinterpret_cast<const float4*>(p + 64);
  qv[0] = qa.x, qv[1] = qa.y, qv[2] = qa.z, qv[3] = qa.w, qv[4] = qb.x, qv[5] = qb.y, qv[6] = qb.z, qv[7] = qb.w;
}

enum class TileForm { DIFF, PROD };

// Columns 0 .. n_col - 1 of the staged slabs, ascending, on the lane's block: every pair's chain in the order of the definition.
// acc[j][h] holds query j of the lane against its rows 2 h and 2 h + 1.
template <TileForm FORM>
__device__ __forceinline__ void tile_slab(const float* qs, const float* rs, int qg, int rg, f2 (&acc)[8][2], int n_col) {
#pragma unroll 4
  for (int c = 0; c < n_col; ++c) {
    float qv[8];
    tile_queries(qs, c, qg, qv);
    const float4 r4 = *reinterpret_cast<const float4*>(rs + c * TILE_TR + (c & ~3) + 4 * rg);
    const f2 r01{r4.x, r4.y}, r23{r4.z, r4.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f2 qq{qv[j], qv[j]};
      if constexpr (FORM == TileForm::DIFF) {
        const f2 d0 = qq - r01, d1 = qq - r23;  // the query first; rounded once; the explicit fma keeps the square and the sum one operation
        acc[j][0] = __builtin_elementwise_fma(d0, d0, acc[j][0]);
        acc[j][1] = __builtin_elementwise_fma(d1, d1, acc[j][1]);
      } else {
        acc[j][0] = __builtin_elementwise_fma(qq, r01, acc[j][0]);
        acc[j][1] = __builtin_elementwise_fma(qq, r23, acc[j][1]);
      }
    }
  }
}

__device__ __forceinline__ void tile_clear(f2 (&acc)[8][2]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = f2{0.f, 0.f};
}

// the lane's query j, 0 .. 7, within the tile, and its chain against its row i, 0 .. 3 (row 4 rg + i of the tile)
__device__ __forceinline__ int tile_query(int qg, int j) { return (j < 4 ? 0 : 60) + 4 * qg + j; }
__device__ __forceinline__ float tile_at(const f2 (&acc)[8][2], int j, int i) { return (i & 1) ? acc[j][i >> 1].y : acc[j][i >> 1].x; }

// The block as part of the tile's 128 x 64 results in LDS, [row][query] with LD floats between two rows.  The tile lies over the slabs:
// every lane has read its last slab (a barrier) before this, and a barrier follows before the tile is read.
template <int LD>
__device__ __forceinline__ void tile_write(float* tile, const f2 (&acc)[8][2], int qg, int rg) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float* dst = tile + (4 * rg + i) * LD + 4 * qg;
    *reinterpret_cast<float4*>(dst) = float4{tile_at(acc, 0, i), tile_at(acc, 1, i), tile_at(acc, 2, i), tile_at(acc, 3, i)};
    *reinterpret_cast<float4*>(dst + 64) = float4{tile_at(acc, 4, i), tile_at(acc, 5, i), tile_at(acc, 6, i), tile_at(acc, 7, i)};
  }
}

// The lane's eight 64-bit sums, one per query of its block, to red [16][128] in LDS (over the slabs, between the same barriers as
// tile_write): the 16 lanes that share query q have then left their parts at red[g * 128 + q], g = 0 .. 15, for the query's owner to add.
__device__ __forceinline__ void tile_sums_write(unsigned long long* red, const unsigned long long (&s64)[8], int qg, int rg) {
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rg * TILE_TQ + tile_query(qg, j)] = s64[j];
}

// 0 where all four are finite, NaN otherwise (x - x is 0 for a finite x only)
__device__ __forceinline__ float row_nonfinite(const float4& v) { return ((v.x - v.x) + (v.y - v.y)) + ((v.z - v.z) + (v.w - v.w)); }
// whether a row of `stride` floats (a multiple of 4; the padding columns are zero) has a non-finite component
__device__ __forceinline__ bool row_nonfinite(const float* row, int stride) {
  float nf = 0.f;
  for (int c = 0; c < stride; c += 4) nf += row_nonfinite(*reinterpret_cast<const float4*>(row + c));
  return nf != nf;
}

}  // namespace scann

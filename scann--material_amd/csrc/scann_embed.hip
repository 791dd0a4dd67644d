// Neighbour embedding of a latent-space index (scann_embed_iterate, include/scann_hip.h): the iterations of t-SNE's gradient descent in two
// dimensions with the exact O(N^2) pair repulsion, every sum over the definition's fixed tree.  Four launches per iteration, one lane
// per row i throughout:
//   embed_repulse_kernel  grid (row groups of 256, spans): the workgroup walks its span's 32 blocks of 128 positions j.  A block's y
//                         (1 KiB) is staged in LDS and read at one address by all lanes -- a broadcast, no bank conflicts --; per lane the
//                         fp32 chains z, rx, ry of the block run in registers and are folded into the lane's fp64 span sums, which go
//                         to part[span][.][i].  Only the (at most two) blocks that hold the workgroup's own rows, and a ragged last
//                         block, take the loop that tests j == i and the bound.
//   embed_rowsum_kernel   Z_i, Rx_i, Ry_i: the spans of part added in span order; the block sums of Z_i, rows in position order.
//   embed_update_kernel   Z from the block sums (every workgroup adds them itself: blocks within a span, then the spans), the attraction
//                         chains over the row's stored edges, gradient, gain and momentum update, y' into the other position buffer; the
//                         block sums of y'.
//   embed_centre_kernel   the mean of y' from the block sums, y = y' - mean.
// No atomics, no scratch: the order of every sum is the definition's.
#pragma clang fp contract(off)

#include "scann_embed.h"

namespace scann {

namespace {

__global__ __launch_bounds__(EMBED_LANES) void embed_repulse_kernel(const float2* __restrict__ y, int N, double* __restrict__ part) {
  __shared__ float2 ys[EMBED_BLOCK];
  const int t = threadIdx.x;
  const int i0 = (int)blockIdx.x * EMBED_LANES, i = i0 + t, span = (int)blockIdx.y;
  const float2 yi = y[min(i, N - 1)];
  double Z = 0.0, Rx = 0.0, Ry = 0.0;
  for (int b = 0; b < EMBED_SPAN; ++b) {
    const int j0 = (span * EMBED_SPAN + b) * EMBED_BLOCK;
    if (j0 >= N) break;
    __syncthreads();  // the previous block's reads are over
    if (t < EMBED_BLOCK) ys[t] = y[min(j0 + t, N - 1)];
    __syncthreads();
    float z = 0.f, rx = 0.f, ry = 0.f;
    const int nj = min(EMBED_BLOCK, N - j0);
    if (nj == EMBED_BLOCK && (j0 + EMBED_BLOCK <= i0 || j0 >= i0 + EMBED_LANES)) {  // (uniform) no row of the workgroup lies in the block
#pragma unroll 8
      for (int j = 0; j < EMBED_BLOCK; ++j) embed_repel(yi.x, yi.y, ys[j].x, ys[j].y, z, rx, ry);
    } else {
      const int self = i - j0;
      for (int j = 0; j < nj; ++j)
        if (j != self) embed_repel(yi.x, yi.y, ys[j].x, ys[j].y, z, rx, ry);
    }
    Z += (double)z;
    Rx += (double)rx;
    Ry += (double)ry;
  }
  if (i < N) {
    double* dst = part + (size_t)span * 3 * N + i;
    dst[0] = Z;
    dst[N] = Rx;
    dst[2 * (size_t)N] = Ry;
  }
}

// bs[block] for the workgroup's (at most two) blocks: the sum of v over the block's rows in position order; v of a row past N is not read
__device__ __forceinline__ void embed_block_sums(double v, double* sh /* [EMBED_LANES] */, int N, double* bs) {
  const int t = threadIdx.x, i = (int)blockIdx.x * EMBED_LANES + t;
  sh[t] = v;
  __syncthreads();
  if ((t & (EMBED_BLOCK - 1)) == 0 && i < N) {
    const int n = min(EMBED_BLOCK, N - i);
    double acc = 0.0;
    for (int r = 0; r < n; ++r) acc += sh[t + r];
    bs[i / EMBED_BLOCK] = acc;
  }
  __syncthreads();
}

// the tree's total of block sums, in every lane: the blocks of a span in block order, then the spans in order
__device__ __forceinline__ double embed_total(const double* __restrict__ bs, int n_block, double* sh /* [EMBED_MAX_SPANS] */) {
  const int t = threadIdx.x, n_span = (n_block + EMBED_SPAN - 1) / EMBED_SPAN;
  if (t < n_span) {
    const int b1 = min(n_block, (t + 1) * EMBED_SPAN);
    double acc = 0.0;
    for (int b = t * EMBED_SPAN; b < b1; ++b) acc += bs[b];
    sh[t] = acc;
  }
  __syncthreads();
  double total = 0.0;
  for (int s = 0; s < n_span; ++s) total += sh[s];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(EMBED_LANES) void embed_rowsum_kernel(TsneArgs a) {
  __shared__ double sh[EMBED_LANES];
  const int N = a.N, i = (int)(blockIdx.x * EMBED_LANES + threadIdx.x);
  double Z = 0.0, Rx = 0.0, Ry = 0.0;
  if (i < N) {
    for (int s = 0; s < a.n_span; ++s) {
      const double* src = a.part + (size_t)s * 3 * N + i;
      Z += src[0];
      Rx += src[N];
      Ry += src[2 * (size_t)N];
    }
    a.rsum[i] = Z;
    a.rsum[(size_t)N + i] = Rx;
    a.rsum[2 * (size_t)N + i] = Ry;
  }
  embed_block_sums(Z, sh, N, a.bsum);
}

__global__ __launch_bounds__(EMBED_LANES) void embed_update_kernel(TsneArgs a, int cur) {
  __shared__ double sh[EMBED_LANES];
  const int N = a.N, i = (int)(blockIdx.x * EMBED_LANES + threadIdx.x), n_block = (N + EMBED_BLOCK - 1) / EMBED_BLOCK;
  const double Z = embed_total(a.bsum, n_block, sh);
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.z_out = Z;
  const float2* __restrict__ y = cur ? a.y[1] : a.y[0];  // (selects, not an indexed read of the argument block)
  float2* __restrict__ y_next = cur ? a.y[0] : a.y[1];
  float2 yn{0.f, 0.f};
  if (i < N) {
    const float2 yi = y[i];
    float ax = 0.f, ay = 0.f;
    const int64_t e1 = a.row_first[i + 1];
    for (int64_t e = a.row_first[i]; e < e1; ++e) {
      const float2 yj = y[a.col[e]];
      embed_attract(yi.x, yi.y, yj.x, yj.y, a.p[e], ax, ay);
    }
    const float gx = embed_gradient(a.exaggeration, ax, a.rsum[(size_t)N + i], Z);
    const float gy = embed_gradient(a.exaggeration, ay, a.rsum[2 * (size_t)N + i], Z);
    float2 u = a.u[i], gain = a.gain[i];
    yn.x = embed_update(gx, a.lr, a.momentum, yi.x, u.x, gain.x);
    yn.y = embed_update(gy, a.lr, a.momentum, yi.y, u.y, gain.y);
    a.u[i] = u;
    a.gain[i] = gain;
    a.grad[i] = float2{gx, gy};
    y_next[i] = yn;
  }
  embed_block_sums((double)yn.x, sh, N, a.bsum + n_block);
  embed_block_sums((double)yn.y, sh, N, a.bsum + 2 * (size_t)n_block);
}

__global__ __launch_bounds__(EMBED_LANES) void embed_centre_kernel(TsneArgs a, int cur) {
  __shared__ double sh[EMBED_MAX_SPANS];
  const int N = a.N, i = (int)(blockIdx.x * EMBED_LANES + threadIdx.x), n_block = (N + EMBED_BLOCK - 1) / EMBED_BLOCK;
  const double Sx = embed_total(a.bsum + n_block, n_block, sh);
  const double Sy = embed_total(a.bsum + 2 * (size_t)n_block, n_block, sh);
  const float mx = (float)(Sx / (double)N), my = (float)(Sy / (double)N);
  if (i < N) {
    float2* y = cur ? a.y[0] : a.y[1];
    const float2 v = y[i];
    y[i] = float2{v.x - mx, v.y - my};
  }
}

}  // namespace

hipError_t launch_embed_iteration(const TsneArgs& a, int cur, hipStream_t s) {
  const unsigned groups = (unsigned)((a.N + EMBED_LANES - 1) / EMBED_LANES);
  hipLaunchKernelGGL(embed_repulse_kernel, dim3(groups, (unsigned)a.n_span), dim3(EMBED_LANES), 0, s, a.y[cur], a.N, a.part);
  hipLaunchKernelGGL(embed_rowsum_kernel, dim3(groups), dim3(EMBED_LANES), 0, s, a);
  hipLaunchKernelGGL(embed_update_kernel, dim3(groups), dim3(EMBED_LANES), 0, s, a, cur);
  hipLaunchKernelGGL(embed_centre_kernel, dim3(groups), dim3(EMBED_LANES), 0, s, a, cur);
  return hipGetLastError();
}

}  // namespace scann

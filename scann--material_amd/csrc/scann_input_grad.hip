// Leaves of the data-gradient backward (scann_input_grads): d y / d input for the Keras graph's float inputs
// (scann_model.py:345-373).  Plain fp32, one fixed summation order per output, no atomics: run-to-run bit-reproducible.  The width
// (local_dim) is a run-time argument, so the same kernels serve the 128 / 8 MFMA handles and the plain-fp32 generic-width ones; the
// weights are read as row-major Keras tensors [in, out] (the 128-wide handles keep raw copies of exactly these in their arena).
#include "scann_train.h"
#include "scann_mma.h"

namespace scann {

namespace {

// Gaussian expansion exp(-(x - c_k)^2 / 0.25) (custom_layers.py:63-65, width 0.5 squared) and its derivative in x
__device__ __forceinline__ void gauss20(float x, const float* __restrict__ cen, float* g, float* dg) {
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const float d = x - cen[k];
    g[k] = gauss(x, cen[k]);
    dg[k] = -8.0f * d * g[k];
  }
}

constexpr int IG_WAVES = 4;  // one wave per edge, four edges per 256-thread workgroup

// g_update branch: geom0 = swish(ad) * swish(aw), ad = G(dist).Wd + bd, aw = G(weight).Ww + bw (scann_model.py:378-389).
// dpd = dG0 * swish(aw) * swish'(ad), d dist = sum_c dpd[c] * sum_k Wd[k,c] * G_k'(dist); the same for the weight.
__global__ __launch_bounds__(256) void basis_input_grad_kernel(const float* __restrict__ dist, const float* __restrict__ weight,
                                                               const float* __restrict__ dG0, const float* __restrict__ Wd,
                                                               const float* __restrict__ bd, const float* __restrict__ Ww,
                                                               const float* __restrict__ bw, const float* __restrict__ cd,
                                                               const float* __restrict__ cw, int n_edge, int width,
                                                               float* __restrict__ d_dist, float* __restrict__ d_weight) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * IG_WAVES + (threadIdx.x >> 6);
  if (e >= n_edge) return;  // (whole waves leave: the shuffles below never see a missing lane)
  float gd[NG], dgd[NG], gw[NG], dgw[NG];
  gauss20(dist[e], cd, gd, dgd);
  gauss20(weight[e], cw, gw, dgw);
  const float* __restrict__ dg = dG0 + (size_t)e * width;
  float sd = 0.f, sw = 0.f;
  for (int c = lane; c < width; c += 64) {
    float ad = bd[c], aw = bw[c], td = 0.f, tw = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const float wdk = Wd[(size_t)k * width + c], wwk = Ww[(size_t)k * width + c];
      ad = fmaf(gd[k], wdk, ad);
      aw = fmaf(gw[k], wwk, aw);
      td = fmaf(dgd[k], wdk, td);
      tw = fmaf(dgw[k], wwk, tw);
    }
    const float g = dg[c];
    sd = fmaf(g * swish_exact(aw) * dswish_exact(ad), td, sd);
    sw = fmaf(g * swish_exact(ad) * dswish_exact(aw), tw, sw);
  }
  sd = shfl_sum64(sd);
  sw = shfl_sum64(sw);
  if (lane == 0) {
    if (d_dist) d_dist[e] = sd;
    if (d_weight) d_weight[e] = sw;
  }
}

// base branch, one LocalAttention layer: geomL = swish(pre) * weight, pre = G(dist).Wf + bf (attention.py:159-163).
// d weight += sum_c dgeomL * swish(pre); d dist += sum_c dgeomL * weight * swish'(pre) * sum_k Wf[k,c] * G_k'(dist).
// Adds to d_dist / d_weight (zeroed by the caller): one launch per layer on one stream, layer order, so the sum's order is fixed.
__global__ __launch_bounds__(256) void base_input_grad_kernel(const float* __restrict__ dist, const float* __restrict__ weight,
                                                              const float* __restrict__ dgeomL, const float* __restrict__ Wf,
                                                              const float* __restrict__ bf, const float* __restrict__ cd, int n_edge,
                                                              int width, float* __restrict__ d_dist,
                                                              float* __restrict__ d_weight) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * IG_WAVES + (threadIdx.x >> 6);
  if (e >= n_edge) return;
  float gd[NG], dgd[NG];
  gauss20(dist[e], cd, gd, dgd);
  const float w = weight[e];
  const float* __restrict__ dg = dgeomL + (size_t)e * width;
  float sd = 0.f, sw = 0.f;
  for (int c = lane; c < width; c += 64) {
    float pre = bf[c], t = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const float wk = Wf[(size_t)k * width + c];
      pre = fmaf(gd[k], wk, pre);
      t = fmaf(dgd[k], wk, t);
    }
    const float g = dg[c];
    sw = fmaf(g, swish_exact(pre), sw);
    sd = fmaf(g * w * dswish_exact(pre), t, sd);
  }
  sd = shfl_sum64(sd);
  sw = shfl_sum64(sw);
  if (lane == 0) {
    if (d_dist) d_dist[e] += sd;
    if (d_weight) d_weight[e] += sw;
  }
}

// Embedding leaf, one atom per workgroup (scann_model.py:362-373): v = [embed_atom(x) | extra_embed(ring)], c0 = swish(v.Wde + bde).
// dpre = dC * swish'(pre), dv = dpre.Wde^T, d ring = dv[emb:emb+10].Wr^T, d cgcnn = dv[0:emb].We^T (both Dense layers are linear).
// LDS: v [cin] | dv [cin] | dpre [width] floats (dynamic).
__global__ __launch_bounds__(256) void embed_input_grad_kernel(InputGradEmbed a) {
  extern __shared__ float lds[];
  const int cin = a.emb_dim + (a.ring ? 10 : 0);
  float* v = lds;
  float* dv = lds + cin;
  float* dpre = lds + 2 * cin;
  const int atom = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = a.width, emb = a.emb_dim;
  for (int t = tid; t < emb; t += blockDim.x) {
    float x;
    if (a.cgcnn) {
      x = a.be[t];
      const float* __restrict__ f = a.cgcnn + (size_t)atom * 92;
      for (int j = 0; j < 92; ++j) x = fmaf(f[j], a.We[(size_t)j * emb + t], x);
    } else {
      x = a.emb[(size_t)a.atomic[atom] * emb + t];
    }
    v[t] = x;
  }
  if (a.ring && tid < 10) {
    const float r0 = a.ring[(size_t)atom * 2], r1 = a.ring[(size_t)atom * 2 + 1];
    v[emb + tid] = fmaf(r1, a.Wr[10 + tid], fmaf(r0, a.Wr[tid], a.br[tid]));
  }
  __syncthreads();
  for (int c = tid; c < W; c += blockDim.x) {
    float pre = a.bde[c];
    for (int k = 0; k < cin; ++k) pre = fmaf(v[k], a.Wde[(size_t)k * W + c], pre);
    dpre[c] = a.dC[(size_t)atom * W + c] * dswish_exact(pre);
  }
  __syncthreads();
  for (int k = wave; k < cin; k += (int)(blockDim.x >> 6)) {  // row k of Wde against dpre: one wave, lanes over the columns
    float s = 0.f;
    for (int c = lane; c < W; c += 64) s = fmaf(dpre[c], a.Wde[(size_t)k * W + c], s);
    s = shfl_sum64(s);
    if (lane == 0) dv[k] = s;
  }
  __syncthreads();
  if (a.d_ring && tid < 2) {
    float s = 0.f;
    for (int j = 0; j < 10; ++j) s = fmaf(dv[emb + j], a.Wr[tid * 10 + j], s);
    a.d_ring[(size_t)atom * 2 + tid] = s;
  }
  if (a.d_cgcnn) {
    for (int t = tid; t < 92; t += blockDim.x) {
      float s = 0.f;
      for (int k = 0; k < emb; ++k) s = fmaf(dv[k], a.We[(size_t)t * emb + k], s);
      a.d_cgcnn[(size_t)atom * 92 + t] = s;
    }
  }
}

}  // namespace

void launch_basis_input_grad(const float* dist, const float* weight, const float* dG0, const float* Wd, const float* bd, const float* Ww,
                             const float* bw, const float* cd, const float* cw, int n_edge, int width, float* d_dist, float* d_weight,
                             hipStream_t s) {
  if (n_edge <= 0) return;
  hipLaunchKernelGGL(basis_input_grad_kernel, dim3((n_edge + IG_WAVES - 1) / IG_WAVES), dim3(64 * IG_WAVES), 0, s, dist, weight, dG0, Wd, bd,
                     Ww, bw, cd, cw, n_edge, width, d_dist, d_weight);
}

void launch_base_input_grad(const float* dist, const float* weight, const float* dgeomL, const float* Wf, const float* bf, const float* cd,
                            int n_edge, int width, float* d_dist, float* d_weight, hipStream_t s) {
  if (n_edge <= 0) return;
  hipLaunchKernelGGL(base_input_grad_kernel, dim3((n_edge + IG_WAVES - 1) / IG_WAVES), dim3(64 * IG_WAVES), 0, s, dist, weight, dgeomL, Wf,
                     bf, cd, n_edge, width, d_dist, d_weight);
}

size_t embed_input_grad_lds(int emb_dim, bool ring, int width) {
  return (size_t)(2 * (emb_dim + (ring ? 10 : 0)) + width) * sizeof(float);
}

void launch_embed_input_grad(const InputGradEmbed& a, int n_atom, hipStream_t s) {
  if (n_atom <= 0) return;
  hipLaunchKernelGGL(embed_input_grad_kernel, dim3(n_atom), dim3(256), embed_input_grad_lds(a.emb_dim, a.ring != nullptr, a.width), s, a);
}

}  // namespace scann

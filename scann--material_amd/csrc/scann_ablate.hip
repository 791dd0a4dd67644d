// Ablated poolings (scann_ablate_pooling): y(S) of the readout for many kept sets S of one structure's atoms, from the resident gq / gk of
// ONE forward.  In the reference atom_mask feeds nothing but GlobalAttention (scann_model.py:329-447), so "atom_mask = 1 on S, 0 elsewhere"
// is: e_i(S) = sum over j in S, j != i of k_i . q_j (attention.py:279-292), softmax over S of e / ||e|| (:295-302), rep = sum a_i k_i
// (:314-316), then bf_property / predict_property (scann_model.py:437-447).  One workgroup per structure walks its entries in tiles of 32:
//   pair tile   G[u][i] = k_i . q_c(u) for the 32 columns c(u) the tile's entries differ by, diagonal zeroed (mask_center, :282-285)
//   scores      leave-one-out: P[u][i] = e_i - G[u][i], e_i = the sum of ALL columns of row i, formed by a first walk over the tiles;
//               curves: P[u][i] = the running sum of G along the ranking (columns in rank order: each entry adds one column)
//   pooling     the reference's masked arithmetic on the n real atoms, literally: agg = m P, agg / ||agg|| (no epsilon), + (1 - m) * -1e9,
//               softmax, m * a -- so a one-atom or empty S under use_ga_norm is the reference's 0 / 0 = NaN, and finite without it
//   rep, head   A K and (rep Wb) as matrix products over the tile's 32 entries
// so a structure's n entries cost O(n^2 d): every pair product is formed once (twice for leave-one-out).  The 128-wide kernel runs the three
// products on v_mfma_f32_32x32x2_f32 (activations of unknown range: no split-fp16); the generic one is plain fp32 at any width and doubles
// as the implementation the MFMA one is cross-checked against (SCANN_GENERIC=1).  Everything else -- ranking, prefix sums, pooling -- is the
// same code.  No atomics, fixed summation orders, and nothing depends on the batch a structure sits in.
#include "../../include/scann_hip.h"
#include "scann_internal.h"
#include "scann_mma.h"

namespace scann {

namespace {

constexpr int AT = 32;  // entries (kept sets) per tile

// descending GlobalAttention score, ties by ascending atom index; a NaN score (the one-atom structure under use_ga_norm) ranks last
__device__ __forceinline__ float rank_key(float g) { return g != g ? -INFINITY : g; }

template <bool MFMA>
__device__ __forceinline__ void ablate_body(const AblateArgs& a) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = a.mol_offset[blockIdx.x], n = a.mol_offset[blockIdx.x + 1] - a0;
  if (n <= 0) return;
  const int dg = a.dg, dout = a.dout;
  const int T = (n + AT - 1) / AT, npad = T * AT;
  const int LP = npad + 2;   // row stride of sP: the A-operand reads of the rep product (lane = entry, two neighbouring atoms) hit 64 banks
  const int RS = dg + 4;     // row stride of sRep
  float* sP = sm;                                       // [32][LP] pair tile -> scores -> masked attention
  float* sBase = sP + AT * LP;                          // [npad] e_i (leave-one-out) / the running prefix sum at the tile's start (curves)
  float* sKey = sBase + npad;                           // [npad] ranking keys
  int* sSeq = reinterpret_cast<int*>(sKey + npad);      // [npad] curves: position in the walk -> atom
  int* sPos = sSeq + npad;                              // [npad] curves: atom -> position in the walk
  float* sRep = reinterpret_cast<float*>(sPos + npad);  // [32][RS] pooled rows of the tile
  float* sY = sRep + AT * RS;                           // [4][32] head partial sums per wave
  const float* __restrict__ gq = a.gq + (size_t)a0 * dg;
  const float* __restrict__ gk = a.gk + (size_t)a0 * dg;
  const int mode = a.mode;
  const bool loo = mode == SCANN_ABLATE_LEAVE_ONE_OUT, del = mode == SCANN_ABLATE_DELETION;

  // ---- ranking by the forward's scores; the walk of the curves: insertion adds atoms best first, deletion's kept sets grow worst first ----
  for (int i = tid; i < npad; i += 256) {
    sKey[i] = i < n ? rank_key(a.ga_attn[a0 + i]) : 0.f;
    sBase[i] = 0.f;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const float gi = sKey[i];
    int before = 0;
    for (int j = 0; j < n; ++j) {
      const float gj = sKey[j];
      before += (gj > gi || (gj == gi && j < i)) ? 1 : 0;
    }
    if (a.order) a.order[a0 + before] = i;
    const int pos = del ? n - 1 - before : before;
    sSeq[pos] = i;
    sPos[i] = pos;
  }
  __syncthreads();

  for (int pass = loo ? 0 : 1; pass < 2; ++pass) {
    for (int vt = 0; vt < T; ++vt) {
      const int g0 = vt * AT, nv = min(AT, n - g0);
      // ---- pair tile: sP[u][i] = k_i . q_c(u), c(u) = the atom entry g0 + u removes (leave-one-out) / the walk's atom g0 + u (curves) ----
      if constexpr (MFMA) {
        const int r = lane & 31, h = lane >> 5;
        const int cu = r < nv ? (loo ? g0 + r : sSeq[g0 + r]) : -1;
        const float4* q4 = reinterpret_cast<const float4*>(gq);
        const float4* k4 = reinterpret_cast<const float4*>(gk);
        float4 qa[16];  // features 8t + 4h .. + 3 of query row c(u): the k index of step (t, component) is h
#pragma unroll
        for (int t = 0; t < 16; ++t) qa[t] = cu >= 0 ? q4[(size_t)cu * 32 + 2 * t + h] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int it = wave; it < T; it += 4) {
          const int i = it * AT + r;
          f32x16 acc;
#pragma unroll
          for (int x = 0; x < 16; ++x) acc[x] = 0.f;
#pragma unroll
          for (int t0 = 0; t0 < 16; t0 += 4) {
            float4 kb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) kb[t] = i < n ? k4[(size_t)i * 32 + 2 * (t0 + t) + h] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t0 + t].x, kb[t].x, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t0 + t].y, kb[t].y, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t0 + t].z, kb[t].z, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t0 + t].w, kb[t].w, acc, 0, 0, 0);
            }
          }
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            const int u = acc_row(x, lane);
            const int c = u < nv ? (loo ? g0 + u : sSeq[g0 + u]) : -1;
            sP[u * LP + i] = c == i ? 0.f : acc[x];  // mask_center (:282-285)
          }
        }
      } else {
        for (int p = tid; p < nv * n; p += 256) {
          const int u = p / n, i = p - u * n;
          const int c = loo ? g0 + u : sSeq[g0 + u];
          const float* __restrict__ qr = gq + (size_t)c * dg;
          const float* __restrict__ kr = gk + (size_t)i * dg;
          float s = 0.f;
          for (int f = 0; f < dg; ++f) s = fmaf(kr[f], qr[f], s);
          sP[u * LP + i] = c == i ? 0.f : s;
        }
      }
      __syncthreads();
      // ---- scores: one thread per atom i runs down the tile's entries, columns in walk order ----
      for (int i = tid; i < n; i += 256) {
        float run = sBase[i];
        if (loo) {
          if (pass == 0) {
            for (int u = 0; u < nv; ++u) run += sP[u * LP + i];
            sBase[i] = run;  // after the last tile: e_i (:289-292)
          } else {
            for (int u = 0; u < nv; ++u) sP[u * LP + i] = run - sP[u * LP + i];
          }
        } else {
          for (int u = 0; u < nv; ++u) {  // insertion: entry g keeps the walk's first g + 1 atoms; deletion: its first g
            const float gv = sP[u * LP + i];
            if (del) sP[u * LP + i] = run;
            run += gv;
            if (!del) sP[u * LP + i] = run;
          }
          sBase[i] = run;
        }
      }
      __syncthreads();
      if (pass == 0) continue;
      // ---- pooling over the n real atoms with the reference's multiplicative mask (:292-302, :314), one wave per entry ----
      for (int u = wave; u < nv; u += 4) {
        const int g = g0 + u;
        float* row = sP + u * LP;
        const int cnt = del ? g : g + 1;
        auto mask_of = [&](int i) { return loo ? (i != g ? 1.f : 0.f) : (sPos[i] < cnt ? 1.f : 0.f); };
        float nrm = 1.f;
        if (a.use_ga_norm) {
          float ss = 0.f;
          for (int i = lane; i < n; i += 64) {
            const float v = mask_of(i) * row[i];
            ss += v * v;
          }
          nrm = sqrtf(wave_sum64(ss));  // tf.linalg.normalize: no epsilon
        }
        float m = -INFINITY;
        for (int i = lane; i < n; i += 64) {
          const float mk = mask_of(i);
          float v = mk * row[i];
          if (a.use_ga_norm) v = v / nrm;
          v = v + (1.0f - mk) * -1e9f;  // :299-300
          row[i] = v;
          m = fmaxf(m, v);
        }
        m = wave_max64(m);
        float ss = 0.f;
        for (int i = lane; i < n; i += 64) {
          const float e = expf(row[i] - m);
          row[i] = e;
          ss += e;
        }
        ss = wave_sum64(ss);
        for (int i = lane; i < n; i += 64) row[i] = mask_of(i) * (row[i] / ss);  // the mask of :314 (0 * NaN stays NaN, as there)
        for (int i = n + lane; i < npad; i += 64) row[i] = 0.f;
      }
      __syncthreads();
      // ---- rep[u] = sum_i a[u][i] k_i (:314-316) ----
      if constexpr (MFMA) {
        const int r = lane & 31, h = lane >> 5;
        f32x16 acc;
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[x] = 0.f;
        const float* __restrict__ kc = gk + 32 * wave + r;  // this wave's 32 features
        const float* __restrict__ ar = sP + r * LP + h;
        for (int i = 0; i < npad; i += 2) {
          const float kv = i + h < n ? kc[(size_t)(i + h) * D] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[i], kv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int x = 0; x < 16; ++x) sRep[acc_row(x, lane) * RS + 32 * wave + r] = acc[x];
      } else {
        for (int p = tid; p < nv * dg; p += 256) {
          const int u = p / dg, f = p - u * dg;
          float s = 0.f;
          for (int i = 0; i < n; ++i) s = fmaf(sP[u * LP + i], gk[(size_t)i * dg + f], s);
          sRep[u * RS + f] = s;
        }
      }
      __syncthreads();
      // ---- bf_property + predict_property (+ mrelu) per entry (scann_model.py:437-447) ----
      if constexpr (MFMA) {
        const int r = lane & 31, h = lane >> 5;
        f32x16 acc;
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[x] = 0.f;
        const float* __restrict__ wc = a.Wb + 32 * wave + r;  // this wave's 32 hidden units
        const float* __restrict__ rr = sRep + r * RS + h;
#pragma unroll 8
        for (int f = 0; f < D; f += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rr[f], wc[(size_t)(f + h) * D], acc, 0, 0, 0);
        const float bbo = a.bb[32 * wave + r], woo = a.wo[32 * wave + r];
#pragma unroll
        for (int x = 0; x < 16; ++x) {
          const float v = sum32(swish_exact(acc[x] + bbo) * woo);  // over this wave's 32 hidden units
          if (r == 0) sY[wave * AT + acc_row(x, lane)] = v;
        }
        __syncthreads();
        if (tid < nv) {
          float y = ((sY[tid] + sY[AT + tid]) + (sY[2 * AT + tid] + sY[3 * AT + tid])) + a.bo[0];
          if (a.relu_out) y = y < 0.f ? 0.f : y;  // mrelu forward (custom_layers.py:15); a NaN stays one, as in the reference
          a.y_abl[a0 + (del ? n - 1 - (g0 + tid) : g0 + tid)] = y;
        }
      } else {
        for (int u = wave; u < nv; u += 4) {
          float part = 0.f;
          for (int o = lane; o < dout; o += 64) {
            float s = 0.f;
            for (int f = 0; f < dg; ++f) s = fmaf(sRep[u * RS + f], a.Wb[(size_t)f * dout + o], s);
            part += swish_exact(s + a.bb[o]) * a.wo[o];
          }
          part = wave_sum64(part);
          if (lane == 0) {
            float y = part + a.bo[0];
            if (a.relu_out) y = y < 0.f ? 0.f : y;
            a.y_abl[a0 + (del ? n - 1 - (g0 + u) : g0 + u)] = y;
          }
        }
      }
      __syncthreads();  // sP / sRep / sY are the next tile's
    }
  }
}

__global__ __launch_bounds__(256) void ablate_kernel(AblateArgs a) { ablate_body<true>(a); }
__global__ __launch_bounds__(256) void gen_ablate_kernel(AblateArgs a) { ablate_body<false>(a); }

}  // namespace

size_t ablate_lds_bytes(int max_atoms, int dg) {
  const size_t npad = (size_t)((max_atoms + AT - 1) / AT) * AT;
  return (AT * (npad + 2) + 4 * npad + AT * ((size_t)dg + 4) + 4 * AT) * sizeof(float);
}

hipError_t launch_ablate(const AblateArgs& a, bool mfma, hipStream_t s) {
  if (a.n_struct <= 0) return hipSuccess;
  const size_t lds = ablate_lds_bytes(a.max_atoms, a.dg);
  const void* fn = mfma ? reinterpret_cast<const void*>(ablate_kernel) : reinterpret_cast<const void*>(gen_ablate_kernel);
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (mfma) hipLaunchKernelGGL(ablate_kernel, dim3(a.n_struct), dim3(256), lds, s, a);
  else hipLaunchKernelGGL(gen_ablate_kernel, dim3(a.n_struct), dim3(256), lds, s, a);
  return hipGetLastError();
}

}  // namespace scann

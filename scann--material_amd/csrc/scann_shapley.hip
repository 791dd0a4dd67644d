// Shapley sampling of the pooling game (scann_shapley): the players are the n real atoms of one structure, v(S) is the readout on the kept
// set S with everything upstream unchanged -- scann_ablate.hip's y(S) -- and the Shapley value of an atom is its marginal v(S + i) - v(S)
// averaged over the orders in which atoms can be added.  Sampled: n_perm random walks per structure, each the insertion walk of
// scann_ablate.hip along a permutation instead of along the GlobalAttention ranking.
//   shapley_pair_kernel    the pair matrix G[c][i] = k_i . q_c of a structure, diagonal zeroed (mask_center, attention.py:282-285), ONCE: it
//                          is the same for every walk, so the walks read its columns in walk order instead of redoing n^2 d products
//   shapley_walk_kernel    grid (structure, chunk of SHAPLEY_PCHUNK walks).  The workgroup makes the permutation in LDS (shapley_permutation
//                          of scann_internal.h: the draws in parallel, the swaps by one thread) or loads an explicit one, then walks its
//                          prefixes in tiles of 32 entries: pair columns in walk order, running sums per atom, the reference's masked
//                          pooling, rep = A K, head.  The 128-wide kernel runs rep and head on v_mfma_f32_32x32x2_f32, the generic one is
//                          plain fp32 at any width (and the cross-check of the other: SCANN_GENERIC=1).
//   shapley_reduce_kernel  fp64: per atom the mean of its marginals over the walks in order and the standard error of that mean (two
//                          passes), per structure the baseline v(empty) and the mean of v(all).  No fp contraction: the host twin
//                          (shapley_reduce_host) gives the same bits.
// The game below two atoms: with use_ga_norm the reference's pooling over one atom or none is 0 / 0, and every walk starts there.  For
// |S| <= 1 the arithmetic is that of use_ga_norm = false whatever the model's setting -- the continuous extension: a softmax over one kept
// atom is 1 for any finite logit, so v({i}) = head(k_i), and the empty pooling has rep = 0, v(empty) = head(0).  The full set keeps the
// forward's arithmetic, so a ONE-atom structure under use_ga_norm has v(all) = y = NaN, and NaN Shapley value.
// No atomics, fixed summation orders; nothing depends on the batch a structure sits in or on how the walks are cut into chunks.
#include "../../include/scann_hip.h"
#include "scann_internal.h"
#include "scann_mma.h"

namespace scann {

namespace {

constexpr int AT = 32;  // entries (prefixes) per tile, as in scann_ablate.hip

__global__ __launch_bounds__(256) void shapley_pair_kernel(ShapleyArgs a, int tiles) {
  const int s = blockIdx.x / tiles, c0 = (blockIdx.x - s * tiles) * AT;
  const int a0 = a.mol_offset[s], n = a.mol_offset[s + 1] - a0;
  if (c0 >= n) return;
  const int nv = min(AT, n - c0), dg = a.dg;
  const float* __restrict__ gq = a.gq + (size_t)a0 * dg;
  const float* __restrict__ gk = a.gk + (size_t)a0 * dg;
  float* __restrict__ G = a.pair + a.pair_offset[s];
  for (int p = threadIdx.x; p < nv * n; p += 256) {
    const int u = p / n, i = p - u * n, c = c0 + u;
    const float* __restrict__ qr = gq + (size_t)c * dg;
    const float* __restrict__ kr = gk + (size_t)i * dg;
    float e = 0.f;
    for (int f = 0; f < dg; ++f) e = fmaf(kr[f], qr[f], e);
    G[(size_t)c * n + i] = c == i ? 0.f : e;
  }
}

template <bool MFMA>
__device__ __forceinline__ void shapley_walk_body(const ShapleyArgs& a, int chunks) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x / chunks, p0 = (blockIdx.x - s * chunks) * SHAPLEY_PCHUNK, p1 = min(a.n_perm, p0 + SHAPLEY_PCHUNK);
  const int a0 = a.mol_offset[s], n = a.mol_offset[s + 1] - a0;
  if (n <= 0) return;
  const int dg = a.dg, dout = a.dout;
  const int T = (n + AT - 1) / AT, npad = T * AT;
  const int LP = npad + 2;   // the layout of ablate_body (ablate_lds_bytes): conflict-free A-operand reads of the rep product
  const int RS = dg + 4;
  float* sP = sm;                                       // [32][LP] pair columns -> scores -> masked attention
  float* sBase = sP + AT * LP;                          // [npad] the running prefix sum of every atom at the tile's start
  int* sDraw = reinterpret_cast<int*>(sBase + npad);    // [npad] the Fisher-Yates draws of the permutation
  int* sSeq = sDraw + npad;                             // [npad] position in the walk -> atom
  int* sPos = sSeq + npad;                              // [npad] atom -> position in the walk
  float* sRep = reinterpret_cast<float*>(sPos + npad);  // [32][RS] pooled rows of the tile
  float* sY = sRep + AT * RS;                           // [4][32] head partial sums per wave
  const float* __restrict__ gk = a.gk + (size_t)a0 * dg;
  const float* __restrict__ G = a.pair + a.pair_offset[s];
  const unsigned long long key = a.keys ? a.keys[s] : 0ull;

  for (int p = p0; p < p1; ++p) {
    const size_t row = (size_t)p * a.n_atom + a0;
    // ---- the walk: explicit, or shapley_permutation(seed, key, p, n) ----
    if (a.perms_in) {
      for (int i = tid; i < n; i += 256) sSeq[i] = a.perms_in[row + i];  // a permutation of 0 .. n - 1: checked on the host
    } else {
      const unsigned long long base = mc_seed(a.seed, (unsigned)p, key);
      for (int i = tid; i < n; i += 256) {
        sSeq[i] = i;
        sDraw[i] = i >= 1 ? (int)shapley_draw(base, i) : 0;  // 0 <= draw <= i
      }
      __syncthreads();
      if (tid == 0) {
        for (int i = n - 1; i >= 1; --i) {
          const int k = sDraw[i], t = sSeq[i];
          sSeq[i] = sSeq[k];
          sSeq[k] = t;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < npad; i += 256) {
      sBase[i] = 0.f;
      if (i < n) {
        const int c = sSeq[i];
        sPos[c] = i;
        a.perms[row + i] = c;
      }
    }
    __syncthreads();

    for (int vt = 0; vt < T; ++vt) {
      const int g0 = vt * AT, nv = min(AT, n - g0);
      // ---- pair columns in walk order: sP[u][i] = k_i . q_c(u), c(u) = the atom entry g0 + u adds; rows past the walk's end zero ----
      for (int q = tid; q < nv * n; q += 256) {
        const int u = q / n, i = q - u * n;
        sP[u * LP + i] = G[(size_t)sSeq[g0 + u] * n + i];
      }
      for (int q = nv * npad + tid; q < AT * npad; q += 256) {
        const int u = q / npad, i = q - u * npad;
        sP[u * LP + i] = 0.f;
      }
      __syncthreads();
      // ---- scores: one thread per atom i runs down the tile's entries; entry g keeps the walk's first g + 1 atoms ----
      for (int i = tid; i < n; i += 256) {
        float run = sBase[i];
        for (int u = 0; u < nv; ++u) {
          run += sP[u * LP + i];
          sP[u * LP + i] = run;
        }
        sBase[i] = run;
      }
      __syncthreads();
      // ---- pooling over the n real atoms with the reference's multiplicative mask (attention.py:292-302, :314), one wave per entry ----
      for (int u = wave; u < nv; u += 4) {
        const int cnt = g0 + u + 1;
        float* row_u = sP + u * LP;
        const bool norm = a.use_ga_norm && (cnt >= 2 || n == 1);  // one kept atom of several: the arithmetic of use_ga_norm = false
        auto mask_of = [&](int i) { return sPos[i] < cnt ? 1.f : 0.f; };
        float nrm = 1.f;
        if (norm) {
          float ss = 0.f;
          for (int i = lane; i < n; i += 64) {
            const float v = mask_of(i) * row_u[i];
            ss += v * v;
          }
          nrm = sqrtf(wave_sum64(ss));  // tf.linalg.normalize: no epsilon
        }
        float m = -INFINITY;
        for (int i = lane; i < n; i += 64) {
          const float mk = mask_of(i);
          float v = mk * row_u[i];
          if (norm) v = v / nrm;
          v = v + (1.0f - mk) * -1e9f;  // :299-300
          row_u[i] = v;
          m = fmaxf(m, v);
        }
        m = wave_max64(m);
        float ss = 0.f;
        for (int i = lane; i < n; i += 64) {
          const float e = expf(row_u[i] - m);
          row_u[i] = e;
          ss += e;
        }
        ss = wave_sum64(ss);
        for (int i = lane; i < n; i += 64) row_u[i] = mask_of(i) * (row_u[i] / ss);  // the mask of :314 (0 * NaN stays NaN, as there)
        for (int i = n + lane; i < npad; i += 64) row_u[i] = 0.f;
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
        for (int q = tid; q < nv * dg; q += 256) {
          const int u = q / dg, f = q - u * dg;
          float e = 0.f;
          for (int i = 0; i < n; ++i) e = fmaf(sP[u * LP + i], gk[(size_t)i * dg + f], e);
          sRep[u * RS + f] = e;
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
          a.values[row + g0 + tid] = y;
        }
      } else {
        for (int u = wave; u < nv; u += 4) {
          float part = 0.f;
          for (int o = lane; o < dout; o += 64) {
            float e = 0.f;
            for (int f = 0; f < dg; ++f) e = fmaf(sRep[u * RS + f], a.Wb[(size_t)f * dout + o], e);
            part += swish_exact(e + a.bb[o]) * a.wo[o];
          }
          part = wave_sum64(part);
          if (lane == 0) {
            float y = part + a.bo[0];
            if (a.relu_out) y = y < 0.f ? 0.f : y;
            a.values[row + g0 + u] = y;
          }
        }
      }
      __syncthreads();  // sP / sRep / sY are the next tile's, sSeq / sPos the next walk's
    }
  }
}

__global__ __launch_bounds__(256) void shapley_walk_kernel(ShapleyArgs a, int chunks) { shapley_walk_body<true>(a, chunks); }
__global__ __launch_bounds__(256) void gen_shapley_walk_kernel(ShapleyArgs a, int chunks) { shapley_walk_body<false>(a, chunks); }

constexpr int RPT = (SCANN_ABLATE_MAX_ATOMS + 255) / 256;  // atoms per thread of the reduction

// the marginal of the atom at position j of a walk whose prefix values are v[0 .. n - 1]
__host__ __device__ inline double shapley_marginal(const float* v, int j, double baseline) {
  return (double)v[j] - (j ? (double)v[j - 1] : baseline);
}

__global__ __launch_bounds__(256) void shapley_reduce_kernel(ShapleyArgs a) {
#pragma clang fp contract(off)
  __shared__ int sInv[RPT * 256];
  __shared__ double sBaseline;
  const int tid = threadIdx.x, s = blockIdx.x;
  const int a0 = a.mol_offset[s], n = a.mol_offset[s + 1] - a0, P = a.n_perm;
  const size_t A = (size_t)a.n_atom;
  if (tid == 0) {
    // v(empty): the head on rep = 0 (scann_model.py:437-447), hidden units in index order
    float acc = 0.f;
    for (int o = 0; o < a.dout; ++o) acc += swish_exact(a.bb[o]) * a.wo[o];
    float y = acc + a.bo[0];
    if (a.relu_out) y = y < 0.f ? 0.f : y;
    const double b = (double)y;
    double f = 0.0;
    for (int p = 0; p < P && n > 0; ++p) f += (double)a.values[p * A + a0 + n - 1];
    a.baseline[s] = b;
    a.full[s] = n > 0 ? f / (double)P : b;
    sBaseline = b;
  }
  __syncthreads();
  if (n <= 0) return;
  const double base = sBaseline;
  double sum[RPT], mean[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) sum[r] = mean[r] = 0.0;
  const int K = max(1, min(8, RPT * 256 / n));  // walks inverted per barrier pair: K * n <= the ints of sInv
  for (int pass = 0; pass < 2; ++pass) {
    for (int p0 = 0; p0 < P; p0 += K) {
      const int kn = min(K, P - p0);
      for (int q = tid; q < kn * n; q += 256) {
        const int k = q / n, j = q - k * n;
        sInv[k * n + a.perms[(p0 + k) * A + a0 + j]] = j;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        const int i = tid + 256 * r;
        if (i < n) {
          for (int k = 0; k < kn; ++k) {  // walks in order
            const double m = shapley_marginal(a.values + (p0 + k) * A + a0, sInv[k * n + i], base);
            if (pass == 0) {
              sum[r] += m;
            } else {
              const double d = m - mean[r];
              sum[r] += d * d;
            }
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int i = tid + 256 * r;
      if (pass == 0) {
        mean[r] = sum[r] / (double)P;
        sum[r] = 0.0;
        if (i < n) a.shapley[a0 + i] = mean[r];
      } else if (i < n) {
        a.stderr_out[a0 + i] = sqrt(sum[r] / (double)(P - 1) / (double)P);  // one walk: 0 / 0 = NaN
      }
    }
  }
}

}  // namespace

void shapley_reduce_host(const float* values, const int32_t* perms, const int32_t* mol_offset, int n_struct, int n_perm, const double* baseline,
                         double* shapley, double* stderr_out, double* full) {
#pragma clang fp contract(off)
  const size_t A = n_struct > 0 ? (size_t)mol_offset[n_struct] : 0;
  const int P = n_perm;
  std::vector<int> inv;
  for (int s = 0; s < n_struct; ++s) {
    const int a0 = mol_offset[s], n = mol_offset[s + 1] - a0;
    const double base = baseline[s];
    double f = 0.0;
    for (int p = 0; p < P && n > 0; ++p) f += (double)values[p * A + a0 + n - 1];
    full[s] = n > 0 ? f / (double)P : base;
    if (n <= 0) continue;
    inv.assign((size_t)P * n, 0);
    for (int p = 0; p < P; ++p)
      for (int j = 0; j < n; ++j) inv[(size_t)p * n + perms[p * A + a0 + j]] = j;
    for (int i = 0; i < n; ++i) {
      double sum = 0.0;
      for (int p = 0; p < P; ++p) sum += shapley_marginal(values + p * A + a0, inv[(size_t)p * n + i], base);
      const double mean = sum / (double)P;
      sum = 0.0;
      for (int p = 0; p < P; ++p) {
        const double d = shapley_marginal(values + p * A + a0, inv[(size_t)p * n + i], base) - mean;
        sum += d * d;
      }
      shapley[a0 + i] = mean;
      stderr_out[a0 + i] = sqrt(sum / (double)(P - 1) / (double)P);
    }
  }
}

hipError_t launch_shapley(const ShapleyArgs& a, bool mfma, hipStream_t s, hipEvent_t* ev) {
  if (a.n_struct <= 0) return hipSuccess;
  const size_t lds = ablate_lds_bytes(a.max_atoms, a.dg);
  const void* fn = mfma ? reinterpret_cast<const void*>(shapley_walk_kernel) : reinterpret_cast<const void*>(gen_shapley_walk_kernel);
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int tiles = (a.max_atoms + AT - 1) / AT, chunks = (a.n_perm + SHAPLEY_PCHUNK - 1) / SHAPLEY_PCHUNK;
  if (ev) (void)hipEventRecord(ev[0], s);
  if (a.n_atom > 0) {
    hipLaunchKernelGGL(shapley_pair_kernel, dim3((unsigned)a.n_struct * tiles), dim3(256), 0, s, a, tiles);
    if (ev) (void)hipEventRecord(ev[1], s);
    if (mfma) hipLaunchKernelGGL(shapley_walk_kernel, dim3((unsigned)a.n_struct * chunks), dim3(256), lds, s, a, chunks);
    else hipLaunchKernelGGL(gen_shapley_walk_kernel, dim3((unsigned)a.n_struct * chunks), dim3(256), lds, s, a, chunks);
  } else if (ev) {
    (void)hipEventRecord(ev[1], s);
  }
  if (ev) (void)hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(shapley_reduce_kernel, dim3(a.n_struct), dim3(256), 0, s, a);
  if (ev) (void)hipEventRecord(ev[3], s);
  return hipGetLastError();
}

}  // namespace scann

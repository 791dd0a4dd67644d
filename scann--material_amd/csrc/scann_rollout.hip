// Attention rollout (scann_attention_rollout; Abnar & Zuidema 2020): the attention maps of the first `depth` LocalAttention layers of ONE
// forward composed per structure.  Layer l acts on a row-stochastic R [n, n] (local atom indices) as
//   (T_l R)[i, :] = residual * R[i, :] + (1 - residual) * sum over the edges e of atom i, in CSR order, of abar[l][e] * R[col(e), :]
// (an atom without edges keeps its row: its context is the LayerNorm of its own query), abar = the mean over the heads in index order
// times 1 / H, or one head; R = T_{depth-1} .. T_0 I; attribution[j] = sum over i, ascending, of ga[i] * R[i, j].
//
// Two launches.  rollout_abar_kernel forms abar [depth][n_edge] once per batch (every column slab of a structure needs the same weights).
// rollout_kernel<C>: T_l acts on rows, so the columns of R are independent: one workgroup owns C columns of one structure, keeps its slab
// [n][C] twice (in / out) in LDS and runs all the layers there, a __syncthreads() between them; global traffic is abar and the edge
// indices only.  At the end it writes its slab of R (if asked for) and attribution for its C columns.  Grid = structures x column slabs of
// the batch's largest structure; slabs past a structure's n leave at once.
//
// Lane mapping and LDS banks.  Lane = column, 64 / C rows per wave, 1024 threads per workgroup.  A row's C lanes load C of its edges at once
// (index and weight, coalesced) and pass them round with __shfl in CSR order, so a row costs one global round trip per C edges and the 16
// waves of the workgroup hide each other's (a first version with one broadcast load per edge and 256 threads spent 0.1 - 0.25 us per edge
// waiting: profiles/rollout_rate.txt).  The gather itself is a ds_read_b32, serviced per 32-lane half over 64 banks, so
//   C = 64 (structures of 33 .. 128 atoms) and C = 32 (up to 32, and 129 .. 512 atoms): a half reads 32 consecutive words of ONE slab row --
//     no two lanes of a half share a bank whatever the neighbour rows are: 0 conflict cycles by construction;
//   C = 16 (513 .. 960 atoms, 2 x n x 16 x 4 bytes + the offsets <= 124 KiB): a half reads two slab rows of 16 words at stride 16, which meet on a
//     bank when the two neighbour rows differ and are congruent modulo 4 -- two-way at worst.  Counted offline over the indices of the test
//     batches (tools/rollout_rate.py --conflicts): 0 extra cycles on the QM9- and MP2018-shaped batches of 128 (C = 32), 23.8 % extra gather
//     cycles on the 960-atom structure (1 in 4 random pairs, as expected).  One row per half with 16 idle lanes would remove it at half the
//     lane occupancy of the gather, which costs more than a quarter.  Measured (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/rollout_rate.txt): 0 on the QM9
//     batch, 8.4 % of all LDS cycles on the 960-atom structure -- a step is two shuffles and one gather, so a quarter of the gathers.
// C is chosen by the batch's largest structure, which changes no bit: every entry R[i, j] is the same chain of fmaf over atom i's edges in
// CSR order in every instantiation (explicit fmaf: nothing is left to contraction), no atomics, no dependence on the batch.
#include "../../include/scann_hip.h"
#include "scann_internal.h"

#include <algorithm>

namespace scann {

namespace {

__global__ __launch_bounds__(256) void rollout_abar_kernel(const float* __restrict__ attn, size_t n, int H, int head, float* __restrict__ abar) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;  // l * n_edge + e: the layers lie one after another in both arrays
  if (idx >= n) return;
  const float* __restrict__ p = attn + idx * (size_t)H;
  if (head >= 0) {
    abar[idx] = p[head];
    return;
  }
  float s = p[0];
  for (int k = 1; k < H; ++k) s += p[k];
  abar[idx] = s * (1.0f / (float)H);
}

constexpr int RT = 1024;  // threads per workgroup: 16 waves whose rows' index loads overlap

template <int C>
__global__ __launch_bounds__(RT) void rollout_kernel(RolloutArgs a) {
  extern __shared__ float sm[];
  const int s = blockIdx.x, c0 = blockIdx.y * C;
  const int a0 = a.mol_offset[s], n = a.mol_offset[s + 1] - a0;
  if (c0 >= n) return;
  constexpr int RP = RT / C;  // rows per pass of the workgroup
  const int tid = threadIdx.x, c = tid % C, r0 = tid / C;
  float* in = sm;
  float* out = sm + (size_t)n * C;
  int* eo = reinterpret_cast<int*>(sm + (size_t)2 * n * C);  // [n + 1] the structure's edge offsets
  for (int i = tid; i <= n; i += RT) eo[i] = a.edge_offset[a0 + i];
  for (int i = r0; i < n; i += RP) in[i * C + c] = i == c0 + c ? 1.f : 0.f;
  __syncthreads();
  const float res = a.residual, om = 1.0f - a.residual;
  const int32_t* __restrict__ col = a.edge_col;
  for (int l = 0; l < a.depth; ++l) {
    const float* __restrict__ ab = a.abar + (size_t)l * a.n_edge;
    for (int i = r0; i < n; i += RP) {
      const int e0 = eo[i], e1 = eo[i + 1];
      const float x = in[i * C + c];
      float v = x;
      if (e1 > e0) {
        float acc = 0.f;
        // the row's C lanes fetch C edges at once (one coalesced load each of the index and the weight) and hand them round in CSR order
        for (int eb = e0; eb < e1; eb += C) {
          const int m = min(C, e1 - eb);
          int jv = 0;
          float wv = 0.f;
          if (c < m) {
            jv = col[eb + c] - a0;
            wv = ab[eb + c];
          }
          for (int t = 0; t < m; ++t) acc = fmaf(__shfl(wv, t, C), in[__shfl(jv, t, C) * C + c], acc);
        }
        const float t = om * acc;
        v = fmaf(res, x, t);
      }
      out[i * C + c] = v;
    }
    __syncthreads();
    float* t = in;
    in = out;
    out = t;
  }
  if (a.rollout && c0 + c < n) {
    float* __restrict__ R = a.rollout + a.roll_offset[s];
    for (int i = r0; i < n; i += RP) R[(size_t)i * n + c0 + c] = in[i * C + c];
  }
  for (int i = tid; i < n; i += RT) out[i] = a.ga[a0 + i];  // (the spare slab: nothing reads it any more)
  __syncthreads();
  if (tid < C && c0 + tid < n) {
    float acc = 0.f;
#pragma unroll 8
    for (int i = 0; i < n; ++i) acc = fmaf(out[i], in[i * C + tid], acc);
    a.attribution[a0 + c0 + tid] = acc;
  }
}

template <int C>
hipError_t launch_c(const RolloutArgs& a, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rollout_kernel<C>, dim3(a.n_struct, (a.max_atoms + C - 1) / C), dim3(RT), lds, s, a);
  return hipGetLastError();
}

}  // namespace

int rollout_slab(int max_atoms) { return max_atoms <= 32 ? 32 : max_atoms <= 128 ? 64 : max_atoms <= 512 ? 32 : 16; }

size_t rollout_lds_bytes(int max_atoms) {  // two slabs [n][C] and the structure's n + 1 edge offsets
  const size_t n = (size_t)std::max(max_atoms, 1);
  return (2 * n * rollout_slab(max_atoms) + n + 1) * sizeof(float);
}

hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s) {
  if (a.n_struct <= 0 || a.max_atoms <= 0) return hipSuccess;
  const size_t n_ab = a.attn ? (size_t)a.depth * a.n_edge : 0;
  if (n_ab) {
    hipLaunchKernelGGL(rollout_abar_kernel, dim3((unsigned)((n_ab + 255) / 256)), dim3(256), 0, s, a.attn, n_ab, a.num_head, a.head, a.abar);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const size_t lds = rollout_lds_bytes(a.max_atoms);
  switch (rollout_slab(a.max_atoms)) {
    case 64: return launch_c<64>(a, lds, s);
    case 32: return launch_c<32>(a, lds, s);
    default: return launch_c<16>(a, lds, s);
  }
}

}  // namespace scann

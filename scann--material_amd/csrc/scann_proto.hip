// Prototypes and criticisms of a latent-space index (MMD-critic; scann_index_prototypes, scann_index_criticisms, include/scann_hip.h).
// Both are greedy selections whose pick folds one kernel column into a per-row integer state and re-ranks every row:
//   t(i, c) = peaks_term(dist2(P[i], P[c]), gamma),   dist2 the fp32 chain of scann_knn_distsq (columns ascending), t of scann_peaks.h;
//   prototypes  B_i += t(i, c),                 score_i = (s + 1) A_i - n B_i           (int64, s = picks made);
//   criticisms  Cmax_i = max(Cmax_i, t(i, c)),  score_i = weight_i (2^30 - Cmax_i)      (int64).
// The pick is the first live row under the total order (score descending, position ascending).
//
// The picks are strictly sequential; one launch of proto_step_kernel makes one pick and the stream orders them, as in scann_select.hip
// whose tile walk this is: a launch reads the previous pick's position from device memory (ProtoState), a workgroup of 256 lanes walks
// tiles of 256 rows, one lane per row; the rows go through LDS in slabs of 32 columns, column-major (the next slab is fetched into
// registers meanwhile), the pick's row sits in LDS and is read as a broadcast.  A chain is never split over lanes, so its bits do not
// depend on the launch geometry.  At the end of its row's chain the lane forms the term in registers, folds it and brings its candidate
// up to date.  Each lane keeps its first row under the order, the workgroup reduces them by comparisons of (score, position) and leaves
// one candidate; the workgroup that arrives last at an integer ticket counter reduces the candidates the same way, records the pick and
// marks the row.  A prototype launch that finds all picks made only folds the last column, so B is the sum over every pick.  No float
// atomics, no scratch.
//
// Visibility inside a launch (the XCDs' L2s are private): a candidate is two words, a 64-bit score and a 32-bit position.  Both are
// write-through stores, and both have left the lane (s_waitcnt vmcnt(0)) before the lane adds to the ticket; the last workgroup reads
// them with loads that bypass its L1.  Everything else (A, B, Cmax, live, ProtoState) is written by one launch and read by the next.
#include "scann_proto.h"

#include <algorithm>

namespace scann {

namespace {

constexpr int PT_RS = PT_SLAB * PT_LANES + 64;  // floats of the staged slab: column c of row i at [c * 256 + 8 * (c / 4) + i]
constexpr int PT_CENTRE = 1024;                 // the pick's row (dim <= 1024), zero behind stride
constexpr int PT_SMEM = PT_RS + PT_CENTRE + 16; // ... then the waves' 4 scores (8 bytes each), their 4 positions and the "last workgroup" word

// candidate x before candidate y: larger score, then lower position; a candidate without a row is behind every other
__device__ __forceinline__ bool pt_before(long long vx, int32_t px, long long vy, int32_t py) {
  if (px < 0) return false;
  if (py < 0) return true;
  return vx > vy || (vx == vy && px < py);
}
__device__ __forceinline__ void pt_wave_first(long long& v, int32_t& p) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long ov = __shfl_xor(v, off);
    const int32_t op = __shfl_xor(p, off);
    if (pt_before(ov, op, v, p)) v = ov, p = op;
  }
}

// one lane per row: the self-join left S_i (the sum over j != i, -1 for an ineligible row) in A
__global__ __launch_bounds__(PT_LANES) void proto_prepare_kernel(ProtoArgs a) {
  const int p = blockIdx.x * PT_LANES + threadIdx.x;
  bool ok = false;
  if (p < a.n_total) {
    const long long s = a.A[p];
    ok = s >= 0;
    if (ok) a.A[p] = s + PT_ONE;
    a.live[p] = ok ? PT_LIVE : PT_OUT;
  }
  const unsigned long long c = (unsigned long long)__popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(reinterpret_cast<unsigned long long*>(&a.st->n), c);
}

// the eligibility scan (scann_prim.h)
__global__ __launch_bounds__(PT_LANES) void crit_prepare_kernel(ProtoArgs a) {
  eligible_scan(a.rows, a.chunk_rows, a.stride, a.n_total, NoExtra{}, [&](int p, int bad) { a.live[p] = !bad && a.A[p] > 0 ? PT_LIVE : PT_OUT; });
}

__global__ __launch_bounds__(PT_LANES) void crit_exclude_kernel(ProtoArgs a, const int32_t* ex, int32_t n_ex) {
  const int i = blockIdx.x * PT_LANES + threadIdx.x;
  if (i >= n_ex) return;
  const int32_t p = ex[i];
  if (p >= 0 && p < a.n_total) a.live[p] = PT_OUT;
}

template <bool CRIT>
__global__ __launch_bounds__(PT_LANES) void proto_step_kernel(ProtoArgs a) {
  __shared__ float4 pt_smem[PT_SMEM / 4];
  float* rs = reinterpret_cast<float*>(pt_smem);
  float* centre = rs + PT_RS;
  long long* redv = reinterpret_cast<long long*>(centre + PT_CENTRE);  // [4]
  int32_t* redp = reinterpret_cast<int32_t*>(redv + 4);                // [4]
  int* last = redp + 4;
  const int t = threadIdx.x;
  const ProtoState st = *a.st;
  if (st.done) return;  // (uniform)
  const int cur = st.cur1 - 1;
  const bool fold_only = !CRIT && st.count >= a.n_pick;  // (uniform) every pick is made: the last column is still to be folded
  const long long s1 = (long long)st.count + 1, n_el = st.n;
  const int stride = a.stride, n_slab = (stride + PT_SLAB - 1) / PT_SLAB;
  const int G = gridDim.x;
  const int n_my = (a.n_tile - (int)blockIdx.x + G - 1) / G;  // tiles blockIdx.x, blockIdx.x + G, ...
  if (cur >= 0) {
    const float* c = tile_row(a.rows, cur, a.chunk_rows, stride);
    for (int j = t; j < n_slab * PT_SLAB; j += PT_LANES) centre[j] = j < stride ? c[j] : 0.f;
  }
  // tile k of this workgroup: its chunk, its first row there and how many rows it holds (<= 0: a tile behind the chunk's last row)
  auto tile_of = [&](int k, int& chunk, int& r0, int& nrow) {
    const int tile = blockIdx.x + k * G;
    chunk = tile / a.tiles_per_chunk;
    r0 = (tile % a.tiles_per_chunk) * PT_LANES;
    nrow = min(a.chunk_rows, a.n_total - chunk * a.chunk_rows) - r0;
  };
  long long bv = 0;
  int32_t bp = -1;
  // the lane's row of tile k has distance d to the latest pick: the column's term is folded into the row's state and the lane's
  // candidate brought up to date.  Tiles come in position order, so among equal scores the earlier row stays
  auto finish = [&](int k, float d) {
    int chunk, r0, nrow;
    tile_of(k, chunk, r0, nrow);
    if (t >= nrow) return;
    const int32_t p = chunk * a.chunk_rows + r0 + t;
    const uint8_t lv = a.live[p];
    if (lv == PT_OUT) return;
    long long score;
    if (CRIT) {
      if (lv != PT_LIVE) return;
      int32_t c = a.cmax[p];
      if (cur >= 0) {
        const int32_t term = peaks_term(d, a.gamma);
        if (term > c) {
          c = term;
          a.cmax[p] = c;
        }
      }
      score = a.A[p] * (PT_ONE - (long long)c);
    } else {
      long long b = a.B[p];
      if (cur >= 0) {
        b += (long long)peaks_term(d, a.gamma);
        a.B[p] = b;
      }
      if (lv != PT_LIVE || fold_only) return;
      score = s1 * a.A[p] - n_el * b;
    }
    if (bp < 0 || score > bv) bv = score, bp = p;
  };
  if (cur < 0) {
    for (int k = 0; k < n_my; ++k) finish(k, 0.f);
  } else {
    // one step = one slab of one tile: 256 rows x 32 columns = 8 float4 per lane, 8 lanes to a row's 128 bytes; rows / columns beyond
    // the end are zero.  Step s + 1 is fetched while step s is computed
    float4 g[8];
    auto fetch = [&](int step) {
      int chunk, r0, nrow;
      tile_of(step / n_slab, chunk, r0, nrow);
      const int c0 = (step % n_slab) * PT_SLAB;
      const float* __restrict__ rows = a.rows[chunk];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = t + PT_LANES * i, item = e >> 3, col = c0 + 4 * (e & 7);
        g[i] = item < nrow && col < stride ? *reinterpret_cast<const float4*>(rows + (size_t)(r0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
      }
    };
    const int n_step = n_my * n_slab;
    float acc = 0.f;
    if (n_step > 0) fetch(0);
    for (int step = 0; step < n_step; ++step) {
      __syncthreads();  // the previous slab's reads are over (first step: the pick's row is in place)
      // the 8 lanes of a row's 128 bytes store to 8 column groups, each shifted by 8 floats: the 64 lanes of a wave hit 64 banks
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = t + PT_LANES * i, item = e >> 3, c = 4 * (e & 7);
        float* d = rs + c * PT_LANES + 2 * c + item;
        d[0] = g[i].x; d[PT_LANES] = g[i].y; d[2 * PT_LANES] = g[i].z; d[3 * PT_LANES] = g[i].w;
      }
      __syncthreads();
      if (step + 1 < n_step) fetch(step + 1);
      const float* cs = centre + (step % n_slab) * PT_SLAB;
#pragma unroll
      for (int c = 0; c < PT_SLAB; ++c) {  // columns ascending: the chain of the definition
        const float d = rs[c * PT_LANES + 2 * (c & ~3) + t] - cs[c];  // rounded once; the square and the sum are one operation
        acc = __builtin_fmaf(d, d, acc);
      }
      if (step % n_slab != n_slab - 1) continue;
      finish(step / n_slab, acc);
      acc = 0.f;
    }
  }
  if (fold_only) return;
  // the workgroup's candidate
  pt_wave_first(bv, bp);
  __syncthreads();
  if ((t & 63) == 0) redv[t >> 6] = bv, redp[t >> 6] = bp;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < PT_LANES / 64; ++w)
      if (pt_before(redv[w], redp[w], bv, bp)) bv = redv[w], bp = redp[w];
    __hip_atomic_store(a.part_v + blockIdx.x, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // write-through, both words
    __hip_atomic_store(a.part_p + blockIdx.x, bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... and both out of this lane before the ticket says so
    const unsigned tk = __hip_atomic_fetch_add(&a.st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last = tk == (unsigned)G - 1;
  }
  __syncthreads();
  if (!*last) return;
  // the last workgroup: every candidate has arrived; read past this CU's L1
  bv = 0, bp = -1;
  for (int i = t; i < G; i += PT_LANES) {
    const long long ov = __hip_atomic_load(a.part_v + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t op = __hip_atomic_load(a.part_p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pt_before(ov, op, bv, bp)) bv = ov, bp = op;
  }
  pt_wave_first(bv, bp);
  __syncthreads();
  if ((t & 63) == 0) redv[t >> 6] = bv, redp[t >> 6] = bp;
  __syncthreads();
  if (t != 0) return;
  for (int w = 1; w < PT_LANES / 64; ++w)
    if (pt_before(redv[w], redp[w], bv, bp)) bv = redv[w], bp = redp[w];
  if (bp < 0 || st.count >= a.n_pick || (CRIT && bv <= 0)) {
    a.st->done = 1;
  } else {
    a.out_pos[st.count] = bp;
    a.out_score[st.count] = bv;
    a.st->count = st.count + 1;
    a.st->cur1 = bp + 1;
    a.live[bp] = PT_PICKED;
  }
  __hip_atomic_store(&a.st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t launch_proto_prepare(const ProtoArgs& a, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  hipLaunchKernelGGL(proto_prepare_kernel, dim3((unsigned)((a.n_total + PT_LANES - 1) / PT_LANES)), dim3(PT_LANES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_crit_prepare(const ProtoArgs& a, const int32_t* ex, int32_t n_ex, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  const int n_pass = (a.n_total + 31) / 32;
  hipLaunchKernelGGL(crit_prepare_kernel, dim3((unsigned)std::min(n_pass, 4 * PT_MAX_GROUPS)), dim3(PT_LANES), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && n_ex > 0) {
    hipLaunchKernelGGL(crit_exclude_kernel, dim3((unsigned)((n_ex + PT_LANES - 1) / PT_LANES)), dim3(PT_LANES), 0, s, a, ex, n_ex);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_proto_step(const ProtoArgs& a, bool crit, int groups, hipStream_t s) {
  if (a.n_total <= 0 || groups <= 0) return hipSuccess;
  if (crit) hipLaunchKernelGGL(proto_step_kernel<true>, dim3((unsigned)groups), dim3(PT_LANES), 0, s, a);
  else hipLaunchKernelGGL(proto_step_kernel<false>, dim3((unsigned)groups), dim3(PT_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

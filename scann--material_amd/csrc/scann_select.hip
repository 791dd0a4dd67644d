// Greedy k-center (farthest-point) selection over a latent-space index (scann_index_select, include/scann_hip.h).  Pick i is the first
// live row under the total order (mind descending, position ascending), mind[p] being the least
//   dist2(P[p], c) = acc_D,  acc_0 = 0,  acc_{j+1} = fmaf(P[p][j] - c[j], P[p][j] - c[j], acc_j)        (fp32, columns ascending)
// over the reference rows and the picks so far: the chain of scann_knn.hip, so the host twin gives the same bits.
//
// The picks are strictly sequential; one launch of kcenter_step_kernel makes one pick and the stream orders them.  A launch reads the
// previous pick's position from device memory (KcState), folds that centre into mind and selects: a workgroup of 256 lanes walks tiles
// of 256 rows, one lane per row.  The rows go through LDS in slabs of 32 columns, column-major, so that the global loads are whole
// 128-byte pieces of a row and a lane then reads its own row's column without a bank conflict (the next slab is fetched into registers
// meanwhile); the centre's row sits in LDS and is read as a broadcast.  A chain is never split over lanes, so its bits do not depend on
// the launch geometry.  Each lane keeps its first row under the order, the workgroup reduces them by comparisons of (mind, position)
// and leaves one 8-byte candidate; the workgroup that arrives last at an integer ticket counter reduces the candidates the same way,
// records the pick and marks the row.  When nothing is left, or the radius falls below stop_dist2, it sets `done` and every later launch
// returns at its first instruction.  No float atomics, no scratch.
//
// Visibility inside a launch (the XCDs' L2s are private): a candidate is one write-through 8-byte store that has left the lane
// (s_waitcnt vmcnt(0)) before the lane adds to the ticket, and the last workgroup reads the candidates with loads that bypass its L1.
// Everything else (mind, live, KcState) is written by one launch and read by the next.
#include "scann_select.h"

#include <algorithm>

namespace scann {

namespace {

constexpr int KC_RS = KC_SLAB * KC_LANES + 64;  // floats of the staged slab: column c of row i at [c * 256 + 8 * (c / 4) + i]
constexpr int KC_CENTRE = 1024;                 // the centre's row (dim <= 1024), zero behind stride
constexpr int KC_SMEM = KC_RS + KC_CENTRE + 16; // ... then 4 candidates of the waves (8 bytes each) and the "last workgroup" word

constexpr unsigned long long KC_NONE = 0xffffffffull;  // position -1: no live row

__device__ __forceinline__ unsigned long long kc_pack(float v, int32_t p) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)p;
}
// candidate x before candidate y: larger mind, then lower position; a candidate without a row is behind every other
__device__ __forceinline__ bool kc_before(unsigned long long x, unsigned long long y) {
  const int32_t px = (int32_t)(unsigned)x, py = (int32_t)(unsigned)y;
  if (px < 0) return false;
  if (py < 0) return true;
  const float vx = __uint_as_float((unsigned)(x >> 32)), vy = __uint_as_float((unsigned)(y >> 32));
  return vx > vy || (vx == vy && px < py);
}
__device__ __forceinline__ unsigned long long kc_wave_first(unsigned long long key) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    if (kc_before(o, key)) key = o;
  }
  return key;
}

// the eligibility scan (scann_prim.h)
__global__ __launch_bounds__(KC_LANES) void kcenter_prepare_kernel(KcArgs a, int has_init) {
  eligible_scan(a.rows, a.chunk_rows, a.stride, a.n_total, NoExtra{}, [&](int p, int bad) {
    a.live[p] = bad ? 0 : 1;
    if (!has_init) a.mind[p] = __builtin_inff();
  });
}

__global__ __launch_bounds__(KC_LANES) void kcenter_step_kernel(KcArgs a) {
  __shared__ float4 kc_smem[KC_SMEM / 4];
  float* rs = reinterpret_cast<float*>(kc_smem);
  float* centre = rs + KC_RS;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(centre + KC_CENTRE);  // [4]
  int* last = reinterpret_cast<int*>(red + 4);
  const int t = threadIdx.x;
  const KcState st = *a.st;
  if (st.done) return;  // (uniform)
  const int cur = st.cur1 - 1;
  const int stride = a.stride, n_slab = (stride + KC_SLAB - 1) / KC_SLAB;
  const int G = gridDim.x;
  const int n_my = (a.n_tile - (int)blockIdx.x + G - 1) / G;  // tiles blockIdx.x, blockIdx.x + G, ...
  if (cur >= 0) {
    const float* c = tile_row(a.rows, cur, a.chunk_rows, stride);
    for (int j = t; j < n_slab * KC_SLAB; j += KC_LANES) centre[j] = j < stride ? c[j] : 0.f;
  }
  // tile k of this workgroup: its chunk, its first row there and how many rows it holds (<= 0: a tile behind the chunk's last row)
  auto tile_of = [&](int k, int& chunk, int& r0, int& nrow) {
    const int tile = blockIdx.x + k * G;
    chunk = tile / a.tiles_per_chunk;
    r0 = (tile % a.tiles_per_chunk) * KC_LANES;
    nrow = min(a.chunk_rows, a.n_total - chunk * a.chunk_rows) - r0;
  };
  float bv = 0.f;
  int32_t bp = -1;
  // the lane's row of tile k has distance d to the centre: mind is brought up to date and the lane's candidate with it.  Tiles come in
  // position order, so among equal mind the earlier row stays
  auto finish = [&](int k, float d) {
    int chunk, r0, nrow;
    tile_of(k, chunk, r0, nrow);
    if (t >= nrow) return;
    const int32_t p = chunk * a.chunk_rows + r0 + t;
    if (!a.live[p]) return;
    float m = a.mind[p];
    if (cur >= 0 && d < m) {
      m = d;
      a.mind[p] = m;
    }
    if (bp < 0 || m > bv) bv = m, bp = p;
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
      const int c0 = (step % n_slab) * KC_SLAB;
      const float* __restrict__ rows = a.rows[chunk];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = t + KC_LANES * i, item = e >> 3, col = c0 + 4 * (e & 7);
        g[i] = item < nrow && col < stride ? *reinterpret_cast<const float4*>(rows + (size_t)(r0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
      }
    };
    const int n_step = n_my * n_slab;
    float acc = 0.f;
    if (n_step > 0) fetch(0);
    for (int step = 0; step < n_step; ++step) {
      __syncthreads();  // the previous slab's reads are over (first step: the centre is in place)
      // the 8 lanes of a row's 128 bytes store to 8 column groups, each shifted by 8 floats: the 64 lanes of a wave hit 64 banks
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = t + KC_LANES * i, item = e >> 3, c = 4 * (e & 7);
        float* d = rs + c * KC_LANES + 2 * c + item;
        d[0] = g[i].x; d[KC_LANES] = g[i].y; d[2 * KC_LANES] = g[i].z; d[3 * KC_LANES] = g[i].w;
      }
      __syncthreads();
      if (step + 1 < n_step) fetch(step + 1);
      const float* cs = centre + (step % n_slab) * KC_SLAB;
#pragma unroll
      for (int c = 0; c < KC_SLAB; ++c) {  // columns ascending: the chain of the definition
        const float d = rs[c * KC_LANES + 2 * (c & ~3) + t] - cs[c];  // rounded once; the square and the sum are one operation
        acc = __builtin_fmaf(d, d, acc);
      }
      if (step % n_slab != n_slab - 1) continue;
      finish(step / n_slab, acc);
      acc = 0.f;
    }
  }
  // the workgroup's candidate
  unsigned long long key = kc_wave_first(kc_pack(bv, bp));
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = key;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < KC_LANES / 64; ++w)
      if (kc_before(red[w], key)) key = red[w];
    __hip_atomic_store(a.part + blockIdx.x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // write-through
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... and out of this lane before the ticket says so
    const unsigned tk = __hip_atomic_fetch_add(&a.st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last = tk == (unsigned)G - 1;
  }
  __syncthreads();
  if (!*last) return;
  // the last workgroup: every candidate has arrived; read past this CU's L1
  key = KC_NONE;
  for (int i = t; i < G; i += KC_LANES) {
    const unsigned long long o = __hip_atomic_load(a.part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (kc_before(o, key)) key = o;
  }
  key = kc_wave_first(key);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = key;
  __syncthreads();
  if (t != 0) return;
  for (int w = 1; w < KC_LANES / 64; ++w)
    if (kc_before(red[w], key)) key = red[w];
  const int32_t p = (int32_t)(unsigned)key;
  const float v = __uint_as_float((unsigned)(key >> 32));
  if (p < 0 || st.count >= a.n_pick || (a.stop > 0.f && v < a.stop)) {
    a.st->done = 1;
  } else {
    a.out_pos[st.count] = p;
    a.out_r2[st.count] = v;
    a.st->count = st.count + 1;
    a.st->cur1 = p + 1;
    a.live[p] = 0;
  }
  __hip_atomic_store(&a.st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t launch_kcenter_prepare(const KcArgs& a, bool has_init, hipStream_t s) {
  if (a.n_total <= 0) return hipSuccess;
  const int n_pass = (a.n_total + 31) / 32;
  hipLaunchKernelGGL(kcenter_prepare_kernel, dim3((unsigned)std::min(n_pass, 4 * KC_MAX_GROUPS)), dim3(KC_LANES), 0, s, a, has_init ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_kcenter_step(const KcArgs& a, int groups, hipStream_t s) {
  if (a.n_total <= 0 || groups <= 0) return hipSuccess;
  hipLaunchKernelGGL(kcenter_step_kernel, dim3((unsigned)groups), dim3(KC_LANES), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

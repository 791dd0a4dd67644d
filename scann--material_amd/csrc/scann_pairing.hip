// One-to-one atom maps between a query structure and an index segment (scann_index_pairing, include/scann_hip.h): the linear assignment
// problem over the matrix of squared distances, solved exactly in integers, one workgroup per pair.
//
// pairing_kernel<QMAX>, QMAX = 32, 64 or 128 (the host sorts the pairs into these classes by Q = max(n, m)); 64, 128 or 256 lanes.
//   phase 1  every lane forms distance chains D[i][j] (the chain of scann_knn.hip over the padded stride, rows through tile_row) and
//            leaves their bits in the cost matrix C [Q][QMAX + 1] in LDS; the workgroup takes max D (exact) and whether any D is NaN
//            or +inf -- then the pair is not comparable and the tail is written.  Lane i < n walks its row: f_i = min_j D[i][j] to LDS,
//            every entry quantised in place, t = rint(ldexp((double) D, shift)), and the dummy columns filled with the row's least t;
//            lane j < m walks its column for the dummy rows.  Rounding is monotone, so the least t is t of the least D.
//   phase 2  the first wave runs the shortest-augmenting-path procedure of the definition.  Lane l owns columns l and l + 64: minv, v,
//            way, used and p in registers, and beside p the potential u of the row that p names, so that no potential lives in LDS.
//            A scan reads row i0 of C with consecutive lanes; (minv, j) goes into one 64-bit key, minv << 7 | j, whose minimum over
//            the wave (DPP steps inside a row of 16 lanes, then v_permlane16_swap and v_permlane32_swap: no LDS round trip in the
//            dependent chain) is delta and the least column that attains it.  Used and absent columns carry the all-ones key, above
//            every real one: minv < 2^39.  What the next scan needs of column j1 -- p, u -- comes by v_readlane.
//   write    total = sum of C[p[j]][j] (a wave sum of int64), shift, score; per query atom its partner's position and D[i][partner],
//            the chain formed once more (C holds t by then), or -1 and f_i for a surplus atom.
// Integer minima and sums only behind the distances: no output bit depends on the launch geometry.  No atomics, no scratch.
#include "scann_pairing.h"

namespace scann {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 pack64(uint32_t lo, uint32_t hi) { return (u64)hi << 32 | lo; }

struct MinU64 {
  __device__ __forceinline__ u64 operator()(u64 a, u64 b) const { return a < b ? a : b; }
};
struct AddU64 {
  __device__ __forceinline__ u64 operator()(u64 a, u64 b) const { return a + b; }
};

#define PAIRING_DPP_STEP(ctrl)                                                                   \
  {                                                                                              \
    const uint32_t plo = __builtin_amdgcn_update_dpp(0u, lo, (ctrl), 0xF, 0xF, true);            \
    const uint32_t phi = __builtin_amdgcn_update_dpp(0u, hi, (ctrl), 0xF, 0xF, true);            \
    const u64 r = op(pack64(lo, hi), pack64(plo, phi));                                          \
    lo = (uint32_t)r, hi = (uint32_t)(r >> 32);                                                  \
  }

// op over the 64 lanes of a wave, every lane getting the result (op commutes and associates): lane ^ 1, lane ^ 2, the 8-lane mirror
// and the 16-lane mirror as DPP operands -- after a step every group holds one value, so the mirror pairs it with the other group's --
// then the two lane swaps
template <class Op>
__device__ __forceinline__ u64 wave_reduce64(u64 v, Op op) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  PAIRING_DPP_STEP(0xB1)   // quad_perm:[1,0,3,2]
  PAIRING_DPP_STEP(0x4E)   // quad_perm:[2,3,0,1]
  PAIRING_DPP_STEP(0x141)  // row_half_mirror
  PAIRING_DPP_STEP(0x140)  // row_mirror
  {
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const u64 r = op(pack64(a[0], b[0]), pack64(a[1], b[1]));
    lo = (uint32_t)r, hi = (uint32_t)(r >> 32);
  }
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return op(pack64(a[0], b[0]), pack64(a[1], b[1]));
}
#undef PAIRING_DPP_STEP

// the value lane `lane` (wave-uniform) holds
__device__ __forceinline__ int lane_i32(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ long long lane_i64(long long v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((u64)v >> 32), lane);
  return (long long)pack64(lo, hi);
}

// the chain of the definition, columns ascending (the padding adds fmaf(0, 0, acc) = acc)
__device__ __forceinline__ float pairing_chain(const float* __restrict__ x, const float* __restrict__ y, int stride) {
  float acc = 0.f;
  for (int c = 0; c < stride; c += 4) {
    const float4 a = *reinterpret_cast<const float4*>(x + c), b = *reinterpret_cast<const float4*>(y + c);
    float d = a.x - b.x;
    acc = __builtin_fmaf(d, d, acc);
    d = a.y - b.y;
    acc = __builtin_fmaf(d, d, acc);
    d = a.z - b.z;
    acc = __builtin_fmaf(d, d, acc);
    d = a.w - b.w;
    acc = __builtin_fmaf(d, d, acc);
  }
  return acc;
}

template <int QMAX>
__global__ __launch_bounds__(QMAX <= 32 ? 64 : 2 * QMAX) void pairing_kernel(PairingArgs a, int base) {
  constexpr int NT = QMAX <= 32 ? 64 : 2 * QMAX, NW = NT / 64, LD = pairing_ld(QMAX), NC = QMAX > 64 ? 2 : 1;
  extern __shared__ uint32_t pairing_smem[];
  uint32_t* C = pairing_smem;                                   // [QMAX][LD] D's bits, then t, dummies included
  float* fs = reinterpret_cast<float*>(C + QMAX * LD);          // [QMAX] f_i
  float* wmax = fs + QMAX;                                      // [4] the waves' max D ...
  int32_t* wbad = reinterpret_cast<int32_t*>(wmax + 4);         // [4] ... and whether they saw a NaN or +inf
  const int t = threadIdx.x, lane = t & 63;
  const PairingDesc d = a.desc[base + blockIdx.x];
  const int n = d.n, m = d.m, Q = n > m ? n : m;
  if (n < 1 || m < 1 || Q > QMAX) return;  // (the host sorts no such pair into this class)
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const float inf = __builtin_inff();
  // ---- phase 1: the distances ----
  float mx = 0.f;
  bool bad = false;
  for (int e = t; e < n * m; e += NT) {
    const int i = e / m, j = e - i * m;
    const float acc = pairing_chain(a.q + (size_t)(d.q0 + i) * stride, tile_row(a.rows, d.first + j, chunk_rows, stride), stride);
    C[i * LD + j] = __float_as_uint(acc);
    bad |= !(acc < inf);  // NaN or +inf
    if (acc > mx) mx = acc;
  }
  // (non-negative floats order as their bits do: the max over the wave as the min of the complemented bits)
  const uint32_t wave_mx = ~(uint32_t)wave_reduce64((u64)(~__float_as_uint(mx)), MinU64());
  const bool wave_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
  if (lane == 0) wmax[t >> 6] = __uint_as_float(wave_mx), wbad[t >> 6] = wave_bad;
  __syncthreads();
  float dmax = wmax[0];
  int any_bad = wbad[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    if (wmax[w] > dmax) dmax = wmax[w];
    any_bad |= wbad[w];
  }
  if (any_bad) {  // not comparable (the same answer in every lane)
    if (t == 0) a.score[d.pair] = inf, a.total[d.pair] = -1, a.shift[d.pair] = 0;
    if (t < n) a.partner_pos[d.out0 + t] = -1, a.partner_d[d.out0 + t] = inf;
    return;
  }
  const int shift = pairing_shift(__float_as_uint(dmax));
  if (t < n) {  // row t: f, the quantisation in place, the dummy columns
    uint32_t* row = C + t * LD;
    float f = inf;
    uint32_t tmin = 0xffffffffu;
    for (int j = 0; j < m; ++j) {
      const float x = __uint_as_float(row[j]);
      if (x < f) f = x;
      const uint32_t q = pairing_quant(x, shift);
      row[j] = q;
      if (q < tmin) tmin = q;
    }
    fs[t] = f;
    for (int j = m; j < Q; ++j) row[j] = tmin;
  }
  __syncthreads();
  if (n < m && t < m) {  // column t: the dummy rows
    uint32_t tmin = 0xffffffffu;
    for (int i = 0; i < n; ++i) {
      const uint32_t q = C[i * LD + t];
      if (q < tmin) tmin = q;
    }
    for (int i = n; i < Q; ++i) C[i * LD + t] = tmin;
  }
  __syncthreads();
  if (t >= 64) return;  // ---- phase 2: one wave, C is read only from here on ----
  long long v[NC], ucol[NC], minv[NC];
  int p[NC], way[NC];
  bool used[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) v[c] = 0, ucol[c] = 0, p[c] = -1;
  for (int i = 0; i < Q; ++i) {
#pragma unroll
    for (int c = 0; c < NC; ++c) minv[c] = PAIRING_INF, used[c] = false, way[c] = -1;
    int j0 = -1, i0 = i;
    long long ui = 0, u0 = 0;
    for (;;) {
      const uint32_t* crow = C + i0 * LD;
      u64 key = ~0ull;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int j = lane + 64 * c;
        if (j < Q && !used[c]) {
          const long long cur = (long long)crow[j] - u0 - v[c];
          if (cur < minv[c]) minv[c] = cur, way[c] = j0;
          const u64 k = (u64)minv[c] << 7 | (u64)j;
          if (k < key) key = k;
        }
      }
      key = wave_reduce64(key, MinU64());
      const uint32_t klo = __builtin_amdgcn_readfirstlane((uint32_t)key), khi = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
      const long long delta = (long long)(pack64(klo, khi) >> 7);
      const int j1 = (int)(klo & 127u);
      ui += delta;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (used[c]) ucol[c] += delta, v[c] -= delta;
        else minv[c] -= delta;
      }
      j0 = j1;
      const int jl = j0 & 63, jc = j0 >> 6;
      const int pj = lane_i32(NC > 1 && jc ? p[NC - 1] : p[0], jl);
      if (pj < 0) break;
      if (lane == jl) {
        if (NC > 1 && jc) used[NC - 1] = true;
        else used[0] = true;
      }
      i0 = pj;
      u0 = lane_i64(NC > 1 && jc ? ucol[NC - 1] : ucol[0], jl);
    }
    for (int jw = j0; jw >= 0;) {  // the rows move one column along the path; row i enters at its end
      const int wl = jw & 63, wc = jw >> 6;
      const int jp = lane_i32(NC > 1 && wc ? way[NC - 1] : way[0], wl);
      int np = i;
      long long nu = ui;
      if (jp >= 0) {
        const int pl = jp & 63, pc = jp >> 6;
        np = lane_i32(NC > 1 && pc ? p[NC - 1] : p[0], pl);
        nu = lane_i64(NC > 1 && pc ? ucol[NC - 1] : ucol[0], pl);
      }
      if (lane == wl) {
        if (NC > 1 && wc) p[NC - 1] = np, ucol[NC - 1] = nu;
        else p[0] = np, ucol[0] = nu;
      }
      jw = jp;
    }
  }
  // ---- the answer ----
  u64 sum = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = lane + 64 * c;
    if (j < Q) sum += C[p[c] * LD + j];
  }
  const long long total = (long long)wave_reduce64(sum, AddU64());
  if (lane == 0) a.score[d.pair] = pairing_score(total, shift, Q), a.total[d.pair] = total, a.shift[d.pair] = shift;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = lane + 64 * c, i = j < Q ? p[c] : n;
    if (i >= n) continue;  // a dummy row
    const bool real = j < m;
    a.partner_pos[d.out0 + i] = real ? d.first + j : -1;
    a.partner_d[d.out0 + i] =
        real ? pairing_chain(a.q + (size_t)(d.q0 + i) * stride, tile_row(a.rows, d.first + j, chunk_rows, stride), stride) : fs[i];
  }
}

template <int QMAX>
hipError_t launch_class(const PairingArgs& a, int base, int count, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const size_t lds = pairing_lds_bytes(QMAX);
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pairing_kernel<QMAX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pairing_kernel<QMAX>, dim3((unsigned)count), dim3(QMAX <= 32 ? 64 : 2 * QMAX), lds, s, a, base);
  return hipGetLastError();
}

}  // namespace

size_t pairing_lds_bytes(int qmax) { return ((size_t)qmax * pairing_ld(qmax) + qmax + 8) * 4; }

hipError_t launch_pairing(const PairingArgs& a, const int32_t* count, hipStream_t s) {
  hipError_t e = launch_class<32>(a, 0, count[0], s);
  if (e == hipSuccess) e = launch_class<64>(a, count[0], count[1], s);
  if (e == hipSuccess) e = launch_class<128>(a, count[0] + count[1], count[2], s);
  return e;
}

}  // namespace scann

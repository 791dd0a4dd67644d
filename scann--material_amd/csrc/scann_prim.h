// The row primitives of the analyses over a latent-space index, once: the small definitions on which a kernel and its host twin must
// agree to the bit.  Every analysis takes them from here (scann_tile.h includes this file); none keeps a copy of its own.  The device
// forms work on fp32 bit patterns, the host forms on <cmath>; each pair implements the one definition its comment states.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace scann {

// ---- host twins ----

// a row is eligible iff all its d components are finite
inline bool finite_row(const float* x, int64_t d) {
  for (int64_t j = 0; j < d; ++j)
    if (!std::isfinite(x[j])) return false;
  return true;
}

// frexp's exponent of a column's largest absolute value m >= 0: m < 2^e; 0 for a column of zeros.  The scale of the integer sums
inline int frexp_exponent(float m) {
  int e = 0;
  if (m > 0.f) (void)std::frexp(m, &e);
  return e;
}

// a kernel width gamma must be finite and > 0
inline bool bad_gamma(float gamma) { return !std::isfinite(gamma) || !(gamma > 0.f); }

// ---- device ----

// x is finite: its exponent field is not all ones (finite_row's test, on the bits)
__device__ __forceinline__ bool f32_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// frexp_exponent of the float whose bits are b (b >= 0: an absolute value): b < 2^e; 0 for zero
__device__ __forceinline__ int f32_exponent(uint32_t b) {
  if (b == 0) return 0;
  const int ef = (int)(b >> 23);
  if (ef) return ef - 126;
  return (31 - __builtin_clz(b)) - 148;  // subnormal: b * 2^-149
}

// b of an integer sum over n rows (scann_pca_bits): |u| <= 2^b, b = min(24, (62 - L) / 2) for n < 2^L, so no partial sum of products reaches 2^62
__device__ __forceinline__ int sum_bits(uint32_t n) {
  const int L = n ? 32 - __builtin_clz(n) : 0;
  return min(24, (62 - L) / 2);
}

// where position pos lies in a table stored in chunks of chunk_rows rows, `stride` elements to a row.  I, int or uint32_t, is the type
// of the 32-bit division
template <class T, class I>
__device__ __forceinline__ const T* tile_row(const T* const* rows, I pos, I chunk_rows, int stride) {
  const I c = pos / chunk_rows;
  return rows[c] + (size_t)(pos - c * chunk_rows) * stride;
}

// (d, p) before (e, q) in the total order that breaks every tie: distance ascending, then position ascending
__device__ __forceinline__ bool dist_before(float d, int32_t p, float e, int32_t q) { return d < e || (d == e && p < q); }

// the `extra` of a scan in which nothing but a non-finite component makes a row bad
struct NoExtra {
  __device__ int operator()(int, int) const { return 0; }
};

// The eligibility scan of an index of n_total rows (rows == nullptr: there are none to read): 8 lanes per row, 32 rows per workgroup
// and pass; lane sub = threadIdx.x & 7 tests columns 4 sub .. + 3, + 32, ... of its row (the padding columns up to the stride are
// zero), and the row's verdict is the OR over its 8 lanes.  extra(p, sub) is what else makes row p bad, asked before the scan;
// verdict(p, bad) is what lane sub == 0 of the row does with the outcome.  cmax is eligible_scan_colmax's alone (LDS, one word per
// column: the maxima of the bits of |x| over the eligible rows); with it, rows must not be null: the rows are read again.
template <class Extra, class Verdict>
__device__ __forceinline__ void eligible_scan(const float* const* rows, int chunk_rows, int stride, int n_total, Extra extra, Verdict verdict,
                                              uint32_t* cmax = nullptr) {
  const int t = threadIdx.x, sub = t & 7;
  const int n_pass = (n_total + 31) / 32;
  for (int g = blockIdx.x; g < n_pass; g += gridDim.x) {
    const int p = g * 32 + (t >> 3);
    int bad = 0;
    const float* row = nullptr;
    if (p < n_total) {
      bad = extra(p, sub);
      if (rows) {
        row = tile_row(rows, p, chunk_rows, stride);
        for (int c = 4 * sub; c < stride; c += 32) {
          const float4 v = *reinterpret_cast<const float4*>(row + c);
          bad |= !(f32_finite(v.x) && f32_finite(v.y) && f32_finite(v.z) && f32_finite(v.w));
        }
      }
    }
    bad |= __shfl_xor(bad, 1);
    bad |= __shfl_xor(bad, 2);
    bad |= __shfl_xor(bad, 4);
    if (p >= n_total) continue;
    if (sub == 0) verdict(p, bad);
    if (!cmax || bad) continue;
    for (int c = 4 * sub; c < stride; c += 32) {  // (the row is in the cache)
      const float4 v = *reinterpret_cast<const float4*>(row + c);
      atomicMax(&cmax[c], __float_as_uint(v.x) & 0x7fffffffu);
      atomicMax(&cmax[c + 1], __float_as_uint(v.y) & 0x7fffffffu);
      atomicMax(&cmax[c + 2], __float_as_uint(v.z) & 0x7fffffffu);
      atomicMax(&cmax[c + 3], __float_as_uint(v.w) & 0x7fffffffu);
    }
  }
}

// The scan with the column maxima of |x| over the eligible rows, by integer max on the bit patterns (order-free): first in LDS, then
// one global atomic per column and workgroup of LANES lanes into colmax (stride <= 1024 words, zero before the launch).  Every lane of
// the workgroup calls it; a barrier lies behind the clearing and one before the flush.
template <int LANES, class Extra, class Verdict>
__device__ __forceinline__ void eligible_scan_colmax(const float* const* rows, int chunk_rows, int stride, int n_total, uint32_t* colmax, Extra extra,
                                                     Verdict verdict) {
  __shared__ uint32_t cmax[1024];
  for (int j = threadIdx.x; j < stride; j += LANES) cmax[j] = 0;
  __syncthreads();
  eligible_scan(rows, chunk_rows, stride, n_total, extra, verdict, cmax);
  __syncthreads();
  for (int j = threadIdx.x; j < stride; j += LANES)
    if (cmax[j]) atomicMax(&colmax[j], cmax[j]);
}

}  // namespace scann

// Internal declarations of the one-to-one pairing of a query structure's atoms with a segment's rows (scann_pairing.hip, host side and
// twins in scann_pairing.cpp); the C ABI and the definition are in include/scann_hip.h (scann_index_pairing).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_knn.h"

namespace scann {

constexpr int PAIRING_MAX = 128;                     // atoms a side at most (SCANN_PAIRING_MAX_ATOMS): lane l of the solving wave owns columns l, l + 64
constexpr long long PAIRING_INF = 1ll << 62;         // minv of a column no row has reached yet (never packed into a key: the first scan lowers it)
constexpr int PAIRING_CLASSES = 3;                   // LDS size classes of a launch: Q <= 32, <= 64, <= 128
constexpr int pairing_class_q(int c) { return 32 << c; }
constexpr int pairing_ld(int qmax) { return qmax + 1; }  // uint32 between two rows of the cost matrix: a lane per row walks its row without bank conflicts

// ---- the fixed point of the definition, one expression for the kernel and the twin ----

// the true exponent of a positive finite float from its bits (ilogbf, subnormals included), in integer arithmetic
__host__ __device__ inline int pairing_ilogb(uint32_t bits) {
  const int e = (int)(bits >> 23) & 0xff;
  if (e) return e - 127;
  return 31 - __builtin_clz(bits & 0x7fffffu) - 149;
}
__host__ __device__ inline int pairing_shift(uint32_t dmax_bits) { return (dmax_bits & 0x7fffffffu) ? 30 - pairing_ilogb(dmax_bits) : 0; }
// t = llrint(ldexp((double) d, shift)): the scaling is exact in fp64, then one rounding to nearest even; 0 <= t <= 2^31
__host__ __device__ inline uint32_t pairing_quant(float d, int shift) { return (uint32_t)__builtin_rint(__builtin_ldexp((double)d, shift)); }
// score = (float)(ldexp((double) total, -shift) / (double) Q), the division in fp64 and rounded once
__host__ __device__ inline float pairing_score(long long total, int shift, int Q) {
  return (float)(__builtin_ldexp((double)total, -shift) / (double)Q);
}

// One pair of a launch: query rows [q0, q0 + n) against index positions [first, first + m), 1 <= n, m <= the class's Q.  The kernel writes
// score / total / shift at [pair] and the n partners at [out0 ..).
struct PairingDesc {
  int32_t q0, n, first, m, out0, pair;
};

// pairing_kernel<QMAX>: one workgroup per pair, the pairs of a launch sorted by class on the host (desc in launch order)
struct PairingArgs {
  const float* const* rows;  // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  int32_t chunk_rows, stride;
  const float* q;            // [n query rows][stride], padded like the rows
  const PairingDesc* desc;
  float* score;              // [n_pairs]
  long long* total;          // [n_pairs]
  int32_t* shift;            // [n_pairs]
  int32_t* partner_pos;      // [sum n] position in the index, -1: surplus
  float* partner_d;          // [sum n]
};
size_t pairing_lds_bytes(int qmax);
// count[c]: pairs of class c; they lie behind one another in a.desc
hipError_t launch_pairing(const PairingArgs& a, const int32_t* count, hipStream_t s);

}  // namespace scann

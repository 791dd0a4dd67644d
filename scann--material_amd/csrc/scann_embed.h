// Internal declarations of the neighbour embedding of a latent-space index (scann_embed.hip; the host half and the twin are in
// scann_embed.cpp); the C ABI is include/scann_hip.h: scann_embed_iterate, scann_embed_iterate_host.  The bodies below are the one place
// that defines a pair, a gradient and an update: the host twin and the kernels include them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace scann {

constexpr int EMBED_LANES = 256;  // lanes of every kernel here: one per row
constexpr int EMBED_BLOCK = 128;  // positions of a block: the innermost level of the summation tree of the definition
constexpr int EMBED_SPAN = 32;    // blocks of a span, the middle level
constexpr int EMBED_SPAN_ROWS = EMBED_BLOCK * EMBED_SPAN;
constexpr int EMBED_MAX_SPANS = 64;  // SCANN_EMBED_MAX_ROWS / EMBED_SPAN_ROWS

// The chains below are written once for a scalar lane (float: the kernels, and the twin's rows beside the diagonal) and for eight rows at
// a time (embed_v8: the twin's other rows); element by element the operations are the same IEEE ones.
// They are always inlined: the twin instantiates them inside functions built for different x86 feature sets, which must not share one
// out-of-line copy (-Wpsabi speaks of exactly that copy).
typedef float embed_v8 __attribute__((ext_vector_type(8)));
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpsabi"
#define EMBED_INLINE __host__ __device__ __attribute__((always_inline)) inline
EMBED_INLINE float embed_fma(float a, float b, float c) { return fmaf(a, b, c); }
EMBED_INLINE embed_v8 embed_fma(embed_v8 a, embed_v8 b, embed_v8 c) { return __builtin_elementwise_fma(a, b, c); }

// The pair (i, j) of the definition: every operation fp32 and rounded once, the division IEEE correctly rounded.
template <class T>
EMBED_INLINE void embed_pair(T xi, T yi, float xj, float yj, T& dx, T& dy, T& w) {
#pragma clang fp contract(off)
  dx = xi - xj;
  dy = yi - yj;
  const T d = embed_fma(dy, dy, dx * dx);
  w = 1.0f / (1.0f + d);
}

// one step of row i's repulsion chains within a block
template <class T>
EMBED_INLINE void embed_repel(T xi, T yi, float xj, float yj, T& z, T& rx, T& ry) {
#pragma clang fp contract(off)
  T dx, dy, w;
  embed_pair(xi, yi, xj, yj, dx, dy, w);
  z = z + w;
  const T ww = w * w;
  rx = embed_fma(ww, dx, rx);
  ry = embed_fma(ww, dy, ry);
}

// one step of row i's attraction chains
EMBED_INLINE void embed_attract(float xi, float yi, float xj, float yj, float p, float& ax, float& ay) {
#pragma clang fp contract(off)
  float dx, dy, w;
  embed_pair(xi, yi, xj, yj, dx, dy, w);
  const float q = p * w;
  ax = fmaf(q, dx, ax);
  ay = fmaf(q, dy, ay);
}

// one coordinate's gradient: fp64, each operation rounded once
EMBED_INLINE float embed_gradient(float exaggeration, float a, double R, double Z) {
#pragma clang fp contract(off)
  const double att = (double)exaggeration * (double)a;
  const double rep = R / Z;
  return (float)(4.0 * (att - rep));
}

// one coordinate's update; returns y'
EMBED_INLINE float embed_update(float g, float lr, float momentum, float y, float& u, float& gain) {
#pragma clang fp contract(off)
  float gn = ((g > 0.f) == (u > 0.f)) ? gain * 0.8f : gain + 0.2f;
  gn = fmaxf(gn, 0.01f);
  const float t = (lr * gn) * g;
  u = fmaf(momentum, u, -t);
  gain = gn;
  return y + u;
}

#pragma clang diagnostic pop

// One call's device arrays.  y0 / y1 are the two position buffers: an iteration reads `cur` and leaves its result in the other one.
struct TsneArgs {
  int32_t N, n_span;
  const int64_t* row_first;  // [N + 1]
  const int32_t* col;        // [E]
  const float* p;            // [E]
  float2* y[2];              // [N] each
  float2* u;                 // [N]
  float2* gain;              // [N]
  float2* grad;              // [N]
  double* part;              // [n_span][3][N]: z, rx, ry of (span, row)
  double* rsum;              // [3][N]: Z_i, Rx_i, Ry_i
  double* bsum;              // [3][n_block]: the block sums of Z_i (kernel rowsum), then of y'x, y'y in places 1, 2 (kernel update)
  double* z_out;             // [1]
  float exaggeration, momentum, lr;
};
// the four launches of one iteration, reading y[cur] and leaving the centred result in y[cur ^ 1]
hipError_t launch_embed_iteration(const TsneArgs& a, int cur, hipStream_t s);

}  // namespace scann

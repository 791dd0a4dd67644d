// Principal-component map of a latent-space index, the host side that needs no GPU (include/scann_hip.h): the twins of the moments and of
// the projection (scann_moments_host, scann_project_host: the kernels' bits, scann_pca.hip) and the symmetric eigen-decomposition
// (scann_sym_eig_host: cyclic Jacobi in fp64, the one function both the product and the tests call).  Every floating-point expression
// here is evaluated as written, each operation rounded to nearest: the file is compiled with floating-point contraction off.  The calls
// that touch an index or run a forward are in scann_knn.cpp, beside the index.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/scann_hip.h"

namespace {

// frexp's exponent of a column's largest absolute value (0 for a column of zeros)
int top_exponent(float m) {
  int e = 0;
  if (m > 0.f) (void)std::frexp(m, &e);
  return e;
}

// T[i][j] += sum over the rows of u[p][i] * u[p][j] for i = first, first + step, ... and j >= i: integer sums, so any split over threads gives the same
void scatter_rows(const int32_t* u, int64_t n, int64_t dim, int64_t first, int64_t step, int64_t* T) {
  for (int64_t p = 0; p < n; ++p) {
    const int32_t* row = u + p * dim;
    for (int64_t i = first; i < dim; i += step) {
      const int64_t ui = row[i];
      if (!ui) continue;
      int64_t* t = T + i * dim;
      for (int64_t j = i; j < dim; ++j) t[j] += ui * (int64_t)row[j];
    }
  }
}

// the projection of n rows; FMA: the host has a fused multiply-add instruction, fmaf is then one instruction instead of a libm call (it
// is correctly rounded either way, so the bits are the same)
template <bool FMA>
inline void project_loop(const float* rows, int64_t n, int64_t dim, const float* mean, const float* components, const float* scale, int32_t m,
                         float* coords, float* md2) {
  std::vector<float> y((size_t)dim);
  for (int64_t p = 0; p < n; ++p) {
    for (int64_t j = 0; j < dim; ++j) y[(size_t)j] = rows[p * dim + j] - mean[j];
    for (int32_t c = 0; c < m; ++c) {
      const float* w = components + (int64_t)c * dim;
      float acc = 0.f;
      for (int64_t j = 0; j < dim; ++j) acc = FMA ? __builtin_fmaf(y[(size_t)j], w[j], acc) : std::fmaf(y[(size_t)j], w[j], acc);
      coords[p * m + c] = acc;
    }
    if (!md2) continue;
    float acc = 0.f;
    for (int32_t c = 0; c < m; ++c) {
      const float t = coords[p * m + c] * scale[c];
      acc = FMA ? __builtin_fmaf(t, t, acc) : std::fmaf(t, t, acc);
    }
    md2[p] = acc;
  }
}
void project_plain(const float* rows, int64_t n, int64_t dim, const float* mean, const float* components, const float* scale, int32_t m,
                   float* coords, float* md2) {
  project_loop<false>(rows, n, dim, mean, components, scale, m, coords, md2);
}
__attribute__((target("fma"))) void project_fma(const float* rows, int64_t n, int64_t dim, const float* mean, const float* components,
                                                const float* scale, int32_t m, float* coords, float* md2) {
  project_loop<true>(rows, n, dim, mean, components, scale, m, coords, md2);
}

}  // namespace

extern "C" {

int scann_pca_bits(int64_t n) {
  if (n < 0 || n > (int64_t)0x7fffffff) return SCANN_ERR_INVALID;
  int L = 0;
  while (L < 32 && ((int64_t)1 << L) <= n) ++L;  // n < 2^L
  return std::min(24, (62 - L) / 2);
}

int scann_moments_host(const float* rows, int64_t n, int64_t dim, int64_t* n_eligible, float* mean, double* cov, int32_t* col_exp, int32_t* bits) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || !n_eligible || !mean || !cov || (n > 0 && !rows)) return SCANN_ERR_INVALID;
  std::vector<int64_t> live;
  std::vector<float> mx((size_t)dim, 0.f);
  for (int64_t p = 0; p < n; ++p) {
    bool ok = true;
    for (int64_t j = 0; j < dim; ++j) ok = ok && std::isfinite(rows[p * dim + j]);
    if (!ok) continue;
    live.push_back(p);
    for (int64_t j = 0; j < dim; ++j) mx[(size_t)j] = std::max(mx[(size_t)j], std::fabs(rows[p * dim + j]));
  }
  const int64_t ne = (int64_t)live.size();
  *n_eligible = ne;
  if (ne < 2) return SCANN_ERR_INVALID;
  const int b = scann_pca_bits(ne);
  if (bits) *bits = b;
  std::vector<int64_t> S((size_t)dim, 0);
  for (int64_t j = 0; j < dim; ++j) {
    const int e = top_exponent(mx[(size_t)j]);
    for (int64_t p : live) S[(size_t)j] += std::llrint(std::ldexp((double)rows[p * dim + j], 30 - e));
    mean[j] = (float)std::ldexp((double)S[(size_t)j] / (double)ne, e - 30);
  }
  std::vector<int> f((size_t)dim, 0);
  for (int64_t j = 0; j < dim; ++j) {
    float m = 0.f;
    for (int64_t p : live) m = std::max(m, std::fabs(rows[p * dim + j] - mean[j]));
    f[(size_t)j] = top_exponent(m);
    if (col_exp) col_exp[j] = f[(size_t)j];
  }
  std::vector<int32_t> u((size_t)ne * dim);
  std::vector<int64_t> R((size_t)dim, 0), T((size_t)dim * dim, 0);
  for (int64_t i = 0; i < ne; ++i)
    for (int64_t j = 0; j < dim; ++j) {
      const float y = rows[live[(size_t)i] * dim + j] - mean[j];
      const int64_t q = std::llrint(std::ldexp((double)y, b - f[(size_t)j]));
      u[(size_t)(i * dim + j)] = (int32_t)q;
      R[(size_t)j] += q;
    }
  const double work = (double)ne * (double)dim * (double)dim;
  const int64_t nt = work < 2e8 ? 1 : std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(), dim}));
  if (nt == 1) {
    scatter_rows(u.data(), ne, dim, 0, 1, T.data());
  } else {  // thread k: the rows k, k + nt, ... of T (their lengths fall evenly)
    std::vector<std::thread> pool;
    for (int64_t k = 0; k < nt; ++k) pool.emplace_back(scatter_rows, u.data(), ne, dim, k, nt, T.data());
    for (auto& th : pool) th.join();
  }
  for (int64_t i = 0; i < dim; ++i)
    for (int64_t j = i; j < dim; ++j) {
      const double prod = (double)R[(size_t)i] * (double)R[(size_t)j];
      const double corr = prod / (double)ne;
      const double diff = (double)T[(size_t)(i * dim + j)] - corr;
      const double c = std::ldexp(diff / (double)(ne - 1), f[(size_t)i] + f[(size_t)j] - 2 * b);
      cov[i * dim + j] = c;
      cov[j * dim + i] = c;
    }
  return SCANN_OK;
}

int scann_project_host(const float* rows, int64_t n, int64_t dim, const float* mean, const float* components, const float* scale, int32_t m,
                       float* coords, float* md2, float* dist2) {
  if (n < 0 || dim < 1 || m < 1 || m > dim || !mean || !components || !coords || (md2 && !scale) || (n > 0 && !rows)) return SCANN_ERR_INVALID;
  if (__builtin_cpu_supports("fma")) project_fma(rows, n, dim, mean, components, scale, m, coords, md2);
  else project_plain(rows, n, dim, mean, components, scale, m, coords, md2);
  for (int64_t p = 0; dist2 && p < n; ++p) dist2[p] = scann_knn_distsq(rows + p * dim, mean, dim);
  return SCANN_OK;
}

int scann_sym_eig_host(const double* a, int64_t d, double* w, double* v, int32_t* sweeps) {
  if (!a || !w || !v || d < 1 || d > 4096) return SCANN_ERR_INVALID;
  for (int64_t i = 0; i < d * d; ++i)
    if (!std::isfinite(a[i])) return SCANN_ERR_INVALID;
  // A: the upper triangle of `a`, mirrored; Vt: row c is the vector that belongs to column c of A
  std::vector<double> A((size_t)(d * d)), Vt((size_t)(d * d), 0.0);
  for (int64_t i = 0; i < d; ++i) {
    for (int64_t j = i; j < d; ++j) A[(size_t)(i * d + j)] = A[(size_t)(j * d + i)] = a[i * d + j];
    Vt[(size_t)(i * d + i)] = 1.0;
  }
  int32_t n_sweep = 0;
  bool rotated = true;
  while (rotated && n_sweep < 64) {
    rotated = false;
    ++n_sweep;
    for (int64_t p = 0; p < d - 1; ++p)
      for (int64_t q = p + 1; q < d; ++q) {
        const double apq = A[(size_t)(p * d + q)];
        if (apq == 0.0) continue;
        const double app = A[(size_t)(p * d + p)], aqq = A[(size_t)(q * d + q)];
        // below half an ulp of both diagonal entries: dropped, not rotated.  (Between two equal eigenvalues theta is rounding noise;
        // rotating such entries shrinks them only linearly, and no sweep would ever find them all exactly 0.)
        if (std::fabs(app) + std::fabs(apq) == std::fabs(app) && std::fabs(aqq) + std::fabs(apq) == std::fabs(aqq)) {
          A[(size_t)(p * d + q)] = A[(size_t)(q * d + p)] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double th2 = theta * theta;
        double t;
        if (std::isinf(th2)) t = 1.0 / (2.0 * theta);
        else t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(th2 + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        double* ap = &A[(size_t)(p * d)];
        double* aq = &A[(size_t)(q * d)];
        for (int64_t r = 0; r < d; ++r) {  // (rows p and q hold columns p and q: A is symmetric)
          const double arp = ap[r], arq = aq[r];
          ap[r] = c * arp - s * arq;
          aq[r] = s * arp + c * arq;
        }
        ap[p] = app - t * apq;
        aq[q] = aqq + t * apq;
        ap[q] = aq[p] = 0.0;
        for (int64_t r = 0; r < d; ++r) {
          A[(size_t)(r * d + p)] = ap[r];
          A[(size_t)(r * d + q)] = aq[r];
        }
        double* vp = &Vt[(size_t)(p * d)];
        double* vq = &Vt[(size_t)(q * d)];
        for (int64_t r = 0; r < d; ++r) {
          const double x = vp[r], y = vq[r];
          vp[r] = c * x - s * y;
          vq[r] = s * x + c * y;
        }
      }
  }
  if (sweeps) *sweeps = n_sweep;
  if (rotated) return SCANN_ERR_UNSUPPORTED;  // 64 sweeps, and the last still rotated
  std::vector<int64_t> order((size_t)d);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return A[(size_t)(x * d + x)] > A[(size_t)(y * d + y)]; });
  for (int64_t k = 0; k < d; ++k) {
    const int64_t c = order[(size_t)k];
    w[k] = A[(size_t)(c * d + c)];
    const double* src = &Vt[(size_t)(c * d)];
    int64_t top = 0;
    for (int64_t j = 1; j < d; ++j)
      if (std::fabs(src[j]) > std::fabs(src[top])) top = j;
    const bool flip = src[top] < 0.0;
    for (int64_t j = 0; j < d; ++j) v[k * d + j] = flip ? -src[j] : src[j];
  }
  return SCANN_OK;
}

}  // extern "C"

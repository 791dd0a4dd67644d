// Principal-component map of a latent-space index, the host side that needs no GPU (include/scann_hip.h): the twins of the moments and of
// the projection (scann_moments_host, scann_project_host: the kernels' bits, scann_pca.hip) and the symmetric eigen-decomposition
// (scann_sym_eig_host: cyclic Jacobi in fp64, the one function both the product and the tests call).  Every floating-point expression
// here is evaluated as written, each operation rounded to nearest: the file is compiled with floating-point contraction off.  The calls
// that touch an index or run a forward (scann_index_moments, scann_index_project, scann_project_batch around the kernels of scann_pca.hip)
// are at the end of the file; the forward of scann_project_batch is forward_and_download (scann_batch.cpp), as for the index's own batch calls.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/scann_hip.h"
#include "scann_call.h"
#include "scann_pca.h"
#include "scann_runtime.h"

namespace {

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
    if (!scann::finite_row(rows + p * dim, dim)) continue;
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
    const int e = scann::frexp_exponent(mx[(size_t)j]);
    for (int64_t p : live) S[(size_t)j] += std::llrint(std::ldexp((double)rows[p * dim + j], 30 - e));
    mean[j] = (float)std::ldexp((double)S[(size_t)j] / (double)ne, e - 30);
  }
  std::vector<int> f((size_t)dim, 0);
  for (int64_t j = 0; j < dim; ++j) {
    float m = 0.f;
    for (int64_t p : live) m = std::max(m, std::fabs(rows[p * dim + j] - mean[j]));
    f[(size_t)j] = scann::frexp_exponent(m);
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

// ---- the calls that touch an index or run a forward (scann_pca.hip) ----

extern "C" {

int scann_index_moments(scann_handle_t* h, scann_index_t* pool, int64_t* n_eligible, float* mean, double* cov, int32_t* col_exp, int32_t* bits) {
  if (const int r = check_pool(h, pool, "scann_index_moments")) return r;
  if (!n_eligible) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: n_eligible is null");
  if (!mean) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: mean is null");
  if (!cov) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: cov is null");
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride;
  if (const int r = check_pool_rows(h, pool, "scann_index_moments", (int64_t)0x7fffffff - 1024)) return r;
  if (N == 0) {
    *n_eligible = 0;
    return fail(h, SCANN_ERR_INVALID, "scann_index_moments: a covariance needs at least 2 rows, the pool has 0");
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  PcaArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride; a.dim = dim;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  // one workspace for the call.  First what the memset clears: the state, the two column maxima, S, R and T; then the mean, the
  // covariance, f, the chunk table and the eligibility bytes
  CallWs ws;
  ws.take(a.st, 1); ws.take(a.colmax, (size_t)stride); ws.take(a.cenmax, (size_t)stride); ws.take(a.sums, (size_t)stride); ws.take(a.R, (size_t)stride);
  ws.take(a.T, (size_t)stride * stride);
  const size_t zeroed = ws.bytes();
  ws.take(a.mean, (size_t)stride); ws.take(a.col_exp, (size_t)stride); ws.take(a.cov, (size_t)dim * dim); ws.take(a.rows, (size_t)a.n_chunk);
  ws.take(a.elig, (size_t)N);
  HIPCHK(h, ws.alloc());
  PcaState st{};
  std::vector<float> mean_h((size_t)dim);
  std::vector<double> cov_h((size_t)dim * dim);
  std::vector<int32_t> exp_h((size_t)dim);
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, a.n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess) e = launch_pca_moments(a, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(PcaState), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(mean_h.data(), a.mean, (size_t)dim * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(cov_h.data(), a.cov, (size_t)dim * dim * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(exp_h.data(), a.col_exp, (size_t)dim * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  *n_eligible = st.n;
  if (st.n < 2)
    return fail(h, SCANN_ERR_INVALID, "scann_index_moments: a covariance needs at least 2 rows without a non-finite component, the pool has " +
                                          std::to_string(st.n) + " among its " + std::to_string(N));
  std::copy(mean_h.begin(), mean_h.end(), mean);
  std::copy(cov_h.begin(), cov_h.end(), cov);
  if (col_exp) std::copy(exp_h.begin(), exp_h.end(), col_exp);
  if (bits) *bits = scann_pca_bits(st.n);
  return SCANN_OK;
}

}  // extern "C"

namespace {

// the arguments of a projection onto rows of `dim` columns
int check_projection(scann_handle* h, const char* who, int64_t dim, const float* mean, const float* components, const float* scale, int32_t m,
                     const float* coords, const float* md2) {
  const std::string w(who);
  if (m < 1 || m > dim) return fail(h, SCANN_ERR_INVALID, w + ": m " + std::to_string(m) + " outside 1 .. " + std::to_string(dim));
  if (!mean) return fail(h, SCANN_ERR_INVALID, w + ": mean is null");
  if (!components) return fail(h, SCANN_ERR_INVALID, w + ": components is null");
  if (!coords) return fail(h, SCANN_ERR_INVALID, w + ": coords is null");
  if (md2 && !scale) return fail(h, SCANN_ERR_INVALID, w + ": md2 needs scale, which is null");
  for (int64_t j = 0; j < dim; ++j)
    if (!std::isfinite(mean[j])) return fail(h, SCANN_ERR_INVALID, w + ": mean holds a non-finite value (column " + std::to_string(j) + ")");
  for (int64_t i = 0; i < (int64_t)m * dim; ++i)
    if (!std::isfinite(components[i]))
      return fail(h, SCANN_ERR_INVALID, w + ": components hold a non-finite value (component " + std::to_string(i / dim) + ", column " +
                                            std::to_string(i % dim) + ")");
  for (int32_t c = 0; scale && c < m; ++c)
    if (!std::isfinite(scale[c])) return fail(h, SCANN_ERR_INVALID, w + ": scale holds a non-finite value (component " + std::to_string(c) + ")");
  return SCANN_OK;
}

// rows [first, first + n) of the chunks in `tab` ([chunk_rows][stride] each, the padding zero) projected; the outputs are host arrays.
// The coordinates pass through a device block of at most 256 MiB, a group of rows at a time
int project_rows(scann_handle* h, const std::vector<const void*>& tab, int32_t chunk_rows, int32_t stride, int32_t dim, int64_t first, int64_t n,
                 const float* mean, const float* components, const float* scale, int32_t m, float* coords, float* md2, float* dist2, hipStream_t s) {
  if (n <= 0) return SCANN_OK;
  const int64_t g = std::min<int64_t>(n, std::max<int64_t>(PCA_TP, (((int64_t)256 << 20) / ((int64_t)m * 4)) / PCA_TP * PCA_TP));
  PcaProjArgs a{};
  a.chunk_rows = chunk_rows; a.stride = stride; a.dim = dim; a.m = m;
  CallWs ws;
  ws.take(a.mean, (size_t)stride); ws.take(a.comp, (size_t)m * stride); ws.take(a.scale, (size_t)m);
  const size_t zeroed = ws.bytes();  // (the padding columns of the mean and of the components are zero)
  ws.take(a.rows, tab.size()); ws.take(a.coords, (size_t)g * m); ws.take(a.md2, (size_t)g); ws.take(a.dist2, (size_t)g);
  HIPCHK(h, ws.alloc());
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.mean), mean, (size_t)dim * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(writable(a.comp), (size_t)stride * 4, components, (size_t)dim * 4, (size_t)dim * 4, (size_t)m, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && scale) e = hipMemcpyAsync(writable(a.scale), scale, (size_t)m * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.rows), tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s);
  if (!md2) a.md2 = nullptr;  // (the kernel writes what it is given)
  if (!dist2) a.dist2 = nullptr;
  for (int64_t r0 = 0; r0 < n && e == hipSuccess; r0 += g) {
    const int64_t cnt = std::min<int64_t>(g, n - r0);
    a.first = (int32_t)(first + r0); a.n = (int32_t)cnt;
    e = launch_pca_project(a, s);  // (the stream orders a group behind the copies of the one before)
    if (e == hipSuccess) e = hipMemcpyAsync(coords + (size_t)r0 * m, a.coords, (size_t)cnt * m * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && md2) e = hipMemcpyAsync(md2 + r0, a.md2, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && dist2) e = hipMemcpyAsync(dist2 + r0, a.dist2, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
  }
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  return SCANN_OK;
}

}  // namespace

extern "C" {

int scann_index_project(scann_handle_t* h, scann_index_t* pool, int64_t first, int64_t n, const float* mean, const float* components,
                        const float* scale, int32_t m, float* coords, float* md2, float* dist2) {
  if (const int r = check_pool(h, pool, "scann_index_project")) return r;
  if (first < 0 || n < 0 || first + n > pool->n)
    return fail(h, SCANN_ERR_INVALID, "scann_index_project: rows " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " + std::to_string(pool->n));
  if (const int r = check_projection(h, "scann_index_project", pool->dim, mean, components, scale, m, coords, md2)) return r;
  if (n == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<const void*> tab(pool->chunks.size());
  for (size_t c = 0; c < tab.size(); ++c) tab[c] = pool->rows_of(c);
  return project_rows(h, tab, pool->chunk_rows, pool->stride, pool->dim, first, n, mean, components, scale, m, coords, md2, dist2, h->streams[0]);
}

int scann_project_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* components, const float* scale,
                        int32_t m, float* y, float* ga, float* coords, float* md2, float* dist2) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_project_batch: null handle or batch");
  const int dim = level_dim(h, level);
  if (!dim) return bad_level(h, level, "scann_project_batch");
  if (const int r = check_projection(h, "scann_project_batch", dim, mean, components, scale, m, coords, md2)) return r;
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_project_batch: weights not loaded");
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int64_t nq = atom ? db->n_atom : db->n_struct;
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  if (nq <= 0) return SCANN_OK;
  hipStream_t s = h->streams[db->last_slot];
  const float* src = atom ? db->out_z : db->out_bf;  // the level's rows where the forward left them
  const int stride = (dim + 3) / 4 * 4;
  CallWs ws;  // rows of the padded width, as an index keeps them
  RowStage st;
  st.take(ws, nq, dim, dim, stride, hipMemcpyDeviceToDevice);
  HIPCHK(h, ws.alloc());
  const hipError_t e = st.stage_rows(src, s);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    ws.release();
    HIPCHK(h, e);
  }
  const std::vector<const void*> tab(1, st.rows(src));
  const int r = project_rows(h, tab, 0x7fffffff, stride, dim, 0, nq, mean, components, scale, m, coords, md2, dist2, s);
  ws.release();
  return r;
}

}  // extern "C"

// Readout head on a latent-space index, the host half (include/scann_hip.h): scann_index_fit_moments, scann_index_ridge_loo and
// scann_head_batch around the kernels of scann_head.hip, and the twin of the leave-one-out pass (scann_ridge_loo_host: the kernels' bits,
// threaded over the 128-row blocks of the definition).  Every floating-point expression here is evaluated as written, each operation
// rounded to nearest: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <cmath>
#include <thread>

#include "scann_call.h"
#include "scann_head.h"
#include "scann_knn.h"
#include "scann_runtime.h"

using namespace scann;

namespace {

// the sums of block g (positions 128 g .. 128 g + 127) -> part [3 L K + L + 1]; resid rows of the block
template <bool FMA>
inline void loo_block(const float* rows, int64_t n, int64_t dim, const float* t, int32_t K, const float* mean, const float* tmean, const float* V,
                      int32_t m, const float* S, const float* B, int32_t L, float lev0, const int32_t* resid_l, float* resid, int64_t g, double* part) {
  const int64_t LK = (int64_t)L * K, Q = 3 * LK + L + 1;
  for (int64_t q = 0; q < Q; ++q) part[q] = 0.0;
  std::vector<float> y((size_t)dim), z((size_t)m), lev((size_t)L);
  const float nan = std::nanf("");
  for (int64_t p = g * HEAD_TILE; p < std::min<int64_t>(n, (g + 1) * HEAD_TILE); ++p) {
    const bool ok = finite_row(rows + p * dim, dim) && finite_row(t + p * K, K);
    if (resid)
      for (int32_t k = 0; k < K; ++k) resid[p * K + k] = nan;
    if (!ok) continue;
    part[3 * LK + L] += 1.0;
    for (int64_t j = 0; j < dim; ++j) y[(size_t)j] = rows[p * dim + j] - mean[j];
    for (int32_t c = 0; c < m; ++c) {
      const float* w = V + (int64_t)c * dim;
      float acc = 0.f;
      for (int64_t j = 0; j < dim; ++j) acc = FMA ? __builtin_fmaf(y[(size_t)j], w[j], acc) : std::fmaf(y[(size_t)j], w[j], acc);
      z[(size_t)c] = acc;
    }
    for (int32_t l = 0; l < L; ++l) {
      float acc = 0.f;
      for (int32_t c = 0; c < m; ++c) {
        const float tc = z[(size_t)c] * S[(int64_t)l * m + c];
        acc = FMA ? __builtin_fmaf(tc, tc, acc) : std::fmaf(tc, tc, acc);
      }
      lev[(size_t)l] = lev0 + acc;
      part[3 * LK + l] += (double)lev[(size_t)l];
    }
    for (int32_t l = 0; l < L; ++l)
      for (int32_t k = 0; k < K; ++k) {
        const float* b = B + ((int64_t)l * K + k) * m;
        float acc = 0.f;
        for (int32_t c = 0; c < m; ++c) acc = FMA ? __builtin_fmaf(z[(size_t)c], b[c], acc) : std::fmaf(z[(size_t)c], b[c], acc);
        const float d = t[p * K + k] - tmean[k];
        const float e = d - acc;
        const float le = lev[(size_t)l];
        const float r = le < 1.f ? (float)((double)e / (1.0 - (double)le)) : INFINITY;
        const double rd = (double)r, ed = (double)e;
        part[l * K + k] += rd * rd;
        part[LK + l * K + k] += std::fabs(rd);
        part[2 * LK + l * K + k] += ed * ed;
        if (resid && resid_l[k] == l) resid[p * K + k] = r;
      }
  }
}

struct LooCall {
  const float *rows, *t, *mean, *tmean, *V, *S, *B;
  int64_t n, dim;
  int32_t K, m, L;
  float lev0;
  const int32_t* resid_l;
  float* resid;
  double* part;
  int64_t n_block, Q;
};
void loo_blocks_plain(const LooCall& c, int64_t first, int64_t step) {
  for (int64_t g = first; g < c.n_block; g += step)
    loo_block<false>(c.rows, c.n, c.dim, c.t, c.K, c.mean, c.tmean, c.V, c.m, c.S, c.B, c.L, c.lev0, c.resid_l, c.resid, g, c.part + g * c.Q);
}
__attribute__((target("fma"))) void loo_blocks_fma(const LooCall& c, int64_t first, int64_t step) {
  for (int64_t g = first; g < c.n_block; g += step)
    loo_block<true>(c.rows, c.n, c.dim, c.t, c.K, c.mean, c.tmean, c.V, c.m, c.S, c.B, c.L, c.lev0, c.resid_l, c.resid, g, c.part + g * c.Q);
}

bool all_finite(const float* a, int64_t n, int64_t* at) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) {
      *at = i;
      return false;
    }
  return true;
}

// what is wrong with the arguments the device call and the twin share, or an empty string
std::string check_loo(int64_t dim, int32_t K, bool targets, const float* mean, const float* tmean, const float* V, int32_t m, const float* S,
                      const float* B, int32_t L, float lev0, const int32_t* resid_l, const void* n_used, const void* sse, const void* sae,
                      const void* sse_fit, const void* dof, const void* resid) {
  if (K < 1 || K > SCANN_HEAD_MAX_TARGETS) return "K " + std::to_string(K) + " outside 1 .. " + std::to_string(SCANN_HEAD_MAX_TARGETS);
  if (L < 1 || L > SCANN_HEAD_MAX_LAMBDA) return "L " + std::to_string(L) + " outside 1 .. " + std::to_string(SCANN_HEAD_MAX_LAMBDA);
  if (m < 1 || m > dim) return "m " + std::to_string(m) + " outside 1 .. " + std::to_string(dim);
  if (!targets) return "targets is null";
  if (!mean) return "mean is null";
  if (!tmean) return "tmean is null";
  if (!V) return "components is null";
  if (!S) return "scale is null";
  if (!B) return "coef is null";
  if (!n_used) return "n_used is null";
  if (!sse) return "sse is null";
  if (!sae) return "sae is null";
  if (!sse_fit) return "sse_fit is null";
  if (!dof) return "dof is null";
  if (resid_l && !resid) return "resid_l needs resid, which is null";
  int64_t at = 0;
  if (!all_finite(mean, dim, &at)) return "mean holds a non-finite value (column " + std::to_string(at) + ")";
  if (!all_finite(tmean, K, &at)) return "tmean holds a non-finite value (target " + std::to_string(at) + ")";
  if (!all_finite(V, (int64_t)m * dim, &at)) return "components hold a non-finite value (component " + std::to_string(at / dim) + ")";
  if (!all_finite(S, (int64_t)L * m, &at)) return "scale holds a non-finite value (strength " + std::to_string(at / m) + ")";
  if (!all_finite(B, (int64_t)L * K * m, &at)) return "coef holds a non-finite value (strength " + std::to_string(at / ((int64_t)K * m)) + ")";
  if (!std::isfinite(lev0)) return "lev0 is not finite";
  for (int32_t k = 0; resid_l && k < K; ++k)
    if (resid_l[k] < -1 || resid_l[k] >= L) return "resid_l[" + std::to_string(k) + "] = " + std::to_string(resid_l[k]) + " outside -1 .. " + std::to_string(L - 1);
  return "";
}

void loo_outputs(const double* q, int32_t L, int32_t K, int64_t* n_used, double* sse, double* sae, double* sse_fit, double* dof) {
  const int64_t LK = (int64_t)L * K;
  std::copy(q, q + LK, sse);
  std::copy(q + LK, q + 2 * LK, sae);
  std::copy(q + 2 * LK, q + 3 * LK, sse_fit);
  std::copy(q + 3 * LK, q + 3 * LK + L, dof);
  *n_used = (int64_t)q[3 * LK + L];
}

}  // namespace

namespace scann {

std::string check_head_eval(int dim, const float* mean, const float* tmean, const float* weights, int32_t K, const float* components, int32_t m,
                            const float* scale, float lev0, const float* pred, const float* lev) {
  if (K < 1 || K > SCANN_HEAD_MAX_TARGETS) return "K " + std::to_string(K) + " outside 1 .. " + std::to_string(SCANN_HEAD_MAX_TARGETS);
  if (m < 1 || m > dim) return "m " + std::to_string(m) + " outside 1 .. " + std::to_string(dim);
  if (!mean) return "mean is null";
  if (!tmean) return "tmean is null";
  if (!weights) return "weights is null";
  if (!components) return "components is null";
  if (!scale) return "scale is null";
  if (!pred) return "pred is null";
  if (!lev) return "lev is null";
  int64_t at = 0;
  if (!all_finite(mean, dim, &at)) return "mean holds a non-finite value (column " + std::to_string(at) + ")";
  if (!all_finite(tmean, K, &at)) return "tmean holds a non-finite value (target " + std::to_string(at) + ")";
  if (!all_finite(weights, (int64_t)K * dim, &at)) return "weights hold a non-finite value (target " + std::to_string(at / dim) + ")";
  if (!all_finite(components, (int64_t)m * dim, &at)) return "components hold a non-finite value (component " + std::to_string(at / dim) + ")";
  if (!all_finite(scale, (int64_t)K * m, &at)) return "scale holds a non-finite value (target " + std::to_string(at / m) + ")";
  if (!std::isfinite(lev0)) return "lev0 is not finite";
  return "";
}

int head_eval_rows(scann_handle* h, hipStream_t s, const float* src, int pitch, int64_t nq, int dim, const float* mean, const float* tmean,
                   const float* weights, int32_t K, const float* components, int32_t m, const float* scale, float lev0, float* pred, float* lev) {
  const int stride = (dim + 3) / 4 * 4;
  PcaProjArgs pa{};
  pa.first = 0; pa.n = (int32_t)nq; pa.chunk_rows = 0x7fffffff; pa.stride = stride; pa.dim = dim;
  HeadEvalArgs ea{};
  ea.n = (int32_t)nq; ea.m = m; ea.K = K; ea.lev0 = lev0;
  CallWs ws;
  RowStage st;  // rows of the padded width, as an index keeps them
  float *d_W, *d_V;
  ws.take(pa.mean, (size_t)stride); ws.take(d_W, (size_t)K * stride); ws.take(d_V, (size_t)m * stride);
  st.take(ws, nq, dim, pitch, stride, hipMemcpyDeviceToDevice);
  const size_t zeroed = ws.bytes();
  ws.take(pa.rows, 1); ws.take(ea.w, (size_t)nq * K); ws.take(ea.z, (size_t)nq * m); ws.take(ea.tmean, (size_t)K); ws.take(ea.scale, (size_t)K * m);
  ws.take(ea.pred, (size_t)nq * K); ws.take(ea.lev, (size_t)nq * K);
  HIPCHK(h, ws.alloc());
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = st.stage_rows(src, s, false);
  const void* tab = st.rows(src);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(pa.mean), mean, (size_t)dim * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(d_W, (size_t)stride * 4, weights, (size_t)dim * 4, (size_t)dim * 4, (size_t)K, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(d_V, (size_t)stride * 4, components, (size_t)dim * 4, (size_t)dim * 4, (size_t)m, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(pa.rows), &tab, 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(ea.tmean), tmean, (size_t)K * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(ea.scale), scale, (size_t)K * m * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {  // w: the projection on the K weight rows (the kernel takes any m)
    pa.comp = d_W; pa.m = K; pa.coords = writable(ea.w);
    e = launch_pca_project(pa, s);
  }
  if (e == hipSuccess) {
    pa.comp = d_V; pa.m = m; pa.coords = writable(ea.z);
    e = launch_pca_project(pa, s);
  }
  if (e == hipSuccess) e = launch_head_eval(ea, s);
  if (e == hipSuccess) e = hipMemcpyAsync(pred, ea.pred, (size_t)nq * K * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(lev, ea.lev, (size_t)nq * K * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  return SCANN_OK;
}

}  // namespace scann

extern "C" {

int scann_ridge_loo_host(const float* rows, int64_t n, int64_t dim, const float* targets, int32_t K, const float* mean, const float* tmean,
                         const float* components, int32_t m, const float* scale, const float* coef, int32_t L, float lev0, const int32_t* resid_l,
                         int64_t* n_used, double* sse, double* sae, double* sse_fit, double* dof, float* resid) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || (n > 0 && !rows)) return SCANN_ERR_INVALID;
  if (!check_loo(dim, K, targets || n == 0, mean, tmean, components, m, scale, coef, L, lev0, resid_l, n_used, sse, sae, sse_fit,
                 dof, resid).empty())
    return SCANN_ERR_INVALID;
  const int64_t LK = (int64_t)L * K, Q = 3 * LK + L + 1, n_block = (n + HEAD_TILE - 1) / HEAD_TILE;
  std::vector<double> part((size_t)(std::max<int64_t>(n_block, 1) * Q), 0.0);
  LooCall c{rows, targets, mean, tmean, components, scale, coef, n, dim, K, m, L, lev0, resid_l, resid_l ? resid : nullptr, part.data(), n_block, Q};
  const bool fma = __builtin_cpu_supports("fma");
  const double work = (double)n * (double)m * ((double)dim + (double)L * (K + 1));
  const int64_t nt = work < 2e7 ? 1 : std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(), n_block}));
  if (nt == 1) {
    fma ? loo_blocks_fma(c, 0, 1) : loo_blocks_plain(c, 0, 1);
  } else {  // thread k: blocks k, k + nt, ...; every block's sums are its own
    std::vector<std::thread> pool;
    for (int64_t k = 0; k < nt; ++k) pool.emplace_back(fma ? loo_blocks_fma : loo_blocks_plain, std::cref(c), k, nt);
    for (auto& th : pool) th.join();
  }
  std::vector<double> q((size_t)Q, 0.0);
  for (int64_t g = 0; g < n_block; ++g)
    for (int64_t i = 0; i < Q; ++i) q[(size_t)i] += part[(size_t)(g * Q + i)];
  loo_outputs(q.data(), L, K, n_used, sse, sae, sse_fit, dof);
  return SCANN_OK;
}

int scann_index_fit_moments(scann_handle_t* h, scann_index_t* pool, const float* targets, int32_t K, int64_t* n_eligible, float* mean, double* cov,
                            int32_t* col_exp, int32_t* bits) {
  if (const int r = check_pool(h, pool, "scann_index_fit_moments")) return r;
  if (K < 1 || K > SCANN_HEAD_MAX_TARGETS)
    return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: K " + std::to_string(K) + " outside 1 .. " + std::to_string(SCANN_HEAD_MAX_TARGETS));
  if (!n_eligible) return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: n_eligible is null");
  if (!mean) return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: mean is null");
  if (!cov) return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: cov is null");
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride, D = dim + K;
  if (const int r = check_pool_rows(h, pool, "scann_index_fit_moments", (int64_t)0x7fffffff - 1024)) return r;
  if (N == 0) {
    *n_eligible = 0;
    return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: a covariance needs at least 2 rows, the pool has 0");
  }
  if (!targets) return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: targets is null");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  PcaArgs a{};
  HeadMomArgs m{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride; a.dim = dim;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  m.K = K;
  // one workspace for the call; what the memset clears comes first
  CallWs ws;
  ws.take(a.st, 1); ws.take(a.colmax, (size_t)stride); ws.take(a.cenmax, (size_t)stride); ws.take(a.sums, (size_t)stride); ws.take(a.R, (size_t)stride);
  ws.take(a.T, (size_t)stride * stride); ws.take(m.tmax, HEAD_KMAX); ws.take(m.tcen, HEAD_KMAX); ws.take(m.tsum, HEAD_KMAX); ws.take(m.Rt, HEAD_KMAX);
  ws.take(m.Ttt, HEAD_KMAX * HEAD_KMAX); ws.take(m.Txt, (size_t)stride * HEAD_KMAX);
  const size_t zeroed = ws.bytes();
  ws.take(a.mean, (size_t)stride); ws.take(a.col_exp, (size_t)stride); ws.take(a.cov, (size_t)dim * dim); ws.take(a.rows, (size_t)a.n_chunk);
  ws.take(a.elig, (size_t)N); ws.take(a.mask, (size_t)N); ws.take(m.t, (size_t)N * K); ws.take(m.tmean, HEAD_KMAX); ws.take(m.texp, HEAD_KMAX);
  ws.take(m.cross, (size_t)D * K);
  HIPCHK(h, ws.alloc());
  PcaState st{};
  std::vector<float> mean_h((size_t)dim), tmean_h(HEAD_KMAX);
  std::vector<double> cov_h((size_t)dim * dim), cross_h((size_t)D * K);
  std::vector<int32_t> exp_h((size_t)dim), texp_h(HEAD_KMAX);
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, a.n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(m.t), targets, (size_t)N * K * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_head_mask(nullptr, 0, 0, a.n_total, m.t, K, writable(a.mask), s);
  if (e == hipSuccess) e = launch_pca_moments(a, s);
  if (e == hipSuccess) e = launch_head_moments(a, m, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(PcaState), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(mean_h.data(), a.mean, (size_t)dim * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(cov_h.data(), a.cov, (size_t)dim * dim * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(exp_h.data(), a.col_exp, (size_t)dim * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tmean_h.data(), m.tmean, HEAD_KMAX * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(texp_h.data(), m.texp, HEAD_KMAX * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(cross_h.data(), m.cross, (size_t)D * K * 8, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  *n_eligible = st.n;
  if (st.n < 2)
    return fail(h, SCANN_ERR_INVALID, "scann_index_fit_moments: a covariance needs at least 2 rows without a non-finite component or target, the pool has " +
                                          std::to_string(st.n) + " among its " + std::to_string(N));
  std::copy(mean_h.begin(), mean_h.end(), mean);
  std::copy(tmean_h.begin(), tmean_h.begin() + K, mean + dim);
  for (int32_t i = 0; i < dim; ++i)
    for (int32_t j = 0; j < dim; ++j) cov[(size_t)i * D + j] = cov_h[(size_t)i * dim + j];
  for (int32_t i = 0; i < D; ++i)
    for (int32_t k = 0; k < K; ++k) cov[(size_t)i * D + dim + k] = cov[(size_t)(dim + k) * D + i] = cross_h[(size_t)i * K + k];
  if (col_exp) {
    std::copy(exp_h.begin(), exp_h.end(), col_exp);
    std::copy(texp_h.begin(), texp_h.begin() + K, col_exp + dim);
  }
  if (bits) *bits = scann_pca_bits(st.n);
  return SCANN_OK;
}

int scann_index_ridge_loo(scann_handle_t* h, scann_index_t* pool, const float* targets, int32_t K, const float* mean, const float* tmean,
                          const float* components, int32_t m, const float* scale, const float* coef, int32_t L, float lev0, const int32_t* resid_l,
                          int64_t* n_used, double* sse, double* sae, double* sse_fit, double* dof, float* resid) {
  if (const int r = check_pool(h, pool, "scann_index_ridge_loo")) return r;
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride;
  const std::string bad = check_loo(dim, K, targets || N == 0, mean, tmean, components, m, scale, coef, L, lev0, resid_l, n_used, sse, sae,
                                    sse_fit, dof, resid);
  if (!bad.empty()) return fail(h, SCANN_ERR_INVALID, "scann_index_ridge_loo: " + bad);
  if (const int r = check_pool_rows(h, pool, "scann_index_ridge_loo", (int64_t)0x7fffffff - 1024)) return r;
  const int64_t LK = (int64_t)L * K, Q = 3 * LK + L + 1, n_tile = (N + HEAD_TILE - 1) / HEAD_TILE;
  std::vector<double> q((size_t)Q, 0.0);
  if (N == 0) {
    loo_outputs(q.data(), L, K, n_used, sse, sae, sse_fit, dof);
    return SCANN_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int n_chunk = (int)pool->chunks.size();
  // the coordinates pass through a device block of at most 256 MiB, a group of whole tiles at a time
  const int64_t g = std::min<int64_t>(n_tile * HEAD_TILE, std::max<int64_t>(HEAD_TILE, (((int64_t)256 << 20) / ((int64_t)m * 4)) / HEAD_TILE * HEAD_TILE));
  PcaProjArgs pa{};
  pa.chunk_rows = pool->chunk_rows; pa.stride = stride; pa.dim = dim; pa.m = m;
  HeadLooArgs la{};
  la.m = m; la.L = L; la.K = K; la.lev0 = lev0;
  double* d_out;
  CallWs ws;
  ws.take(pa.mean, (size_t)stride); ws.take(pa.comp, (size_t)m * stride);
  const size_t zeroed = ws.bytes();  // (the padding columns of the mean and of the components are zero)
  ws.take(pa.rows, (size_t)n_chunk); ws.take(pa.coords, (size_t)g * m); ws.take(la.t, (size_t)N * K); ws.take(la.tmean, (size_t)K);
  ws.take(la.scale, (size_t)L * m); ws.take(la.coef, (size_t)LK * m); ws.take(la.elig, (size_t)N); ws.take(la.resid_l, (size_t)K);
  ws.take(la.resid, resid_l ? (size_t)N * K : 0); ws.take(la.part, (size_t)n_tile * Q); ws.take(d_out, (size_t)Q);
  HIPCHK(h, ws.alloc());
  la.z = pa.coords;
  if (!resid_l) la.resid_l = nullptr, la.resid = nullptr;
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(pa.mean), mean, (size_t)dim * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(writable(pa.comp), (size_t)stride * 4, components, (size_t)dim * 4, (size_t)dim * 4, (size_t)m, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, n_chunk, pa.rows, nullptr, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(la.t), targets, (size_t)N * K * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(la.tmean), tmean, (size_t)K * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(la.scale), scale, (size_t)L * m * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(la.coef), coef, (size_t)LK * m * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && resid_l) e = hipMemcpyAsync(writable(la.resid_l), resid_l, (size_t)K * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && resid_l) e = hipMemsetAsync(la.resid, 0xff, (size_t)N * K * 4, s);  // NaN wherever the kernel writes nothing
  if (e == hipSuccess) e = launch_head_mask(pa.rows, pool->chunk_rows, stride, (int32_t)N, la.t, K, writable(la.elig), s);
  for (int64_t r0 = 0; r0 < N && e == hipSuccess; r0 += g) {
    const int64_t cnt = std::min<int64_t>(g, N - r0);
    pa.first = (int32_t)r0; pa.n = (int32_t)cnt;
    la.first = (int32_t)r0; la.n = (int32_t)cnt;
    e = launch_pca_project(pa, s);
    if (e == hipSuccess) e = launch_head_loo(la, s);  // (the stream orders the next group's projection behind this group's tiles)
  }
  if (e == hipSuccess) e = launch_head_sum(la.part, (int32_t)n_tile, (int32_t)Q, d_out, s);
  if (e == hipSuccess) e = hipMemcpyAsync(q.data(), d_out, (size_t)Q * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && resid_l) e = hipMemcpyAsync(resid, la.resid, (size_t)N * K * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  loo_outputs(q.data(), L, K, n_used, sse, sae, sse_fit, dof);
  return SCANN_OK;
}

int scann_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* tmean, const float* weights, int32_t K,
                     const float* components, int32_t m, const float* scale, float lev0, float* y, float* ga, float* pred, float* lev) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_head_batch: null handle or batch");
  const int dim = level_dim(h, level);
  if (!dim) return bad_level(h, level, "scann_head_batch");
  const std::string bad = check_head_eval(dim, mean, tmean, weights, K, components, m, scale, lev0, pred, lev);
  if (!bad.empty()) return fail(h, SCANN_ERR_INVALID, "scann_head_batch: " + bad);
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_head_batch: weights not loaded");
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int64_t nq = atom ? db->n_atom : db->n_struct;
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  if (nq <= 0) return SCANN_OK;
  // the level's rows where the forward left them
  return head_eval_rows(h, h->streams[db->last_slot], atom ? db->out_z : db->out_bf, dim, nq, dim, mean, tmean, weights, K, components, m, scale, lev0,
                        pred, lev);
}

}  // extern "C"

// Classification head on a latent-space index, the host half (include/scann_hip.h): scann_index_logit_pass and scann_logit_head_batch
// around the kernels of scann_logit.hip, and the twin scann_logit_pass_host (the kernels' bits: the logit chains, logit_softmax of
// scann_logit.h and the block / span / spans summation tree, threaded over the spans).  Every floating-point expression here is evaluated
// as written, each operation rounded to nearest: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <cmath>
#include <thread>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_logit.h"
#include "scann_runtime.h"

using namespace scann;

namespace {

constexpr int64_t SPAN_ROWS = (int64_t)LOGIT_BLOCK * LOGIT_SPAN;

struct PassCall {
  const float* rows;
  int64_t n, dim;
  const int32_t* labels;
  int32_t C;
  const float *mean, *U;
  int32_t M;
  const int32_t* fold;
  int32_t F;
  const int32_t* prob_of_fold;
  float* prob;
  double *gpart, *spart;  // [n_span][M * C * (dim + 1)], [n_span][M * 6]
  int64_t* used;          // [n_span]
  int64_t n_span;
};

// the sums of span s
template <bool FMA>
inline void span_sums(const PassCall& c, int64_t s) {
  const int64_t D1 = c.dim + 1, G = (int64_t)c.M * c.C * D1, S = (int64_t)c.M * 6;
  double *g = c.gpart + s * G, *st = c.spart + s * S;
  std::vector<double> gb((size_t)G), sb((size_t)S);
  std::vector<float> y((size_t)c.dim);
  int64_t used = 0;
  for (int64_t b = 0; b < LOGIT_SPAN; ++b) {
    const int64_t p0 = s * SPAN_ROWS + b * LOGIT_BLOCK;
    if (p0 >= c.n) break;
    std::fill(gb.begin(), gb.end(), 0.0);
    std::fill(sb.begin(), sb.end(), 0.0);
    for (int64_t p = p0; p < std::min<int64_t>(c.n, p0 + LOGIT_BLOCK); ++p) {
      const float* x = c.rows + p * c.dim;
      const int32_t label = c.labels[p];
      if (label < 0 || label >= c.C || !finite_row(x, c.dim)) continue;
      ++used;
      for (int64_t j = 0; j < c.dim; ++j) y[(size_t)j] = x[j] - c.mean[j];
      const int32_t fp = c.F > 0 ? (int32_t)(p % c.F) : 0;
      for (int32_t m = 0; m < c.M; ++m) {
        float a[LOGIT_CMAX] = {}, pv[LOGIT_CMAX], brier;
        int best;
        for (int32_t k = 0; k < c.C; ++k) {
          const float* w = c.U + ((int64_t)m * c.C + k) * D1;
          float acc = w[c.dim];
          for (int64_t j = 0; j < c.dim; ++j) acc = FMA ? __builtin_fmaf(y[(size_t)j], w[j], acc) : std::fmaf(y[(size_t)j], w[j], acc);
          a[k] = acc;
        }
        logit_softmax(a, c.C, label, pv, brier, best);
        const int32_t f = c.fold[m];
        const bool held = f >= 0 && fp == f;
        double* q = sb.data() + (int64_t)m * 6 + (held ? 3 : 0);
        q[0] += 1.0;
        q[1] += best == label ? 1.0 : 0.0;
        q[2] += (double)brier;
        if (c.prob && c.prob_of_fold && c.prob_of_fold[fp] == m)
          for (int32_t k = 0; k < c.C; ++k) c.prob[p * c.C + k] = pv[k];
        if (held) continue;
        for (int32_t k = 0; k < c.C; ++k) {
          const float r = (k == label ? 1.f : 0.f) - pv[k];
          const double rd = (double)r;
          double* gk = gb.data() + ((int64_t)m * c.C + k) * D1;
          for (int64_t j = 0; j < c.dim; ++j) gk[j] = FMA ? __builtin_fma(rd, (double)y[(size_t)j], gk[j]) : std::fma(rd, (double)y[(size_t)j], gk[j]);
          gk[c.dim] += rd;
        }
      }
    }
    for (int64_t i = 0; i < G; ++i) g[i] += gb[(size_t)i];
    for (int64_t i = 0; i < S; ++i) st[i] += sb[(size_t)i];
  }
  c.used[s] = used;
}

void spans_plain(const PassCall& c, int64_t first, int64_t step) {
  for (int64_t s = first; s < c.n_span; s += step) span_sums<false>(c, s);
}
__attribute__((target("fma"))) void spans_fma(const PassCall& c, int64_t first, int64_t step) {
  for (int64_t s = first; s < c.n_span; s += step) span_sums<true>(c, s);
}

// what is wrong with the arguments the device call and the twin share, or an empty string
std::string check_pass(int64_t n, int64_t dim, const int32_t* labels, int32_t C, const float* mean, const float* weights, int32_t M, const int32_t* fold,
                       int32_t F, const int32_t* prob_of_fold, const void* n_used, const void* grad, const void* stats, const void* prob) {
  if (C < 2 || C > SCANN_LOGIT_MAX_CLASSES) return "C " + std::to_string(C) + " outside 2 .. " + std::to_string(SCANN_LOGIT_MAX_CLASSES);
  if (M < 1 || M > SCANN_LOGIT_MAX_MODELS) return "M " + std::to_string(M) + " outside 1 .. " + std::to_string(SCANN_LOGIT_MAX_MODELS);
  if (F != 0 && (F < 2 || F > 16)) return "F " + std::to_string(F) + " is neither 0 nor in 2 .. 16";
  if (n > 0 && !labels) return "labels is null";
  if (!mean) return "mean is null";
  if (!weights) return "weights is null";
  if (!fold) return "fold is null";
  if (!n_used) return "n_used is null";
  if (!grad) return "grad is null";
  if (!stats) return "stats is null";
  if (prob && !prob_of_fold) return "prob needs prob_of_fold, which is null";
  for (int32_t j = 0; j < M; ++j)
    if (fold[j] < -1 || fold[j] >= F) return "fold[" + std::to_string(j) + "] = " + std::to_string(fold[j]) + " outside -1 .. " + std::to_string(F - 1);
  for (int32_t f = 0; prob_of_fold && f < std::max(F, 1); ++f)
    if (prob_of_fold[f] < -1 || prob_of_fold[f] >= M)
      return "prob_of_fold[" + std::to_string(f) + "] = " + std::to_string(prob_of_fold[f]) + " outside -1 .. " + std::to_string(M - 1);
  for (int64_t j = 0; j < dim; ++j)
    if (!std::isfinite(mean[j])) return "mean holds a non-finite value (column " + std::to_string(j) + ")";
  const int64_t D1 = dim + 1;
  for (int64_t i = 0; i < (int64_t)M * C * D1; ++i)
    if (!std::isfinite(weights[i]))
      return "weights hold a non-finite value (model " + std::to_string(i / (C * D1)) + ", class " + std::to_string(i / D1 % C) + ")";
  for (int64_t p = 0; p < n; ++p)
    if (labels[p] < -1 || labels[p] >= C)
      return "labels[" + std::to_string(p) + "] = " + std::to_string(labels[p]) + " outside -1 .. " + std::to_string(C - 1);
  return "";
}

}  // namespace

extern "C" {

int scann_logit_pass_host(const float* rows, int64_t n, int64_t dim, const int32_t* labels, int32_t C, const float* mean, const float* weights, int32_t M,
                          const int32_t* fold, int32_t F, const int32_t* prob_of_fold, int64_t* n_used, double* grad, double* stats, float* prob) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || (n > 0 && !rows)) return SCANN_ERR_INVALID;
  if (!check_pass(n, dim, labels, C, mean, weights, M, fold, F, prob_of_fold, n_used, grad, stats, prob).empty()) return SCANN_ERR_INVALID;
  const int64_t D1 = dim + 1, G = (int64_t)M * C * D1, S = (int64_t)M * 6, n_span = (n + SPAN_ROWS - 1) / SPAN_ROWS;
  std::fill(grad, grad + G, 0.0);
  std::fill(stats, stats + S, 0.0);
  *n_used = 0;
  const float nan = std::nanf("");
  for (int64_t i = 0; prob && i < n * C; ++i) prob[i] = nan;
  if (n == 0) return SCANN_OK;
  std::vector<double> gpart((size_t)(n_span * G), 0.0), spart((size_t)(n_span * S), 0.0);
  std::vector<int64_t> used((size_t)n_span, 0);
  PassCall c{rows, n, dim, labels, C, mean, weights, M, fold, F, prob_of_fold, prob, gpart.data(), spart.data(), used.data(), n_span};
  const bool fma = __builtin_cpu_supports("fma");
  const double work = (double)n * (double)dim * (double)M * C;
  const int64_t nt = work < 2e7 ? 1 : std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(), n_span}));
  if (nt == 1) {
    fma ? spans_fma(c, 0, 1) : spans_plain(c, 0, 1);
  } else {  // thread k: spans k, k + nt, ...; every span's sums (and rows of prob) are its own
    std::vector<std::thread> pool;
    for (int64_t k = 0; k < nt; ++k) pool.emplace_back(fma ? spans_fma : spans_plain, std::cref(c), k, nt);
    for (auto& th : pool) th.join();
  }
  for (int64_t s = 0; s < n_span; ++s) {
    for (int64_t i = 0; i < G; ++i) grad[i] += gpart[(size_t)(s * G + i)];
    for (int64_t i = 0; i < S; ++i) stats[i] += spart[(size_t)(s * S + i)];
    *n_used += used[(size_t)s];
  }
  return SCANN_OK;
}

int scann_index_logit_pass(scann_handle_t* h, scann_index_t* pool, const int32_t* labels, int32_t C, const float* mean, const float* weights, int32_t M,
                           const int32_t* fold, int32_t F, const int32_t* prob_of_fold, int64_t* n_used, double* grad, double* stats, float* prob) {
  const std::string w = "scann_index_logit_pass: ";
  if (const int r = check_pool(h, pool, "scann_index_logit_pass")) return r;
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride;
  const std::string bad = check_pass(N, dim, labels, C, mean, weights, M, fold, F, prob_of_fold, n_used, grad, stats, prob);
  if (!bad.empty()) return fail(h, SCANN_ERR_INVALID, w + bad);
  if (const int r = check_pool_rows(h, pool, "scann_index_logit_pass", (int64_t)0x7fffffff - 1024)) return r;
  const int64_t D1 = (int64_t)dim + 1, G = (int64_t)M * C * D1, S = (int64_t)M * 6, n_span = (N + SPAN_ROWS - 1) / SPAN_ROWS;
  std::fill(grad, grad + G, 0.0);
  std::fill(stats, stats + S, 0.0);
  *n_used = 0;
  if (N == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int n_chunk = (int)pool->chunks.size();
  const int per = LOGIT_COLS / C;  // models of one launch
  const int gcol = std::min(M, per) * C;
  LogitArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride; a.dim = dim;
  a.C = C; a.F = F;
  float *d_u, *d_u0;
  double *d_grad, *d_stats;
  CallWs ws;
  ws.take(a.mean, (size_t)stride); ws.take(d_u, (size_t)M * C * stride);
  const size_t zeroed = ws.bytes();  // (the padding columns of the mean and of the weights are zero)
  ws.take(d_u0, (size_t)M * C); ws.take(a.rows, (size_t)n_chunk); ws.take(a.labels, (size_t)N); ws.take(a.gpart, (size_t)n_span * gcol * D1);
  ws.take(a.spart, (size_t)n_span * LOGIT_GMAX * 6); ws.take(d_grad, (size_t)G); ws.take(d_stats, (size_t)S); ws.take(a.n_used, (size_t)n_span);
  ws.take(a.prob, prob ? (size_t)N * C : 0);
  HIPCHK(h, ws.alloc());
  if (!prob) a.prob = nullptr;
  std::vector<float> u0((size_t)M * C);
  for (int64_t i = 0; i < (int64_t)M * C; ++i) u0[(size_t)i] = weights[i * D1 + dim];
  std::vector<int64_t> used((size_t)n_span, 0);
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.mean), mean, (size_t)dim * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(d_u, (size_t)stride * 4, weights, (size_t)D1 * 4, (size_t)dim * 4, (size_t)M * C, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_u0, u0.data(), (size_t)M * C * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = ws.upload_rows(pool, n_chunk, a.rows, nullptr, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.labels), labels, (size_t)N * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && prob) e = launch_logit_fill_nan(a.prob, N * C, s);  // NaN wherever the kernel writes nothing
  for (int j0 = 0; j0 < M && e == hipSuccess; j0 += per) {  // the stream orders a group's launch behind the sums of the one before
    const int nm = std::min(per, M - j0);
    a.n_model = nm; a.ncol = nm * C;
    a.u = d_u + (size_t)j0 * C * stride;
    a.u0 = d_u0 + (size_t)j0 * C;
    for (int j = 0; j < LOGIT_GMAX; ++j) a.fold[j] = j < nm ? fold[j0 + j] : -1;
    for (int f = 0; f < LOGIT_CMAX; ++f) {
      const int m = prob && f < std::max(F, 1) ? prob_of_fold[f] : -1;
      a.prob_model[f] = m >= j0 && m < j0 + nm ? m - j0 : -1;
    }
    e = hipMemsetAsync(a.gpart, 0, (size_t)n_span * a.ncol * D1 * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.spart, 0, (size_t)n_span * nm * 6 * 8, s);
    if (e == hipSuccess) e = launch_logit_pass(a, s);
    if (e == hipSuccess) e = launch_logit_sum(a.gpart, (int32_t)n_span, (int32_t)(a.ncol * D1), d_grad + (size_t)j0 * C * D1, s);
    if (e == hipSuccess) e = launch_logit_sum(a.spart, (int32_t)n_span, nm * 6, d_stats + (size_t)j0 * 6, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(grad, d_grad, (size_t)G * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(stats, d_stats, (size_t)S * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(used.data(), a.n_used, (size_t)n_span * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && prob) e = hipMemcpyAsync(prob, a.prob, (size_t)N * C * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  for (int64_t i = 0; i < n_span; ++i) *n_used += used[(size_t)i];
  return SCANN_OK;
}

int scann_logit_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* weights, int32_t C, float* y, float* ga,
                           float* prob) {
  const std::string w = "scann_logit_head_batch: ";
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, w + "null handle or batch");
  const int dim = level_dim(h, level);
  if (!dim) return bad_level(h, level, "scann_logit_head_batch");
  if (C < 2 || C > SCANN_LOGIT_MAX_CLASSES)
    return fail(h, SCANN_ERR_INVALID, w + "C " + std::to_string(C) + " outside 2 .. " + std::to_string(SCANN_LOGIT_MAX_CLASSES));
  if (!mean) return fail(h, SCANN_ERR_INVALID, w + "mean is null");
  if (!weights) return fail(h, SCANN_ERR_INVALID, w + "weights is null");
  if (!prob) return fail(h, SCANN_ERR_INVALID, w + "prob is null");
  for (int j = 0; j < dim; ++j)
    if (!std::isfinite(mean[j])) return fail(h, SCANN_ERR_INVALID, w + "mean holds a non-finite value (column " + std::to_string(j) + ")");
  for (int i = 0; i < C * (dim + 1); ++i)
    if (!std::isfinite(weights[i])) return fail(h, SCANN_ERR_INVALID, w + "weights hold a non-finite value (class " + std::to_string(i / (dim + 1)) + ")");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, w + "weights not loaded");
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int64_t nq = atom ? db->n_atom : db->n_struct;
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  if (nq <= 0) return SCANN_OK;
  hipStream_t s = h->streams[db->last_slot];
  const float* src = atom ? db->out_z : db->out_bf;  // the level's rows where the forward left them
  float *d_mean, *d_u, *d_prob;
  CallWs ws;
  ws.take(d_mean, (size_t)dim); ws.take(d_u, (size_t)C * (dim + 1)); ws.take(d_prob, (size_t)nq * C);
  HIPCHK(h, ws.alloc());
  hipError_t e = hipMemcpyAsync(d_mean, mean, (size_t)dim * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_u, weights, (size_t)C * (dim + 1) * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_logit_eval(src, dim, (int32_t)nq, dim, d_mean, d_u, C, d_prob, s);
  if (e == hipSuccess) e = hipMemcpyAsync(prob, d_prob, (size_t)nq * C * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  return SCANN_OK;
}

}  // extern "C"

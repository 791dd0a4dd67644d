// Gaussian landmark features of a latent-space index, the host half (include/scann_hip.h): scann_rbf_weight, scann_index_rbf_features and
// scann_rbf_head_batch around the kernel of scann_rbf.hip, and the twin scann_rbf_features_host (the kernel's bits: the distance chain of
// scann_knn_distsq and the weight chain of scann_rbf.h).  Every floating-point expression here is evaluated as written, each operation
// rounded to nearest: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <cmath>

#include "scann_call.h"
#include "scann_head.h"
#include "scann_knn.h"
#include "scann_rbf.h"
#include "scann_runtime.h"

using namespace scann;

namespace {

// what is wrong with the landmarks and gamma, or an empty string
std::string check_landmarks(const float* landmarks, int32_t m, int64_t dim, float gamma) {
  if (m < 1 || m > 1024) return "m " + std::to_string(m) + " outside 1 .. 1024";
  if (!landmarks) return "landmarks is null";
  for (int64_t i = 0; i < (int64_t)m * dim; ++i)
    if (!std::isfinite(landmarks[i]))
      return "landmarks hold a non-finite value (landmark " + std::to_string(i / dim) + ", column " + std::to_string(i % dim) + ")";
  if (bad_gamma(gamma)) return "gamma must be finite and > 0";
  return "";
}

}  // namespace

extern "C" {

float scann_rbf_weight(float dist2, float gamma) { return rbf_weight(dist2, gamma); }

void scann_rbf_weight_array(const float* dist2, int64_t n, float gamma, float* out) {
  for (int64_t i = 0; dist2 && out && i < n; ++i) out[i] = rbf_weight(dist2[i], gamma);
}

int scann_rbf_features_host(const float* rows, int64_t n, int64_t dim, const float* landmarks, int32_t m, float gamma, float* phi) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || (n > 0 && (!rows || !phi))) return SCANN_ERR_INVALID;
  if (!check_landmarks(landmarks, m, dim, gamma).empty()) return SCANN_ERR_INVALID;
  if (n == 0) return SCANN_OK;
  scann_knn_distsq_matrix(rows, n, landmarks, m, dim, phi);  // the pool row is the chain's first argument
  const float nan = std::nanf("");
  for (int64_t p = 0; p < n; ++p) {
    const bool ok = finite_row(rows + p * dim, dim);
    for (int32_t c = 0; c < m; ++c) phi[p * m + c] = ok ? rbf_weight(phi[p * m + c], gamma) : nan;
  }
  return SCANN_OK;
}

int scann_index_rbf_features(scann_handle_t* h, scann_index_t* pool, const float* landmarks, int32_t m, float gamma, scann_index_t* out) {
  const std::string w = "scann_index_rbf_features: ";
  if (!h || !pool) return fail(h, SCANN_ERR_INVALID, w + "null handle or pool");
  if (!out) return fail(h, SCANN_ERR_INVALID, w + "out is null");
  if (pool->h != h) return fail(h, SCANN_ERR_INVALID, w + "the pool belongs to another handle");
  if (out->h != h) return fail(h, SCANN_ERR_INVALID, w + "out belongs to another handle");
  if (out == pool) return fail(h, SCANN_ERR_INVALID, w + "out is the pool itself");
  const std::string bad = check_landmarks(landmarks, m, pool->dim, gamma);
  if (!bad.empty()) return fail(h, SCANN_ERR_INVALID, w + bad);
  if (out->n != 0 || !out->chunks.empty()) return fail(h, SCANN_ERR_INVALID, w + "out is not empty: it holds " + std::to_string(out->n) + " rows");
  if (out->dim != m) return fail(h, SCANN_ERR_INVALID, w + "out holds rows of " + std::to_string(out->dim) + " columns, m is " + std::to_string(m));
  const int64_t N = pool->n;
  if (N > (int64_t)0x7fffffff - 1024) return fail(h, SCANN_ERR_UNSUPPORTED, w + "the pool has too many rows");
  if (N == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const int32_t stride = pool->stride;
  const int n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows), n_out = (int)((N + out->chunk_rows - 1) / out->chunk_rows);
  RbfArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride;
  a.m = m; a.gamma = gamma;
  a.out_chunk_rows = out->chunk_rows; a.out_stride = out->stride;
  CallWs ws;
  ws.take(a.lm, (size_t)m * stride);
  const size_t zeroed = ws.bytes();  // (the landmarks' padding columns are zero)
  ws.take(a.rows, (size_t)n_chunk); ws.take(a.out, (size_t)n_out);
  HIPCHK(h, ws.alloc());
  int r = SCANN_OK;
  for (int c = 0; c < n_out && !r; ++c) r = index_new_chunk(h, out, s);  // the chunks an append of N rows would take, cleared
  hipError_t e = hipSuccess;
  if (!r) {
    e = hipMemsetAsync(ws.base(), 0, zeroed, s);
    if (e == hipSuccess) e = hipMemcpy2DAsync(writable(a.lm), (size_t)stride * 4, landmarks, (size_t)pool->dim * 4, (size_t)pool->dim * 4, (size_t)m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = ws.upload_rows(pool, n_chunk, a.rows, nullptr, s);
    if (e == hipSuccess) e = ws.upload_rows(out, n_out, a.out, nullptr, s);
    if (e == hipSuccess) e = launch_rbf_features(a, s);
    for (int c = 0; c < n_out && e == hipSuccess; ++c) {  // the ids travel with the rows: the pool's host copies
      const int64_t r0 = (int64_t)c * out->chunk_rows;
      e = hipMemcpyAsync(out->ids_of((size_t)c), pool->ids.data() + r0, (size_t)std::min<int64_t>(out->chunk_rows, N - r0) * 8, hipMemcpyHostToDevice, s);
    }
  }
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  if (r || e != hipSuccess || e_sync != hipSuccess) {  // nothing stays allocated: out is empty again
    for (char* p : out->chunks) cached_free(p);
    out->chunks.clear();
  }
  if (r) return r;
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  index_note_rows(out, N, pool->ids.data(), pool->atoms.data());
  return SCANN_OK;
}

int scann_rbf_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* landmarks, int32_t m, float gamma, const float* mean,
                         const float* tmean, const float* weights, int32_t K, const float* components, int32_t mm, const float* scale, float lev0,
                         float* y, float* ga, float* pred, float* lev, float* phi) {
  const std::string w = "scann_rbf_head_batch: ";
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, w + "null handle or batch");
  const int dim = level_dim(h, level);
  if (!dim) return bad_level(h, level, "scann_rbf_head_batch");
  std::string bad = check_landmarks(landmarks, m, dim, gamma);
  if (bad.empty()) bad = check_head_eval(m, mean, tmean, weights, K, components, mm, scale, lev0, pred, lev);  // a head over the m features
  if (!bad.empty()) return fail(h, SCANN_ERR_INVALID, w + bad);
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, w + "weights not loaded");
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int64_t nq = atom ? db->n_atom : db->n_struct;
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  if (nq <= 0) return SCANN_OK;
  hipStream_t s = h->streams[db->last_slot];
  const float* src = atom ? db->out_z : db->out_bf;  // the level's rows where the forward left them
  const int stride = (dim + 3) / 4 * 4, ms = (m + 3) / 4 * 4;
  RbfArgs a{};
  a.n_total = (int32_t)nq; a.chunk_rows = 0x7fffffff; a.stride = stride;
  a.m = m; a.gamma = gamma;
  a.out_chunk_rows = 0x7fffffff; a.out_stride = ms;
  float* feat;
  CallWs ws;
  RowStage st;  // rows of the padded width, as an index keeps them
  ws.take(a.lm, (size_t)m * stride);
  st.take(ws, nq, dim, dim, stride, hipMemcpyDeviceToDevice);
  const size_t zeroed = ws.bytes();
  ws.take(feat, (size_t)nq * ms); ws.take(a.rows, 1); ws.take(a.out, 1);
  HIPCHK(h, ws.alloc());
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess) e = st.stage_rows(src, s, false);
  const void* tab[2] = {st.rows(src), feat};
  if (e == hipSuccess) e = hipMemcpy2DAsync(writable(a.lm), (size_t)stride * 4, landmarks, (size_t)dim * 4, (size_t)dim * 4, (size_t)m, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.rows), &tab[0], 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.out), &tab[1], 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_rbf_features(a, s);
  if (e == hipSuccess && phi) e = hipMemcpy2DAsync(phi, (size_t)m * 4, feat, (size_t)ms * 4, (size_t)m * 4, (size_t)nq, hipMemcpyDeviceToHost, s);
  int r = SCANN_OK;
  if (e == hipSuccess) r = head_eval_rows(h, s, feat, ms, nq, m, mean, tmean, weights, K, components, mm, scale, lev0, pred, lev);  // (waits)
  else (void)hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  return r;
}

}  // extern "C"

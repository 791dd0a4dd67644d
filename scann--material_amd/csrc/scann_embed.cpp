// Neighbour embedding of a latent-space index, the host half (include/scann_hip.h): scann_embed_iterate around the kernels of
// scann_embed.hip, and the twin scann_embed_iterate_host (the kernels' bits: the pair, gradient and update bodies of scann_embed.h and the
// block / span / spans summation tree, the repulsion threaded over the row blocks).  Every floating-point expression here is evaluated as
// written, each operation rounded to nearest: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <cmath>
#include <thread>

#include "scann_call.h"
#include "scann_embed.h"
#include "scann_runtime.h"

using namespace scann;

namespace {

// what is wrong with the arguments the device call and the twin share, or an empty string
std::string check_embed(int64_t N, const int64_t* row_first, const int32_t* col, const float* p, const float* y, const float* u, const float* gain,
                        int32_t n_iter, float exaggeration, float momentum, float lr, const double* z_out) {
  if (!row_first) return "row_first is null";
  if (!col) return "col is null";
  if (!p) return "p is null";
  if (!y) return "y is null";
  if (!u) return "u is null";
  if (!gain) return "gain is null";
  if (!z_out) return "z_out is null";
  if (N < 2 || N > SCANN_EMBED_MAX_ROWS) return "N " + std::to_string(N) + " outside 2 .. " + std::to_string(SCANN_EMBED_MAX_ROWS);
  if (n_iter < 0 || n_iter > 100000) return "n_iter " + std::to_string(n_iter) + " outside 0 .. 100000";
  if (!(std::isfinite(exaggeration) && exaggeration > 0.f)) return "exaggeration " + std::to_string(exaggeration) + " is not finite and positive";
  if (!(std::isfinite(lr) && lr > 0.f)) return "lr " + std::to_string(lr) + " is not finite and positive";
  if (!(momentum >= 0.f && momentum < 1.f)) return "momentum " + std::to_string(momentum) + " outside [0, 1)";
  if (row_first[0] != 0) return "row_first[0] = " + std::to_string(row_first[0]) + ", not 0";
  for (int64_t i = 0; i < N; ++i)
    if (row_first[i + 1] < row_first[i])
      return "row_first decreases at row " + std::to_string(i) + " (" + std::to_string(row_first[i]) + " -> " + std::to_string(row_first[i + 1]) + ")";
  for (int64_t i = 0; i < N; ++i)
    for (int64_t e = row_first[i]; e < row_first[i + 1]; ++e) {
      if (col[e] < 0 || col[e] >= N) return "col[" + std::to_string(e) + "] = " + std::to_string(col[e]) + " outside 0 .. " + std::to_string(N - 1);
      if (col[e] == i) return "col[" + std::to_string(e) + "] = " + std::to_string(col[e]) + " is its own row";
      if (!(std::isfinite(p[e]) && p[e] >= 0.f)) return "p[" + std::to_string(e) + "] is negative or not finite";
    }
  for (int64_t i = 0; i < 2 * N; ++i) {
    if (!std::isfinite(y[i])) return "y holds a non-finite value (row " + std::to_string(i / 2) + ")";
    if (!std::isfinite(u[i])) return "u holds a non-finite value (row " + std::to_string(i / 2) + ")";
    if (!std::isfinite(gain[i])) return "gain holds a non-finite value (row " + std::to_string(i / 2) + ")";
  }
  return "";
}

// sum over i < n of v(i) in the definition's tree: blocks of 128 in position order, spans of 32 blocks, spans in order
template <class F>
inline double tree_sum(int64_t n, F v) {
  double total = 0.0;
  for (int64_t s0 = 0; s0 < n; s0 += EMBED_SPAN_ROWS) {
    double span = 0.0;
    for (int64_t b0 = s0; b0 < std::min<int64_t>(n, s0 + EMBED_SPAN_ROWS); b0 += EMBED_BLOCK) {
      double block = 0.0;
      for (int64_t i = b0; i < std::min<int64_t>(n, b0 + EMBED_BLOCK); ++i) block += v(i);
      span += block;
    }
    total += span;
  }
  return total;
}

struct Repel {
  int64_t N;
  const float* y;  // [N][2]
  double* rs;      // [3][N]: Z_i, Rx_i, Ry_i
};

// rows i0 .. i0 + 7 (those below N), which lie in one block: eight rows at a time against the blocks that hold none of them, row by row
// against their own block
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpsabi"
__attribute__((always_inline)) inline void repel_rows8(const Repel& c, int64_t i0) {
  const int64_t N = c.N, nr = std::min<int64_t>(8, N - i0), own = i0 / EMBED_BLOCK;
  embed_v8 xi, yi;
  for (int r = 0; r < 8; ++r) {
    const int64_t i = std::min(i0 + r, N - 1);
    xi[r] = c.y[2 * i];
    yi[r] = c.y[2 * i + 1];
  }
  double Z[8] = {}, Rx[8] = {}, Ry[8] = {};
  for (int64_t s0 = 0; s0 < N; s0 += EMBED_SPAN_ROWS) {
    double sz[8] = {}, sx[8] = {}, sy[8] = {};
    for (int64_t j0 = s0; j0 < std::min<int64_t>(N, s0 + EMBED_SPAN_ROWS); j0 += EMBED_BLOCK) {
      const int64_t j1 = std::min<int64_t>(N, j0 + EMBED_BLOCK);
      if (j0 / EMBED_BLOCK != own) {
        embed_v8 z = 0.f, rx = 0.f, ry = 0.f;
        for (int64_t j = j0; j < j1; ++j) embed_repel(xi, yi, c.y[2 * j], c.y[2 * j + 1], z, rx, ry);
        for (int r = 0; r < 8; ++r) sz[r] += (double)z[r], sx[r] += (double)rx[r], sy[r] += (double)ry[r];
      } else {
        for (int r = 0; r < nr; ++r) {
          float z = 0.f, rx = 0.f, ry = 0.f;
          const float x0 = xi[r], y0 = yi[r];
          for (int64_t j = j0; j < j1; ++j)
            if (j != i0 + r) embed_repel(x0, y0, c.y[2 * j], c.y[2 * j + 1], z, rx, ry);
          sz[r] += (double)z, sx[r] += (double)rx, sy[r] += (double)ry;
        }
      }
    }
    for (int r = 0; r < 8; ++r) Z[r] += sz[r], Rx[r] += sx[r], Ry[r] += sy[r];
  }
  for (int r = 0; r < nr; ++r) c.rs[i0 + r] = Z[r], c.rs[N + i0 + r] = Rx[r], c.rs[2 * N + i0 + r] = Ry[r];
}

void repel_plain(const Repel& c, int64_t first, int64_t step) {
  for (int64_t i0 = 8 * first; i0 < c.N; i0 += 8 * step) repel_rows8(c, i0);
}
__attribute__((target("avx2,fma"))) void repel_avx2(const Repel& c, int64_t first, int64_t step) {
  for (int64_t i0 = 8 * first; i0 < c.N; i0 += 8 * step) repel_rows8(c, i0);
}

#pragma clang diagnostic pop

// one iteration on the host: y, u, gain in place; Z returned, grad [N * 2] written; y2 [N * 2], rs [3 * N] are work space
double iterate_host(int64_t N, const int64_t* row_first, const int32_t* col, const float* p, float* y, float* u, float* gain, float exaggeration,
                    float momentum, float lr, float* grad, float* y2, double* rs) {
  const Repel c{N, y, rs};
  const bool fast = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
  const int64_t groups = (N + 7) / 8;
  const int64_t nt = (double)N * (double)N < 4e6 ? 1 : std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(), groups}));
  if (nt == 1) {
    fast ? repel_avx2(c, 0, 1) : repel_plain(c, 0, 1);
  } else {  // thread k: the groups of eight rows k, k + nt, ...; every row's sums are its own
    std::vector<std::thread> pool;
    for (int64_t k = 0; k < nt; ++k) pool.emplace_back(fast ? repel_avx2 : repel_plain, std::cref(c), k, nt);
    for (auto& th : pool) th.join();
  }
  const double Z = tree_sum(N, [&](int64_t i) { return rs[i]; });
  for (int64_t i = 0; i < N; ++i) {
    float ax = 0.f, ay = 0.f;
    for (int64_t e = row_first[i]; e < row_first[i + 1]; ++e) {
      const int64_t j = col[e];
      embed_attract(y[2 * i], y[2 * i + 1], y[2 * j], y[2 * j + 1], p[e], ax, ay);
    }
    const float a[2] = {ax, ay};
    for (int k = 0; k < 2; ++k) {
      const float g = embed_gradient(exaggeration, a[k], rs[(k + 1) * N + i], Z);
      grad[2 * i + k] = g;
      y2[2 * i + k] = embed_update(g, lr, momentum, y[2 * i + k], u[2 * i + k], gain[2 * i + k]);
    }
  }
  for (int k = 0; k < 2; ++k) {
    const double S = tree_sum(N, [&](int64_t i) { return (double)y2[2 * i + k]; });
    const float mean = (float)(S / (double)N);
    for (int64_t i = 0; i < N; ++i) y[2 * i + k] = y2[2 * i + k] - mean;
  }
  return Z;
}

}  // namespace

extern "C" {

int scann_embed_iterate_host(int64_t N, const int64_t* row_first, const int32_t* col, const float* p, float* y, float* u, float* gain, int32_t n_iter,
                             float exaggeration, float momentum, float lr, double* z_out, float* grad_out) {
  if (!check_embed(N, row_first, col, p, y, u, gain, n_iter, exaggeration, momentum, lr, z_out).empty()) return SCANN_ERR_INVALID;
  *z_out = 0.0;
  if (n_iter == 0) return SCANN_OK;
  std::vector<float> grad((size_t)(2 * N)), y2((size_t)(2 * N));
  std::vector<double> rs((size_t)(3 * N));
  for (int32_t it = 0; it < n_iter; ++it)
    *z_out = iterate_host(N, row_first, col, p, y, u, gain, exaggeration, momentum, lr, grad.data(), y2.data(), rs.data());
  if (grad_out) std::copy(grad.begin(), grad.end(), grad_out);
  return SCANN_OK;
}

int scann_embed_iterate(scann_handle_t* h, int64_t N, const int64_t* row_first, const int32_t* col, const float* p, float* y, float* u, float* gain,
                        int32_t n_iter, float exaggeration, float momentum, float lr, double* z_out, float* grad_out) {
  const std::string w = "scann_embed_iterate: ";
  if (!h) return fail(h, SCANN_ERR_INVALID, w + "null handle");
  const std::string bad = check_embed(N, row_first, col, p, y, u, gain, n_iter, exaggeration, momentum, lr, z_out);
  if (!bad.empty()) return fail(h, SCANN_ERR_INVALID, w + bad);
  *z_out = 0.0;
  if (n_iter == 0) return SCANN_OK;
  const int64_t E = row_first[N], n_block = (N + EMBED_BLOCK - 1) / EMBED_BLOCK, n_span = (N + EMBED_SPAN_ROWS - 1) / EMBED_SPAN_ROWS;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  TsneArgs a{};
  a.N = (int32_t)N; a.n_span = (int32_t)n_span;
  a.exaggeration = exaggeration; a.momentum = momentum; a.lr = lr;
  CallWs ws;
  ws.take(a.row_first, (size_t)N + 1); ws.take(a.col, (size_t)E); ws.take(a.p, (size_t)E); ws.take(a.y[0], (size_t)N); ws.take(a.y[1], (size_t)N);
  ws.take(a.u, (size_t)N); ws.take(a.gain, (size_t)N); ws.take(a.grad, (size_t)N); ws.take(a.part, (size_t)n_span * 3 * N); ws.take(a.rsum, (size_t)3 * N);
  ws.take(a.bsum, (size_t)3 * n_block); ws.take(a.z_out, 1);
  HIPCHK(h, ws.alloc());
  hipError_t e = hipMemcpyAsync(writable(a.row_first), row_first, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && E > 0) e = hipMemcpyAsync(writable(a.col), col, (size_t)E * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && E > 0) e = hipMemcpyAsync(writable(a.p), p, (size_t)E * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(a.y[0], y, (size_t)N * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(a.u, u, (size_t)N * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(a.gain, gain, (size_t)N * 8, hipMemcpyHostToDevice, s);
  int cur = 0;
  for (int32_t it = 0; it < n_iter && e == hipSuccess; ++it, cur ^= 1) e = launch_embed_iteration(a, cur, s);
  std::vector<float> grad(grad_out ? (size_t)(2 * N) : 0);  // (the outputs change only if the call succeeds)
  std::vector<float> yo((size_t)(2 * N)), uo((size_t)(2 * N)), go((size_t)(2 * N));
  double z = 0.0;
  if (e == hipSuccess) e = hipMemcpyAsync(yo.data(), a.y[cur], (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(uo.data(), a.u, (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(go.data(), a.gain, (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && grad_out) e = hipMemcpyAsync(grad.data(), a.grad, (size_t)N * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&z, a.z_out, 8, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  std::copy(yo.begin(), yo.end(), y);
  std::copy(uo.begin(), uo.end(), u);
  std::copy(go.begin(), go.end(), gain);
  if (grad_out) std::copy(grad.begin(), grad.end(), grad_out);
  *z_out = z;
  return SCANN_OK;
}

}  // extern "C"

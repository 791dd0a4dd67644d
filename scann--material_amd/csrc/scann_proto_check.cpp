// Stand-alone driver of the prototypes' and criticisms' host twins (scann_prototypes_host, scann_criticisms_host) for the sanitizers:
// `make asan-proto` compiles it with scann_proto.cpp and the density twin it is composed of (scann_peaks.cpp) under AddressSanitizer +
// UBSan (host code only, no device is touched) and runs it.  It walks N = 1, 2, 9, 100 and 1100 (the last over the density pass's threads),
// dim 1, 3 and 130, m from 1 to beyond N, duplicate, coincident and non-finite rows, both loops' refusals, and checks the twins against
// the loops written out in the definition's words over a plain term matrix.
#include "scann_peaks.cpp"
#include "scann_proto.cpp"

#include "scann_check.h"

// the stubs of its own
namespace scann {
hipError_t launch_peaks_density(const PeaksArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_peaks_finish(const PeaksArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_peaks_parent(const PeaksArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_knn_merge(const float*, const int32_t*, int, int, int, float*, int32_t*, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_proto_prepare(const ProtoArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_crit_prepare(const ProtoArgs&, const int32_t*, int32_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_proto_step(const ProtoArgs&, bool, int, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

// t(i, j) of every pair, from the plain chain
std::vector<int64_t> term_matrix(const std::vector<float>& rows, int64_t n, int64_t dim, float gamma) {
  std::vector<int64_t> t((size_t)(n * n));
  std::vector<float> d((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    dist2_to_rows(&rows[(size_t)(i * dim)], rows.data(), n, dim, d.data());
    for (int64_t j = 0; j < n; ++j) t[(size_t)(i * n + j)] = peaks_term(d[(size_t)j], gamma);
  }
  return t;
}

void check_pool(const std::vector<float>& rows, int64_t n, int64_t dim, int64_t m, float gamma) {
  const std::vector<int64_t> t = term_matrix(rows, n, dim, gamma);
  std::vector<char> ok((size_t)n);
  int64_t n_el = 0;
  for (int64_t i = 0; i < n; ++i) n_el += ok[(size_t)i] = finite_row(&rows[(size_t)(i * dim)], dim);
  std::vector<int64_t> A((size_t)n, -1), B((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (!ok[(size_t)i]) continue;
    A[(size_t)i] = 0;
    for (int64_t j = 0; j < n; ++j)
      if (ok[(size_t)j]) A[(size_t)i] += t[(size_t)(i * n + j)];
  }
  std::vector<int32_t> pos((size_t)m, 7);
  std::vector<int64_t> score((size_t)m, 7), bap((size_t)m, 7), gA((size_t)n, 7), gB((size_t)n, 7);
  const int64_t cnt = scann_prototypes_host(rows.data(), n, dim, m, gamma, pos.data(), score.data(), bap.data(), gA.data(), gB.data());
  EXPECT(cnt == std::min(m, n_el));
  EXPECT(gA == A);
  std::vector<char> picked((size_t)n, 0);
  for (int64_t s = 0; s < cnt; ++s) {
    int64_t best = -1, bs = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (!ok[(size_t)i] || picked[(size_t)i]) continue;
      const int64_t sc = (s + 1) * A[(size_t)i] - n_el * B[(size_t)i];
      if (best < 0 || sc > bs) best = i, bs = sc;
    }
    EXPECT(pos[(size_t)s] == best && score[(size_t)s] == bs && bap[(size_t)s] == B[(size_t)best]);
    if (best < 0) break;
    picked[(size_t)best] = 1;
    for (int64_t i = 0; i < n; ++i)
      if (ok[(size_t)i]) B[(size_t)i] += t[(size_t)(i * n + best)];
  }
  EXPECT(gB == B);
  for (int64_t s = cnt; s < m; ++s) EXPECT(pos[(size_t)s] == -1 && score[(size_t)s] == 0 && bap[(size_t)s] == 0);
  if (cnt < 1) return;
  // the criticisms under max(W, 0), scaled to 31 bits, the prototypes excluded
  std::vector<int64_t> weight((size_t)n, 0);
  int64_t top = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (ok[(size_t)i]) weight[(size_t)i] = std::max<int64_t>(cnt * A[(size_t)i] - n_el * B[(size_t)i], 0);
    top = std::max(top, weight[(size_t)i]);
  }
  int shift = 0;
  while ((top >> shift) >> 31) ++shift;
  for (auto& x : weight) x >>= shift;
  const int64_t c = 5;
  std::vector<int32_t> cpos((size_t)c, 7), ex(pos.begin(), pos.begin() + cnt);
  std::vector<int64_t> cscore((size_t)c, 7);
  const int64_t ccnt = scann_criticisms_host(rows.data(), n, dim, weight.data(), ex.data(), cnt, c, gamma, cpos.data(), cscore.data());
  std::vector<int64_t> cmax((size_t)n, 0);
  std::vector<char> live((size_t)n);
  for (int64_t i = 0; i < n; ++i) live[(size_t)i] = ok[(size_t)i] && !picked[(size_t)i] && weight[(size_t)i] > 0;
  int64_t made = 0;
  for (; made < c; ++made) {
    int64_t best = -1, bs = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (!live[(size_t)i]) continue;
      const int64_t sc = weight[(size_t)i] * (((int64_t)1 << 30) - cmax[(size_t)i]);
      if (best < 0 || sc > bs) best = i, bs = sc;
    }
    if (best < 0 || bs <= 0) break;
    EXPECT(made < ccnt && cpos[(size_t)made] == best && cscore[(size_t)made] == bs);
    live[(size_t)best] = 0;
    for (int64_t i = 0; i < n; ++i) cmax[(size_t)i] = std::max(cmax[(size_t)i], t[(size_t)(i * n + best)]);
  }
  EXPECT(made == ccnt);
  for (int64_t s = ccnt; s < c; ++s) EXPECT(cpos[(size_t)s] == -1 && cscore[(size_t)s] == 0);
}

}  // namespace

int main() {
  state = 4321u;
  for (int64_t n : {1, 2, 9, 100, 1100}) {
    for (int64_t dim : {1, 3, 130}) {
      if (n == 1100 && dim != 130) continue;
      std::vector<float> rows((size_t)(n * dim));
      for (auto& x : rows) x = (float)(draw() % 9) * 0.5f - 2.f;
      if (n > 5) rows[(size_t)(5 * dim)] = NAN, rows[(size_t)(3 * dim + dim - 1)] = INFINITY;
      for (int64_t p = 20; p < 30 && p < n; ++p) std::copy(rows.begin() + 7 * dim, rows.begin() + 8 * dim, rows.begin() + p * dim);  // coincident rows
      for (int64_t m : {(int64_t)1, (int64_t)4, n + 3}) {
        if (n == 1100 && m != 4) continue;
        check_pool(rows, n, dim, m, dim == 130 ? 0.01f : 0.3f);
      }
    }
  }
  std::vector<float> same(40 * 3, 1.5f);
  check_pool(same, 40, 3, 6, 0.5f);
  // the refusals
  std::vector<float> rows(12, 1.f);
  std::vector<int32_t> pos(4), ex{4};
  std::vector<int64_t> w{1, 1, 1, 1};
  EXPECT(scann_prototypes_host(rows.data(), 4, 3, 0, 0.5f, pos.data(), nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);       // m
  EXPECT(scann_prototypes_host(rows.data(), 4, 3, 2, 0.f, pos.data(), nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);        // gamma
  EXPECT(scann_prototypes_host(rows.data(), 4, 3, 2, 0.5f, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);          // pos
  EXPECT(scann_prototypes_host(rows.data(), 4, 3, ((int64_t)1 << 30) + 1, 0.5f, pos.data(), nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);  // the range
  EXPECT(scann_prototypes_host(nullptr, 0, 3, 2, 0.5f, pos.data(), nullptr, nullptr, nullptr, nullptr) == 0);                            // an empty pool
  EXPECT(scann_prototypes_host(rows.data(), 4, 3, 2, 0.5f, pos.data(), nullptr, nullptr, nullptr, nullptr) == 2);                        // every optional output null
  EXPECT(scann_criticisms_host(rows.data(), 4, 3, w.data(), ex.data(), 1, 2, 0.5f, pos.data(), nullptr) == SCANN_ERR_INVALID);           // an excluded position outside
  w[2] = ((int64_t)1 << 31) + 1;
  EXPECT(scann_criticisms_host(rows.data(), 4, 3, w.data(), nullptr, 0, 2, 0.5f, pos.data(), nullptr) == SCANN_ERR_INVALID);             // a weight outside
  w[2] = -1;
  EXPECT(scann_criticisms_host(rows.data(), 4, 3, w.data(), nullptr, 0, 2, 0.5f, pos.data(), nullptr) == SCANN_ERR_INVALID);
  w[2] = (int64_t)1 << 31;
  EXPECT(scann_criticisms_host(rows.data(), 4, 3, w.data(), nullptr, 0, 0, 0.5f, pos.data(), nullptr) == SCANN_ERR_INVALID);             // c
  EXPECT(scann_criticisms_host(rows.data(), 4, 3, w.data(), nullptr, 0, 3, 0.5f, pos.data(), nullptr) == 1 && pos[0] == 2 && pos[1] == -1);  // coincident rows: one criticism
  EXPECT(scann_criticisms_host(nullptr, 0, 3, nullptr, nullptr, 0, 2, 0.5f, pos.data(), nullptr) == 0);
  return finish("scann_proto_check");
}

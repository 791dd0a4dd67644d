// Stand-alone driver of the ranks' host twin (scann_ranks_host) for the sanitizers: `make asan-ranks` compiles it with scann_ranks.cpp
// under AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  It walks the twin's paths -- all rows and a qpos
// subset, with and without dist2, m = 1, 31 and 32, probes that are -1, the query itself, repeated or ineligible, coincident rows, one
// and several threads, a pool that is no multiple of the 8-row block, the refusals -- and checks the twin against a count written out
// in the definition's words, and that the thread count does not enter the bytes.
#include "scann_ranks.cpp"

#include "scann_check.h"

// the stubs of its own
namespace scann {
hipError_t launch_ranks_prepare(const RanksArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_ranks_tiles(const RanksArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_ranks_finish(const RanksArgs&, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

// the definition, pair by pair
int32_t rank_by_count(const std::vector<float>& rows, int64_t n, int64_t dim, int64_t i, int64_t j) {
  if (j < 0 || j == i || !finite_row(&rows[(size_t)(i * dim)], dim) || !finite_row(&rows[(size_t)(j * dim)], dim)) return -1;
  const float dj = chain(&rows[(size_t)(i * dim)], &rows[(size_t)(j * dim)], dim);
  int32_t r = 0;
  for (int64_t l = 0; l < n; ++l) {
    if (l == i || !finite_row(&rows[(size_t)(l * dim)], dim)) continue;
    const float dl = chain(&rows[(size_t)(i * dim)], &rows[(size_t)(l * dim)], dim);
    r += dl < dj || (dl == dj && l < j);
  }
  return r;
}

}  // namespace

int main() {
  state = 12345u;
  auto draw = [] { return ::draw() & 0xffff; };
  for (int64_t n : {1, 2, 7, 8, 9, 203}) {
    for (int64_t dim : {1, 3, 130}) {
      std::vector<float> rows((size_t)(n * dim));
      for (auto& x : rows) x = (float)(draw() % 7) - 3.f;  // few values: many equal distances
      if (n > 5) rows[(size_t)(5 * dim)] = NAN, rows[(size_t)(3 * dim + dim - 1)] = INFINITY;
      for (int64_t p = 20; p < 60 && p < n; ++p) std::copy(rows.begin() + 20 * dim, rows.begin() + 21 * dim, rows.begin() + p * dim);  // 40 coincident rows
      std::vector<int32_t> q;
      for (int64_t p = n - 1; p >= 0; p -= 2) q.push_back((int32_t)p);
      for (int32_t m : {1, 31, 32}) {
        std::vector<int32_t> probe((size_t)(n * m));
        for (auto& p : probe) p = (int32_t)(draw() % (unsigned)(n + 1)) - 1;  // -1 .. n - 1: unused, the query itself and repeats among them
        std::vector<int32_t> one((size_t)(n * m), 7), many((size_t)(n * m), 7), part(q.size() * m, 7), qprobe(q.size() * m);
        std::vector<float> d1((size_t)(n * m), 7.f), d2((size_t)(n * m), 7.f);
        for (size_t i = 0; i < q.size(); ++i) std::copy(probe.begin() + q[i] * m, probe.begin() + (q[i] + 1) * m, qprobe.begin() + i * m);
        const int rc1 = scann_ranks_host(rows.data(), n, dim, nullptr, 0, probe.data(), m, 1, one.data(), d1.data());
        const int rc2 = scann_ranks_host(rows.data(), n, dim, nullptr, 0, probe.data(), m, 5, many.data(), d2.data());
        const int rc3 = scann_ranks_host(rows.data(), n, dim, q.data(), (int64_t)q.size(), qprobe.data(), m, 3, part.data(), nullptr);
        if (rc1 || rc2 || rc3 || one != many || std::memcmp(d1.data(), d2.data(), d1.size() * 4))
          ++bad, std::printf("n %lld dim %lld m %d: %d %d %d\n", (long long)n, (long long)dim, m, rc1, rc2, rc3);
        for (size_t i = 0; i < q.size(); ++i)
          if (std::memcmp(&part[i * m], &one[(size_t)q[i] * m], (size_t)m * 4)) ++bad, std::printf("n %lld dim %lld: query %zu of the subset differs\n", (long long)n, (long long)dim, i);
        for (int64_t i = 0; i < n; ++i)
          for (int32_t k = 0; k < m; ++k)
            if (one[(size_t)(i * m + k)] != rank_by_count(rows, n, dim, i, probe[(size_t)(i * m + k)]))
              ++bad, std::printf("n %lld dim %lld m %d: rank[%lld][%d] is not the count\n", (long long)n, (long long)dim, m, (long long)i, k);
      }
    }
  }
  std::vector<float> rows(12, 1.f);
  std::vector<int32_t> probe(8, 0), rank(8), q{4};
  if (scann_ranks_host(rows.data(), 4, 3, nullptr, 0, probe.data(), 0, 0, rank.data(), nullptr) != SCANN_ERR_INVALID) ++bad;   // m outside
  if (scann_ranks_host(rows.data(), 4, 3, nullptr, 0, probe.data(), 33, 0, rank.data(), nullptr) != SCANN_ERR_INVALID) ++bad;
  if (scann_ranks_host(rows.data(), 4, 3, q.data(), 1, probe.data(), 2, 0, rank.data(), nullptr) != SCANN_ERR_INVALID) ++bad;  // a position outside
  probe[5] = 4;
  if (scann_ranks_host(rows.data(), 4, 3, nullptr, 0, probe.data(), 2, 0, rank.data(), nullptr) != SCANN_ERR_INVALID) ++bad;   // a probe outside
  if (scann_ranks_host(rows.data(), 4, 3, nullptr, 0, nullptr, 2, 0, rank.data(), nullptr) != SCANN_ERR_INVALID) ++bad;        // a null argument
  if (scann_ranks_host(rows.data(), 0, 3, nullptr, 0, nullptr, 2, 0, nullptr, nullptr) != SCANN_OK) ++bad;                     // an empty pool
  return finish("scann_ranks_check");
}

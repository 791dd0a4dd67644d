// Stand-alone driver of the silhouette's host twin (scann_silhouette_host) for the sanitizers: `make asan-silhouette` compiles it with
// scann_silhouette.cpp under AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  It walks the twin's paths --
// all rows and a qpos subset, both metrics, the table, non-finite and unlabelled rows, one and several threads, a pool that is no
// multiple of the 8-row block, the refusals -- and checks that the thread count does not enter the bytes.
#include "scann_silhouette.cpp"

#include "scann_check.h"

// the stubs of its own
namespace scann {
hipError_t launch_sil_tiles(const SilArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_sil_finish(const SilArgs&, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

struct Out {
  std::vector<int64_t> counts, sums;
  std::vector<double> a, b;
  std::vector<int32_t> other;
  bool operator==(const Out& o) const {
    return counts == o.counts && sums == o.sums && other == o.other && !std::memcmp(a.data(), o.a.data(), a.size() * 8) &&
           !std::memcmp(b.data(), o.b.data(), b.size() * 8);
  }
};

int run(const std::vector<float>& rows, int64_t n, int64_t dim, const std::vector<int32_t>& lab, int32_t C, const std::vector<int32_t>* q,
        int squared, int shift, int threads, Out* o) {
  const int64_t m = q ? (int64_t)q->size() : n;
  o->counts.assign((size_t)C, 7), o->sums.assign((size_t)(m * C), 7), o->a.assign((size_t)m, 7.0), o->b.assign((size_t)m, 7.0), o->other.assign((size_t)m, 7);
  return scann_silhouette_host(rows.data(), n, dim, lab.data(), C, q ? q->data() : nullptr, m, squared, shift, threads, o->counts.data(), o->a.data(),
                               o->b.data(), o->other.data(), o->sums.data());
}

}  // namespace

int main() {
  state = 12345u;
  auto next = [] { return (float)(draw() & 0xffff) / 65536.f - 0.5f; };
  for (int64_t n : {1, 2, 7, 8, 9, 203}) {
    for (int64_t dim : {1, 3, 130}) {
      std::vector<float> rows((size_t)(n * dim));
      for (auto& x : rows) x = next();
      std::vector<int32_t> lab((size_t)n);
      for (int64_t p = 0; p < n; ++p) lab[(size_t)p] = (int32_t)(p % 5 == 4 ? -1 : p % 3);
      if (n > 5) rows[(size_t)(5 * dim)] = NAN, rows[(size_t)(3 * dim + dim - 1)] = INFINITY;
      std::vector<int32_t> q;
      for (int64_t p = n - 1; p >= 0; p -= 2) q.push_back((int32_t)p);
      for (int squared = 0; squared < 2; ++squared) {
        Out one, many, part;
        const int rc1 = run(rows, n, dim, lab, 4, nullptr, squared, 20, 1, &one), rc2 = run(rows, n, dim, lab, 4, nullptr, squared, 20, 5, &many);
        const int rc3 = run(rows, n, dim, lab, 4, &q, squared, 20, 3, &part);
        if (rc1 || rc2 || rc3 || !(one == many)) ++bad, std::printf("n %lld dim %lld squared %d: %d %d %d\n", (long long)n, (long long)dim, squared, rc1, rc2, rc3);
        for (size_t i = 0; i < q.size(); ++i)
          if (std::memcmp(&part.a[i], &one.a[(size_t)q[i]], 8) || part.other[i] != one.other[(size_t)q[i]] ||
              std::memcmp(&part.sums[i * 4], &one.sums[(size_t)q[i] * 4], 32))
            ++bad, std::printf("n %lld dim %lld: query %zu of the subset differs\n", (long long)n, (long long)dim, i);
        Out far;
        if (n > 1 && run(rows, n, dim, lab, 4, nullptr, squared, 126, 2, &far) != SCANN_ERR_RANGE && n > 2) ++bad, std::printf("shift 126 was not refused\n");
      }
    }
  }
  Out o;
  std::vector<float> rows(12, 1.f);
  std::vector<int32_t> lab{0, 1, 2, 9}, q{4};
  if (run(rows, 4, 3, lab, 3, nullptr, 0, 0, 0, &o) != SCANN_ERR_INVALID) ++bad;                              // a label outside
  lab[3] = -1;
  if (run(rows, 4, 3, lab, 3, &q, 0, 0, 0, &o) != SCANN_ERR_INVALID) ++bad;                                   // a position outside
  if (run(rows, 4, 3, lab, 3, nullptr, 0, 127, 0, &o) != SCANN_ERR_INVALID) ++bad;                            // a shift outside
  if (run(rows, 0, 3, lab, 3, nullptr, 0, 0, 0, &o) != SCANN_OK || o.counts != std::vector<int64_t>{0, 0, 0}) ++bad;  // an empty pool
  return finish("scann_silhouette_check");
}

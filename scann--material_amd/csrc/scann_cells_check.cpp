// Stand-alone driver of the partition's host twin (scann_cells_host) and of the bound (scann_cell_bound) for the sanitizers: `make
// asan-cells` compiles it with scann_cells.cpp and the two twins it is composed of (scann_select.cpp, scann_kmeans.cpp) under
// AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  It walks N = 1, 63, 64, 65 and 1000, a cell of exactly
// 64 rows, cells > N, identical rows, non-finite rows and the refusals, checks the layout's invariants -- every position once, whole
// tiles, shells ascending within a cell, lo / hi the bits of the tile's first and last real row -- and the bound against the chain.
// It also drives the pure pieces the searches share (scann_search.h): the order of a pass's queries, and the walk over a window of rows.
#include "scann_cells.cpp"
#include "scann_kmeans.cpp"
#include "scann_select.cpp"

#include "scann_check.h"

// the stubs of its own
namespace scann {
int search(scann_handle*, scann_index*, const float*, const int64_t*, int64_t, int, hipStream_t, float*, int64_t*, int32_t*, int32_t*, float*) {
  return SCANN_ERR_INVALID;
}
int search_full(scann_handle*, scann_index*, const float*, const int64_t*, int64_t, int, hipStream_t, float*, int64_t*, int32_t*, int32_t*, float*) {
  return SCANN_ERR_INVALID;
}
hipError_t launch_kcenter_prepare(const KcArgs&, bool, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_kcenter_step(const KcArgs&, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_kmeans_prepare(const KmArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_kmeans_gather(const KmArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_kmeans_round(const KmArgs&, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_knn_merge(const float*, const int32_t*, int, int, int, float*, int32_t*, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_cells_gather(const CellGatherArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_cells_roots(const float*, const float*, double*, double*, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_cells_list(const CellSearchArgs&, int, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

float scann_knn_distsq_local(const float* q, const float* r, int64_t d) {  // one pair of the chain
  float out;
  scann::dist2_to_rows(q, r, 1, d, &out);
  return out;
}

void check_partition(const std::vector<float>& rows, int64_t n, int64_t dim, int32_t cells, int32_t max_iter) {
  const int64_t cap = scann_cells_capacity(n, cells);
  std::vector<float> cen((size_t)cells * dim), lo((size_t)cap), hi((size_t)cap), d2((size_t)n);
  std::vector<int32_t> perm((size_t)cap * 64, -7), first((size_t)cells + 2);
  int64_t info[4];
  EXPECT(scann_cells_host(rows.data(), n, dim, cells, max_iter, info, cen.data(), perm.data(), first.data(), lo.data(), hi.data()) == SCANN_OK);
  const int64_t C = info[0], T = info[1];
  EXPECT(C <= cells && C <= n && T <= cap && first[(size_t)C + 1] == T && info[2] == 64 * T - n);
  std::vector<char> seen((size_t)n, 0);
  for (int64_t c = 0; c <= C; ++c)
    for (int64_t t = first[(size_t)c]; t < first[(size_t)c + 1]; ++t) {
      float prev = -1.f;
      int real = 0;
      for (int i = 0; i < 64; ++i) {
        const int32_t p = perm[(size_t)(t * 64 + i)];
        if (p < 0) continue;
        EXPECT(real == i);  // the pad entries close the tile
        ++real;
        EXPECT(p < n && !seen[(size_t)p]);
        if (p >= n) return;
        seen[(size_t)p] = 1;
        if (c == C) continue;
        const float d = scann_knn_distsq_local(&rows[(size_t)(p * dim)], &cen[(size_t)(c * dim)], dim);
        EXPECT(d >= prev);
        prev = d;
        if (i == 0) EXPECT(bits_of(d) == bits_of(lo[(size_t)t]));
        EXPECT(scann_cell_bound(d, lo[(size_t)t], hi[(size_t)t]) == 0.0);  // a row on the centre's side of its own shell is never excluded
      }
      EXPECT(real > 0);
      if (c < C) EXPECT(bits_of(prev) == bits_of(hi[(size_t)t]));
      else EXPECT(lo[(size_t)t] == 0.f && std::isinf(hi[(size_t)t]));
    }
  for (int64_t p = 0; p < n; ++p) EXPECT(seen[(size_t)p]);
}

// query_order (scann_search.h): a permutation of the pass's queries, ascending under (rank of the nearest cell, distance to its centre
// unless there is none, place), queries without a cell last in place order, then -1 to the end of the last group of 128 and no further
void check_query_order() {
  const int32_t C = 5;
  const std::vector<int32_t> ident = {0, 1, 2, 3, 4}, walk = {3, 0, 4, 1, 2};
  for (const std::vector<int32_t>& rank : {ident, walk})
    for (int32_t m : {1, 127, 128, 129}) {
      std::vector<int32_t> cell((size_t)m);
      std::vector<float> d((size_t)m);
      for (int32_t i = 0; i < m; ++i) cell[(size_t)i] = (int32_t)(draw() % (C + 1)) - 1, d[(size_t)i] = (float)(draw() % 3);  // many ties
      const size_t padded = (size_t)(m + 127) / 128 * 128;
      std::vector<int32_t> qperm(padded + 1, -7);
      scann::query_order(cell.data(), d.data(), rank.data(), C, m, qperm.data());
      std::vector<char> seen((size_t)m, 0);
      auto key = [&](int32_t x) { return cell[(size_t)x] < 0 ? C : rank[(size_t)cell[(size_t)x]]; };
      for (int32_t i = 0; i < m; ++i) {
        const int32_t y = qperm[(size_t)i];
        EXPECT(y >= 0 && y < m && !seen[(size_t)y]);
        if (y < 0 || y >= m) return;
        seen[(size_t)y] = 1;
        if (i == 0) continue;
        const int32_t x = qperm[(size_t)i - 1];
        if (key(x) != key(y)) EXPECT(key(x) < key(y));
        else if (key(x) < C && d[(size_t)x] != d[(size_t)y]) EXPECT(d[(size_t)x] < d[(size_t)y]);
        else EXPECT(x < y);
      }
      for (size_t i = (size_t)m; i < padded; ++i) EXPECT(qperm[i] == -1);
      EXPECT(qperm[padded] == -7);
    }
  // written out: cell 1 comes first on the walk {1, 0}; equal (cell, distance) by place; no cell: last, by place whatever the distance
  const int32_t cell[6] = {1, -1, 0, 1, -1, 0}, by_walk[2] = {1, 0}, by_number[2] = {0, 1};
  const float d[6] = {2.f, 9.f, 1.f, 2.f, 0.f, 1.f};
  std::vector<int32_t> qperm(128);
  scann::query_order(cell, d, by_walk, 2, 6, qperm.data());
  EXPECT((std::vector<int32_t>(qperm.begin(), qperm.begin() + 7) == std::vector<int32_t>{0, 3, 2, 5, 1, 4, -1}) && qperm[127] == -1);
  scann::query_order(cell, d, by_number, 2, 6, qperm.data());
  EXPECT((std::vector<int32_t>(qperm.begin(), qperm.begin() + 7) == std::vector<int32_t>{2, 5, 0, 3, 1, 4, -1}));
}

// row_runs (scann_search.h): the window cut at the chunk boundaries and nowhere else, every row once and in order
void check_row_runs() {
  scann_index ix;
  ix.chunk_rows = 64;
  struct Window { int64_t first, n; int runs; };
  // no boundary; starts on one; ends on one; spans one; spans three; a whole chunk; empty
  for (const Window& w : {Window{3, 10, 1}, Window{64, 10, 1}, Window{54, 10, 1}, Window{60, 10, 2}, Window{60, 140, 4}, Window{128, 64, 1}, Window{70, 0, 0}}) {
    int runs = 0;
    int64_t rows = 0;
    EXPECT(scann::row_runs(&ix, w.first, w.n, [&](size_t c, int64_t r0, int64_t m, int64_t done) {
             EXPECT(done == rows && (int64_t)c * 64 + r0 == w.first + done && m >= 1 && r0 >= 0 && r0 + m <= 64);
             EXPECT(runs == 0 ? true : r0 == 0);  // only the first run starts inside a chunk
             ++runs, rows += m;
             return 0;
           }) == 0);
    EXPECT(runs == w.runs && rows == w.n);
  }
  int runs = 0;  // a status that is not 0 ends the walk and is what the walk returns
  EXPECT(scann::row_runs(&ix, 60, 140, [&](size_t, int64_t, int64_t, int64_t) { return ++runs == 2 ? 7 : 0; }) == 7 && runs == 2);
}

std::vector<float> rows_of(int64_t n, int64_t dim, float scale) {
  std::vector<float> x((size_t)(n * dim));
  for (auto& v : x) v = ((float)(draw() % 20001) / 10000.f - 1.f) * scale;
  return x;
}

}  // namespace

int main() {
  state = 2025u;
  for (int64_t n : {1, 63, 64, 65, 1000})
    for (int64_t dim : {1, 3, 33})
      for (int32_t cells : {1, 2, 7, 64, 1024}) check_partition(rows_of(n, dim, 1.f), n, dim, cells, 3);
  {  // a cell of exactly 64 rows beside a far one of 5; identical rows; non-finite rows
    std::vector<float> x = rows_of(69, 2, 1.f);
    for (int i = 64; i < 69; ++i) x[(size_t)(2 * i)] += 1000.f;
    check_partition(x, 69, 2, 2, 8);
    check_partition(std::vector<float>(300, 1.5f), 100, 3, 4, 2);
    std::vector<float> y = rows_of(200, 3, 1.f);
    y[0] = NAN, y[3 * 70 + 1] = INFINITY, y[3 * 199 + 2] = -INFINITY;
    check_partition(y, 200, 3, 5, 8);
    check_partition(std::vector<float>(6, NAN), 2, 3, 2, 1);  // no eligible row: no cell, one loose tile
    std::vector<float> big = rows_of(100, 2, 3e19f);          // distances that overflow
    check_partition(big, 100, 2, 3, 2);
  }
  int64_t info[4];
  const std::vector<float> r = rows_of(10, 2, 1.f);
  EXPECT(scann_cells_host(r.data(), 10, 2, 0, 1, info, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_cells_host(r.data(), 10, 2, 1025, 1, info, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_cells_host(r.data(), 10, 2, 2, -1, info, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_cells_host(nullptr, 10, 2, 2, 1, info, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_cells_host(r.data(), 10, 2, 2, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_OK);
  // the bound: never above the chain, on shells round a centre at several magnitudes; and not always 0
  int positive = 0;
  for (float mag : {1e-22f, 1e-3f, 1.f, 1e6f, 3e18f})
    for (int64_t dim : {1, 3, 33}) {
      const std::vector<float> z = rows_of(1, dim, mag), x = rows_of(40, dim, mag * 0.01f), q = rows_of(40, dim, mag * 4.f);
      std::vector<float> xs((size_t)(40 * dim)), d((size_t)40), dq((size_t)40);
      for (size_t i = 0; i < xs.size(); ++i) xs[i] = z[i % (size_t)dim] + x[i];
      scann::dist2_to_rows(z.data(), xs.data(), 40, dim, d.data());
      float lo = d[0], hi = d[0];
      for (float v : d) lo = std::min(lo, v), hi = std::max(hi, v);
      for (int i = 0; i < 40; ++i) {
        const float D = scann_knn_distsq_local(&q[(size_t)(i * dim)], z.data(), dim);
        const double lb = scann_cell_bound(D, lo, hi);
        positive += lb > 0.0;
        scann::dist2_to_rows(&q[(size_t)(i * dim)], xs.data(), 40, dim, dq.data());
        for (float v : dq) EXPECT(!((double)v < lb));
      }
    }
  EXPECT(positive > 0);
  EXPECT(scann_cell_bound(INFINITY, 0.f, 1.f) == 0.0 && scann_cell_bound(NAN, 0.f, 1.f) == 0.0 && scann_cell_bound(4.f, 0.f, INFINITY) == 0.0);
  EXPECT(scann_cell_bound(100.f, 0.f, 1.f) > 80.0 && scann_cell_bound(0.f, 100.f, 121.f) > 99.0 && scann_cell_bound(1.f, 1.f, 1.f) == 0.0);
  check_query_order();
  check_row_runs();
  return finish("scann_cells_check");
}

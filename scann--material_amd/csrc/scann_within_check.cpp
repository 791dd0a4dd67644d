// Stand-alone driver of the radius search's host twin (scann_within_host) and of the host-side scatter and sort that give a result its
// order (within_finish) for the sanitizers: `make asan-within` compiles it with scann_within.cpp under AddressSanitizer + UBSan (host
// code only, no device is touched) and runs it.  Planted cases: exact copies at radius 0, the inclusive boundary, `upper`, query ids,
// non-finite rows, an empty table, the cap protocol with sentinel-filled arrays, records handed to within_finish in a scrambled order,
// and the refusals.
#include "scann_within.cpp"

#include "scann_check.h"

// the stubs of its own
namespace scann {
int expand_ids(scann_handle*, const scann_dbatch*, bool, const int64_t*, int64_t, std::vector<int64_t>&, std::vector<int32_t>*) { return SCANN_ERR_INVALID; }
hipError_t launch_within_tile(const WithinArgs&, int, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

std::vector<float> rows_of(int64_t n, int64_t dim, int levels) {
  std::vector<float> x((size_t)(n * dim));
  for (auto& v : x) v = (float)(draw() % (unsigned)levels);
  return x;
}

struct Result {
  std::vector<int64_t> counts;
  int64_t total = -1;
  std::vector<float> d;
  std::vector<int32_t> p;
};

// the twin by the protocol: a count-only call, then a call with cap = total; cap = total - 1 must leave sentinels alone
Result run(const std::vector<float>& rows, int64_t n, int64_t dim, const std::vector<float>& q, int64_t nq, const int64_t* row_ids, const int64_t* qid,
           const int32_t* qpos, int upper, float r2) {
  Result out;
  out.counts.assign((size_t)nq, -1);
  EXPECT(scann_within_host(rows.data(), n, dim, row_ids, q.data(), nq, qid, qpos, upper, r2, 0, out.counts.data(), &out.total, nullptr, nullptr) == SCANN_OK);
  const int64_t total = out.total;
  out.d.assign((size_t)total + 1, -7.f);
  out.p.assign((size_t)total + 1, -7);
  std::vector<int64_t> c2((size_t)nq, -1);
  int64_t t2 = -1;
  if (total > 0) {
    EXPECT(scann_within_host(rows.data(), n, dim, row_ids, q.data(), nq, qid, qpos, upper, r2, total - 1 > 0 ? total - 1 : 1, c2.data(), &t2,
                             out.d.data(), out.p.data()) == SCANN_OK);
    if (total > 1) {
      EXPECT(t2 == total && c2 == out.counts);
      for (int64_t i = 0; i <= total; ++i) EXPECT(out.d[(size_t)i] == -7.f && out.p[(size_t)i] == -7);
    }
    EXPECT(scann_within_host(rows.data(), n, dim, row_ids, q.data(), nq, qid, qpos, upper, r2, total, c2.data(), &t2, out.d.data(), out.p.data()) == SCANN_OK);
    EXPECT(t2 == total && c2 == out.counts && out.d[(size_t)total] == -7.f && out.p[(size_t)total] == -7);
  }
  // against the definition, pair by pair
  int64_t at = 0;
  for (int64_t i = 0; i < nq; ++i) {
    std::vector<std::pair<float, int32_t>> want;
    for (int64_t r = 0; r < n; ++r) {
      float d;
      scann::dist2_to_rows(&q[(size_t)(i * dim)], &rows[(size_t)(r * dim)], 1, dim, &d);
      if (!(d <= r2)) continue;
      if (qpos && (r == qpos[i] || (upper && r < qpos[i]))) continue;
      if (qid && (row_ids ? row_ids[r] : r) == qid[i]) continue;
      want.push_back({d, (int32_t)r});
    }
    std::sort(want.begin(), want.end());
    EXPECT((int64_t)want.size() == out.counts[(size_t)i]);
    for (size_t j = 0; j < want.size() && at + (int64_t)j < total; ++j) {
      uint32_t a, b;
      std::memcpy(&a, &want[j].first, 4); std::memcpy(&b, &out.d[(size_t)at + j], 4);
      EXPECT(a == b && want[j].second == out.p[(size_t)at + j]);
    }
    at += (int64_t)want.size();
  }
  EXPECT(at == total);
  return out;
}

}  // namespace

int main() {
  state = 2026u;
  for (int64_t n : {1, 63, 64, 65, 300})
    for (int64_t dim : {1, 2, 33}) {
      const std::vector<float> rows = rows_of(n, dim, 3), q = rows_of(70, dim, 3);
      for (float r2 : {0.f, 1.f, 2.f, 5.5f, INFINITY}) run(rows, n, dim, q, 70, nullptr, nullptr, nullptr, 0, r2);
      // the self-join: every unordered pair once with upper, twice without
      std::vector<int32_t> qpos((size_t)n);
      for (int64_t i = 0; i < n; ++i) qpos[(size_t)i] = (int32_t)i;
      for (float r2 : {0.f, 2.f}) {
        const Result up = run(rows, n, dim, rows, n, nullptr, nullptr, qpos.data(), 1, r2), all = run(rows, n, dim, rows, n, nullptr, nullptr, qpos.data(), 0, r2);
        EXPECT(2 * up.total == all.total);
      }
    }
  {  // ids: rows of the query's id are skipped; non-finite rows and queries; an empty table
    std::vector<float> rows = rows_of(200, 3, 4), q = rows_of(40, 3, 4);
    std::vector<int64_t> ids(200), qid(40);
    for (int i = 0; i < 200; ++i) ids[(size_t)i] = i / 50;
    for (int i = 0; i < 40; ++i) qid[(size_t)i] = i % 5;
    run(rows, 200, 3, q, 40, ids.data(), qid.data(), nullptr, 0, 3.f);
    run(rows, 200, 3, q, 40, nullptr, qid.data(), nullptr, 0, 3.f);
    rows[0] = NAN, rows[3 * 70 + 1] = INFINITY, rows[3 * 199 + 2] = -INFINITY, q[4] = NAN, q[3 * 9] = INFINITY;
    run(rows, 200, 3, q, 40, nullptr, nullptr, nullptr, 0, 3.f);
    const Result inf = run(rows, 200, 3, q, 40, nullptr, nullptr, nullptr, 0, INFINITY);
    // a finite query: the NaN row is out, the two infinite rows are +inf away and qualify; the query with a NaN has no hit; the one with
    // an infinite component is +inf away from every row but the NaN one
    EXPECT(inf.counts[0] == 199 && inf.counts[1] == 0 && inf.counts[9] == 199);
    const Result none = run(rows, 0, 3, q, 40, nullptr, nullptr, nullptr, 0, INFINITY);
    EXPECT(none.total == 0);
  }
  {  // within_finish on scrambled records: the order of arrival is not part of the result
    const int64_t nq = 37, total = 5000;
    std::vector<int32_t> rq((size_t)total), rp((size_t)total);
    std::vector<float> rd((size_t)total);
    std::vector<int64_t> first((size_t)nq + 1, 0);
    for (int64_t i = 0; i < total; ++i) {
      rq[(size_t)i] = (int32_t)(draw() % nq);
      if (rq[(size_t)i] == 5) rq[(size_t)i] = 6;                      // query 5 has no hit, query 6 twice its share
      rp[(size_t)i] = (int32_t)i;                                     // unique positions
      rd[(size_t)i] = (float)(draw() % 7);                            // many ties
      ++first[(size_t)rq[(size_t)i] + 1];
    }
    for (int64_t i = 0; i < nq; ++i) first[(size_t)i + 1] += first[(size_t)i];
    std::vector<float> d1((size_t)total), d2((size_t)total);
    std::vector<int32_t> p1((size_t)total), p2((size_t)total);
    scann::within_finish(first.data(), nq, rq.data(), rp.data(), rd.data(), total, d1.data(), p1.data());
    for (int64_t i = total - 1; i > 0; --i) {
      const int64_t j = draw() % (i + 1);
      std::swap(rq[(size_t)i], rq[(size_t)j]); std::swap(rp[(size_t)i], rp[(size_t)j]); std::swap(rd[(size_t)i], rd[(size_t)j]);
    }
    scann::within_finish(first.data(), nq, rq.data(), rp.data(), rd.data(), total, d2.data(), p2.data());
    EXPECT(d1 == d2 && p1 == p2);
    for (int64_t i = 0; i < nq; ++i)
      for (int64_t j = first[(size_t)i] + 1; j < first[(size_t)i + 1]; ++j)
        EXPECT(d1[(size_t)j - 1] < d1[(size_t)j] || (d1[(size_t)j - 1] == d1[(size_t)j] && p1[(size_t)j - 1] < p1[(size_t)j]));
    scann::within_finish(first.data(), nq, rq.data(), rp.data(), rd.data(), total, nullptr, p2.data());  // one output only
    EXPECT(p1 == p2);
  }
  const std::vector<float> r = rows_of(10, 2, 3);
  int64_t c[10], tot;
  float d[4];
  int32_t p[10] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 0, NAN, 0, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 0, -1.f, 0, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 0, 1.f, -1, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 0, 1.f, ((int64_t)1 << 30) + 1, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 0, 1.f, 0, c, &tot, d, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 1, 1.f, 0, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, p, 2, 1.f, 0, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, nullptr, 10, nullptr, nullptr, 0, 1.f, 0, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 0, nullptr, nullptr, 0, 1.f, 0, c, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, nullptr, 0, 1.f, 0, nullptr, &tot, nullptr, nullptr) == SCANN_ERR_INVALID);
  EXPECT(scann_within_host(r.data(), 10, 2, nullptr, r.data(), 10, nullptr, p, 1, 0.f, 0, c, &tot, nullptr, nullptr) == SCANN_OK);
  return finish("scann_within_check");
}

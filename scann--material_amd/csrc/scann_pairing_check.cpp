// Stand-alone driver of the pairing's host twins (scann_pairing_host, scann_pairing_solve_host) for the sanitizers: `make asan-pairing`
// compiles it with scann_pairing.cpp under AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  It walks the
// twins' paths -- the solver against all permutations for Q <= 7, all-equal, 0/1 and 2^31 matrices, Q = 1, 64 and 128; pairs with n or m
// 1 and 128, dim 1, 3 and 130, a permuted copy, the counting example of the header, Dmax = 0, subnormal and huge distances, overflow,
// a NaN row, a segment above the limit, the refusals -- and checks the symmetry of the score bit for bit and the integer exponent
// against ilogbf.
#include "scann_pairing.cpp"

#include "scann_check.h"

// the stubs of its own
namespace scann {
int read_mol_offset(scann_handle_t*, const scann_dbatch_t*, std::vector<int32_t>&) { return SCANN_ERR_INVALID; }
int match_staged(scann_handle*, scann_index*, const float*, hipMemcpyKind, const int32_t*, int64_t, const int64_t*, int, int, hipStream_t, float*,
                 int32_t*, int64_t*, int32_t*, float*, int32_t*, float*) { return SCANN_ERR_INVALID; }
size_t pairing_lds_bytes(int) { return 0; }
hipError_t launch_pairing(const PairingArgs&, const int32_t*, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

// the least sum over all permutations
long long brute(const std::vector<uint32_t>& C, int Q) {
  std::vector<int> pi((size_t)Q);
  for (int i = 0; i < Q; ++i) pi[(size_t)i] = i;
  long long best = -1;
  do {
    long long s = 0;
    for (int i = 0; i < Q; ++i) s += C[(size_t)(i * Q + pi[(size_t)i])];
    if (best < 0 || s < best) best = s;
  } while (std::next_permutation(pi.begin(), pi.end()));
  return best;
}

void check_solver(const std::vector<uint32_t>& C, int Q, bool identity) {
  std::vector<int32_t> col((size_t)Q, -7);
  int64_t total = -7;
  EXPECT(scann_pairing_solve_host(C.data(), Q, col.data(), &total) == SCANN_OK);
  std::vector<char> seen((size_t)Q, 0);
  long long s = 0;
  for (int i = 0; i < Q; ++i) {
    EXPECT(col[(size_t)i] >= 0 && col[(size_t)i] < Q && !seen[(size_t)col[(size_t)i]]);
    if (col[(size_t)i] < 0 || col[(size_t)i] >= Q) return;
    seen[(size_t)col[(size_t)i]] = 1;
    s += C[(size_t)(i * Q + col[(size_t)i])];
    if (identity) EXPECT(col[(size_t)i] == i);
  }
  EXPECT(s == total);
  if (Q <= 7) EXPECT(brute(C, Q) == total);
}

struct Pair {
  float score;
  int64_t total;
  int32_t shift;
  std::vector<int32_t> partner;
  std::vector<float> pd;
};
Pair run(const std::vector<float>& a, int64_t n, const std::vector<float>& b, int64_t m, int64_t dim, int expect = SCANN_OK) {
  Pair r{7.f, 7, 7, std::vector<int32_t>((size_t)n, 7), std::vector<float>((size_t)n, 7.f)};
  EXPECT(scann_pairing_host(a.data(), n, b.data(), m, dim, &r.score, &r.total, &r.shift, r.partner.data(), r.pd.data()) == expect);
  return r;
}
bool is_tail(const Pair& r) {
  bool ok = std::isinf(r.score) && r.score > 0 && r.total == -1 && r.shift == 0;
  for (size_t i = 0; i < r.partner.size(); ++i) ok = ok && r.partner[i] == -1 && std::isinf(r.pd[i]);
  return ok;
}
std::vector<float> rows_of(int64_t n, int64_t dim, float scale, bool integer) {
  std::vector<float> x((size_t)(n * dim));
  for (auto& v : x) v = integer ? (float)(draw() % 3) * scale : ((float)(draw() % 20001) / 10000.f - 1.f) * scale;
  return x;
}

}  // namespace

int main() {
  state = 2024u;
  // the integer exponent against ilogbf
  for (float x : {1.f, 1.5f, 2.f, 0.75f, 1e-38f, 1e-40f, 1.4e-45f, 3e38f, 1.17549435e-38f, 5.877e-39f}) EXPECT(pairing_ilogb(bits_of(x)) == std::ilogb(x));
  EXPECT(pairing_shift(bits_of(0.f)) == 0 && pairing_shift(bits_of(1.f)) == 30 && pairing_shift(bits_of(1.4e-45f)) == 179 && pairing_shift(bits_of(3.4e38f)) == -97);
  // the solver
  for (int Q : {1, 2, 3, 7, 64, 128}) {
    std::vector<uint32_t> C((size_t)(Q * Q));
    for (int rep = 0; rep < (Q <= 7 ? 20 : 2); ++rep) {
      for (auto& c : C) c = draw() % 1000u;
      check_solver(C, Q, false);
      for (auto& c : C) c = draw() % 2u;
      check_solver(C, Q, false);
      for (auto& c : C) c = (draw() % 4u) ? 0x80000000u : draw();
      check_solver(C, Q, false);
    }
    std::fill(C.begin(), C.end(), 5u);
    check_solver(C, Q, true);  // every permutation attains it: the tie rule gives the identity
    std::fill(C.begin(), C.end(), 0x80000000u);
    check_solver(C, Q, true);
  }
  {
    std::vector<uint32_t> C{1, 2, 3, 0x80000001u};
    int64_t total;
    EXPECT(scann_pairing_solve_host(C.data(), 2, nullptr, &total) == SCANN_ERR_INVALID);
    EXPECT(scann_pairing_solve_host(nullptr, 2, nullptr, &total) == SCANN_ERR_INVALID);
    EXPECT(scann_pairing_solve_host(C.data(), 0, nullptr, &total) == SCANN_ERR_INVALID);
    C[3] = 4;
    EXPECT(scann_pairing_solve_host(C.data(), 2, nullptr, nullptr) == SCANN_OK);
  }
  // pairs
  for (int64_t dim : {1, 3, 130})
    for (int64_t n : {1, 2, 17, 128})
      for (int64_t m : {1, 5, 17, 128}) {
        for (int integer = 0; integer < 2; ++integer) {
          const std::vector<float> a = rows_of(n, dim, 1.f, integer), b = rows_of(m, dim, 1.f, integer);
          const Pair ab = run(a, n, b, m, dim), ba = run(b, m, a, n, dim);
          EXPECT(bits_of(ab.score) == bits_of(ba.score) && ab.total == ba.total && ab.shift == ba.shift && ab.total >= 0);
          int64_t surplus = 0;
          std::vector<char> seen((size_t)m, 0);
          for (int64_t i = 0; i < n; ++i) {
            if (ab.partner[(size_t)i] < 0) { ++surplus; continue; }
            EXPECT(ab.partner[(size_t)i] < m && !seen[(size_t)ab.partner[(size_t)i]]);
            seen[(size_t)ab.partner[(size_t)i]] = 1;
            EXPECT(bits_of(ab.pd[(size_t)i]) == bits_of(chain(&a[(size_t)(i * dim)], &b[(size_t)(ab.partner[(size_t)i] * dim)], dim)));
          }
          EXPECT(surplus == (n > m ? n - m : 0));
        }
      }
  {  // a permuted copy scores 0 and returns the inverse permutation
    const int64_t n = 23, dim = 3;
    const std::vector<float> a = rows_of(n, dim, 1.f, false);
    std::vector<float> b((size_t)(n * dim));
    for (int64_t i = 0; i < n; ++i) std::copy(a.begin() + i * dim, a.begin() + (i + 1) * dim, b.begin() + ((i * 7 + 3) % n) * dim);
    const Pair r = run(a, n, b, n, dim);
    EXPECT(r.score == 0.f && r.total == 0);
    for (int64_t i = 0; i < n; ++i) EXPECT(r.partner[(size_t)i] == (i * 7 + 3) % n && r.pd[(size_t)i] == 0.f);
  }
  {  // {3 x a, 3 x b} against {5 x a, 1 x b}: chamfer 0, but two b rows must take an a, |a - b|^2 = 8 each: 16 / 6
    const std::vector<float> a{0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2}, b{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2};
    const Pair r = run(a, 6, b, 6, 2);
    EXPECT(r.shift == 27 && r.total == (16ll << 27) && bits_of(r.score) == bits_of((float)(8.0 / 3.0)));
  }
  {  // Dmax = 0
    const std::vector<float> a(12, 1.5f);
    const Pair r = run(a, 4, a, 3, 3);
    EXPECT(r.score == 0.f && r.total == 0 && r.shift == 0 && r.partner[0] == 0 && r.partner[1] == 1 && r.partner[2] == 2 && r.partner[3] == -1 && r.pd[3] == 0.f);
  }
  for (float scale : {1e-22f, 1e18f}) {  // subnormal distances, and distances near the top of the range
    const std::vector<float> a = rows_of(9, 3, scale, false), b = rows_of(11, 3, scale, false);
    const Pair ab = run(a, 9, b, 11, 3), ba = run(b, 11, a, 9, 3);
    EXPECT(ab.total > 0 && ab.total < (1ll << 38) && std::isfinite(ab.score) && ab.score > 0 && bits_of(ab.score) == bits_of(ba.score));
    EXPECT(scale < 1.f ? ab.shift > 149 : ab.shift < -60);
  }
  {  // rows at 1e20: the distances overflow; a NaN row; a segment above the limit
    std::vector<float> a = rows_of(5, 3, 1.f, false), b = rows_of(6, 3, 1.f, false);
    a[0] = 1e20f, b[0] = -1e20f;
    EXPECT(is_tail(run(a, 5, b, 6, 3)));
    a[0] = NAN, b[0] = 0.f;
    EXPECT(is_tail(run(a, 5, b, 6, 3)) && is_tail(run(b, 6, a, 5, 3)));
    const std::vector<float> big = rows_of(129, 3, 1.f, false);
    EXPECT(is_tail(run(b, 6, big, 129, 3)));
    run(big, 129, b, 6, 3, SCANN_ERR_UNSUPPORTED);
    run(b, 0, b, 6, 3, SCANN_ERR_INVALID);
    run(b, 6, b, 0, 3, SCANN_ERR_INVALID);
    run(b, 6, b, 6, 0, SCANN_ERR_INVALID);
    EXPECT(scann_pairing_host(nullptr, 1, b.data(), 1, 3, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_ERR_INVALID);
    EXPECT(scann_pairing_host(b.data(), 2, b.data(), 2, 3, nullptr, nullptr, nullptr, nullptr, nullptr) == SCANN_OK);
  }
  return finish("scann_pairing_check");
}

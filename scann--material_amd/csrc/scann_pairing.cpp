// One-to-one atom maps between structures, the host half (include/scann_hip.h; scann_pairing.hip): scann_index_pairing around
// pairing_kernel, scann_index_pairing_batch -- one forward, the shortlist of scann_index_match (match_staged), the pairing, the rerank --
// and the twins scann_pairing_host / scann_pairing_solve_host, which restate the definition with no GPU work.  Every floating-point
// expression here is evaluated as written: the file is compiled with floating-point contraction off.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <numeric>

#include "scann_call.h"
#include "scann_knn.h"
#include "scann_match.h"
#include "scann_pairing.h"
#include "scann_runtime.h"

using namespace scann;

namespace {

static_assert(PAIRING_MAX == SCANN_PAIRING_MAX_ATOMS && pairing_class_q(PAIRING_CLASSES - 1) == PAIRING_MAX, "the header's constant");

// the chain of scann_knn_distsq, q first
inline float chain(const float* q, const float* r, int64_t d) {
  float acc = 0.f;
  for (int64_t j = 0; j < d; ++j) {
    const float t = q[j] - r[j];
    acc = std::fmaf(t, t, acc);
  }
  return acc;
}

// The procedure of the definition on the cost matrix C [Q][ld]: p[j] = the row paired with column j; returns the optimum
long long solve(const uint32_t* C, int Q, int ld, int32_t* p) {
  std::vector<long long> u((size_t)Q, 0), v((size_t)Q, 0), minv((size_t)Q);
  std::vector<int32_t> way((size_t)Q);
  std::vector<char> used((size_t)Q);
  std::fill(p, p + Q, -1);
  for (int i = 0; i < Q; ++i) {
    std::fill(minv.begin(), minv.end(), PAIRING_INF);
    std::fill(used.begin(), used.end(), 0);
    std::fill(way.begin(), way.end(), -1);
    int j0 = -1;
    for (;;) {
      if (j0 >= 0) used[(size_t)j0] = 1;
      const int i0 = j0 < 0 ? i : p[j0];
      long long delta = PAIRING_INF;
      int j1 = -1;
      for (int j = 0; j < Q; ++j) {
        if (used[(size_t)j]) continue;
        const long long cur = (long long)C[(size_t)i0 * ld + j] - u[(size_t)i0] - v[(size_t)j];
        if (cur < minv[(size_t)j]) minv[(size_t)j] = cur, way[(size_t)j] = j0;
        if (minv[(size_t)j] < delta) delta = minv[(size_t)j], j1 = j;  // strict: the least column wins a tie
      }
      u[(size_t)i] += delta;
      for (int j = 0; j < Q; ++j) {
        if (used[(size_t)j]) u[(size_t)p[j]] += delta, v[(size_t)j] -= delta;
        else minv[(size_t)j] -= delta;
      }
      j0 = j1;
      if (p[j0] < 0) break;
    }
    for (; j0 >= 0; j0 = way[(size_t)j0]) p[j0] = way[(size_t)j0] < 0 ? i : p[way[(size_t)j0]];
  }
  long long total = 0;
  for (int j = 0; j < Q; ++j) total += C[(size_t)p[j] * ld + j];
  return total;
}

// what a pair that is not comparable answers
void not_comparable(int64_t n, float* score, int64_t* total, int32_t* shift, int32_t* partner, float* pd) {
  if (score) *score = __builtin_inff();
  if (total) *total = -1;
  if (shift) *shift = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (partner) partner[i] = -1;
    if (pd) pd[i] = __builtin_inff();
  }
}

// the definition for one pair: a [n][dim], b [m][dim], 1 <= n <= PAIRING_MAX, m >= 1; partner: index within b
void pair_twin(const float* a, int64_t n, const float* b, int64_t m, int64_t dim, float* score, int64_t* total, int32_t* shift, int32_t* partner,
               float* pd) {
  if (m > PAIRING_MAX) return not_comparable(n, score, total, shift, partner, pd);
  std::vector<float> D((size_t)(n * m));
  float dmax = 0.f;
  bool bad = false;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < m; ++j) {
      const float d = chain(a + i * dim, b + j * dim, dim);
      D[(size_t)(i * m + j)] = d;
      bad |= !(d < __builtin_inff());
      if (d > dmax) dmax = d;
    }
  if (bad) return not_comparable(n, score, total, shift, partner, pd);
  uint32_t bits;
  std::memcpy(&bits, &dmax, 4);
  const int sh = pairing_shift(bits), Q = (int)std::max(n, m);
  std::vector<uint32_t> C((size_t)Q * Q);
  for (int64_t i = 0; i < n; ++i) {
    uint32_t tmin = 0xffffffffu;
    for (int64_t j = 0; j < m; ++j) tmin = std::min(tmin, C[(size_t)(i * Q + j)] = pairing_quant(D[(size_t)(i * m + j)], sh));
    for (int64_t j = m; j < Q; ++j) C[(size_t)(i * Q + j)] = tmin;
  }
  for (int64_t j = 0; j < m && n < m; ++j) {
    uint32_t tmin = 0xffffffffu;
    for (int64_t i = 0; i < n; ++i) tmin = std::min(tmin, C[(size_t)(i * Q + j)]);
    for (int64_t i = n; i < Q; ++i) C[(size_t)(i * Q + j)] = tmin;
  }
  std::vector<int32_t> p((size_t)Q);
  const long long t = solve(C.data(), Q, Q, p.data());
  if (score) *score = pairing_score(t, sh, Q);
  if (total) *total = t;
  if (shift) *shift = sh;
  for (int j = 0; j < Q; ++j) {
    const int64_t i = p[(size_t)j];
    if (i >= n) continue;
    if (partner) partner[i] = j < m ? j : -1;
    if (pd) pd[i] = j < m ? D[(size_t)(i * m + j)] : *std::min_element(D.begin() + i * m, D.begin() + (i + 1) * m);
  }
}

// q_first [n_sets + 1] of a pairing: starts at 0, every set holds 1 .. SCANN_PAIRING_MAX_ATOMS rows
int check_pairing_sets(scann_handle* h, const int32_t* q_first, int64_t n_sets, const char* who) {
  if (n_sets <= 0 || !q_first) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": an empty query");
  if (n_sets > (int64_t)0x7fffffff / SCANN_KNN_MAX_K / 4) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": too many query structures in one call");
  if (q_first[0] != 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": q_first[0] is " + std::to_string(q_first[0]) + ", not 0");
  for (int64_t s = 0; s < n_sets; ++s) {
    const int64_t n = (int64_t)q_first[s + 1] - q_first[s];
    if (n < 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": q_first decreases at query structure " + std::to_string(s));
    if (n == 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": query structure " + std::to_string(s) + " is an empty set");
    if (n > SCANN_PAIRING_MAX_ATOMS)
      return fail(h, SCANN_ERR_UNSUPPORTED, std::string(who) + ": query structure " + std::to_string(s) + " has " + std::to_string(n) +
                                                " atoms, more than SCANN_PAIRING_MAX_ATOMS = " + std::to_string(SCANN_PAIRING_MAX_ATOMS));
  }
  if ((int64_t)q_first[n_sets] > (int64_t)0x7fffffff / SCANN_KNN_MAX_K) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": too many query rows in one call");
  return SCANN_OK;
}

// The pairs (pair_set[e], pair_seg[e]) -- checked: sets of q_first, segments of ix -- with the query rows on the device (dq
// [q_first[n_sets]][stride], padded like the index's rows).  Host outputs, none null: score, total, shift [n_pairs]; ppos, pd in pair
// order, pair e owning n(pair_set[e]) places.  Synchronous.
int pairing_search(scann_handle* h, scann_index* ix, const float* dq, const int32_t* q_first, const int32_t* pair_set, const int32_t* pair_seg,
                   int64_t n_pairs, hipStream_t s, float* score, int64_t* total, int32_t* shift, int32_t* ppos, float* pd) {
  if (n_pairs <= 0) return SCANN_OK;
  const int64_t n_seg = (int64_t)ix->seg_first.size();
  auto seg_end = [&](int64_t g) { return g + 1 < n_seg ? (int64_t)ix->seg_first[(size_t)(g + 1)] : ix->n; };
  // the pairs by class: -1 (the segment is too long: not comparable, answered here), Q <= 32, <= 64, <= 128
  std::vector<PairingDesc> all((size_t)n_pairs), desc;
  std::vector<int8_t> cls((size_t)n_pairs);
  int32_t count[PAIRING_CLASSES] = {0, 0, 0};
  int64_t at = 0;
  for (int64_t e = 0; e < n_pairs; ++e) {
    const int32_t st = pair_set[e], g = pair_seg[e];
    PairingDesc& d = all[(size_t)e];
    d.q0 = q_first[st];
    d.n = q_first[st + 1] - q_first[st];
    d.first = ix->seg_first[(size_t)g];
    d.m = (int32_t)std::min<int64_t>(seg_end(g) - d.first, 0x7fffffff);
    d.out0 = (int32_t)at;
    d.pair = (int32_t)e;
    at += d.n;
    const int Q = std::max(d.n, d.m);
    cls[(size_t)e] = Q > PAIRING_MAX ? -1 : Q <= pairing_class_q(0) ? 0 : Q <= pairing_class_q(1) ? 1 : 2;
    if (cls[(size_t)e] >= 0) ++count[cls[(size_t)e]];
  }
  const int64_t n_launch = (int64_t)count[0] + count[1] + count[2], n_out = at;
  if (n_launch > 0) {
    desc.resize((size_t)n_launch);
    int64_t next[PAIRING_CLASSES] = {0, count[0], (int64_t)count[0] + count[1]};
    for (int64_t e = 0; e < n_pairs; ++e)
      if (cls[(size_t)e] >= 0) desc[(size_t)next[cls[(size_t)e]]++] = all[(size_t)e];
    const int n_chunk = (int)ix->chunks.size();
    PairingArgs a{};
    CallWs ws;
    ws.take(a.rows, (size_t)std::max(n_chunk, 1)); ws.take(a.desc, (size_t)n_launch); ws.take(a.score, (size_t)n_pairs);
    ws.take(a.total, (size_t)n_pairs); ws.take(a.shift, (size_t)n_pairs); ws.take(a.partner_pos, (size_t)n_out); ws.take(a.partner_d, (size_t)n_out);
    HIPCHK(h, ws.alloc());
    a.chunk_rows = ix->chunk_rows; a.stride = ix->stride; a.q = dq;
    hipError_t e = ws.upload_rows(ix, n_chunk, a.rows, (const int64_t* const*)nullptr, s);
    if (e == hipSuccess) e = hipMemcpyAsync(writable(a.desc), desc.data(), (size_t)n_launch * sizeof(PairingDesc), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_pairing(a, count, s);
    if (e == hipSuccess) e = hipMemcpyAsync(score, a.score, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(total, a.total, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(shift, a.shift, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ppos, a.partner_pos, (size_t)n_out * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pd, a.partner_d, (size_t)n_out * 4, hipMemcpyDeviceToHost, s);
    const hipError_t e_sync = hipStreamSynchronize(s);
    ws.release();
    HIPCHK(h, e);
    HIPCHK(h, e_sync);
  }
  for (int64_t e = 0; e < n_pairs; ++e)  // (the kernel wrote nothing there)
    if (cls[(size_t)e] < 0) {
      const PairingDesc& d = all[(size_t)e];
      not_comparable(d.n, score + e, total + e, shift + e, ppos + d.out0, pd + d.out0);
    }
  return SCANN_OK;
}

// as match_staged: host or device query rows of the index's width staged at the padded width, then paired
int pairing_staged(scann_handle* h, scann_index* ix, const float* q, hipMemcpyKind kind, const int32_t* q_first, int64_t n_sets, const int32_t* pair_set,
                   const int32_t* pair_seg, int64_t n_pairs, hipStream_t s, float* score, int64_t* total, int32_t* shift, int32_t* ppos, float* pd) {
  if (n_pairs <= 0) return SCANN_OK;
  CallWs ws;
  RowStage st;
  st.take(ws, q_first[n_sets], ix->dim, ix->dim, ix->stride, kind);
  HIPCHK(h, ws.alloc());
  const hipError_t e = st.stage_rows(q, s);
  int r = SCANN_OK;
  if (e == hipSuccess)
    r = pairing_search(h, ix, st.rows(q), q_first, pair_set, pair_seg, n_pairs, s, score, total, shift, ppos, pd);
  else
    (void)hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  return r;
}

}  // namespace

extern "C" {

int scann_index_pairing(scann_handle_t* h, scann_index_t* ix, const float* q, const int32_t* q_first, int64_t n_sets, const int32_t* pair_set,
                        const int32_t* pair_segment, int64_t n_pairs, float* score, int64_t* total, int32_t* shift, int32_t* partner_pos,
                        float* partner_dist2) {
  const char* who = "scann_index_pairing";
  if (const int r = check_index(h, ix, who)) return r;
  if (!q) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": an empty query");
  if (const int r = check_pairing_sets(h, q_first, n_sets, who)) return r;
  if (n_pairs < 0 || n_pairs > (int64_t)0x7fffffff / SCANN_PAIRING_MAX_ATOMS)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": n_pairs " + std::to_string(n_pairs) + " outside 0 .. " +
                                          std::to_string(0x7fffffff / SCANN_PAIRING_MAX_ATOMS));
  if (n_pairs == 0) return SCANN_OK;
  if (!pair_set) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": pair_set is null");
  if (!pair_segment) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": pair_segment is null");
  if (!score) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": score is null");
  const int64_t n_seg = (int64_t)ix->seg_first.size();
  int64_t n_out = 0;
  for (int64_t e = 0; e < n_pairs; ++e) {
    if (pair_set[e] < 0 || pair_set[e] >= n_sets)
      return fail(h, SCANN_ERR_INVALID, std::string(who) + ": pair_set[" + std::to_string(e) + "] is " + std::to_string(pair_set[e]) + ", outside the " +
                                            std::to_string(n_sets) + " query structures");
    if (pair_segment[e] < 0 || pair_segment[e] >= n_seg)
      return fail(h, SCANN_ERR_INVALID, std::string(who) + ": pair_segment[" + std::to_string(e) + "] is " + std::to_string(pair_segment[e]) +
                                            ", outside the " + std::to_string(n_seg) + " segments of the index");
    n_out += q_first[pair_set[e] + 1] - q_first[pair_set[e]];
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int64_t> t_tmp(total ? 0 : (size_t)n_pairs);
  std::vector<int32_t> s_tmp(shift ? 0 : (size_t)n_pairs), p_tmp(partner_pos ? 0 : (size_t)n_out);
  std::vector<float> d_tmp(partner_dist2 ? 0 : (size_t)n_out);
  return pairing_staged(h, ix, q, hipMemcpyHostToDevice, q_first, n_sets, pair_set, pair_segment, n_pairs, h->streams[0], score,
                        total ? total : t_tmp.data(), shift ? shift : s_tmp.data(), partner_pos ? partner_pos : p_tmp.data(),
                        partner_dist2 ? partner_dist2 : d_tmp.data());
}

int scann_index_pairing_batch(scann_handle_t* h, scann_index_t* ix, scann_dbatch_t* db, const int64_t* query_ids, int32_t measure, int32_t shortlist,
                              int32_t k, float* y, float* ga, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, int64_t* total,
                              int32_t* shift, float* short_score, int32_t* short_place, int32_t* partner_pos, float* partner_dist2) {
  const char* who = "scann_index_pairing_batch";
  if (const int r = check_index(h, ix, who)) return r;
  if (const int r = check_k(h, k, who)) return r;
  if (shortlist < k || shortlist > SCANN_KNN_MAX_K)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": shortlist " + std::to_string(shortlist) + " outside k = " + std::to_string(k) + " .. " +
                                          std::to_string(SCANN_KNN_MAX_K));
  if (measure < SCANN_MATCH_CHAMFER || measure > SCANN_MATCH_COVER)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": measure " + std::to_string(measure) +
                                          " is none of SCANN_MATCH_CHAMFER (0), SCANN_MATCH_HAUSDORFF (1), SCANN_MATCH_COVER (2)");
  if (!score) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": score is null");
  if (!db) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": null argument");
  if (const int r = check_level(h, ix, SCANN_OUT_AFTER_LC, who)) return r;
  if (db->n_struct <= 0 || db->n_atom <= 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": an empty query");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, std::string(who) + ": weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> mol;
  if (const int r = read_mol_offset(h, db, mol)) return r;
  const int64_t n_sets = db->n_struct, S = shortlist;
  if (const int r = check_pairing_sets(h, mol.data(), n_sets, who)) return r;
  if (const int r = forward_and_download(h, db, 0, SCANN_OUT_AFTER_LC, y, ga)) return r;
  hipStream_t s = h->streams[db->last_slot];
  // the shortlist: the answer of scann_index_match with k = shortlist on the batch's after_Lc rows, where the forward left them
  std::vector<float> sl_score((size_t)(n_sets * S));
  std::vector<int32_t> sl_seg((size_t)(n_sets * S));
  if (const int r = match_staged(h, ix, db->out_z, hipMemcpyDeviceToDevice, mol.data(), n_sets, query_ids, measure, shortlist, s, sl_score.data(),
                                 sl_seg.data(), nullptr, nullptr, nullptr, nullptr, nullptr))
    return r;
  // its pairs, set by set and place by place
  std::vector<int32_t> pset, pseg, place;
  std::vector<int64_t> out0;
  int64_t n_out = 0;
  for (int64_t st = 0; st < n_sets; ++st)
    for (int64_t p = 0; p < S && sl_seg[(size_t)(st * S + p)] >= 0; ++p) {
      pset.push_back((int32_t)st);
      pseg.push_back(sl_seg[(size_t)(st * S + p)]);
      place.push_back((int32_t)p);
      out0.push_back(n_out);
      n_out += mol[(size_t)st + 1] - mol[(size_t)st];
    }
  const int64_t n_pairs = (int64_t)pset.size();
  std::vector<float> p_score((size_t)n_pairs), p_d((size_t)n_out);
  std::vector<int64_t> p_total((size_t)n_pairs);
  std::vector<int32_t> p_shift((size_t)n_pairs), p_pos((size_t)n_out);
  if (const int r = pairing_staged(h, ix, db->out_z, hipMemcpyDeviceToDevice, mol.data(), n_sets, pset.data(), pseg.data(), n_pairs, s, p_score.data(),
                                   p_total.data(), p_shift.data(), p_pos.data(), p_d.data()))
    return r;
  // the rerank: the first k shortlisted segments under (pairing score, segment number); the other places hold the tail
  const float inf = __builtin_inff();
  const int64_t n_seg = (int64_t)ix->seg_first.size();
  std::vector<int64_t> order;
  for (int64_t st = 0, e0 = 0; st < n_sets; ++st) {
    int64_t e1 = e0;
    while (e1 < n_pairs && pset[(size_t)e1] == st) ++e1;
    order.resize((size_t)(e1 - e0));
    std::iota(order.begin(), order.end(), e0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t z) {
      return p_score[(size_t)x] < p_score[(size_t)z] || (p_score[(size_t)x] == p_score[(size_t)z] && pseg[(size_t)x] < pseg[(size_t)z]);
    });
    const int64_t r0 = mol[(size_t)st], r1 = mol[(size_t)st + 1];
    for (int64_t p = 0; p < k; ++p) {
      const int64_t o = st * k + p, e = p < (int64_t)order.size() ? order[(size_t)p] : -1;
      const int64_t g = e < 0 ? -1 : pseg[(size_t)e], first = g < 0 ? 0 : ix->seg_first[(size_t)g];
      score[o] = e < 0 ? inf : p_score[(size_t)e];
      if (segment) segment[o] = (int32_t)g;
      if (ids) ids[o] = g < 0 ? -1 : ix->ids[(size_t)first];
      if (sizes) sizes[o] = g < 0 ? 0 : (int32_t)((g + 1 < n_seg ? (int64_t)ix->seg_first[(size_t)(g + 1)] : ix->n) - first);
      if (total) total[o] = e < 0 ? -1 : p_total[(size_t)e];
      if (shift) shift[o] = e < 0 ? 0 : p_shift[(size_t)e];
      if (short_score) short_score[o] = e < 0 ? inf : sl_score[(size_t)(st * S + place[(size_t)e])];
      if (short_place) short_place[o] = e < 0 ? -1 : place[(size_t)e];
      for (int64_t r = r0; r < r1; ++r) {
        if (partner_pos) partner_pos[r * k + p] = e < 0 ? -1 : p_pos[(size_t)(out0[(size_t)e] + r - r0)];
        if (partner_dist2) partner_dist2[r * k + p] = e < 0 ? inf : p_d[(size_t)(out0[(size_t)e] + r - r0)];
      }
    }
    e0 = e1;
  }
  return SCANN_OK;
}

int scann_pairing_host(const float* a, int64_t n, const float* b, int64_t m, int64_t dim, float* score, int64_t* total, int32_t* shift, int32_t* partner,
                       float* partner_dist2) {
  if (!a || !b || n < 1 || m < 1 || dim < 1) return SCANN_ERR_INVALID;
  if (n > SCANN_PAIRING_MAX_ATOMS) return SCANN_ERR_UNSUPPORTED;
  pair_twin(a, n, b, m, dim, score, total, shift, partner, partner_dist2);
  return SCANN_OK;
}

int scann_pairing_solve_host(const uint32_t* cost, int32_t Q, int32_t* col_of_row, int64_t* total) {
  if (!cost || Q < 1 || Q > SCANN_PAIRING_SOLVE_MAX) return SCANN_ERR_INVALID;
  for (int64_t e = 0; e < (int64_t)Q * Q; ++e)
    if (cost[e] > 0x80000000u) return SCANN_ERR_INVALID;
  std::vector<int32_t> p((size_t)Q);
  const long long t = solve(cost, Q, Q, p.data());
  if (total) *total = t;
  for (int j = 0; j < Q && col_of_row; ++j) col_of_row[p[(size_t)j]] = j;
  return SCANN_OK;
}

}  // extern "C"

// The radius search over a latent-space index, the host half (include/scann_hip.h: scann_index_within): the checks, the passes of
// within_tile_kernel without a partition and through the survivor lists of a partition (scann_cells.hip: the centre distances, the order
// of the queries and plan pass 2), the size-then-fill protocol, and the order of the result.  The kernel leaves exact counts and, where
// they fit, one record per hit in the order of arrival; within_finish puts the records into their queries' segments and sorts each by
// (dist2, position), so the bytes of the result depend on the query, the index and radius2 only.  scann_within_host is the twin: the
// same chain on the host, the same within_finish.
#include "scann_within.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <thread>
#include <utility>

#include "scann_call.h"
#include "scann_runtime.h"
#include "scann_search.h"

using namespace scann;

namespace {

// f(block, begin, end) over n items cut into at most 16 contiguous blocks, one thread each
template <class F>
void in_blocks(int64_t n, int64_t min_per_thread, F f) {
  const int64_t hw = (int64_t)std::thread::hardware_concurrency();
  const int64_t nt = std::max<int64_t>(1, std::min<int64_t>({16, hw > 0 ? hw : 1, n / std::max<int64_t>(min_per_thread, 1)}));
  if (nt == 1) {
    f(0, (int64_t)0, n);
    return;
  }
  std::vector<std::thread> pool;
  for (int64_t b = 0; b < nt; ++b) pool.emplace_back([=] { f((int)b, n * b / nt, n * (b + 1) / nt); });
  for (auto& th : pool) th.join();
}

}  // namespace

void scann::within_finish(const int64_t* first, int64_t nq, const int32_t* rec_q, const int32_t* rec_p, const float* rec_d, int64_t total, float* dist2,
                          int32_t* pos) {
  if (total <= 0 || (!dist2 && !pos)) return;
  std::vector<std::pair<float, int32_t>> seg((size_t)total);
  std::vector<int64_t> at(first, first + nq);
  for (int64_t i = 0; i < total; ++i) seg[(size_t)at[(size_t)rec_q[i]]++] = {rec_d[i], rec_p[i]};
  // (a thread per 32,768 entries or so: a few thousand entries are sorted sooner than a thread starts)
  in_blocks(nq, std::max<int64_t>(64, nq / std::max<int64_t>(total / 32768, 1)), [&](int, int64_t b, int64_t e) {
    for (int64_t i = b; i < e; ++i) std::sort(seg.begin() + first[i], seg.begin() + first[i + 1]);  // (no NaN among hits: a strict order)
    for (int64_t j = first[b]; j < first[e]; ++j) {
      if (dist2) dist2[j] = seg[(size_t)j].first;
      if (pos) pos[j] = seg[(size_t)j].second;
    }
  });
}

namespace {

struct Seg {  // queries that lie together on the device
  const float* dq;
  int64_t m, self_first;  // self_first >= 0: query i is the row at position self_first + i
};
struct Out {
  int64_t cap;
  int64_t *counts, *total;
  float* dist2;
  int32_t* pos;
  int64_t* ids;
  int32_t* atoms;
};

// what every entry point checks of the threshold, the cap and the outputs
int check_out(scann_handle* h, const char* who, float radius2, const Out& o) {
  const std::string w(who);
  if (!o.counts || !o.total) return fail(h, SCANN_ERR_INVALID, w + ": counts or total is null");
  if (!(radius2 >= 0.f)) return fail(h, SCANN_ERR_INVALID, w + ": radius2 must be >= 0 (+inf allowed) and not NaN");
  if (o.cap < 0 || o.cap > WITHIN_MAX_CAP)
    return fail(h, SCANN_ERR_INVALID, w + ": cap " + std::to_string(o.cap) + " outside 0 .. " + std::to_string(WITHIN_MAX_CAP));
  if (o.cap == 0 && (o.dist2 || o.pos || o.ids || o.atoms)) return fail(h, SCANN_ERR_INVALID, w + ": cap 0 is the count-only call, its entry arrays must be null");
  return SCANN_OK;
}

// The hits of the segments' queries (nq in all; dqid: device [nq] or null) in ix, by the size-then-fill protocol.  Synchronous.
int within_core(scann_handle* h, scann_index* ix, const std::vector<Seg>& segs, const int64_t* dqid, int64_t nq, int upper, float radius2,
                hipStream_t s, const Out& o) {
  std::fill(o.counts, o.counts + nq, 0);
  *o.total = 0;
  SearchStats st;
  st.write(ix);
  const int64_t N = ix->n;
  if (N == 0) return SCANN_OK;
  const CellPart* P = ix->part;
  const int stride = ix->stride;
  const int n_chunk = (int)((N + ix->chunk_rows - 1) / ix->chunk_rows);
  const int T_full = (int)SearchStats::full_tiles(ix), T = P ? P->n_tile : T_full, C = P ? P->lay.C : 0;
  const int64_t pass = P ? 1024 : WITHIN_PASS;
  int64_t seg_max = 0, n_groups = 0;
  for (const Seg& sg : segs) {
    seg_max = std::max(seg_max, sg.m);
    for (int64_t q0 = 0; q0 < sg.m; q0 += pass) n_groups += SearchStats::groups(std::min(pass, sg.m - q0));
  }
  const int64_t g = std::min(seg_max, pass);
  const int G = (int)SearchStats::groups(g);
  WithinArgs a{};
  CellSearchArgs ca = P ? cells_args(*P) : CellSearchArgs{};
  CallWs ws;
  const float* const* d_rows;
  const int64_t* const* d_ids;
  int32_t* d_qperm;
  ws.take(a.counts, (size_t)nq); ws.take(a.cursor, 1);
  const size_t zeroed = ws.bytes();
  ws.take(a.rec_q, (size_t)o.cap); ws.take(a.rec_p, (size_t)o.cap); ws.take(a.rec_d, (size_t)o.cap);
  ws.take(d_rows, P ? 0 : (size_t)n_chunk); ws.take(d_ids, P ? 0 : (size_t)n_chunk);
  ws.take(ca.D, P ? (size_t)g * std::max(C, 1) : 0); ws.take(ca.key_cell, P ? (size_t)g : 0); ws.take(ca.key_d, P ? (size_t)g : 0);
  ws.take(d_qperm, P ? (size_t)G * TILE_TQ : 0); ws.take(ca.list, P ? (size_t)G * T : 0); ws.take(ca.count, P ? (size_t)G : 0);
  HIPCHK(h, ws.alloc());  // (staging that does not fit: SCANN_ERR_OOM, and no kernel has run)
  a.stride = stride; a.upper = upper; a.radius2 = radius2; a.cap = o.cap;
  if (P) {
    a.rows = P->d_rows; a.ids = P->d_ids; a.pos = P->d_pos; a.n_entries = T * TILE_TR; a.chunk_rows = P->chunk_rows;
    a.qperm = d_qperm; a.list = ca.list; a.count = ca.count; a.n_tile = T;
    ca.k = 1; ca.qperm = d_qperm; ca.radius2 = radius2;
  } else {
    a.rows = d_rows; a.ids = d_ids; a.n_entries = (int32_t)N; a.chunk_rows = ix->chunk_rows;
  }
  std::vector<int32_t> plan_count((size_t)(P ? n_groups : 0));
  PassOrder order;
  int64_t groups_done = 0, q_off = 0;
  hipError_t e = hipMemsetAsync(ws.base(), 0, zeroed, s);
  if (e == hipSuccess && !P) e = ws.upload_rows(ix, n_chunk, d_rows, d_ids, s);
  for (const Seg& sg : segs) {
    for (int64_t q0 = 0; q0 < sg.m && e == hipSuccess; q0 += pass) {
      const int m = (int)std::min(pass, sg.m - q0), n_group = (int)SearchStats::groups(m);
      a.q = sg.dq + (size_t)q0 * stride; a.qid = dqid ? dqid + q_off + q0 : nullptr; a.nq = m; a.n_group = n_group;
      a.q_base = (int32_t)(q_off + q0); a.self_first = sg.self_first >= 0 ? (int32_t)(sg.self_first + q0) : -1;
      if (!P) {
        e = launch_within_tile(a, std::min(WITHIN_RANGES, T), s);
        int64_t visited = 0;
        for (int i = 0; i < n_group; ++i) visited += T - (upper ? std::min<int64_t>(T, (a.self_first + (int64_t)i * TILE_TQ + 1) / TILE_TR) : 0);
        st.pass(n_group, T_full, 0, visited);
        continue;
      }
      ca.q = a.q; ca.qid = a.qid; ca.nq = m; ca.n_group = n_group;
      e = cells_pass_order(ca, P->cell_rank, order, s);  // (the pass's one wait; the plan counts of the pass before have arrived too)
      if (e == hipSuccess) e = launch_cells_plan(ca, 2, s);
      if (e == hipSuccess) e = launch_within_tile(a, std::max(1, std::min(CELL_LISTS, T)), s);
      if (e == hipSuccess) e = hipMemcpyAsync(plan_count.data() + groups_done, ca.count, (size_t)n_group * 4, hipMemcpyDeviceToHost, s);
      groups_done += n_group;
      st.pass(n_group, T_full, 0, 0);  // (what it visited: the plan's counts, once they have arrived)
    }
    q_off += sg.m;
    if (e != hipSuccess) break;
  }
  std::vector<uint32_t> cnt((size_t)nq);
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), a.counts, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  int64_t total = 0;
  std::vector<int64_t> first((size_t)nq + 1, 0);
  std::vector<int32_t> rq, rp;
  std::vector<float> rd;
  hipError_t e_rec = hipSuccess;
  if (e == hipSuccess && e_sync == hipSuccess) {
    for (int64_t i = 0; i < nq; ++i) first[(size_t)i + 1] = first[(size_t)i] + cnt[(size_t)i];
    total = first[(size_t)nq];
    if (total > 0 && total <= o.cap) {
      rq.resize((size_t)total); rp.resize((size_t)total); rd.resize((size_t)total);
      e_rec = hipMemcpy(rq.data(), a.rec_q, (size_t)total * 4, hipMemcpyDeviceToHost);
      if (e_rec == hipSuccess) e_rec = hipMemcpy(rp.data(), a.rec_p, (size_t)total * 4, hipMemcpyDeviceToHost);
      if (e_rec == hipSuccess) e_rec = hipMemcpy(rd.data(), a.rec_d, (size_t)total * 4, hipMemcpyDeviceToHost);
    }
  }
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  HIPCHK(h, e_rec);
  for (int64_t i = 0; i < nq; ++i) o.counts[i] = cnt[(size_t)i];
  *o.total = total;
  for (int32_t c : plan_count) st.pass(0, 0, 0, c);
  st.write(ix);
  if (total == 0 || total > o.cap) return SCANN_OK;  // nothing to fill, or the caller sizes a second call by *total
  std::vector<int32_t> pos_h(o.pos ? 0 : (size_t)total);
  int32_t* pos = o.pos ? o.pos : pos_h.data();
  within_finish(first.data(), nq, rq.data(), rp.data(), rd.data(), total, o.dist2, pos);
  name_positions(ix, pos, (size_t)total, nullptr, o.ids, o.atoms);
  return SCANN_OK;
}

}  // namespace

extern "C" {

int scann_index_within(scann_handle_t* h, scann_index_t* ix, const float* q, int64_t nq, const int64_t* query_ids, float radius2, int64_t cap,
                       int64_t* counts, int64_t* total, float* dist2, int32_t* pos, int64_t* ids, int32_t* atoms) {
  if (const int r = check_index(h, ix, "scann_index_within")) return r;
  if (nq <= 0 || !q) return fail(h, SCANN_ERR_INVALID, "scann_index_within: an empty query");
  if (nq > (int64_t)0x7fffffff) return fail(h, SCANN_ERR_INVALID, "scann_index_within: too many queries in one call");
  const Out o{cap, counts, total, dist2, pos, ids, atoms};
  if (const int r = check_out(h, "scann_index_within", radius2, o)) return r;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  return staged_queries(h, ix, q, hipMemcpyHostToDevice, query_ids, nq, s, [&](const float* dq, const int64_t* dqid) {
    return within_core(h, ix, {Seg{dq, nq, -1}}, dqid, nq, 0, radius2, s, o);
  });
}

int scann_index_within_rows(scann_handle_t* h, scann_index_t* ix, int64_t first, int64_t n, int32_t upper, float radius2, int64_t cap,
                            int64_t* counts, int64_t* total, float* dist2, int32_t* pos, int64_t* ids, int32_t* atoms) {
  if (const int r = check_index(h, ix, "scann_index_within_rows")) return r;
  if (first < 0 || n <= 0 || first + n > ix->n)
    return fail(h, SCANN_ERR_INVALID, "scann_index_within_rows: rows " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " + std::to_string(ix->n));
  if (upper != 0 && upper != 1) return fail(h, SCANN_ERR_INVALID, "scann_index_within_rows: upper must be 0 or 1, got " + std::to_string(upper));
  const Out o{cap, counts, total, dist2, pos, ids, atoms};
  if (const int r = check_out(h, "scann_index_within_rows", radius2, o)) return r;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<Seg> segs;  // the queries where they lie, chunk by chunk: rows of the index are padded as queries are
  row_runs(ix, first, n, [&](size_t c, int64_t r0, int64_t m, int64_t done) {
    segs.push_back(Seg{ix->rows_of(c) + (size_t)r0 * ix->stride, m, first + done});
    return (int)SCANN_OK;
  });
  return within_core(h, ix, segs, nullptr, n, upper, radius2, h->streams[0], o);
}

int scann_index_within_batch(scann_handle_t* h, scann_index_t* ix, scann_dbatch_t* db, int32_t level, const int64_t* query_ids, float radius2,
                             int64_t cap, float* y, float* ga, int64_t* counts, int64_t* total, float* dist2, int32_t* pos, int64_t* ids,
                             int32_t* atoms) {
  if (const int r = check_index(h, ix, "scann_index_within_batch")) return r;
  if (!db) return fail(h, SCANN_ERR_INVALID, "scann_index_within_batch: null argument");
  if (const int r = check_level(h, ix, level, "scann_index_within_batch")) return r;
  const int64_t nq = level == SCANN_OUT_AFTER_LC ? db->n_atom : db->n_struct;
  if (nq <= 0) return fail(h, SCANN_ERR_INVALID, "scann_index_within_batch: an empty query");
  const Out o{cap, counts, total, dist2, pos, ids, atoms};
  if (const int r = check_out(h, "scann_index_within_batch", radius2, o)) return r;
  return staged_batch_queries(h, ix, db, level, query_ids, y, ga, "scann_index_within_batch", [&](const float* dq, const int64_t* dqid) {
    return within_core(h, ix, {Seg{dq, nq, -1}}, dqid, nq, 0, radius2, h->streams[db->last_slot], o);
  });
}

int scann_within_host(const float* rows, int64_t n, int64_t dim, const int64_t* row_ids, const float* q, int64_t nq, const int64_t* query_ids,
                      const int32_t* query_pos, int32_t upper, float radius2, int64_t cap, int64_t* counts, int64_t* total, float* dist2, int32_t* pos) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || (n > 0 && !rows) || nq <= 0 || nq > (int64_t)0x7fffffff || !q || !counts || !total) return SCANN_ERR_INVALID;
  if (!(radius2 >= 0.f) || cap < 0 || cap > WITHIN_MAX_CAP || (cap == 0 && (dist2 || pos))) return SCANN_ERR_INVALID;
  if ((upper != 0 && upper != 1) || (upper && !query_pos)) return SCANN_ERR_INVALID;
  struct Part {  // one thread's hits, in the order it met them; dropped once they alone exceed cap
    std::vector<int32_t> rq, rp;
    std::vector<float> rd;
    bool dropped = false;
  };
  std::vector<Part> parts(16);
  in_blocks(nq, 1, [&](int b, int64_t q_begin, int64_t q_end) {
    Part& part = parts[(size_t)b];
    std::vector<float> d((size_t)n);
    for (int64_t i = q_begin; i < q_end; ++i) {
      if (n > 0) dist2_to_rows(q + i * dim, rows, n, dim, d.data());
      const int32_t qp = query_pos ? query_pos[i] : -2;
      int64_t c = 0;
      for (int64_t r = upper ? (int64_t)qp + 1 : 0; r < n; ++r) {
        if (!(d[(size_t)r] <= radius2) || r == qp) continue;  // (NaN <= radius2 is false)
        if (query_ids && (row_ids ? row_ids[r] : r) == query_ids[i]) continue;
        ++c;
        if (part.dropped) continue;
        part.rq.push_back((int32_t)i); part.rp.push_back((int32_t)r); part.rd.push_back(d[(size_t)r]);
        if ((int64_t)part.rq.size() > cap) part = Part{{}, {}, {}, true};
      }
      counts[i] = c;
    }
  });
  std::vector<int64_t> first((size_t)nq + 1, 0);
  for (int64_t i = 0; i < nq; ++i) first[(size_t)i + 1] = first[(size_t)i] + counts[i];
  *total = first[(size_t)nq];
  if (*total == 0 || *total > cap) return SCANN_OK;
  std::vector<int32_t> rq, rp;
  std::vector<float> rd;
  for (auto it = parts.rbegin(); it != parts.rend(); ++it) {  // (the blocks back to front: the order of arrival is not part of the result)
    rq.insert(rq.end(), it->rq.begin(), it->rq.end()); rp.insert(rp.end(), it->rp.begin(), it->rp.end()); rd.insert(rd.end(), it->rd.begin(), it->rd.end());
  }
  within_finish(first.data(), nq, rq.data(), rp.data(), rd.data(), *total, dist2, pos);
  return SCANN_OK;
}

}  // extern "C"

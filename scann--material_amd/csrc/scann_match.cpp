// Structure matching on a latent-space index, the host half (include/scann_hip.h; scann_match.hip): the k nearest segments of every query
// structure, both taken as sets of rows, and the host twin scann_match_parts_host.  The forward of scann_index_match_batch is
// forward_and_download (scann_batch.cpp), as for the other batch calls of the index (scann_knn.cpp).
#include "scann_call.h"
#include "scann_knn.h"
#include "scann_match.h"
#include "scann_runtime.h"

using namespace scann;

namespace {

constexpr int MATCH_SET_GROUP = 256;  // query structures per pass over the index (bounds the partial lists)

// f and its witness for one query atom over m distances, g for every row brought up to date: the reductions of the definition
inline void match_reduce_row(const float* d, int64_t m, float* f, int64_t* wit, float* g) {
  *f = __builtin_inff();
  *wit = -1;
  for (int64_t j = 0; j < m; ++j) {
    if (!(d[j] == d[j])) continue;  // a NaN never counts
    if (*wit < 0 || d[j] < *f) *f = d[j], *wit = j;
    if (d[j] < g[j]) g[j] = d[j];
  }
}

// parts[4] of one (set, segment) pair: q [n][dim], rows [m][dim]; tmp [m], g [m]
void match_pair_parts(const float* q, int64_t n, const float* rows, int64_t m, int64_t dim, float* tmp, float* g, float* parts) {
  std::fill(g, g + m, __builtin_inff());
  double F = 0.0, G = 0.0;
  float Fmax = -__builtin_inff(), Gmax = -__builtin_inff();
  for (int64_t i = 0; i < n; ++i) {
    dist2_to_rows(q + i * dim, rows, m, dim, tmp);
    float f;
    int64_t w;
    match_reduce_row(tmp, m, &f, &w, g);
    F += (double)f;
    Fmax = std::max(Fmax, f);
  }
  for (int64_t j = 0; j < m; ++j) {
    G += (double)g[j];
    Gmax = std::max(Gmax, g[j]);
  }
  parts[0] = (float)(F / (double)n);
  parts[1] = (float)(G / (double)m);
  parts[2] = Fmax;
  parts[3] = Gmax;
}

int check_match(scann_handle* h, const scann_index* ix, int32_t measure, int32_t k, const float* score, const char* who) {
  if (const int r = check_index(h, ix, who)) return r;
  if (const int r = check_k(h, k, who)) return r;
  if (measure < SCANN_MATCH_CHAMFER || measure > SCANN_MATCH_COVER)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": measure " + std::to_string(measure) + " is none of SCANN_MATCH_CHAMFER (0), SCANN_MATCH_HAUSDORFF (1), SCANN_MATCH_COVER (2)");
  if (!score) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": score is null");
  return SCANN_OK;
}

// q_first [n_sets + 1] of a match: starts at 0, every set holds 1 .. SCANN_MATCH_MAX_ATOMS rows
int check_match_sets(scann_handle* h, const int32_t* q_first, int64_t n_sets, const char* who) {
  if (n_sets <= 0 || !q_first) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": an empty query");
  if (n_sets > (int64_t)0x7fffffff / SCANN_KNN_MAX_K / 4) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": too many query structures in one call");
  if (q_first[0] != 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": q_first[0] is " + std::to_string(q_first[0]) + ", not 0");
  for (int64_t s = 0; s < n_sets; ++s) {
    const int64_t n = (int64_t)q_first[s + 1] - q_first[s];
    if (n < 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": q_first decreases at query structure " + std::to_string(s));
    if (n == 0) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": query structure " + std::to_string(s) + " is an empty set");
    if (n > SCANN_MATCH_MAX_ATOMS)
      return fail(h, SCANN_ERR_UNSUPPORTED, std::string(who) + ": query structure " + std::to_string(s) + " has " + std::to_string(n) +
                                                " atoms, more than SCANN_MATCH_MAX_ATOMS = " + std::to_string(SCANN_MATCH_MAX_ATOMS));
  }
  if ((int64_t)q_first[n_sets] > (int64_t)0x7fffffff / SCANN_KNN_MAX_K) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": too many query rows in one call");
  return SCANN_OK;
}

// The sets of query rows on the device (dq [q_first[n_sets]][stride], padded like the index's rows) against the segments of the index.
// q_first, qid: host.  The arguments have been checked.
int match_search(scann_handle* h, scann_index* ix, const float* dq, const int32_t* q_first, int64_t n_sets, const int64_t* qid, int measure, int k,
                 hipStream_t s, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos, float* match_d) {
  const int64_t N = ix->n, nq = q_first[n_sets], n_pair = n_sets * k;
  const float inf = __builtin_inff();
  for (int64_t e = 0; e < n_pair; ++e) {  // the places without a segment; the others are overwritten below
    score[e] = inf;
    if (segment) segment[e] = -1;
    if (ids) ids[e] = -1;
    if (sizes) sizes[e] = 0;
  }
  if (parts) std::fill(parts, parts + n_pair * 4, inf);
  if (match_pos) std::fill(match_pos, match_pos + nq * k, -1);
  if (match_d) std::fill(match_d, match_d + nq * k, inf);
  if (N == 0) return SCANN_OK;
  const int64_t n_seg = (int64_t)ix->seg_first.size();
  auto seg_end = [&](int64_t g) { return g + 1 < n_seg ? (int64_t)ix->seg_first[(size_t)(g + 1)] : N; };
  // the tiles: whole structures, at most TILE_TQ atoms and MT_SETS structures each
  std::vector<int32_t> tiles;
  int64_t most_sets = 1;
  for (int64_t b = 0; b < n_sets;) {
    int64_t e = b + 1;
    while (e < n_sets && e - b < MT_SETS && q_first[e + 1] - q_first[b] <= TILE_TQ) ++e;
    most_sets = std::max(most_sets, e - b);
    tiles.push_back((int32_t)b);
    tiles.push_back((int32_t)e);
    b = e;
  }
  // the ranges: whole segments, closed as soon as they hold about 1 / KNN_RANGES of the rows
  const int64_t target = std::max<int64_t>(TILE_TR, ((N + KNN_RANGES - 1) / KNN_RANGES + TILE_TR - 1) / TILE_TR * TILE_TR);
  std::vector<int32_t> ranges;
  for (int64_t g = 0; g < n_seg;) {
    const int64_t g0 = g, r0 = ix->seg_first[(size_t)g];
    while (g < n_seg && seg_end(g) - r0 < target) ++g;
    if (g < n_seg) ++g;
    ranges.push_back((int32_t)r0);
    ranges.push_back((int32_t)seg_end(g - 1));
    ranges.push_back((int32_t)g0);
  }
  const int n_tile = (int)(tiles.size() / 2), n_range = (int)(ranges.size() / 3), n_chunk = (int)ix->chunks.size();
  const bool want_pairs = parts || match_pos || match_d;
  const int64_t g_sets = std::min<int64_t>(n_sets, MATCH_SET_GROUP);
  // one workspace for the call (every region holds at least one element)
  MatchArgs a{};
  MatchPairArgs pa{};
  float* out_d;
  int32_t* out_p;
  const int32_t* d_tiles;
  const size_t n_part = (size_t)std::max<int64_t>(g_sets * n_range * k, 1), n_tab = (size_t)std::max(n_chunk, 1), n_match = (size_t)std::max<int64_t>(nq * k, 1);
  CallWs ws;
  ws.take(a.part_d, n_part); ws.take(a.part_p, n_part); ws.take(out_d, (size_t)n_pair); ws.take(out_p, (size_t)n_pair);
  ws.take(a.rows, n_tab); ws.take(a.ids, n_tab); ws.take(a.q_first, (size_t)n_sets + 1); ws.take(a.qid, (size_t)n_sets);
  ws.take(d_tiles, tiles.size()); ws.take(a.ranges, ranges.size()); ws.take(pa.seg_first, (size_t)n_pair); ws.take(pa.seg_count, (size_t)n_pair);
  ws.take(pa.parts, (size_t)n_pair * 4); ws.take(pa.match_pos, n_match); ws.take(pa.match_d, n_match);
  HIPCHK(h, ws.alloc());
  std::vector<int32_t> seg_h((size_t)n_pair), pf((size_t)n_pair, 0), pc((size_t)n_pair, 0), pos_h;
  std::vector<float> parts_h, md_h;
  hipError_t e = ws.upload_rows(ix, n_chunk, a.rows, a.ids, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.q_first), q_first, (size_t)(n_sets + 1) * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && qid) e = hipMemcpyAsync(writable(a.qid), qid, (size_t)n_sets * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(d_tiles), tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(writable(a.ranges), ranges.data(), ranges.size() * 4, hipMemcpyHostToDevice, s);
  a.chunk_rows = ix->chunk_rows; a.stride = ix->stride; a.q = dq;
  if (!qid) a.qid = nullptr;
  a.n_range = n_range; a.k = k; a.measure = measure; a.sets_ld = most_sets <= MT_SETS_SMALL ? MT_SETS_SMALL : MT_SETS;
  for (int t0 = 0; t0 < n_tile && e == hipSuccess;) {  // a group of tiles: at most MATCH_SET_GROUP structures (a tile holds at most MT_SETS)
    int t1 = t0 + 1;
    while (t1 < n_tile && tiles[(size_t)2 * t1 + 1] - tiles[(size_t)2 * t0] <= g_sets) ++t1;
    const int set0 = tiles[(size_t)2 * t0], set1 = tiles[(size_t)2 * t1 - 1];
    a.tiles = d_tiles + 2 * t0;
    a.n_tile = t1 - t0; a.set_base = set0;
    e = launch_match_tile(a, s);
    if (e == hipSuccess) e = launch_knn_merge(a.part_d, a.part_p, set1 - set0, n_range, k, out_d + (size_t)set0 * k, out_p + (size_t)set0 * k, s);
    t0 = t1;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(score, out_d, (size_t)n_pair * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(seg_h.data(), out_p, (size_t)n_pair * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) {
    for (int64_t i = 0; i < n_pair; ++i) {
      const int32_t g = seg_h[(size_t)i];
      if (g < 0) continue;
      pf[(size_t)i] = ix->seg_first[(size_t)g];
      pc[(size_t)i] = (int32_t)(seg_end(g) - pf[(size_t)i]);
      if (segment) segment[i] = g;
      if (ids) ids[i] = ix->ids[(size_t)pf[(size_t)i]];
      if (sizes) sizes[i] = pc[(size_t)i];
    }
  }
  if (e == hipSuccess && want_pairs) {  // the winning pairs once more: parts and witnesses
    pa.rows = a.rows; pa.chunk_rows = ix->chunk_rows; pa.stride = ix->stride; pa.q = dq; pa.q_first = a.q_first;
    pa.n_sets = (int32_t)n_sets; pa.k = k;
    parts_h.resize((size_t)n_pair * 4);
    pos_h.resize((size_t)nq * k);
    md_h.resize((size_t)nq * k);
    e = hipMemcpyAsync(writable(pa.seg_first), pf.data(), (size_t)n_pair * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(writable(pa.seg_count), pc.data(), (size_t)n_pair * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_match_pair(pa, s);
    if (e == hipSuccess) e = hipMemcpyAsync(parts_h.data(), pa.parts, (size_t)n_pair * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pos_h.data(), pa.match_pos, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(md_h.data(), pa.match_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s);
  }
  const hipError_t e_sync = hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  for (int64_t st = 0; st < n_sets && want_pairs; ++st)  // (the places without a segment keep the tail: the kernel wrote nothing there)
    for (int p = 0; p < k; ++p) {
      const int64_t i = st * k + p;
      if (seg_h[(size_t)i] < 0) continue;
      if (parts) std::copy(parts_h.begin() + i * 4, parts_h.begin() + i * 4 + 4, parts + i * 4);
      for (int64_t r = q_first[st]; r < q_first[st + 1]; ++r) {
        if (match_pos) match_pos[r * k + p] = pos_h[(size_t)(r * k + p)];
        if (match_d) match_d[r * k + p] = md_h[(size_t)(r * k + p)];
      }
    }
  return SCANN_OK;
}

}  // namespace

// as staged_queries (scann_search.h): host or device query rows of the index's width staged at the padded width, then matched (scann_match.h)
int scann::match_staged(scann_handle* h, scann_index* ix, const float* q, hipMemcpyKind kind, const int32_t* q_first, int64_t n_sets, const int64_t* qid,
                 int measure, int k, hipStream_t s, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos,
                 float* match_d) {
  const int64_t nq = q_first[n_sets];
  CallWs ws;
  RowStage st;
  st.take(ws, nq, ix->dim, ix->dim, ix->stride, kind);
  HIPCHK(h, ws.alloc());
  const hipError_t e = st.stage_rows(q, s);
  int r = SCANN_OK;
  if (e == hipSuccess)
    r = match_search(h, ix, st.rows(q), q_first, n_sets, qid, measure, k, s, score, segment, ids, sizes, parts, match_pos, match_d);
  else
    (void)hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  return r;
}

extern "C" {

int64_t scann_index_segments(const scann_index_t* ix, int64_t* first, int32_t* count, int64_t* id) {
  if (!ix) return SCANN_ERR_INVALID;
  const size_t n_seg = ix->seg_first.size();
  for (size_t g = 0; g < n_seg; ++g) {
    const int64_t f = ix->seg_first[g], e = g + 1 < n_seg ? (int64_t)ix->seg_first[g + 1] : ix->n;
    if (first) first[g] = f;
    if (count) count[g] = (int32_t)(e - f);
    if (id) id[g] = ix->ids[(size_t)f];
  }
  return (int64_t)n_seg;
}

int scann_index_match(scann_handle_t* h, scann_index_t* ix, const float* q, const int32_t* q_first, int64_t n_sets, const int64_t* query_ids,
                      int32_t measure, int32_t k, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos,
                      float* match_dist2) {
  if (const int r = check_match(h, ix, measure, k, score, "scann_index_match")) return r;
  if (!q) return fail(h, SCANN_ERR_INVALID, "scann_index_match: an empty query");
  if (const int r = check_match_sets(h, q_first, n_sets, "scann_index_match")) return r;
  HIPCHK(h, hipSetDevice(h->device));
  return match_staged(h, ix, q, hipMemcpyHostToDevice, q_first, n_sets, query_ids, measure, k, h->streams[0], score, segment, ids, sizes, parts,
                      match_pos, match_dist2);
}

int scann_index_match_batch(scann_handle_t* h, scann_index_t* ix, scann_dbatch_t* db, const int64_t* query_ids, int32_t measure, int32_t k, float* y,
                            float* ga, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos,
                            float* match_dist2) {
  if (const int r = check_match(h, ix, measure, k, score, "scann_index_match_batch")) return r;
  if (!db) return fail(h, SCANN_ERR_INVALID, "scann_index_match_batch: null argument");
  if (const int r = check_level(h, ix, SCANN_OUT_AFTER_LC, "scann_index_match_batch")) return r;
  if (db->n_struct <= 0 || db->n_atom <= 0) return fail(h, SCANN_ERR_INVALID, "scann_index_match_batch: an empty query");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_index_match_batch: weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> mol;
  if (const int r = read_mol_offset(h, db, mol)) return r;
  if (const int r = check_match_sets(h, mol.data(), db->n_struct, "scann_index_match_batch")) return r;
  if (const int r = forward_and_download(h, db, 0, SCANN_OUT_AFTER_LC, y, ga)) return r;
  // the batch's after_Lc rows are the queries where the forward left them
  return match_staged(h, ix, db->out_z, hipMemcpyDeviceToDevice, mol.data(), db->n_struct, query_ids, measure, k, h->streams[db->last_slot], score,
                      segment, ids, sizes, parts, match_pos, match_dist2);
}

int scann_match_parts_host(const float* q, const int32_t* q_first, int64_t n_sets, const float* rows, const int32_t* seg_first, int64_t n_seg,
                           int64_t dim, float* parts) {
  if (!q || !q_first || !rows || !seg_first || !parts || n_sets < 1 || n_seg < 1 || dim < 1) return SCANN_ERR_INVALID;
  for (int64_t s = 0; s < n_sets; ++s)
    if (q_first[s + 1] <= q_first[s]) return SCANN_ERR_INVALID;
  int64_t longest = 0;
  for (int64_t g = 0; g < n_seg; ++g) {
    if (seg_first[g + 1] <= seg_first[g]) return SCANN_ERR_INVALID;
    longest = std::max<int64_t>(longest, seg_first[g + 1] - seg_first[g]);
  }
  std::vector<float> tmp((size_t)longest), gv((size_t)longest);
  for (int64_t s = 0; s < n_sets; ++s)
    for (int64_t g = 0; g < n_seg; ++g)
      match_pair_parts(q + (int64_t)q_first[s] * dim, q_first[s + 1] - q_first[s], rows + (int64_t)seg_first[g] * dim, seg_first[g + 1] - seg_first[g],
                       dim, tmp.data(), gv.data(), parts + (s * n_seg + g) * 4);
  return SCANN_OK;
}

}  // extern "C"

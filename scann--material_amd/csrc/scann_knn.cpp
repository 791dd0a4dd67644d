// Latent-space index (include/scann_hip.h: scann_index_*): the rows of bf_property / after_Lc kept on the device in chunks that never
// move, the exact k-nearest-neighbour search over them (scann_knn.hip) and the host twin of the kernel's distance chain.  Every call is
// synchronous: it returns when the device has finished its work, so no query is ever in flight while an add runs.  The analyses over an
// index have host files of their own (scann_select.cpp, scann_kmeans.cpp, scann_pca.cpp, scann_match.cpp, ...); what they use from here is
// declared in scann_knn.h.  The forward of scann_index_add_batch / scann_index_query_batch is forward_and_download (scann_batch.cpp) with
// the level's output flag in that one forward's options: y, the scores, the range guard and the exact re-run behave as in
// scann_batch_download, and the handle is not written.
#include "scann_call.h"
#include "scann_cells.h"
#include "scann_knn.h"
#include "scann_runtime.h"
#include "scann_search.h"

using namespace scann;

namespace {

constexpr int KNN_QGROUP = 1024;     // queries per pass over the index (bounds the partial lists)
constexpr int KNN_MAX_RANGES = 65536;

inline float dist2_chain(const float* q, const float* r, int64_t d) {
  float acc = 0.f;
  for (int64_t j = 0; j < d; ++j) {
    const float t = q[j] - r[j];
    acc = fmaf(t, t, acc);
  }
  return acc;
}
void dist2_matrix_plain(const float* q, int64_t nq, const float* rows, int64_t n, int64_t d, float* out) {
  for (int64_t i = 0; i < nq; ++i)
    for (int64_t r = 0; r < n; ++r) out[i * n + r] = dist2_chain(q + i * d, rows + r * d, d);
}
// the same loop where the host has a fused multiply-add instruction: fmaf is then one instruction instead of a libm call; it is correctly
// rounded either way, so the bits are the same
__attribute__((target("fma"))) void dist2_matrix_fma(const float* q, int64_t nq, const float* rows, int64_t n, int64_t d, float* out) {
  for (int64_t i = 0; i < nq; ++i)
    for (int64_t r = 0; r < n; ++r) {
      const float *a = q + i * d, *b = rows + r * d;
      float acc = 0.f;
      for (int64_t j = 0; j < d; ++j) {
        const float t = a[j] - b[j];
        acc = __builtin_fmaf(t, t, acc);
      }
      out[i * n + r] = acc;
    }
}

}  // namespace

namespace scann {

int check_index(scann_handle* h, const scann_index* ix, const char* who) {
  if (!h || !ix) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": null argument");
  if (ix->h != h) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": the index belongs to another handle");
  return SCANN_OK;
}

int check_k(scann_handle* h, int32_t k, const char* who) {
  if (k < 1 || k > SCANN_KNN_MAX_K)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": k " + std::to_string(k) + " outside 1 .. " + std::to_string(SCANN_KNN_MAX_K));
  return SCANN_OK;
}

int index_new_chunk(scann_handle* h, scann_index* ix, hipStream_t s) {
  char* p = nullptr;
  HIPCHK(h, cached_malloc((void**)&p, ix->chunk_bytes()));
  ix->chunks.push_back(p);
  HIPCHK(h, hipMemsetAsync(p, 0, ix->chunk_bytes(), s));  // the padding columns are zero: fmaf(0, 0, acc) == acc
  return SCANN_OK;
}

void index_note_rows(scann_index* ix, int64_t n, const int64_t* ids, const int32_t* atoms) {
  if (n > 0) cells_drop(ix);  // a partition describes the rows it was built from (the appends are synchronous: nothing reads it now)
  for (int64_t i = 0; i < n; ++i)
    if ((i == 0 ? ix->ids.empty() || ix->ids.back() != ids[0] : ids[i] != ids[i - 1])) ix->seg_first.push_back((int32_t)(ix->n + i));
  ix->ids.insert(ix->ids.end(), ids, ids + n);
  ix->atoms.insert(ix->atoms.end(), atoms, atoms + n);
  ix->n += n;
}

}  // namespace scann

namespace {

// n rows of `dim` floats, `pitch` bytes apart at src (host or device, `kind`), appended behind the index's rows; ids / atoms: host, n each.
// Rows already stored stay where they are: a chunk that is full is never touched again, a new one comes from the handle's cache.
int append_rows(scann_handle* h, scann_index* ix, const void* src, size_t pitch, hipMemcpyKind kind, int64_t n, const int64_t* ids,
                const int32_t* atoms, hipStream_t s) {
  if (n <= 0) return SCANN_OK;
  if (ix->n + n > (int64_t)0x7fffffff) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_index_add: an index holds fewer than 2^31 rows");
  const int r = row_runs(ix, ix->n, n, [&](size_t c, int64_t r0, int64_t m, int64_t done) {
    if (c == ix->chunks.size())
      if (const int r = index_new_chunk(h, ix, s)) return r;
    HIPCHK(h, hipMemcpy2DAsync(ix->rows_of(c) + (size_t)r0 * ix->stride, (size_t)ix->stride * 4, static_cast<const char*>(src) + (size_t)done * pitch,
                               pitch, (size_t)ix->dim * 4, (size_t)m, kind, s));
    HIPCHK(h, hipMemcpyAsync(ix->ids_of(c) + r0, ids + done, (size_t)m * 8, hipMemcpyHostToDevice, s));
    return (int)SCANN_OK;
  });
  if (r) return r;
  HIPCHK(h, hipStreamSynchronize(s));
  index_note_rows(ix, n, ids, atoms);
  return SCANN_OK;
}

}  // namespace

// nq queries on the device ([nq][stride], padded like the rows; qid: device [nq] or null) against the whole index.  dev_d non-null: the
// distances [nq][k] are left there, on the device, and nothing comes back to the host (scann_index_select: the pool's rows against the
// reference, k = 1)
int scann::search(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2, int64_t* ids,
                  int32_t* atoms, int32_t* pos, float* dev_d) {
  return ix->part ? cells_search(h, ix, dq, dqid, nq, k, s, dist2, ids, atoms, pos, dev_d)
                  : search_full(h, ix, dq, dqid, nq, k, s, dist2, ids, atoms, pos, dev_d);
}

// the search that compares every query with every row (what search() is without a partition, and what cells_search falls back to)
int scann::search_full(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2,
                       int64_t* ids, int32_t* atoms, int32_t* pos, float* dev_d) {
  const int64_t N = ix->n;
  const int rpr = (int)std::max<int64_t>(TILE_TR, ((N + KNN_RANGES - 1) / KNN_RANGES + TILE_TR - 1) / TILE_TR * TILE_TR);
  // one launch over all chunks: every chunk is cut into the same number of ranges (those behind the last row stay empty)
  const int n_chunk = (int)((N + ix->chunk_rows - 1) / ix->chunk_rows);
  const int64_t n_range = (int64_t)n_chunk * ((std::min<int64_t>(N, ix->chunk_rows) + rpr - 1) / rpr);
  if (n_range > KNN_MAX_RANGES || n_chunk > 65535) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_index_query: the index has too many chunks");
  const int64_t g = std::min<int64_t>(nq, KNN_QGROUP);
  const size_t n_part = (size_t)std::max<int64_t>(g * n_range * k, 1), n_tab = (size_t)std::max(n_chunk, 1);
  CallWs ws;
  float *part_d, *out_d;
  int32_t *part_p, *out_p;
  const float* const* d_rows;
  const int64_t* const* d_ids;
  ws.take(part_d, n_part); ws.take(part_p, n_part); ws.take(out_d, (size_t)g * k); ws.take(out_p, (size_t)g * k);
  ws.take(d_rows, n_tab); ws.take(d_ids, n_tab);
  HIPCHK(h, ws.alloc());
  std::vector<int32_t> pos_h(dev_d ? 0 : (size_t)nq * k);
  SearchStats st;  // every (128-query group, 64-row tile) pair is visited
  hipError_t e = ws.upload_rows(ix, n_chunk, d_rows, d_ids, s);  // the chunks' rows, and their ids
  for (int64_t q0 = 0; q0 < nq && e == hipSuccess; q0 += g) {
    const int m = (int)std::min<int64_t>(g, nq - q0);
    st.pass(SearchStats::groups(m), SearchStats::full_tiles(ix), 0, SearchStats::groups(m) * SearchStats::full_tiles(ix));
    KnnArgs a{};
    a.rows = d_rows; a.ids = d_ids;
    a.n_total = (int32_t)N; a.chunk_rows = ix->chunk_rows; a.n_chunk = n_chunk;
    a.stride = ix->stride; a.q = dq + (size_t)q0 * ix->stride; a.qid = dqid ? dqid + q0 : nullptr; a.nq = m; a.k = k; a.rows_per_range = rpr;
    a.part_d = part_d; a.part_p = part_p; a.n_range = (int)n_range;
    e = launch_knn_tile(a, s);
    if (e == hipSuccess) e = launch_knn_merge(part_d, part_p, m, (int)n_range, k, dev_d ? dev_d + (size_t)q0 * k : out_d, out_p, s);
    if (dev_d) continue;  // (the stream orders the next group's use of the partial lists)
    if (e == hipSuccess) e = hipMemcpyAsync(dist2 + (size_t)q0 * k, out_d, (size_t)m * k * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pos_h.data() + (size_t)q0 * k, out_p, (size_t)m * k * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (dev_d && e == hipSuccess) e = hipStreamSynchronize(s);
  else if (e != hipSuccess) (void)hipStreamSynchronize(s);
  ws.release();
  HIPCHK(h, e);
  st.write(ix);
  name_positions(ix, pos_h.data(), pos_h.size(), pos, ids, atoms);
  return SCANN_OK;
}

// dist2 of one vector to n rows, the chain above (with the host's fused multiply-add where it has one: the same bits)
void scann::dist2_to_rows(const float* q, const float* rows, int64_t n, int64_t d, float* out) {
  if (__builtin_cpu_supports("fma")) dist2_matrix_fma(q, 1, rows, n, d, out);
  else dist2_matrix_plain(q, 1, rows, n, d, out);
}

// The rows a batch has at a level -- one per structure, or (atom) one per atom in packed order -- named: id_v = the structure's id
// (ids[b]; ids null: first + b), at_v (if asked for) = the atom's index in its structure, -1 for a structure row
int scann::expand_ids(scann_handle* h, const scann_dbatch* db, bool atom, const int64_t* ids, int64_t first, std::vector<int64_t>& id_v,
               std::vector<int32_t>* at_v) {
  const int B = db->n_struct;
  id_v.assign((size_t)(atom ? db->n_atom : B), 0);
  if (at_v) at_v->assign(id_v.size(), -1);
  std::vector<int32_t> mol;
  if (atom)
    if (const int r = read_mol_offset(h, db, mol)) return r;
  for (int b = 0; b < B; ++b) {
    const int64_t id = ids ? ids[b] : first + b;
    if (!atom) id_v[(size_t)b] = id;
    else
      for (int i = mol[b]; i < mol[b + 1]; ++i) {
        id_v[(size_t)i] = id;
        if (at_v) (*at_v)[(size_t)i] = i - mol[b];
      }
  }
  return SCANN_OK;
}

extern "C" {

float scann_knn_distsq(const float* q, const float* r, int64_t d) { return q && r && d > 0 ? dist2_chain(q, r, d) : 0.f; }

void scann_knn_distsq_matrix(const float* q, int64_t nq, const float* rows, int64_t n, int64_t d, float* out) {
  if (!q || !rows || !out || nq <= 0 || n <= 0) return;
  if (d < 0) d = 0;
  if (__builtin_cpu_supports("fma")) dist2_matrix_fma(q, nq, rows, n, d, out);
  else dist2_matrix_plain(q, nq, rows, n, d, out);
}

int scann_index_create(scann_handle_t* h, int32_t dim, scann_index_t** out) {
  if (!h || !out) return fail(h, SCANN_ERR_INVALID, "scann_index_create: null argument");
  if (dim < 1 || dim > 1024) return fail(h, SCANN_ERR_INVALID, "scann_index_create: dim " + std::to_string(dim) + " outside 1 .. 1024");
  scann_index* ix = new scann_index();
  ix->h = h;
  ix->device = h->device;
  ix->dim = dim;
  ix->stride = (dim + 3) / 4 * 4;
  static_assert(4096 % TILE_TR == 0, "a chunk holds whole tiles (SearchStats::full_tiles)");
  ix->chunk_rows = (int32_t)std::max<size_t>(4096, ((size_t)64 << 20) / ((size_t)ix->stride * 4) / TILE_TR * TILE_TR);
  *out = ix;
  return SCANN_OK;
}

void scann_index_free(scann_handle_t* h, scann_index_t* ix) {
  if (!ix) return;
  (void)h;  // (the chunks go back to the device's block cache, which outlives the handle)
  if (hipSetDevice(ix->device) == hipSuccess) (void)hipDeviceSynchronize();
  cells_drop(ix);
  for (char* p : ix->chunks) cached_free(p);
  delete ix;
}

int64_t scann_index_size(const scann_index_t* ix) { return ix ? ix->n : SCANN_ERR_INVALID; }

int scann_index_add(scann_handle_t* h, scann_index_t* ix, const float* rows, int64_t n, const int64_t* ids, const int32_t* atoms) {
  if (const int r = check_index(h, ix, "scann_index_add")) return r;
  if (n < 0 || (n > 0 && !rows)) return fail(h, SCANN_ERR_INVALID, "scann_index_add: n rows need a rows pointer and n >= 0");
  if (n == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int64_t> id_v((size_t)n);
  std::vector<int32_t> at_v((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) id_v[(size_t)i] = ids ? ids[i] : ix->n + i;  // ids NULL: the position
  if (atoms) std::copy(atoms, atoms + n, at_v.begin());
  return append_rows(h, ix, rows, (size_t)ix->dim * 4, hipMemcpyHostToDevice, n, id_v.data(), at_v.data(), h->streams[0]);
}

int scann_index_read(scann_handle_t* h, scann_index_t* ix, int64_t first, int64_t n, float* rows, int64_t* ids, int32_t* atoms) {
  if (const int r = check_index(h, ix, "scann_index_read")) return r;
  if (first < 0 || n < 0 || first + n > ix->n)
    return fail(h, SCANN_ERR_INVALID, "scann_index_read: rows " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " + std::to_string(ix->n));
  HIPCHK(h, hipSetDevice(h->device));
  if (rows)
    if (const int r = row_runs(ix, first, n, [&](size_t c, int64_t r0, int64_t m, int64_t done) {
          HIPCHK(h, hipMemcpy2D(rows + (size_t)done * ix->dim, (size_t)ix->dim * 4, ix->rows_of(c) + (size_t)r0 * ix->stride, (size_t)ix->stride * 4,
                                (size_t)ix->dim * 4, (size_t)m, hipMemcpyDeviceToHost));
          return (int)SCANN_OK;
        }))
      return r;
  if (ids) std::copy(ix->ids.begin() + first, ix->ids.begin() + first + n, ids);
  if (atoms) std::copy(ix->atoms.begin() + first, ix->atoms.begin() + first + n, atoms);
  return SCANN_OK;
}

int scann_index_query(scann_handle_t* h, scann_index_t* ix, const float* q, int64_t nq, const int64_t* query_ids, int32_t k, float* dist2,
                      int64_t* ids, int32_t* atoms, int32_t* pos) {
  if (const int r = check_index(h, ix, "scann_index_query")) return r;
  if (const int r = check_k(h, k, "scann_index_query")) return r;
  if (nq <= 0 || !q) return fail(h, SCANN_ERR_INVALID, "scann_index_query: an empty query");
  if (nq > (int64_t)0x7fffffff / SCANN_KNN_MAX_K) return fail(h, SCANN_ERR_INVALID, "scann_index_query: too many queries in one call");
  if (!dist2) return fail(h, SCANN_ERR_INVALID, "scann_index_query: dist2 is null");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  return staged_queries(h, ix, q, hipMemcpyHostToDevice, query_ids, nq, s, [&](const float* dq, const int64_t* dqid) {
    return search(h, ix, dq, dqid, nq, k, s, dist2, ids, atoms, pos);
  });
}

int scann_index_add_batch(scann_handle_t* h, scann_index_t* ix, scann_dbatch_t* db, int32_t level, const int64_t* ids) {
  if (const int r = check_index(h, ix, "scann_index_add_batch")) return r;
  if (!db) return fail(h, SCANN_ERR_INVALID, "scann_index_add_batch: null argument");
  if (const int r = check_level(h, ix, level, "scann_index_add_batch")) return r;
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_index_add_batch: weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, nullptr, nullptr)) return r;
  const bool atom = level == SCANN_OUT_AFTER_LC;
  std::vector<int64_t> id_v;
  std::vector<int32_t> at_v;
  if (const int r = expand_ids(h, db, atom, ids, atom ? 0 : ix->n, id_v, &at_v)) return r;  // (ids null: the structure's place in the batch / the row's position)
  return append_rows(h, ix, atom ? db->out_z : db->out_bf, (size_t)ix->dim * 4, hipMemcpyDeviceToDevice, (int64_t)id_v.size(), id_v.data(),
                     at_v.data(), h->streams[db->last_slot]);
}

int scann_index_query_batch(scann_handle_t* h, scann_index_t* ix, scann_dbatch_t* db, int32_t level, const int64_t* query_ids, int32_t k, float* y,
                            float* ga, float* dist2, int64_t* ids, int32_t* atoms, int32_t* pos) {
  if (const int r = check_index(h, ix, "scann_index_query_batch")) return r;
  if (!db) return fail(h, SCANN_ERR_INVALID, "scann_index_query_batch: null argument");
  if (const int r = check_k(h, k, "scann_index_query_batch")) return r;
  if (const int r = check_level(h, ix, level, "scann_index_query_batch")) return r;
  const int64_t nq = level == SCANN_OUT_AFTER_LC ? db->n_atom : db->n_struct;
  if (nq <= 0) return fail(h, SCANN_ERR_INVALID, "scann_index_query_batch: an empty query");
  if (!dist2) return fail(h, SCANN_ERR_INVALID, "scann_index_query_batch: dist2 is null");
  return staged_batch_queries(h, ix, db, level, query_ids, y, ga, "scann_index_query_batch", [&](const float* dq, const int64_t* dqid) {
    return search(h, ix, dq, dqid, nq, k, h->streams[db->last_slot], dist2, ids, atoms, pos);
  });
}

}  // extern "C"

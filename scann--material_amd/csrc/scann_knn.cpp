// Latent-space index (include/scann_hip.h: scann_index_*): the rows of bf_property / after_Lc kept on the device in chunks that never
// move, the exact k-nearest-neighbour search over them (scann_knn.hip) and the host twin of the kernel's distance chain.  Every call is
// synchronous: it returns when the device has finished its work, so no query is ever in flight while an add runs.  The host halves of
// the k-center selection (scann_select.hip) and of the k-means clustering (scann_kmeans.hip) and their host twins are here as well, and
// the host half of the principal-component map (scann_pca.hip; its twins and the eigen-decomposition are in scann_pca.cpp), and at the
// end of the file the host half of the structure matching (scann_match.hip) with its host twin.  The forward of
// scann_index_add_batch / scann_index_query_batch / scann_index_match_batch / scann_project_batch is forward_and_download (scann_batch.cpp) with the level's output flag in that one
// forward's options: y, the scores, the range guard and the exact re-run behave as in scann_batch_download, and the handle is not written.
#include "scann_kmeans.h"
#include "scann_knn.h"
#include "scann_match.h"
#include "scann_pca.h"
#include "scann_runtime.h"
#include "scann_select.h"

using namespace scann;

namespace {

constexpr int KNN_QGROUP = 1024;     // queries per pass over the index (bounds the partial lists)
constexpr int KNN_RANGES = 1024;     // about as many row ranges, i.e. workgroups per 128 queries, as this
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

// the level's width in this model, or 0 for an unknown level
int level_dim(const scann_handle* h, int32_t level) {
  return level == SCANN_OUT_BF_PROPERTY ? h->cfg.dense_out : level == SCANN_OUT_AFTER_LC ? h->cfg.global_dim : 0;
}
int check_level(scann_handle* h, const scann_index* ix, int32_t level, const char* who) {
  const int d = level_dim(h, level);
  if (!d) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got " + std::to_string(level));
  if (d != ix->dim)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": the index holds rows of " + std::to_string(ix->dim) + " columns, the model's " +
                                          (level == SCANN_OUT_BF_PROPERTY ? "dense_out" : "global_dim") + " is " + std::to_string(d));
  return SCANN_OK;
}

}  // namespace

namespace scann {

int index_new_chunk(scann_handle* h, scann_index* ix, hipStream_t s) {
  char* p = nullptr;
  HIPCHK(h, cached_malloc((void**)&p, ix->chunk_bytes()));
  ix->chunks.push_back(p);
  HIPCHK(h, hipMemsetAsync(p, 0, ix->chunk_bytes(), s));  // the padding columns are zero: fmaf(0, 0, acc) == acc
  return SCANN_OK;
}

void index_note_rows(scann_index* ix, int64_t n, const int64_t* ids, const int32_t* atoms) {
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
  int64_t done = 0;
  while (done < n) {
    const int64_t at = ix->n + done;
    const size_t c = (size_t)(at / ix->chunk_rows);
    const int64_t r0 = at % ix->chunk_rows, m = std::min<int64_t>(n - done, ix->chunk_rows - r0);
    if (c == ix->chunks.size())
      if (const int r = index_new_chunk(h, ix, s)) return r;
    HIPCHK(h, hipMemcpy2DAsync(ix->rows_of(c) + (size_t)r0 * ix->stride, (size_t)ix->stride * 4, static_cast<const char*>(src) + (size_t)done * pitch,
                               pitch, (size_t)ix->dim * 4, (size_t)m, kind, s));
    HIPCHK(h, hipMemcpyAsync(ix->ids_of(c) + r0, ids + done, (size_t)m * 8, hipMemcpyHostToDevice, s));
    done += m;
  }
  HIPCHK(h, hipStreamSynchronize(s));
  index_note_rows(ix, n, ids, atoms);
  return SCANN_OK;
}

// nq queries on the device ([nq][stride], padded like the rows; qid: device [nq] or null) against the whole index.  dev_d non-null: the
// distances [nq][k] are left there, on the device, and nothing comes back to the host (scann_index_select: the pool's rows against the
// reference, k = 1)
int search(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2, int64_t* ids,
           int32_t* atoms, int32_t* pos, float* dev_d = nullptr) {
  const int64_t N = ix->n;
  const int rpr = (int)std::max<int64_t>(TILE_TR, ((N + KNN_RANGES - 1) / KNN_RANGES + TILE_TR - 1) / TILE_TR * TILE_TR);
  // one launch over all chunks: every chunk is cut into the same number of ranges (those behind the last row stay empty)
  const int n_chunk = (int)((N + ix->chunk_rows - 1) / ix->chunk_rows);
  const int64_t n_range = (int64_t)n_chunk * ((std::min<int64_t>(N, ix->chunk_rows) + rpr - 1) / rpr);
  if (n_range > KNN_MAX_RANGES || n_chunk > 65535) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_index_query: the index has too many chunks");
  const int64_t g = std::min<int64_t>(nq, KNN_QGROUP);
  const size_t bP = align_up((size_t)std::max<int64_t>(g * n_range * k, 1) * 4), bO = align_up((size_t)g * k * 4),
               bT = align_up((size_t)std::max(n_chunk, 1) * 8);
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, 2 * bP + 2 * bO + 2 * bT));
  float* part_d = reinterpret_cast<float*>(ws);
  int32_t* part_p = reinterpret_cast<int32_t*>(ws + bP);
  float* out_d = reinterpret_cast<float*>(ws + 2 * bP);
  int32_t* out_p = reinterpret_cast<int32_t*>(ws + 2 * bP + bO);
  std::vector<const void*> tab((size_t)2 * std::max(n_chunk, 1), nullptr);  // the chunks' rows, then their ids
  for (int c = 0; c < n_chunk; ++c) tab[(size_t)c] = ix->rows_of((size_t)c), tab[(size_t)n_chunk + c] = ix->ids_of((size_t)c);
  std::vector<int32_t> pos_h(dev_d ? 0 : (size_t)nq * k);
  hipError_t e = hipSuccess;
  if (n_chunk > 0) {
    e = hipMemcpyAsync(ws + 2 * bP + 2 * bO, tab.data(), (size_t)n_chunk * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + 2 * bP + 2 * bO + bT, tab.data() + n_chunk, (size_t)n_chunk * 8, hipMemcpyHostToDevice, s);
  }
  for (int64_t q0 = 0; q0 < nq && e == hipSuccess; q0 += g) {
    const int m = (int)std::min<int64_t>(g, nq - q0);
    KnnArgs a{};
    a.rows = reinterpret_cast<const float* const*>(ws + 2 * bP + 2 * bO);
    a.ids = reinterpret_cast<const int64_t* const*>(ws + 2 * bP + 2 * bO + bT);
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
  cached_free(ws);
  HIPCHK(h, e);
  for (size_t i = 0; i < pos_h.size(); ++i) {
    const int32_t p = pos_h[i];
    if (pos) pos[i] = p;
    if (ids) ids[i] = p < 0 ? -1 : ix->ids[(size_t)p];
    if (atoms) atoms[i] = p < 0 ? -1 : ix->atoms[(size_t)p];
  }
  return SCANN_OK;
}

// nq queries of the index's width at q -- host rows (kind = hipMemcpyHostToDevice) or device rows -- and their ids (host [nq], or null) staged
// in one block of the cache and searched: the rows padded to the stride, then the ids.  Device rows whose width is the stride are searched
// where they lie.
int search_staged(scann_handle* h, scann_index* ix, const float* q, hipMemcpyKind kind, const int64_t* qid, int64_t nq, int k, hipStream_t s,
                  float* dist2, int64_t* ids, int32_t* atoms, int32_t* pos) {
  const bool pad = ix->stride != ix->dim, copy = pad || kind == hipMemcpyHostToDevice;
  const size_t bQ = copy ? align_up((size_t)nq * ix->stride * 4) : 0, bI = align_up((size_t)nq * 8);
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, bQ + bI));
  hipError_t e = pad ? hipMemsetAsync(ws, 0, bQ, s) : hipSuccess;
  if (e == hipSuccess && copy) e = hipMemcpy2DAsync(ws, (size_t)ix->stride * 4, q, (size_t)ix->dim * 4, (size_t)ix->dim * 4, (size_t)nq, kind, s);
  if (e == hipSuccess && qid) e = hipMemcpyAsync(ws + bQ, qid, (size_t)nq * 8, hipMemcpyHostToDevice, s);
  int r = SCANN_OK;
  if (e == hipSuccess)
    r = search(h, ix, copy ? reinterpret_cast<const float*>(ws) : q, qid ? reinterpret_cast<const int64_t*>(ws + bQ) : nullptr, nq, k, s, dist2, ids, atoms, pos);
  else
    (void)hipStreamSynchronize(s);
  cached_free(ws);
  HIPCHK(h, e);
  return r;
}

// The rows a batch has at a level -- one per structure, or (atom) one per atom in packed order -- named: id_v = the structure's id
// (ids[b]; ids null: first + b), at_v (if asked for) = the atom's index in its structure, -1 for a structure row
int expand_ids(scann_handle* h, const scann_dbatch* db, bool atom, const int64_t* ids, int64_t first, std::vector<int64_t>& id_v,
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

// dist2 of one vector to n rows, the chain above (with the host's fused multiply-add where it has one: the same bits)
void dist2_to_rows(const float* q, const float* rows, int64_t n, int64_t d, float* out) {
  if (__builtin_cpu_supports("fma")) dist2_matrix_fma(q, 1, rows, n, d, out);
  else dist2_matrix_plain(q, 1, rows, n, d, out);
}

// the places of a selection's outputs from `from` on: no pick
void select_tail(int64_t from, int64_t m, int32_t* pos, int64_t* ids, int32_t* atoms, float* radius2) {
  for (int64_t i = from; i < m; ++i) {
    pos[i] = -1;
    if (ids) ids[i] = -1;
    if (atoms) atoms[i] = -1;
    if (radius2) radius2[i] = __builtin_inff();
  }
}

}  // namespace

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
  ix->chunk_rows = (int32_t)std::max<size_t>(4096, ((size_t)64 << 20) / ((size_t)ix->stride * 4) / TILE_TR * TILE_TR);
  *out = ix;
  return SCANN_OK;
}

void scann_index_free(scann_handle_t* h, scann_index_t* ix) {
  if (!ix) return;
  (void)h;  // (the chunks go back to the device's block cache, which outlives the handle)
  if (hipSetDevice(ix->device) == hipSuccess) (void)hipDeviceSynchronize();
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
  for (int64_t done = 0; rows && done < n;) {
    const int64_t at = first + done;
    const size_t c = (size_t)(at / ix->chunk_rows);
    const int64_t r0 = at % ix->chunk_rows, m = std::min<int64_t>(n - done, ix->chunk_rows - r0);
    HIPCHK(h, hipMemcpy2D(rows + (size_t)done * ix->dim, (size_t)ix->dim * 4, ix->rows_of(c) + (size_t)r0 * ix->stride, (size_t)ix->stride * 4,
                          (size_t)ix->dim * 4, (size_t)m, hipMemcpyDeviceToHost));
    done += m;
  }
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
  return search_staged(h, ix, q, hipMemcpyHostToDevice, query_ids, nq, k, h->streams[0], dist2, ids, atoms, pos);
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
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int B = db->n_struct, A = db->n_atom;
  const int64_t nq = atom ? A : B;
  if (nq <= 0) return fail(h, SCANN_ERR_INVALID, "scann_index_query_batch: an empty query");
  if (!dist2) return fail(h, SCANN_ERR_INVALID, "scann_index_query_batch: dist2 is null");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_index_query_batch: weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  std::vector<int64_t> qid;
  if (query_ids)
    if (const int r = expand_ids(h, db, atom, query_ids, 0, qid, nullptr)) return r;
  // the level's rows are the queries where the forward left them
  return search_staged(h, ix, atom ? db->out_z : db->out_bf, hipMemcpyDeviceToDevice, query_ids ? qid.data() : nullptr, nq, k, h->streams[db->last_slot],
                       dist2, ids, atoms, pos);
}

int64_t scann_kcenter_host(const float* rows, int64_t n, const float* ref, int64_t nr, int64_t dim, int64_t m, float stop_dist2, int32_t* pos,
                           float* radius2) {
  if (n < 0 || nr < 0 || dim < 1 || m < 1 || stop_dist2 != stop_dist2 || !pos || (n > 0 && !rows) || (nr > 0 && !ref) || n > (int64_t)0x7fffffff)
    return SCANN_ERR_INVALID;
  select_tail(0, m, pos, nullptr, nullptr, radius2);
  if (n == 0) return 0;
  std::vector<float> mind((size_t)n, __builtin_inff()), tmp((size_t)std::max(n, nr));
  std::vector<char> live((size_t)n, 1);
  for (int64_t p = 0; p < n; ++p)
    for (int64_t j = 0; j < dim; ++j)
      if (!std::isfinite(rows[p * dim + j])) live[(size_t)p] = 0;
  for (int64_t p = 0; p < n && nr > 0; ++p) {
    if (!live[(size_t)p]) continue;
    dist2_to_rows(rows + p * dim, ref, nr, dim, tmp.data());
    for (int64_t r = 0; r < nr; ++r)  // a NaN distance never counts
      if (tmp[(size_t)r] < mind[(size_t)p]) mind[(size_t)p] = tmp[(size_t)r];
  }
  int64_t cnt = 0;
  while (cnt < m) {
    int64_t best = -1;
    for (int64_t p = 0; p < n; ++p)  // mind descending, position ascending
      if (live[(size_t)p] && (best < 0 || mind[(size_t)p] > mind[(size_t)best])) best = p;
    if (best < 0 || (stop_dist2 > 0.f && mind[(size_t)best] < stop_dist2)) break;
    pos[cnt] = (int32_t)best;
    if (radius2) radius2[cnt] = mind[(size_t)best];
    live[(size_t)best] = 0;
    if (++cnt == m) break;
    dist2_to_rows(rows + best * dim, rows, n, dim, tmp.data());
    for (int64_t p = 0; p < n; ++p)
      if (live[(size_t)p] && tmp[(size_t)p] < mind[(size_t)p]) mind[(size_t)p] = tmp[(size_t)p];
  }
  return cnt;
}

int64_t scann_index_select(scann_handle_t* h, scann_index_t* pool, scann_index_t* reference, int64_t m, float stop_dist2, int32_t* pos, int64_t* ids,
                           int32_t* atoms, float* radius2) {
  if (!h || !pool) return fail(h, SCANN_ERR_INVALID, "scann_index_select: null handle or pool");
  if (pool->h != h) return fail(h, SCANN_ERR_INVALID, "scann_index_select: the pool belongs to another handle");
  if (reference == pool) return fail(h, SCANN_ERR_INVALID, "scann_index_select: the reference is the pool itself");
  if (reference && reference->h != h) return fail(h, SCANN_ERR_INVALID, "scann_index_select: the reference belongs to another handle");
  if (reference && reference->dim != pool->dim)
    return fail(h, SCANN_ERR_INVALID, "scann_index_select: the pool holds rows of " + std::to_string(pool->dim) + " columns, the reference of " +
                                          std::to_string(reference->dim));
  if (m < 1) return fail(h, SCANN_ERR_INVALID, "scann_index_select: m " + std::to_string(m) + " is not >= 1");
  if (stop_dist2 != stop_dist2) return fail(h, SCANN_ERR_INVALID, "scann_index_select: stop_dist2 is NaN");
  if (!pos) return fail(h, SCANN_ERR_INVALID, "scann_index_select: pos is null");
  const int64_t N = pool->n;
  if (N > (int64_t)0x7fffffff - 2 * KC_LANES) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_index_select: the pool has too many rows");
  select_tail(0, m, pos, ids, atoms, radius2);
  if (N == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  KcArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = pool->stride;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  a.tiles_per_chunk = (pool->chunk_rows + KC_LANES - 1) / KC_LANES;
  a.n_tile = a.n_chunk * a.tiles_per_chunk;
  a.n_pick = (int32_t)std::min<int64_t>(m, N);
  a.stop = stop_dist2;
  const int groups = std::min(a.n_tile, KC_MAX_GROUPS);
  // one workspace for the call: the state (first: it is what the memset clears), mind, the picks, the candidates, the chunk table, live
  const size_t bS = 256, bM = align_up((size_t)N * 4), bO = align_up((size_t)a.n_pick * 4), bP = align_up((size_t)groups * 8),
               bT = align_up((size_t)a.n_chunk * 8), bL = align_up((size_t)N);
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, bS + bM + 2 * bO + bP + bT + bL));
  a.st = reinterpret_cast<KcState*>(ws);
  a.mind = reinterpret_cast<float*>(ws + bS);
  a.out_pos = reinterpret_cast<int32_t*>(ws + bS + bM);
  a.out_r2 = reinterpret_cast<float*>(ws + bS + bM + bO);
  a.part = reinterpret_cast<unsigned long long*>(ws + bS + bM + 2 * bO);
  a.rows = reinterpret_cast<const float* const*>(ws + bS + bM + 2 * bO + bP);
  a.live = reinterpret_cast<uint8_t*>(ws + bS + bM + 2 * bO + bP + bT);
  std::vector<const void*> tab((size_t)a.n_chunk);
  for (int c = 0; c < a.n_chunk; ++c) tab[(size_t)c] = pool->rows_of((size_t)c);
  const bool has_ref = reference && reference->n > 0;
  int r = SCANN_OK;
  hipError_t e = hipMemsetAsync(ws, 0, sizeof(KcState), s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + bS + bM + 2 * bO + bP, tab.data(), (size_t)a.n_chunk * 8, hipMemcpyHostToDevice, s);
  // the initial mind: the k = 1 query of the pool's own rows, chunk by chunk where they lie, against the reference
  for (int c = 0; c < a.n_chunk && has_ref && e == hipSuccess && !r; ++c)
    r = search(h, reference, pool->rows_of((size_t)c), nullptr, std::min<int64_t>(pool->chunk_rows, N - (int64_t)c * pool->chunk_rows), 1, s, nullptr,
               nullptr, nullptr, nullptr, a.mind + (size_t)c * pool->chunk_rows);
  if (e == hipSuccess && !r) e = launch_kcenter_prepare(a, has_ref, s);
  // every pick is enqueued at once: a pick reads its predecessor's position, and whether the selection has ended, from device memory
  for (int i = 0; i < a.n_pick && e == hipSuccess && !r; ++i) e = launch_kcenter_step(a, groups, s);
  KcState st{};
  std::vector<int32_t> pos_h((size_t)a.n_pick);
  std::vector<float> r2_h((size_t)a.n_pick);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(pos_h.data(), a.out_pos, (size_t)a.n_pick * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(r2_h.data(), a.out_r2, (size_t)a.n_pick * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(&st, a.st, sizeof(KcState), hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  cached_free(ws);
  if (r) return r;
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  const int64_t cnt = std::min<int64_t>(std::max<int32_t>(st.count, 0), a.n_pick);
  for (int64_t i = 0; i < cnt; ++i) {
    const int32_t p = pos_h[(size_t)i];
    pos[i] = p;
    if (ids) ids[i] = pool->ids[(size_t)p];
    if (atoms) atoms[i] = pool->atoms[(size_t)p];
    if (radius2) radius2[i] = r2_h[(size_t)i];
  }
  return cnt;
}

// frexp's exponent of a column's largest |x| (0 for a column of zeros): the scale of the update's integer sums
static int kmeans_exponent(float m) {
  int e = 0;
  if (m > 0.f) (void)std::frexp(m, &e);
  return e;
}

int64_t scann_kmeans_host(const float* rows, int64_t n, int64_t dim, int32_t k, const float* init, int32_t max_iter, int64_t stop_changed,
                          int32_t* labels, float* dist2, float* centres, int64_t* sizes, int32_t* converged) {
  if (n < 0 || n > (int64_t)0x7fffffff || dim < 1 || k < 1 || k > SCANN_KMEANS_MAX_K || !init || max_iter < 0 || stop_changed < 0 || !centres ||
      (n > 0 && (!rows || !labels)))
    return SCANN_ERR_INVALID;
  for (int64_t i = 0; i < (int64_t)k * dim; ++i)
    if (!std::isfinite(init[i])) return SCANN_ERR_INVALID;
  std::copy(init, init + (int64_t)k * dim, centres);
  std::vector<char> elig((size_t)n, 1);
  std::vector<int> ex((size_t)dim, 0);
  {
    std::vector<float> mx((size_t)dim, 0.f);
    for (int64_t p = 0; p < n; ++p) {
      for (int64_t j = 0; j < dim; ++j)
        if (!std::isfinite(rows[p * dim + j])) elig[(size_t)p] = 0;
      for (int64_t j = 0; j < dim && elig[(size_t)p]; ++j) mx[(size_t)j] = std::max(mx[(size_t)j], std::fabs(rows[p * dim + j]));
    }
    for (int64_t j = 0; j < dim; ++j) ex[(size_t)j] = kmeans_exponent(mx[(size_t)j]);
  }
  std::vector<int32_t> lab((size_t)n, -1);
  std::vector<float> d2((size_t)n, __builtin_inff()), tmp((size_t)k);
  std::vector<int64_t> sum((size_t)k * dim), cnt((size_t)k);
  int32_t t = 0;
  bool conv = false;
  for (;; ++t) {
    int64_t changed = 0;
    for (int64_t p = 0; p < n; ++p) {
      if (!elig[(size_t)p]) continue;
      dist2_to_rows(rows + p * dim, centres, k, dim, tmp.data());  // the row first
      int32_t best = -1;
      for (int32_t c = 0; c < k; ++c)  // dist2 ascending, index ascending; a NaN distance never qualifies
        if (tmp[(size_t)c] == tmp[(size_t)c] && (best < 0 || tmp[(size_t)c] < tmp[(size_t)best])) best = c;
      changed += best != lab[(size_t)p];
      lab[(size_t)p] = best;
      d2[(size_t)p] = best < 0 ? __builtin_inff() : tmp[(size_t)best];
    }
    conv = changed <= stop_changed;
    if (conv || t == max_iter) break;
    std::fill(sum.begin(), sum.end(), 0);
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int64_t p = 0; p < n; ++p) {
      const int32_t c = lab[(size_t)p];
      if (c < 0) continue;
      ++cnt[(size_t)c];
      for (int64_t j = 0; j < dim; ++j) sum[(size_t)c * dim + j] += std::llrint(std::ldexp((double)rows[p * dim + j], 30 - ex[(size_t)j]));
    }
    for (int32_t c = 0; c < k; ++c)
      for (int64_t j = 0; j < dim && cnt[(size_t)c] > 0; ++j)
        centres[(int64_t)c * dim + j] = (float)std::ldexp((double)sum[(size_t)c * dim + j] / (double)cnt[(size_t)c], ex[(size_t)j] - 30);
  }
  if (n > 0) std::copy(lab.begin(), lab.end(), labels);
  if (dist2 && n > 0) std::copy(d2.begin(), d2.end(), dist2);
  if (sizes) {
    std::fill(sizes, sizes + k, 0);
    for (int64_t p = 0; p < n; ++p)
      if (lab[(size_t)p] >= 0) ++sizes[lab[(size_t)p]];
  }
  if (converged) *converged = conv ? 1 : 0;
  return t;
}

int64_t scann_index_kmeans(scann_handle_t* h, scann_index_t* pool, int32_t k, const float* init, const int32_t* init_pos, int32_t max_iter,
                           int64_t stop_changed, int32_t* labels, float* dist2, float* centres, int64_t* sizes, int32_t* converged) {
  if (!h || !pool) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: null handle or pool");
  if (pool->h != h) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: the pool belongs to another handle");
  if (k < 1 || k > SCANN_KMEANS_MAX_K)
    return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: k " + std::to_string(k) + " outside 1 .. " + std::to_string(SCANN_KMEANS_MAX_K));
  if ((init != nullptr) == (init_pos != nullptr))
    return fail(h, SCANN_ERR_INVALID, std::string("scann_index_kmeans: exactly one of init and init_pos must be given, got ") + (init ? "both" : "neither"));
  if (max_iter < 0) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: max_iter " + std::to_string(max_iter) + " is negative");
  if (stop_changed < 0) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: stop_changed " + std::to_string(stop_changed) + " is negative");
  if (!labels) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: labels is null");
  if (!centres) return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: centres is null");
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride;
  if (N > (int64_t)0x7fffffff - 1024) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_index_kmeans: the pool has too many rows");
  for (int64_t i = 0; init && i < (int64_t)k * dim; ++i)
    if (!std::isfinite(init[i]))
      return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: init holds a non-finite value (centre " + std::to_string(i / dim) + ", column " +
                                            std::to_string(i % dim) + ")");
  for (int32_t c = 0; init_pos && c < k; ++c)
    if (init_pos[c] < 0 || init_pos[c] >= N)
      return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: init_pos[" + std::to_string(c) + "] = " + std::to_string(init_pos[c]) + " outside the pool's " +
                                            std::to_string(N) + " rows");
  if (N == 0) {  // (init: init_pos has nothing to point at)
    std::copy(init, init + (int64_t)k * dim, centres);
    if (sizes) std::fill(sizes, sizes + k, 0);
    if (converged) *converged = 1;
    return 0;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  KmArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride; a.dim = dim; a.k = k;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  a.tiles_per_chunk = (pool->chunk_rows + KM_TP - 1) / KM_TP;
  a.n_tile = a.n_chunk * a.tiles_per_chunk;
  a.max_iter = max_iter; a.stop_changed = stop_changed;
  // one workspace for the call.  First what the memset clears: the state, the column maxima, the counts, the sums; then the centres,
  // the initial positions, the chunk table, labels, dist2 and the eligibility bytes
  const size_t bS = align_up(sizeof(KmState)), bX = align_up((size_t)stride * 4), bN = align_up((size_t)k * 4), bU = align_up((size_t)k * stride * 8),
               bC = align_up((size_t)k * stride * 4), bT = align_up((size_t)a.n_chunk * 8), bL = align_up((size_t)N * 4), bE = align_up((size_t)N);
  const size_t zeroed = bS + bX + bN + bU + bC;  // (the centres' padding columns are zero)
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, zeroed + bN + bT + 2 * bL + bE));
  a.st = reinterpret_cast<KmState*>(ws);
  a.colmax = reinterpret_cast<uint32_t*>(ws + bS);
  a.counts = reinterpret_cast<uint32_t*>(ws + bS + bX);
  a.sums = reinterpret_cast<unsigned long long*>(ws + bS + bX + bN);
  a.centres = reinterpret_cast<float*>(ws + bS + bX + bN + bU);
  int32_t* d_pos = reinterpret_cast<int32_t*>(ws + zeroed);
  a.init_pos = init_pos ? d_pos : nullptr;
  a.rows = reinterpret_cast<const float* const*>(ws + zeroed + bN);
  a.labels = reinterpret_cast<int32_t*>(ws + zeroed + bN + bT);
  a.dist2 = reinterpret_cast<float*>(ws + zeroed + bN + bT + bL);
  a.elig = reinterpret_cast<uint8_t*>(ws + zeroed + bN + bT + 2 * bL);
  std::vector<const void*> tab((size_t)a.n_chunk);
  for (int c = 0; c < a.n_chunk; ++c) tab[(size_t)c] = pool->rows_of((size_t)c);
  hipError_t e = hipMemsetAsync(ws, 0, zeroed, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + zeroed + bN, tab.data(), (size_t)a.n_chunk * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && init) e = hipMemcpy2DAsync(a.centres, (size_t)stride * 4, init, (size_t)dim * 4, (size_t)dim * 4, (size_t)k, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && init_pos) e = hipMemcpyAsync(d_pos, init_pos, (size_t)k * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_kmeans_prepare(a, s);
  if (e == hipSuccess) e = launch_kmeans_gather(a, s);  // (init_pos: the centres never leave the device)
  // every round is enqueued at once: whether the loop has ended travels from launch to launch through device memory.  (The state holds
  // KM_ROUNDS counters: a longer run waits after that many rounds and clears them.)
  KmState st{};
  for (int64_t t0 = 0; t0 <= max_iter && e == hipSuccess; t0 += KM_ROUNDS) {
    if (t0 > 0) e = hipMemsetAsync(reinterpret_cast<char*>(a.st) + offsetof(KmState, changed), 0, sizeof(st.changed), s);
    for (int64_t t = t0; t <= max_iter && t < t0 + KM_ROUNDS && e == hipSuccess; ++t) e = launch_kmeans_round(a, (int)t, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(KmState), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (st.done) break;
  }
  const bool ok = e == hipSuccess && st.done && !st.bad_init;
  if (ok) e = hipMemcpyAsync(labels, a.labels, (size_t)N * 4, hipMemcpyDeviceToHost, s);
  if (ok && e == hipSuccess && dist2) e = hipMemcpyAsync(dist2, a.dist2, (size_t)N * 4, hipMemcpyDeviceToHost, s);
  if (ok && e == hipSuccess)
    e = hipMemcpy2DAsync(centres, (size_t)dim * 4, a.centres, (size_t)stride * 4, (size_t)dim * 4, (size_t)k, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);
  cached_free(ws);
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  if (st.bad_init) {
    const int32_t c = k - st.bad_init;
    return fail(h, SCANN_ERR_INVALID, "scann_index_kmeans: init_pos[" + std::to_string(c) + "] = " + std::to_string(init_pos[c]) +
                                          " names a row with a non-finite component");
  }
  if (!st.done) return fail(h, SCANN_ERR_HIP, "scann_index_kmeans: the loop did not end");
  if (sizes) {
    std::fill(sizes, sizes + k, 0);
    for (int64_t p = 0; p < N; ++p)
      if (labels[p] >= 0) ++sizes[labels[p]];
  }
  if (converged) *converged = st.converged;
  return st.n_iter;
}

// ---- principal-component map (scann_pca.hip; the twins and the eigen-decomposition are in scann_pca.cpp) ----

int scann_index_moments(scann_handle_t* h, scann_index_t* pool, int64_t* n_eligible, float* mean, double* cov, int32_t* col_exp, int32_t* bits) {
  if (!h || !pool) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: null handle or pool");
  if (pool->h != h) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: the pool belongs to another handle");
  if (!n_eligible) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: n_eligible is null");
  if (!mean) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: mean is null");
  if (!cov) return fail(h, SCANN_ERR_INVALID, "scann_index_moments: cov is null");
  const int64_t N = pool->n;
  const int32_t dim = pool->dim, stride = pool->stride;
  if (N > (int64_t)0x7fffffff - 1024) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_index_moments: the pool has too many rows");
  if (N == 0) {
    *n_eligible = 0;
    return fail(h, SCANN_ERR_INVALID, "scann_index_moments: a covariance needs at least 2 rows, the pool has 0");
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  PcaArgs a{};
  a.n_total = (int32_t)N; a.chunk_rows = pool->chunk_rows; a.stride = stride; a.dim = dim;
  a.n_chunk = (int)((N + pool->chunk_rows - 1) / pool->chunk_rows);
  // one workspace for the call.  First what the memset clears: the state, the two column maxima, S, R and T; then the mean, the
  // covariance, f, the chunk table and the eligibility bytes
  const size_t bS = align_up(sizeof(PcaState)), bX = align_up((size_t)stride * 4), bU = align_up((size_t)stride * 8),
               bT = align_up((size_t)stride * stride * 8), bC = align_up((size_t)dim * dim * 8), bP = align_up((size_t)a.n_chunk * 8),
               bE = align_up((size_t)N);
  const size_t zeroed = bS + 2 * bX + 2 * bU + bT;
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, zeroed + 2 * bX + bC + bP + bE));
  a.st = reinterpret_cast<PcaState*>(ws);
  a.colmax = reinterpret_cast<uint32_t*>(ws + bS);
  a.cenmax = reinterpret_cast<uint32_t*>(ws + bS + bX);
  a.sums = reinterpret_cast<unsigned long long*>(ws + bS + 2 * bX);
  a.R = reinterpret_cast<unsigned long long*>(ws + bS + 2 * bX + bU);
  a.T = reinterpret_cast<unsigned long long*>(ws + bS + 2 * bX + 2 * bU);
  a.mean = reinterpret_cast<float*>(ws + zeroed);
  a.col_exp = reinterpret_cast<int32_t*>(ws + zeroed + bX);
  a.cov = reinterpret_cast<double*>(ws + zeroed + 2 * bX);
  a.rows = reinterpret_cast<const float* const*>(ws + zeroed + 2 * bX + bC);
  a.elig = reinterpret_cast<uint8_t*>(ws + zeroed + 2 * bX + bC + bP);
  std::vector<const void*> tab((size_t)a.n_chunk);
  for (int c = 0; c < a.n_chunk; ++c) tab[(size_t)c] = pool->rows_of((size_t)c);
  PcaState st{};
  std::vector<float> mean_h((size_t)dim);
  std::vector<double> cov_h((size_t)dim * dim);
  std::vector<int32_t> exp_h((size_t)dim);
  hipError_t e = hipMemsetAsync(ws, 0, zeroed, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + zeroed + 2 * bX + bC, tab.data(), (size_t)a.n_chunk * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_pca_moments(a, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&st, a.st, sizeof(PcaState), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(mean_h.data(), a.mean, (size_t)dim * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(cov_h.data(), a.cov, (size_t)dim * dim * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(exp_h.data(), a.col_exp, (size_t)dim * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e_sync = hipStreamSynchronize(s);  // the call's one wait
  cached_free(ws);
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  *n_eligible = st.n;
  if (st.n < 2)
    return fail(h, SCANN_ERR_INVALID, "scann_index_moments: a covariance needs at least 2 rows without a non-finite component, the pool has " +
                                          std::to_string(st.n) + " among its " + std::to_string(N));
  std::copy(mean_h.begin(), mean_h.end(), mean);
  std::copy(cov_h.begin(), cov_h.end(), cov);
  if (col_exp) std::copy(exp_h.begin(), exp_h.end(), col_exp);
  if (bits) *bits = scann_pca_bits(st.n);
  return SCANN_OK;
}

}  // extern "C"

namespace {

// the arguments of a projection onto rows of `dim` columns
int check_projection(scann_handle* h, const char* who, int64_t dim, const float* mean, const float* components, const float* scale, int32_t m,
                     const float* coords, const float* md2) {
  const std::string w(who);
  if (m < 1 || m > dim) return fail(h, SCANN_ERR_INVALID, w + ": m " + std::to_string(m) + " outside 1 .. " + std::to_string(dim));
  if (!mean) return fail(h, SCANN_ERR_INVALID, w + ": mean is null");
  if (!components) return fail(h, SCANN_ERR_INVALID, w + ": components is null");
  if (!coords) return fail(h, SCANN_ERR_INVALID, w + ": coords is null");
  if (md2 && !scale) return fail(h, SCANN_ERR_INVALID, w + ": md2 needs scale, which is null");
  for (int64_t j = 0; j < dim; ++j)
    if (!std::isfinite(mean[j])) return fail(h, SCANN_ERR_INVALID, w + ": mean holds a non-finite value (column " + std::to_string(j) + ")");
  for (int64_t i = 0; i < (int64_t)m * dim; ++i)
    if (!std::isfinite(components[i]))
      return fail(h, SCANN_ERR_INVALID, w + ": components hold a non-finite value (component " + std::to_string(i / dim) + ", column " +
                                            std::to_string(i % dim) + ")");
  for (int32_t c = 0; scale && c < m; ++c)
    if (!std::isfinite(scale[c])) return fail(h, SCANN_ERR_INVALID, w + ": scale holds a non-finite value (component " + std::to_string(c) + ")");
  return SCANN_OK;
}

// rows [first, first + n) of the chunks in `tab` ([chunk_rows][stride] each, the padding zero) projected; the outputs are host arrays.
// The coordinates pass through a device block of at most 256 MiB, a group of rows at a time
int project_rows(scann_handle* h, const std::vector<const void*>& tab, int32_t chunk_rows, int32_t stride, int32_t dim, int64_t first, int64_t n,
                 const float* mean, const float* components, const float* scale, int32_t m, float* coords, float* md2, float* dist2, hipStream_t s) {
  if (n <= 0) return SCANN_OK;
  const int64_t g = std::min<int64_t>(n, std::max<int64_t>(PCA_TP, (((int64_t)256 << 20) / ((int64_t)m * 4)) / PCA_TP * PCA_TP));
  const size_t bM = align_up((size_t)stride * 4), bW = align_up((size_t)m * stride * 4), bS = align_up((size_t)m * 4), bP = align_up(tab.size() * 8),
               bZ = align_up((size_t)g * m * 4), bD = align_up((size_t)g * 4);
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, bM + bW + bS + bP + bZ + 2 * bD));
  PcaProjArgs a{};
  a.rows = reinterpret_cast<const float* const*>(ws + bM + bW + bS);
  a.chunk_rows = chunk_rows; a.stride = stride; a.dim = dim; a.m = m;
  a.mean = reinterpret_cast<const float*>(ws);
  a.comp = reinterpret_cast<const float*>(ws + bM);
  a.scale = reinterpret_cast<const float*>(ws + bM + bW);
  a.coords = reinterpret_cast<float*>(ws + bM + bW + bS + bP);
  a.md2 = md2 ? reinterpret_cast<float*>(ws + bM + bW + bS + bP + bZ) : nullptr;
  a.dist2 = dist2 ? reinterpret_cast<float*>(ws + bM + bW + bS + bP + bZ + bD) : nullptr;
  hipError_t e = hipMemsetAsync(ws, 0, bM + bW + bS, s);  // (the padding columns of the mean and of the components are zero)
  if (e == hipSuccess) e = hipMemcpyAsync(ws, mean, (size_t)dim * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(ws + bM, (size_t)stride * 4, components, (size_t)dim * 4, (size_t)dim * 4, (size_t)m, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && scale) e = hipMemcpyAsync(ws + bM + bW, scale, (size_t)m * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + bM + bW + bS, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s);
  for (int64_t r0 = 0; r0 < n && e == hipSuccess; r0 += g) {
    const int64_t cnt = std::min<int64_t>(g, n - r0);
    a.first = (int32_t)(first + r0); a.n = (int32_t)cnt;
    e = launch_pca_project(a, s);  // (the stream orders a group behind the copies of the one before)
    if (e == hipSuccess) e = hipMemcpyAsync(coords + (size_t)r0 * m, a.coords, (size_t)cnt * m * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && md2) e = hipMemcpyAsync(md2 + r0, a.md2, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && dist2) e = hipMemcpyAsync(dist2 + r0, a.dist2, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
  }
  const hipError_t e_sync = hipStreamSynchronize(s);
  cached_free(ws);
  HIPCHK(h, e);
  HIPCHK(h, e_sync);
  return SCANN_OK;
}

}  // namespace

extern "C" {

int scann_index_project(scann_handle_t* h, scann_index_t* pool, int64_t first, int64_t n, const float* mean, const float* components,
                        const float* scale, int32_t m, float* coords, float* md2, float* dist2) {
  if (!h || !pool) return fail(h, SCANN_ERR_INVALID, "scann_index_project: null handle or pool");
  if (pool->h != h) return fail(h, SCANN_ERR_INVALID, "scann_index_project: the pool belongs to another handle");
  if (first < 0 || n < 0 || first + n > pool->n)
    return fail(h, SCANN_ERR_INVALID, "scann_index_project: rows " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " + std::to_string(pool->n));
  if (const int r = check_projection(h, "scann_index_project", pool->dim, mean, components, scale, m, coords, md2)) return r;
  if (n == 0) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<const void*> tab(pool->chunks.size());
  for (size_t c = 0; c < tab.size(); ++c) tab[c] = pool->rows_of(c);
  return project_rows(h, tab, pool->chunk_rows, pool->stride, pool->dim, first, n, mean, components, scale, m, coords, md2, dist2, h->streams[0]);
}

int scann_project_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* components, const float* scale,
                        int32_t m, float* y, float* ga, float* coords, float* md2, float* dist2) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_project_batch: null handle or batch");
  const int dim = level_dim(h, level);
  if (!dim) return fail(h, SCANN_ERR_INVALID, "scann_project_batch: level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got " + std::to_string(level));
  if (const int r = check_projection(h, "scann_project_batch", dim, mean, components, scale, m, coords, md2)) return r;
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_project_batch: weights not loaded");
  const bool atom = level == SCANN_OUT_AFTER_LC;
  const int64_t nq = atom ? db->n_atom : db->n_struct;
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = forward_and_download(h, db, 0, level, y, ga)) return r;
  if (nq <= 0) return SCANN_OK;
  hipStream_t s = h->streams[db->last_slot];
  const float* src = atom ? db->out_z : db->out_bf;  // the level's rows where the forward left them
  const int stride = (dim + 3) / 4 * 4;
  char* pad = nullptr;
  if (stride != dim) {  // rows of the padded width, as an index keeps them
    HIPCHK(h, cached_malloc((void**)&pad, align_up((size_t)nq * stride * 4)));
    hipError_t e = hipMemsetAsync(pad, 0, (size_t)nq * stride * 4, s);
    if (e == hipSuccess) e = hipMemcpy2DAsync(pad, (size_t)stride * 4, src, (size_t)dim * 4, (size_t)dim * 4, (size_t)nq, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s);
      cached_free(pad);
      HIPCHK(h, e);
    }
    src = reinterpret_cast<const float*>(pad);
  }
  const std::vector<const void*> tab(1, src);
  const int r = project_rows(h, tab, 0x7fffffff, stride, dim, 0, nq, mean, components, scale, m, coords, md2, dist2, s);
  if (pad) cached_free(pad);
  return r;
}

}  // extern "C"

// ---- structure matching (scann_match.hip): the k nearest segments of every query structure, both taken as sets of rows ----

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
  // one workspace for the call
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += align_up(std::max<size_t>(bytes, 1)); return o; };
  const size_t oPd = take((size_t)g_sets * n_range * k * 4), oPp = take((size_t)g_sets * n_range * k * 4), oOd = take((size_t)n_pair * 4),
               oOp = take((size_t)n_pair * 4), oRows = take((size_t)n_chunk * 8), oIds = take((size_t)n_chunk * 8), oQf = take((size_t)(n_sets + 1) * 4),
               oQid = take((size_t)n_sets * 8), oTiles = take(tiles.size() * 4), oRanges = take(ranges.size() * 4), oSf = take((size_t)n_pair * 4),
               oSc = take((size_t)n_pair * 4), oParts = take((size_t)n_pair * 16), oMp = take((size_t)nq * k * 4), oMd = take((size_t)nq * k * 4);
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, at));
  std::vector<const void*> tab((size_t)2 * n_chunk);
  for (int c = 0; c < n_chunk; ++c) tab[(size_t)c] = ix->rows_of((size_t)c), tab[(size_t)n_chunk + c] = ix->ids_of((size_t)c);
  std::vector<int32_t> seg_h((size_t)n_pair), pf((size_t)n_pair, 0), pc((size_t)n_pair, 0), pos_h;
  std::vector<float> parts_h, md_h;
  hipError_t e = hipMemcpyAsync(ws + oRows, tab.data(), (size_t)n_chunk * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + oIds, tab.data() + n_chunk, (size_t)n_chunk * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + oQf, q_first, (size_t)(n_sets + 1) * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && qid) e = hipMemcpyAsync(ws + oQid, qid, (size_t)n_sets * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + oTiles, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + oRanges, ranges.data(), ranges.size() * 4, hipMemcpyHostToDevice, s);
  MatchArgs a{};
  a.rows = reinterpret_cast<const float* const*>(ws + oRows);
  a.ids = reinterpret_cast<const int64_t* const*>(ws + oIds);
  a.chunk_rows = ix->chunk_rows; a.stride = ix->stride; a.q = dq;
  a.q_first = reinterpret_cast<const int32_t*>(ws + oQf);
  a.qid = qid ? reinterpret_cast<const int64_t*>(ws + oQid) : nullptr;
  a.ranges = reinterpret_cast<const int32_t*>(ws + oRanges);
  a.n_range = n_range; a.k = k; a.measure = measure; a.sets_ld = most_sets <= MT_SETS_SMALL ? MT_SETS_SMALL : MT_SETS;
  a.part_d = reinterpret_cast<float*>(ws + oPd);
  a.part_p = reinterpret_cast<int32_t*>(ws + oPp);
  float* out_d = reinterpret_cast<float*>(ws + oOd);
  int32_t* out_p = reinterpret_cast<int32_t*>(ws + oOp);
  for (int t0 = 0; t0 < n_tile && e == hipSuccess;) {  // a group of tiles: at most MATCH_SET_GROUP structures (a tile holds at most MT_SETS)
    int t1 = t0 + 1;
    while (t1 < n_tile && tiles[(size_t)2 * t1 + 1] - tiles[(size_t)2 * t0] <= g_sets) ++t1;
    const int set0 = tiles[(size_t)2 * t0], set1 = tiles[(size_t)2 * t1 - 1];
    a.tiles = reinterpret_cast<const int32_t*>(ws + oTiles) + 2 * t0;
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
    MatchPairArgs p{};
    p.rows = a.rows; p.chunk_rows = ix->chunk_rows; p.stride = ix->stride; p.q = dq; p.q_first = a.q_first;
    p.seg_first = reinterpret_cast<const int32_t*>(ws + oSf);
    p.seg_count = reinterpret_cast<const int32_t*>(ws + oSc);
    p.n_sets = (int32_t)n_sets; p.k = k;
    p.parts = reinterpret_cast<float*>(ws + oParts);
    p.match_pos = reinterpret_cast<int32_t*>(ws + oMp);
    p.match_d = reinterpret_cast<float*>(ws + oMd);
    parts_h.resize((size_t)n_pair * 4);
    pos_h.resize((size_t)nq * k);
    md_h.resize((size_t)nq * k);
    e = hipMemcpyAsync(ws + oSf, pf.data(), (size_t)n_pair * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + oSc, pc.data(), (size_t)n_pair * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_match_pair(p, s);
    if (e == hipSuccess) e = hipMemcpyAsync(parts_h.data(), p.parts, (size_t)n_pair * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pos_h.data(), p.match_pos, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(md_h.data(), p.match_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s);
  }
  const hipError_t e_sync = hipStreamSynchronize(s);
  cached_free(ws);
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

// as search_staged: host or device query rows of the index's width staged at the padded width, then matched
int match_staged(scann_handle* h, scann_index* ix, const float* q, hipMemcpyKind kind, const int32_t* q_first, int64_t n_sets, const int64_t* qid,
                 int measure, int k, hipStream_t s, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos,
                 float* match_d) {
  const int64_t nq = q_first[n_sets];
  const bool pad = ix->stride != ix->dim, copy = pad || kind == hipMemcpyHostToDevice;
  char* ws = nullptr;
  if (copy) HIPCHK(h, cached_malloc((void**)&ws, align_up((size_t)nq * ix->stride * 4)));
  hipError_t e = pad ? hipMemsetAsync(ws, 0, (size_t)nq * ix->stride * 4, s) : hipSuccess;
  if (e == hipSuccess && copy) e = hipMemcpy2DAsync(ws, (size_t)ix->stride * 4, q, (size_t)ix->dim * 4, (size_t)ix->dim * 4, (size_t)nq, kind, s);
  int r = SCANN_OK;
  if (e == hipSuccess)
    r = match_search(h, ix, copy ? reinterpret_cast<const float*>(ws) : q, q_first, n_sets, qid, measure, k, s, score, segment, ids, sizes, parts,
                     match_pos, match_d);
  else
    (void)hipStreamSynchronize(s);
  if (ws) cached_free(ws);
  HIPCHK(h, e);
  return r;
}

}  // namespace

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

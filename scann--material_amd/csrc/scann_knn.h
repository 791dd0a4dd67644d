// Internal declarations of the latent-space nearest-neighbour search (scann_knn.hip, scann_knn.cpp); the C ABI is include/scann_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "scann_tile.h"

struct scann_handle;
struct scann_dbatch;
namespace scann {
struct CellPart;  // scann_cells.h
}

// A latent-space index (scann_knn.cpp; scann_head.cpp reads it as well)
struct scann_index {
  scann_handle* h = nullptr;
  int device = 0;
  int32_t dim = 0, stride = 0;  // stride: dim rounded up to a multiple of 4, the rest zero
  int32_t chunk_rows = 0;       // rows per chunk (a multiple of 64): about 64 MiB of rows
  int64_t n = 0;
  std::vector<char*> chunks;    // device blocks of the handle's cache: rows [chunk_rows][stride] fp32, then ids [chunk_rows] int64
  std::vector<int64_t> ids;     // host copies: what the calls report by position
  std::vector<int32_t> atoms;
  std::vector<int32_t> seg_first;  // first position of every segment: a maximal run of consecutive rows with one id (scann_index_match)
  scann::CellPart* part = nullptr;  // the partition into cells (scann_index_partition), or none: only search() reads it
  int64_t stats[4] = {0, 0, 0, 0};  // the last search (scann_index_search_stats)
  float* rows_of(size_t c) const { return reinterpret_cast<float*>(chunks[c]); }
  int64_t* ids_of(size_t c) const { return reinterpret_cast<int64_t*>(chunks[c] + (size_t)chunk_rows * stride * 4); }
  size_t chunk_bytes() const { return (size_t)chunk_rows * stride * 4 + (size_t)chunk_rows * 8; }
};

namespace scann {

// How an index grows (scann_knn.cpp): one more chunk from the handle's cache behind the last, cleared on stream s; and, once n rows have
// been written behind the index's rows and their device ids, the host side of the append (ids, atoms, segments, n)
int index_new_chunk(scann_handle* h, scann_index* ix, hipStream_t s);
void index_note_rows(scann_index* ix, int64_t n, const int64_t* ids, const int32_t* atoms);

// What the analyses over an index (scann_select.cpp, scann_kmeans.cpp, scann_match.cpp) use of scann_knn.cpp.  The opening checks of a
// search ("<who>: null argument", ...; 0: fine); search: nq queries on the device ([nq][stride], padded like the rows; dqid: device [nq] or
// null) against the whole index, synchronous -- dev_d non-null: the distances [nq][k] stay there, on the device, and nothing comes back to
// the host; dist2_to_rows: the host twin's distance chain of one vector to n rows
constexpr int KNN_RANGES = 1024;  // about as many row ranges, i.e. workgroups per 128 queries, as this
int check_index(scann_handle* h, const scann_index* ix, const char* who);
int check_k(scann_handle* h, int32_t k, const char* who);
int search(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2, int64_t* ids,
           int32_t* atoms, int32_t* pos, float* dev_d = nullptr);
int search_full(scann_handle* h, scann_index* ix, const float* dq, const int64_t* dqid, int64_t nq, int k, hipStream_t s, float* dist2, int64_t* ids,
                int32_t* atoms, int32_t* pos, float* dev_d = nullptr);  // search() of an index without a partition, whether it has one or not
void dist2_to_rows(const float* q, const float* rows, int64_t n, int64_t d, float* out);
// the rows a batch has at a level (one per structure, or with `atom` one per atom in packed order) named: id_v = the structure's id
// (ids[b]; ids null: first + b), at_v (if asked for) = the atom's index in its structure, -1 for a structure row
int expand_ids(scann_handle* h, const scann_dbatch* db, bool atom, const int64_t* ids, int64_t first, std::vector<int64_t>& id_v,
               std::vector<int32_t>* at_v);

// One launch of knn_tile_kernel: `nq` queries against all `n_total` rows of an index, stored in chunks of `chunk_rows` rows.  Workgroup
// (x, y, z) takes queries [128 y, 128 y + 128) and rows [x * rows_per_range, (x + 1) * rows_per_range) of chunk z and leaves the range's
// k best under the order (dist2, position) in part_d / part_p [query][n_range][k], range = z * gridDim.x + x; unused places (and the
// ranges behind the last row) hold (+inf, -1).
struct KnnArgs {
  const float* const* rows;    // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  const int64_t* const* ids;   // [n_chunk] -> [chunk_rows] (read with qid only)
  int32_t n_total, chunk_rows, n_chunk, stride;
  const float* q;       // [nq][stride], padded like the rows
  const int64_t* qid;   // [nq] or null: rows with ids[r] == qid[query] are skipped
  int32_t nq, k, rows_per_range;
  float* part_d;
  int32_t* part_p;
  int32_t n_range;      // n_chunk * ranges per chunk
};
size_t knn_lds_bytes(int k);
hipError_t launch_knn_tile(const KnnArgs& a, hipStream_t s);
// per query: the k first of its n_range partial lists under (dist2, position) -> out_d / out_p [nq][k]; the tail is (+inf, -1)
hipError_t launch_knn_merge(const float* part_d, const int32_t* part_p, int nq, int n_range, int k, float* out_d, int32_t* out_p, hipStream_t s);

}  // namespace scann

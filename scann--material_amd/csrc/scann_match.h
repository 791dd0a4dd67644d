// Internal declarations of the structure matching over a latent-space index (scann_match.hip, host side in scann_match.cpp); the C ABI and
// the definition are in include/scann_hip.h (scann_index_match).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scann_knn.h"

namespace scann {

// (a tile holds TILE_TQ query atoms, scann_tile.h, and a query structure lies in one tile: that is SCANN_MATCH_MAX_ATOMS)
constexpr int MT_SETS = 32;        // query structures per tile at most (bounds the per-structure LDS: g values and the k-best lists)
constexpr int MT_SETS_SMALL = 16;  // ... and what the per-structure LDS is laid out for when no tile holds more: with k <= 8 the workgroup then
                                   // takes under 40 KiB and four of them share a CU's 160 KiB, as with knn_tile_kernel
constexpr int MT_LD = TILE_TQ + 4;  // floats between two rows of the distance tile: 16-byte stores stay aligned, and the lanes that read one
                                   // query's column down the rows (match_tile_kernel, the g pass) spread over 8 banks instead of 1
constexpr int MT_UNION = TILE_TR * MT_LD;  // floats the slabs and the distance tile share: max(32 * (128 + 64) + 64, 64 * 132)

// One launch of match_tile_kernel.  Workgroup (x, y) takes range x of the index rows -- [row_begin, row_end) in positions, beginning and
// ending on segment boundaries, its first segment's number seg_begin -- and tile y of the query structures: sets [set_begin, set_end),
// whose atoms are the consecutive query rows q_first[set_begin] .. q_first[set_end] (at most TILE_TQ of them, at most MT_SETS sets).  It
// leaves, per set, the range's k best segments under (score, segment) in part_d / part_p [set - set_base][n_range][k]; unused places
// hold (+inf, -1).
struct MatchArgs {
  const float* const* rows;    // [n_chunk] -> [chunk_rows][stride], columns dim .. stride-1 zero
  const int64_t* const* ids;   // [n_chunk] -> [chunk_rows]
  int32_t chunk_rows, stride;
  const float* q;              // [n query rows][stride], padded like the rows
  const int32_t* q_first;      // [n_sets + 1]
  const int64_t* qid;          // [n_sets] or null: segments whose id equals the set's are skipped
  const int32_t* tiles;        // [n_tile][2] set_begin, set_end
  const int32_t* ranges;       // [n_range][3] row_begin, row_end, seg_begin
  int32_t n_tile, n_range, set_base, k, measure;
  int32_t sets_ld;             // MT_SETS_SMALL or MT_SETS: no tile holds more structures (the layout only: no output bit depends on it)
  float* part_d;
  int32_t* part_p;
};
size_t match_lds_bytes(int k, int sets_ld);
hipError_t launch_match_tile(const MatchArgs& a, hipStream_t s);

// match_pair_kernel: one workgroup per (set, place).  Pair e = set * k + place names the segment [seg_first[e], seg_first[e] + seg_count[e])
// (count 0: no segment, nothing is written).  The distances of the set's atoms to the segment's rows are formed again and reduced to
// parts [e][4] = (float) F, (float) G, Fmax, Gmax and, per query atom i of the set, the witness of f_i and f_i itself at
// match_pos / match_d [(q_first[set] + i) * k + place].
struct MatchPairArgs {
  const float* const* rows;
  int32_t chunk_rows, stride;
  const float* q;
  const int32_t* q_first;
  const int32_t* seg_first;
  const int32_t* seg_count;
  int32_t n_sets, k;
  float* parts;
  int32_t* match_pos;
  float* match_d;
};
hipError_t launch_match_pair(const MatchPairArgs& a, hipStream_t s);

// scann_match.cpp, for scann_pairing.cpp's shortlist: scann_index_match on checked arguments -- host or device query rows q of the index's
// width (kind), staged at the padded width and matched on stream s; synchronous.  Outputs as scann_index_match's, all but score may be null
int match_staged(scann_handle* h, scann_index* ix, const float* q, hipMemcpyKind kind, const int32_t* q_first, int64_t n_sets, const int64_t* qid,
                 int measure, int k, hipStream_t s, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos,
                 float* match_d);

}  // namespace scann

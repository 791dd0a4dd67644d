// Host batch packers behind the C ABI.  No GPU work in this file.
//
// The reference builds every batch from nested Python lists in DataIterator.__getitem__
// (datagenerator.py:69-135) with pad_sequence / pad_nested_sequences (general.py:14-50); at the
// rates of the HIP forward that host work is the bottleneck.  Two entry points replace it:
//   scann_pack_padded   padded Keras input dict (scann_model.py:338-357)  ->  packed CSR batch
//   scann_slice_batch   structures `sel` of a dataset held in CSR form    ->  packed CSR batch
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/scann_hip.h"
#include "scann_internal.h"

namespace {
thread_local std::string t_pack_error;
int pack_fail(const char* msg) {
  t_pack_error = msg;
  return SCANN_ERR_INVALID;
}

// fn(t) for t in [0, n): t = 0 on the calling thread, the others on threads of their own, all joined before the return.  A thread that
// cannot be started leaves its range, and every later one, to the calling thread: no exception reaches the C ABI.
template <class Fn>
void fan_out(int n, Fn&& fn) {
  std::vector<std::thread> th;
  int t = 1;
  try {
    th.reserve((size_t)std::max(0, n - 1));
    for (; t < n; ++t) th.emplace_back(fn, t);
  } catch (const std::exception&) {
  }
  fn(0);
  for (int u = t; u < n; ++u) fn(u);
  for (std::thread& x : th) x.join();
}

// Threads of a packer pass over B structures: one below 2,048 (below ~1,000 structures per thread the threads' start-up costs what they
// save: measured at 256 per thread), else min(cores, 8, B / 1024) or SCANN_PACK_THREADS (read on every call), at most B.
int pack_threads(int32_t B) {
  if (B < 2048) return 1;
  const unsigned hw = std::thread::hardware_concurrency();
  int n = (int)std::min<int64_t>(std::min<unsigned>(hw ? hw : 1u, 8u), B / 1024);
  if (const char* e = getenv("SCANN_PACK_THREADS")) n = std::max(1, std::min(64, atoi(e)));
  return std::max(1, std::min<int>(n, B));
}

// structures [b0, b1) of range t of n
std::pair<int32_t, int32_t> pack_range(int32_t B, int t, int n) {
  return {(int32_t)((int64_t)B * t / n), (int32_t)((int64_t)B * (t + 1) / n)};
}
}  // namespace

namespace scann {

// Greedy tiling of atoms [a0, a1): whole atoms, <= want edges and <= tile_atoms atoms per tile; with allow_chunks an atom with more
// than `want` neighbours closes the open tile and becomes ceil(deg / want) single-atom chunk tiles (tile_part = softmax-merge slot).
static void tile_range(const int32_t* edge_offset, int32_t a0, int32_t a1, int want, int tile_atoms, bool allow_chunks,
                       std::vector<EdgeTile>& tiles, std::vector<int32_t>& tile_part, std::vector<int32_t>& big_tab, int32_t& n_slot) {
  EdgeTile cur{a0, a0, edge_offset[a0], edge_offset[a0]};
  for (int a = a0; a < a1; ++a) {
    const int32_t e0 = edge_offset[a], e1 = edge_offset[a + 1];
    if (allow_chunks && e1 - e0 > want) {  // big atom: close the open tile, then one chunk tile per <= tile_rows of its edges
      if (a > cur.atom_begin) {
        cur.atom_end = a;
        cur.edge_end = e0;
        tiles.push_back(cur);
        tile_part.push_back(-1);
      }
      big_tab.push_back(a); big_tab.push_back(n_slot); big_tab.push_back((e1 - e0 + want - 1) / want);
      for (int c0 = e0; c0 < e1; c0 += want) {
        tiles.push_back(EdgeTile{a, a + 1, c0, std::min(c0 + want, e1)});
        tile_part.push_back(n_slot++);
      }
      cur = EdgeTile{a + 1, a + 1, e1, e1};
      continue;
    }
    // greedy tiling: whole atoms, <= tile_rows edges and <= tile_atoms atoms per tile
    if ((e1 - cur.edge_begin) > want || (a - cur.atom_begin) >= tile_atoms) {
      cur.atom_end = a;
      cur.edge_end = e0;
      tiles.push_back(cur);
      tile_part.push_back(-1);
      cur = EdgeTile{a, a, e0, e0};
    }
  }
  if (cur.atom_begin < a1) {
    cur.atom_end = a1;
    cur.edge_end = edge_offset[a1];
    tiles.push_back(cur);
    tile_part.push_back(-1);
  }
}

int plan_tiles(const int32_t* mol_offset, int32_t B, const int32_t* edge_offset, const int32_t* edge_col, int32_t A, int32_t E,
               int tile_rows_req, int tile_atoms, bool allow_chunks, std::vector<EdgeTile>& tiles, std::vector<int32_t>& tile_part,
               std::vector<int32_t>& big_tab, std::vector<int32_t>& edge_row, int* tile_rows_out, int32_t* max_degree,
               int32_t* n_slot_out, std::string& err, bool fill_edge_row) {
  // Validation and the centre atom of every edge in flat passes (long loops the compiler vectorises), the greedy tiling in a loop
  // over the atoms alone: at 1.8 M molecules/s this function runs ~14,000 atoms per millisecond of device time, and the per-edge
  // branches of the first version (one fused loop) were half of scann_batch_upload's host time.
  int32_t n_slot = 0, maxdeg = 0, mindeg = 0;
  for (int a = 0; a < A; ++a) {
    const int32_t deg = edge_offset[a + 1] - edge_offset[a];
    maxdeg = std::max(maxdeg, deg);
    mindeg = std::min(mindeg, deg);
  }
  if (mindeg < 0) { err = "edge_offset not monotone"; return SCANN_ERR_INVALID; }
  if (maxdeg > TE_MAX && !allow_chunks) {
    err = "an atom has more than 64 neighbours (edge-tile limit of the selected edge kernel; edge_kernel_lean, the default on "
          "the g_update path, has none)";
    return SCANN_ERR_UNSUPPORTED;
  }
  for (int s = 0; s < B && edge_col; ++s) {  // every neighbour index inside its own structure (device packing: checked by pack_padded_kernel)
    const int32_t a0 = mol_offset[s], a1 = mol_offset[s + 1];
    int32_t mn = a0, mx = a0;
    for (int e = edge_offset[a0]; e < edge_offset[a1]; ++e) {
      mn = std::min(mn, edge_col[e]);
      mx = std::max(mx, edge_col[e]);
    }
    if (mn < a0 || mx >= a1) { err = "neighbour index outside its structure"; return SCANN_ERR_INVALID; }
  }
  if (fill_edge_row) {  // (scann_batch_upload leaves this to a kernel behind the input copy: launch_edge_row)
    edge_row.resize((size_t)E);
    for (int a = 0; a < A; ++a)
      for (int e = edge_offset[a]; e < edge_offset[a + 1]; ++e) edge_row[(size_t)e] = a;
  }
  int tile_rows = tile_rows_req;
  if (maxdeg > tile_rows && !allow_chunks) tile_rows = TE_MAX;  // a 32-row tile cannot hold the largest atom: 64-row tiles
  tiles.clear(); tile_part.clear(); big_tab.clear(); n_slot = 0;
  tile_range(edge_offset, 0, A, tile_rows, tile_atoms, allow_chunks, tiles, tile_part, big_tab, n_slot);
  if (tiles.empty()) {
    tiles.push_back(EdgeTile{0, A, 0, E});
    tile_part.push_back(-1);
  }
  *tile_rows_out = tile_rows;
  *max_degree = maxdeg;
  *n_slot_out = n_slot;
  return SCANN_OK;
}

// The filled plan of the inference edge kernels (scann_internal.h).  plan_tiles closes a tile as soon as the NEXT atom of the caller's
// order does not fit, and the rows left over are computed for nothing: 6 % of the rows of QM9-shaped batches, 12 % on crystals.  Here
// the atoms of a structure are taken best-fit: the remaining atom of the largest degree that still fits the open tile, the lowest
// index among equals.  A structure's atoms by degree: a stable counting sort (bucket d = its atoms of degree d, ascending), a 65-bit
// mask of the buckets that still hold atoms, and the highest set bit at or below the room that is left -- O(1) per atom.
bool plan_tiles_filled(const int32_t* mol_offset, int32_t B, const int32_t* edge_offset, int32_t A, int rows, int tile_atoms,
                       const std::vector<EdgeTile>& contiguous, int32_t n_big, std::vector<int32_t>& atom_row,
                       std::vector<int32_t>& tile_offset, std::vector<EdgeTile>& tiles) {
  const auto identity = [&]() {
    atom_row.resize((size_t)A);
    for (int a = 0; a < A; ++a) atom_row[(size_t)a] = a;
    tile_offset.assign(edge_offset, edge_offset + A + 1);
    tiles = contiguous;
    return false;
  };
  if (n_big > 0 || rows > 64 || rows <= 0 || tile_atoms <= 0 || contiguous.size() <= 1) return identity();
  // (per structure the passes below touch its own degrees only -- up to its largest, not up to `rows`: a molecule of 18 atoms with at
  // most 12 neighbours each is what a group of batches holds a thousand times.  Offsets are monotone: plan_tiles has checked them)
  atom_row.resize((size_t)A);
  tile_offset.resize((size_t)A + 1);
  tiles.clear();
  tiles.reserve(contiguous.size());
  int32_t* const out_row = atom_row.data();
  int32_t* const out_off = tile_offset.data();
  out_off[0] = 0;
  std::vector<int32_t> order_buf;  // the structure's atoms sorted by degree, stable
  int32_t cnt[66] = {}, head[66], tail[66], fill[66];  // bucket d = order[head[d], tail[d])
  EdgeTile cur{0, 0, 0, 0};
  int32_t k = 0, e = 0;  // atoms / edges placed so far
  for (int s = 0; s < B; ++s) {
    const int32_t a0 = mol_offset[s], a1 = mol_offset[s + 1];
    int maxd = 0;
    for (int a = a0; a < a1; ++a) {
      const int d = edge_offset[a + 1] - edge_offset[a];
      if (d > rows) return identity();  // (a chunked atom, whoever counted them)
      ++cnt[d];
      maxd = std::max(maxd, d);
    }
    uint64_t lo = 0;   // bit d: bucket d < 64 holds atoms
    bool top = false;  // ... and bucket 64
    for (int d = 0, pos = 0; d <= maxd; ++d) {
      head[d] = fill[d] = pos;
      if (cnt[d]) { if (d < 64) lo |= 1ull << d; else top = true; }
      pos += cnt[d];
      tail[d] = pos;
      cnt[d] = 0;
    }
    if (order_buf.size() < (size_t)(a1 - a0)) order_buf.resize((size_t)(a1 - a0) * 2);
    int32_t* const order = order_buf.data();
    for (int a = a0; a < a1; ++a) order[fill[edge_offset[a + 1] - edge_offset[a]]++] = a;
    for (int left = a1 - a0; left > 0; --left) {
      const int room = (k - cur.atom_begin) >= tile_atoms ? -1 : rows - (e - cur.edge_begin);
      int d = -1;
      if (room >= 64 && top) d = 64;
      else if (room >= 0) {
        const uint64_t fit = room >= 63 ? lo : lo & ((2ull << room) - 1);
        if (fit) d = 63 - __builtin_clzll(fit);
      }
      if (d < 0) {  // nothing fits (or the tile has its atoms): close it, then the largest atom that is left
        cur.atom_end = k; cur.edge_end = e;
        tiles.push_back(cur);
        cur = EdgeTile{k, k, e, e};
        d = top ? 64 : 63 - __builtin_clzll(lo);
      }
      const int32_t a = order[head[d]++];
      if (head[d] == tail[d]) { if (d < 64) lo &= ~(1ull << d); else top = false; }
      out_row[k++] = a;
      e += d;
      out_off[k] = e;
    }
  }
  cur.atom_end = k; cur.edge_end = e;
  tiles.push_back(cur);
  if (tiles.size() >= contiguous.size()) return identity();  // best-fit lost (it can: it is a heuristic too): the caller's order
  return true;
}


}  // namespace scann

extern "C" {

const char* scann_pack_last_error(void) { return t_pack_error.c_str(); }

int scann_pack_padded(int32_t B, int32_t M, int32_t N, const int32_t* atomic, const float* cgcnn,
                      const uint8_t* atom_mask, const int32_t* neighbors, const uint8_t* neighbor_mask,
                      const float* neighbor_weight, const float* neighbor_distance, const float* ring,
                      int32_t* out_atomic, float* out_cgcnn, float* out_ring, int32_t* out_mol_offset,
                      int32_t* out_edge_offset, int32_t* out_edge_col, float* out_edge_dist,
                      float* out_edge_weight, int32_t* out_row_of, int32_t* n_atom, int32_t* n_edge) {
  if (B < 0 || M < 0 || N < 0 || !atom_mask ||
      (N > 0 && (!neighbors || !neighbor_mask || !neighbor_weight || !neighbor_distance)) || !out_mol_offset || !out_edge_offset || !out_edge_col || !out_edge_dist ||
      !out_edge_weight || !out_row_of || !n_atom || !n_edge)
    return pack_fail("scann_pack_padded: null argument or negative shape");
  if ((atomic && !out_atomic) || (cgcnn && !out_cgcnn) || (ring && !out_ring))
    return pack_fail("scann_pack_padded: an input is given without its output array");
  // Structures are independent: ranges of them are counted (pass 1: real atoms, unmasked neighbour slots of real atoms), the counts
  // are turned into each range's first atom row / first edge, and the ranges are filled (pass 2) -- by one thread for a batch, by up
  // to 8 for the reference's `model.predict(whole padded dataset)` (130 k structures: 100 ms -> 15-20 ms of host time).  The output
  // does not depend on the number of threads.
  const int n_thr = pack_threads(B);
  std::vector<int64_t> cnt_a((size_t)n_thr + 1, 0), cnt_e((size_t)n_thr + 1, 0);
  std::vector<const char*> err((size_t)n_thr, nullptr);
  // pass 1: counts per range
  fan_out(n_thr, [&](int t) {
    const auto [b0, b1] = pack_range(B, t, n_thr);
    int64_t na_t = 0, ne_t = 0;
    for (int32_t b = b0; b < b1; ++b) {
      const uint8_t* am = atom_mask + (int64_t)b * M;
      int64_t here = 0;
      for (int32_t a = 0; a < M; ++a) {
        if (!am[a]) continue;
        ++here;
        const uint8_t* nm = neighbor_mask + ((int64_t)b * M + a) * N;
        for (int32_t n = 0; n < N; ++n) ne_t += nm[n] != 0;
      }
      if (here == 0) { err[t] = "a structure in the batch has no atoms"; return; }
      na_t += here;
    }
    cnt_a[t + 1] = na_t;
    cnt_e[t + 1] = ne_t;
  });
  for (int t = 0; t < n_thr; ++t) {
    if (err[t]) return pack_fail(err[t]);
    cnt_a[t + 1] += cnt_a[t];
    cnt_e[t + 1] += cnt_e[t];
  }
  const int64_t na = cnt_a[n_thr], ne = cnt_e[n_thr];
  if (na > INT32_MAX) return pack_fail("batch too large for int32 atom rows");
  if (ne > INT32_MAX) return pack_fail("batch too large for int32 edge rows");
  // pass 2: packed row of every real atom (the job of gather_shape, custom_layers.py:18-28, moved to the host), then the unmasked
  // neighbour slots of real atoms, in slot order
  out_mol_offset[0] = 0;
  out_edge_offset[0] = 0;
  fan_out(n_thr, [&](int t) {
    const auto [b0, b1] = pack_range(B, t, n_thr);
    int64_t row = cnt_a[t], e = cnt_e[t];
    for (int32_t b = b0; b < b1; ++b) {
      const uint8_t* am = atom_mask + (int64_t)b * M;
      int32_t* ro = out_row_of + (int64_t)b * M;
      int64_t r = row;
      for (int32_t a = 0; a < M; ++a) ro[a] = am[a] ? (int32_t)r++ : -1;
      for (int32_t a = 0; a < M; ++a) {
        if (ro[a] < 0) continue;
        const int64_t base = ((int64_t)b * M + a) * N;
        for (int32_t n = 0; n < N; ++n) {
          if (!neighbor_mask[base + n]) continue;
          const int32_t tgt = neighbors[base + n];
          if (tgt < 0 || tgt >= M || ro[tgt] < 0) { err[t] = "an unmasked neighbour slot points at a padded atom"; return; }
          out_edge_col[e] = ro[tgt];
          out_edge_dist[e] = neighbor_distance[base + n];
          out_edge_weight[e] = neighbor_weight[base + n];
          ++e;
        }
        if (atomic) out_atomic[row] = atomic[(int64_t)b * M + a];
        if (cgcnn) memcpy(out_cgcnn + row * 92, cgcnn + ((int64_t)b * M + a) * 92, 92 * sizeof(float));
        if (ring) memcpy(out_ring + row * 2, ring + ((int64_t)b * M + a) * 2, 2 * sizeof(float));
        out_edge_offset[++row] = (int32_t)e;
      }
      out_mol_offset[b + 1] = (int32_t)row;
    }
  });
  for (int t = 0; t < n_thr; ++t)
    if (err[t]) return pack_fail(err[t]);
  *n_atom = (int32_t)na;
  *n_edge = (int32_t)ne;
  return SCANN_OK;
}

// The host half of the DEVICE packing (scann_upload_padded): only the 1-byte (or 4-byte) MASKS are read here -- which atoms are real, how
// many unmasked neighbour slots each has -- and turned into mol_offset / edge_offset / the packed row of every padded atom slot.  The
// 4-byte payload arrays (neighbour indices, distances, weights, atomic numbers: 13/14 of the bytes) are never touched by the host: they
// are copied to the device as they are and compacted there (pack_padded_kernel).  Same semantics as scann_pack_padded (datagenerator.py:
// 69-135, custom_layers.py:18-28): a real atom = atom_mask != 0; an edge = an unmasked slot of a real atom, in slot order.
// Masks of 1 byte (bool / uint8) or 4 bytes (the float32 masks of the Keras input dict, int32; -0.0f counts as 0).
namespace {
inline bool mask_at(const void* m, int size, int64_t i) {
  return size == 1 ? static_cast<const uint8_t*>(m)[i] != 0 : (static_cast<const uint32_t*>(m)[i] & 0x7fffffffu) != 0;
}
}  // namespace

// memcpy of a large block on up to 8 threads (the padded payload of a 2,048-structure chunk is ~10 MB, of a whole dataset ~100: one
// thread moves ~7-10 GB/s, which would make the staging copy the longest host step of the padded path).  Disjoint 64-byte-aligned
// ranges, joined before the return.
int scann_host_copy(void* dst, const void* src, int64_t bytes_) {
  if (bytes_ < 0 || ((!dst || !src) && bytes_ > 0)) return pack_fail("scann_host_copy: null argument or negative size");
  const size_t bytes = (size_t)bytes_;
  const unsigned hw = std::thread::hardware_concurrency();
  size_t n_thr = std::min<size_t>(std::min<unsigned>(hw ? hw : 1u, 8u), bytes >> 22);  // >= 4 MiB per thread
  if (const char* e = getenv("SCANN_COPY_THREADS")) n_thr = (size_t)std::max(1, std::min(64, atoi(e)));  // (tests: threads on a small block)
  if (n_thr <= 1 || bytes < 64 * n_thr) { memcpy(dst, src, bytes); return SCANN_OK; }
  fan_out((int)n_thr, [&](int t) {
    const size_t o0 = (bytes * t / n_thr) & ~(size_t)63, o1 = t + 1 == (int)n_thr ? bytes : (bytes * (t + 1) / n_thr) & ~(size_t)63;
    memcpy(static_cast<char*>(dst) + o0, static_cast<const char*>(src) + o0, o1 - o0);
  });
  return SCANN_OK;
}

int scann_count_padded(int32_t B, int32_t M, int32_t N, const void* atom_mask, int32_t atom_mask_size, const void* neighbor_mask,
                       int32_t neighbor_mask_size, int32_t* out_mol_offset, int32_t* out_edge_offset, int32_t* out_row_of, int32_t* n_atom,
                       int32_t* n_edge) {
  if (B < 0 || M < 0 || N < 0 || !atom_mask || (N > 0 && !neighbor_mask) || !out_mol_offset || !out_edge_offset || !out_row_of || !n_atom || !n_edge)
    return pack_fail("scann_count_padded: null argument or negative shape");
  if ((atom_mask_size != 1 && atom_mask_size != 4) || (neighbor_mask_size != 1 && neighbor_mask_size != 4))
    return pack_fail("scann_count_padded: masks must have 1-byte or 4-byte elements");
  const int n_thr = pack_threads(B);
  std::vector<int64_t> cnt_a((size_t)n_thr + 1, 0), cnt_e((size_t)n_thr + 1, 0);
  std::vector<const char*> err((size_t)n_thr, nullptr);
  // degree of every padded atom slot (0 for a padded atom), kept in out_row_of until the second pass turns it into the row
  auto degree = [&](int64_t bm) {
    int32_t d = 0;
    if (neighbor_mask_size == 1) {
      const uint8_t* nm = static_cast<const uint8_t*>(neighbor_mask) + bm * N;
      for (int32_t n = 0; n < N; ++n) d += nm[n] != 0;
    } else {
      const uint32_t* nm = static_cast<const uint32_t*>(neighbor_mask) + bm * N;
      for (int32_t n = 0; n < N; ++n) d += (nm[n] & 0x7fffffffu) != 0;
    }
    return d;
  };
  fan_out(n_thr, [&](int t) {
    const auto [b0, b1] = pack_range(B, t, n_thr);
    int64_t na_t = 0, ne_t = 0;
    for (int32_t b = b0; b < b1; ++b) {
      int64_t here = 0;
      for (int32_t a = 0; a < M; ++a) {
        const int64_t bm = (int64_t)b * M + a;
        if (!mask_at(atom_mask, atom_mask_size, bm)) { out_row_of[bm] = -1; continue; }
        ++here;
        const int32_t d = degree(bm);
        out_row_of[bm] = d;
        ne_t += d;
      }
      if (here == 0) { err[t] = "a structure in the batch has no atoms"; return; }
      na_t += here;
    }
    cnt_a[t + 1] = na_t;
    cnt_e[t + 1] = ne_t;
  });
  for (int t = 0; t < n_thr; ++t) {
    if (err[t]) return pack_fail(err[t]);
    cnt_a[t + 1] += cnt_a[t];
    cnt_e[t + 1] += cnt_e[t];
  }
  if (cnt_a[n_thr] > INT32_MAX) return pack_fail("batch too large for int32 atom rows");
  if (cnt_e[n_thr] > INT32_MAX) return pack_fail("batch too large for int32 edge rows");
  out_mol_offset[0] = 0;
  out_edge_offset[0] = 0;
  fan_out(n_thr, [&](int t) {
    const auto [b0, b1] = pack_range(B, t, n_thr);
    int64_t row = cnt_a[t], e = cnt_e[t];
    for (int32_t b = b0; b < b1; ++b) {
      for (int32_t a = 0; a < M; ++a) {
        const int64_t bm = (int64_t)b * M + a;
        const int32_t d = out_row_of[bm];
        if (d < 0) continue;
        out_row_of[bm] = (int32_t)row;
        e += d;
        out_edge_offset[++row] = (int32_t)e;
      }
      out_mol_offset[b + 1] = (int32_t)row;
    }
  });
  *n_atom = (int32_t)cnt_a[n_thr];
  *n_edge = (int32_t)cnt_e[n_thr];
  return SCANN_OK;
}

int scann_slice_count(const int64_t* ds_mol_offset, const int64_t* ds_edge_offset, const int64_t* sel, int32_t n_sel,
                      int64_t n_struct_total, int64_t* n_atom, int64_t* n_edge) {
  if (!ds_mol_offset || !ds_edge_offset || (!sel && n_sel) || n_sel < 0 || !n_atom || !n_edge)
    return pack_fail("scann_slice_count: null argument");
  int64_t na = 0, ne = 0;
  for (int32_t i = 0; i < n_sel; ++i) {
    const int64_t s = sel[i];
    if (s < 0 || s >= n_struct_total) return pack_fail("scann_slice_count: structure index out of range");
    const int64_t a0 = ds_mol_offset[s], a1 = ds_mol_offset[s + 1];
    na += a1 - a0;
    ne += ds_edge_offset[a1] - ds_edge_offset[a0];
  }
  *n_atom = na;
  *n_edge = ne;
  return SCANN_OK;
}

int scann_slice_batch(const int64_t* ds_mol_offset, const int64_t* ds_edge_offset, const int32_t* ds_atomic,
                      const float* ds_ring, const int32_t* ds_edge_local, const float* ds_edge_dist,
                      const float* ds_edge_weight, const int64_t* sel, int32_t n_sel, int64_t n_struct_total,
                      int32_t* out_atomic, float* out_ring, int32_t* out_mol_offset, int32_t* out_edge_offset,
                      int32_t* out_edge_col, float* out_edge_dist, float* out_edge_weight) {
  if (!ds_mol_offset || !ds_edge_offset || !ds_atomic || !ds_edge_local || !ds_edge_dist || !ds_edge_weight ||
      (!sel && n_sel) || n_sel < 0 || !out_atomic || !out_mol_offset || !out_edge_offset || !out_edge_col ||
      !out_edge_dist || !out_edge_weight || (ds_ring && !out_ring))
    return pack_fail("scann_slice_batch: null argument");
  int64_t na = 0, ne = 0;
  out_mol_offset[0] = 0;
  out_edge_offset[0] = 0;
  for (int32_t i = 0; i < n_sel; ++i) {
    const int64_t s = sel[i];
    if (s < 0 || s >= n_struct_total) return pack_fail("scann_slice_batch: structure index out of range");
    const int64_t a0 = ds_mol_offset[s], a1 = ds_mol_offset[s + 1];
    const int64_t e0 = ds_edge_offset[a0], e1 = ds_edge_offset[a1];
    const int64_t cnt = a1 - a0, ecnt = e1 - e0;
    if (cnt <= 0) return pack_fail("a structure in the batch has no atoms");
    if (na + cnt > INT32_MAX || ne + ecnt > INT32_MAX) return pack_fail("batch too large for int32 rows");
    memcpy(out_atomic + na, ds_atomic + a0, cnt * sizeof(int32_t));
    if (ds_ring) memcpy(out_ring + na * 2, ds_ring + a0 * 2, cnt * 2 * sizeof(float));
    const int64_t shift = ne - e0;  // rebase the structure's CSR row pointers
    for (int64_t a = 0; a < cnt; ++a) out_edge_offset[na + a + 1] = (int32_t)(ds_edge_offset[a0 + a + 1] + shift);
    const int32_t base = (int32_t)na;  // neighbour ids inside the structure -> packed atom rows
    for (int64_t e = 0; e < ecnt; ++e) {
      const int32_t l = ds_edge_local[e0 + e];
      if (l < 0 || l >= cnt) return pack_fail("a neighbour index lies outside its structure");
      out_edge_col[ne + e] = base + l;
    }
    memcpy(out_edge_dist + ne, ds_edge_dist + e0, ecnt * sizeof(float));
    memcpy(out_edge_weight + ne, ds_edge_weight + e0, ecnt * sizeof(float));
    na += cnt;
    ne += ecnt;
    out_mol_offset[i + 1] = (int32_t)na;
  }
  return SCANN_OK;
}

int scann_plan_tiles(const scann_batch_t* b, int32_t tile_rows, int32_t tile_atoms, int32_t allow_chunks, int32_t cap,
                     int32_t* tiles_out, int32_t* part_out, int32_t* n_tiles, int32_t* n_slots) {
  if (!b || !n_tiles || !n_slots || !b->mol_offset || !b->edge_offset || (b->n_edge > 0 && !b->edge_col) || b->n_struct <= 0 ||
      b->n_atom <= 0 || b->n_edge < 0 || (tile_rows != 32 && tile_rows != 64) || tile_atoms <= 0 || tile_atoms > 32)
    return pack_fail("scann_plan_tiles: bad argument");
  if (b->mol_offset[0] != 0 || b->mol_offset[b->n_struct] != b->n_atom || b->edge_offset[0] != 0 || b->edge_offset[b->n_atom] != b->n_edge)
    return pack_fail("scann_plan_tiles: offsets do not cover the batch");
  for (int s = 0; s < b->n_struct; ++s)
    if (b->mol_offset[s + 1] <= b->mol_offset[s]) return pack_fail("scann_plan_tiles: structure without atoms");
  std::vector<scann::EdgeTile> tiles;
  std::vector<int32_t> part, big, row;
  int rows = 0;
  int32_t maxdeg = 0, nslot = 0;
  std::string err;
  const int r = scann::plan_tiles(b->mol_offset, b->n_struct, b->edge_offset, b->edge_col, b->n_atom, b->n_edge, tile_rows, tile_atoms,
                                  allow_chunks != 0, tiles, part, big, row, &rows, &maxdeg, &nslot, err);
  if (r) {
    t_pack_error = "scann_plan_tiles: " + err;
    return r;
  }
  *n_tiles = (int32_t)tiles.size();
  *n_slots = nslot;
  if ((int32_t)tiles.size() > cap || !tiles_out || !part_out) return tiles_out ? pack_fail("scann_plan_tiles: output capacity too small") : SCANN_OK;
  for (size_t i = 0; i < tiles.size(); ++i) {
    tiles_out[4 * i] = tiles[i].atom_begin; tiles_out[4 * i + 1] = tiles[i].atom_end;
    tiles_out[4 * i + 2] = tiles[i].edge_begin; tiles_out[4 * i + 3] = tiles[i].edge_end;
    part_out[i] = part[i];
  }
  return rows;  // 32 or 64: the edge rows per tile actually planned
}

int scann_plan_tiles_filled(const scann_batch_t* b, int32_t tile_rows, int32_t tile_atoms, int32_t cap, int32_t* atom_row_out,
                            int32_t* tile_offset_out, int32_t* tiles_out, int32_t* n_tiles) {
  if (!b || !n_tiles || !atom_row_out || !tile_offset_out || !tiles_out || !b->mol_offset || !b->edge_offset || b->n_struct <= 0 ||
      b->n_atom <= 0 || b->n_edge < 0 || (tile_rows != 32 && tile_rows != 64) || tile_atoms <= 0 || tile_atoms > 32)
    return pack_fail("scann_plan_tiles_filled: bad argument");
  if (b->mol_offset[0] != 0 || b->mol_offset[b->n_struct] != b->n_atom || b->edge_offset[0] != 0 || b->edge_offset[b->n_atom] != b->n_edge)
    return pack_fail("scann_plan_tiles_filled: offsets do not cover the batch");
  for (int s = 0; s < b->n_struct; ++s)
    if (b->mol_offset[s + 1] <= b->mol_offset[s]) return pack_fail("scann_plan_tiles_filled: structure without atoms");
  std::vector<scann::EdgeTile> contiguous, tiles;
  std::vector<int32_t> part, big, row, atom_row, tile_offset;
  int rows = 0;
  int32_t maxdeg = 0, nslot = 0;
  std::string err;
  const int r = scann::plan_tiles(b->mol_offset, b->n_struct, b->edge_offset, nullptr, b->n_atom, b->n_edge, tile_rows, tile_atoms, true,
                                  contiguous, part, big, row, &rows, &maxdeg, &nslot, err, false);
  if (r) {
    t_pack_error = "scann_plan_tiles_filled: " + err;
    return r;
  }
  const bool filled = scann::plan_tiles_filled(b->mol_offset, b->n_struct, b->edge_offset, b->n_atom, rows, tile_atoms, contiguous,
                                               (int32_t)big.size() / 3, atom_row, tile_offset, tiles);
  *n_tiles = (int32_t)tiles.size();
  if ((int32_t)tiles.size() > cap) return pack_fail("scann_plan_tiles_filled: output capacity too small");
  memcpy(atom_row_out, atom_row.data(), atom_row.size() * 4);
  memcpy(tile_offset_out, tile_offset.data(), tile_offset.size() * 4);
  memcpy(tiles_out, tiles.data(), tiles.size() * sizeof(scann::EdgeTile));
  return filled ? 1 : 0;
}

}  // extern "C"


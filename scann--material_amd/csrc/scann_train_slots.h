// Slot bookkeeping of the training backward, host only (no device code; scann_train_check.cpp includes it without a device): the
// partial-slot arenas' one bump, capped at what was reserved, and the partitions -- rows per workgroup and workgroups -- that both
// size the slots and make deterministic mode deterministic, each stated once for its launcher and for the bound.  Internal.
#pragma once
#include "scann_internal.h"

#include <algorithm>
#include <vector>

namespace scann {

// Weight gradients are bit-reproducible: every launch_wgrad* stores per-slab partial sums into slots of `ctx.arena` (bump
// allocated, never reused within a step) and records (destination, slots); wgrad_flush adds them in slab order (one launch per
// WGRAD_REDUCE_MAX tensors; the backward pass flushes once per layer, on the side stream).  wgrad_slabs(rows) slots of 128*128 (+128 with a bias) floats per gradient.
struct WgradReduceEntry {
  float* dst;
  const float* part;
  int32_t n_slab, numel;
};
constexpr int WGRAD_MAX_JOBS = 8;
constexpr int WGRAD_REDUCE_MAX = 32;  // gradient tensors per reduce launch (a layer has <= 19; the last layer + the readout 29)
struct WgradCtx {
  struct Job {
    const float *X, *dY;
    float *part, *bpart;
    int32_t rows, chunks;
    const int32_t* nb = nullptr;  // gated operand: row r of the X operand is X[nb[r]] * X2[r] (ang = c[j] * G', attention.py:157,
    const float* X2 = nullptr;    // which the training forward then does not have to keep)
  };
  std::vector<Job> jobs;                  // queued by wgrad_add, launched together by wgrad_launch
  float* arena = nullptr;                 // partial slots (device)
  size_t cap = 0;                         // floats of the arena, set where `arena` is set
  size_t off = 0;                         // floats used
  bool overrun = false;                   // a reservation passed `cap`: nothing more is handed out, launched or reduced on this context
  std::vector<WgradReduceEntry> entries;  // one per gradient tensor since the last wgrad_flush
};

// THE bump: n_slot slots of numel floats behind what is in use, recorded as (dst, slots) for the next flush.  A reservation that would
// pass the capacity hands out nothing, records nothing and leaves `off` where it is; the context is overrun from then on, and every
// launcher that reserves returns without launching on an overrun context -- no kernel is enqueued with a slot pointer outside its arena.
inline float* reserve_slots(WgradCtx& ctx, float* dst, int n_slot, int numel) {
  const size_t n = (size_t)n_slot * (size_t)numel;
  if (ctx.overrun || n > ctx.cap - ctx.off) {
    ctx.overrun = true;
    return nullptr;
  }
  float* part = ctx.arena + ctx.off;
  ctx.entries.push_back(WgradReduceEntry{dst, part, n_slot, numel});
  ctx.off += n;
  return part;
}
// (dst, slots) of one 128-wide parameter-gradient vector whose per-workgroup partial sums a kernel is about to store
inline float* reserve_vec(WgradCtx& ctx, float* dst, int n_slot) { return reserve_slots(ctx, dst, n_slot, D); }

// ---- partitions: `per` rows to a workgroup, `n` workgroups ----
struct Split {
  int per, n;
};
inline Split split(int rows, int per) { return Split{per, (rows + per - 1) / per}; }

// weight-gradient GEMMs.  Slab per workgroup: at least 4 chunks of 64 rows and <= 80 slabs per gradient (a layer's launch is ~7
// gradients: a few hundred workgroups), so that the partial slots (64 KB each) the reduce re-reads stay small whatever the batch size.
// Measured at batch 128 (profiles/r02_notes.md): 1 -> 4 chunks for the atom-row gradients, 36 -> 9 slabs each, -20 us per step.
inline int wgrad_chunks(int rows) {
  const int tiles = (rows + 63) / 64;
  return std::max(std::min(4, tiles), (tiles + 79) / 80);
}
inline int wgrad_slabs(int rows) { return split(rows, 64 * wgrad_chunks(rows)).n; }
// queue one gradient dW += X^T dY (db += column sums of dY when db) for the next wgrad_launch
inline void wgrad_add(WgradCtx& ctx, const float* X, const float* dY, float* dW, float* db, int rows, const int32_t* nb = nullptr,
                      const float* X2 = nullptr) {
  if (rows <= 0) return;
  WgradCtx::Job j{};
  j.X = X; j.dY = dY; j.rows = rows; j.chunks = wgrad_chunks(rows);
  j.nb = nb; j.X2 = X2;
  const int n_slab = wgrad_slabs(rows);
  j.part = reserve_slots(ctx, dW, n_slab, D * D);
  if (db) j.bpart = reserve_vec(ctx, db, n_slab);
  if (!ctx.overrun) ctx.jobs.push_back(j);
}

// basis MLP leaf: 32-edge chunks per workgroup (the per-edge arithmetic, not the final atomics, bounds this kernel: 4 x fewer
// workgroups measured 105 vs 37 us at 18 k edges)
inline Split basis_split(int n_edge) { return split(n_edge, 32 * (n_edge >= (1 << 20) ? 4 : 1)); }
// base branch's filter_geo leaf: 32 edges per workgroup
inline Split base_geom_split(int n_edge) { return split(n_edge, 32); }
// species table: a run of atoms per workgroup, <= 128 workgroups
inline Split embed_table_split(int n_atom) { return split(n_atom, std::max(32, (n_atom + 127) / 128)); }
// general embedding (ring / cgcnn), deterministic sibling: runs of a multiple of its 8-atom steps, <= 128 workgroups
inline int embed_general_det_run(int n_atom) { return std::max(32, ((n_atom + 127) / 128 + 7) / 8 * 8); }
inline Split embed_general_split(int n_atom) { return split(n_atom, embed_general_det_run(n_atom)); }
// attention backward: four waves per workgroup, `apw` atoms per wave.  attn_bwd16_kernel (every degree <= 16): the wave walks its
// atoms one after the other (each a chain of loads and lane reductions), so as few as fill the chip a few times over (~1,000
// workgroups), and one gamma / beta slot per workgroup; attn_bwd_kernel: two atoms per wave, one slot per wave
inline int attn_apw16(int n_atom) { return std::min(8, std::max(1, (n_atom + 4095) / 4096)); }
inline int attn_bwd_apw(int n_atom, int max_degree) { return max_degree <= 16 ? attn_apw16(n_atom) : 2; }
inline Split attn_bwd_split(int n_atom, int max_degree) { return split(n_atom, 4 * attn_bwd_apw(n_atom, max_degree)); }
inline int attn_bwd_slots(int n_atom, int max_degree) { return (max_degree <= 16 ? 1 : 4) * attn_bwd_split(n_atom, max_degree).n; }
// LayerNorm backward: row groups of 32 per workgroup.  With per-workgroup partial slots instead of atomics the launch no longer has
// to stay small (round 1 capped it at ~160 workgroups); about 1,500 workgroups fill the chip several times over
inline int ln_bwd_groups(int rows) { return std::min(32, std::max(1, (rows + 32 * 1536 - 1) / (32 * 1536))); }
inline Split ln_bwd_split(int rows) { return split(rows, 32 * ln_bwd_groups(rows)); }
inline int ln_bwd_slots(int rows) { return ln_bwd_split(rows).n; }
// fused chains: 32-row tiles while the launch fits one round of workgroups (three per CU): it is then the latency chain of a tile, and
// a 32-row tile's chain is shorter (same choice as launch_atom / the edge-tile plan); 64-row tiles beyond
inline Split fused_split(int rows) { return split(rows, rows <= 32 * 768 ? 32 : 64); }
inline int tile_slots(int rows) { return fused_split(rows).n; }  // workgroups (= gamma / beta slots) of a fused kernel over `rows`

// ---- the bounds: sums of the above ----
// floats of weight-gradient partial slots one backward over this batch shape reserves at most.  Per layer <= 2 gradients over the edge
// rows (key, filter_geo geometry third; base: key) and <= 5 over the atom rows (filter_geo centre / neighbour thirds, query,
// ResidualNorm dense_1 / dense_2), readout 3 over atoms and 1 over structures; each with a bias row per slab
inline size_t wpart_slot_floats(int n_atom, int n_edge, int n_struct, int n_layer, int max_degree, int n_tile) {
  const size_t Lc = (size_t)n_layer;
  const int nE = std::max(n_edge, 1);
  return (size_t)(D * D + D) * (Lc * (2 * (size_t)wgrad_slabs(nE) + 5 * (size_t)wgrad_slabs(n_atom)) +
                                3 * (size_t)wgrad_slabs(n_atom) + (size_t)wgrad_slabs(n_struct)) +
         // LayerNorm gamma / beta partials: per layer ln_bwd over edges and atoms, attention backward over atoms
         (size_t)2 * D * Lc * ((size_t)std::max(ln_bwd_slots(nE), tile_slots(nE)) + (size_t)std::max(ln_bwd_slots(n_atom), tile_slots(n_atom)) +
                               (size_t)attn_bwd_slots(n_atom, max_degree)) +
         (size_t)D * n_struct +            // predict_property/kernel: one slot per structure (readout_bwd_kernel)
         (size_t)4 * D * Lc * (size_t)n_tile;  // attention + edge backward in one launch: four vectors, one slot per tile
}
// floats of det slots one backward over this batch shape reserves at most (bump allocated, never reused within the step)
inline size_t det_slot_floats(int n_atom, int n_edge, int n_layer, int n_species, int emb_dim, bool g_update, bool general, bool cgcnn,
                              bool ring) {
  size_t f = 0;
  if (n_edge > 0) {
    if (g_update) f += (size_t)(2 * NG + 2) * D * basis_split(n_edge).n;
    else f += (size_t)n_layer * (NG + 1) * D * base_geom_split(n_edge).n;
  }
  if (n_atom > 0) {
    if (general) {
      const int cin = emb_dim + (ring ? 10 : 0);
      f += (size_t)embed_general_split(n_atom).n *
           ((size_t)(1 + cin) * D + (cgcnn ? (size_t)93 * emb_dim : (size_t)n_species * emb_dim) + (ring ? 30 : 0));
    } else {
      f += (size_t)embed_table_split(n_atom).n * n_species * D + (size_t)n_species * (emb_dim + 1) * D;
    }
  }
  return f;
}

}  // namespace scann

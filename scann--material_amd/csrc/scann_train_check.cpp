// Stand-alone check of the training backward's slot bookkeeping (scann_train_slots.h) for the sanitizers: `make asan-train` compiles it
// under AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  It checks the capped bump (consecutive regions,
// an exact fill, one float more, a context that stays overrun; wgrad_add through the same bump), every partition over a sweep of row
// counts on both sides of its switches -- that workgroups x rows per workgroup cover the rows, and that the count is the one the
// expression it replaced gives, written out here as it stood in the launcher -- and the two bounds against the sums they replaced.
#include "scann_train_slots.h"

#include "scann_check.h"

namespace {

using namespace scann;

bool same(const WgradReduceEntry& e, const float* dst, const float* part, int n_slab, int numel) {
  return e.dst == dst && e.part == part && e.n_slab == n_slab && e.numel == numel;
}

void check_bump() {
  std::vector<float> arena(1000);
  float dst[4];
  WgradCtx c;
  c.arena = arena.data();
  c.cap = arena.size();
  float* a = reserve_slots(c, dst, 3, 100);
  EXPECT(a == arena.data() && c.off == 300 && c.entries.size() == 1 && same(c.entries[0], dst, a, 3, 100));
  float* b = reserve_vec(c, dst + 1, 2);
  EXPECT(b == arena.data() + 300 && c.off == 300 + 2 * D && c.entries.size() == 2 && same(c.entries[1], dst + 1, b, 2, D));
  float* d = reserve_slots(c, dst + 2, 1000 - 300 - 2 * D, 1);  // exactly the rest
  EXPECT(d == arena.data() + 300 + 2 * D && c.off == 1000 && c.entries.size() == 3 && !c.overrun);
  EXPECT(reserve_slots(c, dst + 3, 1, 1) == nullptr && c.overrun && c.off == 1000 && c.entries.size() == 3);  // one float more
  EXPECT(reserve_vec(c, dst + 3, 0) == nullptr && c.overrun && c.off == 1000 && c.entries.size() == 3);       // overrun stays

  WgradCtx e;  // the first reservation already too large; what would fit afterwards is refused too
  e.arena = arena.data();
  e.cap = 10;
  EXPECT(reserve_slots(e, dst, 11, 1) == nullptr && e.overrun && e.off == 0 && e.entries.empty());
  EXPECT(reserve_slots(e, dst, 1, 1) == nullptr && e.off == 0 && e.entries.empty());

  // wgrad_add: 100 rows are one slab; kernel + bias slots fill an arena of 128 * 128 + 128 floats exactly
  std::vector<float> big((size_t)D * D + D);
  WgradCtx g;
  g.arena = big.data();
  g.cap = big.size();
  const float* X = arena.data();
  wgrad_add(g, X, X, dst, dst + 1, 100);
  EXPECT(!g.overrun && g.off == g.cap && g.jobs.size() == 1 && g.entries.size() == 2 && g.jobs[0].part == big.data() &&
         g.jobs[0].bpart == big.data() + (size_t)D * D && g.jobs[0].rows == 100 && g.jobs[0].chunks == 2);
  EXPECT(same(g.entries[0], dst, big.data(), 1, D * D) && same(g.entries[1], dst + 1, big.data() + (size_t)D * D, 1, D));
  wgrad_add(g, X, X, dst, nullptr, 0);  // no rows: nothing
  EXPECT(!g.overrun && g.jobs.size() == 1 && g.entries.size() == 2);
  wgrad_add(g, X, X, dst, nullptr, 1);
  EXPECT(g.overrun && g.off == g.cap && g.jobs.size() == 1 && g.entries.size() == 2);
  WgradCtx k;  // the bias row does not fit: no job is queued
  k.arena = big.data();
  k.cap = (size_t)D * D;
  wgrad_add(k, X, X, dst, dst + 1, 100);
  EXPECT(k.overrun && k.off == (size_t)D * D && k.jobs.empty());
}

// workgroups x rows per workgroup cover the rows, with no workgroup to spare
bool covers(Split s, int rows) {
  if (rows <= 0) return s.n == 0 && s.per > 0;
  return s.per > 0 && (long long)s.n * s.per >= rows && (long long)(s.n - 1) * s.per < rows;
}

void check_partitions() {
  const int sweep[] = {0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257,
                       4095, 4096, 4097, 8191, 8192, 8193, 7 * 4096, 7 * 4096 + 1, 8 * 4096, 8 * 4096 + 1,  // 4096 atoms per wave step, 128 workgroups of 32
                       128 * 40 - 1, 128 * 40, 128 * 40 + 1,                                                 // 128 workgroups, run 40
                       20479, 20480, 20481,                                                                  // 80 slabs of 4 chunks
                       32 * 768 - 1, 32 * 768, 32 * 768 + 1,                                                 // 32- / 64-row fused tiles
                       32 * 1536 - 1, 32 * 1536, 32 * 1536 + 1, 2 * 32 * 1536, 2 * 32 * 1536 + 1,            // LayerNorm groups
                       32 * 32 * 1536 - 1, 32 * 32 * 1536, 32 * 32 * 1536 + 1,                               // ... their cap of 32
                       (1 << 20) - 1, 1 << 20, (1 << 20) + 1,                                                // basis chunks
                       (1 << 24) - 3, 1 << 24, (1 << 24) + 5};
  for (int rows : sweep) {
    const int n_edge = rows, n_atom = rows;
    {  // launch_basis_bwd
      const int chunks = n_edge >= (1 << 20) ? 4 : 1;
      const int n_wg = (n_edge + 32 * chunks - 1) / (32 * chunks);
      const Split s = basis_split(n_edge);
      EXPECT(s.n == n_wg && s.per == 32 * chunks && covers(s, rows));
    }
    {  // launch_base_geom_bwd
      const int n_wg = (n_edge + 31) / 32;
      const Split s = base_geom_split(n_edge);
      EXPECT(s.n == n_wg && s.per == 32 && covers(s, rows));
    }
    {  // launch_embed_bwd
      const int run = std::max(32, (n_atom + 127) / 128);
      const int n_wg = (n_atom + run - 1) / run;
      const Split s = embed_table_split(n_atom);
      EXPECT(s.n == n_wg && s.per == run && s.n <= 128 && covers(s, rows));
    }
    {  // launch_embed_general_bwd, deterministic
      const int run = std::max(32, ((n_atom + 127) / 128 + 7) / 8 * 8), n_wg = (n_atom + run - 1) / run;
      const Split s = embed_general_split(n_atom);
      EXPECT(s.n == n_wg && s.per == run && run % 8 == 0 && s.n <= 128 && covers(s, rows));
    }
    for (int max_degree : {0, 1, 16, 17, 64}) {  // launch_attn_bwd
      int grid, slots, apw;
      if (max_degree <= 16) {
        const int apw16 = std::min(8, std::max(1, (n_atom + 4095) / 4096));
        apw = apw16;
        grid = (n_atom + 4 * apw16 - 1) / (4 * apw16);
        slots = (n_atom + 4 * apw16 - 1) / (4 * apw16);  // one slot per workgroup
      } else {
        apw = 2;
        grid = (n_atom + 4 * apw - 1) / (4 * apw);
        slots = 4 * ((n_atom + 4 * 2 - 1) / (4 * 2));  // one slot per wave
      }
      const Split s = attn_bwd_split(n_atom, max_degree);
      EXPECT(s.n == grid && s.per == 4 * apw && attn_bwd_apw(n_atom, max_degree) == apw && attn_bwd_slots(n_atom, max_degree) == slots &&
             covers(s, rows));
    }
    {  // launch_ln_bwd / launch_ln_bwd_edge
      const int groups = std::min(32, std::max(1, (rows + 32 * 1536 - 1) / (32 * 1536)));
      const int slots = (rows + 32 * groups - 1) / (32 * groups);
      const Split s = ln_bwd_split(rows);
      EXPECT(ln_bwd_groups(rows) == groups && s.n == slots && ln_bwd_slots(rows) == slots && s.per == 32 * groups && covers(s, rows));
    }
    {  // launch_rn_bwd / launch_edge_bwd
      const int tile_rows = rows <= 32 * 768 ? 32 : 64;
      const int slots = (rows + tile_rows - 1) / tile_rows;
      const Split s = fused_split(rows);
      EXPECT(s.n == slots && tile_slots(rows) == slots && s.per == tile_rows && covers(s, rows));
    }
    {  // wgrad_add / wgrad_launch
      const int tiles = (rows + 63) / 64;
      const int chunks = std::max(std::min(4, tiles), (tiles + 79) / 80);
      EXPECT(wgrad_chunks(rows) == chunks);
      if (rows > 0) EXPECT(wgrad_slabs(rows) == (rows + 64 * chunks - 1) / (64 * chunks) && covers(split(rows, 64 * chunks), rows));
    }
  }
}

// ---- the bounds as they stood: ensure_train_ws's expression and det_slot_floats, over the expressions of the launchers ----
int old_wgrad_slabs(int rows) {
  const int tiles = (rows + 63) / 64;
  const int chunks = std::max(std::min(4, tiles), (tiles + 79) / 80);
  return (rows + 64 * chunks - 1) / (64 * chunks);
}
int old_ln_bwd_slots(int rows) {
  const int groups = std::min(32, std::max(1, (rows + 32 * 1536 - 1) / (32 * 1536)));
  return (rows + 32 * groups - 1) / (32 * groups);
}
int old_tile_slots(int rows) {
  const int tr = rows <= 32 * 768 ? 32 : 64;
  return (rows + tr - 1) / tr;
}
int old_attn_bwd_slots(int n_atom, int max_degree) {
  if (max_degree <= 16) {
    const int apw16 = std::min(8, std::max(1, (n_atom + 4095) / 4096));
    return (n_atom + 4 * apw16 - 1) / (4 * apw16);
  }
  return 4 * ((n_atom + 4 * 2 - 1) / (4 * 2));
}
size_t old_wpart_floats(int n_atom, int n_edge, int n_struct, int n_attention, int max_degree, int n_tile) {
  const size_t Lc = (size_t)n_attention;
  return (size_t)(D * D + D) * (Lc * (2 * (size_t)old_wgrad_slabs(std::max(n_edge, 1)) + 5 * (size_t)old_wgrad_slabs(n_atom)) +
                                3 * (size_t)old_wgrad_slabs(n_atom) + (size_t)old_wgrad_slabs(n_struct)) +
         (size_t)2 * D * Lc * ((size_t)std::max(old_ln_bwd_slots(std::max(n_edge, 1)), old_tile_slots(std::max(n_edge, 1))) +
                               (size_t)std::max(old_ln_bwd_slots(n_atom), old_tile_slots(n_atom)) +
                               (size_t)old_attn_bwd_slots(n_atom, max_degree)) +
         (size_t)D * n_struct +
         (size_t)4 * D * Lc * (size_t)n_tile;
}
size_t old_det_slot_floats(int n_atom, int n_edge, int n_layer, int n_species, int emb_dim, bool g_update, bool general, bool cgcnn,
                           bool ring) {
  size_t f = 0;
  if (n_edge > 0) {
    const int chunks = n_edge >= (1 << 20) ? 4 : 1;
    if (g_update) f += (size_t)(2 * NG + 2) * D * ((n_edge + 32 * chunks - 1) / (32 * chunks));
    else f += (size_t)n_layer * (NG + 1) * D * ((n_edge + 31) / 32);
  }
  if (n_atom > 0) {
    if (general) {
      const int run = std::max(32, ((n_atom + 127) / 128 + 7) / 8 * 8), n_wg = (n_atom + run - 1) / run;
      const int cin = emb_dim + (ring ? 10 : 0);
      f += (size_t)n_wg * ((size_t)(1 + cin) * D + (cgcnn ? (size_t)93 * emb_dim : (size_t)n_species * emb_dim) + (ring ? 30 : 0));
    } else {
      const int run = std::max(32, (n_atom + 127) / 128), n_wg = (n_atom + run - 1) / run;
      f += (size_t)n_wg * n_species * D + (size_t)n_species * (emb_dim + 1) * D;
    }
  }
  return f;
}

void check_bounds() {
  struct Shape {
    int n_atom, n_edge, n_struct, n_layer, max_degree, n_tile;
  };
  const Shape shapes[] = {
      {2304, 27648, 128, 7, 12, 880},      // a QM9 batch of 128
      {288, 3456, 16, 7, 12, 110},         // ... of 16
      {5, 0, 2, 3, 0, 0},                  // no edges
      {40, 300, 3, 0, 9, 10},              // no LocalAttention layers
      {1, 1, 1, 1, 1, 1},
      {1000, 70000, 9, 2, 70, 0},          // atoms above 64 neighbours
      {18432, 221184, 1024, 7, 12, 7000},  // batch 1024: 64-row tiles, two atoms per wave
      {90000, 1100000, 4000, 5, 16, 0},    // past every switch
  };
  for (const Shape& s : shapes) {
    EXPECT(wpart_slot_floats(s.n_atom, s.n_edge, s.n_struct, s.n_layer, s.max_degree, s.n_tile) ==
           old_wpart_floats(s.n_atom, s.n_edge, s.n_struct, s.n_layer, s.max_degree, s.n_tile));
    for (int v = 0; v < 8; ++v) {  // g_update or base; species table, ring, cgcnn, ring + cgcnn
      const bool g_update = v & 1, ring = v & 2, cgcnn = v & 4, general = ring || cgcnn;
      EXPECT(det_slot_floats(s.n_atom, s.n_edge, s.n_layer, 100, 64, g_update, general, cgcnn, ring) ==
             old_det_slot_floats(s.n_atom, s.n_edge, s.n_layer, 100, 64, g_update, general, cgcnn, ring));
    }
  }
  EXPECT(det_slot_floats(0, 0, 7, 100, 64, true, false, false, false) == 0);
}

}  // namespace

int main() {
  check_bump();
  check_partitions();
  check_bounds();
  return finish("scann_train_check");
}

// Internal declarations shared by the HIP kernels (scann_kernels.hip) and the C-ABI runtime
// (scann_runtime.cpp).  Not part of the public boundary (include/scann_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace scann {

constexpr int D = 128;           // local_dim = global_dim = dense_out (all shipped configs)
constexpr int NHEAD = 8;         // num_head
constexpr int HDIM = D / NHEAD;  // 16
constexpr int NG = 20;           // Gaussian basis size (scann_model.py:378)
constexpr int LDS_STRIDE = 132;  // floats per staged row: 128 + 4 pad (conflict-free b128 A-fragment reads)
constexpr int TE_MAX = 64;       // edge rows per edge tile (two 32-row MFMA row tiles)
constexpr int TA = 64;           // atom rows per atom tile (two 32-row MFMA row tiles)
constexpr int TQ = 24;           // atoms per EDGE tile (the query-row buffer of edge_kernel)
constexpr int WPACK = D * D;     // floats in one packed 128x128 weight (fp32 fragment order, or its split-fp16 image: same bytes)
constexpr float WSCALE = 256.f;  // split-fp16 weights are stored times 2^8 (their lo parts stay normal fp16 numbers); exact inverse in the epilogues
constexpr float WMAX = 65504.f / WSCALE;  // largest weight magnitude the fp16 hi part can hold

// Inverted dropout keyed by (seed, tag, element index): the backward pass regenerates the identical mask.
// Returns 0 (dropped) or 1/(1-p).
__host__ __device__ inline float drop_scale(unsigned long long seed, unsigned tag, size_t idx, float p) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1) + ((unsigned long long)tag << 48);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(z >> 40) * (1.0f / 16777216.0f);
  return u < p ? 0.f : 1.0f / (1.0f - p);
}
// Monte Carlo dropout (scann_predict_mc): the masks of sample t of structure s are drop_scale(mc_seed(seed, t, key_s), tag, i, p) with the
// training forward's tags and an element index i LOCAL to the structure -- (atom - first atom) * local_dim + column for the two Dropout(0.1)
// layers, (edge - first edge) * num_head + head for the attention weights -- so that a structure's samples do not depend on its batch.
__host__ __device__ inline unsigned long long mc_mix(unsigned long long z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline unsigned long long mc_seed(unsigned long long seed, unsigned t, unsigned long long key) {
  return mc_mix(mc_mix(seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)t + 1)) + 0x9E3779B97F4A7C15ull * (key + 1));
}
// Shapley sampling (scann_shapley): permutation p of a structure of n atoms with key key_s, a function of (seed, key_s, p, n) only.
//   base = mc_seed(seed, p, key_s);  out = 0, 1, .., n - 1;
//   for i = n - 1 down to 1:  u = mc_mix(base + 0x9E3779B97F4A7C15 * (i + 1)) >> 32        (a 32-bit draw per step, counter-based)
//                             k = (u * (i + 1)) >> 32                                      (multiply-high range reduction: 0 <= k <= i)
//                             swap out[i], out[k]
// out[j] = the structure-local atom added at position j of the walk.  (The draw of a step does not depend on the swaps before it, so a
// kernel may form all draws in parallel and leave the swaps to one thread: shapley_draw is the draw, the swaps are the loop below.)
__host__ __device__ inline unsigned shapley_draw(unsigned long long base, int i) {  // k of step i
  const unsigned long long u = mc_mix(base + 0x9E3779B97F4A7C15ull * ((unsigned long long)i + 1)) >> 32;
  return (unsigned)((u * ((unsigned long long)i + 1)) >> 32);
}
__host__ __device__ inline void shapley_permutation(unsigned long long seed, unsigned long long key, int p, int n, int32_t* out) {
  const unsigned long long base = mc_seed(seed, (unsigned)p, key);
  for (int i = 0; i < n; ++i) out[i] = i;
  for (int i = n - 1; i >= 1; --i) {
    const int k = (int)shapley_draw(base, i);
    const int32_t t = out[i];
    out[i] = out[k];
    out[k] = t;
  }
}
// per atom of an MC batch (launch_mc_rows): the first atom and the first edge of its structure, the structure's key
struct McRow {
  int32_t a0, e0;
  unsigned long long key;
};

#ifdef __HIPCC__
// GlobalAttention score of atom i of a structure (attention.py:279-292): sum over j != i of gk_i . gq_j, exact products, fp64 sums, four
// interleaved partial sums per dot product (shared by the forward and by the pooling backward, which must see the SAME scores)
__device__ __forceinline__ double gen_pool_score(const float* __restrict__ gq, const float* __restrict__ gk, int a0, int n, int i, int dg) {
  const float* ki = gk + (size_t)(a0 + i) * dg;
  double agg = 0.0;
  for (int j = 0; j < n; ++j) {
    if (j == i) continue;
    const float* qj = gq + (size_t)(a0 + j) * dg;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
    int k = 0;
    for (; k + 4 <= dg; k += 4) {
      e0 = fma((double)ki[k], (double)qj[k], e0);
      e1 = fma((double)ki[k + 1], (double)qj[k + 1], e1);
      e2 = fma((double)ki[k + 2], (double)qj[k + 2], e2);
      e3 = fma((double)ki[k + 3], (double)qj[k + 3], e3);
    }
    for (; k < dg; ++k) e0 = fma((double)ki[k], (double)qj[k], e0);
    agg += (e0 + e1) + (e2 + e3);
  }
  return agg;
}
// Sum over the 64 lanes of a wave by the xor butterfly 32 down to 1, every lane getting it: the one order of the plain-fp32 kernels
// (scann_generic.hip, scann_generic_train.hip, scann_input_grad.hip), which keep their summation order whatever scann_mma.h does
__device__ __forceinline__ float shfl_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
#endif

// Range guard of the split-fp16 projections (|activation| and |weight| * 2^8 must stay below 65504, the largest fp16): an operand
// that overflows becomes inf in its hi part, the product NaN, and the NaN reaches the statistics of the next LayerNorm.  The
// kernels therefore test every LayerNorm variance (and the one activation that no LayerNorm follows) for finiteness and, on
// failure, store (site << 8 | layer + 1) in a host-pinned word that the entry points returning results check after their
// synchronisation (SCANN_ERR_RANGE).  Sites: 1 layer_norm_g, 2 layer_norm (context), 3 ResidualNorm, 4 after_Lc activation,
// 5 a weight after an optimiser step.  The guard watches the TOP of the range only.  The bottom -- operand rows or kernel columns so
// small that their lo parts are fp16 subnormals and the pair keeps fewer than 22 bits -- costs precision, not finiteness, and no
// statistic downstream shows it; it is decided per checkpoint when the weights are loaded (scann_runtime.cpp: small_operand_reason;
// scann_weights_exact), at no cost per launch.
__device__ __forceinline__ void flag_range(int32_t* flag, int site, int layer) {
  if (flag && *reinterpret_cast<volatile int32_t*>(flag) == 0)  // the first report stands: kernels run in layer order on their stream
    *flag = (site << 8) | (layer + 1);
}
constexpr float RANGE_FINITE = 3.0e38f;  // !(x < RANGE_FINITE): inf or NaN

constexpr unsigned DROP_TAG_ATTN = 2000;   // + layer: Dropout(0.05) on attention weights, element = edge * 8 + head
constexpr unsigned DROP_TAG_EMBED = 1000;  // Dropout(0.1) after dense_embed (scann_model.py:374); ResidualNorm l uses tag l

// One tile of the edge kernel: a run of whole atoms whose CSR rows are contiguous, <= TE edges.
struct EdgeTile {
  int32_t atom_begin, atom_end;
  int32_t edge_begin, edge_end;
};

// Device pointers of one LocalAttention(+ResidualNorm) iteration.  128x128 kernels are stored in
// the MFMA fragment order produced by pack_weight() (see scann_kernels.hip: gemm128).
struct LayerParams {
  // atom-tile kernel
  const float *bg;              // filter_geo bias
  const float *bq;              // query bias
  const _Float16 *W1h, *W3h, *Wqh, *Wf1h, *Wf2h;  // split-fp16 images (pack_weight_f16): filter_geo rows [0,128) (centre) and [256,384)
                                                  // (neighbour), query, ResidualNorm dense_1 / dense_2
  // edge-tile kernel
  const float *bk;              // key bias
  const _Float16 *W2h, *Wkh;    // filter_geo rows [128,256) (geometry) and key as split-fp16 images: what edge_kernel multiplies with
  const _Float16 *Wfh;          // base branch: filter_geo [20,128] zero-padded to K = 32, split-fp16 image
  const float *lng_g, *lng_b;   // layer_norm_g
  const float *ln_g, *ln_b;     // layer_norm
  const float *Wfg, *bfg;       // base branch (g_update False): filter_geo [20,128] raw + bias (backward of the basis filter)
  // ResidualNorm that follows this LocalAttention (applied at the head of the next atom kernel)
  const float *bf1, *bf2, *lnr_g, *lnr_b;
  // fp32 fragment-order images (pack_weight) of the seven 128x128 kernels: the exact-fp32 fallback of the forward (EX kernels)
  const float *W1p, *W2p, *W3p, *Wqp, *Wkp, *Wf1p, *Wf2p;
};

struct HeadParams {
  const float *Wap, *ba;                // after_Lc
  const float *Wgqp, *bgq, *Wgkp, *bgk; // global_attention query / key
  const _Float16 *Wah, *Wgqh, *Wgkh;    // split-fp16 images (atom_kernel mode 2)
  const float *Wb, *bb;                 // bf_property (row-major [128,128])
  const float *wo, *bo;                 // predict_property [128], [1]
};

struct BasisParams {
  const float *Wd, *bd, *Ww, *bw;  // neighbor_d / neighbor_w [20,128]
  const float *cd, *cw;            // Gaussian centres (20 each)
  const _Float16 *Wdh, *Wwh;       // split-fp16 images of the two kernels, K padded to 32 (basis_kernel)
};

// ---- launch wrappers (defined in scann_kernels.hip) -------------------------------------------

// swish(E . W + b) per species -> lut[n_species,128]   (Embedding + dense_embed folded at load time)
void launch_embed_lut(const float* emb, const float* W, const float* b, int n_species, int emb_dim,
                      float* lut, hipStream_t s);

// geom0[e,:] = swish(G(dist) Wd + bd) * swish(G(weight) Ww + bw)         (g_update)
// or gd[e, 0:20] = G(dist) (base branch: the per-layer filter consumes the raw basis)
void launch_basis(const BasisParams& p, const float* dist, const float* weight, int n_edge,
                  float* geom, hipStream_t s);
void launch_basis_raw(const float* cd, const float* dist, int n_edge, float* gd, hipStream_t s);

// General embedding (use_ring / feature="cgcnn"); the plain Embedding path uses the per-species LUT instead.
struct EmbedArgs {
  int32_t n_atom, emb_dim;
  const int32_t* atomic;   // [n_atom] (feature="atomic")
  const float* cgcnn;      // [n_atom,92] or null
  const float* ring;       // [n_atom,2] or null
  const float *emb;        // embed_atom/embeddings [n_atoms,emb]
  const float *We, *be;    // embed_atom/kernel [92,emb], bias (cgcnn)
  const float *Wr, *br;    // extra_embed [2,10], [10]
  const float *Wde, *bde;  // dense_embed [emb(+10),128], [128]
  float* c0;               // [n_atom,128]
};
void launch_embed(const EmbedArgs& a, hipStream_t s);

struct AtomArgs {
  const float* x;          // [n_atom,128] input rows (context of previous layer, or the LUT)
  const int32_t* x_index;  // optional row indirection (layer 0: atomic number -> LUT row) or null
  int32_t n_atom;
  // ResidualNorm (ffn != 0): c = LN(x + W2 swish(W1 x + b1) + b2)
  int32_t ffn;
  const _Float16 *Wf1h, *Wf2h;   // split-fp16 images (pack_weight_f16)
  const float *bf1, *bf2, *lnr_g, *lnr_b;
  float* c;                // [n_atom,128] centres out (always written)
  // training only: Dropout(0.1) on the staged rows (layer 0, scann_model.py:374) or on the ResidualNorm branch
  // (attention.py:29); drop_p == 0 in inference
  float drop_p;
  uint32_t drop_tag;
  unsigned long long drop_seed;
  // projections
  int32_t mode;            // 0: P1,P3,q (g_update)  1: q only (base)  2: readout (after_Lc -> gq, gk)
  const _Float16 *WAh, *WBh, *WCh, *WDh;  // split-fp16 images: mode 0: W1, W3, Wq | mode 1: -, -, Wq | mode 2: after_Lc, -, ga query, ga key
  const float *bA;         // mode 0: bg        | mode 2: after_Lc bias
  const float *bC;         // mode 0/1: bq      | mode 2: ga query bias
  const float *bD;         // mode 2: ga key bias
  float *oA, *oB, *oC;     // mode 0: P1,P3,q | mode 1: -, -, q | mode 2: -, gk, gq
  // training forward: ResidualNorm intermediates the backward would otherwise recompute (null in inference), [n_atom,128]:
  // pre1 = x W1 + b1, H1 = swish(pre1), T2 = x + drop(H1 W2 + b2) (the LayerNorm input)
  float *keep_pre1, *keep_H1, *keep_T2;
  float *keep_preA, *keep_z;   // mode 2, training forward: after_Lc pre-activation and swish output [n_atom,128]
  unsigned long long* stamps;  // diagnostic build (-DSCANN_STAMPS, env SCANN_STAMP_ATOM=1) only: [n_tiles,16] phase clocks
  int32_t* range_flag;         // host-pinned range-guard word (flag_range) or null
  int32_t layer;               // layer whose projections this launch computes (for the range-guard message)
  // exact-fp32 projections (EX instantiation): Wf1h, Wf2h, WAh .. WDh then point at fp32 fragment-order images (pack_weight)
  int32_t exact;
  // mode 2, inference outputs (scann_set_outputs): after_Lc = swish(c Wa + ba) [n_atom,128] is stored here (the ZOUT instantiation), or null
  float* out_z;
  // Monte Carlo dropout (the MC instantiation, scann_predict_mc): per-atom structure table; the masks are keyed by mc_seed(drop_seed, mc_t,
  // key) and the structure-local element index.  Null otherwise
  const McRow* mc_rows;
  uint32_t mc_t;
  // model set (the SET instantiation, scann_forward_models): n_member members' launches in one grid of n_member x the tiles of one, member m
  // of workgroup b = b / tiles; its pointers are member 0's plus m times a byte stride -- m_w for the weight images (Wf*, bf*, lnr_*,
  // W*h, b*), m_x for x, m_o for c, oA, oB, oC.  x_index is shared.  n_member == 0: not a set launch
  int32_t n_member;
  int64_t m_w, m_x, m_o;
};
// n_cu: compute units of the device; force_rows: the handle's SCANN_ATOM_ROWS (0: automatic) -- the tile height is the launch's choice
void launch_atom(const AtomArgs& a, hipStream_t s, int n_cu, int force_rows);

struct EdgeArgs {
  const EdgeTile* tiles;       // whole atoms per tile: <= TE_MAX edges and <= TQ atoms
  int32_t n_tile;
  int32_t xcd_remap;           // contiguous run of tiles per XCD
  // atoms with more than 64 neighbours: their edges are cut into chunk tiles of one atom each; tile_part[tile] = partial slot
  // of a chunk tile, -1 for ordinary tiles (null: no such atom in the batch); a chunk tile leaves (running max, sum,
  // unnormalised context) per column in part_buf[slot][3][128] for edge_merge_kernel
  const int32_t* tile_part;
  float* part_buf;
  int32_t g_update;
  // The piece-major inference kernels (BLK: g_update, neither exact nor keep) run on the batch's TILE-ORDER side (scann_dbatch::f_tiles,
  // scann_batch_upload): tiles, edge_offset, edge_col, edge_row, dist and edge_weight are then numbered in the order the filled plan
  // puts the atoms in -- edge_col still holds the caller's atom rows, edge_row the tile-order index of the centre -- and every
  // [n_atom,128] tensor, species, mc_rows and attn_out stay in the caller's order: a tile finds the caller's row of its atom in slot s
  // in tile_atom[tile][s] (slots past its last atom repeat it), the row of the tensors c, P1, P3, q of THIS launch in tile_cen (=
  // tile_atom, or the atomic numbers when species is set) and the atom's first edge in the caller's numbering in tile_edge0.  The tables
  // are addressed by the tile's number alone: their loads do not wait for the tile descriptor.  Null for every other family
  const int32_t *tile_atom, *tile_cen, *tile_edge0;  // [n_tile][TQ]
  const int32_t* edge_offset;  // [n_atom+1]
  const int32_t* edge_col;     // [n_edge]
  const int32_t* edge_row;     // [n_edge] centre atom of each edge
  float* geom;                 // [n_edge,128] in/out (g_update)
  // training forward: per-edge tensors the backward would otherwise recompute (null in inference):
  // V = G.W2 + P1[i] + P3[j], T = swish(V) + G (LayerNorm_g input), ang = c[j] * geom', K = ang.Wk + bk -- all [n_edge,128]
  float *keep_V, *keep_T, *keep_ang, *keep_K;
  float* geom_out;             // where geom' goes (null: in place) -- keep-mode writes each layer's geometry to its own slice
  int32_t tile_rows;           // 32 | 64: edge rows per tile of this batch's plan (selects the kernel instantiation)
  int32_t n_edge;              // edges of the batch: geom has ONE SPARE ROW behind them (scann_batch_upload), the dump row of edge-less tiles
  int32_t geom_rows;           // the geometry tensors are [n_edge,128] ROWS (training, debug and exact forwards: someone else reads them); 0: piece-major tiles
  int32_t geom_dead;           // last layer of an inference forward: nobody reads geom' (scann_model.py:415-421 threads it to the NEXT layer only)
  const float* gd;             // [n_edge,20] raw distance basis (base)
  const float* edge_weight;    // [n_edge] (base; g_update with fuse_basis: the second input of the basis MLP)
  // first layer of an inference forward (g_update, 64-row tiles): the tile's geometry rows are COMPUTED from (dist, weight) in the
  // prologue -- basis_kernel's arithmetic on the tile's rows -- instead of being written by basis_kernel and read back here
  int32_t fuse_basis;
  // ... and, with the per-species embedding table (feature = "atomic", no ring input), the layer's atom rows c, P1, P3, q are
  // functions of the atomic number alone: they are [n_species,128] tables computed when the weights change, the kernel indexes them
  // through species[atom], and the first atom launch of the forward does not happen at all
  const int32_t* species;      // [n_atom] atomic numbers, or null: c, P1, P3, q are per-atom arrays
  const float* dist;           // [n_edge]
  BasisParams basis;
  const float *c, *P1, *P3, *q;  // [n_atom,128]
  float* ctx;                  // [n_atom,128] out: LayerNorm(context)
  // training with use_drop: Dropout(0.05) on the attention weights (attention.py:116,191); 0 in inference
  float attn_drop_p;
  uint32_t attn_drop_tag;
  unsigned long long attn_drop_seed;
  unsigned long long* stamps;  // diagnostic build (-DSCANN_STAMPS) only: [n_tile,16] phase clocks, else null
  int32_t* range_flag;         // host-pinned range-guard word (flag_range) or null
  int32_t layer;
  int32_t exact;               // exact-fp32 projections (EX instantiation): p.W2h, p.Wkh then point at fp32 fragment-order images
  LayerParams p;
  // inference outputs (scann_set_outputs): the layer's attention weights (attention.py:189) per (edge, head), [n_edge, NHEAD] (the ATTN
  // instantiation), or null.  A chunk tile stores exp(e - m_chunk) unnormalised; launch_attn_merge finishes those rows
  float* attn_out;
  // Monte Carlo dropout on the attention weights (the MC instantiation, scann_predict_mc; attn_drop_p > 0): as AtomArgs::mc_rows / mc_t
  const McRow* mc_rows;
  uint32_t mc_t;
  // model set (the SET instantiation): n_member x n_tile workgroups, linear (XCD-remapped) index t -> member t / n_tile, tile t % n_tile;
  // byte strides between members: m_w for p and basis, m_r for c, P1, P3, q (per-species tables: the weight block's stride), m_a for geom,
  // ctx and part_buf.  tiles, CSR, dist, edge_weight, gd (model-independent Gaussians), species are shared.  n_member == 0: not a set launch
  int32_t n_member;
  int64_t m_w, m_r, m_a;
};
void launch_edge(const EdgeArgs& a, hipStream_t s);
// softmax merge of the chunk tiles of every big atom (+ unscaled-query residual + LayerNorm, attention.py:189-214)
// inference outputs: the attention weights of the chunk tiles of atoms with more than `chunk` neighbours, exp(e - m_chunk) as the
// chunk tiles stored them, scaled by exp(m_chunk - M) / S (the merged softmax state of edge_merge_kernel) in place
void launch_attn_merge(const int32_t* big_tab, int n_big, const float* part_buf, const int32_t* edge_offset, int chunk, float* attn, hipStream_t s);
void launch_edge_merge(const int32_t* big_tab, int n_big, const float* part_buf, const float* q, const float* ln_g,
                       const float* ln_b, float* ctx, int32_t* range_flag, int layer, hipStream_t s);
// ... for n_member members of a model set at once: member m's part_buf, q, ctx lie m_a bytes, its ln_g / ln_b m_w bytes behind member 0's
void launch_edge_merge_set(const int32_t* big_tab, int n_big, const float* part_buf, const float* q, const float* ln_g, const float* ln_b,
                           float* ctx, int32_t* range_flag, int layer, int n_member, int64_t m_a, int64_t m_w, hipStream_t s);

// ---- generic-width forward (scann_generic.hip): plain fp32 kernels for local_dim / num_head / global_dim / dense_out other than 128 / 8 ----
struct GenSeg {
  const float* p;      // [*, w] rows
  const int32_t* idx;  // row r of the operand reads p[idx[r]] (null: p[r])
  int32_t w;
};
struct GenDenseArgs {
  GenSeg seg[3];
  int32_t n_seg;  // x = concat of the segments' rows ...
  int32_t prod;   // ... or (prod) the elementwise product of segments 0 and 1, both K wide
  const float* W;  // [K, N] row-major (the Keras kernel)
  const float* b;  // [N] or null
  int32_t K, N, rows;
  int32_t act;  // 0 none, 1 swish
  const float* res;        // added after the activation: res[(res_idx ? res_idx[r] : r)][o]
  const int32_t* res_idx;
  const float* row_scale;  // [rows] or null: multiplied last
  float* Y;                // [rows, N]
  // training forward (zero / null in inference): the pre-activation kept for the backward, Dropout on the layer's output
  float* pre;              // [rows, N] or null
  float drop_p;
  uint32_t drop_tag;
  unsigned long long drop_seed;
  // Monte Carlo dropout (scann_predict_mc): structure-local masks keyed by mc_seed(drop_seed, mc_t, key) of the row's atom, null otherwise
  const McRow* mc_rows;
  uint32_t mc_t;
};
void launch_gen_dense(const GenDenseArgs& a, hipStream_t s);
void launch_gen_layernorm(const float* X, const float* res, const float* gamma, const float* beta, int rows, int N, float* Y, hipStream_t s);
void launch_gen_gauss(const float* x, const float* centres, int n, float* out, hipStream_t s);
void launch_gen_mul(const float* a, const float* b, size_t n, float* out, hipStream_t s);
void launch_gen_attn(const float* q, const float* K, const int32_t* edge_offset, int n_atom, int d, int H, int max_degree, float* ctx, hipStream_t s,
                     float drop_p = 0.f, unsigned drop_tag = 0, unsigned long long drop_seed = 0, float* attn_out = nullptr);  // attn_out non-null
                     // (inference outputs): the normalised attention weights are stored, [n_edge, H]
// Monte Carlo dropout on the attention weights (scann_predict_mc): structure-local masks (McRow), drop_p > 0
void launch_gen_attn_mc(const float* q, const float* K, const int32_t* edge_offset, int n_atom, int d, int H, int max_degree, float* ctx, hipStream_t s,
                        float drop_p, unsigned drop_tag, unsigned long long drop_seed, const McRow* mc_rows, uint32_t mc_t);
// scann_predict_mc: rows[a] for every atom from the structure offsets and the per-structure keys (null: all 0)
void launch_mc_rows(const int32_t* mol_offset, const int32_t* edge_offset, const unsigned long long* keys, int n_struct, int n_atom, McRow* rows,
                    hipStream_t s);
// scann_predict_mc: per column j of a [T, n] sample matrix, the mean and the unbiased standard deviation (fp64, samples summed in order)
void launch_mc_reduce(const float* samples, int T, int n, float* mean, float* std_out, hipStream_t s);
// rep_out non-null (training forward): the pooled rows [n_struct, dg] are stored and the property head is NOT evaluated;
// bf_out non-null (inference outputs): bf_property [n_struct, dout] is stored
void launch_gen_readout(const int32_t* mol_offset, int n_struct, int max_atoms, const float* gq, const float* gk, int dg, int dout, int use_ga_norm,
                        int relu_out, const float* Wb, const float* bb, const float* wo, const float* bo, float* ga_attn, float* y, hipStream_t s,
                        float* rep_out = nullptr, float* bf_out = nullptr);

// ---- generic-width training (scann_generic_train.hip) ----
struct GenTransDesc {  // WT[dst + o * kn + kk] = W[src + (k0 + kk) * N + o]: rows [k0, k0 + kn) of a row-major [*, N] kernel, transposed
  int64_t src, dst;
  int32_t k0, kn, N;
};
struct GenDwArgs {
  GenSeg seg[3];  // the forward operand X, assembled as in GenDenseArgs
  int32_t n_seg, prod;
  const float* dZ;  // [rows, N] gradient of the layer's pre-activation
  int32_t K, N, rows;
  float *dW, *db;   // [K, N], [N] (null: no bias): ACCUMULATED into
  float* part;      // gen_dw_part_floats(rows, K, N) floats of per-slab partial tiles
  int32_t slab_rows;  // (set by the launcher)
};
int gen_dw_slabs(int rows, int K, int N);
size_t gen_dw_part_floats(int rows, int K, int N);
void launch_gen_transpose(const GenTransDesc* descs, int n_desc, int max_elems, const float* W, float* WT, hipStream_t s);
void launch_gen_act_bwd(const float* dY, const float* pre, const float* row_scale, int rows, int N, float drop_p, unsigned drop_tag,
                        unsigned long long drop_seed, float* out, hipStream_t s);
void launch_gen_mul_gather(const float* a, const float* B, const int32_t* idx, const float* c, int rows, int N, float* out, hipStream_t s);
void launch_gen_relu(float* y, int n, hipStream_t s);
void launch_gen_dense_dw(const GenDwArgs& a, hipStream_t s);
int gen_ln_chunks(int rows);  // row chunks of the gamma / beta sums: `part` holds gen_ln_chunks(rows) * 2 * N floats
void launch_gen_layernorm_bwd(const float* X, const float* res, const float* gamma, const float* dY, int rows, int N, float* dX, float* stats,
                              float* part, float* dgamma, float* dbeta, hipStream_t s);
void launch_gen_attn_bwd(const float* q, const float* K, const int32_t* edge_offset, int n_atom, int d, int H, int max_degree, const float* dctx,
                         float drop_p, unsigned drop_tag, unsigned long long drop_seed, float* dq, float* dK, hipStream_t s);
void launch_gen_pool_bwd(const int32_t* mol_offset, int n_struct, int max_atoms, const float* gq, const float* gk, int dg, int use_ga_norm,
                         const float* drep, float* dgq, float* dgk, hipStream_t s);
void launch_gen_edge_to_atom(const int32_t* edge_offset, const int32_t* in_off, const int32_t* in_edge, const float* S_out, const float* S_in,
                             const float* P_a, const float* P_b, const float* acc, int n_atom, int d, float* out, hipStream_t s);
// part: ceil(n_atom / 64) * n_species * emb floats of per-chunk sums
void launch_gen_table_grad(const int32_t* atomic, int n_atom, const float* dV, int emb, int n_species, float* part, float* dTable, hipStream_t s);

struct ReadoutArgs {
  const int32_t* mol_offset;  // [n_struct+1]
  int32_t n_struct;
  int32_t max_atoms;          // largest structure (sizes the dynamic LDS score buffer)
  const float *gq, *gk;       // [n_atom,128]
  int32_t use_ga_norm, relu_out;
  HeadParams p;
  float* ga_attn;             // [n_atom]
  float* y;                   // [n_struct]
  float* bf_out;              // [n_struct,128] bf_property = swish(rep Wb + bb) (scann_model.py:437-442), or null (inference outputs)
  // model set: n_member x n_struct workgroups, member m = b / n_struct; byte strides between members: m_w (p), m_a (gq, gk), m_g (ga_attn),
  // m_y (y); relu_out is then a bit mask (bit m: member m's mrelu).  bf_out null.  n_member == 0: not a set launch
  int32_t n_member;
  int64_t m_w, m_a, m_g, m_y;
};
void launch_readout(const ReadoutArgs& a, hipStream_t s);

// scann_ablate.hip (scann_ablate_pooling): y(S) of the readout for the kept sets of one mode, one workgroup per structure
struct AblateArgs {
  const int32_t* mol_offset;  // [n_struct+1]
  int32_t n_struct, max_atoms;
  const float *gq, *gk;       // [n_atom, dg] of the batch's last forward
  int32_t dg, dout;           // global_dim, dense_out (128 / 128 on the MFMA kernel)
  int32_t use_ga_norm, relu_out, mode;  // mode: SCANN_ABLATE_*
  const float *Wb, *bb, *wo, *bo;       // bf_property [dg, dout], [dout]; predict_property [dout], [1]
  const float* ga_attn;       // [n_atom] the forward's GlobalAttention scores (the ranking)
  float* y_abl;               // [n_atom] entry e of structure s at mol_offset[s] + e
  int32_t* order;             // [n_atom] structure-local atom index by rank, or null
};
size_t ablate_lds_bytes(int max_atoms, int dg);  // dynamic LDS of a launch whose largest structure has max_atoms atoms
hipError_t launch_ablate(const AblateArgs& a, bool mfma, hipStream_t s);

// scann_shapley.hip (scann_shapley): Shapley sampling of the pooling game -- the pair matrix of every structure once, the prefix values of
// n_perm walks per structure, then the fp64 reduction.  LDS of the walk: ablate_lds_bytes (the same layout)
struct ShapleyArgs {
  const int32_t* mol_offset;  // [n_struct+1]
  int32_t n_struct, n_atom, max_atoms, n_perm;
  const float *gq, *gk;       // [n_atom, dg] of the batch's last forward
  int32_t dg, dout;           // global_dim, dense_out (128 / 128 on the MFMA kernel)
  int32_t use_ga_norm, relu_out;
  const float *Wb, *bb, *wo, *bo;  // bf_property [dg, dout], [dout]; predict_property [dout], [1]
  unsigned long long seed;
  const unsigned long long* keys;  // [n_struct] or null (all 0)
  const int32_t* perms_in;    // [n_perm][n_atom] explicit walks (validated on the host), or null: sampled
  const int64_t* pair_offset; // [n_struct] first float of each structure's n x n pair matrix
  float* pair;                // pair[pair_offset[s] + c * n + i] = k_i . q_c, 0 for c == i
  float* values;              // [n_perm][n_atom] v of the first j + 1 atoms of walk p at p * n_atom + mol_offset[s] + j
  int32_t* perms;             // [n_perm][n_atom] the walks: structure-local atom by position
  double *shapley, *stderr_out;  // [n_atom]
  double *baseline, *full;    // [n_struct]
};
constexpr int SHAPLEY_PCHUNK = 4;  // walks per workgroup of shapley_walk_kernel (no result depends on it)
// ev: null, or four events recorded before the pair kernel, behind it, behind the walks and behind the reduction (scann_shapley_profile)
hipError_t launch_shapley(const ShapleyArgs& a, bool mfma, hipStream_t s, hipEvent_t* ev = nullptr);
// fp64 reduction of walks (the host twin of shapley_reduce_kernel; scann_shapley_reduce_host)
void shapley_reduce_host(const float* values, const int32_t* perms, const int32_t* mol_offset, int n_struct, int n_perm, const double* baseline,
                         double* shapley, double* stderr_out, double* full);

// scann_rollout.hip (scann_attention_rollout): the first `depth` attention maps of one forward composed per structure
struct RolloutArgs {
  const int32_t *mol_offset, *edge_offset, *edge_col;  // [n_struct+1], [n_atom+1], [n_edge] (global atom rows)
  int32_t n_struct, n_edge, max_atoms;
  int32_t num_head, head, depth;  // head: -1 = the mean over the heads
  float residual;
  const float* attn;           // [depth][n_edge][num_head]: layers 0 .. depth-1 of the forward's output block (null: a batch without edges)
  const float* ga;             // [n_atom] the forward's GlobalAttention scores
  float* abar;                 // [depth][n_edge] scratch: the edge weights of every layer
  float* attribution;          // [n_atom]
  float* rollout;              // the structures' n x n row-major blocks one after another, or null
  const int64_t* roll_offset;  // [n_struct] first float of each structure's block (with rollout)
};
int rollout_slab(int max_atoms);          // columns per workgroup for a launch whose largest structure has max_atoms atoms
size_t rollout_lds_bytes(int max_atoms);  // dynamic LDS of such a launch
hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s);

// Host-side edge-tile plan of a packed batch (scann_pack.cpp): whole atoms per tile, <= tile_rows edges and <= tile_atoms
// atoms; atoms with more than TE_MAX neighbours become chunk tiles when allow_chunks.  Validates the CSR arrays and, with
// fill_edge_row, fills edge_row (centre atom of each edge).  Returns SCANN_OK or a negative status with `err` set.
int plan_tiles(const int32_t* mol_offset, int32_t B, const int32_t* edge_offset, const int32_t* edge_col, int32_t A, int32_t E,
               int tile_rows_req, int tile_atoms, bool allow_chunks, std::vector<EdgeTile>& tiles, std::vector<int32_t>& tile_part,
               std::vector<int32_t>& big_tab, std::vector<int32_t>& edge_row, int* tile_rows_out, int32_t* max_degree,
               int32_t* n_slot, std::string& err, bool fill_edge_row = true);
// The filled plan (scann_plan_tiles_filled, include/scann_hip.h) behind `contiguous`, plan_tiles' result at `rows` edges per tile, of
// which n_big atoms are chunked: atom_row [A], tile_offset [A + 1], tiles.  Returns whether the plan is filled (false: the identity
// order, the offsets as they came and `contiguous`).
bool plan_tiles_filled(const int32_t* mol_offset, int32_t B, const int32_t* edge_offset, int32_t A, int rows, int tile_atoms,
                       const std::vector<EdgeTile>& contiguous, int32_t n_big, std::vector<int32_t>& atom_row,
                       std::vector<int32_t>& tile_offset, std::vector<EdgeTile>& tiles);
// The tile-order side of a batch for the piece-major inference edge kernels (scann_batch_upload, behind the input copy and the device
// packing).  Always: the per-tile slot tables tile_atom [n_tile][TQ] = the caller's atom row of the tile's atom in slot s (slots past
// the tile's last atom repeat it), tile_edge0 = that atom's first edge in the caller's numbering, tile_species = its atomic number
// (with `atomic`).  With atom_row (a filled plan): the tile-order copies of the edges -- col (still the caller's atom rows), dist,
// weight, and row = the tile-order index of the centre atom.
struct TileOrderArgs {
  const EdgeTile* tiles;
  int32_t n_tile, n_atom;
  const int32_t* atom_row;      // [n_atom] or null (identity)
  const int32_t* tile_offset;   // [n_atom+1] offsets in tile order (with atom_row)
  const int32_t* edge_offset;   // [n_atom+1] the caller's
  const int32_t* atomic;        // [n_atom] or null
  const int32_t* col;
  const float *dist, *weight;   // [n_edge] the caller's order
  int32_t *tile_atom, *tile_edge0, *tile_species;  // [n_tile][TQ]
  int32_t *out_col, *out_row;
  float *out_dist, *out_weight; // [n_edge] tile order (with atom_row)
};
void launch_tile_order(const TileOrderArgs& a, hipStream_t s);
// edge_row[e] = centre atom of edge e from the CSR offsets, on the device (scann_batch_upload: behind the input copy)
void launch_edge_row(const int32_t* edge_offset, int n_atom, int32_t* edge_row, hipStream_t s, int32_t* zero_word = nullptr);

// Padded Keras input -> packed CSR on the device (scann_upload_padded): the payload arrays of the padded dict as they came over the bus.
struct PackPaddedArgs {
  int32_t B, M, N, n_species;
  const int32_t* row_of;        // [B*M] packed row of every padded atom slot, -1 = padded (host: scann_count_padded)
  const int32_t* edge_offset;   // [n_atom+1]
  const int32_t* atomic;        // [B*M]
  const int32_t* neighbors;     // [B*M*N] intra-structure atom index
  const void* neighbor_mask;    // [B*M*N] 1- or 4-byte elements
  int32_t mask_size;
  const float *weight, *dist;   // [B*M*N]
  int32_t* out_atomic;          // [n_atom]
  int32_t* out_col;             // [n_edge] global atom row of the neighbour
  float *out_dist, *out_weight; // [n_edge]
  int32_t* flag;                // |= 1: an unmasked slot points at a padded atom, |= 2: atomic number outside the embedding table
};
void launch_pack_padded(const PackPaddedArgs& a, hipStream_t s);

// Host-side permutation of a row-major [128,128] (in,out) kernel into MFMA fragment order.
void pack_weight(const float* W, int ld, float* Wp);
// Split-fp16 image of rows [0, k_real) of a row-major [*,128] kernel for v_mfma_f32_32x32x16_f16 (edge_kernel: mma_split):
// [wave 4][k-step ks][plane hi|lo][lane 64][8 halfs], element j of lane l = fp16 part of WSCALE * W[16 s + 8 (l >> 5) + j][32 w + (l & 31)]
// (zero for k >= k_real).  4 * ks * 2 * 64 * 8 halfs = ks * 2048 floats' worth of bytes.
void pack_weight_f16(const float* W, int ld, int k_real, int ks, uint16_t* out);

}  // namespace scann

// Hand-written CDNA4 (gfx950) kernels for the SCANN / SCANN+ forward hot path.
//
// Layout: structures are packed -- atoms [n_atom,128] and CSR edges [n_edge,128] -- so
// the reference's padded [B,M,N,d] tensors (attention.py:136-212) are never materialised.  Every
// dense projection is a split-fp16 MFMA product with fp32 accumulation (v_mfma_f32_32x32x16_f16, three
// products per operand pair: fp32 accuracy at 3/16 of the fp32-MFMA time; scheme and evidence in the
// edge-tile section) of a row tile staged in LDS as hi / lo planes against a 128x128 weight that each
// wave streams straight from L2 into registers in fragment order (no LDS staging of weights: a wave
// owns 32 output columns, so every weight element is read by exactly one wave of the workgroup).
//
// Kernels (one launch each per LocalAttention iteration, see scann_runtime.cpp: run_forward):
//   atom_kernel   : [ResidualNorm of previous layer] -> centres c; P1 = c W1 + bg, P3 = c W3, q = c Wq + bq
//                   (attention.py:37-40, :160, and the centre/neighbour thirds of filter_geo :142-151)
//                   (atom_wide_kernel: the same body on 96-row tiles, for the ResidualNorm launches of a plain inference forward whose
//                   32- / 64-row tiles would leave a CU more than two -- launch_atom picks the height from n_atom and the CU count)
//   edge_kernel   : per tile of <=64 edges (whole atoms): U = G W2; geom' = LN_g(swish(U+P1[i]+P3[j])+G)
//                   (:141-153); ang = c[j]*geom' (:136,:157); K = ang Wk + bk (:163);
//                   per (atom, head) softmax over its edges and ctx = LN(sum attn K + q) (:180-214)
//   readout_kernel: GlobalAttention + bf_property + predict_property (attention.py:267-318,
//                   scann_model.py:437-447), one workgroup per structure (pair energies: exact-fp32 MFMA)
//   basis_kernel  : Gaussian expansion + neighbor_d/neighbor_w MLP (custom_layers.py:63-65,
//                   scann_model.py:378-389)
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "scann_internal.h"
#include "scann_mma.h"

namespace scann {

// ---- atom-tile kernel ------------------------------------------------------------------------------
//
// One workgroup (4 waves) per tile of 64 (or, for small launches, 32: launch_atom) atom rows, three (four) workgroups per CU; every projection is a split-fp16 MFMA GEMM
// of the tile (hi / lo planes in ONE LDS buffer in which x, the ResidualNorm hidden row, the centres and -- readout --
// swish(after_Lc) take turns) against a 128x128 weight streamed from L2 in two halves of 32 VGPRs, the next half always
// requested while the current one multiplies.  Everything between the GEMMs happens in the accumulator layout (lane = row,
// 16 columns): bias, swish, dropout, the residual (x stays in registers, exact fp32), LayerNorm statistics (lane pair ->
// LDS -> the row's four waves), and the output stores (16-byte pieces).
//   FFN  : c = LN(x + drop(W2 swish(W1 x + b1) + b2))                       ResidualNorm of the previous layer, attention.py:37-40
//   MODE 0: P1 = c W1 + bg, P3 = c W3, q = c Wq + bq                        centre / neighbour thirds of filter_geo :142-151, query :160
//   MODE 1: q only (base branch)           MODE 2: z = swish(c Wa + ba); gq = z Wgq + b, gk = z Wgk + b   (scann_model.py:424, attention.py:269-272)

// EX: exact-fp32 projections (scann_mma.h: the fallback run_forward takes when the split-fp16 range guard fired)
// KEEP: the training forward's instantiation (Dropout, keep_* stores); never exact
// (workgroups per CU: three at 64 rows, four at 32 -- except where the register allocator could not be kept below the limit without
// spilling and occupancy is not what bounds the launch: the exact-fp32 re-run at 64 rows (1/16 of the matrix rate), the base branch's
// query-only kernel at 32 rows; tests/test_host.py reads scratch sizes and register counts from the built library)
// ZOUT: mode 2 of an inference forward that returns after_Lc (scann_set_outputs): z is stored to out_z as the training forward stores
// keep_z (a compile-time flag: a branch around a store in these kernels has cost a spill before, tests/test_host.py)
// MC: Monte Carlo dropout of an inference forward (scann_predict_mc) -- the Dropout(0.1) of the staged rows (!FFN: after dense_embed) or of
// the ResidualNorm branch (FFN) applied unconditionally, with structure-local masks (scann_internal.h: mc_seed); no keep_* stores
//
// MC: the row's structure seed and the structure-local index of its element 0 (McRow of the atom)
__device__ __forceinline__ void mc_row_key(const AtomArgs& a, int atom, unsigned long long& seed, size_t& e) {
  const McRow m = a.mc_rows[atom];
  seed = mc_seed(a.drop_seed, a.mc_t, m.key);
  e = (size_t)(atom - m.a0) * D;
}
__device__ __forceinline__ float4 mc_drop4(unsigned long long seed, unsigned tag, size_t e, float p, float4 v) {
  v.x *= drop_scale(seed, tag, e, p);
  v.y *= drop_scale(seed, tag, e + 1, p);
  v.z *= drop_scale(seed, tag, e + 2, p);
  v.w *= drop_scale(seed, tag, e + 3, p);
  return v;
}
// MC: the factors of four elements from their keep bits (bit k: element k kept) -- drop_scale's values, 0 or 1 / (1 - p)
__device__ __forceinline__ float4 mc_keep4(uint32_t bits, float p, float4 v) {
  const float sc = 1.0f / (1.0f - p);
  v.x *= (bits & 1u) ? sc : 0.f;
  v.y *= (bits & 2u) ? sc : 0.f;
  v.z *= (bits & 4u) ? sc : 0.f;
  v.w *= (bits & 8u) ? sc : 0.f;
  return v;
}
// SET: a model set's launch (scann_forward_models) -- K members of one architecture in one grid of K x the tiles of one; the workgroup's
// member shifts every per-member pointer once, in scalar registers (set_member), and the body is the plain inference kernel's
template <class T>
__device__ __forceinline__ T* set_member(T* p, int64_t bytes) {
  return reinterpret_cast<T*>(reinterpret_cast<typename std::conditional<std::is_const<T>::value, const char, char>::type*>(p) + bytes);
}
template <bool FFN, int MODE, int RT, bool EX = false, bool KEEP = false, bool ZOUT = false, bool MC = false, bool SET = false>
__global__ __launch_bounds__(256, RT == 2 ? (EX ? 2 : 3) : (MODE == 1 ? 3 : 4)) void atom_kernel(AtomArgs a) {
#pragma clang fp contract(off)  // fusions are written out: both row-tile copies of a formula round alike (see edge_kernel)
  static_assert(!(EX && KEEP), "the training forward runs the split-fp16 kernels");
  static_assert(!ZOUT || (MODE == 2 && !KEEP), "after_Lc is an output of the readout launch of inference forwards");
  static_assert(!MC || (!EX && !KEEP && !ZOUT), "Monte Carlo dropout runs on the plain split-fp16 inference kernels");
  static_assert(!SET || (!EX && !KEEP && !ZOUT && !MC), "a model set runs the plain split-fp16 inference kernels");
  constexpr int TAR = 32 * RT;  // atom rows per tile
  unsigned set_bix = blockIdx.x;
  if constexpr (SET) {
    const unsigned nt = ((unsigned)a.n_atom + TAR - 1) / TAR, m = blockIdx.x / nt;
    set_bix = blockIdx.x - m * nt;
    const int64_t w = (int64_t)m * a.m_w, o = (int64_t)m * a.m_o;
    a.x = set_member(a.x, (int64_t)m * a.m_x);
    a.Wf1h = set_member(a.Wf1h, w); a.Wf2h = set_member(a.Wf2h, w);
    a.bf1 = set_member(a.bf1, w); a.bf2 = set_member(a.bf2, w); a.lnr_g = set_member(a.lnr_g, w); a.lnr_b = set_member(a.lnr_b, w);
    a.WAh = set_member(a.WAh, w); a.WBh = set_member(a.WBh, w); a.WCh = set_member(a.WCh, w); a.WDh = set_member(a.WDh, w);
    a.bA = set_member(a.bA, w); a.bC = set_member(a.bC, w); a.bD = set_member(a.bD, w);
    a.c = set_member(a.c, o); a.oA = set_member(a.oA, o); a.oB = set_member(a.oB, o); a.oC = set_member(a.oC, o);
  }
  __shared__ __attribute__((aligned(16))) unsigned char sTile[2 * TAR * PLANE_STRIDE * 2];  // hi / lo planes of the current GEMM input
  __shared__ __attribute__((aligned(16))) float sRed[TAR * 8];  // LayerNorm partial statistics [wave][row][mean, m2]
#ifdef SCANN_DIAG_SE_ROWMAJOR  // A/B build: round 5's [row][wave][2]
#define SR_STAT(w, r) (((r) * 4 + (w)) * 2)
#else
#define SR_STAT(w, r) (((w) * TAR + (r)) * 2)
#endif
  __shared__ __attribute__((aligned(16))) float sPar[7 * D];   // bf1 | bf2 | lnr_g | lnr_b | bA | bC | bD
#define SCANN_ATOM_BIX set_bix
#include "scann_atom_body.inc"
#undef SR_STAT
#undef SCANN_ATOM_BIX
}

// Wide tiles (96 rows: RT = 3) of the plain split-fp16 inference launches with a ResidualNorm -- MODE 0 of layers 1 .. L-1 and MODE 2 of
// the readout's launch.  The body is atom_kernel's, text for text: every weight half a wave loads multiplies three row groups instead
// of one or two, so a tile streams its five 64 KB images once for 96 rows; a row's values come out of the same instruction sequence at
// every height (scann_atom_body.inc; tests/test_gpu_atom_rows.py).  Two workgroups per CU: 208-210 VGPRs, 58,880 B of LDS, no scratch (a
// bound of 3 sends the allocator to occupancy 1 with AGPR spills).  A kernel of its own name: tests/test_host.py holds atom_kernel's
// instantiations to the three- and four-workgroup register budgets, tests/test_host_atom_wide.py this one's.  Everything else -- exact,
// training / debug, Monte Carlo, model sets, after_Lc outputs, the base branch's MODE 1 and the first layer's FFN = false launch --
// stays on atom_kernel (launch_atom).
// (RT = 4, 128 rows, compiles to 254 VGPRs / 77,312 B without scratch and was measured with this one: it won at no launch size --
//  atom_tile_rows -- and is not instantiated.)
template <bool FFN, int MODE, int RT>
__global__ __launch_bounds__(256, 2) void atom_wide_kernel(AtomArgs a) {
#pragma clang fp contract(off)  // (as in atom_kernel)
  static_assert(FFN && (MODE == 0 || MODE == 2) && RT == 3, "the wide tiles exist for the ResidualNorm launches of plain inference forwards");
  constexpr bool EX = false, KEEP = false, ZOUT = false, MC = false;
  constexpr int TAR = 32 * RT;
  __shared__ __attribute__((aligned(16))) unsigned char sTile[2 * TAR * PLANE_STRIDE * 2];
  __shared__ __attribute__((aligned(16))) float sRed[TAR * 8];
#define SR_STAT(w, r) (((w) * TAR + (r)) * 2)
  __shared__ __attribute__((aligned(16))) float sPar[7 * D];
#define SCANN_ATOM_BIX blockIdx.x
#include "scann_atom_body.inc"
#undef SR_STAT
#undef SCANN_ATOM_BIX
}

// Rows per tile of the launch `a` on n_cu compute units.  `wide`: a ResidualNorm launch of a plain inference forward, the one kind that
// has atom_wide_kernel (96 rows) and whose heights were measured.  `force` (env SCANN_ATOM_ROWS, read by scann_create): 32 / 64 / 96
// where the launch has that instantiation, anything else is the automatic choice.
static int atom_tile_rows(const AtomArgs& a, int n_cu, bool wide, int force) {
  if (force == 32 || force == 64 || (wide && force == 96)) return force;
  // 32-row tiles (<= 128 VGPRs, 22 KB of LDS: four workgroups per CU = 1,024 slots) while they all fit ONE round of workgroups: the
  // launch is then the latency chain of a tile, and a 32-row tile's chain is shorter (one batch per launch: 490 k -> 568 k
  // molecules/s, training step 1.14 -> 1.09 ms).  Beyond that 64-row tiles (half the weight traffic per row).
  // (re-measured in round 5 at the driver's 10-batch shape, 23 k atoms: 64-row tiles -- half the weight traffic, 360 tiles -- 0.159-0.170 ms
  //  of atom launches per forward against 0.152-0.157 ms for the 720 32-row tiles: the threshold stays)
  const int rows = a.n_atom <= 32 * 1024 ? 32 : 64;
  if (!wide || n_cu <= 0) return rows;
  // The plain inference launches, measured at every height (ms of atom launches per forward, bench.py --no-extras --group G, QM9 L = 7:
  // seven launches; one 256-CU device; G >= 8: mean of four passes that lie within 3 % of each other; profiles/atom_rows_notes.md):
  //   G   atoms     32 rows   64 rows   96 rows   128 rows
  //   1    2.3 k    0.0711    0.0953    0.1175    0.1441      a lone tile's chain: 10.2 / 13.6 / 16.8 / 20.6 us per launch
  //   2    4.6 k    0.0808    0.1016    0.1256    0.1490
  //   8   18.4 k    0.1377    0.1444    0.1358    0.1569
  //  10   23.0 k    0.1433    0.1509    0.1486    0.1667      720 / 360 / 240 / 180 tiles
  //  12   27.6 k    0.1800    0.1576    0.1903    0.1751      864 / 432 / 288 / 216 tiles
  //  14   32.2 k    0.1869    0.1654    0.1927    0.1824
  //  16   36.8 k    0.2170    0.2086    0.1998    0.2453      1,150 / 575 / 384 / 288 tiles
  // A launch is not the weight stream of its busiest CU: a third of the L1 -> L2 read requests (96 rows at G = 10) buys nothing, because
  // with one workgroup on a CU each SIMD holds ONE wave and every epilogue, barrier and weight wait of its chain lies open -- a lone
  // 96-row tile lives 16.8 us against 10.2.  What pays is two or three waves per SIMD from tiles as high as that allows:
  //   32 rows up to three tiles per CU (G <= 10); 64 rows up to two per CU (G = 12, 14: -12 %); 96 rows up to two per CU (G = 16: -4 %);
  //   beyond that (unmeasured) 64 rows as before.  128 rows wins nowhere.
  if ((a.n_atom + 31) / 32 <= 3 * n_cu) return 32;
  if ((a.n_atom + 63) / 64 <= 2 * n_cu) return 64;
  if ((a.n_atom + 95) / 96 <= 2 * n_cu) return 96;
  return 64;
}

void launch_atom(const AtomArgs& a, hipStream_t s, int n_cu, int force_rows) {
  if (a.n_atom <= 0) return;
  const bool keep = !a.exact && (a.drop_p > 0.f || a.keep_pre1 || a.keep_T2 || a.keep_preA);  // training forward
  const bool wide = a.ffn && (a.mode == 0 || a.mode == 2) && !a.exact && !keep && a.n_member <= 0 && !(a.mc_rows && a.drop_p > 0.f) &&
                    !(a.mode == 2 && a.out_z);  // atom_wide_kernel's launches
  const int rows = atom_tile_rows(a, n_cu, wide, force_rows);
  if (rows == 96) {
    const dim3 grid((a.n_atom + rows - 1) / rows), block(256);
    if (a.mode == 0) hipLaunchKernelGGL((atom_wide_kernel<true, 0, 3>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((atom_wide_kernel<true, 2, 3>), grid, block, 0, s, a);
    return;
  }
  if (a.n_member > 0) {  // model set: the plain inference kernels (scann_forward_models), 32- or 64-row tiles by one member's rows
    const dim3 grid(((a.n_atom + rows - 1) / rows) * a.n_member), block(256);
#define SCANN_ATOM_SET(F, M)                                                                                          \
  do {                                                                                                                \
    if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, M, 1, false, false, false, false, true>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((atom_kernel<F, M, 2, false, false, false, false, true>), grid, block, 0, s, a);           \
  } while (0)
    if (a.ffn) {
      if (a.mode == 0) SCANN_ATOM_SET(true, 0);
      else if (a.mode == 1) SCANN_ATOM_SET(true, 1);
      else SCANN_ATOM_SET(true, 2);
    } else {
      if (a.mode == 0) SCANN_ATOM_SET(false, 0);
      else if (a.mode == 1) SCANN_ATOM_SET(false, 1);
      else SCANN_ATOM_SET(false, 2);
    }
#undef SCANN_ATOM_SET
    return;
  }
  const dim3 grid((a.n_atom + rows - 1) / rows), block(256);
  if (a.mc_rows && a.drop_p > 0.f) {  // Monte Carlo dropout (scann_predict_mc: never exact, no keep_* tensors, no outputs)
#define SCANN_ATOM_MC(F, M)                                                                                   \
  do {                                                                                                        \
    if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, M, 1, false, false, false, true>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((atom_kernel<F, M, 2, false, false, false, true>), grid, block, 0, s, a);           \
  } while (0)
    if (a.ffn) {
      if (a.mode == 0) SCANN_ATOM_MC(true, 0);
      else if (a.mode == 1) SCANN_ATOM_MC(true, 1);
      else SCANN_ATOM_MC(true, 2);
    } else {
      if (a.mode == 0) SCANN_ATOM_MC(false, 0);
      else if (a.mode == 1) SCANN_ATOM_MC(false, 1);
      else SCANN_ATOM_MC(false, 2);
    }
#undef SCANN_ATOM_MC
    return;
  }
  if (a.mode == 2 && a.out_z) {  // inference forward that returns after_Lc (never a training forward: run_forward)
#define SCANN_ATOM_Z(F)                                                                                        \
  do {                                                                                                         \
    if (a.exact) {                                                                                             \
      if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, 2, 1, true, false, true>), grid, block, 0, s, a);     \
      else hipLaunchKernelGGL((atom_kernel<F, 2, 2, true, false, true>), grid, block, 0, s, a);                \
    } else if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, 2, 1, false, false, true>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((atom_kernel<F, 2, 2, false, false, true>), grid, block, 0, s, a);                 \
  } while (0)
    if (a.ffn) SCANN_ATOM_Z(true);
    else SCANN_ATOM_Z(false);
#undef SCANN_ATOM_Z
    return;
  }
#define SCANN_ATOM_CASE(F, M)                                                                               \
  do {                                                                                                      \
    if (a.exact) {                                                                                          \
      if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, M, 1, true>), grid, block, 0, s, a);               \
      else hipLaunchKernelGGL((atom_kernel<F, M, 2, true>), grid, block, 0, s, a);                          \
    } else if (keep) {                                                                                      \
      if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, M, 1, false, true>), grid, block, 0, s, a);        \
      else hipLaunchKernelGGL((atom_kernel<F, M, 2, false, true>), grid, block, 0, s, a);                   \
    } else if (rows == 32) hipLaunchKernelGGL((atom_kernel<F, M, 1>), grid, block, 0, s, a);                \
    else hipLaunchKernelGGL((atom_kernel<F, M, 2>), grid, block, 0, s, a);                                  \
  } while (0)
  if (a.ffn) {
    if (a.mode == 0) SCANN_ATOM_CASE(true, 0);
    else if (a.mode == 1) SCANN_ATOM_CASE(true, 1);
    else SCANN_ATOM_CASE(true, 2);
  } else {
    if (a.mode == 0) SCANN_ATOM_CASE(false, 0);
    else if (a.mode == 1) SCANN_ATOM_CASE(false, 1);
    else SCANN_ATOM_CASE(false, 2);
  }
#undef SCANN_ATOM_CASE
}

// ---- edge-tile kernel ------------------------------------------------------------------------------
//
// One workgroup (4 waves) per tile of <= 64 edges of <= TQ whole atoms; three workgroups per CU (<= 53.3 KB of LDS,
// <= 168 VGPRs).  LocalAttention.call for those edges (attention.py:136-216), fused:
//
//   GEMM 1   U = G . W2 (g_update; base branch: gd . Wf, K = 20 padded to 32)                    split-fp16 MFMA
//   epilogue IN THE ACCUMULATOR LAYOUT (lane = edge row, 16 columns): V = U + P1[i] + P3[j], T = swish(V) + G,
//            LayerNorm_g statistics (lane pair -> LDS -> the row's four waves), geom' -> HBM, ang = c[j] * geom' -> LDS
//   GEMM 2   K = ang . Wk + bk                                                                    split-fp16 MFMA
//   epilogue logits q[i].K per (edge, head) straight from the accumulators, K -> LDS
//   softmax over each atom's edges (online), context + unscaled-query residual, LayerNorm -> HBM
//
// Split-fp16 projections: every fp32 operand x is carried as two fp16 numbers, hi = fp16(x) and lo = fp16(x - hi)
// (22 significant bits; fp16 subnormals are honoured by the matrix pipe, tools/mfma_f16_probe.hip), and a product of two
// such operands is three v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator: lo.hi + hi.lo + hi.hi (the lo.lo term is below
// fp32 resolution).  Measured against fp64 the result is as close as the exact-fp32 MFMA chain (1.5e-7 of sum |a b| for
// K = 128; profiles/r02_notes.md) at 3/16 of its matrix-pipe time: f16 MFMA runs at 16x the f32 rate.  Weights are split
// once at load time (pack_weight_f16: pre-scaled by 2^8 so that their lo parts stay normal numbers; the exact inverse is
// applied to the accumulators), activations when a tile is written to LDS -- the tile buffer holds a hi plane and a lo plane
// of 64 x 128 fp16 instead of 64 x 128 fp32: same bytes, same b128 fragment reads.
// Range, top: |activation| and |weight * 256| must stay below 65504 (a 128x128 kernel beyond that sends the handle to the EX
// kernels at load time, an activation beyond it trips flag_range and the forward is re-run on them).
// Range, bottom: hi + lo has 22 significant bits only while lo is a normal fp16 number; below that the pair has an absolute quantum
// (error <= 2^-25), so a row of operands whose LARGEST element is m is carried to about 2^-25 / m of that element.  Nothing in
// these kernels scales a row (the fused backward does: row_scale, scann_train_fused.hip).  Instead scann_load_weights classifies
// the checkpoint (scann_runtime.cpp: small_operand_reason, which lists every operand): LayerNorm outputs, whose size gamma and beta
// fix; the first layer's centres (the embedding table through dense_embed) and geometry (the K = 20 filters over their scalar input);
// ang = c[j] * geom', the PRODUCT of two such rows; the swish of one Dense layer of a LayerNorm output; and the kernels' own columns --
// where one of them stays below 2^-8 (a column of a kernel times 2^8: the same) the handle runs on the EX kernels from the start,
// like one with |w| >= 255.9.  Not covered: rows that are small for reasons of the DATA alone under ordinary weights, cgcnn feature
// rows beyond an upper bound, and weights that training makes small after the load.

//
// FB (g_update, 64-row tiles, first layer of an inference forward): the geometry rows come out of basis_kernel's arithmetic, done
// here on the tile's rows (Gaussian expansions -> planes -> two K = 20 products -> bias, swish, product), not out of memory.
// EX: exact-fp32 projections for the 128x128 kernels (scann_mma.h; the K = 20 filters keep the split form: their inputs are Gaussians
// in [0, 1]) -- the fallback run_forward takes when the split-fp16 range guard fired.  Never with FB.
// KEEP: the training forward's instantiation -- the keep_* stores and the attention dropout exist only there (as uniform branches in
// the inference kernels they cut every epilogue into basic blocks of one LDS read -> wait -> arithmetic -> store each).
// DEAD: the last layer of an inference forward -- nobody reads geom' (scann_model.py:415-421 threads it to the NEXT layer only).
// ATTN: an inference forward that returns this layer's attention weights (scann_set_outputs) -- the softmax stores them per (edge,
// head).  A template flag like KEEP: with it off every instantiation is the code it was.
// MC: Monte Carlo dropout on the attention weights of an inference forward (scann_predict_mc): Dropout(0.05) applied unconditionally with
// structure-local masks; the piece-major family (FB, plain, DEAD) and the base branch's row-major kernel, no keep_* stores
// SET: a model set's launch (scann_forward_models): the linear workgroup index -- XCD-remapped over the whole K x n_tile grid -- is
// member * n_tile + tile; the member's pointers are shifted once per workgroup (set_member), the body is the plain inference kernel's
template <bool GUPD, int RT, bool FB = false, bool EX = false, bool KEEP = false, bool DEAD = false, bool ATTN = false, bool MC = false,
          bool SET = false>
__global__ __launch_bounds__(256, RT == 2 ? 3 : 4) void edge_kernel(EdgeArgs a) {
#pragma clang fp contract(off)  // fusions are written out (fmaf): both unrolled row-tile copies of a formula must round alike,
                                // so that a row's result does not depend on where in a tile it lands (batch-composition invariance)
  static_assert(!FB || GUPD, "the fused basis exists for the g_update kernel only");
  static_assert(!(FB && EX), "the exact fallback runs the plain first layer");
  static_assert(!KEEP || (!FB && !EX && !DEAD), "the training forward runs the plain split-fp16 kernel and keeps every layer's geometry");
  static_assert(!DEAD || GUPD, "the base branch stores no geometry");
  static_assert(!(ATTN && KEEP), "the training forward returns no attention weights");
  static_assert(!MC || (!EX && !KEEP && !ATTN), "Monte Carlo dropout runs on the split-fp16 inference kernels and returns no attention weights");
  static_assert(!SET || (!EX && !KEEP && !ATTN && !MC), "a model set runs the split-fp16 inference kernels and returns no attention weights");
  constexpr int TEK = 32 * RT;  // edge rows per tile: 64 (three workgroups per CU) or, for launches of one round, 32 (four)
  // piece-major geometry tiles (scann_edge_body.inc): the inference kernels, whose geometry nobody else reads.  The training / debug
  // forward (KEEP) and the exact re-run (EX: its first layer reads basis_kernel's row-major geom0) keep [n_edge,128] rows.
  constexpr bool BLK = GUPD && !EX && !KEEP;
  // hi / lo planes of the A operand (G or the basis, then ang): 2 x 64 x 272 B; afterwards K as fp32 [64][LDS_STRIDE]
  __shared__ __attribute__((aligned(16))) unsigned char sTile[2 * TEK * PLANE_STRIDE * 2];
  __shared__ __attribute__((aligned(16))) float sQ[TQ * LDS_STRIDE];  // P1 rows, then query rows of the tile's atoms, then context
  // LayerNorm_g partial statistics [wave][row] (mean, m2), then logits [head][row] with one float of padding per head: lanes that one LDS
  // cycle serves hold consecutive rows, so the row is the fastest index of both (scann_edge_body.inc)
  __shared__ __attribute__((aligned(16))) float sE[NHEAD * (TEK + 1)];
#ifdef SCANN_DIAG_SE_ROWMAJOR  // A/B build: round 5's [row][wave][2] / [row][head] layouts
#define SE_STAT(w, r) (((r) * 4 + (w)) * 2)
#define SE_LOGIT(r, h) ((r) * NHEAD + (h))
#else
#define SE_STAT(w, r) (((w) * TEK + (r)) * 2)
#define SE_LOGIT(r, h) ((h) * (TEK + 1) + (r))
#endif
  __shared__ __attribute__((aligned(16))) float sPar[5 * D];          // layer_norm_g gamma/beta (base: filter bias), layer_norm gamma/beta, key bias
  __shared__ int sOff[TQ + 1];
  // BLK: the tile's slots of the per-tile tables (EdgeArgs::tile_atom, tile_cen with FB, tile_edge0 with ATTN / MC), see the body
  __shared__ int sRow[TQ], sCen[TQ], sE0[TQ];
#ifdef SCANN_DIAG_OCC2  // diagnostic: two workgroups per CU instead of three (how much of the time is latency hidden by occupancy?)
  __shared__ float sDummy[7 * 1024];
  if (a.n_tile < 0) sDummy[threadIdx.x] = 1.f;
#endif
  static_assert(2 * TEK * PLANE_STRIDE * 2 >= TEK * LDS_STRIDE * (int)sizeof(float), "K tile must fit the plane buffer");
  int set_tix = 0;
  if constexpr (SET) {
    const int t = a.xcd_remap ? xcd_tile(blockIdx.x, gridDim.x) : blockIdx.x, m = t / a.n_tile;
    set_tix = t - m * a.n_tile;
    const int64_t w = (int64_t)m * a.m_w, r = (int64_t)m * a.m_r, x = (int64_t)m * a.m_a;
    a.p.W2h = set_member(a.p.W2h, w); a.p.Wkh = set_member(a.p.Wkh, w); a.p.Wfh = set_member(a.p.Wfh, w);
    a.p.bfg = set_member(a.p.bfg, w); a.p.bk = set_member(a.p.bk, w);
    a.p.lng_g = set_member(a.p.lng_g, w); a.p.lng_b = set_member(a.p.lng_b, w); a.p.ln_g = set_member(a.p.ln_g, w); a.p.ln_b = set_member(a.p.ln_b, w);
    a.basis.Wdh = set_member(a.basis.Wdh, w); a.basis.Wwh = set_member(a.basis.Wwh, w); a.basis.bd = set_member(a.basis.bd, w);
    a.basis.bw = set_member(a.basis.bw, w); a.basis.cd = set_member(a.basis.cd, w); a.basis.cw = set_member(a.basis.cw, w);
    a.c = set_member(a.c, r); a.P1 = set_member(a.P1, r); a.P3 = set_member(a.P3, r); a.q = set_member(a.q, r);
    a.geom = set_member(a.geom, x); a.ctx = set_member(a.ctx, x); a.part_buf = set_member(a.part_buf, x);
  }
#define SCANN_EDGE_TIX (SET ? set_tix : a.xcd_remap ? xcd_tile(blockIdx.x, gridDim.x) : blockIdx.x)
#include "scann_edge_body.inc"
#undef SCANN_EDGE_TIX
#undef SE_STAT
#undef SE_LOGIT
#ifdef SCANN_DIAG_TAILWAIT  // diagnostic: what the layer launch's producer side costs an edge tile (its stores acknowledged before it ends)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
#endif
}

// Atoms with more than 64 neighbours: combine the per-chunk softmax states (running max m, sum s, unnormalised context x per
// column) exactly as the online softmax combines edges -- M = max m_i, s = sum s_i e^(m_i - M), x = sum x_i e^(m_i - M) -- then
// add the unscaled query and apply the LayerNorm (attention.py:189-214).  One workgroup of 128 threads per such atom.
// SET: a model set's launch -- n_member x n_big workgroups, member m = b / n_big (the big-atom table is the batch's, shared); member m's
// part_buf, q, ctx lie m * m_a bytes, its ln_g / ln_b m * m_w bytes behind member 0's.  The trailing arguments are unused otherwise
template <bool SET = false>
__global__ __launch_bounds__(128) void edge_merge_kernel(const int32_t* __restrict__ big_tab, const float* __restrict__ part_buf,
                                                         const float* __restrict__ q, const float* __restrict__ ln_g,
                                                         const float* __restrict__ ln_b, float* __restrict__ ctx,
                                                         int32_t* __restrict__ range_flag, int layer, int n_big, int64_t m_a, int64_t m_w) {
  __shared__ float sRed[2][2];
  unsigned bix = blockIdx.x;
  if constexpr (SET) {
    const unsigned m = blockIdx.x / (unsigned)n_big;
    bix = blockIdx.x - m * (unsigned)n_big;
    part_buf = set_member(part_buf, (int64_t)m * m_a); q = set_member(q, (int64_t)m * m_a); ctx = set_member(ctx, (int64_t)m * m_a);
    ln_g = set_member(ln_g, (int64_t)m * m_w); ln_b = set_member(ln_b, (int64_t)m * m_w);
  }
  const int c = threadIdx.x, atom = big_tab[3 * bix], s0 = big_tab[3 * bix + 1], ns = big_tab[3 * bix + 2];
  const float* pb = part_buf + (size_t)s0 * 3 * D + c;
  float M = -INFINITY;
  for (int i = 0; i < ns; ++i) M = fmaxf(M, pb[(size_t)i * 3 * D]);
  float S = 0.f, X = 0.f;
  for (int i = 0; i < ns; ++i) {
    const float wgt = fast_exp(pb[(size_t)i * 3 * D] - M);
    S += pb[(size_t)i * 3 * D + D] * wgt;
    X += pb[(size_t)i * 3 * D + 2 * D] * wgt;
  }
  const float t = X * __builtin_amdgcn_rcpf(S) + q[(size_t)atom * D + c];
  float s = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  if ((c & 63) == 0) sRed[0][c >> 6] = s;
  __syncthreads();
  const float mean = (sRed[0][0] + sRed[0][1]) * (1.0f / D);
  const float d = t - mean;
  float v = d * d;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  if ((c & 63) == 0) sRed[1][c >> 6] = v;
  __syncthreads();
  if (!(sRed[1][0] + sRed[1][1] < RANGE_FINITE) && c == 0) flag_range(range_flag, 2, layer);
  const float rstd = ln_rstd((sRed[1][0] + sRed[1][1]) * (1.0f / D));
  ctx[(size_t)atom * D + c] = ln_apply(t, rstd, -mean * rstd, ln_g[c], ln_b[c]);
}

void launch_edge_merge(const int32_t* big_tab, int n_big, const float* part_buf, const float* q, const float* ln_g,
                       const float* ln_b, float* ctx, int32_t* range_flag, int layer, hipStream_t s) {
  if (n_big > 0)
    hipLaunchKernelGGL(edge_merge_kernel<false>, dim3(n_big), dim3(128), 0, s, big_tab, part_buf, q, ln_g, ln_b, ctx, range_flag, layer, n_big,
                       (int64_t)0, (int64_t)0);
}
void launch_edge_merge_set(const int32_t* big_tab, int n_big, const float* part_buf, const float* q, const float* ln_g, const float* ln_b,
                           float* ctx, int32_t* range_flag, int layer, int n_member, int64_t m_a, int64_t m_w, hipStream_t s) {
  if (n_big > 0 && n_member > 0)
    hipLaunchKernelGGL(edge_merge_kernel<true>, dim3(n_big * n_member), dim3(128), 0, s, big_tab, part_buf, q, ln_g, ln_b, ctx, range_flag, layer,
                       n_big, m_a, m_w);
}

// Attention weights of the atoms with more than 64 neighbours (inference outputs): chunk i's tile stored exp(e - m_i) per (edge, head);
// the weight is that times exp(m_i - M) / S, with M = max m_i and S = sum s_i exp(m_i - M) formed in edge_merge_kernel's order
// (column 16 h of part_buf holds head h's m_i, s_i).  One workgroup per such atom, one thread per (edge, head).
__global__ __launch_bounds__(256) void attn_merge_kernel(const int32_t* __restrict__ big_tab, const float* __restrict__ part_buf,
                                                         const int32_t* __restrict__ edge_offset, int chunk, float* __restrict__ attn) {
  const int atom = big_tab[3 * blockIdx.x], s0 = big_tab[3 * blockIdx.x + 1], ns = big_tab[3 * blockIdx.x + 2];
  const int e0 = edge_offset[atom], deg = edge_offset[atom + 1] - e0;
  for (int i = threadIdx.x; i < deg * NHEAD; i += blockDim.x) {
    const int n = i / NHEAD, h = i - n * NHEAD;
    const float* pb = part_buf + (size_t)s0 * 3 * D + HDIM * h;
    float M = -INFINITY;
    for (int k = 0; k < ns; ++k) M = fmaxf(M, pb[(size_t)k * 3 * D]);
    float S = 0.f;
    for (int k = 0; k < ns; ++k) S += pb[(size_t)k * 3 * D + D] * fast_exp(pb[(size_t)k * 3 * D] - M);
    const float mi = pb[(size_t)(n / chunk) * 3 * D];
    float* const w = attn + (size_t)(e0 + n) * NHEAD + h;
    *w = *w * fast_exp(mi - M) * __builtin_amdgcn_rcpf(S);
  }
}

void launch_attn_merge(const int32_t* big_tab, int n_big, const float* part_buf, const int32_t* edge_offset, int chunk, float* attn, hipStream_t s) {
  if (n_big > 0 && attn) hipLaunchKernelGGL(attn_merge_kernel, dim3(n_big), dim3(256), 0, s, big_tab, part_buf, edge_offset, chunk, attn);
}

// centre atom of every edge: one thread per atom writes its CSR row's entries (a batch has ~8 edges per atom)
// (zero_word: a device word this launch clears on its way -- the flag of the pack_padded_kernel launch behind it)
__global__ void edge_row_kernel(const int32_t* __restrict__ edge_offset, int n_atom, int32_t* __restrict__ edge_row, int32_t* __restrict__ zero_word) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a == 0 && zero_word) *zero_word = 0;
  if (a >= n_atom) return;
  for (int e = edge_offset[a]; e < edge_offset[a + 1]; ++e) edge_row[e] = a;
}
void launch_edge_row(const int32_t* edge_offset, int n_atom, int32_t* edge_row, hipStream_t s, int32_t* zero_word) {
  if (n_atom > 0 || zero_word)
    hipLaunchKernelGGL(edge_row_kernel, dim3(std::max(1, (n_atom + 255) / 256)), dim3(256), 0, s, edge_offset, n_atom, edge_row, zero_word);
}

// Padded -> CSR (what gather_shape + the masks express: custom_layers.py:18-28, datagenerator.py:69-135): one thread per padded atom
// slot.  A real atom walks its N neighbour slots in slot order and writes the unmasked ones behind edge_offset[row] -- the neighbour's
// intra-structure index becomes its packed row through row_of -- HBM-bound streaming work (13 bytes read, 12 written per kept slot;
// 160 B per atom slot read in all), a few tens of microseconds per 2,048-structure chunk.
__global__ __launch_bounds__(256) void pack_padded_kernel(PackPaddedArgs a) {
  const int bm = blockIdx.x * blockDim.x + threadIdx.x;
  if (bm >= a.B * a.M) return;
  const int row = a.row_of[bm];
  if (row < 0) return;
  const int z = a.atomic[bm];
  int bad = (z < 0 || z >= a.n_species) ? 2 : 0;
  a.out_atomic[row] = bad ? 0 : z;  // (a valid table row either way: the forward must not fault on an input that is about to be refused)
  const int b0 = (bm / a.M) * a.M;  // first atom slot of this structure
  int e = a.edge_offset[row];
  const size_t base = (size_t)bm * a.N;
  for (int n = 0; n < a.N; ++n) {
    const bool on = a.mask_size == 1 ? static_cast<const uint8_t*>(a.neighbor_mask)[base + n] != 0
                                     : (static_cast<const uint32_t*>(a.neighbor_mask)[base + n] & 0x7fffffffu) != 0;
    if (!on) continue;
    const int tgt = a.neighbors[base + n];
    const int r = (tgt >= 0 && tgt < a.M) ? a.row_of[b0 + tgt] : -1;
    if (r < 0) bad |= 1;
    a.out_col[e] = r < 0 ? row : r;
    a.out_dist[e] = a.dist[base + n];
    a.out_weight[e] = a.weight[base + n];
    ++e;
  }
  if (bad) atomicOr(a.flag, bad);
}
void launch_pack_padded(const PackPaddedArgs& a, hipStream_t s) {
  const int n = a.B * a.M;
  if (n > 0) hipLaunchKernelGGL(pack_padded_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

// The tile-order side of a batch (TileOrderArgs): thread i < n_tile TQ fills slot i of the per-tile tables, thread i < n_atom (a filled
// plan only) copies the edges of the i-th atom in tile order behind its tile-order offset.
__global__ __launch_bounds__(256) void tile_order_kernel(TileOrderArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n_tile * TQ) {
    const int t = i / TQ, s = i - t * TQ;
    const EdgeTile tile = a.tiles[t];
    const int k = min(tile.atom_begin + s, tile.atom_end - 1);
    const int r = a.atom_row ? a.atom_row[k] : k;
    a.tile_atom[i] = r;
    a.tile_edge0[i] = a.edge_offset[r];
    if (a.atomic) a.tile_species[i] = a.atomic[r];
  }
  if (a.atom_row && i < a.n_atom) {
    const int r = a.atom_row[i];
    const int src = a.edge_offset[r], dst = a.tile_offset[i], deg = a.tile_offset[i + 1] - dst;
    for (int n = 0; n < deg; ++n) {
      a.out_col[dst + n] = a.col[src + n];
      a.out_dist[dst + n] = a.dist[src + n];
      a.out_weight[dst + n] = a.weight[src + n];
      a.out_row[dst + n] = i;
    }
  }
}
void launch_tile_order(const TileOrderArgs& a, hipStream_t s) {
  const int n = std::max(a.n_tile * TQ, a.atom_row ? a.n_atom : 0);
  if (n > 0) hipLaunchKernelGGL(tile_order_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

void launch_edge(const EdgeArgs& a, hipStream_t s) {
  if (a.n_tile <= 0) return;
  const dim3 grid(a.n_tile * std::max(a.n_member, 1)), block(256);
  // tile_rows is the height the batch's tile plan was made for (scann_batch_upload: 32 for launches of one round of workgroups)
  // three families: EX (exact-fp32 re-run of an inference forward), KEEP (training / debug forwards: row-major geometry, keep_* stores,
  // attention dropout), and the inference kernels proper (piece-major geometry tiles; FB = the first layer, DEAD = the last)
  const bool keep = !a.exact && (a.geom_rows || a.keep_V || a.keep_T || a.keep_ang || a.keep_K || a.attn_drop_p > 0.f);
  const bool dead = a.g_update && a.geom_dead && !keep;
#define SCANN_EDGE_GO(...) hipLaunchKernelGGL((edge_kernel<__VA_ARGS__>), grid, block, 0, s, a)
#define SCANN_EDGE_ROWS(G, ...)                                             \
  do {                                                                      \
    if (a.tile_rows == 32) SCANN_EDGE_GO(G, 1, __VA_ARGS__);                \
    else SCANN_EDGE_GO(G, 2, __VA_ARGS__);                                  \
  } while (0)
  if (a.n_member > 0) {  // model set (scann_forward_models): the inference kernels proper -- g_update piece-major, base branch row-major
    if (!a.g_update) SCANN_EDGE_ROWS(false, false, false, false, false, false, false, true);
    else if (a.fuse_basis) SCANN_EDGE_ROWS(true, true, false, false, false, false, false, true);
    else if (a.geom_dead) SCANN_EDGE_ROWS(true, false, false, false, true, false, false, true);
    else SCANN_EDGE_ROWS(true, false, false, false, false, false, false, true);
  } else if (a.mc_rows && a.attn_drop_p > 0.f) {  // Monte Carlo dropout (scann_predict_mc; g_update: the piece-major family, run_forward)
    if (!a.g_update) SCANN_EDGE_ROWS(false, false, false, false, false, false, true);
    else if (a.fuse_basis) SCANN_EDGE_ROWS(true, true, false, false, false, false, true);
    else if (a.geom_dead) SCANN_EDGE_ROWS(true, false, false, false, true, false, true);
    else SCANN_EDGE_ROWS(true, false, false, false, false, false, true);
  } else if (a.exact && a.attn_out) {  // (the exact re-run of a forward that returns attention weights returns the re-run's)
    if (!a.g_update) SCANN_EDGE_ROWS(false, false, true, false, false, true);
    else if (dead) SCANN_EDGE_ROWS(true, false, true, false, true, true);
    else SCANN_EDGE_ROWS(true, false, true, false, false, true);
  } else if (a.exact) {  // never with the fused first layer (run_forward launches basis_kernel for it)
    if (!a.g_update) SCANN_EDGE_ROWS(false, false, true, false, false);
    else if (dead) SCANN_EDGE_ROWS(true, false, true, false, true);
    else SCANN_EDGE_ROWS(true, false, true, false, false);
  } else if (a.attn_out) {  // inference kernels that store the attention weights: the base branch's row-major kernel (its KEEP twin differs
                            // only by the training stores), the piece-major g_update family (run_forward refuses row-major g_update forwards)
    if (!a.g_update) SCANN_EDGE_ROWS(false, false, false, false, false, true);
    else if (a.fuse_basis) SCANN_EDGE_ROWS(true, true, false, false, false, true);
    else if (a.geom_dead) SCANN_EDGE_ROWS(true, false, false, false, true, true);
    else SCANN_EDGE_ROWS(true, false, false, false, false, true);
  } else if (keep) {
    if (a.g_update) SCANN_EDGE_ROWS(true, false, false, true, false);
    else SCANN_EDGE_ROWS(false, false, false, true, false);
  } else if (!a.g_update) {
    SCANN_EDGE_ROWS(false, false, false, false, false);
  } else if (a.fuse_basis) {  // (a one-layer model's only launch stores its geometry: no instantiation for that corner)
    SCANN_EDGE_ROWS(true, true, false, false, false);
  } else {
    if (dead) SCANN_EDGE_ROWS(true, false, false, false, true);
    else SCANN_EDGE_ROWS(true, false, false, false, false);
  }
#undef SCANN_EDGE_ROWS
#undef SCANN_EDGE_GO
}

// ---- basis kernel ----------------------------------------------------------------------------------

// geom0 = swish(G(dist) Wd + bd) * swish(G(weight) Ww + bw) for a tile of 64 edges: the two K = 20 products run on the matrix
// pipe (split-fp16, K padded to 32; the VALU form of round 1 issued 2,600 instructions per wave and was VALU-bound at 92 us
// per 16-batch launch), bias / swish / product in the accumulator layout, rows stored in 16-byte pieces.
__global__ __launch_bounds__(256) void basis_kernel(BasisParams p, const float* __restrict__ dist,
                                                    const float* __restrict__ weight, int n_edge,
                                                    float* __restrict__ geom) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) _Float16 sH[64 * BASIS_STRIDE];  // per row: distance basis [0,32) | angle basis [32,64), hi parts
  __shared__ __attribute__((aligned(16))) _Float16 sL[64 * BASIS_STRIDE];  // lo parts
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane & 31, lh = lane >> 5, cbase = 32 * wave + 4 * lh;
  const int e0 = blockIdx.x * 64;
  const int ne = min(64, n_edge - e0);
  f16x8 bdh[2], bdl[2], bwh[2], bwl[2];
  load_wsplit<2>(p.Wdh, wave, lane, bdh, bdl);
  load_wsplit<2>(p.Wwh, wave, lane, bwh, bwl);
  float4 bd[4], bw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bd[j] = *reinterpret_cast<const float4*>(p.bd + cbase + 8 * j);
    bw[j] = *reinterpret_cast<const float4*>(p.bw + cbase + 8 * j);
  }
  {
    const int r = tid >> 2, sub = tid & 3;  // 4 threads per edge row, 8 basis columns each
    const int rs = min(r, ne - 1);
    const float xd = dist[e0 + rs], xw = weight[e0 + rs];
    f16x8 gh[2], gl[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = 8 * sub + i;
      const float cdk = p.cd[min(k, NG - 1)], cwk = p.cw[min(k, NG - 1)];
      const float vd = (k < NG && r < ne) ? gauss_fast(xd, cdk) : 0.f, vw = (k < NG && r < ne) ? gauss_fast(xw, cwk) : 0.f;
      gh[0][i] = (_Float16)vd; gl[0][i] = (_Float16)(vd - (float)gh[0][i]);
      gh[1][i] = (_Float16)vw; gl[1][i] = (_Float16)(vw - (float)gh[1][i]);
    }
    *reinterpret_cast<f16x8*>(sH + r * BASIS_STRIDE + 8 * sub) = gh[0];
    *reinterpret_cast<f16x8*>(sL + r * BASIS_STRIDE + 8 * sub) = gl[0];
    *reinterpret_cast<f16x8*>(sH + r * BASIS_STRIDE + 32 + 8 * sub) = gh[1];
    *reinterpret_cast<f16x8*>(sL + r * BASIS_STRIDE + 32 + 8 * sub) = gl[1];
  }
  __syncthreads();
  f32x16 accd[2], accw[2];
  mma_split<2, true, BASIS_STRIDE>(sH, sL, bdh, bdl, lane, accd);
  mma_split<2, true, BASIS_STRIDE>(sH + 32, sL + 32, bwh, bwl, lane, accw);
  constexpr float WINV = 1.0f / WSCALE;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int row = lrow + 32 * rt;
    if (row < ne) {
      const unsigned off = ((unsigned)(e0 + row) * D + cbase) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 sd = f4swish(make_float4(fmaf(accd[rt][4 * j], WINV, bd[j].x), fmaf(accd[rt][4 * j + 1], WINV, bd[j].y),
                                              fmaf(accd[rt][4 * j + 2], WINV, bd[j].z), fmaf(accd[rt][4 * j + 3], WINV, bd[j].w)));
        const float4 sw = f4swish(make_float4(fmaf(accw[rt][4 * j], WINV, bw[j].x), fmaf(accw[rt][4 * j + 1], WINV, bw[j].y),
                                              fmaf(accw[rt][4 * j + 2], WINV, bw[j].z), fmaf(accw[rt][4 * j + 3], WINV, bw[j].w)));
        st4(geom, off + 32 * j, f4mul(sd, sw));  // neighbor_d * neighbor_w (scann_model.py:381-389)
      }
    }
  }
}

__global__ void basis_raw_kernel(const float* __restrict__ cd, const float* __restrict__ dist, int n_edge,
                                 float* __restrict__ gd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_edge * NG) gd[i] = gauss(dist[i / NG], cd[i % NG]);
}

void launch_basis(const BasisParams& p, const float* dist, const float* weight, int n_edge, float* geom,
                  hipStream_t s) {
  if (n_edge <= 0) return;
  hipLaunchKernelGGL(basis_kernel, dim3((n_edge + 63) / 64), dim3(256), 0, s, p, dist, weight, n_edge, geom);
}

void launch_basis_raw(const float* cd, const float* dist, int n_edge, float* gd, hipStream_t s) {
  if (n_edge <= 0) return;
  const int n = n_edge * NG;
  hipLaunchKernelGGL(basis_raw_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cd, dist, n_edge, gd);
}

// ---- embedding LUT (weight-load time) ----------------------------------------------------------------

// lut[s,:] = swish(E[s,:] . W + b): Embedding (scann_model.py:362) followed by dense_embed (:373) has only
// n_atoms distinct results, so it is folded into a table when weights are loaded.
__global__ void embed_lut_kernel(const float* __restrict__ emb, const float* __restrict__ W,
                                 const float* __restrict__ b, int emb_dim, float* __restrict__ lut) {
  const int sp = blockIdx.x, col = threadIdx.x;
  float acc = 0.f;
  // the same sum in the same order, its operands requested sixteen at a time (the one-by-one loop was emb_dim dependent round trips:
  // 13 us at the head of every training step)
  for (int k0 = 0; k0 < emb_dim; k0 += 16) {
    float e[16], w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int k = min(k0 + u, emb_dim - 1);
      e[u] = emb[sp * emb_dim + k];
      w[u] = W[k * D + col];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (k0 + u < emb_dim) acc += e[u] * w[u];
  }
  lut[sp * D + col] = swishf(acc + b[col]);
}

void launch_embed_lut(const float* emb, const float* W, const float* b, int n_species, int emb_dim, float* lut,
                      hipStream_t s) {
  hipLaunchKernelGGL(embed_lut_kernel, dim3(n_species), dim3(D), 0, s, emb, W, b, emb_dim, lut);
}

// ---- general embedding kernel (use_ring / feature="cgcnn") -----------------------------------------------

// c0 = swish(dense_embed(concat[embed, extra_embed(ring)]))  (scann_model.py:361-374): `embed` is the Embedding row
// (feature="atomic", :362) or Dense(92 -> emb) of the CGCNN features without activation (:365); ring/aromatic flags go
// through Dense(2 -> 10) (:368) and are concatenated (:371).  8 atoms per 128-thread workgroup.
__global__ __launch_bounds__(128) void embed_kernel(EmbedArgs a) {
  __shared__ float sV[8][160];
  const int tid = threadIdx.x;
  const int a0 = blockIdx.x * 8;
  const int na = min(8, a.n_atom - a0);
  const int cin = a.emb_dim + (a.ring ? 10 : 0);
  for (int i = tid; i < na * cin; i += 128) {
    const int la = i / cin, k = i % cin, at = a0 + la;
    float v;
    if (k < a.emb_dim) {
      if (a.cgcnn) {
        float acc = 0.f;
        for (int j = 0; j < 92; ++j) acc += a.cgcnn[(size_t)at * 92 + j] * a.We[j * a.emb_dim + k];
        v = acc + a.be[k];
      } else {
        v = a.emb[(size_t)a.atomic[at] * a.emb_dim + k];
      }
    } else {
      const int r = k - a.emb_dim;
      v = (a.ring[(size_t)at * 2] * a.Wr[r] + a.ring[(size_t)at * 2 + 1] * a.Wr[10 + r]) + a.br[r];
    }
    sV[la][k] = v;
  }
  __syncthreads();
  for (int la = 0; la < na; ++la) {
    float acc = 0.f;
    for (int k = 0; k < cin; ++k) acc += sV[la][k] * a.Wde[k * D + tid];
    a.c0[(size_t)(a0 + la) * D + tid] = swishf(acc + a.bde[tid]);
  }
}

void launch_embed(const EmbedArgs& a, hipStream_t s) {
  if (a.n_atom <= 0) return;
  hipLaunchKernelGGL(embed_kernel, dim3((a.n_atom + 7) / 8), dim3(128), 0, s, a);
}

// ---- readout kernel ----------------------------------------------------------------------------------

// (wave_sum64 / wave_max64, scann_mma.h: DPP / lane-swap forms of the xor butterflies, the same additions and maxima without six LDS
//  round trips each -- in the readout they sit one behind the other: norm -> maximum -> sum of the exponentials -> head)

// One workgroup per structure.  GlobalAttention.call (attention.py:267-318) on the real atoms only (the
// multiplicative atom mask zeroes every padded term).  The pair energies E[i][j] = k_i . q_j (:279) are 32x32 MFMA
// tiles; wave w contracts features [32w, 32w+32) of every tile, masks the diagonal (:282-285) and rows/columns past
// the structure, keeps per-lane partial row sums over all column tiles, reduces them across the 32 columns once
// per row tile, and the four waves' partial sums are added in fixed order (deterministic).
// SET: a model set's launch (n_member x n_struct workgroups, member m = b / n_struct): the member's pointers are shifted once and its mrelu
// is bit m of relu_out; the body is the plain kernel's with `sid` for the workgroup's structure
template <bool SET = false>
__global__ __launch_bounds__(256) void readout_kernel(ReadoutArgs a) {
  extern __shared__ float sDyn[];  // [4][npad] partial row sums, then [npad] scores / attention
  __shared__ float sRep[D];
  __shared__ float sHead[D];
  __shared__ float sRed[4];
  unsigned sid = blockIdx.x;
  if constexpr (SET) {
    const unsigned m = blockIdx.x / (unsigned)a.n_struct;
    sid = blockIdx.x - m * (unsigned)a.n_struct;
    a.relu_out = (a.relu_out >> m) & 1;
    const int64_t w = (int64_t)m * a.m_w, x = (int64_t)m * a.m_a;
    a.p.Wb = set_member(a.p.Wb, w); a.p.bb = set_member(a.p.bb, w); a.p.wo = set_member(a.p.wo, w); a.p.bo = set_member(a.p.bo, w);
    a.gq = set_member(a.gq, x); a.gk = set_member(a.gk, x);
    a.ga_attn = set_member(a.ga_attn, (int64_t)m * a.m_g); a.y = set_member(a.y, (int64_t)m * a.m_y);
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = a.mol_offset[sid];
  const int n = a.mol_offset[sid + 1] - a0;
  const int T = (n + 31) >> 5, npad = T << 5;
  float* sPart = sDyn;            // [4][npad]
  float* sAgg = sDyn + 4 * npad;  // [npad]
  const float4* gq4 = reinterpret_cast<const float4*>(a.gq) + (size_t)a0 * 32;
  const float4* gk4 = reinterpret_cast<const float4*>(a.gk) + (size_t)a0 * 32;
  const int r = lane & 31, h = lane >> 5;

  for (int it = 0; it < T; ++it) {
    const int irow = it * 32 + r;
    float4 ka[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)  // features 32*wave + 8t + 4h .. +3 of key row irow
      ka[t] = irow < n ? gk4[(size_t)irow * 32 + 8 * wave + 2 * t + h] : make_float4(0.f, 0.f, 0.f, 0.f);
    float part[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
    for (int jt = 0; jt < T; ++jt) {
      const int jrow = jt * 32 + r;
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float4 qb = jrow < n ? gq4[(size_t)jrow * 32 + 8 * wave + 2 * t + h] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[t].x, qb.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[t].y, qb.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[t].z, qb.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[t].w, qb.w, acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int gi = it * 32 + acc_row(i, lane);  // key index (row), this lane's column is query index jrow
        part[i] += (gi != jrow) ? acc[i] : 0.f;     // mask_center (:282-285); padded rows/cols contribute exact zeros
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float v = sum32(part[i]);  // over the 32 query columns of this lane's half
      if (r == 0) sPart[wave * npad + it * 32 + acc_row(i, lane)] = v;
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256)  // agg_i (:289-292)
    sAgg[i] = ((sPart[i] + sPart[npad + i]) + sPart[2 * npad + i]) + sPart[3 * npad + i];
  __syncthreads();
  // normalise + softmax over atoms by wave 0 (:295-302)
  if (wave == 0) {
    float nrm = 1.0f;
    if (a.use_ga_norm) {
      float ss = 0.f;
      for (int i = lane; i < n; i += 64) ss += sAgg[i] * sAgg[i];
      nrm = sqrtf(wave_sum64(ss));  // tf.linalg.normalize: no epsilon (n == 1 -> 0/0 = NaN as in the reference)
    }
    float m = -INFINITY;
    for (int i = lane; i < n; i += 64) {
      const float v = a.use_ga_norm ? sAgg[i] / nrm : sAgg[i];
      sAgg[i] = v;
      m = fmaxf(m, v);
    }
    m = wave_max64(m);
    float ss = 0.f;
    for (int i = lane; i < n; i += 64) {
      const float e = expf(sAgg[i] - m);
      sAgg[i] = e;
      ss += e;
    }
    ss = wave_sum64(ss);
    for (int i = lane; i < n; i += 64) {
      const float at = sAgg[i] / ss;
      sAgg[i] = at;
      a.ga_attn[a0 + i] = at;
    }
  }
  __syncthreads();
  // rep = sum_i attn_i k_i  (:314-316): two half-sums over interleaved atoms per feature, fixed order
  {
    const int f = tid & (D - 1), half = tid >> 7;
    float rsum = 0.f;
    // (four key rows requested per step -- the terms past the last atom are a valid row times an exact zero, added in the order of the
    //  one-row-per-step loop: each step was a memory round trip of its own)
    for (int i = half; i < n; i += 8) {
      float kv[4], av[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int iu = i + 2 * u;
        kv[u] = a.gk[(size_t)(a0 + min(iu, n - 1)) * D + f];
        av[u] = iu < n ? sAgg[iu] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) rsum += av[u] * kv[u];
    }
    if (half == 1) sRep[f] = rsum;
    __syncthreads();
    if (half == 0) sRep[f] = rsum + sRep[f];
  }
  __syncthreads();
  // bf_property + predict_property (scann_model.py:437-447)
  // (both halves of the workgroup walk 64 of the 128 input features each, 16 weight loads in flight: the 128 dependent-in-order
  // loads of a one-thread-per-output loop were the longest wait of this kernel)
  float part = 0.f;
  {
    const int f = tid & (D - 1), half = tid >> 7;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f;  // four interleaved chains, fixed association
    const float* __restrict__ wcol = a.p.Wb + (size_t)(64 * half) * D + f;
    const float* __restrict__ rp = sRep + 64 * half;
    for (int k0 = 0; k0 < 64; k0 += 16) {  // sixteen weights requested per step: four memory round trips instead of sixteen
      float wv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) wv[u] = wcol[(size_t)(k0 + u) * D];
#pragma unroll
      for (int u = 0; u < 16; u += 4) {
        h0 = fmaf(rp[k0 + u], wv[u], h0);
        h1 = fmaf(rp[k0 + u + 1], wv[u + 1], h1);
        h2 = fmaf(rp[k0 + u + 2], wv[u + 2], h2);
        h3 = fmaf(rp[k0 + u + 3], wv[u + 3], h3);
      }
    }
    const float hs = (h0 + h1) + (h2 + h3);
    if (half == 1) sHead[f] = hs;
    __syncthreads();
    if (half == 0) {
      const float hb = swish_exact((hs + sHead[f]) + a.p.bb[f]);
      if (a.bf_out) a.bf_out[(size_t)sid * D + f] = hb;  // inference outputs: bf_property (uniform per workgroup)
      part = hb * a.p.wo[f];
    }
  }
  part = wave_sum64(part);
  if (lane == 0) sRed[wave] = part;
  __syncthreads();
  if (tid == 0) {
    float y = (sRed[0] + sRed[1]) + a.p.bo[0];
    if (a.relu_out) y = fmaxf(y, 0.f);  // mrelu forward (custom_layers.py:15)
    a.y[sid] = y;
  }
}

void launch_readout(const ReadoutArgs& a, hipStream_t s) {
  if (a.n_struct <= 0) return;
  const size_t npad = (size_t)((a.max_atoms + 31) / 32) * 32;
  const size_t lds = 5 * npad * sizeof(float);  // 4 partial-sum rows + the score row
  if (a.n_member > 0) hipLaunchKernelGGL(readout_kernel<true>, dim3(a.n_struct * a.n_member), dim3(256), lds, s, a);
  else hipLaunchKernelGGL(readout_kernel<false>, dim3(a.n_struct), dim3(256), lds, s, a);
}

}  // namespace scann


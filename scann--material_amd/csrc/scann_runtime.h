// Internal header of libscann_hip.so's host runtime (not installed): what its units share -- the handle and resident-batch structs,
// the device-block cache, the error helpers and the forward launch schedule.  The C ABI itself is include/scann_hip.h.
#pragma once
#include "../../include/scann_hip.h"
#include "scann_internal.h"
#include "scann_train.h"
#include "scann_train_plan.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace scann;

namespace scann {

constexpr int MAX_STREAM = 16;

// device-block cache (scann_runtime.cpp)
hipError_t cached_malloc(void** p, size_t bytes);
void cached_free(void* p);
void cache_release(int dev);

struct WeightSpec {
  std::string name;
  int64_t rows, cols;  // cols == 0: vector of length rows
  int64_t numel() const { return cols ? rows * cols : rows; }
};

// What the generic-width TRAINING forward keeps for the backward (gen_backward): every tensor a formula's derivative reads, in buffers of
// their own per layer (the inference forward rotates five atom-row and three edge-row buffers instead).
struct GenLayerKeep {
  float *cc_in = nullptr, *G_in = nullptr;  // centres / geometry entering the layer
  float *Z = nullptr;                       // filter_geo pre-activation
  float *T = nullptr;                       // g_update: swish(Z) + G_in, the input of layer_norm_g
  float *Gn = nullptr;                      // the geometry the key projection is gated with (g_update: the layer's output geometry)
  float *K = nullptr, *q = nullptr;
  float *t1 = nullptr, *ctx = nullptr;      // attention context + query (input of layer_norm), its LayerNorm
  float *pre1 = nullptr, *h1 = nullptr, *t2 = nullptr;  // ResidualNorm: dense_1 pre-activation, its swish, Dropout(dense_2)
  float *cc_out = nullptr;
};
struct GenKeep {
  char* arena = nullptr;   // forward tensors
  size_t bytes = 0;
  char* barena = nullptr;  // backward temporaries + the transposed kernels
  size_t bbytes = 0;
  std::vector<GenLayerKeep> layer;
  float *embE = nullptr, *ring10 = nullptr, *pre_e = nullptr, *cc0 = nullptr;
  float *gd = nullptr, *gw = nullptr, *pre_d = nullptr, *pre_w = nullptr, *Td = nullptr, *Tw = nullptr, *G0 = nullptr;
  float *cc_L = nullptr, *z_pre = nullptr, *z = nullptr, *gq = nullptr, *gk = nullptr, *rep = nullptr, *hid_pre = nullptr, *hid = nullptr;
  float drop_p = 0.f, attn_p = 0.f;
  unsigned long long seed = 0;
  std::map<std::string, std::pair<const float*, size_t>> dbg;  // scann_train_debug_read: tensors of the last backward's readout stage
};

struct scann_train_ws {  // per resident batch (scann_dbatch::train), allocated on first use
  char* arena = nullptr;
  std::vector<float*> tA;  // [n_atom,128] temporaries: 5 shared + 5 per layer and readout (operands of that layer's weight gradients)
  float *keep_q = nullptr, *keep_V = nullptr, *keep_T = nullptr, *keep_ang = nullptr, *keep_K = nullptr;  // [L][rows,128] or null
  float *keep_pre1 = nullptr, *keep_H1 = nullptr, *keep_T2 = nullptr;
  float *keep_preA = nullptr, *keep_z = nullptr;
  std::vector<float*> tE;  // [n_edge,128] temporaries: 4 shared + 2 per layer and readout
  float *rep = nullptr, *dpre = nullptr, *dy = nullptr, *targets = nullptr, *dlut = nullptr;
  float* wpart = nullptr;  // per-slab partial sums of every weight gradient of a step (WgradCtx::arena)
  size_t wpart_floats = 0;
  float* det_part = nullptr;  // deterministic mode: the slots of the otherwise atomic reductions (first deterministic backward)
  size_t det_floats = 0;
  double* sse = nullptr;
  char* ig = nullptr;  // scann_input_grads: the device copies of its outputs (first such call on the batch)
  size_t ig_bytes = 0;
  float drop_p = 0.f, attn_p = 0.f;
  unsigned long long seed = 0;
  GenKeep gen;  // generic widths: the training forward's tensors and the backward's temporaries
  ~scann_train_ws() {  // freed with its batch (free_batch): the arenas go back to the block cache
    cached_free(arena);
    cached_free(det_part);
    cached_free(ig);
    cached_free(gen.arena);
    cached_free(gen.barena);
  }
};

struct Timer;  // scann_forward_profile's launch timer (scann_forward.cpp)
struct ModelSet;  // scann_models_load's members (scann_models.cpp)
void free_models(ModelSet* ms);  // no work of the set may still be running

// scann_predict_mc: the sample a forward is to compute (FwdOpts::mc)
struct McState {
  const McRow* rows;        // [n_atom] of the batch (launch_mc_rows)
  unsigned long long seed;  // the call's seed
  uint32_t t;               // sample index
  float p_drop, p_attn;     // Dropout(0.1) layers / attention-weight rates (0: the site is off)
};

}  // namespace scann

struct scann_handle {
  scann_config_t cfg{};
  int device = 0;
  std::string err;
  hipStream_t streams[MAX_STREAM]{};
  int nstream = 2;  // HIP streams batches are spread over (env SCANN_STREAMS, 1..16).  Two launch groups in flight fill each other's
                    // latency-bound launches; with the upload off the launching thread more only split the caches (1.83 M vs 1.71 M
                    // molecules/s host-inclusive at 4, tools/e2e_size.py)
  std::vector<WeightSpec> specs;
  bool loaded = false;
  bool debug = false;
  // scann_set_outputs: what later inference forwards also write -- bit k: local_attention_k's weights; out_flags: SCANN_OUT_AFTER_LC |
  // SCANN_OUT_BF_PROPERTY.  Zero: the forward launches exactly the plain schedule.  Written there and read by selected_opts only: a
  // forward runs under the selection in its FwdOpts
  uint64_t out_layers = 0;
  int32_t out_flags = 0;
  int tile_atoms = TQ;     // atoms per edge tile the tile builder allows (edge_kernel's query-row buffer)
  int n_cu = 256;      // compute units of the device
  int time_every = 0;  // > 0: sample edge-kernel launch durations on every n-th forward (scann_edge_timing)
  int64_t time_count = 0;
  std::vector<hipEvent_t> time_ev;  // pairs (start, stop)
  std::vector<int> time_edges;
  int xcd_remap = 1;   // env SCANN_XCD_REMAP=0 disables the XCD-contiguous tile order
  int atom_rows = 0;   // env SCANN_ATOM_ROWS=32 / 64 / 96: atom tile height where the launch has that instantiation (0, anything else: launch_atom chooses)
  int fuse_basis = 1;  // env SCANN_FUSE_BASIS=0: basis_kernel writes geom0 and layer 0 reads it, as in training (A/B switch)
  int tile_fill = 1;   // env SCANN_TILE_FILL=0: the inference edge kernels run on the contiguous tile plan (the identity order; A/B switch)
  int species_tables = 1;  // env SCANN_SPECIES_TABLES=0: the first layer's atom rows come from an atom launch, not from per-species tables
  bool generic = false;        // widths other than 128 / 8: the plain-fp32 kernels of scann_generic.hip / scann_generic_train.hip
  float* g_weights = nullptr;  // generic: the flat fp32 parameter vector on the device (spec order, spec_off offsets)
  float* g_centres = nullptr;  // generic: 20 + 20 Gaussian centres (distance, Voronoi weight)
  std::map<std::string, int64_t> g_off;  // generic: tensor name -> offset in g_weights
  // generic-width training: W^T images of the kernels (refreshed at the head of every backward), one descriptor per transposed block
  std::vector<GenTransDesc> gt_descs;
  GenTransDesc* d_gt_descs = nullptr;
  std::map<std::string, int64_t> gt_off;  // "<tensor name>#<block>" -> offset in g_WT
  float* g_WT = nullptr;
  int gt_max = 0;                         // elements of the largest block
  bool weights_exact = false;  // a loaded 128x128 kernel has |w| >= 255.9 (the split-fp16 images cannot hold it), or an operand of a projection
                               // stays below the scheme's low end (small_operands; scann_runtime.cpp: small_operand_reason): inference runs exact
  bool small_operands = false;
  std::string exact_reason;    // why weights_exact is set, naming the tensor (the text of the errors that refuse such a handle)
  bool force_exact = false;    // env SCANN_EXACT=1: every inference forward on the exact-fp32 kernels (test / diagnosis switch)
  bool strict_range = false;   // env SCANN_STRICT_RANGE=1: SCANN_ERR_RANGE instead of the exact-fp32 re-run of an inference forward
  int64_t exact_reruns = 0;    // forwards re-run on the exact-fp32 kernels so far (scann_exact_reruns)
  float* d_weights = nullptr;  // one arena with every device-side weight image
  std::vector<LayerParams> layers;
  HeadParams head{};
  BasisParams basis{};
  const float* lut = nullptr;  // [n_atoms,128] swish(Embedding . dense_embed)
  // per-species rows of the first layer (feature = "atomic" without ring): P1 = lut W1 + bg, P3 = lut W3, q = lut Wq + bq of layer 0
  // [n_atoms,128] each and a copy of the centres; recomputed on the next inference forward after the weights changed (sp_dirty)
  float *sp_c = nullptr, *sp_P1 = nullptr, *sp_P3 = nullptr, *sp_q = nullptr;
  bool sp_dirty = true;
  const float* cd = nullptr;   // distance Gaussian centres
  EmbedArgs embed{};           // weight pointers of the general embedding path (use_ring / cgcnn)
  // canonical (spec-order) flat parameter vector and how the device arena is derived from it
  std::vector<float> host_master;
  std::vector<int64_t> spec_off;
  std::vector<RepackDesc> descs;
  size_t arena_floats = 0, o_lut = 0, o_emb = 0, o_Wde = 0, o_bde = 0;
  struct LayerT {
    const float *W1T, *W2T, *W3T, *WqT, *WkT, *Wf1T, *Wf2T;                  // fp32 fragment order (modular backward)
    const _Float16 *W1Th, *W2Th, *W3Th, *WqTh, *WkTh, *Wf1Th, *Wf2Th;        // split-fp16 images (fused backward kernels)
  };
  std::vector<LayerT> layersT;  // packed transposes for the backward dX GEMMs
  const float *WaT = nullptr, *WgqT = nullptr, *WgkT = nullptr;
  const _Float16* WaTh = nullptr;  // split-fp16 image of after_Lc^T (folded into the first rn_bwd_kernel)
  // training state (scann_train_begin)
  float *t_master = nullptr, *t_grad = nullptr, *t_m = nullptr, *t_v = nullptr, *t_l2 = nullptr;
  RepackDesc* t_descs = nullptr;
  // scann_input_grads: where its backward's parameter-gradient side products go (never the training state above), allocated by its first call
  float* ig_grad = nullptr;
  int64_t t_step = 0;
  // scann_set_lr_scale: one factor per tensor (empty: none set -- the unscaled adam_kernel, the whole backward), its per-element image
  // for the scaled Adam kernel (built where the scale is set, and by scann_train_begin), and the backward's plan under it
  std::vector<float> lr_scale;
  float* t_lrs = nullptr;
  scann::TrainPlan plan;
  uint64_t stages_ran = 0;             // scann_train_stages: a bit per stage the last training backward entered
  float attn_drop_p = 0.f;             // use_drop: Dropout(0.05) on attention weights (scann_set_attention_dropout)
  bool deterministic = false;          // scann_set_deterministic: the backward's small reductions in a fixed order, no float atomics
  ncclComm_t comm = nullptr;
  // scann_train_step_begin / _end: up to two steps may be enqueued before the first is ended (the host prepares step k + 1 while the
  // device runs step k); slot = step number & 1.  Slot 2 of the targets belongs to the synchronous scann_train_forward.
  double* h_stat = nullptr;              // pinned [2][4]: {sse, count, sum |y - t|} of the step in that slot
  float* h_targets[3] = {nullptr, nullptr, nullptr};  // pinned staging of a step's targets (read by the loss kernel directly)
  size_t h_targets_cap[3] = {0, 0, 0};
  hipEvent_t step_ev[2] = {nullptr, nullptr};         // recorded at the end of the step in that slot
  int64_t step_begun = 0, step_ended = 0;
  bool grads_zeroed = false;             // the gradient vector is known to be all zeros (Adam of scann_train_step leaves it so)
  // scann_batch_upload: pinned staging buffers (a ring, grow-only) copied to the device on a stream of their own -- the call returns
  // when the copy is ENQUEUED; the batch's first launches wait for it through the batch's event
  struct Stage { char* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
  static constexpr int N_STAGE = 8;
  Stage stage[N_STAGE];
  int stage_next = 0;
  // results come back through one pinned block per stream slot (one D2H for y and the GlobalAttention scores, which sit next to each
  // other in the batch arena) instead of two staged copies into the caller's pageable arrays
  struct PadScratch { std::vector<int32_t> gidx, at, mol, eoff, col; std::vector<float> dist, wgt, ga; };  // scann_forward_padded
  PadScratch pad_scratch;
  struct DlStage { char* p = nullptr; size_t cap = 0; };
  DlStage dl_stage[MAX_STREAM];
  hipStream_t copy_stream = nullptr;
  hipStream_t train_aux2 = nullptr;      // second side stream: the basis-MLP gradients beside the embedding chain
  bool train_fused = true;               // fused backward chains (scann_train_fused.hip); SCANN_TRAIN_FUSED=0: modular kernels
  bool train_aux_borrowed = false;       // train_aux is streams[1] (not destroyed separately)
  hipStream_t train_aux = nullptr;       // side stream of the backward pass: weight-gradient GEMMs run beside the data-gradient chain
  std::vector<hipEvent_t> train_ev;      // ring of fork / join events between the two streams
  // reusable scratch of the synchronous scann_forward path (grow-only device arena + pinned host staging)
  char* sc_arena = nullptr;
  size_t sc_cap = 0;
  // scann_forward_padded: the padded payload goes over the bus BEFORE the host reads the masks (pinned + device block, grow-only)
  char* pp_host = nullptr;
  char* pp_dev = nullptr;
  size_t pp_cap = 0;
  char* sc_host = nullptr;
  size_t sc_host_cap = 0;
  struct scann_dbatch* sc_db = nullptr;
  int comm_world = 1;
  int32_t* range_flag = nullptr;  // host-pinned [MAX_STREAM], one word per stream slot (training: slot 0), written by the kernels'
                                  // range guard (flag_range), read after that stream's synchronisation
  ModelSet* models = nullptr;     // scann_models_load: K weight sets of this configuration, run by scann_forward_models (null: none)
  uint64_t models_gen = 0;        // loads of a model set so far (ModelSet::gen)
};

struct scann_dbatch {
  int32_t n_struct = 0, n_atom = 0, n_edge = 0, n_tile = 0, max_atoms = 0, tile_rows = 64, max_degree = 0, tile_atoms = TQ;
  char* arena = nullptr;  // inputs + workspace, one allocation
  // inputs
  int32_t *atomic = nullptr, *mol_offset = nullptr, *edge_offset = nullptr, *edge_col = nullptr, *edge_row = nullptr;
  float *dist = nullptr, *weight = nullptr, *ring = nullptr, *cgcnn = nullptr, *c0 = nullptr;
  EdgeTile* tiles = nullptr;
  // the tile-order side, read by the piece-major inference edge kernels alone (scann_batch_upload, launch_tile_order): their tile plan,
  // the CSR arrays in that plan's atom order -- the arrays above when the plan is the identity (filled false) -- and the per-tile slot
  // tables [n_ftile][TQ].  Null for a batch that never runs those kernels (base branch, generic widths, no edges)
  bool filled = false;      // the tile-order side is the filled plan's (ensure_tile_fill: made when the batch is forwarded again)
  bool fill_tried = false;  // ... or it has been decided that it stays the contiguous plan's
  int64_t n_fused = 0;      // forwards of the piece-major family enqueued on the batch so far
  char* fill_block = nullptr;  // the filled plan's arrays (one block of the device cache, freed with the batch)
  int32_t n_ftile = 0;
  EdgeTile* f_tiles = nullptr;
  int32_t *t_offset = nullptr, *t_col = nullptr, *t_row = nullptr;
  float *t_dist = nullptr, *t_weight = nullptr;
  int32_t *tile_atom = nullptr, *tile_edge0 = nullptr, *tile_species = nullptr;
  float *keep_q = nullptr, *keep_V = nullptr, *keep_T = nullptr, *keep_ang = nullptr, *keep_K = nullptr;  // [L][rows,128], training forward (owned by the train workspace)
  float *keep_pre1 = nullptr, *keep_H1 = nullptr, *keep_T2 = nullptr;  // ResidualNorm intermediates, [L][n_atom,128]
  float *keep_preA = nullptr, *keep_z = nullptr;  // after_Lc pre-activation / output [n_atom,128]
  bool kept = false;  // the last training forward filled them
  std::unique_ptr<scann_train_ws> train;  // created by the batch's first training forward (ensure_train_ws), freed with the batch
  hipEvent_t busy_ev = nullptr;  // end of the last scann_train_step that used the batch (scann_batch_release)
  bool idle = false;             // nothing enqueued on the batch since its last scann_batch_download returned (scann_batch_release)
  int32_t *in_off = nullptr, *in_edge = nullptr;  // reverse adjacency: edges sorted by their neighbour atom (backward pass)
  bool has_rev = false;          // in_off / in_edge are filled (uploads of a handle in training mode; else built on first backward)
  hipEvent_t upload_ev = nullptr;  // end of the asynchronous input copy (scann_batch_upload); null: the copy was synchronous
  bool upload_done = false;        // ... and it has been seen complete: launches on the batch no longer wait for it (wait_upload)
  int32_t* tile_part = nullptr;  // per tile: partial slot of a chunk tile or -1 (null without big atoms)
  int32_t* big_tab = nullptr;    // per atom with > 64 neighbours: atom row, first slot, number of slots
  float* part_buf = nullptr;     // [n_slot][3][128] softmax state of the chunk tiles
  int32_t n_big = 0, n_slot = 0;
  int32_t* pack_flag = nullptr;  // device packing (scann_upload_padded): what pack_padded_kernel found wrong with the input, behind y
  size_t gen_ws_bytes = 0;
  char* gen_ws = nullptr;  // generic-width forward: its per-batch workspace (sized by the handle's widths; cached_malloc)
  float *gen_gq = nullptr, *gen_gk = nullptr;  // ... and the readout's operands in it after an inference forward (scann_ablate_pooling)
  // workspace
  float *geom = nullptr, *gd = nullptr, *c = nullptr, *ctx = nullptr, *P1 = nullptr, *P3 = nullptr, *q = nullptr;
  float *gq = nullptr, *gk = nullptr, *ga = nullptr, *y = nullptr;
  // debug copies (allocated on demand)
  float *dbg_c = nullptr, *dbg_g = nullptr, *dbg_ctx = nullptr;
  unsigned long long* stamps = nullptr;  // diagnostic build only
  int n_stamp = 0;
  int dbg_layers = -1;
  int last_slot = 0;
  bool owns_arena = true;  // false: the arena belongs to the handle's scratch (scann_forward)
  // inference outputs of the last forward (scann_set_outputs, scann_output_read): one block of the device cache, allocated by the first
  // forward that needs it, grown when a selection needs more, freed with the batch
  char* out_block = nullptr;
  size_t out_cap = 0;
  float* out_attn = nullptr;  // [selected layers, in layer order][n_edge][num_head]
  float *out_z = nullptr, *out_bf = nullptr;  // after_Lc [n_atom, global_dim], bf_property [n_struct, dense_out]
  uint64_t out_layers = 0;  // what the last forward wrote (a training forward: nothing)
  int32_t out_flags = 0;
  // scann_predict_mc: per-atom structure table, keys, the [T, B] / [T, n_atom] samples and the reduced outputs (one block, grow-only)
  char* mc_ws = nullptr;
  size_t mc_bytes = 0;
  // scann_forward_models: every member's workspace at a fixed stride, then y [K, n_struct] and the scores [K, n_atom] (one block, grow-only)
  char* set_ws = nullptr;
  size_t set_bytes = 0;
  int set_slot = -1;    // stream slot of the batch's last set forward (-1: none)
  uint64_t set_gen = 0; // ... and the load (ModelSet::gen) whose members it ran
  int set_busy = -1;    // slot of a set forward not yet waited for by scann_models_download (-1: none): scann_batch_release then synchronises
  bool fwd_pending = false;  // a forward was enqueued (run_forward) since the batch's last scann_batch_download
};

namespace scann {

// The inputs' copy runs on the copy stream (scann_batch_upload returns when it is ENQUEUED): the first launches on the batch wait for
// its event.  A resident batch is launched on again and again; once the event has been seen complete the wait -- a barrier packet
// that costs the stream ~5 us even when it has nothing to wait for -- is left out.
inline hipError_t wait_upload(scann_dbatch* db, hipStream_t s) {
  if (!db->upload_ev || db->upload_done) return hipSuccess;
  if (hipEventQuery(db->upload_ev) == hipSuccess) {
    db->upload_done = true;
    return hipSuccess;
  }
  (void)hipGetLastError();  // (hipErrorNotReady is an answer, not an error)
  return hipStreamWaitEvent(s, db->upload_ev, 0);
}

int fail(scann_handle* h, int code, const std::string& msg);  // h null: the error of scann_create (scann_last_error(NULL))
int check_range(scann_handle* h, const char* where, int slot = 0);

#define HIPCHK(h, expr)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return fail(h, e_ == hipErrorOutOfMemory ? SCANN_ERR_OOM : SCANN_ERR_HIP,                       \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
  } while (0)

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// scann_runtime.cpp: scann_load_weights; at non-null: the arena (and the first layer's per-species tables behind it) is placed there, not
// allocated; need non-null: validation only, *need = the floats such a placement takes
int load_weights(scann_handle* h, const float* blob, const scann_tensor_desc_t* manifest, int n, float* at, size_t* need);

// The workspace pointers a forward writes: the batch's own (FwdBufs(db)) unless the caller sends the activations or the results
// elsewhere (scann_predict_mc: row t of its sample matrices as y / ga; a set forward: a member's slice of the set workspace)
struct FwdBufs {
  float *geom, *gd, *c0, *c, *ctx, *P1, *P3, *q, *gq, *gk, *part_buf, *y, *ga;
  explicit FwdBufs(const scann_dbatch* db)
      : geom(db->geom), gd(db->gd), c0(db->c0), c(db->c), ctx(db->ctx), P1(db->P1), P3(db->P3), q(db->q), gq(db->gq), gk(db->gk),
        part_buf(db->part_buf), y(db->y), ga(db->ga) {}
};

// A training forward: the Dropout layers active, the tensors of the backward kept
struct FwdTrain {
  float drop_p, attn_p;     // Dropout(0.1) layers / attention-weight rates
  unsigned long long seed;
  bool keep_backward;       // 128 / 8 kernels: q, V, T, ang, K, the ResidualNorm and after_Lc intermediates go to the batch's keep_* buffers
  GenKeep* gen;             // generic widths: where every intermediate is kept
};

constexpr int32_t FWD_OUT_UNTOUCHED = -1;  // FwdOpts::out_flags: the forward writes no outputs and leaves the batch's output block and db->out_* alone

// The forward run_forward is to enqueue: everything that distinguishes one forward from another is here, nothing is looked up in the
// handle or the batch at launch time.  The defaults mean: the plain inference forward of the batch on the handle's own weights, no outputs.
struct FwdOpts {
  bool exact = false;               // on the exact-fp32 instantiations (forced by SCANN_EXACT=1 and by weights the split-fp16 images cannot hold)
  Timer* tm = nullptr;              // scann_forward_profile
  const FwdTrain* train = nullptr;  // kind of forward -- null, null: inference; a training forward; ...
  const McState* mc = nullptr;      // ... a Monte Carlo dropout sample (an inference forward under that sample's masks)
  int keep_layers = -1;             // every layer's centres / context / geometry into the debug buffers (scann_debug_read); -1: the handle's
                                    // scann_set_debug switch
  // the outputs this forward also writes into the batch's output block -- bit k: local_attention_k's weights; out_flags: SCANN_OUT_AFTER_LC
  // | SCANN_OUT_BF_PROPERTY -- and db->out_* record (a training forward: none, whatever is asked for).  out_flags = FWD_OUT_UNTOUCHED: a
  // forward beside the batch's own (a Monte Carlo sample, the members of a model set), which leaves the block and db->out_* as they are
  uint64_t out_layers = 0;
  int32_t out_flags = 0;
  const FwdBufs* bufs = nullptr;    // where activations and results go; null: the batch's own workspace
  int slot = -1;                    // stream slot whose range-guard word the kernels write; -1: db->last_slot
  // whose weight images (layers, head, basis, lut, sp_*, cd, embed, g_*, weights_exact, cfg.relu_out); null: the handle's own.  Streams,
  // switches, range-guard words, timing state and the error text are always those of the handle the call is made on
  scann_handle* weights = nullptr;
  // one launch sequence for n_member members of a model set (the SET instantiations; never with exact, train, mc, keep_layers): their
  // weight holders, whose images lie m_w bytes apart; bufs is the first one's, the others' m_a bytes (y: m_y, ga: m_g) further each
  int n_member = 0;                 // 0: not a set launch
  scann_handle* const* members = nullptr;
  int64_t m_w = 0, m_a = 0, m_y = 0, m_g = 0;
  // part of a set forward: not the batch's single-model work (db->idle / db->fwd_pending stay; set work is db->set_busy), no edge-timing samples
  bool of_set = false;
};

// The options of a public inference forward: the outputs scann_set_outputs selected, plus `layers` / `flags` for this one forward.  The
// one place that reads the handle's selection
inline FwdOpts selected_opts(const scann_handle* h, uint64_t layers = 0, int32_t flags = 0) {
  FwdOpts o;
  o.out_layers = h->out_layers | layers;
  o.out_flags = h->out_flags | flags;
  return o;
}

// scann_forward.cpp: the forward graph as a launch schedule on stream s
int run_forward(scann_handle* h, scann_dbatch* db, hipStream_t s, const FwdOpts& o);

// scann_batch.cpp
int check_pack_flag(scann_handle_t* h, scann_dbatch_t* db, const char* who);
// after the batch's stream has been synchronised: the forward's range guard fired -> run it again on the exact-fp32 instantiations,
// writing the outputs the batch recorded for it (*rerun = true), unless SCANN_STRICT_RANGE asks for the error (check_range reports it)
int rerun_if_out_of_range(scann_handle_t* h, scann_dbatch_t* db, hipStream_t s, bool* rerun);
// the filled tile plan of a batch that is forwarded again (scann_batch.cpp); a no-op once it has been made or decided against
int ensure_tile_fill(scann_handle_t* h, scann_dbatch_t* db, hipStream_t s);
// One inference forward of a resident batch on its last_slot stream, writing `layers` / `flags` besides the handle's selected outputs,
// and its results fetched as scann_batch_download fetches them (pack flag, range guard, exact re-run, db->idle); y / ga: host, or null
int forward_and_download(scann_handle_t* h, scann_dbatch_t* db, uint64_t layers, int32_t flags, float* y, float* ga);
// atoms of a resident batch by structure: its device copy of mol_offset [n_struct + 1] (the host keeps none), once the upload has ended
int read_mol_offset(scann_handle_t* h, const scann_dbatch_t* db, std::vector<int32_t>& mol);
void free_batch(scann_dbatch* db);  // everything the batch holds, and the batch; no work on it may still be running

}  // namespace scann

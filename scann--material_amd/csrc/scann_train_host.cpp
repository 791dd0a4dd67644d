// Training path: the per-batch training workspace, training-mode forward, hand-written backward, Adam
// and the one-call step.  The all-reduces between ranks are in scann_comm.cpp.
#include "scann_runtime.h"

namespace {

int ensure_train_ws(scann_handle* h, scann_dbatch* db, scann_train_ws** out) {
  if (!db->train) db->train = std::make_unique<scann_train_ws>();
  scann_train_ws& w = *db->train;
  *out = &w;
  if (w.arena) return SCANN_OK;
  if (h->generic) {  // loss statistics, targets, d loss / d y; the tensors live in w.gen (run_forward_generic, gen_backward)
    const size_t nb = align_up((size_t)db->n_struct * 4);
    HIPCHK(h, cached_malloc((void**)&w.arena, 256 + 2 * nb));
    w.sse = (double*)w.arena;
    w.dy = (float*)(w.arena + 256);
    w.targets = (float*)(w.arena + 256 + nb);
    return SCANN_OK;
  }
  const size_t rowA = align_up((size_t)db->n_atom * D * 4), rowE = align_up((size_t)std::max(db->n_edge, 1) * D * 4);
  const size_t rowB = align_up((size_t)db->n_struct * D * 4);
  // per-layer tensors kept by the training forward (edge_kernel_lean on 64-edge tiles): q [A,128]; V, T, ang, K [E,128]
  // (base branch: geomL in the V slices, T unused)
  const size_t Lk = (size_t)h->cfg.n_attention;
  const size_t Lc = (size_t)h->cfg.n_attention;
  w.wpart_floats = wpart_slot_floats(db->n_atom, db->n_edge, db->n_struct, h->cfg.n_attention, db->max_degree, db->n_tile);
  // the operands of a layer's weight gradients live until the end of the step (sets of their own per layer): the gradient launches on
  // the side stream never have to be waited for before a buffer is reused
  // the modular backward (SCANN_TRAIN_FUSED=0) reads T and ang as tensors; the fused chains form them again
  const bool keep_all = !h->train_fused;
  const size_t n_keepE = keep_all ? 4 : h->cfg.g_update ? 2 : 3;
  const size_t nTA = 5 + 5 * (Lc + 1), nTE = 4 + 2 * (Lc + 1);
  const size_t total = nTA * rowA + nTE * rowE + 2 * rowB + 2 * align_up((size_t)db->n_struct * 4) +
                       align_up((size_t)h->cfg.n_atoms * D * 4) + 256 + Lk * (4 * rowA + n_keepE * rowE) + 2 * rowA + align_up(w.wpart_floats * 4);
  HIPCHK(h, cached_malloc((void**)&w.arena, total));
  char* p = w.arena;
  w.tA.assign(nTA, nullptr);
  w.tE.assign(nTE, nullptr);
  for (size_t i = 0; i < nTA; ++i) { w.tA[i] = (float*)p; p += rowA; }
  for (size_t i = 0; i < nTE; ++i) { w.tE[i] = (float*)p; p += rowE; }
  w.rep = (float*)p; p += rowB;
  w.dpre = (float*)p; p += rowB;
  w.dy = (float*)p; p += align_up((size_t)db->n_struct * 4);
  w.targets = (float*)p; p += align_up((size_t)db->n_struct * 4);
  w.dlut = (float*)p; p += align_up((size_t)h->cfg.n_atoms * D * 4);
  // (zero from here on between steps: embed_bwd_kernel clears every row it consumes -- one memset command per step less on the
  //  main stream; this one is the workspace's first and only, on the stream every training launch of the handle goes to)
  HIPCHK(h, hipMemsetAsync(w.dlut, 0, (size_t)h->cfg.n_atoms * D * 4, h->streams[0]));
  w.sse = (double*)p; p += 256;
  w.wpart = (float*)p; p += align_up(w.wpart_floats * 4);
  if (Lk) {  // slices are [rows,128] without padding between layers: size them from the un-aligned row counts
    w.keep_q = (float*)p; p += Lk * rowA;
    w.keep_V = (float*)p; p += Lk * rowE;
    if (keep_all) {
      w.keep_T = (float*)p; p += Lk * rowE;
      w.keep_ang = (float*)p; p += Lk * rowE;
    } else if (!h->cfg.g_update) {  // base branch: the gated rows feed edge_dang_kernel as they are
      w.keep_ang = (float*)p; p += Lk * rowE;
    }
    w.keep_K = (float*)p; p += Lk * rowE;
    w.keep_pre1 = (float*)p; p += Lk * rowA;
    w.keep_H1 = (float*)p; p += Lk * rowA;
    w.keep_preA = (float*)p; p += rowA;
    w.keep_z = (float*)p; p += rowA;
    w.keep_T2 = (float*)p; p += Lk * rowA;
  }
  return SCANN_OK;
}

// Data-gradient mode of the backward (scann_input_grads): device outputs of its leaves, null where not asked for.  In this mode the
// backward seeds nothing itself (dy = 1 is in place), enqueues no weight-gradient work and leaves the training state alone.
struct InGrad {
  float *d_dist, *d_weight, *d_ring, *d_cgcnn;
};

// generic widths: the backward's d x = d z . W^T runs through gen_dense_kernel on transposed images of the kernels: one block per kernel,
// except that filter_geo of the g_update branch is cut into its centre / geometry / neighbour thirds (attention.py:142-150) and
// dense_embed with the ring input into its embedding / ring rows (scann_model.py:367-373) -- each third's d x is a tensor of its own.
// The descriptors depend on the configuration only; gen_backward refreshes the images from the current weights.
int build_gen_transposes(scann_handle* h) {
  h->gt_descs.clear();
  h->gt_off.clear();
  int64_t off = 0;
  h->gt_max = 0;
  const int d = h->cfg.local_dim, emb = h->cfg.embedding_dim;
  for (size_t i = 0; i < h->specs.size(); ++i) {
    const WeightSpec& sp = h->specs[i];
    const std::string& nm = sp.name;
    if (!(sp.cols > 0 && nm.size() > 7 && nm.compare(nm.size() - 7, 7, "/kernel") == 0)) continue;
    std::vector<int> cuts{0, (int)sp.rows};
    if (h->cfg.g_update && nm.find("/filter_geo/") != std::string::npos && sp.rows == 3 * d) cuts = {0, d, 2 * d, 3 * d};
    if (nm == "dense_embed/kernel" && h->cfg.use_ring) cuts = {0, emb, emb + 10};
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
      const int kn = cuts[b + 1] - cuts[b];
      h->gt_descs.push_back(GenTransDesc{h->spec_off[i], off, cuts[b], kn, (int32_t)sp.cols});
      h->gt_off[nm + "#" + std::to_string(b)] = off;
      off += (int64_t)kn * sp.cols;
      h->gt_max = std::max(h->gt_max, kn * (int)sp.cols);
    }
  }
  if (h->g_WT) (void)hipFree(h->g_WT);
  if (h->d_gt_descs) (void)hipFree(h->d_gt_descs);
  h->g_WT = nullptr;
  h->d_gt_descs = nullptr;
  HIPCHK(h, hipMalloc((void**)&h->g_WT, (size_t)std::max<int64_t>(off, 1) * 4));
  HIPCHK(h, hipMalloc((void**)&h->d_gt_descs, h->gt_descs.size() * sizeof(GenTransDesc)));
  HIPCHK(h, hipMemcpy(h->d_gt_descs, h->gt_descs.data(), h->gt_descs.size() * sizeof(GenTransDesc), hipMemcpyHostToDevice));
  return SCANN_OK;
}

// scann_set_lr_scale: the per-element image of the per-tensor factors, as t_l2 is of the regulariser mask
int upload_lr_scale(scann_handle* h) {
  const size_t n = h->host_master.size();
  std::vector<float> e(n, 1.0f);
  for (size_t i = 0; i < h->specs.size(); ++i)
    std::fill(e.begin() + h->spec_off[i], e.begin() + h->spec_off[i] + h->specs[i].numel(), h->lr_scale[i]);
  if (!h->t_lrs) HIPCHK(h, hipMalloc((void**)&h->t_lrs, n * 4));
  HIPCHK(h, hipMemcpy(h->t_lrs, e.data(), n * 4, hipMemcpyHostToDevice));
  return SCANN_OK;
}

int64_t spec_offset(const scann_handle* h, const std::string& name) {
  for (size_t i = 0; i < h->specs.size(); ++i)
    if (h->specs[i].name == name) return h->spec_off[i];
  return -1;
}

}  // namespace

// the training forward (activations kept for the backward) and the batch's sum of squared errors + count -> w->sse[0..1]; no sync
// attn_p: the attention-dropout rate (training: the handle's scann_set_attention_dropout; scann_input_grads: 0)
static int train_forward_impl(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, float attn_p, uint64_t seed,
                              scann_train_ws** wout, int slot) {  // slot 0 / 1: a scann_train_step in that slot; 2: the synchronous scann_train_forward
  const bool fused_step = slot < 2;
  scann_train_ws* w = nullptr;
  int r = ensure_train_ws(h, db, &w);
  if (r) return r;
  hipStream_t s = h->streams[0];
  db->last_slot = 0;
  w->drop_p = dropout;
  w->seed = seed;
  db->keep_q = w->keep_q; db->keep_V = w->keep_V; db->keep_T = w->keep_T; db->keep_ang = w->keep_ang; db->keep_K = w->keep_K;
  db->keep_pre1 = w->keep_pre1; db->keep_H1 = w->keep_H1; db->keep_T2 = w->keep_T2;
  db->keep_preA = w->keep_preA; db->keep_z = w->keep_z;
  db->kept = false;
  if (h->generic) {  // run_forward_generic keeps its tensors in w->gen
    w->gen.drop_p = dropout;
    w->gen.attn_p = attn_p;
    w->gen.seed = seed;
  }
  w->attn_p = attn_p;
  const FwdTrain tr{dropout, attn_p, (unsigned long long)seed, /*keep_backward=*/true, h->generic ? &w->gen : nullptr};
  FwdOpts o;
  o.train = &tr;
  o.keep_layers = !h->generic;  // keep centres / geometry / context of every layer (and, with edge_kernel_lean, q / V / T / ang / K)
  db->last_slot = 0;  // training runs on stream 0 (its range-guard word is slot 0's)
  r = run_forward(h, db, s, o);
  if (r) return r;
  if (h->generic) {
    db->kept = true;
    db->dbg_layers = h->cfg.n_attention;
  }
  if (!targets) {  // scann_input_grads: no loss
    *wout = w;
    return SCANN_OK;
  }
  // targets: staged in pinned memory that the loss kernel reads directly (it leaves the device copy the backward uses): no copy operation
  if (h->h_targets_cap[slot] < (size_t)db->n_struct) {
    if (h->h_targets[slot]) {
      HIPCHK(h, hipStreamSynchronize(s));  // an earlier step may still be reading the buffer that is about to be replaced
      (void)hipHostFree(h->h_targets[slot]);
    }
    h->h_targets[slot] = nullptr;
    h->h_targets_cap[slot] = 0;
    HIPCHK(h, hipHostMalloc((void**)&h->h_targets[slot], (size_t)db->n_struct * 4));
    h->h_targets_cap[slot] = (size_t)db->n_struct;
  }
  memcpy(h->h_targets[slot], targets, (size_t)db->n_struct * 4);
  const bool single = !(h->comm && h->comm_world > 1);
  if (fused_step && !h->h_stat) HIPCHK(h, hipHostMalloc((void**)&h->h_stat, 2 * 4 * sizeof(double)));
  // single-rank fused step: the loss kernel also forms d rmse / d y and posts {sse, count, sum |y - t|} to the slot's pinned triple
  launch_sse(db->y, h->h_targets[slot], db->n_struct, w->sse, w->targets, fused_step && single ? w->dy : nullptr,
             fused_step && single ? h->h_stat + 4 * slot : nullptr, s);
  *wout = w;
  return SCANN_OK;
}

// Reverse adjacency of a batch that was uploaded while the handle was not in training mode (scann_batch_upload skips it then):
// the neighbour indices come back from the device, the counting sort runs on the host as in upload_impl.  Synchronous; once per batch.
static int ensure_reverse(scann_handle_t* h, scann_dbatch_t* db) {
  if (db->has_rev) return SCANN_OK;
  const int A = db->n_atom, E = db->n_edge;
  hipStream_t s = h->streams[0];
  HIPCHK(h, wait_upload(db, s));
  std::vector<int32_t> col((size_t)std::max(E, 1)), in_off((size_t)A + 1, 0), in_edge((size_t)std::max(E, 1));
  if (E > 0) HIPCHK(h, hipMemcpyAsync(col.data(), db->edge_col, (size_t)E * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  for (int e = 0; e < E; ++e) ++in_off[(size_t)col[(size_t)e] + 1];
  for (int a = 0; a < A; ++a) in_off[(size_t)a + 1] += in_off[(size_t)a];
  std::vector<int32_t> fill(in_off.begin(), in_off.begin() + A);
  for (int e = 0; e < E; ++e) in_edge[(size_t)fill[(size_t)col[(size_t)e]]++] = e;
  HIPCHK(h, hipMemcpyAsync(db->in_off, in_off.data(), (size_t)(A + 1) * 4, hipMemcpyHostToDevice, s));
  if (E > 0) HIPCHK(h, hipMemcpyAsync(db->in_edge, in_edge.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));
  db->has_rev = true;
  return SCANN_OK;
}

// The backward pass of create_model (scann_model.py:362-447) for a generic-width handle: the formulas of backward_impl below, one plain
// kernel each (scann_generic_train.hip), on the tensors the training forward kept (GenKeep).  One stream; gradients are ACCUMULATED
// into the flat gradient vector (two backward calls give the gradient of the sum, as on the 128-wide path).
// ig non-null: the data-gradient mode (InGrad): no weight gradients, the parameter-gradient side products of the LayerNorm backward go to
// h->ig_grad, and the input leaves are called where the weight-gradient leaves would be.
static int gen_backward(scann_handle_t* h, scann_dbatch_t* db, scann_train_ws& w, float scale, const double* d_stat, bool dy_done,
                        const InGrad* ig) {
  hipStream_t s = h->streams[0];
  const scann_config_t& c = h->cfg;
  GenKeep& kp = w.gen;
  const int L = c.n_attention, A = db->n_atom, E = db->n_edge, B = db->n_struct;
  const int d = c.local_dim, dg = c.global_dim, dout = c.dense_out, H = c.num_head, emb = c.embedding_dim;
  const int cin = emb + (c.use_ring ? 10 : 0);
  if (!kp.arena || (int)kp.layer.size() != L) return fail(h, SCANN_ERR_INVALID, "scann_train_backward: run scann_train_forward on this batch first");
  if ((size_t)std::max(std::max(dg, dout), std::max(3 * d, std::max(cin, 92))) * 4 * 4 > 60000)
    return fail(h, SCANN_ERR_UNSUPPORTED, "backward (generic widths): a layer's rows exceed one workgroup's LDS");
  // launch limits of two kernels, checked BEFORE anything is launched (a refused launch would otherwise surface as a bare hipGetLastError at
  // the end, after earlier kernels have added into the gradient vector): gen_table_part_kernel's grid.y = 64-atom chunks,
  // gen_attn_bwd_kernel's dynamic LDS = 3 x max_degree x heads floats
  if (!c.feature_cgcnn && (A + 63) / 64 > 65535)
    return fail(h, SCANN_ERR_UNSUPPORTED, "backward (generic widths): more than 4,194,240 atoms in one batch (Embedding gradient: 65,535 chunks of 64 atoms)");
  if ((size_t)3 * std::max(1, db->max_degree) * H * sizeof(float) > 65536)
    return fail(h, SCANN_ERR_UNSUPPORTED, "backward (generic widths): an atom's neighbours x heads exceed one workgroup's LDS (3 x max_degree x num_head floats <= 64 KiB)");
  if (((size_t)3 * db->max_atoms + 4) * sizeof(double) > 65536)
    return fail(h, SCANN_ERR_UNSUPPORTED, "backward (generic widths): a structure's atoms exceed one workgroup's LDS (GlobalAttention pooling: 3 x atoms doubles <= 64 KiB)");
  // ---- temporaries ----
  const size_t fA = (size_t)A, fE = (size_t)std::max(E, 1), fB = (size_t)B;
  const size_t dmax = (size_t)std::max(d, std::max(dg, dout));
  const size_t need0 = 4 * (fA * (8 * (size_t)d + 4 * (size_t)dg + (size_t)emb + 10) + fE * 9 * (size_t)d + fB * (2 * (size_t)dout + (size_t)dg) +
                           2 * std::max(fA, fE) + 2 * 512 * dmax) + 256 * 48;
  // per-slab partial tiles of a weight gradient (gen_dense_dw_kernel): slabs x tiles <= 1024 + tiles (gen_dw_slabs), 1024 floats a tile
  const size_t Kmax = (size_t)std::max(std::max(3 * d, dg), std::max(std::max(dout, cin), 92));
  const size_t wpart = (1024 + ((Kmax + 31) / 32) * ((dmax + 31) / 32)) * 1024 + 64 * dmax;
  const size_t tpart = c.feature_cgcnn ? 0 : ((fA + 63) / 64) * (size_t)c.n_atoms * (size_t)emb;  // Embedding gradient: per-chunk sums
  const size_t need = need0 + 4 * (wpart + tpart);
  if (kp.bbytes < need) {
    HIPCHK(h, hipStreamSynchronize(s));
    cached_free(kp.barena);
    kp.barena = nullptr;
    kp.bbytes = 0;
    HIPCHK(h, cached_malloc((void**)&kp.barena, need));
    kp.bbytes = need;
  }
  float* p = reinterpret_cast<float*>(kp.barena);
  auto take = [&](size_t n) { float* q = p; p += (n + 63) & ~(size_t)63; return q; };
  float *dCa = take(fA * d), *dCb = take(fA * d), *dXr = take(fA * d), *tA1 = take(fA * d), *tA2 = take(fA * d), *dT1 = take(fA * d), *dQ = take(fA * d);
  float *dz = take(fA * dg), *dgq = take(fA * dg), *dgk = take(fA * dg), *dv = take(fA * (emb + 10));
  float *dK = take(fE * d), *dang = take(fE * d), *dGt = take(fE * d), *dT = take(fE * d), *dZ = take(fE * d), *dXi = take(fE * d), *dXj = take(fE * d);
  float *dGa = take(fE * d), *dGb = take(fE * d);
  float *dhid = take(fB * dout), *drep = take(fB * dg);
  float *stats = take(2 * std::max(fA, fE)), *part = take(2 * 512 * dmax), *wp = take(wpart), *tp_ = take(tpart);
  if (reinterpret_cast<char*>(p) > kp.barena + kp.bbytes) return fail(h, SCANN_ERR_HIP, "backward (generic widths): workspace overrun");
  // ---- helpers ----
  launch_gen_transpose(h->d_gt_descs, (int)h->gt_descs.size(), h->gt_max, h->g_weights, h->g_WT, s);
  auto Wp = [&](const std::string& name) -> const float* { return h->g_weights + h->g_off.at(name); };
  auto WT = [&](const std::string& name, int blk = 0) -> const float* { return h->g_WT + h->gt_off.at(name + "/kernel#" + std::to_string(blk)); };
  auto G = [&](const std::string& name) -> float* { return (ig ? h->ig_grad : h->t_grad) + h->g_off.at(name); };
  const GenSeg none{nullptr, nullptr, 0};
  // d x [rows, n_in] = d z [rows, n_out] . W^T (+ res)
  auto dx = [&](const float* dZ_, int rows, int n_out, int n_in, const float* wt, const float* res, float* out) {
    GenDenseArgs a{};
    a.seg[0] = GenSeg{dZ_, nullptr, n_out}; a.seg[1] = none; a.seg[2] = none; a.n_seg = 1;
    a.W = wt; a.b = nullptr; a.K = n_out; a.N = n_in; a.rows = rows; a.res = res; a.Y = out;
    launch_gen_dense(a, s);
  };
  bool part_overrun = false;
  auto dw = [&](GenSeg s0, GenSeg s1, GenSeg s2, int n_seg, int prod, const float* dZ_, int K_, int N_, int rows, const std::string& name) {
    if (ig) return;
    GenDwArgs a{};
    a.seg[0] = s0; a.seg[1] = s1; a.seg[2] = s2; a.n_seg = n_seg; a.prod = prod;
    a.dZ = dZ_; a.K = K_; a.N = N_; a.rows = rows; a.dW = G(name + "/kernel"); a.db = G(name + "/bias"); a.part = wp;
    if (rows > 0 && gen_dw_part_floats(rows, K_, N_) > wpart) { part_overrun = true; return; }
    launch_gen_dense_dw(a, s);
  };
  auto lnb = [&](const float* X, const float* res, const std::string& name, const float* dY, int rows, float* dX) {
    launch_gen_layernorm_bwd(X, res, Wp(name + "/gamma"), dY, rows, d, dX, stats, part, G(name + "/gamma"), G(name + "/beta"), s);
  };
  if (!dy_done) launch_dy(db->y, w.targets, B, scale, d_stat, w.dy, s);
  // ---- property head (scann_model.py:437-447; mrelu's gradient is the identity, custom_layers.py:6-15) ----
  dw(GenSeg{kp.hid, nullptr, dout}, none, none, 1, 0, w.dy, dout, 1, B, "predict_property");
  dx(w.dy, B, 1, dout, WT("predict_property"), nullptr, dhid);
  launch_gen_act_bwd(dhid, kp.hid_pre, nullptr, B, dout, 0.f, 0, 0, dhid, s);
  dw(GenSeg{kp.rep, nullptr, dg}, none, none, 1, 0, dhid, dg, dout, B, "bf_property");
  dx(dhid, B, dout, dg, WT("bf_property"), nullptr, drep);
  // ---- GlobalAttention pooling, its projections, after_Lc (attention.py:279-316; scann_model.py:424-434) ----
  launch_gen_pool_bwd(db->mol_offset, B, db->max_atoms, kp.gq, kp.gk, dg, c.use_ga_norm, drep, dgq, dgk, s);
  kp.dbg = {{"gq", {kp.gq, fA * dg}}, {"gk", {kp.gk, fA * dg}}, {"z", {kp.z, fA * dg}}, {"rep", {kp.rep, fB * dg}}, {"drep", {drep, fB * dg}},
            {"dgq", {dgq, fA * dg}}, {"dgk", {dgk, fA * dg}}, {"dz", {dz, fA * dg}}};
  dw(GenSeg{kp.z, nullptr, dg}, none, none, 1, 0, dgq, dg, dg, A, "global_attention/query");
  dw(GenSeg{kp.z, nullptr, dg}, none, none, 1, 0, dgk, dg, dg, A, "global_attention/key");
  dx(dgq, A, dg, dg, WT("global_attention/query"), nullptr, dz);
  dx(dgk, A, dg, dg, WT("global_attention/key"), dz, dz);
  launch_gen_act_bwd(dz, kp.z_pre, nullptr, A, dg, 0.f, 0, 0, dz, s);
  dw(GenSeg{kp.cc_L, nullptr, d}, none, none, 1, 0, dz, d, dg, A, "after_Lc");
  float *dC = dCa, *dC_other = dCb;
  dx(dz, A, dg, d, WT("after_Lc"), nullptr, dC);
  const float* dGn = nullptr;  // gradient of the geometry leaving layer l (nothing reads the last layer's)
  float *dG_next = dGa, *dG_spare = dGb;
  // ---- LocalAttention + ResidualNorm iterations, last to first (attention.py:118-216, :37-40) ----
  for (int l = L - 1; l >= 0; --l) {
    const GenLayerKeep& b = kp.layer[(size_t)l];
    const std::string la = "local_attention_" + std::to_string(l), rn = "residual_norm_" + std::to_string(l);
    const float* dCtx = dC;
    if (c.use_attn_norm) {  // c' = LayerNorm(ctx + Dropout(dense_2(swish(dense_1 ctx))))
      lnb(b.ctx, b.t2, rn + "/layer_norm", dC, A, dXr);
      launch_gen_act_bwd(dXr, nullptr, nullptr, A, d, kp.drop_p, (unsigned)l, kp.seed, tA1, s);  // through the Dropout mask
      dw(GenSeg{b.h1, nullptr, d}, none, none, 1, 0, tA1, d, d, A, rn + "/dense_2");
      dx(tA1, A, d, d, WT(rn + "/dense_2"), nullptr, tA2);
      launch_gen_act_bwd(tA2, b.pre1, nullptr, A, d, 0.f, 0, 0, tA2, s);
      dw(GenSeg{b.ctx, nullptr, d}, none, none, 1, 0, tA2, d, d, A, rn + "/dense_1");
      dx(tA2, A, d, d, WT(rn + "/dense_1"), dXr, dXr);  // + the residual branch
      dCtx = dXr;
    }
    lnb(b.t1, nullptr, la + "/layer_norm", dCtx, A, dT1);
    launch_gen_attn_bwd(b.q, b.K, db->edge_offset, A, d, H, db->max_degree, dT1, kp.attn_p, DROP_TAG_ATTN + (unsigned)l, kp.seed, dQ, dK, s);
    dw(GenSeg{b.cc_in, nullptr, d}, none, none, 1, 0, dQ, d, d, A, la + "/query");
    dw(GenSeg{b.cc_in, db->edge_col, d}, GenSeg{b.Gn, nullptr, d}, none, 2, 1, dK, d, d, E, la + "/key");
    dx(dQ, A, d, d, WT(la + "/query"), nullptr, dC_other);
    dx(dK, E, d, d, WT(la + "/key"), nullptr, dang);  // gradient of the gated rows c[j] * g (attention.py:157)
    if (c.g_update) {
      launch_gen_mul_gather(dang, b.cc_in, db->edge_col, dGn, E, d, dGt, s);  // d g' = dang * c[j] + what the layer above left
      lnb(b.T, nullptr, la + "/layer_norm_g", dGt, E, dT);
      launch_gen_act_bwd(dT, b.Z, nullptr, E, d, 0.f, 0, 0, dZ, s);
      dw(GenSeg{b.cc_in, db->edge_row, d}, GenSeg{b.G_in, nullptr, d}, GenSeg{b.cc_in, db->edge_col, d}, 3, 0, dZ, 3 * d, d, E, la + "/filter_geo");
      dx(dZ, E, d, d, WT(la + "/filter_geo", 0), nullptr, dXi);
      dx(dZ, E, d, d, WT(la + "/filter_geo", 1), dT, dG_next);  // + the residual geometry (attention.py:152)
      dx(dZ, E, d, d, WT(la + "/filter_geo", 2), nullptr, dXj);
      launch_gen_edge_to_atom(db->edge_offset, db->in_off, db->in_edge, dXi, dXj, dang, b.Gn, dC_other, A, d, dC_other, s);
      dGn = dG_next;
      std::swap(dG_next, dG_spare);
    } else {  // g = swish(basis . Wf + bf) * Voronoi weight (attention.py:159-163)
      launch_gen_mul_gather(dang, b.cc_in, db->edge_col, nullptr, E, d, dGt, s);
      if (ig) {
        launch_base_input_grad(db->dist, db->weight, dGt, Wp(la + "/filter_geo/kernel"), Wp(la + "/filter_geo/bias"), h->g_centres, E, d,
                               ig->d_dist, ig->d_weight, s);
      } else {
        launch_gen_act_bwd(dGt, b.Z, db->weight, E, d, 0.f, 0, 0, dZ, s);
        dw(GenSeg{kp.gd, nullptr, NG}, none, none, 1, 0, dZ, NG, d, E, la + "/filter_geo");
      }
      launch_gen_edge_to_atom(db->edge_offset, db->in_off, db->in_edge, nullptr, nullptr, dang, b.Gn, dC_other, A, d, dC_other, s);
    }
    std::swap(dC, dC_other);
  }
  if (ig) {  // the input leaves (scann_input_grad.hip) in place of the basis-MLP and embedding weight gradients
    if (c.g_update && dGn)
      launch_basis_input_grad(db->dist, db->weight, dGn, Wp("neighbor_d/kernel"), Wp("neighbor_d/bias"), Wp("neighbor_w/kernel"),
                              Wp("neighbor_w/bias"), h->g_centres, h->g_centres + NG, E, d, ig->d_dist, ig->d_weight, s);
    if (ig->d_ring || ig->d_cgcnn) {
      InputGradEmbed e{};
      e.width = d; e.emb_dim = emb; e.dC = dC; e.atomic = db->atomic;
      e.cgcnn = c.feature_cgcnn ? db->cgcnn : nullptr;
      e.ring = c.use_ring ? db->ring : nullptr;
      if (c.feature_cgcnn) { e.We = Wp("embed_atom/kernel"); e.be = Wp("embed_atom/bias"); }
      else e.emb = Wp("embed_atom/embeddings");
      if (c.use_ring) { e.Wr = Wp("extra_embed/kernel"); e.br = Wp("extra_embed/bias"); }
      e.Wde = Wp("dense_embed/kernel"); e.bde = Wp("dense_embed/bias");
      e.d_ring = ig->d_ring; e.d_cgcnn = ig->d_cgcnn;
      launch_embed_input_grad(e, A, s);
    }
    HIPCHK(h, hipGetLastError());
    return SCANN_OK;
  }
  // ---- basis MLP of the initial geometry (scann_model.py:386-391) ----
  if (c.g_update && dGn) {
    launch_gen_mul_gather(dGn, kp.Tw, nullptr, nullptr, E, d, dT, s);
    launch_gen_act_bwd(dT, kp.pre_d, nullptr, E, d, 0.f, 0, 0, dT, s);
    dw(GenSeg{kp.gd, nullptr, NG}, none, none, 1, 0, dT, NG, d, E, "neighbor_d");
    launch_gen_mul_gather(dGn, kp.Td, nullptr, nullptr, E, d, dZ, s);
    launch_gen_act_bwd(dZ, kp.pre_w, nullptr, E, d, 0.f, 0, 0, dZ, s);
    dw(GenSeg{kp.gw, nullptr, NG}, none, none, 1, 0, dZ, NG, d, E, "neighbor_w");
  }
  // ---- embedding (scann_model.py:362-374) ----
  launch_gen_act_bwd(dC, kp.pre_e, nullptr, A, d, kp.drop_p, DROP_TAG_EMBED, kp.seed, tA1, s);
  const GenSeg e0 = c.feature_cgcnn ? GenSeg{kp.embE, nullptr, emb} : GenSeg{Wp("embed_atom/embeddings"), db->atomic, emb};
  if (c.use_ring) dw(e0, GenSeg{kp.ring10, nullptr, 10}, none, 2, 0, tA1, cin, d, A, "dense_embed");
  else dw(e0, none, none, 1, 0, tA1, emb, d, A, "dense_embed");
  dx(tA1, A, d, emb, WT("dense_embed", 0), nullptr, dv);
  if (c.feature_cgcnn) dw(GenSeg{db->cgcnn, nullptr, 92}, none, none, 1, 0, dv, 92, emb, A, "embed_atom");
  else launch_gen_table_grad(db->atomic, A, dv, emb, c.n_atoms, tp_, G("embed_atom/embeddings"), s);
  if (c.use_ring) {
    dx(tA1, A, d, 10, WT("dense_embed", 1), nullptr, dv);
    dw(GenSeg{db->ring, nullptr, 2}, none, none, 1, 0, dv, 2, 10, A, "extra_embed");
  }
  if (part_overrun) return fail(h, SCANN_ERR_HIP, "backward (generic widths): a weight gradient's partial tiles exceed their scratch");
  HIPCHK(h, hipGetLastError());
  return SCANN_OK;
}

// ---- the 128-wide backward: a stream plan, a context, stages; backward_impl below them reads as the order of stages and hand-offs ----

namespace {

// The streams of one backward and every hand-off between them: the only code of the backward that records an event or makes a stream
// wait for one (a launch_* given a `done` event records it by the kernel's own completion signal).
// Weight-gradient GEMMs are off the critical path (only the final reduce needs them): with the kept-activation forward their operands
// are never overwritten inside a layer, so they run on a side stream beside the data-gradient chain, which alone does not fill the
// chip at batch 128; the second side stream takes the layers' reductions and the basis leaf.
// One stream (the data-gradient mode, or a handle without side streams) is ONE state: side and side2 are null, every hand-off returns
// the main stream, next_ev() null, and nothing is recorded or waited for.
struct BwdStreams {
  hipStream_t main, side = nullptr, side2 = nullptr;

  BwdStreams(const scann_handle* h, bool single) : main(h->streams[0]), ring(h->train_ev) {
    if (!single && h->train_aux) side = h->train_aux, side2 = h->train_aux2;
  }
  // the next event of the ring: for a producer launched with it as its own completion signal (launch_atom_gather3 /
  // launch_attn_edge_bwd, `done`), so that after_event() needs no marker packet behind the producer on its stream -- 4.0 instead of
  // 6.7 us per hand-off (tools/fork_probe.hip, mode 3 vs 0)
  hipEvent_t next_ev() { return side ? ring[ev_i++ % ring.size()] : nullptr; }
  // `to` waits for everything on `from` so far; returns where to launch: `to`, or `from` where there is no `to`.  From the main stream
  // this costs it ~7 us (tools/fork_probe.hip)
  hipStream_t after(hipStream_t from, hipStream_t to) {
    if (!side) return main;
    if (!to) return from;
    wait_all(from, to);
    side2_given = side2_given || to == side2;
    return to;
  }
  // `to` waits for the completion event `e` of one launch
  hipStream_t after_event(hipEvent_t e, hipStream_t to) {
    if (!side || !to) return main;
    (void)hipStreamWaitEvent(to, e, 0);
    return to;
  }
  // the stream of the basis leaf: the second side stream behind `produced`, the completion event of the kernel that wrote the leaf's
  // input (null: behind everything on the main stream so far); leaf_done() marks the leaf's end there for the closing join
  hipStream_t leaf(hipEvent_t produced) {
    if (!side2) return main;
    if (produced) return after_event(produced, side2);
    wait_all(main, side2);
    return side2;
  }
  void leaf_done(hipStream_t ls) {
    if (ls == main) return;
    leaf_ev = next_ev();
    (void)hipEventRecord(leaf_ev, ls);
  }
  // the closing join: the main stream waits for the side stream, and for the second one by what it was given -- everything after()
  // handed it (the leaf, earlier on that stream, included), or else the leaf alone
  void join_all() {
    if (!side) return;
    wait_all(side, main);
    if (side2_given) wait_all(side2, main);
    else if (leaf_ev) (void)hipStreamWaitEvent(main, leaf_ev, 0);
  }

 private:
  void wait_all(hipStream_t from, hipStream_t to) {
    hipEvent_t e = next_ev();
    (void)hipEventRecord(e, from);
    (void)hipStreamWaitEvent(to, e, 0);
  }
  const std::vector<hipEvent_t>& ring;  // fork / join events of the handle
  size_t ev_i = 0;
  bool side2_given = false;
  hipEvent_t leaf_ev = nullptr;
};

// projections of layer l + 1 that still have to be added to dC (d loss / d centres_{l+1}): folded into the next rn_bwd_kernel, or
// launched by flush() where nobody folds them in
struct Pend {
  int n = 0;
  const float* X[3];
  const _Float16* Wh[3];
  const float* W[3];
  bool fresh = false;  // dC holds nothing yet: the terms ARE d loss / d centres (first use: dpreA.Wa^T of the readout)
  void add(const float* x, const _Float16* wh, const float* w) {
    X[n] = x; Wh[n] = wh; W[n] = w;
    ++n;
  }
  void fold_into(RnBwdArgs& ra, const float* dC) {
    ra.dC = fresh ? nullptr : dC;
    ra.n_pre = n;
    for (int t = 0; t < n; ++t) { ra.X[t] = X[t]; ra.Wh[t] = Wh[t]; }
    n = 0;
    fresh = false;
  }
  void flush(float* dC, int rows, hipStream_t s) {
    if (n)
      launch_linear_sum(X[0], W[0], n > 1 ? X[1] : nullptr, n > 1 ? W[1] : nullptr, n > 2 ? X[2] : nullptr, n > 2 ? W[2] : nullptr, dC, rows,
                        fresh ? 0 : 1, s);
    n = 0;
    fresh = false;
  }
};

// The operands of a layer's weight gradients exist once per layer (set L = the readout): the gradient launch of layer l runs on the
// side stream beside the data-gradient chains of the layers below and nothing it reads is overwritten before the end of the step.
struct BwdOperands {
  float *t3, *t4, *dQ, *dP1, *dP3;  // [A,128]
  float *edK, *eU;                  // [E,128]
};

// What the stages of one backward share.  ig non-null: the data-gradient mode (InGrad).
struct Bwd {
  scann_handle_t* const h;
  scann_dbatch_t* const db;
  scann_train_ws& w;
  const InGrad* const ig;
  const scann_config_t& c;
  const int L, A, E, B;
  const size_t nA, nE;
  float* const G;   // the gradient vector the parameter gradients go to
  const bool fused;  // fused chains (scann_train_fused.hip); SCANN_TRAIN_FUSED=0 selects the modular one-kernel-per-operation backward
  // On the forward's 32-row tile plan (whole atoms per tile, every degree <= 16) the softmax / LayerNorm backward of a tile's atoms
  // runs at the head of the tile's edge_bwd workgroup: one launch less per layer.
  const bool fuse_attn;
  BwdStreams st;
  WgradCtx wg;             // weight-gradient jobs and partial slots (w.wpart)
  WgradCtx dct;            // deterministic mode: slots of the six reductions that otherwise end in float atomics (scann_train.h)
  WgradCtx* det = nullptr;
  // named temporaries
  float *dC, *dCtx;                  // [A,128] d loss / d centres leaving / d context of the layer at hand
  float *edAng, *eT, *edGa, *edGb;   // [E,128]
  Pend pend;
  const float* dG_in = nullptr;  // gradient w.r.t. the geometry leaving layer l (none for the last layer)
  hipStream_t tail_s;            // where the embedding chain goes
  bool basis_done = false;
  // which stages run and which jobs are queued (scann_train_plan.h): the handle's under scann_set_lr_scale; the data-gradient mode
  // ignores the scale and runs everything
  const TrainPlan plan;

  Bwd(scann_handle_t* h, scann_dbatch_t* db, scann_train_ws& w, const InGrad* ig)
      : h(h), db(db), w(w), ig(ig), c(h->cfg), L(c.n_attention), A(db->n_atom), E(db->n_edge), B(db->n_struct),
        nA((size_t)A * D), nE((size_t)E * D), G(ig ? h->ig_grad : h->t_grad), fused(h->train_fused),
        fuse_attn(fused && c.g_update && db->tile_rows == 32 && db->n_big == 0 && db->max_degree <= 16 && E > 0),
        st(h, ig != nullptr), dC(w.tA[0]), dCtx(w.tA[1]), edAng(w.tE[0]), eT(w.tE[1]), edGa(w.tE[2]), edGb(w.tE[3]),
        tail_s(st.main), plan(ig || h->lr_scale.empty() ? train_plan(c.n_attention, {}, nullptr) : h->plan) {
    wg.arena = w.wpart;
    wg.cap = w.wpart_floats;
  }
  float* g(const std::string& name) const { return G + spec_offset(h, name); }
  // the stage functions mark the stage they enter (scann_train_stages); the data-gradient mode leaves the training state alone
  void enter(int stage) const {
    if (!ig && stage >= 0 && stage < 64) h->stages_ran |= (uint64_t)1 << stage;
  }
  int tensor_at(const float* p) const {  // the tensor a gradient pointer lies in (spec_off ascends)
    const int64_t off = p - G;
    return (int)(std::upper_bound(h->spec_off.begin(), h->spec_off.end(), off) - h->spec_off.begin()) - 1;
  }
  // a weight gradient's GEMM job (none in the data-gradient mode, none whose kernel and bias are both frozen)
  void wadd(const float* X, const float* dY, float* dW, float* db, int rows, const int32_t* nb = nullptr, const float* X2 = nullptr) {
    if (ig) return;
    if (!plan.live.empty() && !plan.keep_job(tensor_at(dW), db ? tensor_at(db) : -1)) return;
    wgrad_add(wg, X, dY, dW, db, rows, nb, X2);
  }
  BwdOperands operands(int l) const {
    float* const* a = &w.tA[5 + 5 * (size_t)l];
    float* const* e = &w.tE[4 + 2 * (size_t)l];
    return BwdOperands{a[0], a[1], a[2], a[3], a[4], e[0], e[1]};
  }
};

// layer l: its parameters, its operand set and the tensors the training forward kept (nothing is recomputed)
struct BwdLayer : BwdOperands {
  const int l;
  const LayerParams& p;
  const scann_handle::LayerT& pt;
  const std::string la, rn;
  const float *c_in, *ctx;      // centres entering LocalAttention l; its output (after layer_norm)
  const float *Gin, *Gout;      // geometry entering / leaving layer l (= layer_norm_g output); null on the base branch
  const float *qL, *KL, *VL;    // q [A,128]; K, V (base branch: geomL) [E,128]
  const float *angL, *TL;       // [E,128]; null: formed again from c[j] and G' / from V and G
  BwdLayer(const Bwd& b, int l_)
      : BwdOperands(b.operands(l_)), l(l_), p(b.h->layers[l_]), pt(b.h->layersT[l_]), la("local_attention_" + std::to_string(l_) + "/"),
        rn("residual_norm_" + std::to_string(l_) + "/"), c_in(b.db->dbg_c + (size_t)l_ * b.nA), ctx(b.db->dbg_ctx + (size_t)l_ * b.nA),
        Gin(b.c.g_update ? b.db->dbg_g + (size_t)l_ * b.nE : nullptr), Gout(b.c.g_update ? b.db->dbg_g + (size_t)(l_ + 1) * b.nE : nullptr),
        qL(b.db->keep_q + (size_t)l_ * b.nA), KL(b.db->keep_K + (size_t)l_ * b.nE), VL(b.db->keep_V + (size_t)l_ * b.nE),
        angL(b.db->keep_ang ? b.db->keep_ang + (size_t)l_ * b.nE : nullptr), TL(b.db->keep_T ? b.db->keep_T + (size_t)l_ * b.nE : nullptr) {}
};

// deterministic mode: the slots are allocated with the batch's workspace on the first such backward and sized from the batch shape alone
int bwd_det_arena(Bwd& b) {
  if (!b.h->deterministic || b.ig) return SCANN_OK;
  scann_handle_t* h = b.h;
  scann_train_ws& w = b.w;
  const scann_config_t& c = b.c;
  const bool general = c.use_ring || c.feature_cgcnn;
  const size_t need = det_slot_floats(b.A, b.E, b.L, c.n_atoms, c.embedding_dim, c.g_update, general, c.feature_cgcnn, c.use_ring);
  if (need > w.det_floats) {
    // (the slots of a previous step on this batch may still be read by its reductions: the stream order of the main stream
    //  alone does not cover the side streams, so wait for the device before the block goes back to the cache)
    if (w.det_part) {
      HIPCHK(h, hipDeviceSynchronize());
      cached_free(w.det_part);
      w.det_part = nullptr;
      w.det_floats = 0;
    }
    HIPCHK(h, cached_malloc((void**)&w.det_part, need * 4));
    w.det_floats = need;
  }
  b.dct.arena = w.det_part;
  b.dct.cap = w.det_floats;
  b.det = &b.dct;
  return SCANN_OK;
}

// ---- readout (scann_model.py:424-447, attention.py:267-318): "layer L" of the operand-set scheme ----
void bwd_readout(Bwd& b) {
  scann_handle_t* h = b.h;
  scann_dbatch_t* db = b.db;
  hipStream_t s = b.st.main;
  const BwdOperands o = b.operands(b.L);
  float *const dgq = b.w.tA[4], *const dgk = o.t3, *const dpreA = o.dQ;
  // the training forward kept preA = cL.Wa + ba and z = swish(preA); gq, gk, ga, y are still in the batch workspace
  const float *preA = db->keep_preA, *z = db->keep_z;
  const float* cL = db->dbg_c + (size_t)b.L * b.nA;  // centres entering after_Lc
  ReadoutBwdArgs ra{};
  ra.mol_offset = db->mol_offset; ra.n_struct = b.B; ra.max_atoms = db->max_atoms; ra.use_ga_norm = b.c.use_ga_norm;
  ra.gq = db->gq; ra.gk = db->gk; ra.ga = db->ga; ra.dy = b.w.dy;
  ra.Wb = h->head.Wb; ra.bb = h->head.bb; ra.wo = h->head.wo;
  ra.dgq = dgq; ra.dgk = dgk; ra.rep_out = b.w.rep; ra.dpre_out = b.w.dpre;
  // (one slot per structure, summed in structure order with the layer's other vectors: 128 workgroups adding to the same 128
  // addresses was a queue of 16 k atomics)
  ra.dwo = reserve_vec(b.wg, b.g("predict_property/kernel"), b.B); ra.dbo = b.g("predict_property/bias");
  b.enter(b.L + 2);
  if (!b.wg.overrun) launch_readout_bwd(ra, s, b.det != nullptr);
  if (!b.plan.readout_body()) {  // floor at the property head: what bf_property and predict_property need, and no more
    b.wadd(b.w.rep, b.w.dpre, b.g("bf_property/kernel"), b.g("bf_property/bias"), b.B);
    return;
  }
  b.enter(b.L + 1);
  // the readout's four weight gradients ride with the first layer's launch on the side stream (their operands -- rep, dpre, z, dgq,
  // dgk and dpreA in the readout's operand set -- are not written again before the end of the step): no hand-off of their own,
  // each of which costs the main stream ~7 us (tools/fork_probe.hip)
  b.wadd(b.w.rep, b.w.dpre, b.g("bf_property/kernel"), b.g("bf_property/bias"), b.B);
  b.wadd(z, dgq, b.g("global_attention/query/kernel"), b.g("global_attention/query/bias"), b.A);
  b.wadd(z, dgk, b.g("global_attention/key/kernel"), b.g("global_attention/key/bias"), b.A);
  launch_linear_sum(dgq, h->WgqT, dgk, h->WgkT, nullptr, nullptr, dpreA, b.A, 0, s, preA);  // dpreA = (dgq.Wgq^T + dgk.Wgk^T) * swish'(preA)
  b.wadd(cL, dpreA, b.g("after_Lc/kernel"), b.g("after_Lc/bias"), b.A);
  // d loss / d centres_L = dpreA.Wa^T: folded into the first rn_bwd_kernel (or launched by Pend::flush)
  b.pend.add(dpreA, h->WaTh, h->WaT);
  b.pend.fresh = true;
}

// ---- ResidualNorm backward (attention.py:37-40): c_{l+1} = LN(x + drop(W2 swish(W1 x + b1) + b2)), x = ctx ----
int bwd_residual_norm(Bwd& b, const BwdLayer& y) {
  scann_handle_t* h = b.h;
  hipStream_t s = b.st.main;
  b.enter(y.l + 1);
  if (!(b.fused && b.c.use_attn_norm)) b.pend.flush(b.dC, b.A, s);  // nobody below folds the projections of the layer above in
  if (!b.c.use_attn_norm) {
    HIPCHK(h, hipMemcpyAsync(b.dCtx, b.dC, b.nA * 4, hipMemcpyDeviceToDevice, s));
    return SCANN_OK;
  }
  const float* pre1 = b.db->keep_pre1 + (size_t)y.l * b.nA;
  const float* H1 = b.db->keep_H1 + (size_t)y.l * b.nA;
  const float* T2 = b.db->keep_T2 + (size_t)y.l * b.nA;
  if (b.fused) {
    // one kernel: [dC += the projections of the layer above] -> LayerNorm backward -> Dropout mask -> dense_2^T, swish' -> dense_1^T
    RnBwdArgs ra{};
    b.pend.fold_into(ra, b.dC);
    ra.T2 = T2; ra.pre1 = pre1; ra.gamma = y.p.lnr_g; ra.Wf2Th = y.pt.Wf2Th; ra.Wf1Th = y.pt.Wf1Th;
    ra.dY = y.t3; ra.dpre1 = y.t4; ra.dCtx = b.dCtx; ra.n_atom = b.A;
    ra.drop_p = b.w.drop_p; ra.drop_seed = b.w.seed; ra.drop_tag = (unsigned)y.l;
    launch_rn_bwd(b.wg, ra, b.g(y.rn + "layer_norm/gamma"), b.g(y.rn + "layer_norm/beta"), s);
  } else {
    launch_ln_bwd(b.wg, T2, y.p.lnr_g, b.dC, b.dCtx, b.g(y.rn + "layer_norm/gamma"), b.g(y.rn + "layer_norm/beta"), b.A, 0, s);  // dT2 -> dCtx
    // gradient of the Dense_2 output = dT2 through the Dropout mask, in a buffer of its own: dT2 (dCtx) is the residual path and
    // is accumulated into below, while the queued weight gradient reads its operand at the end of the layer
    if (b.w.drop_p > 0.f) launch_dropout_copy(y.t3, b.dCtx, b.nA, b.w.seed, (unsigned)y.l, b.w.drop_p, s);
    else HIPCHK(h, hipMemcpyAsync(y.t3, b.dCtx, b.nA * 4, hipMemcpyDeviceToDevice, s));
    launch_linear(y.t3, y.pt.Wf2T, nullptr, y.t4, const_cast<float*>(pre1), b.A, 4, s);  // dpre1 = (dY.W2^T) * swish'(pre1)
    launch_linear(y.t4, y.pt.Wf1T, nullptr, b.dCtx, nullptr, b.A, 1, s);                 // dctx = dT2 + dpre1.W1^T
  }
  b.wadd(H1, y.t3, b.g(y.rn + "dense_2/kernel"), b.g(y.rn + "dense_2/bias"), b.A);
  b.wadd(y.ctx, y.t4, b.g(y.rn + "dense_1/kernel"), b.g(y.rn + "dense_1/bias"), b.A);
  return SCANN_OK;
}

// ---- LocalAttention backward (attention.py:118-216): softmax / LayerNorm backward per atom (unless it rides in the edge launch of
// bwd_geometry), and the key / query weight-gradient jobs ----
void bwd_attention(Bwd& b, const BwdLayer& y) {
  b.enter(y.l + 1);
  if (!b.fuse_attn)
    launch_attn_bwd(b.wg, y.qL, y.KL, b.db->edge_offset, b.dCtx, y.p.ln_g, y.dQ, y.edK, b.g(y.la + "layer_norm/gamma"),
                    b.g(y.la + "layer_norm/beta"), b.A, b.db->max_degree, b.w.attn_p, DROP_TAG_ATTN + (unsigned)y.l, b.w.seed, b.st.main);
  if (y.angL) b.wadd(y.angL, y.edK, b.g(y.la + "key/kernel"), b.g(y.la + "key/bias"), b.E);
  else b.wadd(y.c_in, y.edK, b.g(y.la + "key/kernel"), b.g(y.la + "key/bias"), b.E, b.db->edge_col, y.Gout);  // ang = c[j] * G'
  b.wadd(y.c_in, y.dQ, b.g(y.la + "query/kernel"), b.g(y.la + "query/bias"), b.A);
}

// The fixed-order sums of a layer's partial slots (and of its LayerNorm gamma / beta slots) behind its gradient launch on `ws`.
// The side stream's chain per layer is a gradient launch (~32 us) and two reductions of its partial slots (~34 us): as long as the
// main stream's chain per layer (~70 us), so the step ended when the SIDE stream did, ~65 us after the main one.  The reductions go
// to the second side stream (idle but for the basis leaf): gradient launch of layer l - 1 beside the reductions of layer l.
// (the LAST layer's reductions stay behind their gradient launch: the second side stream is busy with the basis leaf, 46 us, by then)
void bwd_reduce(Bwd& b, hipStream_t ws, bool last) { wgrad_flush(b.wg, last ? ws : b.st.after(ws, b.st.side2)); }

// ---- LocalAttention, base branch (attention.py:155): geomL = swish(gd.Wf + bf) * weight from the raw basis (kept in the V slices),
// no geometry threading; its leaf is filter_geo ----
void bwd_base_branch(Bwd& b, const BwdLayer& y) {
  scann_dbatch_t* db = b.db;
  hipStream_t s = b.st.main;
  b.enter(y.l + 1);
  launch_linear(y.edK, y.pt.WkT, nullptr, b.edAng, nullptr, b.E, 0, s);            // dang
  launch_edge_dang(y.c_in, db->edge_col, y.VL, b.edAng, nullptr, b.eT, y.eU, b.E, s);  // eT = dang * geomL ; eU = dgeomL = dang * c[j]
  // dC[j] = sum over the edges that point at j (at the floor nothing below reads it)
  if (b.plan.feeds_below(y.l)) launch_gather_sum(b.eT, db->in_off, db->in_edge, b.dC, b.A, 0, s);
  if (b.ig) {
    launch_base_input_grad(db->dist, db->weight, y.eU, y.p.Wfg, y.p.bfg, b.h->cd, b.E, D, b.ig->d_dist, b.ig->d_weight, s);
  } else {
    // the layer's weight gradients, their reduction and the filter_geo leaf beside the chain of the layers below
    hipStream_t ws = b.st.after(s, b.st.side);
    wgrad_launch(b.wg, ws);
    bwd_reduce(b, ws, y.l == b.plan.lowest_layer());
    launch_base_geom_bwd(db->gd, y.p.Wfg, y.p.bfg, db->weight, y.eU, b.E, b.g(y.la + "filter_geo/kernel"), b.g(y.la + "filter_geo/bias"), ws,
                         b.det);
  }
  b.pend.add(y.dQ, y.pt.WqTh, y.pt.WqT);  // dC += dq.Wq^T: folded into the next rn_bwd_kernel (or launched by Pend::flush)
}

// ---- basis MLP (scann_model.py:378-389): a leaf (parameter gradients, or d y / d (dist, weight)) on a stream of its own, started as
// soon as the geometry gradient entering layer 0 exists -- at 45 us it is the longest thing between there and the optimiser ----
void bwd_basis_leaf(Bwd& b, const float* dG, hipEvent_t produced) {  // `produced`: completion event of the kernel that wrote dG, or null
  scann_handle_t* h = b.h;
  scann_dbatch_t* db = b.db;
  hipStream_t bs = b.st.leaf(produced);
  b.enter(0);
  if (b.ig)
    launch_basis_input_grad(db->dist, db->weight, dG, h->basis.Wd, h->basis.bd, h->basis.Ww, h->basis.bw, h->basis.cd, h->basis.cw, b.E, D,
                            b.ig->d_dist, b.ig->d_weight, bs);
  else
    launch_basis_bwd(h->basis, db->dist, db->weight, dG, b.E, b.g("neighbor_d/kernel"), b.g("neighbor_d/bias"), b.g("neighbor_w/kernel"),
                     b.g("neighbor_w/bias"), bs, b.det);
  b.st.leaf_done(bs);
  b.basis_done = true;
}

// ---- LocalAttention with geometry update: G' = LN_g(swish(V) + G), V = G.W2 + P1[i] + P3[j]; gate ang = c[j] * G' ----
// Returns the completion event of the launch that wrote the last operands of the layer's weight gradients (null: none was made).
hipEvent_t bwd_geometry(Bwd& b, const BwdLayer& y) {
  scann_dbatch_t* db = b.db;
  hipStream_t s = b.st.main;
  float* dGnext = (b.dG_in == b.edGa) ? b.edGb : b.edGa;  // d loss / d geometry entering layer l
  hipEvent_t ev_sums = nullptr;
  const bool leaf = y.l == 0 && b.plan.leaves();  // the basis leaf is started from in here
  b.enter(y.l + 1);
  if (b.fused) {
    // one kernel: dang = dK.Wk^T -> dG'tot = dang * c[j] + dG'(next layer) -> LayerNorm_g backward -> dV = dT * swish'(V) -> dG = dT + dV.W2^T
    EdgeBwdArgs ea{};
    ea.dK = y.edK; ea.c = y.c_in; ea.dG_in = b.dG_in; ea.T = y.TL; ea.G = y.Gin; ea.V = y.VL; ea.gamma = y.p.lng_g; ea.nb = db->edge_col;
    ea.WkTh = y.pt.WkTh; ea.W2Th = y.pt.W2Th; ea.dang = b.edAng; ea.dV = y.eU; ea.dG = dGnext; ea.n_edge = b.E;
    hipEvent_t ev_dg = nullptr;  // layer 0: the basis leaf waits for the geometry gradient this launch leaves
    if (b.fuse_attn) {
      AttnPart ab{};
      ab.q = y.qL; ab.K = y.KL; ab.dctx = b.dCtx; ab.gamma = y.p.ln_g; ab.edge_offset = db->edge_offset; ab.tiles = db->tiles;
      ab.dq = y.dQ; ab.dK = y.edK; ab.drop_p = b.w.attn_p; ab.drop_tag = DROP_TAG_ATTN + (unsigned)y.l; ab.drop_seed = b.w.seed;
      if (leaf && b.st.side2) ev_dg = b.st.next_ev();
      launch_attn_edge_bwd(b.wg, ea, ab, db->n_tile, b.g(y.la + "layer_norm_g/gamma"), b.g(y.la + "layer_norm_g/beta"),
                           b.g(y.la + "layer_norm/gamma"), b.g(y.la + "layer_norm/beta"), s, ev_dg);
    } else {
      launch_edge_bwd(b.wg, ea, b.g(y.la + "layer_norm_g/gamma"), b.g(y.la + "layer_norm_g/beta"), s);
    }
    if (leaf) bwd_basis_leaf(b, dGnext, ev_dg);  // (before the atom sums below: they do not touch the geometry gradient)
    // dC[j] = sum over the edges that point at j of dang * G' (gate), dP3[j] = the same sum of dV, dP1[i] = sum of dV over i's own edges
    ev_sums = b.st.next_ev();  // ... and this launch's completion is what the layer's weight-gradient launch on the side stream waits for
    launch_atom_gather3(b.edAng, y.Gout, y.eU, db->edge_offset, db->in_off, db->in_edge, b.dC, y.dP1, y.dP3, b.A, s, ev_sums);
  } else {
    launch_linear(y.edK, y.pt.WkT, nullptr, b.edAng, nullptr, b.E, 0, s);  // dang
    if (b.plan.feeds_below(y.l)) launch_gather_prod_sum(b.edAng, y.Gout, db->in_off, db->in_edge, b.dC, b.A, 0, s);  // (at the floor nothing reads dC)
    // LayerNorm_g backward with its neighbours fused: in  dG'tot = dang * c[j] + dG'(next layer), out  dT (residual path, -> dGnext)
    // and dV = dT * swish'(V) (-> eU)
    launch_ln_bwd_edge(b.wg, y.TL, y.p.lng_g, b.edAng, y.c_in, db->edge_col, b.dG_in, y.VL, dGnext, y.eU, b.g(y.la + "layer_norm_g/gamma"),
                       b.g(y.la + "layer_norm_g/beta"), b.E, s);
    launch_atom_sums(y.eU, db->edge_offset, db->in_off, db->in_edge, y.dP1, y.dP3, b.A, s);  // dP1[i]: the atom's own edges; dP3[j]: the edges that point at j
    if (b.plan.feeds_below(y.l)) launch_linear(y.eU, y.pt.W2T, nullptr, dGnext, nullptr, b.E, 1, s);  // dG += dV.W2^T
  }
  float* fgk = b.g(y.la + "filter_geo/kernel");
  b.wadd(y.Gin, y.eU, fgk + (size_t)D * D, nullptr, b.E);  // dW2
  b.wadd(y.c_in, y.dP1, fgk, b.g(y.la + "filter_geo/bias"), b.A);
  b.wadd(y.c_in, y.dP3, fgk + (size_t)2 * D * D, nullptr, b.A);
  // dC += dP1.W1^T + dP3.W3^T + dq.Wq^T: folded into the next layer's rn_bwd_kernel (or launched by Pend::flush)
  b.pend.add(y.dP1, y.pt.W1Th, y.pt.W1T);
  b.pend.add(y.dP3, y.pt.W3Th, y.pt.W3T);
  b.pend.add(y.dQ, y.pt.WqTh, y.pt.WqT);
  b.dG_in = dGnext;
  return ev_sums;
}

// ---- every weight gradient of the layer (ResidualNorm 2, key, query, filter_geo 3) in ONE launch, then the fixed-order sum of its
// partial slots: both beside the chains of the layers below.  `ev_sums`: bwd_geometry's ----
// (a hand-off per layer: 2 / 3 / 4 / 7 layers sharing one measured slower, profiles/r04_notes.md)
void bwd_layer_wgrad(Bwd& b, int l, hipEvent_t ev_sums) {
  if (b.ig) return;  // (no weight gradients)
  if (l == 0 && ev_sums) {
    // The FIRST layer's gradient launch and its reductions are the longest thing left (the main stream only has the embedding chain,
    // ~40 us): they stay on the main stream, with no hand-over in front of them, and the embedding chain goes to the side stream
    // instead (0.830 -> 0.819 ms per step, eight alternations on one box: profiles/r05_notes.md)
    wgrad_launch(b.wg, b.st.main);
    wgrad_flush(b.wg, b.st.main);
    b.tail_s = b.st.after_event(ev_sums, b.st.side);
    return;
  }
  hipStream_t ws = ev_sums ? b.st.after_event(ev_sums, b.st.side) : b.st.after(b.st.main, b.st.side);
  wgrad_launch(b.wg, ws);
  bwd_reduce(b, ws, l == b.plan.lowest_layer());
}

// ---- embedding (scann_model.py:362-374): the weight gradients of the table / dense_embed (general: ring, cgcnn), or in the
// data-gradient mode d y / d (ring, cgcnn) from d y / d centres after dense_embed (no Dropout: inference semantics) ----
void bwd_embed_leaf(Bwd& b) {
  scann_handle_t* h = b.h;
  scann_dbatch_t* db = b.db;
  const scann_config_t& c = b.c;
  hipStream_t s = b.tail_s;
  b.enter(0);
  if (b.ig) {
    if (!b.ig->d_ring && !b.ig->d_cgcnn) return;
    InputGradEmbed e{};
    const EmbedArgs& ea = h->embed;
    e.width = D; e.emb_dim = c.embedding_dim; e.dC = b.dC; e.atomic = db->atomic;
    e.cgcnn = c.feature_cgcnn ? db->cgcnn : nullptr;
    e.ring = c.use_ring ? db->ring : nullptr;
    e.emb = ea.emb; e.We = ea.We; e.be = ea.be; e.Wr = ea.Wr; e.br = ea.br; e.Wde = ea.Wde; e.bde = ea.bde;
    e.d_ring = b.ig->d_ring; e.d_cgcnn = b.ig->d_cgcnn;
    launch_embed_input_grad(e, b.A, s);
    return;
  }
  // deterministic mode: the readout's bias gradient = the sum of d loss / d y, in structure order, beside the embedding chain
  if (b.det) launch_scalar_sum(b.w.dy, b.B, b.g("predict_property/bias"), s);
  if (c.use_ring || c.feature_cgcnn) {
    launch_dropout(b.dC, b.nA, b.w.seed, DROP_TAG_EMBED, b.w.drop_p, s);
    EmbedArgs e = h->embed;
    e.n_atom = b.A; e.atomic = db->atomic; e.c0 = db->c0;
    e.ring = c.use_ring ? db->ring : nullptr;
    e.cgcnn = c.feature_cgcnn ? db->cgcnn : nullptr;
    launch_embed_general_bwd(e, b.dC, c.feature_cgcnn ? nullptr : b.g("embed_atom/embeddings"),
                             c.feature_cgcnn ? b.g("embed_atom/kernel") : nullptr, c.feature_cgcnn ? b.g("embed_atom/bias") : nullptr,
                             c.use_ring ? b.g("extra_embed/kernel") : nullptr, c.use_ring ? b.g("extra_embed/bias") : nullptr,
                             b.g("dense_embed/kernel"), b.g("dense_embed/bias"), s, b.det, c.n_atoms);
  } else {
    launch_embed_bwd(b.dC, db->atomic, b.A, h->d_weights + h->o_emb, h->d_weights + h->o_Wde, h->d_weights + h->o_bde, b.w.dlut,
                     c.n_atoms, c.embedding_dim, b.g("embed_atom/embeddings"), b.g("dense_embed/kernel"), b.g("dense_embed/bias"), b.w.seed,
                     DROP_TAG_EMBED, b.w.drop_p, s, b.det);
  }
}

}  // namespace

// d_stat (device, {global sse, global count}) non-null: the loss scale is formed on the device (scann_train_step: no host round trip)
// ig non-null: the data-gradient mode (InGrad; scann_input_grads): one stream, no weight-gradient launch or reduction, no deterministic
// slots; what the fused kernels store per workgroup for the LayerNorm gradients stays in the partial arena, the readout's bias
// gradient goes to h->ig_grad, and the input leaves replace the basis / filter_geo / embedding weight-gradient leaves.
static int backward_impl(scann_handle_t* h, scann_dbatch_t* db, scann_train_ws& w, float scale, const double* d_stat, bool dy_done,
                         const InGrad* ig = nullptr) {
  if (const int r = ensure_reverse(h, db)) return r;
  if (h->generic) {  // the plain-fp32 backward is not cut at the floor: it enters every stage, and says so
    if (!ig) h->stages_ran = train_plan(h->cfg.n_attention, {}, nullptr).stage_bits();
    return gen_backward(h, db, w, scale, d_stat, dy_done, ig);
  }
  Bwd b(h, db, w, ig);
  hipStream_t s = b.st.main;
  if (!ig) h->stages_ran = 0;
  if (!dy_done) launch_dy(db->y, w.targets, b.B, scale, d_stat, w.dy, s);
  if (const int r = bwd_det_arena(b)) return r;
  bwd_readout(b);  // its weight gradients ride with the first layer's launch
  for (int l = b.L - 1; l >= b.plan.lowest_layer(); --l) {  // the layers at and above the floor
    const BwdLayer y(b, l);
    if (const int r = bwd_residual_norm(b, y)) return r;
    bwd_attention(b, y);
    if (!b.c.g_update) {
      bwd_base_branch(b, y);  // with its gradient launch, reductions and filter_geo leaf on the side streams
      continue;
    }
    const hipEvent_t ev_sums = bwd_geometry(b, y);  // (layer 0, fused: the basis leaf goes to the second side stream from in here)
    bwd_layer_wgrad(b, l, ev_sums);                 // side stream; layer 0: main stream, and the embedding chain to the side stream
  }
  // (the basis leaf first: it needs only the geometry gradient the last edge backward left, and at 43 us on its own stream it is
  // the longest thing between here and the optimiser -- started behind the embedding chain it ended 30 us after it)
  if (b.plan.leaves()) {
    if (b.dG_in && !b.basis_done) bwd_basis_leaf(b, b.dG_in, nullptr);
    b.pend.flush(b.dC, b.A, b.tail_s);
    bwd_embed_leaf(b);
  } else if (b.det) {
    // (deterministic mode sums the readout's bias gradient beside the embedding chain: without that chain, here)
    launch_scalar_sum(b.w.dy, b.B, b.g("predict_property/bias"), s);
  }
  if (b.det && b.dct.overrun) return fail(h, SCANN_ERR_HIP, "scann_train_backward: deterministic partial arena overrun");
  if (b.wg.overrun) return fail(h, SCANN_ERR_HIP, "scann_train_backward: weight-gradient partial arena overrun");
  if (!ig) {
    // a model without LocalAttention layers, or a floor above them: the readout's gradients were never launched
    if (!b.wg.jobs.empty()) wgrad_launch(b.wg, s);
    b.st.join_all();
    wgrad_flush(b.wg, s);  // ONE launch adds the per-slab partials of every weight gradient, in slab order
  }
  HIPCHK(h, hipGetLastError());
  return SCANN_OK;
}

static int adam_impl(scann_handle_t* h, float lr_t, float beta1, float beta2, float eps, float l2, int zero_g) {
  hipStream_t s = h->streams[0];
  h->t_step += 1;
  const double t = (double)h->t_step;
  const float lr_hat = (float)((double)lr_t * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
  const size_t n = h->host_master.size();
  // t_l2 holds a 0/1 mask; fold the coefficient in by scaling through the kernel argument
  if (h->lr_scale.empty()) launch_adam(h->t_master, h->t_grad, h->t_m, h->t_v, h->t_l2, n, lr_hat, beta1, beta2, eps, l2, zero_g, s);
  else launch_adam_scaled(h->t_master, h->t_grad, h->t_m, h->t_v, h->t_l2, h->t_lrs, n, lr_hat, beta1, beta2, eps, l2, zero_g, s);
  if (h->generic) {  // the plain kernels read the Keras tensors as they are: the forward's copy is the master vector
    HIPCHK(h, hipMemcpyAsync(h->g_weights, h->t_master, n * 4, hipMemcpyDeviceToDevice, s));
    return SCANN_OK;
  }
  launch_repack(h->t_descs, (int)h->descs.size(), h->t_master, h->d_weights, h->range_flag, s);
  h->sp_dirty = true;
  if (!h->cfg.use_ring && !h->cfg.feature_cgcnn)
    launch_embed_lut(h->d_weights + h->o_emb, h->d_weights + h->o_Wde, h->d_weights + h->o_bde, h->cfg.n_atoms,
                     h->cfg.embedding_dim, h->d_weights + h->o_lut, s);
  HIPCHK(h, hipGetLastError());
  return SCANN_OK;
}

extern "C" {

int scann_train_begin(scann_handle_t* h) {
  if (!h) return SCANN_ERR_INVALID;
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_train_begin: weights not loaded");
  if (h->weights_exact)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_train_begin: " + h->exact_reason + "; the training kernels multiply in split-fp16 "
                                          "form only (inference of such a checkpoint runs on the exact-fp32 kernels)");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = h->host_master.size();
  if (!h->t_master) {
    HIPCHK(h, hipMalloc((void**)&h->t_master, n * 4));
    HIPCHK(h, hipMalloc((void**)&h->t_grad, n * 4));
    HIPCHK(h, hipMalloc((void**)&h->t_m, n * 4));
    HIPCHK(h, hipMalloc((void**)&h->t_v, n * 4));
    HIPCHK(h, hipMalloc((void**)&h->t_l2, n * 4));
    if (!h->generic) HIPCHK(h, hipMalloc((void**)&h->t_descs, h->descs.size() * sizeof(RepackDesc)));
  }
  HIPCHK(h, hipMemcpy(h->t_master, h->host_master.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemset(h->t_grad, 0, n * 4));
  HIPCHK(h, hipMemset(h->t_m, 0, n * 4));
  HIPCHK(h, hipMemset(h->t_v, 0, n * 4));
  if (!h->generic) HIPCHK(h, hipMemcpy(h->t_descs, h->descs.data(), h->descs.size() * sizeof(RepackDesc), hipMemcpyHostToDevice));
  // kernel_regularizer=l2(1e-4) mask: LocalAttention query/key/filter_geo, ResidualNorm dense_1/2, GlobalAttention
  // query/key, after_Lc, bf_property (attention.py:27-28,95-109,260-265; scann_model.py:428,441)
  std::vector<float> l2(n, 0.f);
  for (size_t i = 0; i < h->specs.size(); ++i) {
    const std::string& nm = h->specs[i].name;
    const bool is_kernel = nm.size() > 7 && nm.compare(nm.size() - 7, 7, "/kernel") == 0;
    const bool reg = is_kernel && (nm.find("local_attention_") == 0 || nm.find("residual_norm_") == 0 ||
                                   nm.find("global_attention/") == 0 || nm.find("after_Lc/") == 0 || nm.find("bf_property/") == 0);
    if (reg) std::fill(l2.begin() + h->spec_off[i], l2.begin() + h->spec_off[i] + h->specs[i].numel(), 1.0f);
  }
  HIPCHK(h, hipMemcpy(h->t_l2, l2.data(), n * 4, hipMemcpyHostToDevice));
  if (!h->lr_scale.empty())  // a scale set before this call survives it
    if (const int r = upload_lr_scale(h)) return r;
  if (h->generic) {
    if (const int r = build_gen_transposes(h)) return r;
  } else if (!h->train_aux) {
    // (side streams created with the lowest priority changed nothing: 0.895 vs 0.895 ms per step, profiles/r04_notes.md)
    // (and so did confining them to half / a quarter of the CUs with hipExtStreamCreateWithCUMask: 0.89-0.93 ms either way)
    // A handle with a second forward stream lends it to the backward pass as its side stream instead of creating a fifth stream: HIP
    // deals a process's streams onto 4 hardware queues, and the fifth shares one (training step 0.91-0.92 -> 0.88-0.89 ms with the
    // default two forward streams; validation forwards on that stream never overlap a step).
    if (h->nstream >= 2) {
      h->train_aux = h->streams[1];
      h->train_aux_borrowed = true;
    } else {
      HIPCHK(h, hipStreamCreateWithFlags(&h->train_aux, hipStreamNonBlocking));
    }
    HIPCHK(h, hipStreamCreateWithFlags(&h->train_aux2, hipStreamNonBlocking));
    h->train_ev.resize(128);
    // fork / join events between streams of ONE device: no system-scope fence (the kernels' own end-of-kernel release already makes
    // their results visible device-wide, and nothing the host or a DMA engine wrote is ordered by them)
    const unsigned ev_flags = hipEventDisableTiming | hipEventDisableSystemFence;
    for (hipEvent_t& e : h->train_ev) HIPCHK(h, hipEventCreateWithFlags(&e, ev_flags));
  }
  h->grads_zeroed = false;  // (re)allocated gradient vector: contents unknown
  h->step_begun = h->step_ended = 0;
  {
    const char* e = getenv("SCANN_TRAIN_FUSED");
    h->train_fused = !(e && e[0] == '0');
  }
  h->t_step = 0;
  return SCANN_OK;
}

int scann_set_attention_dropout(scann_handle_t* h, float p) {
  if (!h || !(p >= 0.f && p < 1.f)) return fail(h, SCANN_ERR_INVALID, "scann_set_attention_dropout: rate must be in [0, 1)");
  h->attn_drop_p = p;
  return SCANN_OK;
}

int scann_set_deterministic(scann_handle_t* h, int on) {
  if (!h) return SCANN_ERR_INVALID;
  h->deterministic = on != 0;  // read by each backward as it is enqueued (plain-fp32 handles: every sum is fixed-order already)
  return SCANN_OK;
}

int scann_tensor_stage(const char* name, int n_attention) { return tensor_stage(name, n_attention); }

int scann_set_lr_scale(scann_handle_t* h, const float* scale) {
  if (!h) return fail(h, SCANN_ERR_INVALID, "scann_set_lr_scale: h is null");
  if (h->step_begun != h->step_ended)
    return fail(h, SCANN_ERR_INVALID, "scann_set_lr_scale: a step is in flight (between scann_train_step_begin and its _end)");
  if (!scale) {  // all 1: the unscaled kernel and the whole backward
    h->lr_scale.clear();
    h->plan = TrainPlan{};
    return SCANN_OK;
  }
  const size_t nt = h->specs.size();
  bool any = false;
  for (size_t i = 0; i < nt; ++i) {
    if (!(scale[i] >= 0.f) || !std::isfinite(scale[i]))
      return fail(h, SCANN_ERR_INVALID, "scann_set_lr_scale: scale[" + std::to_string(i) + "] (" + h->specs[i].name + ") is negative or not finite");
    any = any || scale[i] > 0.f;
  }
  if (!any) return fail(h, SCANN_ERR_INVALID, "scann_set_lr_scale: every entry of scale is 0: nothing to train");
  std::vector<float> keep(scale, scale + nt);
  if (h->t_master) {  // in training mode: the per-element image now (scann_train_begin builds it otherwise)
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->streams[0]));  // an optimiser step enqueued earlier may still read the image
    h->lr_scale.swap(keep);
    const int r = upload_lr_scale(h);
    if (r) {
      h->lr_scale.swap(keep);
      return r;
    }
  } else {
    h->lr_scale.swap(keep);
  }
  std::vector<std::string> names;
  for (const WeightSpec& sp : h->specs) names.push_back(sp.name);
  h->plan = train_plan(h->cfg.n_attention, names, h->lr_scale.data());
  return SCANN_OK;
}

int scann_get_lr_scale(const scann_handle_t* h, float* out) {
  if (!h || !out) return fail(const_cast<scann_handle_t*>(h), SCANN_ERR_INVALID, h ? "scann_get_lr_scale: out is null" : "scann_get_lr_scale: h is null");
  for (size_t i = 0; i < h->specs.size(); ++i) out[i] = h->lr_scale.empty() ? 1.0f : h->lr_scale[i];
  return SCANN_OK;
}

int scann_train_stages(const scann_handle_t* h, uint64_t* ran) {
  if (!h || !ran) return fail(const_cast<scann_handle_t*>(h), SCANN_ERR_INVALID, h ? "scann_train_stages: ran is null" : "scann_train_stages: h is null");
  *ran = h->stages_ran;
  return SCANN_OK;
}

int scann_zero_grads(scann_handle_t* h) {
  if (!h || !h->t_grad) return fail(h, SCANN_ERR_INVALID, "scann_zero_grads: call scann_train_begin first");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(h->t_grad, 0, h->host_master.size() * 4, h->streams[0]));
  h->grads_zeroed = true;
  return SCANN_OK;
}

int scann_get_grads(scann_handle_t* h, float* out) {
  if (!h || !h->t_grad || !out) return fail(h, SCANN_ERR_INVALID, "scann_get_grads: no training state");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  HIPCHK(h, hipMemcpy(out, h->t_grad, h->host_master.size() * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

int scann_get_weights(scann_handle_t* h, float* out) {
  if (!h || !out) return SCANN_ERR_INVALID;
  if (!h->t_master) {
    memcpy(out, h->host_master.data(), h->host_master.size() * 4);
    return SCANN_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  HIPCHK(h, hipMemcpy(out, h->t_master, h->host_master.size() * 4, hipMemcpyDeviceToHost));
  memcpy(h->host_master.data(), out, h->host_master.size() * 4);
  return SCANN_OK;
}

int scann_train_forward(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, uint64_t seed, double* sse_out) {
  if (!h || !db || !targets || !sse_out) return fail(h, SCANN_ERR_INVALID, "scann_train_forward: null argument");
  if (!h->t_master) return fail(h, SCANN_ERR_INVALID, "scann_train_forward: call scann_train_begin first");
  HIPCHK(h, hipSetDevice(h->device));
  scann_train_ws* w = nullptr;
  const int r = train_forward_impl(h, db, targets, dropout, h->attn_drop_p, seed, &w, 2);
  if (r) return r;
  hipStream_t s = h->streams[0];
  HIPCHK(h, hipMemcpyAsync(sse_out, w->sse, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return check_range(h, "scann_train_forward");
}

int scann_train_backward(scann_handle_t* h, scann_dbatch_t* db, double sse_global, int64_t count_global) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_train_backward: null argument");
  if (!h->t_grad || !db->train || db->dbg_layers != h->cfg.n_attention || !db->kept)
    return fail(h, SCANN_ERR_INVALID, "scann_train_backward: run scann_train_forward on this batch first");
  HIPCHK(h, hipSetDevice(h->device));
  const double rmse = std::sqrt(sse_global / (double)count_global);
  const float scale = rmse > 0 ? (float)(1.0 / ((double)count_global * rmse)) : 0.f;
  h->grads_zeroed = false;
  return backward_impl(h, db, *db->train, scale, nullptr, false);
}

int64_t scann_train_debug_read(scann_handle_t* h, scann_dbatch_t* db, const char* name, float* out, int64_t cap) {
  if (!h || !db || !name || !out) return fail(h, SCANN_ERR_INVALID, "scann_train_debug_read: null argument");
  if (!h->generic) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_train_debug_read: plain-fp32 (generic-width) training handles only");
  const scann_train_ws* w = db->train.get();
  if (!w || w->gen.dbg.empty()) return fail(h, SCANN_ERR_INVALID, "scann_train_debug_read: run scann_train_backward on this batch first");
  auto it = w->gen.dbg.find(name);
  if (it == w->gen.dbg.end()) return fail(h, SCANN_ERR_INVALID, std::string("scann_train_debug_read: no tensor named ") + name);
  if ((int64_t)it->second.second > cap) return fail(h, SCANN_ERR_INVALID, "scann_train_debug_read: output buffer too small");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  HIPCHK(h, hipMemcpy(out, it->second.first, it->second.second * 4, hipMemcpyDeviceToHost));
  return (int64_t)it->second.second;
}

int scann_adam_step(scann_handle_t* h, float lr_t, float beta1, float beta2, float eps, float l2) {
  if (!h || !h->t_master) return fail(h, SCANN_ERR_INVALID, "scann_adam_step: call scann_train_begin first");
  HIPCHK(h, hipSetDevice(h->device));
  const int r = adam_impl(h, lr_t, beta1, beta2, eps, l2, 0);
  if (r) return r;
  HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  return check_range(h, "scann_adam_step");
}

// One optimisation step without a host round trip in the middle: forward, [all-reduce of {sse, count}], backward with the loss scale
// formed on the device, [all-reduce of the gradients], Adam + weight-image refresh; ONE synchronisation at the end.  Same results as
// scann_train_forward / scann_allreduce_sse / scann_zero_grads / scann_train_backward / scann_allreduce_grads / scann_adam_step.
int scann_train_step_begin(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, uint64_t seed, float lr_t, float beta1,
                           float beta2, float eps, float l2) {
  if (!h || !db || !targets) return fail(h, SCANN_ERR_INVALID, "scann_train_step: null argument");
  if (h->step_begun - h->step_ended >= 2) return fail(h, SCANN_ERR_INVALID, "scann_train_step_begin: two steps are already in flight; end one first");
  const int slot = (int)(h->step_begun & 1);
  if (!h->t_master) return fail(h, SCANN_ERR_INVALID, "scann_train_step: call scann_train_begin first");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  scann_train_ws* w = nullptr;
  int r = train_forward_impl(h, db, targets, dropout, h->attn_drop_p, seed, &w, slot);
  if (r) return r;
  // From here on kernels of this step are queued: a failure below must not leave the slot's pinned buffers (targets, statistics)
  // looking free while that work is still running -- drain the stream before the error goes back (the step is not counted).
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(s);
    if (h->train_aux) (void)hipStreamSynchronize(h->train_aux);
    if (h->train_aux2) (void)hipStreamSynchronize(h->train_aux2);
    h->grads_zeroed = false;
    return code;
  };
  const bool single = !(h->comm && h->comm_world > 1);
  if (!single) {  // losses.py:5-6 is the RMSE of the GLOBAL batch
    const ncclResult_t nr = ncclAllReduce(w->sse, w->sse, 3, ncclDouble, ncclSum, h->comm, s);
    if (nr != ncclSuccess) return drained(fail(h, SCANN_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(nr)));
    if (hipMemcpyAsync(h->h_stat + 4 * slot, w->sse, 3 * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
      return drained(fail(h, SCANN_ERR_HIP, "scann_train_step_begin: hipMemcpyAsync(statistics) failed"));
  }
  if (!h->grads_zeroed && hipMemsetAsync(h->t_grad, 0, h->host_master.size() * 4, s) != hipSuccess)
    return drained(fail(h, SCANN_ERR_HIP, "scann_train_step_begin: hipMemsetAsync(gradients) failed"));
  h->grads_zeroed = false;
  r = backward_impl(h, db, *w, 0.f, w->sse, /*dy_done=*/single);
  if (r) return drained(r);
  r = scann_allreduce_grads(h);
  if (r) return drained(r);
  r = adam_impl(h, lr_t, beta1, beta2, eps, l2, /*zero_g=*/1);  // leaves the gradient vector zeroed for the next step
  if (r) return drained(r);
  h->grads_zeroed = true;
  if (!h->step_ev[slot]) HIPCHK(h, hipEventCreateWithFlags(&h->step_ev[slot], hipEventDisableTiming));
  HIPCHK(h, hipEventRecord(h->step_ev[slot], s));
  db->busy_ev = h->step_ev[slot];
  h->step_begun += 1;
  return SCANN_OK;
}

int scann_train_step_end(scann_handle_t* h, double* sse_out, int64_t* count_out, double* abs_err_out) {
  if (!h || !sse_out || !count_out) return fail(h, SCANN_ERR_INVALID, "scann_train_step_end: null argument");
  if (h->step_begun == h->step_ended) return fail(h, SCANN_ERR_INVALID, "scann_train_step_end: no step in flight");
  HIPCHK(h, hipSetDevice(h->device));
  const int slot = (int)(h->step_ended & 1);  // the OLDEST step in flight
  HIPCHK(h, hipEventSynchronize(h->step_ev[slot]));
  h->step_ended += 1;  // only now: after a failed wait the slot still counts as in flight (its buffers are not reused)
  *sse_out = h->h_stat[4 * slot];
  *count_out = (int64_t)(h->h_stat[4 * slot + 1] + 0.5);
  if (abs_err_out) *abs_err_out = h->h_stat[4 * slot + 2];
  return check_range(h, "scann_train_step_end");
}

int scann_train_step(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, uint64_t seed, float lr_t, float beta1,
                     float beta2, float eps, float l2, double* sse_out, int64_t* count_out) {
  if (!sse_out || !count_out) return fail(h, SCANN_ERR_INVALID, "scann_train_step: null argument");
  const int r = scann_train_step_begin(h, db, targets, dropout, seed, lr_t, beta1, beta2, eps, l2);
  return r ? r : scann_train_step_end(h, sse_out, count_out, nullptr);
}

// d y_s / d input for every structure of a resident batch: the training forward with inference semantics (no Dropout, no attention
// dropout) and the backward in its data-gradient mode, seeded with d y_s = 1 for every structure (structures are independent, so one
// pass gives each structure's own gradients).  Touches none of the training state: on a training handle it reads the current weights,
// on an inference handle it allocates what the training forward needs privately.  Synchronous.
int scann_input_grads(scann_handle_t* h, scann_dbatch_t* db, float* y, float* d_distance, float* d_weight, float* d_ring, float* d_cgcnn) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_input_grads: null argument");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_input_grads: weights not loaded");
  const scann_config_t& c = h->cfg;
  if (d_ring && !c.use_ring) return fail(h, SCANN_ERR_INVALID, "scann_input_grads: the model has no ring_aromatic input (use_ring off)");
  if (d_cgcnn && !c.feature_cgcnn) return fail(h, SCANN_ERR_INVALID, "scann_input_grads: the model has no cgcnn input (feature is not cgcnn)");
  if (h->weights_exact)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_input_grads: " + h->exact_reason + "; the backward kernels multiply in split-fp16 "
                                          "form only (inference of such a checkpoint runs on the exact-fp32 kernels)");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->generic && !h->g_WT)
    if (const int r = build_gen_transposes(h)) return r;
  if (!h->ig_grad) HIPCHK(h, hipMalloc((void**)&h->ig_grad, h->host_master.size() * 4));
  hipStream_t s = h->streams[0];
  scann_train_ws* w = nullptr;
  int r = train_forward_impl(h, db, nullptr, 0.f, 0.f, 0, &w, 2);
  if (r) {
    db->kept = false;
    return r;
  }
  const int A = db->n_atom, E = db->n_edge, B = db->n_struct;
  const size_t bE = align_up((size_t)std::max(E, 1) * 4), bR = c.use_ring ? align_up((size_t)A * 2 * 4) : 0,
               bC = c.feature_cgcnn ? align_up((size_t)A * 92 * 4) : 0, need = 2 * bE + bR + bC;
  if (w->ig_bytes < need) {
    HIPCHK(h, hipStreamSynchronize(s));
    cached_free(w->ig);
    w->ig = nullptr;
    w->ig_bytes = 0;
    HIPCHK(h, cached_malloc((void**)&w->ig, need));
    w->ig_bytes = need;
  }
  InGrad ig{};
  ig.d_dist = d_distance ? reinterpret_cast<float*>(w->ig) : nullptr;
  ig.d_weight = d_weight ? reinterpret_cast<float*>(w->ig + bE) : nullptr;
  ig.d_ring = d_ring ? reinterpret_cast<float*>(w->ig + 2 * bE) : nullptr;
  ig.d_cgcnn = d_cgcnn ? reinterpret_cast<float*>(w->ig + 2 * bE + bR) : nullptr;
  HIPCHK(h, hipMemsetAsync(w->ig, 0, need, s));  // (the base branch's leaf adds per layer; a model without layers leaves zeros)
  HIPCHK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w->dy), 0x3f800000, (size_t)B, s));  // d y_s = 1.0f
  r = backward_impl(h, db, *w, 0.f, nullptr, /*dy_done=*/true, &ig);
  db->kept = false;  // the kept tensors are this call's, not a training forward's (scann_train_backward asks for a new one)
  const hipError_t se = hipStreamSynchronize(s);
  if (r) return r;
  HIPCHK(h, se);
  if ((r = check_range(h, "scann_input_grads", 0))) return r;
  if ((r = check_pack_flag(h, db, "scann_input_grads"))) return r;
  if (y) HIPCHK(h, hipMemcpy(y, db->y, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (E > 0 && d_distance) HIPCHK(h, hipMemcpy(d_distance, ig.d_dist, (size_t)E * 4, hipMemcpyDeviceToHost));
  if (E > 0 && d_weight) HIPCHK(h, hipMemcpy(d_weight, ig.d_weight, (size_t)E * 4, hipMemcpyDeviceToHost));
  if (A > 0 && d_ring) HIPCHK(h, hipMemcpy(d_ring, ig.d_ring, (size_t)A * 2 * 4, hipMemcpyDeviceToHost));
  if (A > 0 && d_cgcnn) HIPCHK(h, hipMemcpy(d_cgcnn, ig.d_cgcnn, (size_t)A * 92 * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

}  // extern "C"

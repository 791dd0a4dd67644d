// Forward launch schedules -- run_forward (the split-fp16 MFMA kernels and their exact-fp32 instantiations), run_forward_generic
// (the plain-fp32 kernels of other widths) -- and the entry points that run, time or inspect one forward.  Every forward of the library
// -- inference, training, a Monte Carlo dropout sample, a member or a run of members of a model set -- is run_forward with the FwdOpts
// (scann_runtime.h) that describe it; no caller selects a mode by writing into the handle or the batch.
#include "scann_runtime.h"

namespace {

// Events that only time kernels on one stream: no system-scope cache write-back / invalidate when they fire (the HIP headers' own
// advice for timing events), so that a sampled launch is not lengthened by its own measurement.
constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;

int ensure_debug(scann_handle* h, scann_dbatch* db) {
  const int L = h->cfg.n_attention;
  if (db->dbg_layers == L) return SCANN_OK;
  HIPCHK(h, cached_malloc((void**)&db->dbg_c, (size_t)(L + 1) * db->n_atom * D * 4));
  HIPCHK(h, cached_malloc((void**)&db->dbg_ctx, (size_t)std::max(L, 1) * db->n_atom * D * 4));
  if (h->cfg.g_update) HIPCHK(h, cached_malloc((void**)&db->dbg_g, (size_t)(L + 1) * std::max(db->n_edge, 1) * D * 4));
  db->dbg_layers = L;
  return SCANN_OK;
}

// The inference outputs this forward of `db` is to write (o.out_*; a training forward: none): the batch's output block is sized for them
// -- allocated by the first forward that needs it, grown when a selection or batch needs more -- and db->out_* record what this forward
// writes.  With nothing selected nothing happens.
int ensure_outputs(scann_handle* h, scann_dbatch* db, const FwdOpts& o) {
  db->out_layers = o.train ? 0 : o.out_layers;
  db->out_flags = o.train ? 0 : o.out_flags;
  db->out_attn = db->out_z = db->out_bf = nullptr;
  if (!db->out_layers && !db->out_flags) return SCANN_OK;
  const scann_config_t& c = h->cfg;
  const size_t n_attn = (size_t)__builtin_popcountll(db->out_layers) * db->n_edge * c.num_head;
  const size_t n_z = db->out_flags & SCANN_OUT_AFTER_LC ? (size_t)db->n_atom * c.global_dim : 0;
  const size_t n_bf = db->out_flags & SCANN_OUT_BF_PROPERTY ? (size_t)db->n_struct * c.dense_out : 0;
  const size_t need = align_up(n_attn * 4) + align_up(n_z * 4) + align_up(n_bf * 4) + 256;
  if (db->out_cap < need) {
    HIPCHK(h, hipDeviceSynchronize());  // (an earlier forward of the batch, on any stream, may still write the old block)
    cached_free(db->out_block);
    db->out_block = nullptr;
    db->out_cap = 0;
    HIPCHK(h, cached_malloc((void**)&db->out_block, need));
    db->out_cap = need;
  }
  char* p = db->out_block;
  if (n_attn) db->out_attn = reinterpret_cast<float*>(p);
  p += align_up(n_attn * 4);
  if (n_z) db->out_z = reinterpret_cast<float*>(p);
  p += align_up(n_z * 4);
  if (n_bf) db->out_bf = reinterpret_cast<float*>(p);
  return SCANN_OK;
}

// where layer l's attention weights go in this forward (null: not selected, or a batch without edges)
float* attn_out_of(const scann_handle* h, const scann_dbatch* db, int l) {
  if (!db->out_attn || !((db->out_layers >> l) & 1) || db->n_edge <= 0) return nullptr;
  const uint64_t below = db->out_layers & ((uint64_t(1) << l) - 1);
  return db->out_attn + (size_t)__builtin_popcountll(below) * db->n_edge * h->cfg.num_head;
}

// create_model (scann_model.py:362-447) for a handle whose widths are not 128 / 8: one plain-fp32 kernel per formula
// (scann_generic.hip) on the same packed batch.  kp non-null: the training forward -- Dropout layers active (kp->drop_p, kp->attn_p,
// kp->seed), every intermediate kept in kp, the property head as dense launches.  wh: whose weights; buf: where y and the scores go
int run_forward_generic(scann_handle* h, scann_dbatch* db, hipStream_t s, const FwdOpts& o, const scann_handle* wh, const FwdBufs& buf) {
  const scann_config_t& c = h->cfg;
  GenKeep* const kp = o.train ? o.train->gen : nullptr;
  const bool outs = o.out_flags != FWD_OUT_UNTOUCHED && !kp;  // (the selected outputs of an inference forward)
  const int L = c.n_attention, A = db->n_atom, E = db->n_edge, B = db->n_struct;
  const int d = c.local_dim, dg = c.global_dim, dout = c.dense_out, H = c.num_head, emb = c.embedding_dim;
  const int cin = emb + (c.use_ring ? 10 : 0);
  if (kp) kp->dbg.clear();  // (scann_train_debug_read: the tensors it names belong to the backward of THIS forward's arena)
  if ((size_t)std::max(1, db->max_degree) * H * 4 * (kp ? 3 : 1) > 60000 || ((size_t)db->max_atoms * (kp ? 3 : 1) + dg + dout + 4) * 4 > 60000 ||
      (size_t)4 * 3 * d * 4 > 60000)
    return fail(h, SCANN_ERR_UNSUPPORTED, "forward (generic widths): an atom's neighbours x heads, or a structure's atoms, exceed one workgroup's LDS");
  // the training forward also admits only what its backward can run (gen_backward's GlobalAttention pooling: 3 x atoms + 4 doubles of LDS),
  // so that a step is refused here, before it has touched anything, and not halfway through
  if (kp && ((size_t)3 * db->max_atoms + 4) * sizeof(double) > 65536)
    return fail(h, SCANN_ERR_UNSUPPORTED, "training forward (generic widths): a structure's atoms exceed one workgroup's LDS in the backward (GlobalAttention pooling: 3 x atoms doubles <= 64 KiB)");
  auto W =[&](const std::string& name) -> const float* { return wh->g_weights + wh->g_off.at(name); };
  // workspace: atom rows, edge rows, Gaussian bases
  const size_t fA = (size_t)A, fE = (size_t)std::max(E, 1), fB = (size_t)B, Ls = (size_t)L;
  float* p = nullptr;
  char* p_end = nullptr;
  if (!kp) {
    const size_t need = 4 * (fA * (5 * (size_t)d + (size_t)cin + (size_t)emb + 10 + 3 * (size_t)dg) + fE * (3 * (size_t)d + 2 * NG)) + 4096;
    if (db->gen_ws_bytes < need) {
      HIPCHK(h, hipStreamSynchronize(s));
      cached_free(db->gen_ws);
      db->gen_ws = nullptr;
      db->gen_ws_bytes = 0;
      HIPCHK(h, cached_malloc((void**)&db->gen_ws, need));
      db->gen_ws_bytes = need;
    }
    p = reinterpret_cast<float*>(db->gen_ws);
    p_end = db->gen_ws + db->gen_ws_bytes;
  } else {
    const size_t need = 4 * (fA * ((size_t)emb + 10 + (2 + 7 * Ls) * (size_t)d + 4 * (size_t)dg) + fE * (2 * NG + (5 + 4 * Ls) * (size_t)d) +
                             fB * ((size_t)dg + 2 * (size_t)dout + 1)) + 256 * (32 + 12 * Ls);
    if (kp->bytes < need) {
      HIPCHK(h, hipStreamSynchronize(s));
      cached_free(kp->arena);
      kp->arena = nullptr;
      kp->bytes = 0;
      HIPCHK(h, cached_malloc((void**)&kp->arena, need));
      kp->bytes = need;
    }
    p = reinterpret_cast<float*>(kp->arena);
    p_end = kp->arena + kp->bytes;
    kp->layer.assign((size_t)L, GenLayerKeep{});
  }
  auto take = [&](size_t n) { float* q = p; p += (n + 63) & ~(size_t)63; return q; };
  float *cc = take(fA * d), *ctx = nullptr, *t1 = nullptr, *t2 = nullptr, *q = nullptr;
  if (!kp) { ctx = take(fA * d); t1 = take(fA * d); t2 = take(fA * d); q = take(fA * d); }
  float *embE = take(fA * emb), *ring10 = take(fA * 10);
  float *z = take(fA * dg), *gq = take(fA * dg), *gk = take(fA * dg);
  if (!kp) { db->gen_gq = gq; db->gen_gk = gk; }
  float *G = take(fE * d), *T = nullptr, *K = nullptr, *gd = take(fE * NG), *gw = take(fE * NG);
  if (!kp) { T = take(fE * d); K = take(fE * d); }
  const McState* mc = kp ? nullptr : o.mc;  // Monte Carlo dropout (scann_predict_mc): structure-local masks
  const float tp = kp ? kp->drop_p : mc ? mc->p_drop : 0.f;
  const unsigned long long seed = kp ? kp->seed : mc ? mc->seed : 0;
  auto dense = [&](GenSeg s0, GenSeg s1, GenSeg s2, int n_seg, int prod, const std::string& name, int K_, int N_, int rows, int act,
                   const float* res, const float* row_scale, float* Y, float* pre = nullptr, float drop_p = 0.f, unsigned drop_tag = 0) {
    GenDenseArgs a{};
    a.seg[0] = s0; a.seg[1] = s1; a.seg[2] = s2; a.n_seg = n_seg; a.prod = prod;
    a.W = W(name + "/kernel"); a.b = W(name + "/bias"); a.K = K_; a.N = N_; a.rows = rows; a.act = act;
    a.res = res; a.res_idx = nullptr; a.row_scale = row_scale; a.Y = Y;
    a.pre = pre; a.drop_p = drop_p; a.drop_tag = drop_tag; a.drop_seed = seed;
    if (mc) { a.mc_rows = mc->rows; a.mc_t = mc->t; }
    launch_gen_dense(a, s);
  };
  const GenSeg none{nullptr, nullptr, 0};
  // ---- embedding (scann_model.py:362-374; Dropout(0.1) on the centres in training, :374) ----
  float* pre_e = kp ? take(fA * d) : nullptr;
  GenSeg e0;
  if (c.feature_cgcnn) {
    dense(GenSeg{db->cgcnn, nullptr, 92}, none, none, 1, 0, "embed_atom", 92, emb, A, 0, nullptr, nullptr, embE);
    e0 = GenSeg{embE, nullptr, emb};
  } else {
    e0 = GenSeg{W("embed_atom/embeddings"), db->atomic, emb};
  }
  if (c.use_ring) {
    dense(GenSeg{db->ring, nullptr, 2}, none, none, 1, 0, "extra_embed", 2, 10, A, 0, nullptr, nullptr, ring10);
    dense(e0, GenSeg{ring10, nullptr, 10}, none, 2, 0, "dense_embed", emb + 10, d, A, 1, nullptr, nullptr, cc, pre_e, tp, DROP_TAG_EMBED);
  } else {
    dense(e0, none, none, 1, 0, "dense_embed", emb, d, A, 1, nullptr, nullptr, cc, pre_e, tp, DROP_TAG_EMBED);
  }
  if (kp) { kp->embE = embE; kp->ring10 = ring10; kp->pre_e = pre_e; kp->cc0 = cc; kp->gd = gd; kp->gw = gw; }
  // ---- Gaussian bases and the initial geometry (scann_model.py:376-391) ----
  launch_gen_gauss(db->dist, wh->g_centres, E, gd, s);
  if (c.g_update) {
    launch_gen_gauss(db->weight, wh->g_centres + NG, E, gw, s);
    float *Td = kp ? take(fE * d) : T, *Tw = kp ? take(fE * d) : K;
    float *pre_d = kp ? take(fE * d) : nullptr, *pre_w = kp ? take(fE * d) : nullptr;
    dense(GenSeg{gd, nullptr, NG}, none, none, 1, 0, "neighbor_d", NG, d, E, 1, nullptr, nullptr, Td, pre_d);
    dense(GenSeg{gw, nullptr, NG}, none, none, 1, 0, "neighbor_w", NG, d, E, 1, nullptr, nullptr, Tw, pre_w);
    launch_gen_mul(Td, Tw, (size_t)E * d, G, s);
    if (kp) { kp->Td = Td; kp->Tw = Tw; kp->pre_d = pre_d; kp->pre_w = pre_w; kp->G0 = G; }
  }
  // ---- LocalAttention iterations (scann_model.py:413-421; attention.py:118-216, :37-40) ----
  for (int l = 0; l < L; ++l) {
    const std::string la = "local_attention_" + std::to_string(l), rn = "residual_norm_" + std::to_string(l);
    GenLayerKeep b;
    b.cc_in = cc; b.G_in = G;
    if (kp) {
      b.Z = take(fE * d); b.Gn = take(fE * d); b.K = take(fE * d);
      if (c.g_update) b.T = take(fE * d);
      b.q = take(fA * d); b.t1 = take(fA * d); b.ctx = take(fA * d);
      if (c.use_attn_norm) { b.pre1 = take(fA * d); b.h1 = take(fA * d); b.t2 = take(fA * d); b.cc_out = take(fA * d); }
      else b.cc_out = b.ctx;
    } else {
      b.T = T; b.Gn = c.g_update ? G : T; b.K = K; b.q = q; b.t1 = t1; b.ctx = ctx; b.h1 = t1; b.t2 = t2;
      b.cc_out = c.use_attn_norm ? cc : ctx;
    }
    if (c.g_update) {
      dense(GenSeg{cc, db->edge_row, d}, GenSeg{G, nullptr, d}, GenSeg{cc, db->edge_col, d}, 3, 0, la + "/filter_geo", 3 * d, d, E, 1, G, nullptr, b.T, b.Z);
      launch_gen_layernorm(b.T, nullptr, W(la + "/layer_norm_g/gamma"), W(la + "/layer_norm_g/beta"), E, d, b.Gn, s);
    } else {
      dense(GenSeg{gd, nullptr, NG}, none, none, 1, 0, la + "/filter_geo", NG, d, E, 1, nullptr, db->weight, b.Gn, b.Z);
    }
    dense(GenSeg{cc, db->edge_col, d}, GenSeg{b.Gn, nullptr, d}, none, 2, 1, la + "/key", d, d, E, 0, nullptr, nullptr, b.K);
    dense(GenSeg{cc, nullptr, d}, none, none, 1, 0, la + "/query", d, d, A, 0, nullptr, nullptr, b.q);
    if (mc && mc->p_attn > 0.f)
      launch_gen_attn_mc(b.q, b.K, db->edge_offset, A, d, H, db->max_degree, b.t1, s, mc->p_attn, DROP_TAG_ATTN + (unsigned)l, seed, mc->rows, mc->t);
    else
      launch_gen_attn(b.q, b.K, db->edge_offset, A, d, H, db->max_degree, b.t1, s, kp ? kp->attn_p : 0.f, DROP_TAG_ATTN + (unsigned)l, seed,
                      outs ? attn_out_of(h, db, l) : nullptr);
    launch_gen_layernorm(b.t1, nullptr, W(la + "/layer_norm/gamma"), W(la + "/layer_norm/beta"), A, d, b.ctx, s);
    if (c.use_attn_norm) {  // ResidualNorm (attention.py:37-40): LayerNorm(x + Dropout(dense_2(swish(dense_1 x))))
      dense(GenSeg{b.ctx, nullptr, d}, none, none, 1, 0, rn + "/dense_1", d, d, A, 1, nullptr, nullptr, b.h1, b.pre1);
      dense(GenSeg{b.h1, nullptr, d}, none, none, 1, 0, rn + "/dense_2", d, d, A, 0, nullptr, nullptr, b.t2, nullptr, tp, (unsigned)l);
      launch_gen_layernorm(b.ctx, b.t2, W(rn + "/layer_norm/gamma"), W(rn + "/layer_norm/beta"), A, d, b.cc_out, s);
    }
    if (kp) {
      kp->layer[(size_t)l] = b;
      cc = b.cc_out;
      if (c.g_update) G = b.Gn;
    } else if (!c.use_attn_norm) {
      std::swap(cc, ctx);
    }
  }
  // ---- readout (scann_model.py:424-447; attention.py:267-318) ----
  float* z_pre = kp ? take(fA * dg) : nullptr;
  if (outs && db->out_z) z = db->out_z;  // inference outputs: after_Lc straight into the batch's output block
  dense(GenSeg{cc, nullptr, d}, none, none, 1, 0, "after_Lc", d, dg, A, 1, nullptr, nullptr, z, z_pre);
  dense(GenSeg{z, nullptr, dg}, none, none, 1, 0, "global_attention/query", dg, dg, A, 0, nullptr, nullptr, gq);
  dense(GenSeg{z, nullptr, dg}, none, none, 1, 0, "global_attention/key", dg, dg, A, 0, nullptr, nullptr, gk);
  float* rep = kp ? take(fB * dg) : nullptr;
  launch_gen_readout(db->mol_offset, B, db->max_atoms, gq, gk, dg, dout, c.use_ga_norm, wh->cfg.relu_out, W("bf_property/kernel"), W("bf_property/bias"),
                     W("predict_property/kernel"), W("predict_property/bias"), buf.ga, buf.y, s, rep, outs ? db->out_bf : nullptr);
  if (kp) {
    float *hid_pre = take(fB * dout), *hid = take(fB * dout);
    dense(GenSeg{rep, nullptr, dg}, none, none, 1, 0, "bf_property", dg, dout, B, 1, nullptr, nullptr, hid, hid_pre);
    dense(GenSeg{hid, nullptr, dout}, none, none, 1, 0, "predict_property", dout, 1, B, 0, nullptr, nullptr, buf.y);
    if (wh->cfg.relu_out) launch_gen_relu(buf.y, B, s);  // mrelu forward (custom_layers.py:15); its gradient is the identity
    kp->cc_L = cc; kp->z_pre = z_pre; kp->z = z; kp->gq = gq; kp->gk = gk; kp->rep = rep; kp->hid_pre = hid_pre; kp->hid = hid;
  }
  if (reinterpret_cast<char*>(p) > p_end) return fail(h, SCANN_ERR_HIP, "forward (generic widths): workspace overrun");
  HIPCHK(h, hipGetLastError());
  return SCANN_OK;
}

}  // namespace

namespace scann {

struct Timer {
  hipStream_t s;
  bool on;
  std::vector<hipEvent_t> ev;
  std::vector<int> kind;
  void mark(int k) {
    if (!on) return;
    hipEvent_t e;
    (void)hipEventCreateWithFlags(&e, kTimingEventFlags);
    (void)hipEventRecord(e, s);
    ev.push_back(e);
    kind.push_back(k);
  }
};

// The forward graph of create_model (scann_model.py:362-447) as a launch schedule on one stream: THE schedule of the 128 / 8 kernels -- what
// kind of forward it enqueues, on whose weights, into which buffers, for how many members of a model set at once is all in `o`.
// kind codes for the timer: 0 basis, 1 atom, 2 edge, 3 readout.
int run_forward(scann_handle* h, scann_dbatch* db, hipStream_t s, const FwdOpts& o) {
  scann_handle* const W = o.n_member ? o.members[0] : o.weights ? o.weights : h;  // the weight holder (a set launch: member 0's, the others by stride)
  const FwdTrain* const tr = o.train;
  const McState* const mc = o.mc;
  Timer* const tm = o.tm;
  const bool debug = o.keep_layers < 0 ? h->debug : o.keep_layers != 0;
  const bool exact = o.exact || ((h->force_exact || W->weights_exact) && !debug && !tr);
  const int nm = o.n_member;
  const int64_t wst = o.m_w, ast = o.m_a;  // byte strides between members' weight images / workspaces (0: not a set launch)
  if (!W->loaded) return fail(h, SCANN_ERR_WEIGHTS, "forward: weights not loaded");
  if (W->small_operands && !exact && !h->generic)  // a debug or a training forward: only the split-fp16 kernels keep what those read
    return fail(h, SCANN_ERR_UNSUPPORTED, "forward: " + W->exact_reason + "; per-layer intermediates (scann_set_debug) and the training forward exist on "
                                          "the split-fp16 kernels only (inference of such a checkpoint runs on the exact-fp32 kernels)");
  if (!o.of_set) {
    db->idle = false;  // work is being enqueued on the batch (scann_batch_release)
    db->fwd_pending = true;
  }
  const scann_config_t& c = h->cfg;
  const int L = c.n_attention;
  const bool outs = o.out_flags != FWD_OUT_UNTOUCHED;  // this forward writes the batch's output block and db->out_* record what
  // exact: the forward's range guard fired (an operand outside the split-fp16 range): the same launches on the EX instantiations of
  // the atom / edge kernels -- exact-fp32 projections -- with the plain first layer (basis_kernel, no per-species tables)
  // inference: the first layer's edge kernel computes its geometry rows from (dist, weight) itself -- geom0 is never written by a
  // basis launch and read back (282 MB of the 16-batch forward's traffic and one launch)
  // Monte Carlo dropout (scann_predict_mc, never exact): the sample's masks at the training forward's Dropout sites, on the MC instantiations
  // (the piece-major family: the fused first layer whatever SCANN_FUSE_BASIS says)
  const bool fuse_basis = !exact && (h->fuse_basis || mc) && c.g_update && L > 0 && !debug && !tr && db->n_edge > 0;
  // the attention-weight stores exist in the piece-major g_update kernels (and the row-major base / exact ones) only.  Refused before the
  // output block is touched: db->out_* go on describing what it holds
  if (outs && !tr && o.out_layers && !h->generic && c.g_update && !exact && !fuse_basis && db->n_edge > 0)
    return fail(h, SCANN_ERR_UNSUPPORTED, "forward: local-attention outputs need the fused first layer (not with scann_set_debug or SCANN_FUSE_BASIS=0)");
  if (fuse_basis && !h->generic && !db->tile_atom) return fail(h, SCANN_ERR_INVALID, "forward: the batch was uploaded without its tile-order side");
  // a batch that is forwarded AGAIN is resident: from its second forward on the piece-major family runs on the filled tile plan (same
  // bytes, 5-10 % fewer tiles), which a one-shot batch would pay more host time for than its forward gains
  if (fuse_basis && !h->generic && db->n_fused++ >= 1 && !db->fill_tried)
    if (const int r = ensure_tile_fill(h, db, s)) return r;
  HIPCHK(h, wait_upload(db, s));  // the inputs' copy (scann_batch_upload returned when it was enqueued)
  if (outs)
    if (const int r = ensure_outputs(h, db, o)) return r;
  const FwdBufs b = o.bufs ? *o.bufs : FwdBufs(db);
  if (h->generic) {
    if (tm) { tm->mark(-1); }
    const int r = run_forward_generic(h, db, s, o, W, b);
    if (tm) tm->mark(3);
    return r;
  }
  if (debug) {
    const int r = ensure_debug(h, db);
    if (r) return r;
  }
  // keep-mode (training / scann_set_debug): every layer writes its centres, context and geometry straight into its slice of
  // the per-layer buffers (base branch: no geometry to thread)
  const size_t nA_ = (size_t)db->n_atom * D, nE_ = (size_t)db->n_edge * D;
  auto c_of = [&](int l) { return debug ? db->dbg_c + (size_t)l * nA_ : b.c; };
  auto ctx_of = [&](int l) { return debug ? db->dbg_ctx + (size_t)l * nA_ : b.ctx; };
  auto g_of = [&](int l) { return debug && c.g_update ? db->dbg_g + (size_t)l * nE_ : b.geom; };
  int32_t* const rflag = h->range_flag ? h->range_flag + (o.slot >= 0 ? o.slot : db->last_slot) : nullptr;  // this stream's range-guard word
  if (tm) tm->mark(-1);
  if (!fuse_basis) {
    if (c.g_update) launch_basis(W->basis, db->dist, db->weight, db->n_edge, g_of(0), s);
    else launch_basis_raw(W->cd, db->dist, db->n_edge, b.gd, s);  // (the Gaussians of the distances: model independent, one launch per set run)
  }
  if (tm) tm->mark(0);

  const bool general_embed = c.use_ring || c.feature_cgcnn;
  if (general_embed) {
    for (int m = 0; m < std::max(nm, 1); ++m) {  // (no SET instantiation: one launch per member)
      EmbedArgs e = nm ? o.members[m]->embed : W->embed;
      e.n_atom = db->n_atom; e.atomic = db->atomic;
      e.c0 = reinterpret_cast<float*>(reinterpret_cast<char*>(b.c0) + m * ast);
      e.ring = c.use_ring ? db->ring : nullptr;
      e.cgcnn = c.feature_cgcnn ? db->cgcnn : nullptr;
      launch_embed(e, s);
    }
    if (tm) tm->mark(0);
  }
  // first layer from per-species tables: no atom launch at all (see EdgeArgs::species)
  // (not with chunked atoms: edge_merge_kernel reads the query rows per atom)
  const bool species0 = fuse_basis && h->species_tables && !general_embed && !(mc && mc->p_drop > 0.f) && W->sp_c && db->n_big == 0;
  bool sp_dirty = W->sp_dirty;  // (a set launch: the whole run's tables again when any of its members' are to be computed)
  for (int m = 1; m < nm; ++m) sp_dirty |= o.members[m]->sp_dirty;
  if (species0 && sp_dirty) {
    AtomArgs a{};
    a.n_atom = c.n_atoms; a.x = W->lut; a.ffn = 0; a.c = W->sp_c;
    a.range_flag = rflag; a.layer = 0;
    const LayerParams& p = W->layers[0];
    a.mode = 0;
    a.WAh = p.W1h; a.bA = p.bg; a.WBh = p.W3h; a.WCh = p.Wqh; a.bC = p.bq;
    a.oA = W->sp_P1; a.oB = W->sp_P3; a.oC = W->sp_q;
    a.n_member = nm; a.m_w = a.m_x = a.m_o = wst;
    launch_atom(a, s, h->n_cu, h->atom_rows);
    HIPCHK(h, hipStreamSynchronize(s));  // once per weight change: forwards on the handle's other streams read the tables too
    W->sp_dirty = false;
    for (int m = 1; m < nm; ++m) o.members[m]->sp_dirty = false;
  }
  const bool keep_bwd = tr && tr->keep_backward;
  for (int l = 0; l <= L; ++l) {
    // training forward through edge_kernel_lean: q, V, T, ang, K of every layer are kept for the backward
    const bool keep = keep_bwd && db->keep_K && l < L;
    // atom kernel at the head of layer l: ResidualNorm of layer l-1, centres, projections of layer l
    AtomArgs a{};
    a.n_atom = db->n_atom;
    a.n_member = nm; a.m_w = wst; a.m_x = a.m_o = ast;
    if (l == 0) {
      a.x = general_embed ? b.c0 : W->lut;
      a.x_index = general_embed ? nullptr : db->atomic;
      a.ffn = 0;
      if (!general_embed) a.m_x = wst;
    } else {
      a.x = ctx_of(l - 1);
      a.x_index = nullptr;
      a.ffn = c.use_attn_norm ? 1 : 0;
      const LayerParams& pp = W->layers[l - 1];
      a.Wf1h = pp.Wf1h; a.bf1 = pp.bf1; a.Wf2h = pp.Wf2h; a.bf2 = pp.bf2; a.lnr_g = pp.lnr_g; a.lnr_b = pp.lnr_b;
      if (a.ffn && keep_bwd && db->keep_T2) {
        a.keep_pre1 = db->keep_pre1 + (size_t)(l - 1) * nA_; a.keep_H1 = db->keep_H1 + (size_t)(l - 1) * nA_;
        a.keep_T2 = db->keep_T2 + (size_t)(l - 1) * nA_;
      }
    }
    a.c = c_of(l);
    a.range_flag = rflag; a.layer = l;
    if (tr && tr->drop_p > 0.f) {  // training-mode Dropout(0.1) layers (scann_model.py:374, attention.py:29)
      a.drop_p = (l == 0 || c.use_attn_norm) ? tr->drop_p : 0.f;
      a.drop_seed = tr->seed;
      a.drop_tag = l == 0 ? DROP_TAG_EMBED : (unsigned)(l - 1);
    }
    if (mc && mc->p_drop > 0.f && (l == 0 || c.use_attn_norm)) {  // the same sites and tags, structure-local masks
      a.drop_p = mc->p_drop;
      a.drop_seed = mc->seed;
      a.drop_tag = l == 0 ? DROP_TAG_EMBED : (unsigned)(l - 1);
      a.mc_rows = mc->rows;
      a.mc_t = mc->t;
    }
    if (l < L) {
      const LayerParams& p = W->layers[l];
      a.mode = c.g_update ? 0 : 1;
      a.WAh = p.W1h; a.bA = p.bg; a.WBh = p.W3h; a.WCh = p.Wqh; a.bC = p.bq;
      a.oA = b.P1; a.oB = b.P3; a.oC = keep ? db->keep_q + (size_t)l * nA_ : b.q;
    } else {
      a.mode = 2;
      a.WAh = W->head.Wah; a.bA = W->head.ba; a.WCh = W->head.Wgqh; a.bC = W->head.bgq; a.WDh = W->head.Wgkh; a.bD = W->head.bgk;
      a.oB = b.gk; a.oC = b.gq;
      if (keep_bwd && db->keep_preA) { a.keep_preA = db->keep_preA; a.keep_z = db->keep_z; }
      a.out_z = outs ? db->out_z : nullptr;
    }
#ifdef SCANN_STAMPS
    if (getenv("SCANN_STAMP_ATOM") && l >= 1 && l < L) {  // phase clocks of atom_kernel<true, 0> (the last such launch wins)
      const int nt = (db->n_atom + 31) / 32;  // 32- or 64-row tiles (launch_atom): room for either
      if (!db->stamps) HIPCHK(h, hipMalloc((void**)&db->stamps, (size_t)nt * 16 * sizeof(unsigned long long)));
      a.stamps = db->stamps;
      db->n_stamp = nt;
    }
#endif
    if (exact) {  // fp32 fragment-order images in place of the split-fp16 ones
      a.exact = 1;
      if (l > 0 && a.ffn) {
        const LayerParams& pp = W->layers[l - 1];
        a.Wf1h = reinterpret_cast<const _Float16*>(pp.Wf1p); a.Wf2h = reinterpret_cast<const _Float16*>(pp.Wf2p);
      }
      if (l < L) {
        const LayerParams& p = W->layers[l];
        a.WAh = reinterpret_cast<const _Float16*>(p.W1p); a.WBh = reinterpret_cast<const _Float16*>(p.W3p);
        a.WCh = reinterpret_cast<const _Float16*>(p.Wqp);
      } else {
        a.WAh = reinterpret_cast<const _Float16*>(W->head.Wap); a.WCh = reinterpret_cast<const _Float16*>(W->head.Wgqp);
        a.WDh = reinterpret_cast<const _Float16*>(W->head.Wgkp);
      }
    }
    if (!(species0 && l == 0)) launch_atom(a, s, h->n_cu, h->atom_rows);
    if (tm) tm->mark(l < L ? 1 : 3);
    if (l == L) break;
    EdgeArgs ea{};
    ea.tiles = db->tiles; ea.n_tile = db->n_tile; ea.g_update = c.g_update; ea.tile_rows = db->tile_rows;
    ea.edge_offset = db->edge_offset; ea.edge_col = db->edge_col; ea.edge_row = db->edge_row;
    ea.geom = g_of(l); ea.geom_out = debug && c.g_update ? g_of(l + 1) : nullptr; ea.gd = b.gd; ea.edge_weight = db->weight;
    if (fuse_basis) {  // the piece-major family runs on the batch's tile-order side: the filled plan (EdgeArgs::tile_atom)
      ea.tiles = db->f_tiles; ea.n_tile = db->n_ftile;
      ea.edge_offset = db->t_offset; ea.edge_col = db->t_col; ea.edge_row = db->t_row; ea.edge_weight = db->t_weight;
      ea.tile_atom = ea.tile_cen = db->tile_atom; ea.tile_edge0 = db->tile_edge0;
    }
    if (fuse_basis && l == 0) { ea.fuse_basis = 1; ea.dist = db->t_dist; ea.basis = W->basis; }
    ea.n_edge = db->n_edge;
    ea.geom_rows = fuse_basis ? 0 : 1;  // piece-major tiles only when the first layer computed its own geometry rows (plain inference)
    ea.geom_dead = (l == L - 1 && !debug) ? 1 : 0;  // the geometry leaving the last layer is never consumed (141 MB of writes per 16-batch launch)
    ea.c = c_of(l); ea.P1 = b.P1; ea.P3 = b.P3; ea.q = keep ? db->keep_q + (size_t)l * nA_ : b.q; ea.ctx = ctx_of(l);
    ea.n_member = nm; ea.m_w = wst; ea.m_a = ea.m_r = ast;
    if (species0 && l == 0) { ea.species = db->atomic; ea.tile_cen = db->tile_species; ea.c = W->sp_c; ea.P1 = W->sp_P1; ea.P3 = W->sp_P3; ea.q = W->sp_q; ea.m_r = wst; }
    if (keep) {
      ea.keep_V = db->keep_V + (size_t)l * nE_; ea.keep_K = db->keep_K + (size_t)l * nE_;
      // T = swish(V) + G and ang = c[j] * G' are formed again where the fused backward needs them (edge_bwd_kernel, the key weight
      // gradient's operand load): two of the six [n_edge,128] streams of the training forward's edge launch
      if (db->keep_T) ea.keep_T = db->keep_T + (size_t)l * nE_;
      if (db->keep_ang) ea.keep_ang = db->keep_ang + (size_t)l * nE_;
      db->kept = true;
    }
    ea.p = W->layers[l];
    if (exact) {
      ea.exact = 1;
      ea.p.W2h = reinterpret_cast<const _Float16*>(ea.p.W2p); ea.p.Wkh = reinterpret_cast<const _Float16*>(ea.p.Wkp);
    }
    ea.range_flag = rflag; ea.layer = l;
    // (the first layer's launch with the basis MLP fused in is a different kernel: not part of edge_kernel's sampled average)
    // (... nor is the last layer's, whose geometry is not stored -- the DEAD instantiation, ~10 % shorter: the sampled average is the
    //  kernel rocprofv3 lists as edge_kernel<true, RT, false, false, false, false>, and its algorithmic bytes include that store)
    const bool sample = !tm && !mc && !o.of_set && h->time_every > 0 && (h->time_count % h->time_every) == 0 && !(fuse_basis && l == 0) &&
                        !(ea.geom_dead && L > 2);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (sample) {
      (void)hipEventCreateWithFlags(&ev0, kTimingEventFlags);
      (void)hipEventCreateWithFlags(&ev1, kTimingEventFlags);
      (void)hipEventRecord(ev0, s);
    }
    ea.tile_part = db->tile_part; ea.part_buf = b.part_buf;
    ea.xcd_remap = h->xcd_remap;
    ea.attn_out = outs ? attn_out_of(h, db, l) : nullptr;
    if (tr && tr->attn_p > 0.f) {  // validation passes run with scann_set_attention_dropout(h, 0): trainer.fit
      ea.attn_drop_p = tr->attn_p;
      ea.attn_drop_seed = tr->seed;
      ea.attn_drop_tag = DROP_TAG_ATTN + (unsigned)l;
    }
    if (mc && mc->p_attn > 0.f && db->n_edge > 0) {
      ea.attn_drop_p = mc->p_attn;
      ea.attn_drop_seed = mc->seed;
      ea.attn_drop_tag = DROP_TAG_ATTN + (unsigned)l;
      ea.mc_rows = mc->rows;
      ea.mc_t = mc->t;
    }
#ifdef SCANN_STAMPS
    if (!getenv("SCANN_STAMP_ATOM") && l == (getenv("SCANN_STAMP_LAYER") ? atoi(getenv("SCANN_STAMP_LAYER")) : L - 1)) {  // one launch's picture
      if (!db->stamps) HIPCHK(h, hipMalloc((void**)&db->stamps, (size_t)db->n_tile * 16 * sizeof(unsigned long long)));
      ea.stamps = db->stamps;
      db->n_stamp = db->n_tile;
    }
#endif
    launch_edge(ea, s);
    if (nm) launch_edge_merge_set(db->big_tab, db->n_big, b.part_buf, ea.q, ea.p.ln_g, ea.p.ln_b, ea.ctx, rflag, l, nm, ast, wst, s);
    else launch_edge_merge(db->big_tab, db->n_big, b.part_buf, ea.q, ea.p.ln_g, ea.p.ln_b, ea.ctx, rflag, l, s);
    if (ea.attn_out) launch_attn_merge(db->big_tab, db->n_big, b.part_buf, db->edge_offset, db->tile_rows, ea.attn_out, s);
    if (sample) {
      (void)hipEventRecord(ev1, s);
      h->time_ev.push_back(ev0);
      h->time_ev.push_back(ev1);
      h->time_edges.push_back(db->n_edge);
    }
    if (tm) tm->mark(2);
  }
  if (!tm && !mc && !o.of_set) h->time_count++;
  ReadoutArgs r{};
  r.mol_offset = db->mol_offset; r.n_struct = db->n_struct; r.max_atoms = db->max_atoms;
  r.gq = b.gq; r.gk = b.gk; r.use_ga_norm = c.use_ga_norm; r.relu_out = W->cfg.relu_out;
  for (int m = 1; m < nm; ++m) r.relu_out |= o.members[m]->cfg.relu_out << m;  // (a set launch: bit m is member m's mrelu)
  r.p = W->head; r.ga_attn = b.ga; r.y = b.y; r.bf_out = outs ? db->out_bf : nullptr;
  r.n_member = nm; r.m_w = wst; r.m_a = ast; r.m_g = o.m_g; r.m_y = o.m_y;
  launch_readout(r, s);
  if (tm) tm->mark(3);
  HIPCHK(h, hipGetLastError());
  return SCANN_OK;
}

}  // namespace scann

extern "C" {

int scann_forward_resident(scann_handle_t* h, scann_dbatch_t* db, int stream_slot) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_forward_resident: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  const int slot = ((stream_slot % h->nstream) + h->nstream) % h->nstream;
  db->last_slot = slot;
  return run_forward(h, db, h->streams[slot], selected_opts(h));
}

int scann_forward_profile(scann_handle_t* h, scann_dbatch_t* db, scann_profile_t* prof) {
  if (!h || !db || !prof) return fail(h, SCANN_ERR_INVALID, "scann_forward_profile: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  memset(prof, 0, sizeof(*prof));
  Timer tm{h->streams[0], true, {}, {}};
  db->last_slot = 0;
  FwdOpts o = selected_opts(h);
  o.tm = &tm;
  const int r = run_forward(h, db, h->streams[0], o);
  if (r) return r;
  HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  if (const int rp = check_pack_flag(h, db, "scann_forward_profile")) return rp;
  for (size_t i = 1; i < tm.ev.size(); ++i) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, tm.ev[i - 1], tm.ev[i]);
    switch (tm.kind[i]) {
      case 0: prof->ms_basis += ms; break;
      case 1: prof->ms_atom += ms; prof->n_atom_launch++; break;
      case 2: prof->ms_edge += ms; prof->n_edge_launch++; break;
      default: prof->ms_readout += ms; break;
    }
  }
  if (tm.ev.size() >= 2) (void)hipEventElapsedTime(&prof->ms_total, tm.ev.front(), tm.ev.back());
  for (hipEvent_t e : tm.ev) (void)hipEventDestroy(e);
  return SCANN_OK;
}

int scann_edge_timing(scann_handle_t* h, int every) {
  if (!h) return SCANN_ERR_INVALID;
  h->time_every = every > 0 ? every : 0;
  h->time_count = 0;
  return SCANN_OK;
}

int scann_edge_timing_read(scann_handle_t* h, double* avg_us, int64_t* n_launches, double* avg_edges) {
  if (!h || !avg_us || !n_launches) return SCANN_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  double tot = 0, edges = 0;
  int64_t n = 0;
  for (size_t i = 0; i + 1 < h->time_ev.size(); i += 2) {
    float ms = 0.f;
    if (hipEventSynchronize(h->time_ev[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, h->time_ev[i], h->time_ev[i + 1]) == hipSuccess) {
      tot += ms * 1e3;
      edges += h->time_edges[i / 2];
      ++n;
    }
    (void)hipEventDestroy(h->time_ev[i]);
    (void)hipEventDestroy(h->time_ev[i + 1]);
  }
  h->time_ev.clear();
  h->time_edges.clear();
  *avg_us = n ? tot / n : 0.0;
  *n_launches = n;
  if (avg_edges) *avg_edges = n ? edges / n : 0.0;
  return SCANN_OK;
}

int scann_debug_stamps(scann_handle_t* h, scann_dbatch_t* db, uint64_t* out, int max_tiles) {
  if (!h || !db || !out) return fail(h, SCANN_ERR_INVALID, "scann_debug_stamps: null argument");
#ifdef SCANN_STAMPS
  if (!db->stamps) return fail(h, SCANN_ERR_INVALID, "scann_debug_stamps: no forward has run");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  const int n = std::min(max_tiles, db->n_stamp);
  HIPCHK(h, hipMemcpy(out, db->stamps, (size_t)n * 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return n;
#else
  (void)max_tiles;
  return fail(h, SCANN_ERR_UNSUPPORTED, "scann_debug_stamps: library was not built with -DSCANN_STAMPS");
#endif
}

int scann_debug_read(scann_handle_t* h, scann_dbatch_t* db, int what, int layer, float* out) {
  if (!h || !db || !out) return fail(h, SCANN_ERR_INVALID, "scann_debug_read: null argument");
  const int L = h->cfg.n_attention;
  if (db->dbg_layers != L) return fail(h, SCANN_ERR_INVALID, "scann_debug_read: forward was not run with debug on");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->streams[db->last_slot]));
  if (const int rp = check_pack_flag(h, db, "scann_debug_read")) return rp;
  const size_t rowA = (size_t)db->n_atom * D, rowE = (size_t)db->n_edge * D;
  const float* src = nullptr;
  size_t n = 0;
  if (what == 0 && layer >= 0 && layer <= L) { src = db->dbg_c + layer * rowA; n = rowA; }
  else if (what == 1 && h->cfg.g_update && layer >= 0 && layer <= L) { src = db->dbg_g + layer * rowE; n = rowE; }
  else if (what == 2 && layer >= 1 && layer <= L) { src = db->dbg_ctx + (layer - 1) * rowA; n = rowA; }
  else if (what >= 3 && what <= 7 && db->kept && layer >= 1 && layer <= L) {
    // per-layer tensors kept by the last TRAINING forward (scann_train_forward): 3 = K, 4 = ang, 5 = V, 6 = T [n_edge,128]; 7 = q [n_atom,128]
    const float* base = what == 3 ? db->keep_K : what == 4 ? db->keep_ang : what == 5 ? db->keep_V : what == 6 ? db->keep_T : db->keep_q;
    if (!base)  // the fused backward forms T and the gated rows again instead of reading them: the training forward does not store them
      return fail(h, SCANN_ERR_UNSUPPORTED, "scann_debug_read: this tensor is not kept by the training forward (selectors 4 = ang and 6 = T exist with the "
                                            "modular backward only: SCANN_TRAIN_FUSED=0; the base branch keeps no T)");
    n = what == 7 ? rowA : rowE;
    src = base + (size_t)(layer - 1) * n;
  }
  else return fail(h, SCANN_ERR_INVALID, "scann_debug_read: bad selector");
  if (n) HIPCHK(h, hipMemcpy(out, src, n * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

int64_t scann_exact_reruns(const scann_handle_t* h) { return h ? h->exact_reruns : -1; }
int scann_weights_exact(const scann_handle_t* h) { return h ? (int)h->weights_exact : -1; }

int scann_set_outputs(scann_handle_t* h, uint64_t attn_layers, int32_t flags) {
  if (!h) return SCANN_ERR_INVALID;
  const int L = h->cfg.n_attention;
  if (L < 64 && (attn_layers >> L) != 0)
    return fail(h, SCANN_ERR_INVALID, "scann_set_outputs: local_attention layer >= n_attention (" + std::to_string(L) + ")");
  if (flags & ~(SCANN_OUT_AFTER_LC | SCANN_OUT_BF_PROPERTY)) return fail(h, SCANN_ERR_INVALID, "scann_set_outputs: unknown output flag");
  h->out_layers = attn_layers;
  h->out_flags = flags;
  return SCANN_OK;
}

int64_t scann_output_read(scann_handle_t* h, scann_dbatch_t* db, int32_t what, int32_t layer, float* out, int64_t cap) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_output_read: null argument");
  const scann_config_t& c = h->cfg;
  int64_t n = 0;
  if (what == SCANN_OUT_LOCAL_ATTENTION) {
    if (layer < 0 || layer >= c.n_attention || layer >= 64 || !((db->out_layers >> layer) & 1))
      return fail(h, SCANN_ERR_INVALID, "scann_output_read: local_attention_" + std::to_string(layer) + " was not selected for the batch's last forward");
    n = (int64_t)db->n_edge * c.num_head;
  } else if (what == SCANN_OUT_AFTER_LC || what == SCANN_OUT_BF_PROPERTY) {
    if (!(db->out_flags & what))
      return fail(h, SCANN_ERR_INVALID, std::string("scann_output_read: ") + (what == SCANN_OUT_AFTER_LC ? "after_Lc" : "bf_property") +
                                            " was not selected for the batch's last forward");
    n = what == SCANN_OUT_AFTER_LC ? (int64_t)db->n_atom * c.global_dim : (int64_t)db->n_struct * c.dense_out;
  } else {
    return fail(h, SCANN_ERR_INVALID, "scann_output_read: unknown output");
  }
  if (!out) return n;  // the size, without waiting for the forward
  if (cap < n) return fail(h, SCANN_ERR_INVALID, "scann_output_read: " + std::to_string(n) + " floats do not fit a buffer of " + std::to_string(cap));
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[db->last_slot];
  HIPCHK(h, hipStreamSynchronize(s));
  if (const int rp = check_pack_flag(h, db, "scann_output_read")) return rp;
  bool rerun = false;  // (the forward's range guard fired: the outputs come from the exact-fp32 re-run, as y does from scann_batch_download)
  if (const int r = rerun_if_out_of_range(h, db, s, &rerun)) return r;
  if (const int r = check_range(h, "scann_output_read", db->last_slot)) return r;
  const float* src = what == SCANN_OUT_LOCAL_ATTENTION ? attn_out_of(h, db, layer) : what == SCANN_OUT_AFTER_LC ? db->out_z : db->out_bf;
  if (n && src) HIPCHK(h, hipMemcpy(out, src, (size_t)n * 4, hipMemcpyDeviceToHost));
  return n;
}

double scann_mc_drop_scale(uint64_t seed, int32_t t, uint64_t key, uint32_t tag, uint64_t idx, float p) {
  return drop_scale(mc_seed(seed, (unsigned)t, key), tag, (size_t)idx, p);
}

// Monte Carlo dropout: n_samples inference forwards of the resident batch, each with the Dropout layers of the training graph active under
// structure-local masks (scann_internal.h: mc_seed), y and the GlobalAttention scores of sample t written to row t of [T, B] / [T, n_atom]
// buffers in the batch's workspace, and one reduction per output.  The samples' options ask for no selected outputs and no debug buffers and
// send y / ga to those rows, so that later forwards and downloads see what they would have seen.
int scann_predict_mc(scann_handle_t* h, scann_dbatch_t* db, int32_t n_samples, uint64_t seed, const uint64_t* keys, float p_drop, float p_attn,
                     float* y_mean, float* y_std, float* ga_mean, float* ga_std, float* y_samples) {
  if (!h || !db || !y_mean || !y_std) return fail(h, SCANN_ERR_INVALID, "scann_predict_mc: null argument");
  if (n_samples < 2) return fail(h, SCANN_ERR_INVALID, "scann_predict_mc: n_samples must be >= 2 (the standard deviation divides by T - 1)");
  if (p_drop < 0.f) p_drop = 0.1f;  // Dropout(0.1), scann_model.py:374 and attention.py:29
  if (p_attn < 0.f) p_attn = h->attn_drop_p;
  if (!(p_drop < 1.f) || !(p_attn < 1.f)) return fail(h, SCANN_ERR_INVALID, "scann_predict_mc: dropout rates must lie in [0, 1)");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_predict_mc: weights not loaded");
  if (!h->generic && (h->weights_exact || h->force_exact))
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_predict_mc: this handle's forwards run on the exact-fp32 kernels (" +
                                              (h->weights_exact ? h->exact_reason : std::string("SCANN_EXACT=1")) + "), which have no dropout instantiations");
  HIPCHK(h, hipSetDevice(h->device));
  const int T = n_samples, A = db->n_atom, B = db->n_struct;
  const int slot = db->last_slot;  // behind whatever was last enqueued on the batch
  hipStream_t s = h->streams[slot];
  // workspace: rows [A], keys [B], y samples [T, B], ga samples [T, A], means / stds [2 B + 2 A]
  const size_t bR = align_up((size_t)std::max(A, 1) * sizeof(McRow)), bK = align_up((size_t)std::max(B, 1) * 8),
               bY = align_up((size_t)T * B * 4), bG = align_up((size_t)T * A * 4), bO = align_up((size_t)(2 * B + 2 * A + 1) * 4);
  const size_t need = bR + bK + bY + bG + bO;
  if (db->mc_bytes < need) {
    HIPCHK(h, hipStreamSynchronize(s));
    cached_free(db->mc_ws);
    db->mc_ws = nullptr;
    db->mc_bytes = 0;
    HIPCHK(h, cached_malloc((void**)&db->mc_ws, need));
    db->mc_bytes = need;
  }
  char* p = db->mc_ws;
  McRow* rows = reinterpret_cast<McRow*>(p);
  unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(p + bR);
  float* ys = reinterpret_cast<float*>(p + bR + bK);
  float* gs = reinterpret_cast<float*>(p + bR + bK + bY);
  float* outs = reinterpret_cast<float*>(p + bR + bK + bY + bG);
  float *o_ym = outs, *o_ys = outs + B, *o_gm = outs + 2 * B, *o_gs = outs + 2 * B + A;
  HIPCHK(h, wait_upload(db, s));
  if (keys && B > 0) HIPCHK(h, hipMemcpyAsync(d_keys, keys, (size_t)B * 8, hipMemcpyHostToDevice, s));
  launch_mc_rows(db->mol_offset, db->edge_offset, keys ? d_keys : nullptr, B, A, rows, s);
  McState mc{rows, (unsigned long long)seed, 0u, p_drop, p_attn};
  FwdBufs bufs(db);
  FwdOpts o;
  o.mc = &mc;
  o.keep_layers = 0;
  o.out_flags = FWD_OUT_UNTOUCHED;
  o.bufs = &bufs;
  int r = SCANN_OK;
  for (int t = 0; t < T && r == SCANN_OK; ++t) {
    mc.t = (uint32_t)t;
    bufs.y = ys + (size_t)t * B;
    bufs.ga = gs + (size_t)t * A;
    r = run_forward(h, db, s, o);
  }
  if (r == SCANN_OK) {
    launch_mc_reduce(ys, T, B, o_ym, o_ys, s);
    if (ga_mean || ga_std) launch_mc_reduce(gs, T, A, o_gm, o_gs, s);
  }
  const hipError_t se = hipStreamSynchronize(s);
  if (r) return r;
  HIPCHK(h, se);
  HIPCHK(h, hipGetLastError());
  if ((r = check_range(h, "scann_predict_mc", slot))) return r;
  if ((r = check_pack_flag(h, db, "scann_predict_mc"))) return r;
  if (B > 0) {
    HIPCHK(h, hipMemcpy(y_mean, o_ym, (size_t)B * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(y_std, o_ys, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (y_samples) HIPCHK(h, hipMemcpy(y_samples, ys, (size_t)T * B * 4, hipMemcpyDeviceToHost));
  }
  if (A > 0 && ga_mean) HIPCHK(h, hipMemcpy(ga_mean, o_gm, (size_t)A * 4, hipMemcpyDeviceToHost));
  if (A > 0 && ga_std) HIPCHK(h, hipMemcpy(ga_std, o_gs, (size_t)A * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

}  // extern "C"

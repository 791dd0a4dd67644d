// Model sets (scann_models_load / scann_forward_models / scann_models_download): K weight sets of the handle's configuration over one
// resident batch.  Each member is a weight-only handle (its device images, layer pointers and relu_out; the parent's streams and range-guard
// words); on the 128 / 8 kernels their images lie at a fixed stride in one block, so that the SET instantiations reach member m's weights
// as member 0's plus m strides, and their activations likewise in one per-batch block.
#include "scann_runtime.h"

namespace scann {

struct ModelSet {
  std::vector<scann_handle*> member;
  float* block = nullptr;           // 128 / 8 kernels: member m's weight arena + per-species tables at block + m * stride
  size_t stride = 0;                // floats
  std::vector<char> sp_dirty;       // member m's per-species tables are to be computed (first set forward after the load)
  int32_t relu_mask = 0;            // bit m: member m's mrelu
  uint64_t gen = 0;                 // the handle's load number of this set (scann_dbatch::set_gen)
};

namespace {

// A handle that holds weights only: the parent's configuration (relu_out its own), switches and streams; nothing of it is owned but
// what load_weights allocates outside the set's block (generic widths: g_weights, g_centres)
scann_handle* make_member(const scann_handle* h, int relu_out) {
  scann_handle* m = new scann_handle();
  m->cfg = h->cfg;
  m->cfg.relu_out = relu_out;
  m->device = h->device;
  m->generic = h->generic;
  m->specs = h->specs;
  for (int i = 0; i < MAX_STREAM; ++i) m->streams[i] = h->streams[i];
  m->nstream = h->nstream;
  m->tile_atoms = h->tile_atoms;
  m->n_cu = h->n_cu;
  m->xcd_remap = h->xcd_remap;
  m->fuse_basis = h->fuse_basis;
  m->species_tables = h->species_tables;
  m->force_exact = h->force_exact;
  m->strict_range = h->strict_range;
  m->range_flag = h->range_flag;
  return m;
}

void free_member(scann_handle* m) {
  if (!m) return;
  if (m->generic) {
    if (m->g_weights) (void)hipFree(m->g_weights);
    if (m->g_centres) (void)hipFree(m->g_centres);
  }
  delete m;
}

// The batch's set workspace: per member (stride ws) geom [E + 1, 128] (g_update), c0 (ring / cgcnn), c, ctx, P1, P3, q, gq, gk [A, 128],
// part_buf [n_slot, 3, 128]; shared gd [E, 20] (base branch); y [K, B], ga [K, A].  The layout of the batch arena's workspace, per member.
struct SetWs {
  size_t ws = 0;  // bytes between members
  size_t o_geom = 0, o_c0 = 0, o_c = 0, o_ctx = 0, o_P1 = 0, o_P3 = 0, o_q = 0, o_gq = 0, o_gk = 0, o_pbuf = 0;
  size_t o_gd = 0, o_y = 0, o_ga = 0, bytes = 0;
};
SetWs set_layout(const scann_config_t& c, const scann_dbatch* db, int K) {
  SetWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes); return o; };
  const size_t rowA = (size_t)db->n_atom * D * 4, rowE = (size_t)std::max(db->n_edge, 1) * D * 4;
  w.o_geom = take(c.g_update ? rowE + D * 4 : 0);
  w.o_c0 = take((c.use_ring || c.feature_cgcnn) ? rowA : 0);
  w.o_c = take(rowA); w.o_ctx = take(rowA); w.o_P1 = take(rowA); w.o_P3 = take(rowA); w.o_q = take(rowA);
  w.o_gq = take(rowA); w.o_gk = take(rowA);
  w.o_pbuf = take((size_t)db->n_slot * 3 * D * 4);
  w.ws = align_up(off);
  off = w.ws * K;
  w.o_gd = take(c.g_update ? 0 : (size_t)std::max(db->n_edge, 1) * NG * 4);
  w.o_y = take((size_t)K * db->n_struct * 4);
  w.o_ga = take((size_t)K * db->n_atom * 4);
  w.bytes = off + 256;
  return w;
}

// What a set forward repoints of the batch (its workspace, y, ga, the slot whose range-guard word the kernels write) and what a member's
// run_forward changes (the selected outputs, idle / fwd_pending of the batch's single-model work): saved at construction, restored at
// destruction.  So db->last_slot stays the slot of the batch's last SINGLE forward (scann_batch_download waits for that stream and reads
// its range-guard word); the set forward's slot is db->set_slot, and db->set_busy keeps scann_batch_release from freeing the batch
// without a synchronisation until scann_models_download has waited for it
struct BatchView {
  scann_dbatch* db;
  scann_dbatch saved_ptrs;
  explicit BatchView(scann_dbatch* d) : db(d) {
    saved_ptrs.geom = d->geom; saved_ptrs.gd = d->gd; saved_ptrs.c0 = d->c0; saved_ptrs.c = d->c; saved_ptrs.ctx = d->ctx;
    saved_ptrs.P1 = d->P1; saved_ptrs.P3 = d->P3; saved_ptrs.q = d->q; saved_ptrs.gq = d->gq; saved_ptrs.gk = d->gk;
    saved_ptrs.part_buf = d->part_buf; saved_ptrs.y = d->y; saved_ptrs.ga = d->ga; saved_ptrs.last_slot = d->last_slot;
    saved_ptrs.out_attn = d->out_attn; saved_ptrs.out_z = d->out_z; saved_ptrs.out_bf = d->out_bf;
    saved_ptrs.out_layers = d->out_layers; saved_ptrs.out_flags = d->out_flags;
    saved_ptrs.idle = d->idle; saved_ptrs.fwd_pending = d->fwd_pending;
  }
  // member m's slice of the set workspace
  void point(const SetWs& w, int m) {
    char* const b = db->set_ws + (size_t)m * w.ws;
    if (db->geom) db->geom = reinterpret_cast<float*>(b + w.o_geom);
    if (db->c0) db->c0 = reinterpret_cast<float*>(b + w.o_c0);
    db->gd = reinterpret_cast<float*>(db->set_ws + w.o_gd);
    db->c = reinterpret_cast<float*>(b + w.o_c); db->ctx = reinterpret_cast<float*>(b + w.o_ctx);
    db->P1 = reinterpret_cast<float*>(b + w.o_P1); db->P3 = reinterpret_cast<float*>(b + w.o_P3); db->q = reinterpret_cast<float*>(b + w.o_q);
    db->gq = reinterpret_cast<float*>(b + w.o_gq); db->gk = reinterpret_cast<float*>(b + w.o_gk);
    if (db->part_buf) db->part_buf = reinterpret_cast<float*>(b + w.o_pbuf);
    db->y = reinterpret_cast<float*>(db->set_ws + w.o_y) + (size_t)m * db->n_struct;
    db->ga = reinterpret_cast<float*>(db->set_ws + w.o_ga) + (size_t)m * db->n_atom;
  }
  ~BatchView() {
    const scann_dbatch& s = saved_ptrs;
    db->geom = s.geom; db->gd = s.gd; db->c0 = s.c0; db->c = s.c; db->ctx = s.ctx; db->P1 = s.P1; db->P3 = s.P3; db->q = s.q;
    db->gq = s.gq; db->gk = s.gk; db->part_buf = s.part_buf; db->y = s.y; db->ga = s.ga; db->last_slot = s.last_slot;
    db->out_attn = s.out_attn; db->out_z = s.out_z; db->out_bf = s.out_bf; db->out_layers = s.out_layers; db->out_flags = s.out_flags;
    db->idle = s.idle; db->fwd_pending = s.fwd_pending;  // (they describe the batch's single-model work; set work is db->set_busy)
  }
};

int member_fail(scann_handle* h, const scann_handle* m, int r) {
  if (r) h->err = m->err;
  return r;
}

// members [b, b + n) of the set -- all on the split-fp16 kernels -- in one schedule: run_forward's plain inference path (fused first layer,
// per-species tables where it takes them), every launch on the SET instantiations; the batch points at member b's workspace (BatchView)
int run_set(scann_handle* h, ModelSet* ms, scann_dbatch* db, const SetWs& w, hipStream_t s, int b, int n) {
  const scann_config_t& c = h->cfg;
  const int L = c.n_attention;
  const scann_handle* M0 = ms->member[(size_t)b];
  const int64_t wst = (int64_t)(ms->stride * sizeof(float)), ast = (int64_t)w.ws;
  int32_t* const rflag = h->range_flag ? h->range_flag + db->last_slot : nullptr;
  const bool general_embed = c.use_ring || c.feature_cgcnn;
  if (!c.g_update) launch_basis_raw(M0->cd, db->dist, db->n_edge, db->gd, s);  // (the Gaussians of the distances: model independent)
  if (general_embed) {
    for (int m = b; m < b + n; ++m) {
      EmbedArgs e = ms->member[(size_t)m]->embed;
      e.n_atom = db->n_atom; e.atomic = db->atomic;
      e.c0 = reinterpret_cast<float*>(reinterpret_cast<char*>(db->c0) + (m - b) * ast);
      e.ring = c.use_ring ? db->ring : nullptr;
      e.cgcnn = c.feature_cgcnn ? db->cgcnn : nullptr;
      launch_embed(e, s);
    }
  }
  const bool species0 = c.g_update && h->species_tables && !general_embed && M0->sp_c && db->n_big == 0;
  if (species0 && std::any_of(ms->sp_dirty.begin() + b, ms->sp_dirty.begin() + b + n, [](char d) { return d != 0; })) {
    AtomArgs a{};
    a.n_atom = c.n_atoms; a.x = M0->lut; a.ffn = 0; a.c = M0->sp_c;
    a.range_flag = rflag; a.layer = 0;
    const LayerParams& p = M0->layers[0];
    a.mode = 0;
    a.WAh = p.W1h; a.bA = p.bg; a.WBh = p.W3h; a.WCh = p.Wqh; a.bC = p.bq;
    a.oA = M0->sp_P1; a.oB = M0->sp_P3; a.oC = M0->sp_q;
    a.n_member = n; a.m_w = a.m_x = a.m_o = wst;
    launch_atom(a, s);
    HIPCHK(h, hipStreamSynchronize(s));  // once per load: forwards on the handle's other streams read the tables too
    std::fill(ms->sp_dirty.begin() + b, ms->sp_dirty.begin() + b + n, 0);
  }
  for (int l = 0; l <= L; ++l) {
    AtomArgs a{};
    a.n_atom = db->n_atom;
    a.m_x = ast;
    if (l == 0) {
      a.x = general_embed ? db->c0 : M0->lut;
      a.x_index = general_embed ? nullptr : db->atomic;
      a.ffn = 0;
      if (!general_embed) a.m_x = wst;
    } else {
      a.x = db->ctx;
      a.ffn = c.use_attn_norm ? 1 : 0;
      const LayerParams& pp = M0->layers[l - 1];
      a.Wf1h = pp.Wf1h; a.bf1 = pp.bf1; a.Wf2h = pp.Wf2h; a.bf2 = pp.bf2; a.lnr_g = pp.lnr_g; a.lnr_b = pp.lnr_b;
    }
    a.c = db->c;
    a.range_flag = rflag; a.layer = l;
    if (l < L) {
      const LayerParams& p = M0->layers[l];
      a.mode = c.g_update ? 0 : 1;
      a.WAh = p.W1h; a.bA = p.bg; a.WBh = p.W3h; a.WCh = p.Wqh; a.bC = p.bq;
      a.oA = db->P1; a.oB = db->P3; a.oC = db->q;
    } else {
      a.mode = 2;
      a.WAh = M0->head.Wah; a.bA = M0->head.ba; a.WCh = M0->head.Wgqh; a.bC = M0->head.bgq; a.WDh = M0->head.Wgkh; a.bD = M0->head.bgk;
      a.oB = db->gk; a.oC = db->gq;
    }
    a.n_member = n; a.m_w = wst; a.m_o = ast;
    if (!(species0 && l == 0)) launch_atom(a, s);
    if (l == L) break;
    EdgeArgs ea{};
    ea.tiles = db->tiles; ea.n_tile = db->n_tile; ea.g_update = c.g_update; ea.tile_rows = db->tile_rows;
    ea.edge_offset = db->edge_offset; ea.edge_col = db->edge_col; ea.edge_row = db->edge_row;
    ea.geom = db->geom; ea.gd = db->gd; ea.edge_weight = db->weight;
    if (c.g_update && l == 0) { ea.fuse_basis = 1; ea.dist = db->dist; ea.basis = M0->basis; }
    ea.n_edge = db->n_edge;
    ea.geom_rows = c.g_update ? 0 : 1;
    ea.geom_dead = l == L - 1 ? 1 : 0;
    ea.c = db->c; ea.P1 = db->P1; ea.P3 = db->P3; ea.q = db->q; ea.ctx = db->ctx;
    ea.m_r = ast;
    if (species0 && l == 0) { ea.species = db->atomic; ea.c = M0->sp_c; ea.P1 = M0->sp_P1; ea.P3 = M0->sp_P3; ea.q = M0->sp_q; ea.m_r = wst; }
    ea.p = M0->layers[l];
    ea.range_flag = rflag; ea.layer = l;
    ea.tile_part = db->tile_part; ea.part_buf = db->part_buf;
    ea.xcd_remap = h->xcd_remap;
    ea.n_member = n; ea.m_w = wst; ea.m_a = ast;
    launch_edge(ea, s);
    launch_edge_merge_set(db->big_tab, db->n_big, db->part_buf, ea.q, ea.p.ln_g, ea.p.ln_b, ea.ctx, rflag, l, n, ast, wst, s);
  }
  ReadoutArgs r{};
  r.mol_offset = db->mol_offset; r.n_struct = db->n_struct; r.max_atoms = db->max_atoms;
  r.gq = db->gq; r.gk = db->gk; r.use_ga_norm = c.use_ga_norm; r.relu_out = (ms->relu_mask >> b) & ((1 << n) - 1);
  r.p = M0->head; r.ga_attn = db->ga; r.y = db->y;
  r.n_member = n; r.m_w = wst; r.m_a = ast; r.m_g = (int64_t)db->n_atom * 4; r.m_y = (int64_t)db->n_struct * 4;
  launch_readout(r, s);
  HIPCHK(h, hipGetLastError());
  return SCANN_OK;
}

// one forward of every member on stream s: runs of members on the split-fp16 kernels share launches (run_set); a member whose weights need
// the exact-fp32 kernels, generic widths, and the corners run_set has no schedule for run alone through run_forward.  exact: every member on
// the exact-fp32 kernels (the re-run after the range guard fired)
int forward_all(scann_handle* h, ModelSet* ms, scann_dbatch* db, hipStream_t s, int slot, bool exact) {
  const scann_config_t& c = h->cfg;
  const int K = (int)ms->member.size();
  const SetWs w = set_layout(c, db, K);
  if (db->set_busy >= 0 && db->set_busy != slot) {  // an earlier set forward on another stream writes the same block: behind it
    hipEvent_t ev = nullptr;
    HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(ev, h->streams[db->set_busy]));
    const hipError_t e = hipStreamWaitEvent(s, ev, 0);
    (void)hipEventDestroy(ev);  // (released once it has fired)
    HIPCHK(h, e);
  }
  if (db->set_bytes < w.bytes) {
    if (db->set_ws) HIPCHK(h, hipStreamSynchronize(s));  // (the stream, behind any earlier set forward of the batch, may still use the block)
    cached_free(db->set_ws);
    db->set_ws = nullptr;
    db->set_bytes = 0;
    HIPCHK(h, cached_malloc((void**)&db->set_ws, w.bytes));
    db->set_bytes = w.bytes;
  }
  HIPCHK(h, wait_upload(db, s));
  db->set_busy = slot;
  BatchView view(db);
  db->last_slot = slot;  // (the range-guard word the kernels write)
  const bool shared = !exact && !h->generic && !h->force_exact && c.n_attention > 0 && db->n_edge > 0 && (!c.g_update || h->fuse_basis);
  for (int m = 0; m < K;) {
    scann_handle* mh = ms->member[(size_t)m];
    if (shared && !mh->weights_exact) {
      int n = 1;
      while (m + n < K && !ms->member[(size_t)(m + n)]->weights_exact) ++n;
      view.point(w, m);
      if (const int r = run_set(h, ms, db, w, s, m, n)) return r;
      m += n;
    } else {
      view.point(w, m);
      if (const int r = member_fail(h, mh, run_forward(mh, db, s, nullptr, exact))) return r;
      ++m;
    }
  }
  db->set_slot = slot;
  db->set_gen = ms->gen;
  return SCANN_OK;
}

}  // namespace

void free_models(ModelSet* ms) {
  if (!ms) return;
  for (scann_handle* m : ms->member) free_member(m);
  if (ms->block) (void)hipFree(ms->block);
  delete ms;
}

}  // namespace scann

extern "C" {

int scann_models_load(scann_handle_t* h, int32_t n_models, const float* const* blobs, const scann_tensor_desc_t* const* manifests,
                      const int32_t* n_tensors, const int32_t* relu_out) {
  if (!h || !blobs || !manifests || !n_tensors) return fail(h, SCANN_ERR_INVALID, "scann_models_load: null argument");
  if (n_models < 1 || n_models > 16) return fail(h, SCANN_ERR_INVALID, "scann_models_load: n_models must lie in [1, 16]");
  HIPCHK(h, hipSetDevice(h->device));
  std::unique_ptr<ModelSet, void (*)(ModelSet*)> ms(new ModelSet(), free_models);
  ms->sp_dirty.assign((size_t)n_models, 1);
  size_t stride = 0;
  for (int m = 0; m < n_models; ++m) {  // every member validated (and, on the 128 / 8 kernels, sized) before anything is allocated
    const int relu = relu_out ? relu_out[m] : h->cfg.relu_out;
    if (relu != 0 && relu != 1) return fail(h, SCANN_ERR_INVALID, "scann_models_load: relu_out[" + std::to_string(m) + "] must be 0 or 1");
    ms->member.push_back(make_member(h, relu));
    ms->relu_mask |= relu << m;
    scann_handle* mh = ms->member.back();
    if (!blobs[m] || !manifests[m] || n_tensors[m] <= 0)
      return fail(h, SCANN_ERR_INVALID, "scann_models_load: member " + std::to_string(m) + ": null argument");
    if (h->generic) continue;
    size_t need = 0;
    if (const int r = load_weights(mh, blobs[m], manifests[m], n_tensors[m], nullptr, &need))
      return fail(h, r, "scann_models_load: member " + std::to_string(m) + ": " + mh->err);
    stride = std::max(stride, (need + 63) & ~(size_t)63);
  }
  if (!h->generic) {
    HIPCHK(h, hipMalloc((void**)&ms->block, stride * n_models * sizeof(float)));
    ms->stride = stride;
  }
  for (int m = 0; m < n_models; ++m) {
    scann_handle* mh = ms->member[(size_t)m];
    if (const int r = load_weights(mh, blobs[m], manifests[m], n_tensors[m], ms->block ? ms->block + (size_t)m * stride : nullptr, nullptr))
      return fail(h, r, "scann_models_load: member " + std::to_string(m) + ": " + mh->err);
    mh->host_master.clear();  // (a member never trains: no parameter vector to keep)
    mh->host_master.shrink_to_fit();
    mh->descs.clear();
  }
  if (h->models) {
    HIPCHK(h, hipDeviceSynchronize());  // (forwards of the previous set may still be running)
    free_models(h->models);
  }
  ms->gen = ++h->models_gen;
  h->models = ms.release();
  return SCANN_OK;
}

int scann_models_count(const scann_handle_t* h) { return h && h->models ? (int)h->models->member.size() : 0; }

int scann_forward_models(scann_handle_t* h, scann_dbatch_t* db, int stream_slot) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_forward_models: null argument");
  if (!h->models) return fail(h, SCANN_ERR_WEIGHTS, "scann_forward_models: no model set loaded (scann_models_load)");
  HIPCHK(h, hipSetDevice(h->device));
  const int slot = ((stream_slot % h->nstream) + h->nstream) % h->nstream;
  return forward_all(h, h->models, db, h->streams[slot], slot, false);
}

int scann_models_download(scann_handle_t* h, scann_dbatch_t* db, float* y, float* ga) {
  if (!h || !db || !y) return fail(h, SCANN_ERR_INVALID, "scann_models_download: null argument");
  if (!h->models) return fail(h, SCANN_ERR_WEIGHTS, "scann_models_download: no model set loaded (scann_models_load)");
  if (db->set_slot < 0 || db->set_gen != h->models->gen)
    return fail(h, SCANN_ERR_INVALID, "scann_models_download: no forward of the handle's current model set ran on this batch");
  HIPCHK(h, hipSetDevice(h->device));
  const int slot = db->set_slot;
  hipStream_t s = h->streams[slot];
  HIPCHK(h, hipStreamSynchronize(s));
  if (const int r = check_pack_flag(h, db, "scann_models_download")) return r;
  if (h->range_flag && !h->strict_range) {  // the range guard fired: every member again on the exact-fp32 kernels
    const int32_t code = *reinterpret_cast<volatile int32_t*>(h->range_flag + slot);
    const int site = code >> 8;
    if (code && site >= 1 && site <= 4) {
      h->range_flag[slot] = 0;
      if (const int r = forward_all(h, h->models, db, s, slot, true)) return r;
      h->exact_reruns++;
      HIPCHK(h, hipStreamSynchronize(s));
    }
  }
  if (db->set_busy == slot) {
    db->set_busy = -1;
    if (!db->fwd_pending) db->idle = true;  // (the set stream waited for the upload; no single forward is outstanding)
  }
  if (const int r = check_range(h, "scann_models_download", slot)) return r;
  const SetWs w = set_layout(h->cfg, db, (int)h->models->member.size());
  const size_t K = h->models->member.size();
  if (db->n_struct > 0) HIPCHK(h, hipMemcpy(y, db->set_ws + w.o_y, K * db->n_struct * 4, hipMemcpyDeviceToHost));
  if (ga && db->n_atom > 0) HIPCHK(h, hipMemcpy(ga, db->set_ws + w.o_ga, K * db->n_atom * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

}  // extern "C"

// Model sets (scann_models_load / scann_forward_models / scann_models_download): K weight sets of the handle's configuration over one
// resident batch.  Each member is a weight holder (its device images, layer pointers and relu_out) that run_forward is pointed at through
// FwdOpts; streams, switches, range-guard words and errors are the user's handle's.  On the 128 / 8 kernels the images lie at a fixed stride
// in one block, so that the SET instantiations reach member m's weights as member 0's plus m strides, and their activations likewise in
// one per-batch block.  There is no schedule here: a run of members is run_forward with n_member set.
#include "scann_runtime.h"

namespace scann {

struct ModelSet {
  std::vector<scann_handle*> member;
  float* block = nullptr;           // 128 / 8 kernels: member m's weight arena + per-species tables at block + m * stride
  size_t stride = 0;                // floats
  uint64_t gen = 0;                 // the handle's load number of this set (scann_dbatch::set_gen)
};

namespace {

// A handle that holds weights only (FwdOpts::weights / members): what load_weights reads -- the parent's configuration (relu_out its own),
// device, tensor list and the stream it folds the embedding table on; nothing of it is owned but what load_weights allocates outside the
// set's block (generic widths: g_weights, g_centres)
scann_handle* make_member(const scann_handle* h, int relu_out) {
  scann_handle* m = new scann_handle();
  m->cfg = h->cfg;
  m->cfg.relu_out = relu_out;
  m->device = h->device;
  m->generic = h->generic;
  m->specs = h->specs;
  m->streams[0] = h->streams[0];
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

// member m's slice of the set workspace (gd, the base branch's Gaussians, is shared; the batch's own geom, c0, part_buf say which exist)
FwdBufs member_bufs(const scann_dbatch* db, const SetWs& w, int m) {
  FwdBufs f(db);
  char* const b = db->set_ws + (size_t)m * w.ws;
  auto at = [](char* p, size_t o) { return reinterpret_cast<float*>(p + o); };
  if (f.geom) f.geom = at(b, w.o_geom);
  if (f.c0) f.c0 = at(b, w.o_c0);
  f.gd = at(db->set_ws, w.o_gd);
  f.c = at(b, w.o_c); f.ctx = at(b, w.o_ctx); f.P1 = at(b, w.o_P1); f.P3 = at(b, w.o_P3); f.q = at(b, w.o_q);
  f.gq = at(b, w.o_gq); f.gk = at(b, w.o_gk);
  if (f.part_buf) f.part_buf = at(b, w.o_pbuf);
  f.y = at(db->set_ws, w.o_y) + (size_t)m * db->n_struct;
  f.ga = at(db->set_ws, w.o_ga) + (size_t)m * db->n_atom;
  return f;
}

// one forward of every member on stream s: runs of members on the split-fp16 kernels share launches (run_forward with n_member, the SET
// instantiations); a member whose weights need the exact-fp32 kernels, generic widths, and the corners the SET instantiations do not cover
// run alone, as single forwards on that member's weights.  exact: every member on the exact-fp32 kernels (the re-run after the range guard
// fired).  The batch's own workspace, y, ga, selected outputs, last_slot and idle / fwd_pending are not touched: db->last_slot stays the
// slot of the batch's last SINGLE forward (scann_batch_download waits for that stream and reads its range-guard word); the set forward's
// slot is db->set_slot, and db->set_busy keeps scann_batch_release from freeing the batch without a synchronisation until
// scann_models_download has waited for it
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
  db->set_busy = slot;
  FwdOpts o;
  o.exact = exact;
  o.keep_layers = 0;
  o.out_flags = FWD_OUT_UNTOUCHED;
  o.slot = slot;
  o.of_set = true;
  const bool shared = !exact && !h->generic && !h->force_exact && c.n_attention > 0 && db->n_edge > 0 && (!c.g_update || h->fuse_basis);
  for (int m = 0, n = 1; m < K; m += n, n = 1) {
    scann_handle* mh = ms->member[(size_t)m];
    const FwdBufs bufs = member_bufs(db, w, m);
    FwdOpts f = o;
    f.bufs = &bufs;
    if (shared && !mh->weights_exact) {  // members [m, m + n) in one launch sequence
      while (m + n < K && !ms->member[(size_t)(m + n)]->weights_exact) ++n;
      f.n_member = n; f.members = &ms->member[(size_t)m];
      f.m_w = (int64_t)(ms->stride * sizeof(float)); f.m_a = (int64_t)w.ws;
      f.m_y = (int64_t)db->n_struct * 4; f.m_g = (int64_t)db->n_atom * 4;
    } else {
      f.weights = mh;
    }
    if (const int r = run_forward(h, db, s, f)) return r;
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
  size_t stride = 0;
  for (int m = 0; m < n_models; ++m) {  // every member validated (and, on the 128 / 8 kernels, sized) before anything is allocated
    const int relu = relu_out ? relu_out[m] : h->cfg.relu_out;
    if (relu != 0 && relu != 1) return fail(h, SCANN_ERR_INVALID, "scann_models_load: relu_out[" + std::to_string(m) + "] must be 0 or 1");
    ms->member.push_back(make_member(h, relu));
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

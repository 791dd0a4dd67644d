// scann_ablate_pooling (include/scann_hip.h): one forward of the resident batch, then every ablated pooling of one mode from the readout's
// operands gq / gk that the forward left on the device (scann_ablate.hip).  The forward and its download are forward_and_download
// (scann_batch.cpp): y, the GlobalAttention scores, the range guard and the exact re-run behave as in scann_batch_download.
#include "scann_call.h"
#include "scann_runtime.h"

using namespace scann;

extern "C" {

int scann_ablate_pooling(scann_handle_t* h, scann_dbatch_t* db, int32_t mode, float* y, float* ga, float* y_abl, int32_t* order) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_ablate_pooling: null argument");
  if (mode != SCANN_ABLATE_LEAVE_ONE_OUT && mode != SCANN_ABLATE_DELETION && mode != SCANN_ABLATE_INSERTION)
    return fail(h, SCANN_ERR_INVALID, "scann_ablate_pooling: unknown mode " + std::to_string(mode) + " (0 leave-one-out, 1 deletion, 2 insertion)");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_ablate_pooling: weights not loaded");
  const scann_config_t& c = h->cfg;
  // a structure's 32-entry score tile lives in one workgroup's LDS: refuse before anything is launched
  if (db->max_atoms > SCANN_ABLATE_MAX_ATOMS || ablate_lds_bytes(db->max_atoms, c.global_dim) > (size_t)160 * 1024)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_ablate_pooling: a structure of " + std::to_string(db->max_atoms) + " atoms exceeds the limit of " +
                                              std::to_string(SCANN_ABLATE_MAX_ATOMS) + " atoms per structure (32 score rows of one structure in 160 KiB of LDS)");
  const int A = db->n_atom, B = db->n_struct;
  if (const int r = forward_and_download(h, db, 0, 0, y, ga)) return r;
  hipStream_t s = h->streams[db->last_slot];
  AblateArgs a{};
  CallWs ws;
  ws.take(a.y_abl, (size_t)std::max(A, 1)); ws.take(a.order, (size_t)std::max(A, 1));
  HIPCHK(h, ws.alloc());
  a.mol_offset = db->mol_offset; a.n_struct = B; a.max_atoms = db->max_atoms;
  a.dg = c.global_dim; a.dout = c.dense_out; a.use_ga_norm = c.use_ga_norm; a.relu_out = c.relu_out; a.mode = mode;
  if (h->generic) {
    auto W = [&](const char* name) -> const float* { return h->g_weights + h->g_off.at(name); };
    a.gq = db->gen_gq; a.gk = db->gen_gk;
    a.Wb = W("bf_property/kernel"); a.bb = W("bf_property/bias"); a.wo = W("predict_property/kernel"); a.bo = W("predict_property/bias");
  } else {
    a.gq = db->gq; a.gk = db->gk;
    a.Wb = h->head.Wb; a.bb = h->head.bb; a.wo = h->head.wo; a.bo = h->head.bo;
  }
  a.ga_attn = db->ga;
  hipError_t e = A > 0 ? launch_ablate(a, !h->generic, s) : hipSuccess;
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && A > 0 && y_abl) e = hipMemcpy(y_abl, a.y_abl, (size_t)A * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && A > 0 && order) e = hipMemcpy(order, a.order, (size_t)A * 4, hipMemcpyDeviceToHost);
  ws.release();
  HIPCHK(h, e);
  return SCANN_OK;
}

}  // extern "C"

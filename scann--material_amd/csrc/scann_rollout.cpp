// scann_attention_rollout (include/scann_hip.h): one forward of the resident batch with the first `depth` attention maps added to the
// handle's selected outputs, then the maps composed per structure where the forward left them (scann_rollout.hip).  The forward and the
// download are the public ones, so y, the GlobalAttention scores, the range guard and the exact re-run behave exactly as they do there.
#include "scann_runtime.h"

using namespace scann;

namespace {

// atoms per structure of a resident batch, from its device copy of mol_offset (the host keeps none)
int read_mol_offset(scann_handle* h, scann_dbatch* db, std::vector<int32_t>& mol) {
  mol.assign((size_t)db->n_struct + 1, 0);
  if (db->upload_ev && !db->upload_done) HIPCHK(h, hipEventSynchronize(db->upload_ev));
  if (db->n_struct > 0) HIPCHK(h, hipMemcpy(mol.data(), db->mol_offset, mol.size() * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

}  // namespace

extern "C" {

int64_t scann_rollout_floats(scann_handle_t* h, const scann_dbatch_t* db) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_rollout_floats: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> mol;
  if (const int r = read_mol_offset(h, const_cast<scann_dbatch_t*>(db), mol)) return r;
  int64_t n = 0;
  for (int s = 0; s < db->n_struct; ++s) n += (int64_t)(mol[s + 1] - mol[s]) * (mol[s + 1] - mol[s]);
  return n;
}

int scann_attention_rollout(scann_handle_t* h, scann_dbatch_t* db, float residual, int32_t head, int32_t depth, float* y, float* ga,
                            float* attribution, float* rollout) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_attention_rollout: null argument");
  const scann_config_t& c = h->cfg;
  if (!(residual >= 0.f && residual <= 1.f))
    return fail(h, SCANN_ERR_INVALID, "scann_attention_rollout: residual must lie in [0, 1], got " + std::to_string(residual));
  if (head < -1 || head >= c.num_head)
    return fail(h, SCANN_ERR_INVALID, "scann_attention_rollout: head " + std::to_string(head) + " outside -1 .. " + std::to_string(c.num_head - 1));
  if (depth > c.n_attention)
    return fail(h, SCANN_ERR_INVALID, "scann_attention_rollout: depth " + std::to_string(depth) + " exceeds the model's " +
                                          std::to_string(c.n_attention) + " local-attention layers");
  if (depth <= 0) depth = c.n_attention;
  if (depth > 63) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_attention_rollout: more than 63 layers cannot be selected as outputs");
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_attention_rollout: weights not loaded");
  // a structure's column slab lives twice in one workgroup's LDS: refuse before anything is launched
  if (db->max_atoms > SCANN_ROLLOUT_MAX_ATOMS || rollout_lds_bytes(db->max_atoms) > (size_t)160 * 1024)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_attention_rollout: a structure of " + std::to_string(db->max_atoms) + " atoms exceeds the limit of " +
                                              std::to_string(SCANN_ROLLOUT_MAX_ATOMS) + " atoms per structure (two 16-column slabs of one structure in 160 KiB of LDS)");
  const int A = db->n_atom, B = db->n_struct, E = db->n_edge;
  std::vector<float> y_h((size_t)std::max(B, 1)), ga_h((size_t)std::max(A, 1));
  // this one forward also writes layers 0 .. depth-1: the lowest selected layers, so they lie first in the batch's output block.  The
  // re-run of a forward whose range guard fired happens inside the download, under the same selection
  const uint64_t selected = h->out_layers;
  h->out_layers |= (uint64_t(1) << depth) - 1;
  int r = scann_forward_resident(h, db, db->last_slot);
  if (!r) r = scann_batch_download(h, db, y_h.data(), ga_h.data());
  h->out_layers = selected;
  if (r) return r;
  hipStream_t s = h->streams[db->last_slot];
  std::vector<int64_t> off;
  int64_t total = 0;
  if (rollout) {
    std::vector<int32_t> mol;
    if ((r = read_mol_offset(h, db, mol))) return r;
    off.resize((size_t)std::max(B, 1));
    for (int b = 0; b < B; ++b) {
      off[(size_t)b] = total;
      total += (int64_t)(mol[b + 1] - mol[b]) * (mol[b + 1] - mol[b]);
    }
  }
  const size_t bAb = align_up((size_t)depth * std::max(E, 1) * 4), bAt = align_up((size_t)std::max(A, 1) * 4),
               bOf = align_up((size_t)std::max(B, 1) * 8), bR = align_up((size_t)std::max<int64_t>(total, 1) * 4);
  char* ws = nullptr;
  HIPCHK(h, cached_malloc((void**)&ws, bAb + bAt + bOf + bR));
  RolloutArgs a{};
  a.mol_offset = db->mol_offset; a.edge_offset = db->edge_offset; a.edge_col = db->edge_col;
  a.n_struct = B; a.n_edge = E; a.max_atoms = db->max_atoms;
  a.num_head = c.num_head; a.head = head; a.depth = depth; a.residual = residual;
  a.attn = E > 0 ? db->out_attn : nullptr;
  a.ga = db->ga;
  a.abar = reinterpret_cast<float*>(ws);
  a.attribution = reinterpret_cast<float*>(ws + bAb);
  a.roll_offset = reinterpret_cast<const int64_t*>(ws + bAb + bAt);
  a.rollout = rollout ? reinterpret_cast<float*>(ws + bAb + bAt + bOf) : nullptr;
  hipError_t e = hipSuccess;
  if (rollout && B > 0) e = hipMemcpyAsync(ws + bAb + bAt, off.data(), (size_t)B * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && A > 0) e = launch_rollout(a, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && A > 0 && attribution) e = hipMemcpy(attribution, a.attribution, (size_t)A * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && total > 0) e = hipMemcpy(rollout, a.rollout, (size_t)total * 4, hipMemcpyDeviceToHost);
  cached_free(ws);
  HIPCHK(h, e);
  if (y && B > 0) memcpy(y, y_h.data(), (size_t)B * 4);
  if (ga && A > 0) memcpy(ga, ga_h.data(), (size_t)A * 4);
  return SCANN_OK;
}

}  // extern "C"

// scann_attention_rollout (include/scann_hip.h): one forward of the resident batch that writes the first `depth` attention maps besides
// the handle's selected outputs -- its own options say so, the handle is not written -- then the maps composed per structure where the
// forward left them (scann_rollout.hip).  The forward and its download are forward_and_download (scann_batch.cpp): y, the GlobalAttention
// scores, the range guard and the exact re-run behave as in scann_batch_download.
#include "scann_call.h"
#include "scann_runtime.h"

using namespace scann;

extern "C" {

int64_t scann_rollout_floats(scann_handle_t* h, const scann_dbatch_t* db) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_rollout_floats: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> mol;
  if (const int r = read_mol_offset(h, db, mol)) return r;
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
  // this one forward also writes layers 0 .. depth-1: the lowest selected layers, so they lie first in the batch's output block.  The
  // re-run of a forward whose range guard fired happens inside the download, under the selection the batch recorded
  int r = forward_and_download(h, db, (uint64_t(1) << depth) - 1, 0, y, ga);
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
  RolloutArgs a{};
  a.mol_offset = db->mol_offset; a.edge_offset = db->edge_offset; a.edge_col = db->edge_col;
  a.n_struct = B; a.n_edge = E; a.max_atoms = db->max_atoms;
  a.num_head = c.num_head; a.head = head; a.depth = depth; a.residual = residual;
  a.attn = E > 0 ? db->out_attn : nullptr;
  a.ga = db->ga;
  CallWs ws;
  ws.take(a.abar, (size_t)depth * std::max(E, 1)); ws.take(a.attribution, (size_t)std::max(A, 1)); ws.take(a.roll_offset, (size_t)std::max(B, 1));
  ws.take(a.rollout, (size_t)std::max<int64_t>(total, 1));
  HIPCHK(h, ws.alloc());
  if (!rollout) a.rollout = nullptr;
  hipError_t e = hipSuccess;
  if (rollout && B > 0) e = hipMemcpyAsync(writable(a.roll_offset), off.data(), (size_t)B * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && A > 0) e = launch_rollout(a, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && A > 0 && attribution) e = hipMemcpy(attribution, a.attribution, (size_t)A * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && total > 0) e = hipMemcpy(rollout, a.rollout, (size_t)total * 4, hipMemcpyDeviceToHost);
  ws.release();
  HIPCHK(h, e);
  return SCANN_OK;
}

}  // extern "C"

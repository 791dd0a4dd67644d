// scann_shapley (include/scann_hip.h): one forward of the resident batch, then Shapley sampling of the pooling game from the readout's
// operands gq / gk that the forward left on the device (scann_shapley.hip).  The forward and its download are forward_and_download
// (scann_batch.cpp), as in scann_ablate_pooling.  Every refusal comes before anything is launched.
#include "scann_call.h"
#include "scann_runtime.h"

using namespace scann;

extern "C" {

void scann_shapley_permutation(uint64_t seed, uint64_t key, int32_t p, int32_t n, int32_t* out) {
  if (!out || n <= 0 || p < 0) return;
  shapley_permutation(seed, key, p, n, out);
}

int scann_shapley_reduce_host(const float* values, const int32_t* perms, const int32_t* mol_offset, int32_t n_struct, int32_t n_perm,
                              const double* baseline, double* shapley, double* stderr_out, double* full) {
  if (n_struct < 0 || n_perm < 1 || !mol_offset || !baseline || !shapley || !stderr_out || !full)
    return fail(nullptr, SCANN_ERR_INVALID, "scann_shapley_reduce_host: null argument, n_struct < 0 or n_perm < 1");
  if (n_struct > 0 && mol_offset[n_struct] > 0 && (!values || !perms))
    return fail(nullptr, SCANN_ERR_INVALID, "scann_shapley_reduce_host: null argument");
  for (int s = 0; s < n_struct; ++s) {
    const int a0 = mol_offset[s], n = mol_offset[s + 1] - a0;
    if (a0 < 0 || n < 0) return fail(nullptr, SCANN_ERR_INVALID, "scann_shapley_reduce_host: mol_offset must start at >= 0 and not decrease");
    for (int p = 0; p < n_perm; ++p)
      for (int j = 0; j < n; ++j) {
        const int32_t c = perms[(size_t)p * mol_offset[n_struct] + a0 + j];
        if (c < 0 || c >= n) return fail(nullptr, SCANN_ERR_INVALID, "scann_shapley_reduce_host: perms holds an atom outside its structure");
      }
  }
  shapley_reduce_host(values, perms, mol_offset, n_struct, n_perm, baseline, shapley, stderr_out, full);
  return SCANN_OK;
}

}  // extern "C"

// scann_shapley, and with `ms` scann_shapley_profile: the times of the pair kernel, the walks and the reduction between events
static int run_shapley(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, const int32_t* perms_in,
                       float* y, float* ga, double* shapley, double* stderr_out, double* baseline, double* full, float* values,
                       int32_t* perms_out, float* ms) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_shapley: null argument");
  if (n_perm < 1) return fail(h, SCANN_ERR_INVALID, "scann_shapley: n_perm must be >= 1, got " + std::to_string(n_perm));
  if (!h->loaded) return fail(h, SCANN_ERR_WEIGHTS, "scann_shapley: weights not loaded");
  const scann_config_t& c = h->cfg;
  // a structure's 32-entry score tile lives in one workgroup's LDS, as in scann_ablate_pooling
  if (db->max_atoms > SCANN_ABLATE_MAX_ATOMS || ablate_lds_bytes(db->max_atoms, c.global_dim) > (size_t)160 * 1024)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_shapley: a structure of " + std::to_string(db->max_atoms) + " atoms exceeds the limit of " +
                                              std::to_string(SCANN_ABLATE_MAX_ATOMS) + " atoms per structure (32 score rows of one structure in 160 KiB of LDS)");
  const int A = db->n_atom, B = db->n_struct, P = n_perm;
  constexpr size_t GiB = (size_t)1 << 30;
  if (2 * (size_t)P * (size_t)A * 4 > GiB)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_shapley: the values and walks of " + std::to_string(P) + " permutations of a batch of " + std::to_string(B) +
                                              " structures (" + std::to_string(A) + " atoms) exceed 1 GiB of scratch: run fewer structures per batch");
  const int64_t chunks = ((int64_t)P + SHAPLEY_PCHUNK - 1) / SHAPLEY_PCHUNK;
  if (chunks * std::max(B, 1) > INT32_MAX)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_shapley: " + std::to_string(P) + " permutations of a batch of " + std::to_string(B) +
                                              " structures exceed one launch's grid: run fewer structures per batch");
  std::vector<int32_t> mol;
  if (const int r = read_mol_offset(h, db, mol)) return r;
  std::vector<int64_t> off((size_t)std::max(B, 1), 0);
  int64_t total = 0;
  for (int s = 0; s < B; ++s) {
    off[(size_t)s] = total;
    total += (int64_t)(mol[s + 1] - mol[s]) * (mol[s + 1] - mol[s]);
  }
  if ((size_t)total * 4 > GiB)
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_shapley: the pair matrices of a batch of " + std::to_string(B) + " structures (" + std::to_string(A) +
                                              " atoms) exceed 1 GiB of scratch: run fewer structures per batch");
  if (perms_in) {
    std::vector<int64_t> seen((size_t)std::max(db->max_atoms, 1), -1);
    for (int p = 0; p < P; ++p)
      for (int s = 0; s < B; ++s) {
        const int a0 = mol[s], n = mol[s + 1] - a0;
        for (int j = 0; j < n; ++j) {
          const int32_t v = perms_in[(size_t)p * A + a0 + j];
          if (v < 0 || v >= n || seen[(size_t)v] == (int64_t)p * B + s)
            return fail(h, SCANN_ERR_INVALID, "scann_shapley: row " + std::to_string(p) + " of perms_in is not a permutation of the " +
                                                  std::to_string(n) + " atoms of structure " + std::to_string(s));
          seen[(size_t)v] = (int64_t)p * B + s;
        }
      }
  }
  if (const int r = forward_and_download(h, db, 0, 0, y, ga)) return r;
  hipStream_t st = h->streams[db->last_slot];
  ShapleyArgs a{};
  a.mol_offset = db->mol_offset; a.n_struct = B; a.n_atom = A; a.max_atoms = db->max_atoms; a.n_perm = P;
  a.dg = c.global_dim; a.dout = c.dense_out; a.use_ga_norm = c.use_ga_norm; a.relu_out = c.relu_out;
  if (h->generic) {
    auto W = [&](const char* name) -> const float* { return h->g_weights + h->g_off.at(name); };
    a.gq = db->gen_gq; a.gk = db->gen_gk;
    a.Wb = W("bf_property/kernel"); a.bb = W("bf_property/bias"); a.wo = W("predict_property/kernel"); a.bo = W("predict_property/bias");
  } else {
    a.gq = db->gq; a.gk = db->gk;
    a.Wb = h->head.Wb; a.bb = h->head.bb; a.wo = h->head.wo; a.bo = h->head.bo;
  }
  a.seed = seed;
  const size_t nV = (size_t)P * std::max(A, 1), nB = (size_t)std::max(B, 1), nA = (size_t)std::max(A, 1);
  int32_t* d_in;
  int64_t* d_off;
  unsigned long long* d_keys;
  CallWs ws;
  ws.take(a.values, nV); ws.take(a.perms, nV); ws.take(d_in, perms_in ? nV : 0); ws.take(a.pair, (size_t)std::max<int64_t>(total, 1));
  ws.take(d_off, nB); ws.take(d_keys, nB); ws.take(a.baseline, nB); ws.take(a.full, nB); ws.take(a.shapley, nA); ws.take(a.stderr_out, nA);
  HIPCHK(h, ws.alloc());
  a.pair_offset = d_off;
  a.keys = keys ? d_keys : nullptr;
  a.perms_in = perms_in ? d_in : nullptr;
  hipError_t e = hipSuccess;
  hipEvent_t ev[4] = {};
  for (int i = 0; ms && i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  if (e == hipSuccess && B > 0) e = hipMemcpyAsync(d_off, off.data(), (size_t)B * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && keys && B > 0) e = hipMemcpyAsync(d_keys, keys, (size_t)B * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && perms_in && A > 0) e = hipMemcpyAsync(d_in, perms_in, (size_t)P * A * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_shapley(a, !h->generic, st, ms ? ev : nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (int i = 0; ms && i < 3; ++i) {
    ms[i] = 0.f;
    if (e == hipSuccess && B > 0) e = hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  }
  for (int i = 0; i < 4; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  if (e == hipSuccess && B > 0 && baseline) e = hipMemcpy(baseline, a.baseline, (size_t)B * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && B > 0 && full) e = hipMemcpy(full, a.full, (size_t)B * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && A > 0 && shapley) e = hipMemcpy(shapley, a.shapley, (size_t)A * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && A > 0 && stderr_out) e = hipMemcpy(stderr_out, a.stderr_out, (size_t)A * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && A > 0 && values) e = hipMemcpy(values, a.values, (size_t)P * A * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && A > 0 && perms_out) e = hipMemcpy(perms_out, a.perms, (size_t)P * A * 4, hipMemcpyDeviceToHost);
  ws.release();
  HIPCHK(h, e);
  return SCANN_OK;
}

extern "C" {

int scann_shapley(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, const int32_t* perms_in,
                  float* y, float* ga, double* shapley, double* stderr_out, double* baseline, double* full, float* values, int32_t* perms_out) {
  return run_shapley(h, db, n_perm, seed, keys, perms_in, y, ga, shapley, stderr_out, baseline, full, values, perms_out, nullptr);
}

int scann_shapley_profile(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, float* ms) {
  if (!ms) return fail(h, SCANN_ERR_INVALID, "scann_shapley_profile: null argument");
  return run_shapley(h, db, n_perm, seed, keys, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ms);
}

}  // extern "C"

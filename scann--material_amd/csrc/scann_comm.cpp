// Data-parallel training over RCCL: the communicator, the initial weight broadcast and the all-reduces of a step.
#include "scann_runtime.h"

extern "C" {

int scann_comm_unique_id(char* out128) {
  if (!out128) return SCANN_ERR_INVALID;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return SCANN_ERR_HIP;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, 128);
  return SCANN_OK;
}

int scann_comm_init(scann_handle_t* h, const char* id128, int rank, int world) {
  if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return fail(h, SCANN_ERR_INVALID, "scann_comm_init: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  if (h->comm) { ncclCommDestroy(h->comm); h->comm = nullptr; }
  const ncclResult_t r = ncclCommInitRank(&h->comm, world, id, rank);
  if (r != ncclSuccess) return fail(h, SCANN_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  h->comm_world = world;
  return SCANN_OK;
}

int scann_comm_ranks(scann_handle_t* h) {
  if (!h) return SCANN_ERR_INVALID;
  if (!h->comm) return 0;
  int n = 0;
  const ncclResult_t r = ncclCommCount(h->comm, &n);  // what RCCL itself says the communicator spans
  if (r != ncclSuccess) return fail(h, SCANN_ERR_HIP, std::string("ncclCommCount: ") + ncclGetErrorString(r));
  return n;
}

int scann_broadcast_weights(scann_handle_t* h, int root) {
  if (!h || !h->t_master) return fail(h, SCANN_ERR_INVALID, "scann_broadcast_weights: call scann_train_begin first");
  if (!h->comm || h->comm_world == 1) return SCANN_OK;
  if (root < 0 || root >= h->comm_world) return fail(h, SCANN_ERR_INVALID, "scann_broadcast_weights: bad root");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->streams[0];
  const ncclResult_t r = ncclBroadcast(h->t_master, h->t_master, h->host_master.size(), ncclFloat, root, h->comm, s);
  if (r != ncclSuccess) return fail(h, SCANN_ERR_HIP, std::string("ncclBroadcast: ") + ncclGetErrorString(r));
  if (h->generic) {
    HIPCHK(h, hipMemcpyAsync(h->g_weights, h->t_master, h->host_master.size() * 4, hipMemcpyDeviceToDevice, s));
  } else {
    launch_repack(h->t_descs, (int)h->descs.size(), h->t_master, h->d_weights, h->range_flag, s);
    h->sp_dirty = true;
    if (!h->cfg.use_ring && !h->cfg.feature_cgcnn)
      launch_embed_lut(h->d_weights + h->o_emb, h->d_weights + h->o_Wde, h->d_weights + h->o_bde, h->cfg.n_atoms,
                       h->cfg.embedding_dim, h->d_weights + h->o_lut, s);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(h->host_master.data(), h->t_master, h->host_master.size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return SCANN_OK;
}

int scann_allreduce_grads(scann_handle_t* h) {
  if (!h || !h->t_grad) return fail(h, SCANN_ERR_INVALID, "scann_allreduce_grads: no training state");
  if (!h->comm || h->comm_world == 1) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  // one fused flat all-reduce (890,977 floats = 3.56 MB at the QM9 config): latency-bound on xGMI, so a single call
  const ncclResult_t r = ncclAllReduce(h->t_grad, h->t_grad, h->host_master.size(), ncclFloat, ncclSum, h->comm, h->streams[0]);
  if (r != ncclSuccess) return fail(h, SCANN_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  return SCANN_OK;
}

int scann_allreduce_sse(scann_handle_t* h, double* sse, int64_t* count) {
  if (!h || !sse || !count) return SCANN_ERR_INVALID;
  if (!h->comm || h->comm_world == 1) return SCANN_OK;
  HIPCHK(h, hipSetDevice(h->device));
  double* d = nullptr;
  HIPCHK(h, cached_malloc((void**)&d, 2 * sizeof(double)));
  const double v[2] = {*sse, (double)*count};
  HIPCHK(h, hipMemcpy(d, v, sizeof(v), hipMemcpyHostToDevice));
  const ncclResult_t r = ncclAllReduce(d, d, 2, ncclDouble, ncclSum, h->comm, h->streams[0]);
  if (r != ncclSuccess) { cached_free(d); return fail(h, SCANN_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r)); }
  double o[2];
  HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  HIPCHK(h, hipMemcpy(o, d, sizeof(o), hipMemcpyDeviceToHost));
  cached_free(d);
  *sse = o[0];
  *count = (int64_t)(o[1] + 0.5);
  return SCANN_OK;
}

}  // extern "C"

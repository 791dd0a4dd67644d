/*
 * scann_hip.h -- C ABI of libscann_hip.so: the MI355X (gfx950) implementation of the SCANN / SCANN+
 * forward hot path.
 *
 * The reference (sinhvt3421/scann--material) has no FFI: its hot path is the Keras graph built by
 * scann/models/scann_model.py:329-453 (create_model) and executed by `model.predict(inputs)`
 * (scann_model.py:266,316).  This header is the boundary that replaces that graph execution; the
 * Python facade (`scann--material_amd/scann`, class SCANN, `.model.predict`) binds it with ctypes.
 * Each entry point names the reference interface it stands in for.
 *
 * Conventions: every function returns 0 on success or a negative scann_status code and never
 * throws; all host buffers are caller-owned plain pointers; the library owns device memory.
 * One handle per GPU; a handle is not thread-safe, distinct handles are.
 */
#ifndef SCANN_HIP_H
#define SCANN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCANN_ABI_VERSION 1

typedef enum scann_status {
  SCANN_OK = 0,
  SCANN_ERR_INVALID = -1,     /* bad argument / malformed batch (index out of range, ...) */
  SCANN_ERR_UNSUPPORTED = -2, /* configuration outside what the kernels implement */
  SCANN_ERR_NO_DEVICE = -3,   /* no HIP device / device_id out of range */
  SCANN_ERR_HIP = -4,         /* a HIP runtime call failed (see scann_last_error) */
  SCANN_ERR_WEIGHTS = -5,     /* weights missing / wrong shape / not loaded */
  SCANN_ERR_OOM = -6,
  SCANN_ERR_RANGE = -7        /* an activation or a weight left the range of the split-fp16 projections (|x| < 65504, |w| < 255.9):
                                 the results of the call are not valid; scann_last_error names the layer and the site */
} scann_status;

/* Model hyper-parameters: the `model:` section of configs/ *.yaml as read by create_model
 * (scann_model.py:330-447).  Keys not listed there (e.g. `scale`) are never read by the reference. */
typedef struct scann_config {
  int32_t n_atoms;        /* Embedding vocabulary, scann_model.py:362 */
  int32_t embedding_dim;  /* :362 */
  int32_t local_dim;      /* :373  (128 with num_head 8, global_dim 128, dense_out 128 = every shipped yaml: the MFMA kernels; */
  int32_t num_head;       /* :399   any other widths: the plain-fp32 kernels of scann_generic*.hip, ~10 x slower) */
  int32_t n_attention;    /* :413 */
  int32_t global_dim;     /* :425 */
  int32_t dense_out;      /* :438 */
  int32_t n_gauss;        /* 20, scann_model.py:378 */
  float gaussian_d;       /* :378 */
  int32_t g_update;       /* :380  SCANN+ geometry update */
  int32_t use_attn_norm;  /* :404  ResidualNorm after each LocalAttention */
  int32_t use_ga_norm;    /* :433  GlobalAttention(norm=...) */
  int32_t use_ring;       /* :356  extra ring/aromatic input */
  int32_t feature_cgcnn;  /* :334  92-d CGCNN features instead of the Embedding */
  int32_t relu_out;       /* :446  mrelu on the output iff hyper.target == "e_b" */
} scann_config_t;

/* One named fp32 tensor inside a flat weight blob (the library's weight container; replaces the
 * Keras HDF5 checkpoint read by load_model, scann_model.py:79,87,323).  Names are listed by
 * scann_weight_name(); kernels are stored [in, out] like Keras Dense kernels. */
typedef struct scann_tensor_desc {
  const char* name;
  int64_t offset; /* element offset into the blob */
  int64_t numel;
} scann_tensor_desc_t;

/* A batch in packed (CSR) form.  The padded Keras input dict (scann_model.py:338-357; produced by
 * DataIterator.__getitem__, datagenerator.py:123-133) maps to it as: real atoms (atom_mask) of all
 * structures concatenated; per atom its unmasked neighbour slots in slot order; neighbour ids made
 * global (structure offset + neighbors[b, a, n], the job of gather_shape, custom_layers.py:18-28). */
typedef struct scann_batch {
  int32_t n_struct;           /* B */
  int32_t n_atom;             /* sum of real atoms */
  int32_t n_edge;             /* sum of unmasked neighbour slots */
  const int32_t* atomic;      /* [n_atom]  atomic number / embedding row ("atomic") */
  const int32_t* mol_offset;  /* [n_struct + 1] first atom of each structure */
  const int32_t* edge_offset; /* [n_atom + 1]  CSR row pointers */
  const int32_t* edge_col;    /* [n_edge] global atom row of the neighbour */
  const float* edge_dist;     /* [n_edge] "neighbor_distance" */
  const float* edge_weight;   /* [n_edge] "neighbor_weight" */
  const float* ring;          /* [n_atom, 2] "ring_aromatic" or NULL */
  const float* cgcnn;         /* [n_atom, 92] CGCNN features or NULL */
} scann_batch_t;

typedef struct scann_handle scann_handle_t;
typedef struct scann_dbatch scann_dbatch_t; /* a batch resident in HBM with its own workspace */

/* Per-kernel device timing of one forward (HIP events on the handle's stream). */
typedef struct scann_profile {
  float ms_basis;     /* embed + edge basis MLP            (scann_model.py:362-389) */
  float ms_atom;      /* sum over layers: atom-tile kernel (attention.py:37-40,160 + split filter_geo) */
  float ms_edge;      /* sum over layers: edge-tile kernel (attention.py:136-216) */
  float ms_readout;   /* after_Lc + GlobalAttention + head (scann_model.py:424-447) */
  float ms_total;
  int32_t n_edge_launch; /* number of edge-kernel launches timed (= n_attention) */
  int32_t n_atom_launch;
  int32_t reserved;
} scann_profile_t;

int scann_abi_version(void);
int scann_device_count(void);

/* Replaces create_model(config) (scann_model.py:329).  local_dim = global_dim = dense_out = 128 with num_head = 8 (every shipped
 * reference yaml) runs on the split-fp16 MFMA kernels; any other widths the reference accepts (scann_model.py:330-434; here: each
 * <= 1024, local_dim a multiple of num_head) evaluate AND train on the plain-fp32 kernels of csrc/scann_generic.hip /
 * csrc/scann_generic_train.hip -- same entry points, same packed batch, about ten times slower at equal width (a training step
 * about seven times).  Env SCANN_GENERIC=1 forces that path for a 128 / 8 handle (the cross-check of tests/test_gpu_parity.py and
 * tests/test_gpu_training.py). */
int scann_create(const scann_config_t* cfg, int device_id, scann_handle_t** out);
void scann_destroy(scann_handle_t* h);
const char* scann_last_error(const scann_handle_t* h); /* h may be NULL: last create error */

/* Canonical tensor list for this configuration (index 0..n-1); shape as up to 2 dims. */
int scann_weight_count(const scann_handle_t* h);
int scann_weight_name(const scann_handle_t* h, int index, const char** name, int64_t* rows, int64_t* cols);

/* Replaces load_model / model.set_weights (scann_model.py:79,323). */
int scann_load_weights(scann_handle_t* h, const float* blob, const scann_tensor_desc_t* manifest, int n);

/* Replaces model.predict(inputs) (scann_model.py:266,316) on host buffers:
 * y_out[n_struct]; ga_attn_out[n_atom] (packed GlobalAttention scores, attention.py:302) or NULL. */
int scann_forward(scann_handle_t* h, const scann_batch_t* batch, float* y_out, float* ga_attn_out);

/* The same on the PADDED Keras input dict itself (scann_model.py:338-357; DataIterator.__getitem__,
 * datagenerator.py:123-133): atomic[B,M] int32, atom_mask[B,M] bytes (bool), neighbors[B,M,N] int32,
 * neighbor_mask[B,M,N] bytes, neighbor_weight / neighbor_distance [B,M,N] float.  Packing to CSR (what gather_shape +
 * the masks express, custom_layers.py:18-28) is done natively; ga_out[B*M] (or NULL) receives the GlobalAttention scores
 * re-padded with exact zeros for padded atoms.  feature="atomic" without ring features only. */
int scann_forward_padded(scann_handle_t* h, int32_t B, int32_t M, int32_t N, const int32_t* atomic,
                         const uint8_t* atom_mask, const int32_t* neighbors, const uint8_t* neighbor_mask,
                         const float* neighbor_weight, const float* neighbor_distance, float* y_out, float* ga_out);

/* Resident-batch path (inputs already in HBM; used for pipelined inference and by bench.py).  scann_batch_upload validates the
 * CSR arrays, plans the edge tiles, copies the inputs into a pinned staging buffer of the handle and returns when the copy to the
 * device is ENQUEUED on a stream of its own: the caller's arrays may be reused at once, and whatever is launched on the batch
 * afterwards waits for the copy through the batch's event.  May be called from a second thread while the handle's owner thread
 * launches and fetches other batches (HipModel.predict_dataset, trainer.fit do). */
int scann_batch_upload(scann_handle_t* h, const scann_batch_t* batch, scann_dbatch_t** out);
/* The same, from the PADDED Keras input arrays (scann_model.py:338-357; shapes as scann_forward_padded; masks of 1-byte bool / uint8
 * or 4-byte float32 / int32 elements): the host reads the masks only (real atoms, neighbour counts -> offsets -> edge-tile plan), the
 * payload arrays are copied to the device as they are and packed to CSR there (pack_padded_kernel; replaces the host loop
 * DataIterator.__getitem__ + gather_shape amount to, datagenerator.py:69-135, custom_layers.py:18-28).  What the host packer refuses at
 * packing time -- an unmasked slot that points at a padded atom, an atomic number outside the embedding table -- is reported by
 * scann_batch_download of this batch (SCANN_ERR_INVALID).  feature="atomic" without ring features, inference handles.
 * n_atom_out / n_edge_out (or NULL) receive the packed counts.  scann_batch_read_csr copies the packed arrays of a resident batch back
 * (any pointer may be NULL): the test hook behind "device packing == scann_pack_padded, byte for byte". */
int scann_upload_padded(scann_handle_t* h, int32_t B, int32_t M, int32_t N, const int32_t* atomic, const void* atom_mask,
                        int32_t atom_mask_size, const int32_t* neighbors, const void* neighbor_mask, int32_t neighbor_mask_size,
                        const float* neighbor_weight, const float* neighbor_distance, scann_dbatch_t** out, int32_t* n_atom_out,
                        int32_t* n_edge_out);
int scann_batch_read_csr(scann_handle_t* h, scann_dbatch_t* db, int32_t* atomic, int32_t* mol_offset, int32_t* edge_offset,
                         int32_t* edge_col, float* edge_dist, float* edge_weight);
void scann_batch_free(scann_handle_t* h, scann_dbatch_t* db);
void scann_batch_release(scann_handle_t* h, scann_dbatch_t* db); /* see scann_train_step_begin */
int scann_forward_resident(scann_handle_t* h, scann_dbatch_t* db, int stream_slot); /* async */
int scann_batch_download(scann_handle_t* h, scann_dbatch_t* db, float* y_out, float* ga_attn_out); /* syncs that batch */
/* out8 = { structures, atoms, edges, atoms with more than 64 neighbours, their softmax-merge slots, largest neighbour count, edge tiles
 * and rows per tile (32 | 64) of the batch's tile plan }. */
int scann_batch_info(scann_handle_t* h, const scann_dbatch_t* db, int32_t* out8);
int scann_sync(scann_handle_t* h); /* all streams of the handle */
/* hipMemGetInfo of the handle's device: what is left of the 288 GB for resident batches (the library keeps freed blocks in a
 * per-device cache, so `free` does not rise when a batch is released; it must not FALL across repeated calls of one shape). */
int scann_device_memory(scann_handle_t* h, int64_t* free_bytes, int64_t* total_bytes);
/* Inference forwards whose range guard fired -- an activation left the range of the split-fp16 projections (|x| < 65504) -- are run
 * again by scann_batch_download / scann_forward on exact-fp32 matrix instructions (v_mfma_f32_32x32x2_f32, the arithmetic of the
 * reference's fp32 Dense layers, attention.py:95-113) instead of returning SCANN_ERR_RANGE; this counts them.  Env
 * SCANN_STRICT_RANGE=1 turns the re-run off (the error is returned).  Training entry points always return the error. */
int64_t scann_exact_reruns(const scann_handle_t* h);
/* 1 if every inference forward of the handle runs on the exact-fp32 kernels because of its checkpoint: a 128x128 kernel with
 * |w| >= 255.9, or an operand of a split-fp16 projection that stays below the scheme's low end -- a kernel column below 2^-16
 * throughout, or operand rows whose largest element the loaded tensors keep below 2^-8: LayerNorm outputs, the first layer's centres
 * and geometry, the key projection's centres x geometry product, the swish rows of the ResidualNorm and of after_Lc (there a hi + lo
 * pair has an absolute quantum of 2^-25, not 22 significant bits).  Decided by scann_load_weights, not repeated after optimiser steps.  Such a handle refuses to train, to sample MC
 * dropout, to return input gradients or per-layer intermediates, with an error that names the tensor.  0 otherwise. */
int scann_weights_exact(const scann_handle_t* h);
int scann_num_streams(const scann_handle_t* h);

/* ---- outputs beyond y and the GlobalAttention scores (what a user of the reference reads through a Keras sub-model, as
 * load_model_infer does for the GlobalAttention scores, scann_model.py:86-91) ----
 * scann_set_outputs selects what the handle's later INFERENCE forwards also write into each batch's own workspace: bit k of
 * attn_layers = the attention weights of LocalAttention layer k ("local_attention_<k>", attention.py:189); flags = SCANN_OUT_AFTER_LC
 * (the representation of each local structure, scann_model.py:423-429) | SCANN_OUT_BF_PROPERTY (the structure vector fed to the
 * head, :437-442).  A layer >= n_attention or an unknown flag is SCANN_ERR_INVALID.  (0, 0) -- the default -- selects nothing: a
 * forward then launches exactly the kernels it launches without outputs.  Training forwards ignore the selection.  The buffers are
 * allocated on the first forward of a batch that needs them and freed with the batch.  On the 128-wide kernels, attention weights
 * of a g_update model need the fused first layer: a forward with scann_set_debug on or SCANN_FUSE_BASIS=0 is SCANN_ERR_UNSUPPORTED.
 * scann_output_read copies one output of the batch's last forward to host, once that forward has finished (it waits for it; a forward
 * whose range guard fired is re-run on the exact-fp32 kernels first, as scann_batch_download does): what = SCANN_OUT_LOCAL_ATTENTION
 * (layer k) -> [n_edge, num_head] in packed edge order, every atom's weights summing to 1 per head; SCANN_OUT_AFTER_LC ->
 * [n_atom, global_dim]; SCANN_OUT_BF_PROPERTY -> [n_struct, dense_out].  `cap` = floats `out` holds; returns the number of floats
 * copied (out == NULL: the number it would copy) or a negative status -- SCANN_ERR_INVALID if the output was not selected for the
 * batch's last forward or does not fit. */
#define SCANN_OUT_LOCAL_ATTENTION 0
#define SCANN_OUT_AFTER_LC 1
#define SCANN_OUT_BF_PROPERTY 2
int scann_set_outputs(scann_handle_t* h, uint64_t attn_layers, int32_t flags);
int64_t scann_output_read(scann_handle_t* h, scann_dbatch_t* db, int32_t what, int32_t layer, float* out, int64_t cap);

/* Timed forward of a resident batch: HIP events around every kernel on its stream. */
int scann_forward_profile(scann_handle_t* h, scann_dbatch_t* db, scann_profile_t* prof);

/* Live kernel timing inside a pipelined run: while enabled, every `every`-th forward brackets each of its edge-kernel
 * launches (not the first layer's launch of an inference forward, which has the basis MLP fused in: a different kernel) with
 * HIP events on the launch stream.  scann_edge_timing_read (after scann_sync) returns the average launch
 * duration in microseconds and the number of launches sampled, and clears the samples. */
int scann_edge_timing(scann_handle_t* h, int every);
int scann_edge_timing_read(scann_handle_t* h, double* avg_us, int64_t* n_launches, double* avg_edges);

/* Test hook: copy an intermediate of the last forward of `db` to host.
 * what: 0 = centers after layer `layer` (0 = after dense_embed) [n_atom,128];
 *       1 = geometry features after layer `layer` [n_edge,128];
 *       2 = context (LocalAttention output incl. layer_norm) of layer `layer`>=1 [n_atom,128];
 *       3, 5, 7 (after scann_train_forward only) = K, V [n_edge,128] and q [n_atom,128] kept for the backward by LocalAttention
 *       `layer`>=1;  4, 6 = ang, T [n_edge,128]: kept only when the modular backward runs (env SCANN_TRAIN_FUSED=0) -- the fused
 *       backward forms them again from (c, geometry) and (V, geometry) -- otherwise SCANN_ERR_UNSUPPORTED.
 * Only valid when the forward was run with scann_set_debug(h, 1) (keeps per-layer copies). */
int scann_set_debug(scann_handle_t* h, int on);
int scann_debug_read(scann_handle_t* h, scann_dbatch_t* db, int what, int layer, float* out);
/* Test hook, plain-fp32 (generic-width) training only: copy a tensor of the readout's backward of the last scann_train_backward on
 * `db` to host -- name one of "gq", "gk", "z" [n_atom, global_dim] (kept by the forward), "rep" [n_struct, global_dim],
 * "drep" [n_struct, global_dim], "dgq", "dgk", "dz" [n_atom, global_dim] (dz: gradient of after_Lc's pre-activation).  `cap` = floats `out` holds; returns the number of floats copied or a negative status. */
int64_t scann_train_debug_read(scann_handle_t* h, scann_dbatch_t* db, const char* name, float* out, int64_t cap);

/* Diagnostic builds (-DSCANN_STAMPS) only: per-tile phase clocks [n_tile, 16] of the last edge-kernel launch of
 * `db`; returns the number of tiles copied.  The shipped library returns SCANN_ERR_UNSUPPORTED. */
int scann_debug_stamps(scann_handle_t* h, scann_dbatch_t* db, uint64_t* out, int max_tiles);

/* ---- training step: replaces model.compile(loss=rmse, Adam(lr, decay=1e-5)) + model.fit (scann_model.py:199-241) ----
 * Gradients are hand-written derivatives of the forward graph; parameters, gradients and Adam moments are flat fp32
 * vectors in scann_weight_name() order.  Every architecture switch of create_model is covered (g_update on/off,
 * use_attn_norm, use_ga_norm, use_ring, feature="cgcnn", target "e_b"), at the shipped widths (128 / 8: MFMA kernels) and at any
 * other widths scann_create accepts (plain-fp32 kernels, every sum in a fixed order: a step is bit-reproducible on both).
 * Data-parallel use: every rank calls forward on its shard, the SSE / count are summed over ranks (host side or
 * scann_allreduce_sse), then backward, scann_allreduce_grads (one flat RCCL all-reduce), scann_adam_step. */
int64_t scann_param_count(const scann_handle_t* h);
int scann_train_begin(scann_handle_t* h);
/* training-mode forward on stream 0: keeps per-layer activations in `db`; `dropout` = rate of the two Dropout(0.1)
 * layers (scann_model.py:374, attention.py:29), 0 disables; targets[n_struct]; *sse_out = sum (y - target)^2 of this batch */
int scann_train_forward(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, uint64_t seed, double* sse_out);
/* accumulates d(rmse)/d(params) into the gradient vector; rmse = sqrt(sse_global / count_global) (losses.py:5-6) */
int scann_train_backward(scann_handle_t* h, scann_dbatch_t* db, double sse_global, int64_t count_global);
/* model.use_drop (train.py --use_drop): Dropout(0.05) on the local-attention weights during training forwards
 * (attention.py:116,191); 0 disables.  Both branches (g_update on / off), MFMA and plain-fp32 kernels alike. */
int scann_set_attention_dropout(scann_handle_t* h, float p);
/* on != 0: deterministic training mode, from the next scann_train_backward / scann_train_step[_begin] on (it may be switched
 * between steps).  The six small gradient reductions of the 128-wide backward that otherwise end in float atomics (readout bias,
 * basis MLP, base-branch filter_geo, embedding table, dense_embed, ring / cgcnn embedding) store per-workgroup partial sums and
 * add them in a fixed order over a partition that depends on the batch shape only: a step's gradients, and so its weights, are
 * then bitwise the same on every run.  Their slots live in the batch's training workspace (allocated on the batch's first
 * deterministic backward, freed with the batch).  Plain-fp32 handles (other widths) are deterministic already and ignore it, as do
 * inference forwards.  Across ranks the gradient all-reduce keeps RCCL's order. */
int scann_set_deterministic(scann_handle_t* h, int on);
int scann_zero_grads(scann_handle_t* h);
int scann_allreduce_grads(scann_handle_t* h);                 /* RCCL sum over the communicator; no-op without one */
int scann_allreduce_sse(scann_handle_t* h, double* sse, int64_t* count); /* in-place sum over ranks */
/* g += 2*l2*w on the regularised kernels, then Adam (epsilon outside the sqrt, as tf.keras); lr_t already includes the
 * schedule and the legacy decay 1/(1 + 1e-5*iterations); refreshes the packed device weights */
int scann_adam_step(scann_handle_t* h, float lr_t, float beta1, float beta2, float eps, float l2);
/* One whole optimisation step, asynchronous until its end: scann_train_forward, [sum of {sse, count} over the communicator],
 * scann_zero_grads, scann_train_backward with the loss scale formed on the device, scann_allreduce_grads, scann_adam_step -- the
 * same kernels and results, without the host round trips between them (one fit step of model.fit, scann_model.py:225-241).
 * *sse_out / *count_out = the GLOBAL batch's sum of squared errors and size.  Adam leaves the gradient vector zeroed (the next step
 * needs no scann_zero_grads; scann_get_grads after a step returns zeros). */
int scann_train_step(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, uint64_t seed, float lr_t, float beta1,
                     float beta2, float eps, float l2, double* sse_out, int64_t* count_out);
/* The same step in two halves: _begin enqueues everything and returns; _end waits for the OLDEST step in flight and returns its
 * {sse, count, sum |y - target|} (global over the communicator).  Up to TWO steps may be in flight: the host assembles, uploads
 * (scann_batch_upload copies on a stream of its own; the step waits for the batch's copy event) and begins step k + 1 while the
 * device still runs step k, so the device never waits for the host.  A batch must not be freed or downloaded before the _end of
 * its step; scann_batch_release then frees it without the device-wide synchronisation of scann_batch_free.  The gradient vector
 * is left zeroed. */
int scann_train_step_begin(scann_handle_t* h, scann_dbatch_t* db, const float* targets, float dropout, uint64_t seed, float lr_t, float beta1,
                           float beta2, float eps, float l2);
int scann_train_step_end(scann_handle_t* h, double* sse_out, int64_t* count_out, double* abs_err_out /* sum |y - target|, or NULL */);
int scann_get_grads(scann_handle_t* h, float* out);           /* [scann_param_count] */
int scann_get_weights(scann_handle_t* h, float* out);         /* current master parameters, same order */

/* ---- fine-tuning: frozen tensors, per-tensor learning rates and a backward that stops at the floor ----
 * Stage of a tensor, with L = n_attention:
 *   0              the leaves: embed_atom, extra_embed, dense_embed, neighbor_d, neighbor_w
 *   l + 1          local_attention_<l> and residual_norm_<l>, l = 0 .. L-1 (the base branch's per-layer filter_geo belongs to its layer)
 *   L + 1          after_Lc, global_attention
 *   L + 2          bf_property, predict_property
 * scann_tensor_stage is pure host code and needs no handle; a name that is no tensor of such a model returns -1.
 * Learning-rate scale: one fp32 factor s per tensor in scann_weight_name() order, finite and >= 0; NULL restores "all 1" and the
 * unscaled optimiser kernel.  It may be set before or after scann_train_begin (it survives that call) and takes effect from the next
 * scann_train_backward, scann_train_step[_begin] and scann_adam_step.  SCANN_ERR_INVALID, with a message that names the argument: a
 * null handle, a negative or non-finite entry, every entry 0 (nothing to train), a call between scann_train_step_begin and its _end.
 * Optimiser: an element of a tensor with s == 0 is frozen (Keras trainable = False) -- its weight and both Adam moments keep their
 * bytes and the l2 regulariser term is not applied; its gradient entry is still zeroed where the step zeroes gradients.  For s > 0 the
 * update is scann_adam_step's with lr_hat replaced by lr_hat * s (one fp32 product), through the same device function as the unscaled
 * kernel: s == 1 gives its bytes.  The step counter advances as before.  With no scale set the launch is the unscaled kernel itself.
 * Floor: the lowest stage that holds a tensor with s > 0.  A training backward launches nothing whose only consumers lie below the
 * floor: no ResidualNorm / attention / geometry / base-branch backward, weight-gradient launch or reduction for the layers
 * l < floor - 1; above stage 0 no basis leaf, no embedding leaf and no projection into them; at floor L + 2 the readout launches only
 * what bf_property and predict_property need.  Inside the stages that run, the weight-gradient jobs of frozen tensors are not queued
 * (a job that writes a kernel and its bias stays while either is trained); partial sums a fused kernel stores anyway stay.
 * Gradient vector: entries of tensors in stages below the floor are not written by the backward (zero after scann_zero_grads);
 * entries of frozen tensors in stages that ran are unspecified and never applied; trained tensors get the bytes of the whole
 * backward.  The flat all-reduce is unchanged.
 * scann_train_stages: bit k of *ran = stage k was entered by the last training backward enqueued on the handle (set by the stages
 * themselves, not derived from the scale).
 * The training forward is unchanged (Dropout stays active in frozen layers, as in Keras).  scann_input_grads, inference, model sets
 * and every analysis call ignore scale and floor.  Plain-fp32 handles (widths other than 128 / 8): the optimiser rule holds; their
 * backward is NOT cut at the floor, and scann_train_stages reports every stage. */
int scann_tensor_stage(const char* name, int n_attention);
int scann_set_lr_scale(scann_handle_t* h, const float* scale /* [scann_weight_count] or NULL */);
int scann_get_lr_scale(const scann_handle_t* h, float* out /* [scann_weight_count]; all 1 when none is set */);
int scann_train_stages(const scann_handle_t* h, uint64_t* ran);

/* ---- gradients of the prediction with respect to the inputs (inference semantics) ----
 * d y_s / d input for every structure of a resident batch (inference semantics, dy_s = 1 per structure); synchronous.
 * y is the raw output (predict_property, before any target de-normalisation); mrelu (target e_b) passes the gradient through as the
 * identity, as in training.  Writes nothing into the training state (gradients, Adam moments, master weights, step counter); on a
 * training handle it uses the current weights.  SCANN_ERR_UNSUPPORTED for a checkpoint with |w| >= 255.9 in a 128x128 kernel,
 * SCANN_ERR_RANGE when the forward's range guard fires; either is returned before any output is written.
 * Any output pointer may be NULL (that leaf is not computed): y[n_struct], d_distance[n_edge], d_weight[n_edge],
 * d_ring[n_atom*2] (use_ring), d_cgcnn[n_atom*92] (feature cgcnn; otherwise SCANN_ERR_INVALID if non-NULL). */
int scann_input_grads(scann_handle_t* h, scann_dbatch_t* db, float* y, float* d_distance, float* d_weight,
                      float* d_ring, float* d_cgcnn);

/* ---- Monte Carlo dropout ----
 * n_samples forwards of a resident batch with the model's Dropout layers active -- Keras' model(x, training=True) -- reduced on the
 * device to the mean and the unbiased standard deviation (divided by T - 1; fp64 sums over the samples in order) of y and, if asked
 * for, of the GlobalAttention scores.  The masks of sample t of structure s are drop_scale(mc_seed(seed, t, key_s), tag, i, p) with the
 * training forward's tags and a structure-local element index (scann_mc_drop_scale), so a structure's samples do not depend on its
 * batch: two identical structures with the same key get identical samples.  keys: [n_struct] or NULL (all 0).  p_drop: the two
 * Dropout(0.1) layers (< 0: 0.1); p_attn: the attention-weight Dropout of use_drop models (< 0: the rate of scann_set_attention_dropout,
 * 0 unless set); a rate outside [0, 1) or n_samples < 2 is SCANN_ERR_INVALID.  Both rates 0: every sample is the plain forward's y.
 * Outputs: y_mean, y_std [n_struct]; ga_mean, ga_std [n_atom] (NULL: not computed); y_samples [n_samples * n_struct] (NULL: not copied).
 * Works on inference and training handles and changes neither (weights, gradients, Adam state, step counter, selected outputs, the
 * batch's last y).  SCANN_ERR_UNSUPPORTED on a handle whose forwards run on the exact-fp32 kernels (|w| >= 255.9, SCANN_EXACT=1), and
 * SCANN_ERR_RANGE when a sample trips the split-fp16 range guard; either before any output is written.  Synchronous. */
int scann_predict_mc(scann_handle_t* h, scann_dbatch_t* db, int32_t n_samples, uint64_t seed, const uint64_t* keys, float p_drop, float p_attn,
                     float* y_mean, float* y_std, float* ga_mean, float* ga_std, float* y_samples);
/* the Monte Carlo dropout factor of one element: 0 or 1 / (1 - p) (host; the kernels' definition) */
double scann_mc_drop_scale(uint64_t seed, int32_t t, uint64_t key, uint32_t tag, uint64_t idx, float p);

/* ---- per-atom contributions: the prediction with atoms left out of the global pooling ----
 * In the reference atom_mask feeds nothing but GlobalAttention (scann_model.py:329-447; the LocalAttention layers take neighbor_mask
 * only), so model.predict with atom_mask = 1 on a kept set S of a structure's atoms and 0 elsewhere is "the prediction with the other
 * atoms' local-structure representations left out of the pooling, everything upstream unchanged": e_i(S) = sum over j in S, j != i of
 * k_i . q_j (attention.py:279-292), softmax over S of e / ||e|| (:295-302, the division with use_ga_norm only), rep = sum a_i k_i
 * (:314-316), then the head (scann_model.py:437-447).  This call runs one forward of the resident batch and computes y(S) for all the
 * kept sets of one mode from the forward's gq / gk, with atoms ranked by the forward's GlobalAttention scores, descending, ties by
 * ascending atom index:
 *   SCANN_ABLATE_LEAVE_ONE_OUT  entry r (atom r):  all atoms of the structure but r
 *   SCANN_ABLATE_DELETION       entry k - 1, k = 1..n:  all but the k highest-ranked atoms (k = n: the empty pooling)
 *   SCANN_ABLATE_INSERTION      entry k - 1, k = 1..n:  the k highest-ranked atoms only (k = n: the plain forward's y, up to summation order)
 * Non-finite results are the reference's: with use_ga_norm a pooling over one atom or none is 0 / 0 = NaN; without it both are finite.
 * Outputs, any of them NULL: y [n_struct] and ga [n_atom], bitwise those of scann_forward_resident + scann_batch_download;
 * y_abl [n_atom], entry e of structure s at mol_offset[s] + e; order [n_atom], the structure-local atom index by rank at
 * mol_offset[s] + rank.  Raw outputs (before any target de-normalisation).  Synchronous.  An unknown mode is SCANN_ERR_INVALID; a
 * structure of more than SCANN_ABLATE_MAX_ATOMS atoms is SCANN_ERR_UNSUPPORTED, returned before anything is launched;
 * SCANN_ERR_RANGE as from scann_batch_download (an inference handle re-runs the forward on the exact-fp32 kernels first).  Works on
 * inference and training handles, at 128 / 8 and at generic widths, and changes neither weights, gradients, Adam state, step counter
 * nor the selected outputs. */
#define SCANN_ABLATE_LEAVE_ONE_OUT 0
#define SCANN_ABLATE_DELETION 1
#define SCANN_ABLATE_INSERTION 2
#define SCANN_ABLATE_MAX_ATOMS 960 /* atoms per structure: 32 score rows of the structure live in one workgroup's 160 KiB of LDS */
int scann_ablate_pooling(scann_handle_t* h, scann_dbatch_t* db, int32_t mode, float* y, float* ga, float* y_abl, int32_t* order);

/* ---- Shapley values of the atoms for the global pooling, sampled ----
 * The game: the players are the n real atoms of one structure, v(S) is the prediction with the atoms outside S left out of the
 * GlobalAttention pooling and everything upstream unchanged -- for |S| >= 2 exactly scann_ablate_pooling's y(S).  With use_ga_norm the
 * reference's pooling over one atom or none is 0 / 0, and every walk starts there, so for |S| <= 1 the game uses the arithmetic of
 * use_ga_norm = false whatever the model's setting, the continuous extension: a softmax over one kept atom is 1 for any finite logit, so
 * v({i}) = head(k_i), and the empty pooling has rep = 0, so v(empty) = head(0), the baseline.  (The full set keeps the forward's
 * arithmetic: a ONE-atom structure under use_ga_norm has v(all) = y = NaN, and its Shapley value and stderr are NaN.  A NaN arising at
 * |S| >= 2 propagates into that structure's outputs as it is.  scann_ablate_pooling keeps returning the reference's NaN.)
 * This call runs one forward of the resident batch, then n_perm walks per structure from the forward's gq / gk.  Walk p of structure s adds
 * the atoms in the order pi_p = scann_shapley_permutation(seed, keys[s], p, n) (keys NULL: all 0), or in the order of row p of perms_in
 * ([n_perm * n_atom], structure-local atom indices at mol_offset[s] + position; every row a permutation of every structure, else
 * SCANN_ERR_INVALID):
 *   values[p][j] = v({pi_p(0..j)}) in fp32, j = 0 .. n - 1;  marginal of atom pi_p(j) = (double)values[p][j] - (double)(j ? values[p][j-1] : baseline)
 *   shapley[i]   = the fp64 mean of atom i's marginals over p = 0 .. n_perm - 1, added in p order
 *   stderr[i]    = sqrt(sum (m - mean)^2 / (n_perm - 1) / n_perm), two passes, same order; NaN when n_perm = 1
 *   full         = the fp64 mean of values[p][n - 1];  sum_i shapley[i] = full - baseline up to fp64 rounding (efficiency)
 * Outputs, any of them NULL: y [n_struct] and ga [n_atom], bitwise the forward's; shapley, stderr_out [n_atom]; baseline, full [n_struct];
 * values [n_perm * n_atom] and perms_out [n_perm * n_atom] (entry j of walk p of structure s at p * n_atom + mol_offset[s] + j).  Raw
 * outputs (before any target de-normalisation).  A structure's results depend on the structure, seed, its key and n_perm only -- not on
 * its batch.  Synchronous.  n_perm < 1 is SCANN_ERR_INVALID; a structure of more than SCANN_ABLATE_MAX_ATOMS atoms, or scratch
 * 2 * n_perm * n_atom * 4 bytes (or the batch's pair matrices, 4 * sum n^2 bytes) above 1 GiB, is SCANN_ERR_UNSUPPORTED; all returned
 * before anything is launched.  SCANN_ERR_RANGE as from scann_batch_download.  Works on inference and training handles, at 128 / 8 and
 * at generic widths, and changes neither weights, gradients, Adam state, step counter nor the selected outputs. */
int scann_shapley(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, const int32_t* perms_in,
                  float* y, float* ga, double* shapley, double* stderr_out, double* baseline, double* full, float* values, int32_t* perms_out);
/* scann_shapley without outputs, timed between events: ms[0] the pair kernel, ms[1] the walks, ms[2] the reduction (milliseconds) */
int scann_shapley_profile(scann_handle_t* h, scann_dbatch_t* db, int32_t n_perm, uint64_t seed, const uint64_t* keys, float* ms);
/* walk p of a structure of n atoms with key `key` (host; the kernels' definition): a Fisher-Yates shuffle, a function of (seed, key, p, n)
 * only.  base = mix(mix(seed + G * (p + 1)) + G * (key + 1)), G = 0x9E3779B97F4A7C15, mix = the splitmix64 finaliser; out = 0 .. n - 1;
 * for i = n - 1 down to 1: u = mix(base + G * (i + 1)) >> 32, k = (u * (i + 1)) >> 32 (multiply-high, 0 <= k <= i), swap out[i], out[k].
 * Nothing is written for n <= 0, p < 0 or out NULL. */
void scann_shapley_permutation(uint64_t seed, uint64_t key, int32_t p, int32_t n, int32_t* out);
/* the reduction of scann_shapley on the host, bit for bit: values, perms [n_perm * n_atom] (n_atom = mol_offset[n_struct]) and baseline
 * [n_struct] in; shapley, stderr_out [n_atom] and full [n_struct] out.  SCANN_ERR_INVALID for a NULL argument, n_perm < 1 or an entry
 * of perms outside its structure. */
int scann_shapley_reduce_host(const float* values, const int32_t* perms, const int32_t* mol_offset, int32_t n_struct, int32_t n_perm,
                              const double* baseline, double* shapley, double* stderr_out, double* full);

/* ---- attention rollout: a prediction traced through the LocalAttention layers ----
 * A GlobalAttention score belongs to an atom's local structure after n_attention rounds of message passing, not to the atom.  Attention
 * rollout (Abnar & Zuidema 2020) composes the layers' attention maps: for one structure of n atoms, packed edges in CSR order, and the
 * weights a[l][e][h] of layer l exactly as scann_output_read(.., SCANN_OUT_LOCAL_ATTENTION, l, ..) returns them for this forward,
 *   abar[l][e] = (a[l][e][0] + ... + a[l][e][H-1]) * (1 / H), heads added in index order (head = -1), or a[l][e][k] (head = k);
 *   (T_l R)[i, :] = residual * R[i, :] + (1 - residual) * sum over the edges e of atom i, in CSR order, of abar[l][e] * R[col(e), :]
 *                   for an atom with at least one edge, R[i, :] for an atom without (its context is the LayerNorm of its own query);
 *                   several edges to one neighbour add, an edge from an atom to itself is an ordinary edge;
 *   R = T_{depth-1} ... T_1 T_0 I: R[i, j] = the share of atom i's representation after `depth` layers that traces back to atom j, every
 *                   row sums to 1;  attribution[j] = sum over i, ascending, of ga[i] * R[i, j], which sums to 1 wherever ga does (a
 *                   one-atom structure under use_ga_norm has ga = NaN, and so has its attribution).
 * fp32 sums in the stated order, no atomics; a structure's results are bitwise the same in any batch and at any position.
 * The call runs one forward of the resident batch -- for this forward the first `depth` attention maps are added to what
 * scann_set_outputs selected, and the handle's selection is put back before the call returns, also when it fails -- downloads it as
 * scann_batch_download does (range guard, exact-fp32 re-run, SCANN_STRICT_RANGE; SCANN_ERR_UNSUPPORTED for a g_update model whose forward
 * does not run the fused first layer, as with selected attention maps), and rolls the maps up where the forward left them.  The batch's
 * output block then belongs to that forward: scann_output_read on the batch returns the maps the rollout was made from, until the
 * batch's next forward, which writes the handle's own selection again.  residual in [0, 1] (0.5: attention and skip connection weigh the
 * same); head in -1 .. num_head - 1; depth <= 0: n_attention, depth > n_attention: SCANN_ERR_INVALID.  Outputs, any of them NULL:
 * y [n_struct] and ga [n_atom], bitwise those of scann_forward_resident + scann_batch_download; attribution [n_atom];
 * rollout [scann_rollout_floats]: the structures' n x n row-major blocks one after another (NULL: not formed).  Synchronous.  Errors
 * before anything is launched: SCANN_ERR_INVALID (null handle or batch, residual, head, depth), SCANN_ERR_WEIGHTS, and
 * SCANN_ERR_UNSUPPORTED for a structure of more than SCANN_ROLLOUT_MAX_ATOMS atoms.  An empty batch and a batch without edges (R = I,
 * attribution = ga) are computed.  Works on inference and training handles, at 128 / 8 and at generic widths, and changes neither
 * weights, gradients, Adam state, step counter nor the selected outputs.  scann_rollout_floats: the sum over the batch's structures of
 * n^2 (it waits for the batch's upload), or a negative status. */
#define SCANN_ROLLOUT_MAX_ATOMS 960 /* atoms per structure: two 16-column slabs [n][16] of the structure live in one workgroup's 160 KiB of LDS */
int64_t scann_rollout_floats(scann_handle_t* h, const scann_dbatch_t* db);
int scann_attention_rollout(scann_handle_t* h, scann_dbatch_t* db, float residual, int32_t head, int32_t depth, float* y, float* ga,
                            float* attribution, float* rollout);

/* ---- latent-space index: the nearest training structures of a prediction, searched on the device ----
 * An index holds N < 2^31 rows of `dim` fp32 values in insertion order (position 0 .. N-1); each row carries an int64 id and an int32
 * atom (-1 for a structure-level row).  For a query vector q and a row r
 *   dist2(q, r) = acc_dim,  acc_0 = 0,  acc_{j+1} = fmaf(q[j] - r[j], q[j] - r[j], acc_j)
 * in fp32, the difference rounded once, columns ascending (scann_knn_distsq is this chain on the host: the kernel's bits), and the k
 * nearest rows of q are the first k rows under the TOTAL order (dist2 ascending, then position ascending).  A query's result therefore
 * depends on the query and the index contents only: not on the batch it is in, on how the rows are split over workgroups or on how many
 * calls built the index.  With query ids, rows whose id equals the query's are skipped (leave-one-out distances of a set to itself).
 * Places for which no row qualifies hold id -1, atom -1, position -1, dist2 +inf; a row whose distance is NaN never qualifies.  The
 * distance is not the product form |q|^2 + |r|^2 - 2 q.r, which loses near-duplicates to cancellation; its error against exact
 * arithmetic is at most (dim + 3) * 2^-24 relative.
 *
 * The rows live in device blocks of the handle's cache, allocated a chunk (about 64 MiB) at a time; rows already stored are never moved.
 * EVERY call below is synchronous (it returns when the device has finished), so no query is in flight while rows are added.
 * scann_index_add / scann_index_query take host vectors (rows [n * dim], q [nq * dim]); ids NULL: the row's position; atoms NULL: -1;
 * query_ids NULL: nothing is skipped.  scann_index_read copies rows [first, first + n) back (any output NULL), for saving an index.
 * Outputs of the queries: dist2, ids, atoms, pos [nq * k] (ids, atoms, pos may be NULL).
 * level = SCANN_OUT_BF_PROPERTY (one row per structure of the batch) or SCANN_OUT_AFTER_LC (one row per atom in packed order, atom = its
 * index within its structure).  scann_index_add_batch runs one inference forward of the resident batch -- with the level's output added
 * to what scann_set_outputs selected for that forward only; the handle's selection is put back before the call returns, also when it
 * fails -- and appends the level's rows device to device; ids [n_struct] (NULL: structure level the position, atom level the structure's
 * index in the batch).  scann_index_query_batch runs the same forward and searches the level's rows: y [n_struct] and ga [n_atom] (or
 * NULL) are bitwise those of scann_forward_resident + scann_batch_download (range guard, exact-fp32 re-run, SCANN_STRICT_RANGE as there);
 * query_ids [n_struct] or NULL.  After either call the batch's output block belongs to that forward, as after scann_attention_rollout.
 * SCANN_ERR_INVALID before anything is launched: a null argument, k outside 1 .. SCANN_KNN_MAX_K, a dim outside 1 .. 1024 or that is
 * not the model's dense_out / global_dim for the level, an unknown level, an empty query, an index created on another handle.  An empty
 * index answers with the +inf tail.  The calls work on inference and training handles, at 128 / 8 and at generic widths and on handles
 * whose forwards run on the exact-fp32 kernels, and change neither weights, gradients, Adam state, step counter nor the selected
 * outputs.  An index must be freed before its handle's device is reset; scann_index_free(h, idx) needs no live handle (h may be NULL). */
#define SCANN_KNN_MAX_K 32
typedef struct scann_index scann_index_t;
int scann_index_create(scann_handle_t* h, int32_t dim, scann_index_t** out);
void scann_index_free(scann_handle_t* h, scann_index_t* idx);
int64_t scann_index_size(const scann_index_t* idx);
int scann_index_add(scann_handle_t* h, scann_index_t* idx, const float* rows, int64_t n, const int64_t* ids, const int32_t* atoms);
int scann_index_read(scann_handle_t* h, scann_index_t* idx, int64_t first, int64_t n, float* rows, int64_t* ids, int32_t* atoms);
int scann_index_query(scann_handle_t* h, scann_index_t* idx, const float* q, int64_t nq, const int64_t* query_ids, int32_t k, float* dist2,
                      int64_t* ids, int32_t* atoms, int32_t* pos);
int scann_index_add_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, const int64_t* ids);
int scann_index_query_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, const int64_t* query_ids, int32_t k, float* y,
                            float* ga, float* dist2, int64_t* ids, int32_t* atoms, int32_t* pos);
/* the kernel's distance chain on the host (no GPU work), one pair and out[i * n + r] for every (query i, row r) */
float scann_knn_distsq(const float* q, const float* r, int64_t d);
void scann_knn_distsq_matrix(const float* q, int64_t nq, const float* rows, int64_t n, int64_t d, float* out);

/* ---- structure matching: the nearest structures of an atom-level index by their local structures ----
 * Which indexed structures are made of the same local structures as this one?  A query structure and an indexed structure are compared
 * as SETS of after_Lc rows (the best-match / average-kernel comparison of atomic environments), on the device right behind the forward.
 *
 * Segments.  The structures of an index are its segments: the maximal runs of consecutive positions whose rows carry the same id.
 * Segment s is the rows [first_s, first_s + m_s); segments are numbered in position order.  scann_index_add_batch at atom level gives one
 * segment per structure; an id that occurs in two separate runs gives two segments.  A segment may be of any length and may lie across
 * a storage-chunk boundary.  scann_index_segments reads the table from the host copies the index keeps (any output NULL) and returns
 * the number of segments.
 *
 * Pair quantities, for a query structure A = a_0 .. a_{n-1} (n >= 1) and a segment B = b_0 .. b_{m-1}:
 *   D[i][j] = dist2(a_i, b_j), exactly the fp32 chain of scann_index_query (scann_knn_distsq: its bits);
 *   f_i = min_j D[i][j] over the j whose D[i][j] is not NaN, +inf if there is none; its witness is the least position that attains it
 *         (position -1 if there is none);
 *   g_j = min_i D[i][j] likewise, the least query atom as witness;
 *   F: fp64, acc = 0, acc += (double) f_i for i ascending, F = acc / n;    G: the same over j ascending, divided by m;
 *   Fmax = max_i f_i, Gmax = max_j g_j (fp32);    parts = {(float) F, (float) G, Fmax, Gmax}.
 * Score, by `measure`:
 *   SCANN_MATCH_CHAMFER    (float)(F + G), the add in fp64 and rounded once;
 *   SCANN_MATCH_HAUSDORFF  max(Fmax, Gmax);
 *   SCANN_MATCH_COVER      (float) F, the directed form: does every local structure of the query occur in B?
 * A score is never NaN; it is +inf if an atom has no finite partner.  Chamfer and Hausdorff are symmetric in (A, B) bit for bit: the
 * difference is negated exactly, its square is the same, and the fp64 add commutes.
 *
 * Ranking.  The k nearest segments of A are the first k under the TOTAL order (score ascending, then segment number ascending), k in
 * 1 .. SCANN_KNN_MAX_K, so the answer depends on the query and the index contents only, bit for bit: not on the batch the structure is
 * in, on the launch geometry or on how many calls built the index.  With query ids, segments whose id equals the query's are skipped.
 * Places without a segment hold segment -1, id -1, size 0, score and parts +inf, match positions -1, match dist2 +inf.
 * Matches.  For every query atom i and every place p: the position of the witness of f_i in the place's segment, and f_i.
 *
 * scann_index_match takes host vectors: q [q_first[n_sets] * dim], the rows of set s being q_first[s] .. q_first[s + 1] - 1 (q_first[0]
 * = 0).  Outputs: score, segment, ids, sizes [n_sets * k], parts [n_sets * k * 4], match_pos, match_dist2 [q_first[n_sets] * k]; all
 * but score may be NULL.  scann_index_match_batch runs one inference forward of the resident batch with after_Lc added for that forward
 * only and matches every structure of the batch; y, ga, the handle's selection, training state, generic widths and SCANN_EXACT are
 * exactly as for scann_index_query_batch.  SCANN_ERR_INVALID before anything is launched: a null argument, a bad k or measure, an empty
 * query or an empty query set, a q_first that does not start at 0 or decreases, an index of another handle or width.  A query structure
 * of more than SCANN_MATCH_MAX_ATOMS atoms is SCANN_ERR_UNSUPPORTED, before anything is launched, and the message names it; segments
 * have no length limit.  An empty index answers with the +inf tail.  Synchronous.
 * scann_match_parts_host is the host twin (no GPU work, the scann_knn_distsq chain): parts [n_sets * n_seg * 4] of every (set,
 * segment) pair of q [q_first[n_sets] * dim] and rows [seg_first[n_seg] * dim]; q_first [n_sets + 1], seg_first [n_seg + 1] increasing. */
#define SCANN_MATCH_CHAMFER 0
#define SCANN_MATCH_HAUSDORFF 1
#define SCANN_MATCH_COVER 2
#define SCANN_MATCH_MAX_ATOMS 128 /* atoms per query structure: a structure's atoms are the query rows of one workgroup, which holds the
                                     128 x 64 distances of a tile in LDS (33 KiB) and an 8 x 4 register block of chains per lane */
int64_t scann_index_segments(const scann_index_t* idx, int64_t* first, int32_t* count, int64_t* id);
int scann_index_match(scann_handle_t* h, scann_index_t* idx, const float* q, const int32_t* q_first /* [n_sets + 1] */, int64_t n_sets,
                      const int64_t* query_ids, int32_t measure, int32_t k, float* score, int32_t* segment, int64_t* ids, int32_t* sizes,
                      float* parts, int32_t* match_pos, float* match_dist2);
int scann_index_match_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, const int64_t* query_ids, int32_t measure, int32_t k,
                            float* y, float* ga, float* score, int32_t* segment, int64_t* ids, int32_t* sizes, float* parts, int32_t* match_pos,
                            float* match_dist2);
int scann_match_parts_host(const float* q, const int32_t* q_first, int64_t n_sets, const float* rows, const int32_t* seg_first, int64_t n_seg,
                           int64_t dim, float* parts /* [n_sets * n_seg * 4] */);

/* ---- pairing: one-to-one atom maps between a query structure and a segment, the exact assignment on the device ----
 * The measures of scann_index_match are best-match reductions: every atom picks its nearest partner on its own, so the correspondence is
 * many-to-one and the score cannot count (rows {3 x a, 3 x b} against {5 x a, 1 x b}: chamfer 0).  The pairing solves the linear
 * assignment problem over the matrix of squared distances (the best-match structural kernel of De et al., PCCP 2016) and returns a
 * true atom map.  "assign" means cluster assignment in this library; this is called pairing everywhere.
 *
 * Definition, for a query structure A = a_0 .. a_{n-1} and a segment B = b_0 .. b_{m-1}, 1 <= n, m <= SCANN_PAIRING_MAX_ATOMS:
 *  1. Distances.  D[i][j] = dist2(a_i, b_j), exactly the fp32 chain of scann_knn_distsq with the query atom as q.
 *  2. Not comparable.  If any D[i][j] is NaN or +inf, or m > SCANN_PAIRING_MAX_ATOMS: score = +inf, total = -1, shift = 0, every
 *     partner -1 and every partner distance +inf.
 *  3. Per-pair fixed point.  Dmax = max D (exact).  shift = 30 - ilogbf(Dmax) for Dmax > 0 (the true exponent, subnormals included),
 *     0 for Dmax = 0.  t[i][j] = llrint(ldexp((double) D[i][j], shift)): the scaling is exact, then one rounding to nearest even.  So
 *     0 <= t <= 2^31 and the largest entry keeps 30 bits; shift lies in -97 .. 179.  No caller-chosen shift, no range error.
 *  4. Square cost matrix.  Q = max(n, m); rows are the query side, columns the segment side.  C[i][j] = t[i][j] for i < n, j < m.  For
 *     n < m the dummy rows i >= n have C[i][j] = min_{i' < n} t[i'][j]: a surplus atom of the segment is charged its nearest partner.
 *     For m < n the dummy columns j >= m have C[i][j] = min_{j' < m} t[i][j'], likewise.
 *  5. Optimum.  total = min over permutations pi of sum_i C[i][pi(i)], an int64 below 2^38: an integer minimum, so it has no summation
 *     order and depends on no algorithm, launch geometry or thread count.  score = (float)(ldexp((double) total, -shift) / (double) Q),
 *     the division in fp64 and rounded once.  It is symmetric in (A, B) bit for bit: D transposes exactly, Dmax and shift are the
 *     same, C transposes.
 *  6. The map is not unique under ties, so the procedure is part of the definition: the shortest-augmenting-path method with
 *     potentials in exact int64 arithmetic.  State: u[Q] = v[Q] = 0, p[j] = -1.  For each row i = 0 .. Q-1 ascending: minv[j] = INF,
 *     used[j] = false, way[j] = -1, j0 = -1 (the virtual column that holds row i).  Repeat until the break:
 *       if j0 >= 0 mark j0 used;  i0 = j0 < 0 ? i : p[j0];  delta = INF;
 *       over the unused j ascending: cur = C[i0][j] - u[i0] - v[j]; if cur < minv[j] then minv[j] = cur, way[j] = j0; if minv[j] < delta
 *         then delta = minv[j], j1 = j (strict: the least column index wins a tie);
 *       u[i] += delta;  for used j: u[p[j]] += delta, v[j] -= delta;  for the others: minv[j] -= delta;
 *       j0 = j1;  break when p[j0] == -1.
 *     Then walk way back from j0: p[j0] = (way[j0] == -1) ? i : p[way[j0]], j0 = way[j0], until j0 == -1.  pi(p[j]) = j.
 *     Reduced costs never go negative and stay below 2^39, so a parallel argmin over (minv, j) reproduces the sequential scan.
 *     Per query atom i: its partner is segment atom pi(i) if pi(i) < m, with partner_dist2 = D[i][pi(i)]; otherwise the atom is
 *     surplus: partner -1 and partner_dist2 = f_i = min_j D[i][j], what it was charged.
 *
 * scann_index_pairing pairs explicit (query set, segment number) pairs -- any order, repeats allowed, n_pairs = 0 is fine -- of host
 * query rows q [q_first[n_sets] * dim] with segments of the index, one workgroup per pair.  Outputs: score, total, shift [n_pairs];
 * partner_pos (the partner's POSITION in the index, -1 for a surplus atom) and partner_dist2 in pair order, pair e owning
 * n(pair_set[e]) places; all but score may be NULL.  scann_index_pairing_batch runs one inference forward of the resident batch with
 * after_Lc added for that forward only (y, ga, the handle's selection, training state, generic widths and SCANN_EXACT exactly as for
 * scann_index_match_batch), takes each structure's shortlist -- the answer of scann_index_match with k = shortlist under `measure`, query
 * ids applied there, k <= shortlist <= SCANN_KNN_MAX_K -- pairs the structure with every shortlisted segment and answers the first k of
 * them under the TOTAL order (pairing score ascending, then segment number ascending); pairs that are not comparable rank last, by
 * segment number.  Outputs: score, segment, ids, sizes, total, shift, short_score (the segment's score under `measure`), short_place
 * (its place in the shortlist) [n_struct * k]; partner_pos, partner_dist2 [n_atom * k] at [(atom) * k + place]; all but score may be
 * NULL.  Places without a segment hold score +inf, segment -1, id -1, size 0, total -1, shift 0, short_score +inf, short_place -1,
 * partner -1, partner_dist2 +inf.  The result is a function of the query, the index and (k, shortlist, measure) only.
 * SCANN_ERR_INVALID before anything is launched, the message naming the argument: a null argument, k or shortlist out of range or
 * shortlist < k, a bad measure, an index of another handle or width, a pair index out of range, an empty query.  A query structure of
 * more than SCANN_PAIRING_MAX_ATOMS atoms is SCANN_ERR_UNSUPPORTED; a SEGMENT above it is no error: that pair is not comparable.
 * Synchronous.
 * The twins do no GPU work.  scann_pairing_host is the definition for one pair, a [n * dim] against b [m * dim]: score, total, shift,
 * partner [n] (the index within b, -1: surplus), partner_dist2 [n], any NULL; n above the limit is SCANN_ERR_UNSUPPORTED.
 * scann_pairing_solve_host is step 6 alone on any cost matrix [Q * Q] (row-major, rows first) with entries <= 2^31, 1 <= Q <=
 * SCANN_PAIRING_SOLVE_MAX: col_of_row [Q] = pi, total. */
#define SCANN_PAIRING_MAX_ATOMS 128 /* a side: lane l of the solving wave owns columns l and l + 64 of the cost matrix, 66 KiB of LDS */
#define SCANN_PAIRING_SOLVE_MAX 4096
int scann_index_pairing(scann_handle_t* h, scann_index_t* idx, const float* q, const int32_t* q_first /* [n_sets + 1] */, int64_t n_sets,
                        const int32_t* pair_set, const int32_t* pair_segment, int64_t n_pairs, float* score, int64_t* total, int32_t* shift,
                        int32_t* partner_pos, float* partner_dist2);
int scann_index_pairing_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, const int64_t* query_ids, int32_t measure,
                              int32_t shortlist, int32_t k, float* y, float* ga, float* score, int32_t* segment, int64_t* ids, int32_t* sizes,
                              int64_t* total, int32_t* shift, float* short_score, int32_t* short_place, int32_t* partner_pos,
                              float* partner_dist2);
int scann_pairing_host(const float* a, int64_t n, const float* b, int64_t m, int64_t dim, float* score, int64_t* total, int32_t* shift,
                       int32_t* partner, float* partner_dist2);
int scann_pairing_solve_host(const uint32_t* cost, int32_t Q, int32_t* col_of_row, int64_t* total);

/* ---- greedy k-center selection: the most diverse rows of an index, picked on the device ----
 * Which m candidates should be labelled next, given what is labelled already?  Farthest-point selection in latent space (the core-set
 * rule of Sener & Savarese, ICLR 2018): repeatedly take the candidate whose distance to everything labelled or already taken is
 * largest.  Each pick comes with the covering radius at that moment.  Without a reference the same call thins a redundant set to m
 * representative rows.
 * Inputs: a pool index P with N rows; an optional reference index R (NULL or empty: none; otherwise of the same dim, of the same handle
 * and a different object from P); a count m >= 1; a threshold stop_dist2 (<= 0: none).
 * Distance: dist2 is exactly the chain of scann_knn_distsq above: fp32, acc = fmaf(q[j] - r[j], q[j] - r[j], acc), columns ascending.
 * It is symmetric bit for bit, because fl(a - b) = -fl(b - a).
 * Eligibility: a pool row is eligible if and only if all its dim components are finite.  Ineligible rows are never picked; this includes
 * a row picked as a centre already.  Between eligible rows no distance is NaN; overflow gives +inf, which is ordered.
 * Initial distances: mind[p] is the least dist2(P[p], R[r]) over the rows r of R, with the rule of scann_index_query: a NaN distance
 * never counts.  With no such row it is +inf.  (It is the k = 1 query of the pool's own rows against R, run device to device.)
 * Each pick i = 0, 1, ...: (1) among the eligible rows not yet picked, take the first under the TOTAL order (mind descending, position
 * ascending); (2) report its position, id, atom and radius2[i] = mind at that moment; (3) mark it picked; (4) update
 * mind[p] = min(mind[p], dist2(P[p], P[pick])) for every p.
 * Selection ends when m picks are made, or no eligible unpicked row is left, or stop_dist2 > 0 and the next pick's mind < stop_dist2
 * (that pick is not made).
 * Consequences: radius2 is non-increasing.  Without a reference the first pick is the lowest-positioned eligible row, with radius +inf.
 * An exact duplicate of a picked row has mind 0 and is picked only after every row at a positive distance.  The result depends on the
 * contents of P and R alone: not on chunking, on how many add calls built the indices or on the launch geometry.
 * Return: the number of picks made (>= 0) or a negative status.  Places behind that count hold position -1, id -1, atom -1, radius2 +inf.
 * SCANN_ERR_INVALID before anything is launched: a null handle or pool, an index of another handle, P == R, different dim, m < 1, a NaN
 * stop_dist2, a null pos.  An empty pool returns 0.
 * The call is synchronous.  It changes nothing in P, R, the handle's weights, training state or selected outputs; it works on inference
 * and training handles at any width and runs no forward.  All m picks are enqueued on one stream and the host waits once: the picked
 * position and the end of the selection travel from pick to pick through device memory. */
int64_t scann_index_select(scann_handle_t* h, scann_index_t* pool, scann_index_t* reference /* or NULL */, int64_t m, float stop_dist2,
                           int32_t* pos, int64_t* ids, int32_t* atoms, float* radius2);   /* [m] each; ids, atoms, radius2 may be NULL */
/* the definition on the host, no GPU work: rows [n * dim], ref [nr * dim] (nr may be 0); the kernel's bits */
int64_t scann_kcenter_host(const float* rows, int64_t n, const float* ref, int64_t nr, int64_t dim, int64_t m, float stop_dist2,
                           int32_t* pos, float* radius2);

/* ---- k-means over an index: which kinds of local structure the model distinguishes, clustered on the device ----
 * Lloyd's iteration over the rows of an index, defined so that the labels and the centres depend on the index contents and the initial
 * centres only, bit for bit: not on chunking, on how many add calls built the index, on the launch geometry or on the order of any sum.
 * Inputs: a pool index P with N rows of dim columns; k initial centres C_0, 1 <= k <= SCANN_KMEANS_MAX_K; max_iter >= 0; stop_changed >= 0.
 * Distance: dist2(P[p], C[c]) is exactly the chain of scann_knn_distsq(row, centre, dim): fp32, acc = fmaf(x[j] - c[j], x[j] - c[j], acc),
 * columns ascending, the row as first argument.
 * Eligibility: a row is eligible if and only if all its components are finite (the rule of scann_index_select).  Ineligible rows get
 * label -1 and dist2 +inf, and count for nothing.
 * Assignment A(C): for each eligible row, label[p] is the first centre under the TOTAL order (dist2 ascending, centre index ascending).  A
 * NaN distance never qualifies; a row for which no centre qualifies gets -1 / +inf and counts for nothing.  For an eligible row this is
 * the k = 1 answer of scann_index_query of that row against an index that holds the centres in order: label = that answer's position,
 * dist2 = its dist2.
 * Column scales, once per call: m_j is the largest |x[p][j]| over the eligible rows, e_j the frexp exponent of m_j (m_j < 2^e_j; e_j = 0
 * if m_j = 0 or there is no eligible row), and q(x, j) = llrint(ldexp((double)x, 30 - e_j)), round to nearest even, so |q| <= 2^30.
 * Update U(label, C): for centre c, n_c is the number of rows labelled c and S[c][j] the sum of q(P[p][j], j) over those rows as an int64
 * (N < 2^31: it cannot overflow).  If n_c > 0 the new C[c][j] = (float) ldexp((double)S[c][j] / (double)n_c, e_j - 30), every conversion
 * and the division rounded to nearest; if n_c = 0 the centre keeps its value.  The integer sum is what makes the result independent of
 * the summation order; its error against the exact mean is at most 2^(e_j - 31) per component, 128 times finer than an fp32 ulp at the
 * top of the column's range.
 * Loop: label_{-1} is -1 everywhere.  For t = 0, 1, ...: (1) label_t, dist2_t = A(C_t); (2) changed_t = the number of rows with
 * label_t[p] != label_{t-1}[p]; (3) if changed_t <= stop_changed or t == max_iter, stop with n_iter = t and
 * converged = (changed_t <= stop_changed); (4) otherwise C_{t+1} = U(label_t, C_t).
 * Consequences: the returned labels, distances and sizes (the bincount of the labels) always belong to the returned centres; at most
 * max_iter updates are made; max_iter = 0 is a pure assignment to the given centres.
 * Exactly one of init [k * dim] and init_pos [k] (positions in the pool, whose rows are copied device to device) is given.
 * Return: n_iter (>= 0) or a negative status.  SCANN_ERR_INVALID, with a message that names the argument: a null handle, pool, labels or
 * centres, an index of another handle, k outside 1 .. SCANN_KMEANS_MAX_K, both or neither of init and init_pos, a non-finite init value,
 * an init_pos out of range, max_iter < 0, stop_changed < 0 -- all before anything is launched -- and an init_pos that names an ineligible
 * row, found by the eligibility pass on the device before the first round; no output is written then.  An empty pool returns 0 with
 * centres = init.
 * The call is synchronous.  It changes nothing in the pool, the handle's weights, training state or selected outputs; it works on
 * inference and training handles at any width and runs no forward.  All max_iter + 1 rounds are enqueued on one stream and the host
 * waits once (once per 256 rounds of a longer run): the end of the loop travels from round to round through device memory. */
#define SCANN_KMEANS_MAX_K 1024
int64_t scann_index_kmeans(scann_handle_t* h, scann_index_t* pool, int32_t k, const float* init /* [k * dim] or NULL */,
                           const int32_t* init_pos /* [k] positions in pool, or NULL */, int32_t max_iter, int64_t stop_changed,
                           int32_t* labels /* [N] */, float* dist2 /* [N] or NULL */, float* centres /* [k * dim] */,
                           int64_t* sizes /* [k] or NULL */, int32_t* converged /* or NULL */);
/* the definition on the host, no GPU work: rows [n * dim], init [k * dim]; the kernels' bits */
int64_t scann_kmeans_host(const float* rows, int64_t n, int64_t dim, int32_t k, const float* init, int32_t max_iter, int64_t stop_changed,
                          int32_t* labels, float* dist2, float* centres, int64_t* sizes, int32_t* converged);

/* ---- principal-component map of an index: mean, covariance and projection on the device ----
 * The low-dimensional map of a latent space, and the Mahalanobis distance to the indexed distribution (Lee et al., NeurIPS 2018) as an
 * applicability-domain score beside the k-nearest-neighbour distance.  Mean and covariance are defined so that they depend on the index
 * contents only, bit for bit: not on the order of any sum, on the launch geometry, on chunking or on how many add calls built the index.
 * Eligibility: a row is eligible if and only if all its components are finite (the rule of scann_index_select).  n is the number of
 * eligible rows; ineligible rows count for nothing.
 * Mean: the k-means update with one cluster.  e_j is the frexp exponent of the largest |x[p][j]| over the eligible rows (0 if that is
 * 0), q(x, j) = llrint(ldexp((double)x, 30 - e_j)), S_j the int64 sum of q over the eligible rows, and
 *   mean_j = (float) ldexp((double)S_j / (double)n, e_j - 30).
 * Centred values: y[p][j] = x[p][j] - mean_j in fp32, rounded once.  f_j is the frexp exponent of the largest |y[p][j]| over the
 * eligible rows (0 if that is 0).  L is the bit length of n (n < 2^L) and b = min(24, (62 - L) / 2), integer division: 24 bits up to
 * 16,383 rows, 20 at 2.4 M, 15 at 2^31 - 1 (scann_pca_bits).  u(y, j) = llrint(ldexp((double)y, b - f_j)), round to nearest even, so
 * |u| <= 2^b.
 * Scatter: T[i][j] is the int64 sum over the eligible rows of u_i * u_j, R_j the int64 sum of u_j.  Every partial sum of T is bounded by
 * n * 2^(2b) < 2^62: no order of the adds can overflow, and the sum is the same in any order.
 * Covariance, fp64:
 *   cov[i][j] = ldexp(((double)T_ij - (double)R_i * (double)R_j / (double)n) / (double)(n - 1), f_i + f_j - 2b)
 * as written, left to right, each operation rounded to nearest, none contracted; computed for i <= j and mirrored.
 * Error against the exact covariance cov* of the fp32 rows: |cov_ij - cov*_ij| <= 2^(f_i + f_j - b + 2).  (|u - y 2^(b - f)| <= 1/2 gives
 * n (2^b + 1/4) on T_ij; the remaining factor covers the fp32 centring, 2^-24 relative per factor, and the R term.)  The noise floor
 * nu = dim * 2^(2 max_j f_j - b + 2): by Weyl's inequality an eigenvalue at or below nu cannot be told from 0.
 * Eigen-decomposition (scann_sym_eig_host): on the host, fp64, cyclic Jacobi over the upper triangle of a [d * d], row-cyclic order
 * (p, q), p < q ascending.  An a_pq with |a_pp| + |a_pq| == |a_pp| and |a_qq| + |a_pq| == |a_qq| in fp64 -- below half an ulp of both
 * diagonal entries -- is set to exactly 0 without a rotation (between two equal eigenvalues theta is rounding noise, and rotating such
 * entries would never leave them all exactly 0); otherwise a rotation is made if and only if a_pq != 0: theta = (a_qq - a_pp) / (2 a_pq);
 * t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) with sign(0) = +1, or t = 1 / (2 theta) if theta^2 overflows; c = 1 / sqrt(t^2 + 1),
 * s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0 exactly, and for every other r (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq); the
 * vectors turn the same way.  Sweeps continue until one makes no rotation; *sweeps counts them, that last one included; 64 sweeps that
 * all rotated are SCANN_ERR_UNSUPPORTED.  Order: eigenvalue descending, ties by original column ascending.  Sign: the entry of largest
 * magnitude (first index among ties) of each vector is positive.  w [d]; v [d * d], vector c in v[c * d .. c * d + d - 1].
 * Projection.  Inputs: mean [dim]; components W [m * dim], row c one vector, 1 <= m <= dim; scale s [m]; all fp32 and finite.  For a row x:
 *   z_c    = acc_dim,  acc_0 = 0,  acc_{j+1} = fmaf(x[j] - mean[j], W[c][j], acc_j), fp32, columns ascending, the difference rounded once;
 *   md2    = acc_m,  acc_0 = 0,  acc_{c+1} = fmaf(t_c, t_c, acc_c),  t_c = z_c * s_c rounded once, c ascending (with s_c = 1 / sqrt(lambda_c)
 *            the squared Mahalanobis distance; s_c = 0 leaves a component out);
 *   dist2  = the chain of scann_knn_distsq with the row as first and the mean as second argument.
 * A row with a non-finite component gives what the chains give: a NaN stays a NaN (its sign and payload are not part of the definition).
 *
 * scann_index_moments: n_eligible, mean [dim], cov [dim * dim] fp64, col_exp [dim] = f_j (or NULL), bits = b (or NULL) of the pool's rows.
 * Synchronous, one host wait.  Fewer than 2 eligible rows -- an empty pool among them -- are SCANN_ERR_INVALID with a message that says
 * so; n_eligible is written then, the other outputs are not.  scann_index_project: rows [first, first + n) of the pool, device-resident;
 * coords [n * m]; md2, dist2 [n] or NULL (scale may be NULL without md2).  scann_project_batch: one inference forward of the resident
 * batch with the level's output added for that forward only (as scann_index_query_batch: y [n_struct] and ga [n_atom] or NULL are bitwise
 * those of scann_forward_resident + scann_batch_download; range guard, exact-fp32 re-run and SCANN_STRICT_RANGE as there), and the level's
 * rows -- one per structure, or per atom in packed order -- projected device to device.  SCANN_ERR_INVALID before anything is launched,
 * with a message that names the argument: a null handle, pool, batch or output, an index of another handle, rows outside the pool, m
 * outside 1 .. dim, an unknown level, a non-finite mean, component or scale.  The calls change nothing in the pool, the handle's
 * weights, training state or selected outputs, and work on inference and training handles at any width.
 * The twins need no GPU and give the kernels' bits: scann_moments_host (rows [n * dim]; threads over the rows of T, integer sums being
 * order-free), scann_project_host. */
int scann_index_moments(scann_handle_t* h, scann_index_t* pool, int64_t* n_eligible, float* mean /* [dim] */, double* cov /* [dim * dim] */,
                        int32_t* col_exp /* [dim] or NULL */, int32_t* bits /* or NULL */);
int scann_index_project(scann_handle_t* h, scann_index_t* pool, int64_t first, int64_t n, const float* mean, const float* components,
                        const float* scale, int32_t m, float* coords /* [n * m] */, float* md2 /* [n] or NULL */, float* dist2 /* [n] or NULL */);
int scann_project_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* components, const float* scale,
                        int32_t m, float* y, float* ga, float* coords, float* md2, float* dist2);
int scann_moments_host(const float* rows, int64_t n, int64_t dim, int64_t* n_eligible, float* mean, double* cov, int32_t* col_exp, int32_t* bits);
int scann_project_host(const float* rows, int64_t n, int64_t dim, const float* mean, const float* components, const float* scale, int32_t m,
                       float* coords, float* md2, float* dist2);
int scann_sym_eig_host(const double* a, int64_t d, double* w, double* v, int32_t* sweeps);
int scann_pca_bits(int64_t n);  /* b for n eligible rows, 0 <= n < 2^31; SCANN_ERR_INVALID otherwise */

/* ---- a readout head for another property, fitted on an index: ridge regression with exact leave-one-out residuals ----
 * The linear probe of transfer learning: K new targets regressed on the frozen rows of an index, the ridge strength chosen by
 * leave-one-out without a refit (r_i = e_i / (1 - h_i) with the leverage h_i), and the predictive standard deviation
 * sqrt(sigma^2 (1 + leverage)) of Bayesian linear regression as an uncertainty.  Everything is defined so that it depends on the index
 * contents and the targets only, bit for bit.
 * Inputs: a pool of N rows of dim columns and host targets t [N * K] fp32, 1 <= K <= SCANN_HEAD_MAX_TARGETS.  A row counts if and only if
 * all its dim components and all its K targets are finite -- a NaN target means "unlabelled"; n is the number of rows that count.
 * Augmented moments (scann_index_fit_moments): exactly the definition of scann_index_moments applied to the N x (dim + K) matrix
 * [rows | t] -- the same eligibility (over all dim + K columns), column exponents, b = scann_pca_bits(n), int64 sums and fp64 covariance
 * expression.  Outputs: n_eligible, mean [dim + K], cov [(dim + K)^2] fp64, col_exp [dim + K] (or NULL), bits (or NULL).  Its twin is
 * scann_moments_host on the augmented matrix.  Fewer than 2 rows that count are SCANN_ERR_INVALID as there (n_eligible is written).
 * Leave-one-out pass (scann_index_ridge_loo).  Inputs, all fp32 and finite: mean [dim], tmean [K], components V [m * dim] (row c one
 * vector, 1 <= m <= dim), scales S [L * m], coefficients B [L * K * m], lev0, 1 <= L <= SCANN_HEAD_MAX_LAMBDA, and resid_l [K] with
 * entries in -1 .. L - 1, or NULL.  For each row p that counts, in fp32, every operation rounded once and none contracted beyond the
 * stated fmaf:
 *   y_j  = x_j - mean_j;
 *   z_c  = the chain of scann_index_project: acc = fmaf(y_j, V[c][j], acc), j ascending from 0;
 *   t_lc = z_c * S[l][c];   a_l = the chain acc = fmaf(t_lc, t_lc, acc), c ascending from 0 (scann_index_project's md2 with scale S[l]);
 *   lev_l = lev0 + a_l;
 *   p_lk = the chain acc = fmaf(z_c, B[l][k][c], acc), c ascending from 0;
 *   d_k  = t_k - tmean_k;   e_lk = d_k - p_lk;
 *   r_lk = (float)((double)e_lk / (1.0 - (double)lev_l)) if lev_l < 1, else +inf (a NaN leverage gives +inf).
 * Sums, fp64: block g is positions 128 g .. 128 g + 127; within a block acc += term with the position ascending, rows that do not count
 * skipped; then the block sums are added with g ascending.  The block is part of the definition; launch geometry and storage chunks are
 * not.  sse [L * K]: (double)r * (double)r; sae [L * K]: fabs((double)r); sse_fit [L * K]: (double)e * (double)e; dof [L]: (double)lev_l;
 * n_used: the rows that counted.  With resid_l, resid [N * K] fp32 holds r_{resid_l[k], k} for the rows that count, NaN for the others
 * and NaN throughout column k where resid_l[k] = -1.
 * The call is synchronous, one host wait; it changes nothing in the pool, the handle's weights, training state or selected outputs, runs
 * no forward and works on inference and training handles at any width.  SCANN_ERR_INVALID before anything is launched, with a message
 * that names the argument: a null argument, an index of another handle, K, L or m out of range, a non-finite mean, tmean, V, S, B or lev0,
 * a resid_l entry out of range.  An empty pool returns zeros and n_used = 0.  The twin scann_ridge_loo_host (rows [n * dim], no GPU)
 * gives the same bits, threaded over the blocks.
 * Head evaluation (scann_head_batch): one inference forward of a resident batch with the level's output added for that forward only
 * (y, ga, range guard, exact-fp32 re-run and selection restore exactly as scann_project_batch), and for every row of the level
 *   pred_k = tmean_k + w_k, w_k the projection chain of y on W[k] (W [K * dim]);
 *   lev_k  = lev0 + md2 with components V [m * dim] and scale S[k] (S [K * m]: every target has its own ridge strength);
 * pred, lev [n * K]: the bits of scann_project_batch called with (mean, W) and with (mean, V, S[k]), plus one fp32 add each. */
#define SCANN_HEAD_MAX_TARGETS 16
#define SCANN_HEAD_MAX_LAMBDA 32
int scann_index_fit_moments(scann_handle_t* h, scann_index_t* pool, const float* targets /* [N * K] */, int32_t K, int64_t* n_eligible,
                            float* mean /* [dim + K] */, double* cov /* [(dim + K)^2] */, int32_t* col_exp /* [dim + K] or NULL */,
                            int32_t* bits /* or NULL */);
int scann_index_ridge_loo(scann_handle_t* h, scann_index_t* pool, const float* targets /* [N * K] */, int32_t K, const float* mean,
                          const float* tmean, const float* components, int32_t m, const float* scale /* [L * m] */,
                          const float* coef /* [L * K * m] */, int32_t L, float lev0, const int32_t* resid_l /* [K] or NULL */, int64_t* n_used,
                          double* sse /* [L * K] */, double* sae /* [L * K] */, double* sse_fit /* [L * K] */, double* dof /* [L] */,
                          float* resid /* [N * K] or NULL */);
int scann_ridge_loo_host(const float* rows, int64_t n, int64_t dim, const float* targets, int32_t K, const float* mean, const float* tmean,
                         const float* components, int32_t m, const float* scale, const float* coef, int32_t L, float lev0,
                         const int32_t* resid_l, int64_t* n_used, double* sse, double* sae, double* sse_fit, double* dof, float* resid);
int scann_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean, const float* tmean,
                     const float* weights /* [K * dim] */, int32_t K, const float* components /* [m * dim] */, int32_t m,
                     const float* scale /* [K * m] */, float lev0, float* y, float* ga, float* pred /* [n * K] */, float* lev /* [n * K] */);

/* ---- Gaussian landmark features: a nonlinear readout head on an index ----
 * The second half of a probing study: is a property decodable from the frozen latent space at all, by a nonlinear readout.  The feature
 * map is the standard one of kernel ridge regression with a fixed basis (Nystroem / sparse Gaussian process):
 *   phi_c(x) = exp(-|x - z_c|^2 / 2 h^2) = 2^(-dist2(x, z_c) gamma),  gamma = log2(e) / (2 h^2),
 * to m landmarks z_c.  Ridge regression on the features -- the calls above, unchanged, on an index that holds the features -- is sparse
 * GP regression with that basis, and sqrt(sigma^2 (1 + leverage)) its predictive standard deviation.
 * The weight, defined to the bit: scann_rbf_weight(dist2, gamma), no GPU work; the kernel runs the same body.  Every operation is fp32
 * and rounded once, nothing is contracted beyond the stated fmaf:
 *   u = dist2 * gamma;   u NaN -> NaN;   u >= 126 (+inf included) -> 0 (no denormal result ever arises);
 *   i = floorf(u);   g = (u - i) - 0.5f   (g in [-0.5, 0.5));
 *   p = c7;  p = fmaf(p, g, c_j) for j = 6 .. 0;   result = ldexpf(p, -(int)i);
 *   c_j = the fp32 rounding of 2^(-1/2) (-ln 2)^j / j!:  0x1.6a09e6p-1, -0x1.f5e466p-2, 0x1.5be298p-3, -0x1.41839ep-5, 0x1.bdb696p-8,
 *         -0x1.ee4fd2p-11, 0x1.c8d752p-14, -0x1.69e51ep-17.
 * Consequences: scann_rbf_weight(0, gamma) == 1.0f exactly; for dist2 >= 0 the result lies in [0, 1]; against exp2(-(double)u) with the
 * same fp32 u the relative error stays below 3 x 2^-24 on [0, 126) (measured 2.02 x 2^-24).  gamma must be finite and > 0 in the calls
 * below; u < 0 does not arise from a distance (the result is then above 1, +inf from 2^128 on).
 * Features of an index (scann_index_rbf_features): `out` is an EMPTY index of the same handle with dim == m, 1 <= m <= 1024; landmarks
 * is host [m * dim], dim the pool's.  The call appends one row per pool row, in position order, with the pool row's id and atom:
 *   phi[p][c] = scann_rbf_weight(dist2(x_p, z_c), gamma),  dist2 exactly the chain of scann_knn_distsq with the pool row as q.
 * A pool row with any non-finite component gets NaN in all m features (downstream it does not count, as nowhere else).  Between finite
 * values a distance may overflow to +inf, which gives the feature 0, never NaN.  The rows never leave the device; the result depends
 * on the pool contents, the landmarks and gamma only -- not on the chunking, the adds that built the pool or the launch geometry.
 * SCANN_ERR_INVALID before anything is launched, with a message that names the argument: a null argument, an index of another handle,
 * out not empty or out->dim != m, out == pool, m out of range, a non-finite landmark value (landmark and column are named), gamma not
 * finite or <= 0.  An empty pool returns SCANN_OK and appends nothing.  Synchronous, one host wait; inference and training handles at
 * any width; weights, training state and selected outputs are untouched.  scann_rbf_features_host (rows [n * dim], phi [n * m]; no GPU)
 * is the twin: the same bits.
 * A kernel head behind a forward (scann_rbf_head_batch): one inference forward of the resident batch with the level's output added for
 * that forward only (y, ga, range guard, exact-fp32 re-run and selection restore exactly as scann_head_batch), the features of the level's
 * rows where the forward left them (landmarks [m * dim], dim the level's width), and scann_head_batch's evaluation on the FEATURE rows:
 * mean [m], weights [K * m], components [mm * m], 1 <= mm <= m, scale [K * mm].  pred, lev [n * K] are the bits of scann_project_host on
 * phi with (mean, weights) and with (mean, components, scale[k]), plus one fp32 add each; phi [n * m] or NULL receives the features. */
float scann_rbf_weight(float dist2, float gamma);
void scann_rbf_weight_array(const float* dist2, int64_t n, float gamma, float* out);  /* out[i] = scann_rbf_weight(dist2[i], gamma) */
int scann_index_rbf_features(scann_handle_t* h, scann_index_t* pool, const float* landmarks /* host [m * dim] */, int32_t m, float gamma,
                             scann_index_t* out);
int scann_rbf_features_host(const float* rows, int64_t n, int64_t dim, const float* landmarks, int32_t m, float gamma, float* phi /* [n * m] */);
int scann_rbf_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* landmarks, int32_t m, float gamma,
                         const float* mean /* [m] */, const float* tmean /* [K] */, const float* weights /* [K * m] */, int32_t K,
                         const float* components /* [mm * m] */, int32_t mm, const float* scale /* [K * mm] */, float lev0, float* y, float* ga,
                         float* pred /* [n * K] */, float* lev /* [n * K] */, float* phi /* [n * m] or NULL */);

/* ---- A classification head on an index: multinomial logistic regression ----
 * The categorical twin of the readout head: is a class label (metal or insulator, crystal system, the kind of local structure an atom
 * has) decodable from the frozen latent space, with probabilities.  Softmax regression has no closed form, so the fit is iterative; the
 * split keeps a device result a function of the index contents and the arguments only, bit for bit.  The DEVICE PASS below has a fully
 * specified definition: given the weights of M models at once it returns each model's log-likelihood gradient and a few score sums over
 * the rows of the index, in the original coordinates (no projection pass, no N x m scratch).  The OPTIMISER runs on the host in fp64
 * (LatentIndex.fit_class_head) and needs gradients only, so no logarithm has to be defined to the bit.
 * The pass (scann_index_logit_pass), defined to the bit.  Every fp32 operation is rounded once, nothing is contracted beyond the stated
 * fmaf; the host twin and the kernel run the same softmax body (csrc/scann_logit.h).
 *   Rows that count: row p counts iff all its dim components are finite and 0 <= labels[p] < C; -1 means unlabelled.
 *   Folds: the fold of row p is p mod F (p the position in the index), F = 0 or 2 .. 16.  Model j with fold[j] = f >= 0 trains on the
 *     counting rows of the other folds and holds out fold f; with fold[j] = -1 it trains on all counting rows.  F = 0: every entry -1.
 *   Logits of model j (weights U = weights[j], [C][dim + 1]): y_c = x_c - mean_c;  a_k: acc = U[k][dim] (the intercept), then
 *     acc = fmaf(y_c, U[k][c], acc) for c ascending.
 *   Softmax: amax = the fmaxf chain of the a_k, k ascending;  u_k = amax - a_k;  w_k = scann_rbf_weight(u_k, 0x1.715476p+0f) (the
 *     bit-defined 2^-x above: e^-u_k, exactly 1 at the maximum);  S = the sum of the w_k, k ascending;  p_k = w_k / S, the IEEE correctly
 *     rounded division.  Non-finite logits are not special-cased: a NaN propagates into that model's sums.
 *   Per row: r_k = (k == label ? 1.0f : 0.0f) - p_k;  hit: the lowest k that no later logit exceeds (k moves on only for a_k' > a_k)
 *     equals the label;  brier: b = fmaf(e_k, e_k, b) from 0 with e_k = p_k - onehot_k, k ascending.
 *   Sums: fp64 over a fixed tree.  Within a block of 128 consecutive positions acc += term in position order; within a span of 32 blocks
 *     the block sums are added in block order; the span sums are added in span order.  Launch geometry, storage chunks and the grouping
 *     of models into launches are not part of the definition.
 *   grad[j][k][c], c < dim: over the training rows of model j, fma((double)r_k, (double)y_c, acc) (the product is exact);  grad[j][k][dim]:
 *     acc += (double)r_k.  stats[j][0][0 .. 2]: the training rows' count, hits, and brier (acc += (double)brier);  stats[j][1][..]: the
 *     same over the held-out rows.  n_used: the rows that count.  prob [N * C] or NULL: for a row that counts the p_k under model
 *     prob_of_fold[p mod max(F, 1)]; NaN where that entry is -1 and for rows that do not count.
 * SCANN_ERR_INVALID before anything is launched, with a message that names the argument: a null argument, an index of another handle, C
 * outside 2 .. 16, M outside 1 .. 64, F neither 0 nor 2 .. 16, a fold entry outside -1 .. F - 1, a prob_of_fold entry outside -1 .. M - 1, a
 * non-finite mean or weight, a label outside -1 .. C - 1 (the position is named).  An empty pool returns zeros.  Synchronous, one host
 * wait; nothing in the pool, the handle's weights, the training state or the output selection changes; inference and training handles
 * at any width the index accepts.  scann_logit_pass_host (rows [n * dim]; no GPU) is the twin: the same bits.
 * A classification head behind a forward (scann_logit_head_batch): one inference forward of the resident batch with the level's output
 * added for that forward only (y, ga, range guard, exact-fp32 re-run and selection restore exactly as scann_head_batch), then the logit
 * chain and the softmax above on the level's rows where the forward left them: prob [n * C], weights [C * (dim + 1)]. */
#define SCANN_LOGIT_MAX_CLASSES 16
#define SCANN_LOGIT_MAX_MODELS  64
int scann_index_logit_pass(scann_handle_t* h, scann_index_t* pool, const int32_t* labels /* [N] */, int32_t C, const float* mean /* [dim] */,
                           const float* weights /* [M][C][dim + 1] */, int32_t M, const int32_t* fold /* [M] */, int32_t F,
                           const int32_t* prob_of_fold /* [max(F,1)] or NULL */, int64_t* n_used, double* grad /* [M][C][dim + 1] */,
                           double* stats /* [M][2][3] */, float* prob /* [N * C] or NULL */);
int scann_logit_pass_host(const float* rows, int64_t n, int64_t dim, const int32_t* labels, int32_t C, const float* mean, const float* weights,
                          int32_t M, const int32_t* fold, int32_t F, const int32_t* prob_of_fold, int64_t* n_used, double* grad, double* stats,
                          float* prob);
int scann_logit_head_batch(scann_handle_t* h, scann_dbatch_t* db, int32_t level, const float* mean /* [dim] */,
                           const float* weights /* [C][dim + 1] */, int32_t C, float* y, float* ga, float* prob /* [n * C] */);

/* ---- A neighbour embedding (t-SNE) of an index: the iterations on the device ----
 * The two-dimensional map of a latent space that keeps neighbourhoods (van der Maaten & Hinton, JMLR 2008): gradient descent on the
 * Kullback-Leibler divergence between the neighbour affinities p of the rows and the Student-t affinities of the map, with the exact
 * O(N^2) pair repulsion -- no Barnes-Hut, no interpolation --, so that a map is a function of the index contents and the arguments only,
 * bit for bit.  The neighbour graph and the affinities are host work on top of scann_index_query (LatentIndex.embed); the call below runs
 * n_iter iterations of the descent on a symmetric affinity graph in CSR form: row i's entries e in [row_first[i], row_first[i + 1]) name
 * the rows col[e] with the weights p[e].
 * The iteration, defined to the bit.  Every fp32 operation is rounded once, nothing is contracted beyond the stated fmaf, gradual
 * underflow is part of the definition (no flush to zero), and every row reads the y of the iteration's start.  Every sum starts from +0.
 *   Pair (i, j): dx = y[i][0] - y[j][0];  dy = y[i][1] - y[j][1];  d = fmaf(dy, dy, dx * dx);  w = 1.0f / (1.0f + d), the IEEE correctly
 *     rounded division.
 *   Repulsion of row i: positions j ascending, j = i skipped.  Within a block of 128 consecutive positions (block g: 128 g .. 128 g + 127)
 *     the fp32 chains  z = z + w;  ww = w * w;  rx = fmaf(ww, dx, rx);  ry = fmaf(ww, dy, ry).  The block sums, converted to fp64, are
 *     added in block order within a span of 32 blocks; the span sums are added in span order: Z_i, Rx_i, Ry_i.
 *   Z: the sum of the Z_i over the same fp64 tree over i -- 128-row blocks in position order, 32-block spans, spans in order.
 *   Attraction of row i: its entries e ascending, j = col[e], the pair as above:  q = p[e] * w;  ax = fmaf(q, dx, ax);  ay = fmaf(q, dy, ay).
 *   Gradient, fp64, each operation rounded once:  gx = (float)(4.0 * ((double)exaggeration * (double)ax - Rx_i / Z)), and gy alike.
 *   Update, per coordinate:  gain = ((g > 0) == (u > 0)) ? gain * 0.8f : gain + 0.2f;  gain = fmaxf(gain, 0.01f);  t = (lr * gain) * g;
 *     u = fmaf(momentum, u, -t);  y' = y + u.
 *   Centre: mean_c = (float)(S_c / (double)N), S_c the fp64 tree sum of the y'[.][c] over the positions;  y = y' - mean_c.
 * y, u, gain [N * 2] are read and replaced; z_out is the Z and grad_out [N * 2] (or NULL) the gradient of the last iteration.  With
 * n_iter = 0 nothing changes and z_out = 0.  Nothing non-finite that arises during the iterations is special-cased.  Launch geometry, the
 * grouping of spans into workgroups and the work space (24 bytes per row and span: 101 MB at 134 k rows) are not part of the definition.
 * The call uploads once, runs every iteration on the device, downloads once; synchronous, one host wait.  Nothing in the handle's weights,
 * training state, output selection or any index changes; inference and training handles.  SCANN_ERR_INVALID before anything is launched,
 * with a message that names the argument: a null argument, N outside 2 .. SCANN_EMBED_MAX_ROWS, row_first not starting at 0 or
 * decreasing, a column outside 0 .. N - 1 or equal to its own row, a p that is negative or not finite, a non-finite y, u or gain, n_iter
 * outside 0 .. 100000, exaggeration or lr not finite and positive, momentum outside [0, 1).  scann_embed_iterate_host (no GPU) is the
 * twin: the same bits, the repulsion threaded over the rows. */
#define SCANN_EMBED_MAX_ROWS 262144
int scann_embed_iterate(scann_handle_t* h, int64_t N, const int64_t* row_first /* [N + 1] */, const int32_t* col /* [E] */,
                        const float* p /* [E] */, float* y /* [N * 2] in/out */, float* u /* [N * 2] in/out */, float* gain /* [N * 2] in/out */,
                        int32_t n_iter, float exaggeration, float momentum, float lr, double* z_out, float* grad_out /* [N * 2] or NULL */);
int scann_embed_iterate_host(int64_t N, const int64_t* row_first, const int32_t* col, const float* p, float* y, float* u, float* gain,
                             int32_t n_iter, float exaggeration, float momentum, float lr, double* z_out, float* grad_out);

/* ---- Density-peak clustering and kernel density of an index ----
 * A clustering that needs neither k nor round clusters (Rodriguez & Laio, Science 344, 1492, 2014): a row is a cluster centre if it is
 * denser than its surroundings and far from anything denser; every other row follows its nearest denser row.  Both passes are exact
 * O(N^2 dim) self-joins of the index, and the first one, with other rows as queries, is the kernel density of a new structure under the
 * index: the third applicability-domain score beside the mean k-NN distance and the Mahalanobis distance.  The device part is defined to
 * the bit; thresholds, labels and the decision graph are host work on top of it (LatentIndex.density_peaks).
 *   Eligibility: a row is eligible iff all its components are finite (the rule of scann_index_select).
 *   Weight term of a query x against pool row r:  d = dist2(x, r), exactly the chain of scann_knn_distsq with x as q;
 *     w = scann_rbf_weight(d, gamma);  t = llrintf(ldexpf(w, 30)), round to nearest even.  So 0 <= t <= 2^30, and t = 2^30 exactly at
 *     distance 0.  A NaN d contributes nothing (this happens only with a non-finite row).  gamma is finite and > 0.
 *   Density sum: S(x) = the int64 sum of t over the pool rows that count.  N < 2^31, so no order of the adds can overflow, and the sum is
 *     the same in any order: no tree is part of the definition.  An ineligible query gets S = -1.
 *   Density order: row j is ABOVE row i iff S_j > S_i, or S_j == S_i and j < i.
 *   Parent pass over a pool's own rows (the self-join): S_i is summed over the eligible j != i;  parent_i is the first row, under the
 *     total order (dist2 ascending, position ascending), among the eligible rows above i, and delta2_i that dist2.  The one eligible row
 *     with nothing above it (the root) gets parent -1 and delta2 +inf; so does every ineligible row, with S = -1.
 * Consequences: dist2 is symmetric bit for bit; following parents strictly ascends the density order, so the parents form a tree; the
 * result does not depend on the chunking, on how many add calls built the index or on the launch geometry.
 * scann_index_density: nq arbitrary queries (host [nq * dim], dim the pool's) against an index; position skip_pos[i] >= 0 is left out of
 * query i's sum (skip_pos NULL: nothing is).  An empty pool gives 0 for a finite query.  scann_index_peaks: both passes over the pool's own
 * rows, device to device -- nothing N x N-sized is ever stored; sums, parent, delta2 [N]; an empty pool returns SCANN_OK.
 * scann_index_density_batch: one inference forward of the resident batch with the level's output added for that forward only (y
 * [n_struct] and ga [n_atom] or NULL bitwise, range guard, exact-fp32 re-run and selection restore exactly as scann_index_query_batch;
 * generic widths, training handles), then the density of the level's rows where the forward left them: sums [n_struct or n_atom].
 * Synchronous, one host wait per call.  SCANN_ERR_INVALID before anything is launched, with a message that names the argument: a null
 * argument, an index of another handle, gamma not finite or <= 0, a bad level or width, an empty batch.  The calls change nothing in the
 * pool, the handle's weights, the training state or the selected outputs.  scann_density_host and scann_peaks_host (rows [n * dim]; no
 * GPU work, threaded over the rows) are the twins: the kernels' bits. */
int scann_index_density(scann_handle_t* h, scann_index_t* pool, const float* q /* host [nq * dim] */, int64_t nq,
                        const int32_t* skip_pos /* [nq] or NULL */, float gamma, int64_t* sums /* [nq] */);
int scann_index_peaks(scann_handle_t* h, scann_index_t* pool, float gamma, int64_t* sums /* [N] */, int32_t* parent /* [N] */,
                      float* delta2 /* [N] */);
int scann_index_density_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, float gamma, float* y, float* ga,
                              int64_t* sums);
int scann_density_host(const float* rows, int64_t n, int64_t dim, const float* q, int64_t nq, const int32_t* skip_pos, float gamma,
                       int64_t* sums);
int scann_peaks_host(const float* rows, int64_t n, int64_t dim, float gamma, int64_t* sums, int32_t* parent, float* delta2);

/* ---- Hierarchical clustering of an index: the exact minimum spanning tree ----
 * Single linkage and density-based hierarchical clustering (HDBSCAN: Campello, Moulavi & Sander, PAKDD 2013) both rest on one object: the
 * minimum spanning tree of the complete graph over the rows, the second with mutual-reachability weights.  The tree is a series of exact
 * O(N^2 dim) self-joins of the index -- at most ceil(log2 N) rounds of Boruvka's algorithm -- and, under a total order on the edges, it is
 * unique: so it is defined to the bit here.  The dendrogram, the cuts, the condensed tree and the stability selection are host work on
 * the N - 1 edges (LatentIndex.hierarchy, LatentHierarchy).
 *   Eligibility: a row is eligible iff all its components are finite (the rule of scann_index_select / scann_index_peaks).  Ineligible
 *     rows are in no edge.
 *   Weight: for eligible positions i != j,  w(i, j) = max(dist2(i, j), core2[i], core2[j]),  dist2 exactly the chain of
 *     scann_knn_distsq; the max is exact.  With core2 NULL, w = dist2: plain single linkage.  dist2 of two finite rows may overflow to
 *     +inf; such an edge is an ordinary edge and ranks last.  A weight is never NaN and never negative.
 *   Edge order: edges are ordered totally by (w ascending, min(i, j) ascending, max(i, j) ascending).
 *   Result: the unique minimum spanning tree of the complete graph on the eligible rows under that order;
 *     n_edges = max(n_eligible - 1, 0); the edges are listed in ascending order of the edge order, with a[e] < b[e].
 * Consequences: a, b, w and n_edges are a function of the index contents and core2 only, bit for bit -- not of the chunking, of how many
 * add calls built the pool, of the launch geometry or of a thread count.  For a fixed row q the edge order restricted to the edges at q
 * is the order (w, r) of the other end r (rows r < q sort before rows r > q either way), which is what the search of a round walks.
 * rounds (or NULL) receives the number of Boruvka rounds run: at most ceil(log2 n_eligible); it is no part of the definition.
 * scann_index_mst is synchronous (one 12-byte read-back per round -- the edges, the components and the skipped tiles so far --; no kernel waits on another workgroup, and the host stops with an
 * internal error if a round did not reduce the components).  core2 is a host array [N], checked before anything is launched: a NaN or
 * negative entry at any position is SCANN_ERR_INVALID with a message that names it.  An empty pool returns SCANN_OK with 0 edges; a pool
 * above SCANN_MST_MAX_ROWS is SCANN_ERR_UNSUPPORTED before any launch (as scann_embed_iterate: the bound keeps one synchronous call
 * short); an index of another handle or a null output is SCANN_ERR_INVALID.  The call changes nothing in the pool, the handle's weights,
 * the training state or the selected outputs, and works on inference, training, generic-width and exact-fp32 handles.
 * scann_mst_host (rows [n * dim]; no GPU work, the distances threaded over the rows) is the twin: the same bits.
 * scann_mst_last_rounds is a measurement aid (tools/mst_rate.py) with no promise of stability, not part of the definition: the record of
 * the calling thread's last scann_index_mst -- per round (up to cap) the
 * components before it, the host seconds around it and the tiles whose arithmetic the label rule skipped; *tiles: the tiles of one
 * round.  Returns the rounds recorded. */
#define SCANN_MST_MAX_ROWS 262144
int scann_index_mst(scann_handle_t* h, scann_index_t* pool, const float* core2 /* host [N] or NULL */, int64_t* n_edges,
                    int32_t* a /* [max(N - 1, 0)] */, int32_t* b, float* w, int32_t* rounds /* or NULL */);
int scann_mst_host(const float* rows, int64_t n, int64_t dim, const float* core2, int64_t* n_edges, int32_t* a, int32_t* b, float* w);
int scann_mst_last_rounds(int32_t cap, int32_t* components, double* seconds, int64_t* skipped, int64_t* tiles);

/* ---- Silhouette of a labelled index ----
 * Whether a labelling of the rows -- from scann_index_kmeans, from the density peaks, from a cut of the hierarchy -- is any good, and how
 * many clusters the rows support (Rousseeuw, J. Comput. Appl. Math. 20, 53, 1987): for row i, a is its mean distance to the other rows
 * of its own cluster and b the least mean distance to any other cluster; s = (b - a) / max(a, b), formed by the caller.  The pass is an
 * exact O(N^2 dim) self-join of the index and is defined to the bit; the score, its mean and the choice of k are host work on top of it
 * (LatentIndex.silhouette, LatentIndex.choose_k).
 *   Eligibility: a row is eligible iff all its components are finite (the rule of scann_index_select).  A row COUNTS iff it is eligible
 *     and its label is >= 0; labels are host [N], -1 .. C - 1, -1 for noise or unlabelled.  counts[c] = the counting rows with label c.
 *   Term of a counting query i (a row of the index, by position) against a counting row j != i (by position):
 *     d = dist2(row_i, row_j), exactly the chain of scann_knn_distsq with row i as q;  e = d if `squared`, else the correctly rounded fp32
 *     square root of d;  t = llrintf(ldexpf(e, shift)), round to nearest even.  These are the terms of the call: if any of them has e not
 *     finite or t > 2^31, the call returns SCANN_ERR_RANGE and its outputs are unspecified (a lower shift is the remedy).  N < 2^31, so
 *     no order of the adds can overflow int64.
 *   Sums: S[i][c] = the int64 sum of t over the counting rows j != i with label c.  No tree is part of the definition.
 *   Finish, in fp64 IEEE operations, each rounded once, nothing contracted, for a counting query i with label ci:
 *     a_i = ldexp((double)S[i][ci], -shift) / (counts[ci] - 1), or 0 when counts[ci] == 1;
 *     b_i = the least of ldexp((double)S[i][c], -shift) / counts[c] over c != ci with counts[c] > 0, ties to the lower c, other_i that c;
 *     with no such c, b_i = NaN and other_i = -1.
 *     A query that does not count gets a = b = NaN, other = -1, and its row of `sums` is -1.
 * qpos: host [nq] positions 0 .. N - 1 in any order, repeats allowed, or NULL: all N rows in position order (nq is then ignored).
 * counts [C], a, b, other [nq], sums [nq * C] or NULL.
 * Consequences: the result does not depend on the chunking, on how many add calls built the index, on the launch geometry or on a thread
 * count; a qpos subset gives the rows of the full answer; dist2 is symmetric bit for bit.  The call changes nothing in the pool, the
 * handle's weights, the training state or the selected outputs; inference, training and generic-width handles.  Synchronous: one small
 * read-back of the rows' eligibility, then one host wait; the rows never leave the device, and the queries are taken in slices whose
 * device table [slice][C] stays within 512 MiB.
 * SCANN_ERR_INVALID before anything is launched, with a message that names the argument: a null argument, C outside 1 ..
 * SCANN_KMEANS_MAX_K, a label outside -1 .. C - 1, a qpos outside 0 .. N - 1 (the entry is named), shift outside -126 .. 126, a pool of
 * another handle.  An empty pool returns SCANN_OK with zero counts.
 * scann_silhouette_host (rows [n * dim]; no GPU work) is the twin: the same bits, threaded over the queries -- `threads` > 0 fixes the
 * thread count, 0 leaves it to the call (at most 16); the result does not depend on it. */
int scann_index_silhouette(scann_handle_t* h, scann_index_t* pool, const int32_t* labels /* host [N], -1 .. C-1 */, int32_t C,
                           const int32_t* qpos /* host [nq] positions, or NULL: all N rows */, int64_t nq, int32_t squared, int32_t shift,
                           int64_t* counts /* [C] */, double* a /* [nq] */, double* b /* [nq] */, int32_t* other /* [nq] */,
                           int64_t* sums /* [nq * C] or NULL */);
int scann_silhouette_host(const float* rows, int64_t n, int64_t dim, const int32_t* labels, int32_t C, const int32_t* qpos, int64_t nq,
                          int32_t squared, int32_t shift, int32_t threads, int64_t* counts, double* a, double* b, int32_t* other,
                          int64_t* sums);

/* ---- Exact neighbour ranks of an index ----
 * Whether a map of the rows -- the principal-component map, the neighbour embedding -- can be believed is a question about ranks
 * (trustworthiness and continuity: Venna & Kaski, ICANN 2001; the co-ranking framework: Lee & Verleysen, Neurocomputing 72, 1431, 2009):
 * how far down row i's ranking in one space do its neighbours in the other space sit.  The one primitive all these scores need is the
 * rank of row j among all rows, seen from row i: an exact O(N^2 dim) self-join of the index, and a count of integers, so it is defined to
 * the bit without any summation order.  The scores themselves are host work on top of it (LatentIndex.map_quality,
 * LatentIndex.choose_perplexity).
 *   Eligibility: a row is eligible iff all its components are finite (the rule of scann_index_select, scann_index_peaks and
 *     scann_index_silhouette).
 *   Key: for an eligible query i (a row of the pool, by position) and an eligible row l != i,  d(i, l) = dist2(row_i, row_l), exactly
 *     the chain of scann_knn_distsq with row i as q.  Two finite rows never give NaN; +inf is an ordinary value.  The key of l seen from i
 *     is (d(i, l), l) under the search's total order: dist2 ascending, then position ascending.
 *   Rank: for a probe j = probe[i * m + p] that is eligible and != i,  rank[i * m + p] = the number of eligible rows l != i whose key is
 *     strictly less than j's key -- the nearest other row has rank 0 -- and dist2[i * m + p] = d(i, j).
 *   No rank: a probe that is -1, equals i, is ineligible or belongs to an ineligible query gets rank -1 and dist2 +inf.
 *   Probe lists may repeat a position and need no order; equal probes get equal ranks.
 * qpos: host [nq] positions 0 .. N - 1 in any order, repeats allowed, or NULL: all N rows in position order (nq is then ignored).
 * probe: host [nq * m], 1 <= m <= SCANN_RANKS_MAX_PROBES.  rank [nq * m]; dist2 [nq * m] or NULL.
 * Consequences: the result is a function of the pool's contents and the arguments only -- it does not depend on the chunking, on how
 * many add calls built the index, on the launch geometry, on the query slicing or on a thread count; a qpos subset gives the rows of the
 * full answer; the row at place p of query i's leave-self-out answer from scann_index_query has rank p; probing all other rows of an
 * eligible query yields a permutation of 0 .. n_eligible - 2.
 * The call is synchronous with one host wait, the rows never leave the device, and the queries are taken in slices of
 * SCANN_RANKS_SLICE; it changes nothing in the pool, the handle's weights, the training state or the selected outputs and works on
 * inference, training, generic-width and exact-fp32 handles and on an index of any dim 1 .. 1024 (a 2-column index of map coordinates
 * is a first-class use).  SCANN_ERR_INVALID before anything is launched, with a message that names the argument: a null argument, m
 * outside 1 .. SCANN_RANKS_MAX_PROBES, a qpos outside 0 .. N - 1 or a probe outside -1 .. N - 1 (the entry is named), a pool of another
 * handle.  An empty pool returns SCANN_OK.
 * scann_ranks_host (rows [n * dim]; no GPU work) is the twin: the same bits, threaded over the queries -- `threads` > 0 fixes the
 * thread count, 0 leaves it to the call (at most 16); the result does not depend on it. */
#define SCANN_RANKS_MAX_PROBES 32
#define SCANN_RANKS_SLICE 262144
int scann_index_ranks(scann_handle_t* h, scann_index_t* pool,
                      const int32_t* qpos /* host [nq] positions, or NULL: all N rows, nq ignored */, int64_t nq,
                      const int32_t* probe /* host [nq * m] positions, -1: unused */, int32_t m,
                      int32_t* rank /* [nq * m] */, float* dist2 /* [nq * m] or NULL */);
int scann_ranks_host(const float* rows, int64_t n, int64_t dim, const int32_t* qpos, int64_t nq, const int32_t* probe, int32_t m,
                     int32_t threads, int32_t* rank, float* dist2);

/* ---- A partition of an index into cells: the exact nearest-row search that skips cells out of reach ----
 * scann_index_query and everything built on the same search (scann_index_query_batch, the reference pass of scann_index_select, the
 * neighbour graph) compare each query with every row.  Latent rows fall into kinds; a search that knows the kinds can leave most rows
 * unread and still give the brute-force answer IN EVERY BYTE.  A partition is a cell-ordered COPY of the rows attached to the index:
 * it doubles the index's device memory.  The original rows never move and positions keep their meaning.
 * Definition of scann_index_partition(h, idx, cells, max_iter, info), 1 <= cells <= SCANN_KMEANS_MAX_K (cells = 0 drops the partition):
 *   Centres.  The first C = min(cells, eligible rows) picks of scann_index_select(idx, no reference, no threshold), refined by
 *     scann_index_kmeans(init_pos = picks, max_iter, stop_changed = 0); its labels, its dist2 (row to its final centre) and its centres
 *     are used as they come.
 *   Order.  The rows sorted by (label, dist2 to the centre ascending, position ascending); rows with label -1 (a non-finite component)
 *     form a final LOOSE segment in position order.  Every cell, and the loose segment, is padded to whole tiles of 64 entries with pad
 *     entries of position -1; an empty cell has no tile.  A tile therefore belongs to one cell and one shell of distances round its centre.
 *   Per tile.  lo_t / hi_t = the least / greatest dist2 to the centre among the tile's real rows, in the bits scann_index_kmeans returned;
 *     a loose tile has lo = 0, hi = +inf.
 *   Storage.  The copy holds rows, ids and original positions in blocks of the handle's cache, chunked like the index.
 *   Lifetime.  scann_index_add / scann_index_add_batch of one row or more drop the partition (the index then behaves as without one);
 *     scann_index_free frees it.
 *   info [4] (may be NULL): cells in use C, tiles, pad entries, rows of the largest cell.
 * scann_index_cells_read returns info, centres [C * dim], perm [64 * tiles] (original position per entry of the cell order, read back
 * from the device copy; -1: a pad entry), first_tile [C + 2] (first tile of cell c; [C]: first loose tile; [C + 1]: tiles), lo and hi
 * [tiles]; every output may be NULL, so a first call with only info sizes the second; without a partition info is all zero.
 * scann_cells_host(rows [n * dim], ...) is the twin composed of scann_kcenter_host and scann_kmeans_host, the same bytes, no GPU work;
 * its arrays are sized by scann_cells_capacity(n, cells) tiles (perm: 64 times as many entries; centres cells * dim; first_tile cells + 2).
 *
 * The bound.  scann_cell_bound(D, lo, hi), with D = dist2(q, z_c) the chain of scann_knn_distsq with the query first, a = sqrt(D),
 * r_lo = sqrt(lo), r_hi = sqrt(hi), eps = 2^-12, everything in fp64:
 *     g  = max((1 - eps) a - (1 + eps) r_hi,  (1 - eps) r_lo - (1 + eps) a) - 2^-64
 *     lb = g > 0 ? (1 - eps) g^2 : 0,      and lb = 0 whenever D or hi is not finite.
 *   Claim: for every real row x of tile t, the chain value dist2(q, x) >= lb (a NaN chain value never qualifies and is not claimed).
 *   Proof.  Write d(.,.) for the exact Euclidean distance of two fp32 vectors and c(.,.) for the chain.  A finite chain value obeys
 *     c = d^2 (1 + th) + et,  |th| <= gam = (dim + 3) 2^-24 <= 1027 * 2^-24 < 2^-13 = eps / 2  (one rounding of the difference squared,
 *     one per fused step),  |et| <= u = 1024 * 2^-149 = 2^-139  (products that underflow; w = sqrt(u) < 2^-69).
 *     Hence for any pair  (1 - eps/2)(sqrt(c) - w) <= d <= (1 + eps/2)(sqrt(c) + w).  The fp64 square roots and the few fp64 operations
 *     of g are off by relative 2^-52 each, of the larger operand at worst: against the margin between eps and eps/2, i.e. 2^-13 of that
 *     operand, this is nothing, so  d(q, z) >= (1 - eps) a - w,  d(q, z) <= (1 + eps) a + w,  and for a real row x of the tile, whose
 *     c(x, z) lies in [lo, hi]:  d(x, z) <= (1 + eps) r_hi + w,  d(x, z) >= (1 - eps) r_lo - w.  By the triangle inequality on the exact
 *     distances  d(q, x) >= max(d(q, z) - d(x, z), d(x, z) - d(q, z)) >= g + (2^-64 - 2 w) > g + 2^-65.  For g > 0 therefore
 *     d(q, x)^2 > g^2 + 2^-130, and  c(q, x) >= (1 - gam) d(q, x)^2 - u > (1 - gam) g^2 + (1 - gam) 2^-130 - 2^-139 > (1 - eps) g^2 = lb;
 *     a c(q, x) that overflowed is +inf >= lb.  eps carries a four-fold margin over gam at dim 1024 and 2^-64 covers more than three w.
 *     (Checked on the CPU as well: tests/test_cells_host.py walks dim 1 .. 1024 and magnitudes 1e-22 .. 3e18 and finds no violation.)
 *
 * The search.  With a partition, scann_index_query, scann_index_query_batch, scann_index_query_rows and the reference pass of
 * scann_index_select take the pruned route.  Per group of 128 queries (the queries of a pass of up to 1,024 are ordered by their
 * nearest centres, so that a group looks at few cells) a tile may be skipped only if, for EVERY query q of the group, q already holds k qualifying rows with exact chain distances, tau_q
 * being the k-th of them, and scann_cell_bound(D(q, c(t)), lo_t, hi_t) > tau_q, strictly.  Loose tiles are always visited.  Qualifying
 * rows are those of scann_index_query: a NaN distance never qualifies, rows whose id equals the query's id are skipped, +inf is an
 * ordinary value; the order is (dist2, original position).  A skipped row has dist2 >= lb > tau_q, so it is behind k rows that were
 * seen: the output -- dist2, position, id, atom and the +inf / -1 tail -- is scann_index_query's without a partition in every byte.
 * The other analyses over an index (match, kmeans, density, mst, silhouette, ranks, ...) never read the copy.
 * Fall-back.  A pass whose plan keeps more than 1/2 of its (group, tile) pairs -- seeds and survivors over groups x tiles of the copy --
 * is answered by the full kernel if k <= 3, or k <= 7 where the copy has at least 16,384 tiles: there the pruned route measured slower
 * (profiles/cells_rate.txt); at larger k it wins even where it visits every tile, because its second pass drops a distance above tau_q
 * after one compare.  The answer is the same either way.
 * The stats then count, for that pass, its seeds plus every pair of the full search as visited (visited = total + seeds).
 * scann_index_search_stats(idx, out[4]): for the last search on idx the (128-query group, 64-row tile) pairs a full search visits,
 * the pairs visited as seeds, the pairs visited in all, and the groups; without a partition visited == total and seeds == 0.
 * scann_index_partition_args: the (cells, max_iter) the partition was asked for, (0, 0) without one.
 * scann_index_query_rows(h, idx, first, n, k, ...): the queries are rows first .. first + n - 1 of the index itself, read where they
 * lie on the device; the answer is that of scann_index_read followed by scann_index_query (no query ids) in every byte.
 * SCANN_ERR_INVALID before anything is launched: a null argument, an index of another handle, cells outside 0 .. SCANN_KMEANS_MAX_K,
 * max_iter < 0, rows outside the index, k outside 1 .. SCANN_KNN_MAX_K.  All calls are synchronous and change neither weights, training
 * state nor selected outputs. */
int scann_index_partition(scann_handle_t* h, scann_index_t* idx, int32_t cells, int32_t max_iter, int64_t* info /* [4] or NULL */);
int scann_index_partition_args(const scann_index_t* idx, int32_t* cells, int32_t* max_iter);
int scann_index_cells_read(scann_handle_t* h, scann_index_t* idx, int64_t* info /* [4] */, float* centres, int32_t* perm, int32_t* first_tile,
                           float* lo, float* hi);
int scann_index_search_stats(const scann_index_t* idx, int64_t* out /* [4] */);
int scann_index_query_rows(scann_handle_t* h, scann_index_t* idx, int64_t first, int64_t n, int32_t k, float* dist2, int64_t* ids,
                           int32_t* atoms, int32_t* pos);
int64_t scann_cells_capacity(int64_t n, int32_t cells);
int scann_cells_host(const float* rows, int64_t n, int64_t dim, int32_t cells, int32_t max_iter, int64_t* info, float* centres, int32_t* perm,
                     int32_t* first_tile, float* lo, float* hi);
double scann_cell_bound(float D, float lo, float hi);

/* ---- Radius search: the rows within a distance of a query, exact, and near-duplicate pairs ----
 * scann_index_query answers "which are the k nearest rows"; these calls answer "which rows lie within r".  The number of answers per
 * query is unknown beforehand and may be zero, so the calls follow a size-then-fill protocol.
 * Definition.  For a query q, a threshold radius2 and an index, the HITS of q are the rows with dist2(q, row) <= radius2, where
 *   radius2 is fp32, >= 0, and +inf is allowed;
 *   dist2 is exactly the chain of scann_knn_distsq with the query first;
 *   the compare is an fp32 <=, inclusive; a NaN distance never qualifies; +inf is an ordinary value, so it qualifies only at
 *     radius2 = +inf;
 *   with query ids, rows whose id equals the query's are skipped, as in scann_index_query.
 * A query's hits are listed in the total order (dist2 ascending, position ascending).  The first k hits of a query are therefore
 * scann_index_query's first k places wherever those places qualify (tests/test_within_host.py, tests/test_gpu_within.py).
 * The answer is a function of the queries, the index contents and radius2 only, in every byte: the kernel appends hits in the order
 * they arrive, and the order above is established afterwards, by a sort of each query's segment whose keys (dist2, position) are unique.
 * Counts and total.  counts[i] (the hits of query i) and *total (their sum) are always written and always exact; they are integers
 *   added without an order, and a result in their own right: the ball count.
 * Size-then-fill.  If *total <= cap, the hits of query i occupy places [F_i, F_i + counts[i]) of dist2 / pos / ids / atoms, F being the
 *   exclusive prefix sum of counts; any of the four may be NULL.  Otherwise the entry arrays are NOT TOUCHED and the call still returns
 *   SCANN_OK: the caller compares *total with cap and calls again.  cap = 0 with all four arrays NULL is the count-only call; an entry
 *   array given with cap = 0 is SCANN_ERR_INVALID.  0 <= cap <= SCANN_WITHIN_MAX_CAP = 2^30.  The device staging is 12 bytes per entry
 *   of cap; staging that does not fit is SCANN_ERR_OOM before any kernel runs.
 * scann_index_within takes host queries q [nq * dim].  scann_index_within_rows takes rows first .. first + n - 1 of the index itself as
 * the queries, read where they lie (as scann_index_query_rows); the query's own position never qualifies, and upper = 1 keeps only
 * positions greater than the query's.  dist2 is symmetric bit for bit (the difference is negated exactly, its square is the same), so
 * a self-join with upper = 1 lists every unordered pair exactly once.  scann_index_within_batch runs one inference forward of the
 * resident batch with the level's output added for that forward only -- y [n_struct], ga [n_atom] or NULL, the range guard, the
 * exact-fp32 re-run, the selection restore, generic widths and training handles exactly as scann_index_query_batch -- and then searches
 * the level's rows where the forward left them; query_ids [n_struct] or NULL name the structures.
 * With a partition (scann_index_partition) all three take a pruned route: the queries of a pass of up to 1,024 are ordered by their
 * nearest centres as for scann_index_query, and a (group of 128 queries, tile) pair is skipped iff
 *   scann_cell_bound(D(q, c(t)), lo_t, hi_t) > radius2, strictly, for EVERY query q of the group.
 * The claim proved above gives dist2 >= lb > radius2 for every real row of a skipped tile, so no hit is lost.  The threshold is known
 * before the first tile: there are no seeds.  Loose tiles are always visited; pad entries never qualify; positions are the original
 * positions.  The result is that of the index without a partition in every byte.  scann_index_search_stats reports the pass like a
 * search, with seeds = 0 (without a partition and upper = 1 the tiles that lie wholly at or below a group's least query position are
 * not launched, so there visited < total).
 * scann_within_host is the twin: rows [n * dim] with row_ids [n] (NULL: the position), queries q [nq * dim] with query_ids [nq] or NULL
 * and query_pos [nq] (NULL, or the position each query holds in rows: that position never qualifies, and upper = 1, which needs
 * query_pos, keeps only greater positions); counts, total, dist2 and pos are the device's bytes, no GPU work, at most 16 threads.
 * SCANN_ERR_INVALID before anything is launched, with a message that names the argument: a null handle, index, counts or total, an
 * index of another handle, an empty query or batch, rows outside the index, upper not 0 or 1, radius2 NaN or negative, cap negative
 * or above the bound, an entry array with cap = 0, a bad level or width.  An empty index gives zeros.  The calls are synchronous and
 * change nothing in the index, the weights, the training state or the selected outputs. */
#define SCANN_WITHIN_MAX_CAP ((int64_t)1 << 30)
int scann_index_within(scann_handle_t* h, scann_index_t* idx, const float* q, int64_t nq, const int64_t* query_ids, float radius2, int64_t cap,
                       int64_t* counts /* [nq] */, int64_t* total, float* dist2, int32_t* pos, int64_t* ids, int32_t* atoms /* [cap], any may be NULL */);
int scann_index_within_rows(scann_handle_t* h, scann_index_t* idx, int64_t first, int64_t n, int32_t upper, float radius2, int64_t cap,
                            int64_t* counts, int64_t* total, float* dist2, int32_t* pos, int64_t* ids, int32_t* atoms);
int scann_index_within_batch(scann_handle_t* h, scann_index_t* idx, scann_dbatch_t* db, int32_t level, const int64_t* query_ids, float radius2,
                             int64_t cap, float* y, float* ga, int64_t* counts, int64_t* total, float* dist2, int32_t* pos, int64_t* ids,
                             int32_t* atoms);
int scann_within_host(const float* rows, int64_t n, int64_t dim, const int64_t* row_ids, const float* q, int64_t nq, const int64_t* query_ids,
                      const int32_t* query_pos, int32_t upper, float radius2, int64_t cap, int64_t* counts, int64_t* total, float* dist2,
                      int32_t* pos);

/* ---- Prototypes and criticisms of an index: MMD-critic, the greedy loops on the device ----
 * The few rows that stand for all of an index, and the rows those do not stand for (Kim, Khanna & Koyejo, NeurIPS 2016): prototypes are
 * picked greedily so that the kernel mean of the picked set matches the kernel mean of the pool, criticisms are the rows where the two
 * still differ most.  Every quantity is an integer, so the picks are defined to the bit; weights, the witness function and the MMD
 * curve are host work on the calls' integers (LatentIndex.prototypes).
 *   Terms.  Pool P of N rows of dim columns; gamma finite and > 0; a row is eligible iff all its components are finite (the rule of
 *     scann_index_select), n = the number of eligible rows.  t(i, j) = the weight term of scann_index_peaks at dist2(P[i], P[j]), so
 *     0 <= t <= 2^30, t is symmetric bit for bit and t(i, i) = 2^30.  A_i = the int64 sum of t(i, j) over all eligible j, j = i included:
 *     the self-join sum of scann_index_peaks + 2^30.  An ineligible row gets A = -1 and B = 0 and is never picked.
 *   Prototypes.  B_i (int64) starts at 0.  Pick s = 0, 1, .., m-1 is the first row, among the eligible rows not picked yet, under the total
 *     order (score descending, position ascending), score_i = (s + 1) A_i - n B_i, an exact int64.  The call reports the pick's position,
 *     its score and b_at_pick = B_pick; then B_i += t(i, pick) for every eligible i.  The last pick's column is folded as well, so the
 *     returned B is the sum over all picks.  Selection ends after m picks or when no eligible unpicked row is left.
 *   Why this score.  With |S| = s the greedy MMD-critic objective is J(S) = 2/(n s) sum_{l in S} A_l - 1/s^2 sum_{l,l' in S} t(l, l').
 *     J(S + c) differs among the candidates c only through (s + 1) A_c - n B_c, t(c, c) being the same constant for all of them: the
 *     integer score is the exact argmax of J; no summation order and no rounding enter.
 *   Range.  |score| <= N m 2^30.  The calls require N m <= 2^32 (1,024 prototypes of 2.4 M rows, 32,768 of 131,072) and refuse anything
 *     above with SCANN_ERR_INVALID and a message that names both numbers, before anything is launched.  No 128-bit arithmetic.
 *   Criticisms, a weighted greedy selection with kernel suppression.  weight [N] int64, each in 0 .. 2^31 (checked on the host before
 *     anything is launched); a row is live iff it is eligible, not among the excluded positions, and has weight > 0.  Cmax_i (int32)
 *     starts at 0.  Each pick is the first live unpicked row under (score descending, position ascending), score_i = weight_i (2^30 -
 *     Cmax_i) <= 2^61; the selection ends after c picks or when no live row has score > 0.  After a pick Cmax_i = max(Cmax_i, t(i, pick)).
 * Consequences: the first prototype is the densest row, ties to the lowest position; an exact duplicate of a pick falls behind it by
 * n 2^30 and an exact duplicate of a criticism scores 0; the result depends on the pool's contents, gamma and m only, not on the
 * chunking, the number of add calls or the launch geometry.
 * scann_index_prototypes returns the number of picks m' (pos, ids, atoms, score, b_at_pick [m]; behind m': position -1, id -1, atom -1,
 * score 0, b 0; ids, atoms, score, b_at_pick, A [N], B [N] may be NULL); scann_index_criticisms likewise (exclude [n_exclude], positions
 * of the pool).  Synchronous, every launch on one stream, one host wait; an empty pool returns 0.  SCANN_ERR_INVALID before anything is
 * launched, with a message that names the argument: a null handle, pool or pos, a pool of another handle, m or c < 1, gamma not finite or
 * <= 0, N m above 2^32, a weight outside 0 .. 2^31, an excluded position outside the pool.  The calls change nothing in the pool, the
 * weights, the training state or the selected outputs; inference and training handles, any width.  scann_prototypes_host and
 * scann_criticisms_host (rows [n * dim]; no GPU work, threaded over the rows -- the sums are integers, so the thread count cannot enter
 * the result) are the twins: the kernels' bits. */
int64_t scann_index_prototypes(scann_handle_t* h, scann_index_t* pool, int64_t m, float gamma, int32_t* pos, int64_t* ids, int32_t* atoms,
                               int64_t* score, int64_t* b_at_pick /* [m] */, int64_t* A /* [N] or NULL */, int64_t* B /* [N] or NULL */);
int64_t scann_index_criticisms(scann_handle_t* h, scann_index_t* pool, const int64_t* weight /* [N] */, const int32_t* exclude,
                               int64_t n_exclude, int64_t c, float gamma, int32_t* pos, int64_t* ids, int32_t* atoms, int64_t* score /* [c] */);
int64_t scann_prototypes_host(const float* rows, int64_t n, int64_t dim, int64_t m, float gamma, int32_t* pos, int64_t* score,
                              int64_t* b_at_pick, int64_t* A, int64_t* B);
int64_t scann_criticisms_host(const float* rows, int64_t n, int64_t dim, const int64_t* weight, const int32_t* exclude, int64_t n_exclude,
                              int64_t c, float gamma, int32_t* pos, int64_t* score);

int scann_comm_unique_id(char* out128);                       /* ncclGetUniqueId on rank 0; broadcast by the caller */
int scann_comm_init(scann_handle_t* h, const char* id128, int rank, int world);
/* ranks of the handle's RCCL communicator as RCCL reports them (ncclCommCount); 0 without a communicator (single rank, or the
 * collective-free inference path); negative status on error.  bench.py --train prints it as `rccl_ranks`. */
int scann_comm_ranks(scann_handle_t* h);
/* Data-parallel start-up: every rank's master parameters become rank `root`'s (one flat ncclBroadcast) and the packed
 * device images are regenerated from them, so that replicas created with different initialiser draws train ONE model
 * (the reference is single-process: create_model runs once, scann_model.py:77).  No-op without a communicator.
 * Needs scann_train_begin. */
int scann_broadcast_weights(scann_handle_t* h, int root);

/* ---- model sets: several weight sets of one architecture in one forward ------------------------------------------------------------
 * A model set is K (1..16) weight sets of the handle's scann_config_t -- K targets of one dataset, or K seeds of one target (a deep
 * ensemble) -- run over one resident batch by the same launches: every atom, edge, merge and readout launch of scann_forward_models
 * covers all K members (grids of K x the tiles of one member).  Member m's y and GlobalAttention scores are bitwise what a handle holding
 * only member m's weights (and its relu_out) gives through scann_forward_resident + scann_batch_download for the same batch.
 * Generic widths run the members one after another on the plain-fp32 kernels; a member with |w| >= 255.9 in a 128x128 kernel runs alone
 * on the exact-fp32 kernels (the others still share their launches).  The set leaves the handle's own weights, predictions, selected
 * outputs (a set forward writes none), training state and the batch's last single-model y untouched.
 *
 * scann_models_load replaces the handle's set, atomically: on any error the previous set stays.  Member m is validated exactly like
 * scann_load_weights (blobs[m], manifests[m], n_tensors[m] as its blob / manifest / n); relu_out[m] is its mrelu flag (target e_b), or
 * relu_out NULL: all cfg.relu_out.  scann_models_count: the members of the handle's set (0: none). */
int scann_models_load(scann_handle_t* h, int32_t n_models, const float* const* blobs, const scann_tensor_desc_t* const* manifests,
                      const int32_t* n_tensors, const int32_t* relu_out);
int scann_models_count(const scann_handle_t* h);
/* Enqueue one forward of every member over a resident batch on stream slot `stream_slot` (asynchronous; SCANN_ERR_WEIGHTS without a
 * set).  The batch keeps one workspace block for the members, allocated by its first set forward and freed with it.  A batch's set forwards
 * are tracked apart from its single-model forwards: scann_batch_download waits for the batch's last single forward only, a set forward
 * queues behind an earlier set forward of the batch on another stream, and scann_batch_release synchronises the device while a set forward
 * has not been waited for by scann_models_download. */
int scann_forward_models(scann_handle_t* h, scann_dbatch_t* db, int stream_slot);
/* Wait for the batch's last set forward and copy its results, member-major: y[K * n_struct], ga[K * n_atom] (or NULL).  If that
 * forward's range guard fired, every member is run again on the exact-fp32 kernels first (one count of scann_exact_reruns; each member
 * then equals its single handle under SCANN_EXACT=1); with SCANN_STRICT_RANGE=1 the result is SCANN_ERR_RANGE.  A device-packing error
 * of a scann_upload_padded batch is reported here.  SCANN_ERR_INVALID if no forward of the handle's current set (the last
 * scann_models_load) ran on the batch. */
int scann_models_download(scann_handle_t* h, scann_dbatch_t* db, float* y, float* ga);

/* ---- host batch packers (no GPU work) --------------------------------------------------------------
 * Replace DataIterator.__getitem__ + pad_sequence / pad_nested_sequences (datagenerator.py:69-135, general.py:14-50).
 * All arrays are caller-allocated; on error the return is SCANN_ERR_INVALID and scann_pack_last_error() has the text
 * (thread-local). */
const char* scann_pack_last_error(void);
/* Padded Keras input dict (scann_model.py:338-357) -> packed CSR.  atomic[B,M] or NULL with cgcnn[B,M,92];
 * ring[B,M,2] or NULL; masks as bytes.  Outputs sized for the worst case: out_atomic[B*M], out_cgcnn[B*M*92],
 * out_ring[B*M*2], out_mol_offset[B+1], out_edge_offset[B*M+1], out_edge_col/dist/weight[B*M*N];
 * out_row_of[B*M] = packed row of (b, m) or -1 for padded atoms (used to re-pad the GlobalAttention scores). */
int scann_pack_padded(int32_t B, int32_t M, int32_t N, const int32_t* atomic, const float* cgcnn,
                      const uint8_t* atom_mask, const int32_t* neighbors, const uint8_t* neighbor_mask,
                      const float* neighbor_weight, const float* neighbor_distance, const float* ring,
                      int32_t* out_atomic, float* out_cgcnn, float* out_ring, int32_t* out_mol_offset,
                      int32_t* out_edge_offset, int32_t* out_edge_col, float* out_edge_dist,
                      float* out_edge_weight, int32_t* out_row_of, int32_t* n_atom, int32_t* n_edge);
/* A whole dataset kept in CSR form (ds_mol_offset[n_struct_total+1] atoms per structure, ds_edge_offset[atoms+1],
 * ds_edge_local = neighbour index INSIDE its structure as stored by the preprocessing, voronoi_neighbor.py:38-47):
 * the batch made of structures sel[0..n_sel) in that order (the structures DataIterator.__getitem__(idx) would hold).
 * scann_slice_count gives the output sizes first. */
int scann_slice_count(const int64_t* ds_mol_offset, const int64_t* ds_edge_offset, const int64_t* sel, int32_t n_sel,
                      int64_t n_struct_total, int64_t* n_atom, int64_t* n_edge);
int scann_slice_batch(const int64_t* ds_mol_offset, const int64_t* ds_edge_offset, const int32_t* ds_atomic,
                      const float* ds_ring, const int32_t* ds_edge_local, const float* ds_edge_dist,
                      const float* ds_edge_weight, const int64_t* sel, int32_t n_sel, int64_t n_struct_total,
                      int32_t* out_atomic, float* out_ring, int32_t* out_mol_offset, int32_t* out_edge_offset,
                      int32_t* out_edge_col, float* out_edge_dist, float* out_edge_weight);
/* The host half of scann_upload_padded (host only; exposed so that it can be checked without a GPU): the MASKS of a padded Keras input
 * (1-byte bool / uint8 or 4-byte float32 / int32 elements) -> mol_offset[B+1], edge_offset[n_atom+1] (capacity B*M+1) and the packed row
 * of every padded atom slot, row_of[B*M] (-1: padded).  Same arrays as scann_pack_padded gives. */
int scann_count_padded(int32_t B, int32_t M, int32_t N, const void* atom_mask, int32_t atom_mask_size, const void* neighbor_mask,
                       int32_t neighbor_mask_size, int32_t* out_mol_offset, int32_t* out_edge_offset, int32_t* out_row_of,
                       int32_t* n_atom, int32_t* n_edge);
/* The staging copy of the padded path (host only): memcpy on up to 8 threads for blocks of >= 8 MiB (disjoint ranges, joined before the
 * return); what scann_upload_padded / scann_forward_padded move the payload arrays into pinned memory with.  Exposed so that it can be
 * checked without a GPU and under ThreadSanitizer (tests/test_tsan.py). */
int scann_host_copy(void* dst, const void* src, int64_t bytes);
/* The edge-tile plan scann_batch_upload builds for a packed batch (host only; exposed so that it can be checked without a
 * GPU): whole atoms per tile, <= tile_rows (32 | 64) edges and <= tile_atoms (<= 32) atoms; with allow_chunks an atom with
 * more than 64 neighbours becomes ceil(deg/64) single-atom chunk tiles, part_out[tile] = its softmax-merge slot (-1 for
 * ordinary tiles), otherwise such a batch is SCANN_ERR_UNSUPPORTED.  tiles_out[cap][4] = atom_begin, atom_end, edge_begin,
 * edge_end.  Returns the planned edge rows per tile (32 | 64) or a negative status (text: scann_pack_last_error). */
int scann_plan_tiles(const scann_batch_t* batch, int32_t tile_rows, int32_t tile_atoms, int32_t allow_chunks, int32_t cap,
                     int32_t* tiles_out, int32_t* part_out, int32_t* n_tiles, int32_t* n_slots);
/* The FILLED edge-tile plan of the inference edge kernels (host only, for the same reason): a tile's atoms need not be a contiguous
 * range of the batch.  atom_row_out[n_atom] = the caller's row of the k-th atom in TILE ORDER, a permutation that never leaves a
 * structure (inside a structure: the remaining atom of the largest degree that still fits the open tile, the lowest row among
 * equals; the open tile carries over into the next structure); tile_offset_out[n_atom + 1] = the CSR offsets of the atoms in that
 * order (an atom's edges stay contiguous and in their order); tiles_out[cap][4] = atom_begin, atom_end, edge_begin, edge_end in
 * tile-order numbering.  When that does not take FEWER tiles than scann_plan_tiles (same tile_rows, tile_atoms, chunks allowed), or
 * the batch has an atom of more than tile_rows neighbours, the result is the identity order and the contiguous tiles.
 * Returns 1 (filled), 0 (identity) or a negative status (text: scann_pack_last_error). */
int scann_plan_tiles_filled(const scann_batch_t* batch, int32_t tile_rows, int32_t tile_atoms, int32_t cap, int32_t* atom_row_out,
                            int32_t* tile_offset_out, int32_t* tiles_out, int32_t* n_tiles);
/* Which plan the piece-major inference edge kernels run a resident batch on: out2[0] = 1 when it is the filled plan (made when the
 * batch is forwarded a second time, unless SCANN_TILE_FILL=0 was set when the handle was created, an atom is chunked, or best fit
 * saves no tile), out2[1] = its tiles.  scann_batch_info goes on reporting the contiguous plan. */
int scann_batch_tile_plan(scann_handle_t* h, const scann_dbatch_t* batch, int32_t* out2);

#ifdef __cplusplus
}
#endif
#endif /* SCANN_HIP_H */

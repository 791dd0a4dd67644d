// Resident batches: upload (a host-packed CSR batch, or the padded Keras arrays packed on the device), results download with the
// exact-fp32 re-run, release, and the synchronous forward paths built on them (scann_forward, scann_forward_padded).
#include "scann_runtime.h"

namespace {

// Device packing (scann_upload_padded): the payload arrays of a padded Keras input dict, which go to the device AS THEY ARE and are
// compacted there (pack_padded_kernel); `b` then carries the counts and the two offset arrays only (host: scann_count_padded).
struct PaddedSrc {
  int32_t M, N;
  const int32_t *atomic, *neighbors;
  const void* neighbor_mask;
  int32_t mask_size;
  const float *weight, *dist;
  const int32_t* row_of;  // [B*M] host
  // the payload arrays are ALREADY on their way to the device (scann_forward_padded enqueued the copy on the stream the upload uses,
  // before it read the masks): their device addresses; null: upload_impl stages and copies them itself
  const int32_t *d_atomic = nullptr, *d_neighbors = nullptr;
  const void* d_mask = nullptr;
  const float *d_weight = nullptr, *d_dist = nullptr;
};

}  // namespace

// (the threaded staging copy of the padded payload: scann_host_copy, scann_pack.cpp -- host-only code, built under ThreadSanitizer too)
static inline void par_memcpy(void* dst, const void* src, size_t bytes) { (void)scann_host_copy(dst, src, (int64_t)bytes); }

static int upload_impl(scann_handle_t* h, const scann_batch_t* b, scann_dbatch_t** out, bool scratch, const PaddedSrc* pad = nullptr) {
  if (!h || !b || !out) return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: null argument");
  *out = nullptr;
  const int32_t B = b->n_struct, A = b->n_atom, E = b->n_edge;
  if (B <= 0 || A <= 0 || E < 0) return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: empty batch");
  if (!b->mol_offset || !b->edge_offset ||
      (!pad && ((!b->atomic && !h->cfg.feature_cgcnn) || (E > 0 && (!b->edge_col || !b->edge_dist || !b->edge_weight)))))
    return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: null array");
  if (pad && (h->cfg.feature_cgcnn || h->cfg.use_ring || h->t_master))
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_upload_padded: atomic feature without ring, inference handles (a training handle needs the edges on the host)");
  if (b->mol_offset[0] != 0 || b->mol_offset[B] != A || b->edge_offset[0] != 0 || b->edge_offset[A] != E)
    return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: offsets do not cover the batch");
  int32_t max_atoms = 0;
  for (int s = 0; s < B; ++s) {
    const int32_t n = b->mol_offset[s + 1] - b->mol_offset[s];
    if (n <= 0) return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: structure without atoms");
    max_atoms = std::max(max_atoms, n);
  }
  if ((size_t)max_atoms * 5 * sizeof(float) > 60000) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_batch_upload: structure too large");
  if ((uint64_t)std::max(A, E) * D * 4 >= (1ull << 32))  // edge_kernel addresses a tensor row as base + 32-bit byte offset
    return fail(h, SCANN_ERR_UNSUPPORTED, "scann_batch_upload: more than 8,388,607 atoms or edges in one batch; split it");
  if (pad) {
    // (atomic numbers and neighbour indices are checked where they are read: pack_padded_kernel's flag word, scann_batch_download)
  } else if (!h->cfg.feature_cgcnn) {
    for (int a = 0; a < A; ++a)
      if (b->atomic[a] < 0 || b->atomic[a] >= h->cfg.n_atoms)
        return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: atomic number outside the embedding table (n_atoms)");
  } else if (!b->cgcnn) {
    return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: feature=cgcnn needs batch.cgcnn [n_atom,92]");
  }
  if (h->cfg.use_ring && !b->ring) return fail(h, SCANN_ERR_INVALID, "scann_batch_upload: use_ring needs batch.ring [n_atom,2]");
  std::vector<int32_t> edge_row;
  std::vector<EdgeTile> tiles;
  std::vector<int32_t> tile_part, big_tab;  // atoms with more than TE_MAX neighbours (edge_kernel_lean only)
  int32_t n_slot = 0, max_degree = 0;
  int tile_rows = TE_MAX;
  {
    std::string err;
    // A launch that fits ONE round of workgroups is the latency chain of a tile: 32-row tiles (four workgroups per CU = 1,024 slots)
    // make that chain shorter.  Only when no atom needs chunking at 32 rows: such a batch is planned at 32 rows first (one pass for
    // the reference's batch of 128) and again at 64 if an atom turns out to have more than 32 neighbours.
    const bool small = E > 0 && E <= 32 * 1024;
    int r = plan_tiles(b->mol_offset, B, b->edge_offset, pad ? nullptr : b->edge_col, A, E, small ? 32 : TE_MAX, h->tile_atoms, true, tiles,
                       tile_part, big_tab, edge_row, &tile_rows, &max_degree, &n_slot, err, false);
    if (r) return fail(h, r, "scann_batch_upload: " + err);
    if (small && max_degree > 32) {
      r = plan_tiles(b->mol_offset, B, b->edge_offset, pad ? nullptr : b->edge_col, A, E, TE_MAX, h->tile_atoms, true, tiles, tile_part, big_tab, edge_row,
                     &tile_rows, &max_degree, &n_slot, err, false);
      if (r) return fail(h, r, "scann_batch_upload: " + err);
    }
  }
  const int32_t n_big = (int32_t)big_tab.size() / 3;
  // The piece-major inference edge kernels find a tile's atoms through per-tile slot tables (EdgeArgs::tile_atom), built behind the copy
  // (launch_tile_order): here for the contiguous plan.  The filled plan, in which a tile's atoms need not be a contiguous range, costs
  // the host more than one forward gains from it: it is made when the batch is forwarded AGAIN (ensure_tile_fill).
  const bool tile_side = h->cfg.g_update && !h->generic && E > 0;
  const size_t n_ftile = tiles.size();
  HIPCHK(h, hipSetDevice(h->device));
  scann_dbatch* db = nullptr;
  if (scratch) {
    if (!h->sc_db) h->sc_db = new scann_dbatch();
    db = h->sc_db;
    if (db->dbg_c || db->stamps) (void)hipStreamSynchronize(h->streams[0]);
    cached_free(db->dbg_c);
    cached_free(db->dbg_g);
    cached_free(db->dbg_ctx);
    cached_free(db->fill_block);
    if (db->stamps) (void)hipFree(db->stamps);
    char* const gen_ws = db->gen_ws;  // (the generic-width forward's workspace is kept across calls, like the arena below)
    const size_t gen_ws_bytes = db->gen_ws_bytes;
    char* const out_block = db->out_block;  // (... and so is the block of the inference outputs)
    const size_t out_cap = db->out_cap;
    char* const mc_ws = db->mc_ws;  // (... and scann_predict_mc's)
    const size_t mc_bytes = db->mc_bytes;
    char* const set_ws = db->set_ws;  // (... and scann_forward_models')
    const size_t set_bytes = db->set_bytes;
    *db = scann_dbatch();
    db->set_ws = set_ws; db->set_bytes = set_bytes;
    db->gen_ws = gen_ws; db->gen_ws_bytes = gen_ws_bytes;
    db->out_block = out_block; db->out_cap = out_cap;
    db->mc_ws = mc_ws; db->mc_bytes = mc_bytes;
    db->owns_arena = false;
  } else {
    db = new scann_dbatch();
  }
  db->n_struct = B; db->n_atom = A; db->n_edge = E; db->n_tile = (int32_t)tiles.size(); db->max_atoms = max_atoms; db->tile_rows = tile_rows; db->max_degree = max_degree; db->tile_atoms = h->tile_atoms; db->n_big = n_big; db->n_slot = n_slot;
  // arena layout: inputs first (one H2D copy), then workspace
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes); return o; };
  const size_t o_atomic = take((size_t)A * 4), o_mol = take((size_t)(B + 1) * 4), o_eoff = take((size_t)(A + 1) * 4);
  const size_t o_col = take((size_t)E * 4), o_row = take((size_t)E * 4), o_dist = take((size_t)E * 4), o_wgt = take((size_t)E * 4);
  const size_t o_tiles = take(tiles.size() * sizeof(EdgeTile));
  const size_t o_tpart = take(n_big ? tiles.size() * 4 : 0), o_big = take((size_t)n_big * 3 * 4);
  const size_t o_inoff = take((size_t)(A + 1) * 4), o_inedge = take((size_t)E * 4);
  const size_t o_ring = take(h->cfg.use_ring ? (size_t)A * 2 * 4 : 0), o_cg = take(h->cfg.feature_cgcnn ? (size_t)A * 92 * 4 : 0);
  // device packing: the padded payload as it came (transient: read once by pack_padded_kernel), the row map and the flag word
  const size_t BM = pad ? (size_t)B * pad->M : 0, BMN = pad ? BM * pad->N : 0;
  const bool pre = pad && pad->d_atomic;  // the payload is already on the device
  const size_t o_prow = take(BM * 4), o_pat = take(pre ? 0 : BM * 4), o_pnbr = take(pre ? 0 : BMN * 4);
  const size_t o_pmask = take(pad && !pre ? BMN * pad->mask_size : 0), o_pw = take(pre ? 0 : BMN * 4), o_pd = take(pre ? 0 : BMN * 4);
  const size_t in_bytes = off;
  const size_t rowA = (size_t)A * D * 4, rowE = (size_t)std::max(E, 1) * D * 4;
  const size_t o_geom = take(h->cfg.g_update ? rowE + D * 4 : 0);  // + the spare row edge-less tiles store to (EdgeArgs::n_edge)
  const size_t o_gd = take(h->cfg.g_update ? 0 : (size_t)std::max(E, 1) * NG * 4);
  const size_t o_c0 = take((h->cfg.use_ring || h->cfg.feature_cgcnn) ? rowA : 0);
  const size_t o_c = take(rowA), o_ctx = take(rowA), o_P1 = take(rowA), o_P3 = take(rowA), o_q = take(rowA);
  const size_t o_gq = take(rowA), o_gk = take(rowA), o_ga = take((size_t)A * 4), o_y = take((size_t)B * 4);
  const size_t o_pflag = take(pad ? 4 : 0);  // right behind y: fetched with the results in one copy
  const size_t o_pbuf = take((size_t)n_slot * 3 * D * 4);
  const size_t slot_bytes = tile_side ? n_ftile * TQ * 4 : 0;
  const size_t o_tatom = take(slot_bytes), o_te0 = take(slot_bytes), o_tsp = take(h->cfg.feature_cgcnn ? 0 : slot_bytes);
  hipError_t e = hipSuccess;
  scann_handle::Stage* stage = nullptr;
  char* img_ptr = nullptr;
  if (scratch) {
    if (off > h->sc_cap) {  // grow-only (dynamic M, N: SURVEY 8b "workspace sized on first call and grown monotonically")
      if (h->sc_arena) { (void)hipStreamSynchronize(h->streams[0]); (void)hipFree(h->sc_arena); h->sc_arena = nullptr; h->sc_cap = 0; }
      const size_t want = off + off / 2;
      e = hipMalloc((void**)&h->sc_arena, want);
      if (e == hipSuccess) h->sc_cap = want;
    }
    if (e == hipSuccess && in_bytes > h->sc_host_cap) {
      if (h->sc_host) { (void)hipStreamSynchronize(h->streams[0]); (void)hipHostFree(h->sc_host); h->sc_host = nullptr; h->sc_host_cap = 0; }
      const size_t want = in_bytes + in_bytes / 2;
      e = hipHostMalloc((void**)&h->sc_host, want, hipHostMallocDefault);
      if (e == hipSuccess) h->sc_host_cap = want;
    }
    db->arena = h->sc_arena;
    img_ptr = h->sc_host;
  } else {
    e = cached_malloc((void**)&db->arena, off);
    if (e == hipSuccess && !h->copy_stream) e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) {  // next pinned staging buffer of the ring: free once its previous copy has completed (normally long ago)
      stage = &h->stage[h->stage_next++ % scann_handle::N_STAGE];
      if (stage->used) (void)hipEventSynchronize(stage->ev);
      if (!stage->ev) e = hipEventCreateWithFlags(&stage->ev, hipEventDisableTiming);  // (the host waits on it: a default, fenced event)
      if (e == hipSuccess && in_bytes > stage->cap) {
        if (stage->p) (void)hipHostFree(stage->p);
        stage->p = nullptr; stage->cap = 0;
        const size_t want = in_bytes + in_bytes / 4;
        e = hipHostMalloc((void**)&stage->p, want, hipHostMallocDefault);
        if (e == hipSuccess) stage->cap = want;
      }
      img_ptr = stage->p;
    }
  }
  if (e != hipSuccess) {
    if (!scratch) {
      if (db->arena) cached_free(db->arena);
      delete db;
    }
    return fail(h, e == hipErrorOutOfMemory ? SCANN_ERR_OOM : SCANN_ERR_HIP, std::string("hipMalloc(batch arena): ") + hipGetErrorString(e));
  }
  struct ImgView { char* p; char* data() const { return p; } } img{img_ptr};
  if (b->atomic && !pad) memcpy(img.data() + o_atomic, b->atomic, (size_t)A * 4);
  if (pad) memcpy(img.data() + o_prow, pad->row_of, BM * 4);
  if (pad && !pre) {
    memcpy(img.data() + o_pat, pad->atomic, BM * 4);
    par_memcpy(img.data() + o_pnbr, pad->neighbors, BMN * 4);
    par_memcpy(img.data() + o_pmask, pad->neighbor_mask, BMN * pad->mask_size);
    par_memcpy(img.data() + o_pw, pad->weight, BMN * 4);
    par_memcpy(img.data() + o_pd, pad->dist, BMN * 4);
  }
  if (h->cfg.use_ring) memcpy(img.data() + o_ring, b->ring, (size_t)A * 2 * 4);
  if (h->cfg.feature_cgcnn) memcpy(img.data() + o_cg, b->cgcnn, (size_t)A * 92 * 4);
  memcpy(img.data() + o_mol, b->mol_offset, (size_t)(B + 1) * 4);
  memcpy(img.data() + o_eoff, b->edge_offset, (size_t)(A + 1) * 4);
  if (E > 0 && !pad) {
    memcpy(img.data() + o_col, b->edge_col, (size_t)E * 4);
    memcpy(img.data() + o_dist, b->edge_dist, (size_t)E * 4);
    memcpy(img.data() + o_wgt, b->edge_weight, (size_t)E * 4);
  }
  memcpy(img.data() + o_tiles, tiles.data(), tiles.size() * sizeof(EdgeTile));
  // reverse adjacency (counting sort of the edges by neighbour atom, stable): the backward pass sums per neighbour without atomics.
  // Only a handle in training mode (scann_train_begin) pays for it at upload; ensure_reverse builds it for a batch that was
  // uploaded before, on its first backward pass.
  const bool want_rev = h->t_master != nullptr;
  if (want_rev) {
    int32_t* in_off = reinterpret_cast<int32_t*>(img.data() + o_inoff);
    int32_t* in_edge = reinterpret_cast<int32_t*>(img.data() + o_inedge);
    memset(in_off, 0, (size_t)(A + 1) * 4);
    for (int e = 0; e < E; ++e) ++in_off[b->edge_col[e] + 1];
    for (int a = 0; a < A; ++a) in_off[a + 1] += in_off[a];
    std::vector<int32_t> fill(in_off, in_off + A);
    for (int e = 0; e < E; ++e) in_edge[fill[b->edge_col[e]]++] = e;
  }
  if (n_big) {
    memcpy(img.data() + o_tpart, tile_part.data(), tiles.size() * 4);
    memcpy(img.data() + o_big, big_tab.data(), (size_t)n_big * 3 * 4);
  }
  // (the centre atom of every edge is derived from the offsets on the device, behind the copy: no host loop, no bytes over the bus)
  int32_t* const d_eoff = (int32_t*)(db->arena + o_eoff);
  int32_t* const d_erow = (int32_t*)(db->arena + o_row);
  PackPaddedArgs pa{};
  if (pad) {
    char* a0 = db->arena;
    pa.B = B; pa.M = pad->M; pa.N = pad->N; pa.n_species = h->cfg.n_atoms;
    pa.row_of = (const int32_t*)(a0 + o_prow); pa.edge_offset = d_eoff; pa.atomic = pre ? pad->d_atomic : (const int32_t*)(a0 + o_pat);
    pa.neighbors = pre ? pad->d_neighbors : (const int32_t*)(a0 + o_pnbr); pa.neighbor_mask = pre ? pad->d_mask : a0 + o_pmask;
    pa.mask_size = pad->mask_size;
    pa.weight = pre ? pad->d_weight : (const float*)(a0 + o_pw); pa.dist = pre ? pad->d_dist : (const float*)(a0 + o_pd);
    pa.out_atomic = (int32_t*)(a0 + o_atomic); pa.out_col = (int32_t*)(a0 + o_col);
    pa.out_dist = (float*)(a0 + o_dist); pa.out_weight = (float*)(a0 + o_wgt);
    pa.flag = (int32_t*)(a0 + o_pflag);
  }
  TileOrderArgs ta{};
  if (tile_side) {
    char* a0 = db->arena;
    ta.tiles = (const EdgeTile*)(a0 + o_tiles); ta.n_tile = (int32_t)n_ftile; ta.n_atom = A;
    ta.edge_offset = d_eoff; ta.atomic = h->cfg.feature_cgcnn ? nullptr : (const int32_t*)(a0 + o_atomic);
    ta.tile_atom = (int32_t*)(a0 + o_tatom); ta.tile_edge0 = (int32_t*)(a0 + o_te0); ta.tile_species = (int32_t*)(a0 + o_tsp);
  }
  // (the pack kernel's flag word is zeroed by edge_row_kernel, launched BEFORE it: no memset command of its own)
  if (scratch) {
    if (e == hipSuccess) e = hipMemcpyAsync(db->arena, img.data(), in_bytes, hipMemcpyHostToDevice, h->streams[0]);
    if (e == hipSuccess && (E > 0 || pad)) launch_edge_row(d_eoff, E > 0 ? A : 0, d_erow, h->streams[0], pad ? pa.flag : nullptr);
    if (e == hipSuccess && pad) launch_pack_padded(pa, h->streams[0]);
    if (e == hipSuccess && tile_side) launch_tile_order(ta, h->streams[0]);
  } else {
    if (e == hipSuccess) e = hipMemcpyAsync(db->arena, img.data(), in_bytes, hipMemcpyHostToDevice, h->copy_stream);
    if (e == hipSuccess && (E > 0 || pad)) launch_edge_row(d_eoff, E > 0 ? A : 0, d_erow, h->copy_stream, pad ? pa.flag : nullptr);
    if (e == hipSuccess && pad) launch_pack_padded(pa, h->copy_stream);
    if (e == hipSuccess && tile_side) launch_tile_order(ta, h->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(stage->ev, h->copy_stream);
    if (e == hipSuccess) stage->used = true;
    // a default (system-fenced) event: it orders a DMA engine's write into a REUSED arena (cached_malloc) before kernels on another
    // stream, whose caches may still hold lines of the arena's previous life -- not the place for the fence-free timing-event flavour
    if (e == hipSuccess) e = hipEventCreateWithFlags(&db->upload_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(db->upload_ev, h->copy_stream);
  }
  if (e != hipSuccess) {
    if (!scratch) {
      (void)hipStreamSynchronize(h->copy_stream);
      if (db->upload_ev) (void)hipEventDestroy(db->upload_ev);
      cached_free(db->arena);
      delete db;
    }
    return fail(h, SCANN_ERR_HIP, std::string("hipMemcpy(batch inputs): ") + hipGetErrorString(e));
  }
  char* a0 = db->arena;
  db->atomic = (int32_t*)(a0 + o_atomic); db->mol_offset = (int32_t*)(a0 + o_mol); db->edge_offset = (int32_t*)(a0 + o_eoff);
  db->edge_col = (int32_t*)(a0 + o_col); db->edge_row = (int32_t*)(a0 + o_row);
  db->dist = (float*)(a0 + o_dist); db->weight = (float*)(a0 + o_wgt); db->tiles = (EdgeTile*)(a0 + o_tiles);
  db->in_off = (int32_t*)(a0 + o_inoff); db->in_edge = (int32_t*)(a0 + o_inedge);
  db->has_rev = want_rev;
  db->n_ftile = (int32_t)n_ftile;
  db->f_tiles = db->tiles; db->t_offset = db->edge_offset; db->t_col = db->edge_col; db->t_row = db->edge_row;
  db->t_dist = db->dist; db->t_weight = db->weight;
  if (tile_side) {
    db->tile_atom = (int32_t*)(a0 + o_tatom); db->tile_edge0 = (int32_t*)(a0 + o_te0);
    db->tile_species = h->cfg.feature_cgcnn ? nullptr : (int32_t*)(a0 + o_tsp);
  }
  db->ring = (float*)(a0 + o_ring); db->cgcnn = (float*)(a0 + o_cg); db->c0 = (float*)(a0 + o_c0);
  db->geom = (float*)(a0 + o_geom); db->gd = (float*)(a0 + o_gd);
  db->c = (float*)(a0 + o_c); db->ctx = (float*)(a0 + o_ctx); db->P1 = (float*)(a0 + o_P1); db->P3 = (float*)(a0 + o_P3);
  db->q = (float*)(a0 + o_q); db->gq = (float*)(a0 + o_gq); db->gk = (float*)(a0 + o_gk);
  db->ga = (float*)(a0 + o_ga); db->y = (float*)(a0 + o_y);
  db->pack_flag = pad ? (int32_t*)(a0 + o_pflag) : nullptr;
  if (n_big) {
    db->tile_part = (int32_t*)(a0 + o_tpart); db->big_tab = (int32_t*)(a0 + o_big); db->part_buf = (float*)(a0 + o_pbuf);
  }
  *out = db;
  return SCANN_OK;
}

// y (and the GlobalAttention scores) of the batch's last forward -> the caller's arrays: one D2H into the slot's pinned block, then
// plain memcpy (two hipMemcpyAsync into pageable numpy arrays were two staged copies: 23 us of a one-batch call's 280;
// polling the stream before the blocking wait changed nothing: hipStreamSynchronize already spins for waits this short)
static int fetch_results(scann_handle_t* h, scann_dbatch_t* db, hipStream_t s, float* y_out, float* ga_attn_out) {
  const char* src = reinterpret_cast<const char*>(ga_attn_out ? db->ga : db->y);
  const size_t y_off = (size_t)(reinterpret_cast<const char*>(db->y) - src);
  const size_t f_off = db->pack_flag ? (size_t)(reinterpret_cast<const char*>(db->pack_flag) - src) : 0;  // (behind y in the arena)
  const size_t bytes = db->pack_flag ? f_off + 4 : y_off + (size_t)db->n_struct * 4;
  scann_handle::DlStage& st = h->dl_stage[db->last_slot];
  if (st.cap < bytes) {
    if (st.p) {
      HIPCHK(h, hipStreamSynchronize(s));
      (void)hipHostFree(st.p);
      st.p = nullptr;
      st.cap = 0;
    }
    const size_t cap = std::max<size_t>(bytes + bytes / 2, (size_t)1 << 16);
    HIPCHK(h, hipHostMalloc((void**)&st.p, cap, hipHostMallocDefault));
    st.cap = cap;
  }
  HIPCHK(h, hipMemcpyAsync(st.p, src, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (db->pack_flag) {  // a batch packed on the device: what the host packer refuses when it packs, the kernel reports here
    const int32_t bad = *reinterpret_cast<const int32_t*>(st.p + f_off);
    if (bad & 1) return fail(h, SCANN_ERR_INVALID, "scann_batch_download: an unmasked neighbour slot points at a padded atom (or outside the structure)");
    if (bad & 2) return fail(h, SCANN_ERR_INVALID, "scann_batch_download: atomic number outside the embedding table (n_atoms)");
  }
  if (y_out) memcpy(y_out, st.p + y_off, (size_t)db->n_struct * 4);
  if (ga_attn_out) memcpy(ga_attn_out, st.p, (size_t)db->n_atom * 4);
  return SCANN_OK;
}

namespace scann {

void free_batch(scann_dbatch* db) {
  if (db->arena && db->owns_arena) cached_free(db->arena);
  cached_free(db->gen_ws);
  cached_free(db->out_block);
  cached_free(db->mc_ws);
  cached_free(db->set_ws);
  cached_free(db->dbg_c);
  cached_free(db->dbg_g);
  cached_free(db->dbg_ctx);
  cached_free(db->fill_block);
  if (db->stamps) (void)hipFree(db->stamps);
  if (db->upload_ev) (void)hipEventDestroy(db->upload_ev);
  delete db;
}

// A batch packed on the device (scann_upload_padded) carries what pack_padded_kernel found wrong with the input in a flag word that
// scann_batch_download reads with the results.  The entry points that hand device-side tensors back WITHOUT a download (read_csr,
// forward_profile, debug_read) read the word themselves -- otherwise they would return the kernel's sanitised stand-ins (col = row,
// z = 0) as if they were the caller's data.  Call with the packing finished (upload event or stream synchronised).
int check_pack_flag(scann_handle_t* h, scann_dbatch_t* db, const char* who) {
  if (!db->pack_flag) return SCANN_OK;
  int32_t bad = 0;
  HIPCHK(h, hipMemcpy(&bad, db->pack_flag, 4, hipMemcpyDeviceToHost));
  if (bad & 1) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": an unmasked neighbour slot points at a padded atom (or outside the structure)");
  if (bad & 2) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": atomic number outside the embedding table (n_atoms)");
  return SCANN_OK;
}

// The filled plan of a batch that is forwarded again (run_forward): the host plans it from the offsets read back, one block of the
// device cache takes the plan, the tile-order copies of the edges and the slot tables, and launch_tile_order fills it on `s`, which is
// waited for -- once per batch; the forwards that follow, on whatever stream, find the block complete.  A one-shot batch (the streamed
// and padded calls, a dataset pass) never comes here: planning costs the host about what the plan saves the device in thirty forwards.
int ensure_tile_fill(scann_handle_t* h, scann_dbatch_t* db, hipStream_t s) {
  if (db->fill_tried) return SCANN_OK;
  db->fill_tried = true;
  if (!h->tile_fill || !db->tile_atom || db->n_big > 0 || db->n_tile <= 1) return SCANN_OK;
  const int32_t B = db->n_struct, A = db->n_atom, E = db->n_edge;
  std::vector<int32_t> mol((size_t)B + 1), eoff((size_t)A + 1), atom_row, tile_offset;
  std::vector<EdgeTile> ftiles;
  if (db->upload_ev && !db->upload_done) HIPCHK(h, hipEventSynchronize(db->upload_ev));
  else if (!db->upload_ev) HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  HIPCHK(h, hipMemcpy(mol.data(), db->mol_offset, mol.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(eoff.data(), db->edge_offset, eoff.size() * 4, hipMemcpyDeviceToHost));
  const std::vector<EdgeTile> contiguous((size_t)db->n_tile);  // (its size is what the filled plan has to beat)
  if (!plan_tiles_filled(mol.data(), B, eoff.data(), A, db->tile_rows, db->tile_atoms, contiguous, db->n_big, atom_row, tile_offset, ftiles))
    return SCANN_OK;
  const size_t nt = ftiles.size();
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes); return o; };
  const size_t o_arow = take((size_t)A * 4), o_toff = take((size_t)(A + 1) * 4), o_ftiles = take(nt * sizeof(EdgeTile));
  const size_t in_bytes = off;
  const size_t o_tcol = take((size_t)E * 4), o_trow = take((size_t)E * 4), o_tdist = take((size_t)E * 4), o_twgt = take((size_t)E * 4);
  const size_t o_tatom = take(nt * TQ * 4), o_te0 = take(nt * TQ * 4), o_tsp = take(db->tile_species ? nt * TQ * 4 : 0);
  std::vector<char> img(in_bytes);
  memcpy(img.data() + o_arow, atom_row.data(), (size_t)A * 4);
  memcpy(img.data() + o_toff, tile_offset.data(), (size_t)(A + 1) * 4);
  memcpy(img.data() + o_ftiles, ftiles.data(), nt * sizeof(EdgeTile));
  char* blk = nullptr;
  if (cached_malloc((void**)&blk, off) != hipSuccess) return SCANN_OK;  // (no room for it: the contiguous plan goes on)
  hipError_t e = hipMemcpy(blk, img.data(), in_bytes, hipMemcpyHostToDevice);
  TileOrderArgs ta{};
  ta.tiles = (const EdgeTile*)(blk + o_ftiles); ta.n_tile = (int32_t)nt; ta.n_atom = A;
  ta.atom_row = (const int32_t*)(blk + o_arow); ta.tile_offset = (const int32_t*)(blk + o_toff);
  ta.edge_offset = db->edge_offset; ta.atomic = db->tile_species ? db->atomic : nullptr;
  ta.col = db->edge_col; ta.dist = db->dist; ta.weight = db->weight;
  ta.tile_atom = (int32_t*)(blk + o_tatom); ta.tile_edge0 = (int32_t*)(blk + o_te0); ta.tile_species = (int32_t*)(blk + o_tsp);
  ta.out_col = (int32_t*)(blk + o_tcol); ta.out_row = (int32_t*)(blk + o_trow);
  ta.out_dist = (float*)(blk + o_tdist); ta.out_weight = (float*)(blk + o_twgt);
  if (e == hipSuccess) {
    launch_tile_order(ta, s);
    e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    cached_free(blk);
    return fail(h, SCANN_ERR_HIP, std::string("filled tile plan: ") + hipGetErrorString(e));
  }
  db->fill_block = blk;
  db->filled = true; db->n_ftile = (int32_t)nt;
  db->f_tiles = (EdgeTile*)(blk + o_ftiles); db->t_offset = (int32_t*)(blk + o_toff);
  db->t_col = ta.out_col; db->t_row = ta.out_row; db->t_dist = ta.out_dist; db->t_weight = ta.out_weight;
  db->tile_atom = ta.tile_atom; db->tile_edge0 = ta.tile_edge0;
  if (db->tile_species) db->tile_species = ta.tile_species;
  return SCANN_OK;
}

int rerun_if_out_of_range(scann_handle_t* h, scann_dbatch_t* db, hipStream_t s, bool* rerun) {
  *rerun = false;
  if (!h->range_flag || h->strict_range || db->kept) return SCANN_OK;
  const int32_t code = *reinterpret_cast<volatile int32_t*>(h->range_flag + db->last_slot);
  const int site = code >> 8;
  if (!code || site < 1 || site > 4) return SCANN_OK;
  h->range_flag[db->last_slot] = 0;
  FwdOpts o;  // (what the batch recorded for the forward that is run again, not what the handle selects by now)
  o.exact = true;
  o.out_layers = db->out_layers;
  o.out_flags = db->out_flags;
  const int r = run_forward(h, db, s, o);
  if (r) return r;
  h->exact_reruns++;
  *rerun = true;
  HIPCHK(h, hipStreamSynchronize(s));
  return SCANN_OK;
}

// scann_batch_download behind its argument checks
static int download(scann_handle_t* h, scann_dbatch_t* db, float* y_out, float* ga_attn_out) {
  hipStream_t s = h->streams[db->last_slot];
  const int rf = fetch_results(h, db, s, y_out, ga_attn_out);
  if (rf) return rf;
  // The forward's range guard fired: an activation left the range of the split-fp16 projections (sites 1-4).  The reference runs any
  // fp32 values (attention.py:95-113), so the forward is run again on the exact-fp32 instantiations (1/16 of the matrix rate, this
  // batch only) instead of handing an error back -- unless SCANN_STRICT_RANGE=1 asks for the error.
  bool rerun = false;
  if (const int r = rerun_if_out_of_range(h, db, s, &rerun)) return r;
  if (rerun) {
    const int rf3 = fetch_results(h, db, s, y_out, ga_attn_out);
    if (rf3) return rf3;
  }
  db->idle = true;
  db->fwd_pending = false;
  return check_range(h, "scann_batch_download", db->last_slot);
}

int forward_and_download(scann_handle_t* h, scann_dbatch_t* db, uint64_t layers, int32_t flags, float* y, float* ga) {
  HIPCHK(h, hipSetDevice(h->device));
  if (const int r = run_forward(h, db, h->streams[db->last_slot], selected_opts(h, layers, flags))) return r;
  return download(h, db, y, ga);
}

int read_mol_offset(scann_handle_t* h, const scann_dbatch_t* db, std::vector<int32_t>& mol) {
  mol.assign((size_t)db->n_struct + 1, 0);
  if (db->upload_ev && !db->upload_done) HIPCHK(h, hipEventSynchronize(db->upload_ev));
  if (db->n_struct > 0) HIPCHK(h, hipMemcpy(mol.data(), db->mol_offset, mol.size() * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

}  // namespace scann

extern "C" {

int scann_batch_upload(scann_handle_t* h, const scann_batch_t* b, scann_dbatch_t** out) { return upload_impl(h, b, out, false); }

int scann_upload_padded(scann_handle_t* h, int32_t B, int32_t M, int32_t N, const int32_t* atomic, const void* atom_mask,
                        int32_t atom_mask_size, const int32_t* neighbors, const void* neighbor_mask, int32_t neighbor_mask_size,
                        const float* neighbor_weight, const float* neighbor_distance, scann_dbatch_t** out, int32_t* n_atom_out,
                        int32_t* n_edge_out) {
  if (!h || !out || B <= 0 || M <= 0 || N < 0 || !atomic || !atom_mask || (N > 0 && (!neighbors || !neighbor_mask || !neighbor_weight || !neighbor_distance)))
    return fail(h, SCANN_ERR_INVALID, "scann_upload_padded: bad argument");
  *out = nullptr;
  const size_t BM = (size_t)B * M;
  std::vector<int32_t> row_of(BM), mol((size_t)B + 1), eoff(BM + 1);  // (per call: the caller may upload from a second thread)
  int32_t na = 0, ne = 0;
  if (scann_count_padded(B, M, N, atom_mask, atom_mask_size, neighbor_mask, neighbor_mask_size, mol.data(), eoff.data(), row_of.data(), &na, &ne))
    return fail(h, SCANN_ERR_INVALID, std::string("scann_upload_padded: ") + scann_pack_last_error());
  scann_batch_t pb{};
  pb.n_struct = B; pb.n_atom = na; pb.n_edge = ne; pb.mol_offset = mol.data(); pb.edge_offset = eoff.data();
  const PaddedSrc src{M, N, atomic, neighbors, neighbor_mask, neighbor_mask_size, neighbor_weight, neighbor_distance, row_of.data()};
  const int r = upload_impl(h, &pb, out, false, &src);
  if (r) return r;
  if (n_atom_out) *n_atom_out = na;
  if (n_edge_out) *n_edge_out = ne;
  return SCANN_OK;
}

void scann_batch_free(scann_handle_t* h, scann_dbatch_t* db) {
  if (!db) return;
  if (h) (void)hipSetDevice(h->device);
  if (h) (void)hipDeviceSynchronize();
  free_batch(db);
}

// scann_batch_free without the device-wide synchronisation: for a batch whose last use was a scann_train_step that has been ended
// (its event has fired), or a forward whose results have been downloaded (scann_batch_download waits for the batch's stream), while
// LATER work on other batches may still be running.  Falls back to the synchronising free otherwise.
void scann_batch_release(scann_handle_t* h, scann_dbatch_t* db) {
  if (!db) return;
  const bool step_done = db->busy_ev && hipEventQuery(db->busy_ev) == hipSuccess;
  if (!h || !(step_done || (db->idle && db->set_busy < 0))) {  // (a set forward not yet downloaded: scann_models_download)
    scann_batch_free(h, db);
    return;
  }
  (void)hipSetDevice(h->device);
  free_batch(db);
}

int scann_batch_info(scann_handle_t* h, const scann_dbatch_t* db, int32_t* out8) {
  if (!h || !db || !out8) return fail(h, SCANN_ERR_INVALID, "scann_batch_info: null argument");
  out8[0] = db->n_struct; out8[1] = db->n_atom; out8[2] = db->n_edge; out8[3] = db->n_big;
  out8[4] = db->n_slot; out8[5] = db->max_degree; out8[6] = db->n_tile; out8[7] = db->tile_rows;
  return SCANN_OK;
}

int scann_batch_tile_plan(scann_handle_t* h, const scann_dbatch_t* db, int32_t* out2) {
  if (!h || !db || !out2) return fail(h, SCANN_ERR_INVALID, "scann_batch_tile_plan: null argument");
  out2[0] = db->filled ? 1 : 0;
  out2[1] = db->tile_atom ? db->n_ftile : db->n_tile;
  return SCANN_OK;
}

int scann_batch_download(scann_handle_t* h, scann_dbatch_t* db, float* y_out, float* ga_attn_out) {
  if (!h || !db || !y_out) return fail(h, SCANN_ERR_INVALID, "scann_batch_download: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  return download(h, db, y_out, ga_attn_out);
}

int scann_device_memory(scann_handle_t* h, int64_t* free_bytes, int64_t* total_bytes) {
  if (!h || !free_bytes || !total_bytes) return fail(h, SCANN_ERR_INVALID, "scann_device_memory: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  size_t f = 0, t = 0;
  HIPCHK(h, hipMemGetInfo(&f, &t));
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return SCANN_OK;
}

int scann_forward(scann_handle_t* h, const scann_batch_t* batch, float* y_out, float* ga_attn_out) {
  // synchronous convenience path: the batch lives in the handle's reusable scratch (no hipMalloc per call)
  scann_dbatch_t* db = nullptr;
  int r = upload_impl(h, batch, &db, true);
  if (r) return r;
  r = scann_forward_resident(h, db, 0);
  if (!r) r = scann_batch_download(h, db, y_out, ga_attn_out);
  return r;
}

int scann_forward_padded(scann_handle_t* h, int32_t B, int32_t M, int32_t N, const int32_t* atomic, const uint8_t* atom_mask,
                         const int32_t* neighbors, const uint8_t* neighbor_mask, const float* neighbor_weight,
                         const float* neighbor_distance, float* y_out, float* ga_out) {
  if (!h || B <= 0 || M <= 0 || N < 0 || !atomic || !atom_mask || !y_out || (N > 0 && (!neighbors || !neighbor_mask || !neighbor_weight || !neighbor_distance)))
    return fail(h, SCANN_ERR_INVALID, "scann_forward_padded: bad argument");
  if (h->cfg.use_ring || h->cfg.feature_cgcnn) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_forward_padded: atomic feature without ring only");
  const size_t BM = (size_t)B * M;
  // the handle's own packing buffers, grown when a call needs more: seven fresh vectors per call were 0.6 MB of mmap + page faults +
  // zero fill at the reference's batch size -- a good part of what a one-batch call spends before the device can start
  scann_handle::PadScratch& ps = h->pad_scratch;
  auto grow_i = [](std::vector<int32_t>& v, size_t n) { if (v.size() < n) v.resize(n + n / 4); };
  auto grow_f = [](std::vector<float>& v, size_t n) { if (v.size() < n) v.resize(n + n / 4); };
  grow_i(ps.gidx, BM); grow_i(ps.mol, (size_t)B + 1); grow_i(ps.eoff, BM + 1);
  std::vector<int32_t>&gidx = ps.gidx, &mol = ps.mol, &eoff = ps.eoff;
  int32_t na = 0, ne = 0;
  // the host reads the MASKS only (real atoms, degrees -> offsets, tile plan); the payload arrays go to the device as they are and
  // are compacted there (pack_padded_kernel) -- a training handle, whose uploads carry the reverse adjacency, packs on the host
  const bool device_pack = !h->t_master;
  scann_batch_t pb{};
  std::vector<float>& ga_packed = ps.ga;
  int r;
  if (device_pack) {
    // The payload (13/14 of the bytes) does not depend on what the masks say: it is staged and its copy ENQUEUED first, on the stream the
    // rest of the call uses, and crosses the bus while this thread reads the masks and plans the tiles -- for one batch of 128 the copy
    // (~25 us) and the mask pass + plan (~20 us) used to run one after the other in front of the first launch.
    HIPCHK(h, hipSetDevice(h->device));
    const size_t BMN = BM * (size_t)N;
    const size_t p_at = 0, p_nbr = align_up(BM * 4), p_mask = p_nbr + align_up(BMN * 4), p_w = p_mask + align_up(BMN), p_d = p_w + align_up(BMN * 4);
    const size_t p_bytes = p_d + align_up(BMN * 4);
    if (p_bytes > h->pp_cap) {
      HIPCHK(h, hipStreamSynchronize(h->streams[0]));
      if (h->pp_dev) (void)hipFree(h->pp_dev);
      if (h->pp_host) (void)hipHostFree(h->pp_host);
      h->pp_dev = h->pp_host = nullptr;
      h->pp_cap = 0;
      const size_t want = p_bytes + p_bytes / 2;
      HIPCHK(h, hipMalloc((void**)&h->pp_dev, want));
      HIPCHK(h, hipHostMalloc((void**)&h->pp_host, want, hipHostMallocDefault));
      h->pp_cap = want;
    }
    memcpy(h->pp_host + p_at, atomic, BM * 4);
    if (BMN) {
      par_memcpy(h->pp_host + p_nbr, neighbors, BMN * 4);
      par_memcpy(h->pp_host + p_mask, neighbor_mask, BMN);
      par_memcpy(h->pp_host + p_w, neighbor_weight, BMN * 4);
      par_memcpy(h->pp_host + p_d, neighbor_distance, BMN * 4);
    }
    HIPCHK(h, hipMemcpyAsync(h->pp_dev, h->pp_host, p_bytes, hipMemcpyHostToDevice, h->streams[0]));
    if (scann_count_padded(B, M, N, atom_mask, 1, neighbor_mask, 1, mol.data(), eoff.data(), gidx.data(), &na, &ne)) {
      (void)hipStreamSynchronize(h->streams[0]);  // (the staging block is about to be reusable again)
      return fail(h, SCANN_ERR_INVALID, std::string("scann_forward_padded: ") + scann_pack_last_error());
    }
    pb.n_struct = B; pb.n_atom = na; pb.n_edge = ne; pb.mol_offset = mol.data(); pb.edge_offset = eoff.data();
    PaddedSrc src{M, N, atomic, neighbors, neighbor_mask, 1, neighbor_weight, neighbor_distance, gidx.data()};
    src.d_atomic = (const int32_t*)(h->pp_dev + p_at); src.d_neighbors = (const int32_t*)(h->pp_dev + p_nbr); src.d_mask = h->pp_dev + p_mask;
    src.d_weight = (const float*)(h->pp_dev + p_w); src.d_dist = (const float*)(h->pp_dev + p_d);
    if (ga_out) grow_f(ps.ga, (size_t)na);
    scann_dbatch_t* db = nullptr;
    r = upload_impl(h, &pb, &db, true, &src);
    if (!r) r = scann_forward_resident(h, db, 0);
    if (!r) r = scann_batch_download(h, db, y_out, ga_out ? ga_packed.data() : nullptr);
  } else {
    grow_i(ps.at, BM); grow_i(ps.col, BM * N + 1); grow_f(ps.dist, BM * N + 1); grow_f(ps.wgt, BM * N + 1);
    if (scann_pack_padded(B, M, N, atomic, nullptr, atom_mask, neighbors, neighbor_mask, neighbor_weight, neighbor_distance,
                          nullptr, ps.at.data(), nullptr, nullptr, mol.data(), eoff.data(), ps.col.data(), ps.dist.data(), ps.wgt.data(),
                          gidx.data(), &na, &ne))
      return fail(h, SCANN_ERR_INVALID, std::string("scann_forward_padded: ") + scann_pack_last_error());
    pb.n_struct = B; pb.n_atom = na; pb.n_edge = ne;
    pb.atomic = ps.at.data(); pb.mol_offset = mol.data(); pb.edge_offset = eoff.data();
    pb.edge_col = ps.col.data(); pb.edge_dist = ps.dist.data(); pb.edge_weight = ps.wgt.data();
    if (ga_out) grow_f(ps.ga, (size_t)na);
    r = scann_forward(h, &pb, y_out, ga_out ? ga_packed.data() : nullptr);
  }
  if (r) return r;
  if (ga_out)
    for (size_t i = 0; i < BM; ++i) ga_out[i] = gidx[i] >= 0 ? ga_packed[gidx[i]] : 0.f;  // softmax of -1e9 -> 0
  return SCANN_OK;
}

int scann_batch_read_csr(scann_handle_t* h, scann_dbatch_t* db, int32_t* atomic, int32_t* mol_offset, int32_t* edge_offset, int32_t* edge_col,
                         float* edge_dist, float* edge_weight) {
  if (!h || !db) return fail(h, SCANN_ERR_INVALID, "scann_batch_read_csr: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  if (db->upload_ev) HIPCHK(h, hipEventSynchronize(db->upload_ev));
  else HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  if (const int rp = check_pack_flag(h, db, "scann_batch_read_csr")) return rp;
  const size_t A = (size_t)db->n_atom, E = (size_t)db->n_edge;
  if (atomic) HIPCHK(h, hipMemcpy(atomic, db->atomic, A * 4, hipMemcpyDeviceToHost));
  if (mol_offset) HIPCHK(h, hipMemcpy(mol_offset, db->mol_offset, ((size_t)db->n_struct + 1) * 4, hipMemcpyDeviceToHost));
  if (edge_offset) HIPCHK(h, hipMemcpy(edge_offset, db->edge_offset, (A + 1) * 4, hipMemcpyDeviceToHost));
  if (edge_col && E) HIPCHK(h, hipMemcpy(edge_col, db->edge_col, E * 4, hipMemcpyDeviceToHost));
  if (edge_dist && E) HIPCHK(h, hipMemcpy(edge_dist, db->dist, E * 4, hipMemcpyDeviceToHost));
  if (edge_weight && E) HIPCHK(h, hipMemcpy(edge_weight, db->weight, E * 4, hipMemcpyDeviceToHost));
  return SCANN_OK;
}

}  // extern "C"

// The body of edge_kernel<GUPD, RT, FB, EX, KEEP, DEAD, ATTN, MC> (scann_kernels.hip) as text, in a file of its own (round 4's layer launches included
// it a second time; as an inlined device function the same body moved hipcc's register allocation of the 168-VGPR kernel: +3.7 %).
// Expects in scope: GUPD, RT, FB, EX, KEEP (training forward: the keep_* stores and the attention
// dropout exist), DEAD (geom' is not stored), ATTN (inference outputs: the attention weights are stored), MC (Monte Carlo dropout on the
// attention weights with structure-local masks, scann_predict_mc), BLK (piece-major geometry
// tiles), TEK; `a` (EdgeArgs); LDS sTile [2 TEK PLANE_STRIDE halfs],
// sQ [TQ LDS_STRIDE], sE [NHEAD (TEK + 1)] with the index maps SE_STAT(wave, row) / SE_LOGIT(row, head), sPar [5 D], sOff [TQ + 1],
// sRow / sCen / sE0 [TQ] (BLK: the tile's slots of EdgeArgs::tile_atom / tile_cen / tile_edge0);
// SCANN_EDGE_TIX = the edge tile of this workgroup.
  _Float16* const sH = reinterpret_cast<_Float16*>(sTile);
  _Float16* const sL = sH + TEK * PLANE_STRIDE;
  float* const sK = reinterpret_cast<float*>(sTile);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tix = SCANN_EDGE_TIX;
  const EdgeTile tile = a.tiles[tix];
  const int part = a.tile_part ? a.tile_part[tix] : -1;  // >= 0: one <= 64-edge chunk of an atom with more than 64 neighbours
  const int eb = tile.edge_begin, ne = tile.edge_end - eb, natom = tile.atom_end - tile.atom_begin;
  const int nem1 = ne > 0 ? ne - 1 : 0;
  // Ragged tail: the rows of a tile past its last edge (row >= ne) are DUPLICATES of the last real row -- every per-row load is issued from
  // the clamped row min(row, ne - 1), a row's arithmetic depends on nothing but that row's own inputs (MFMA output row r = X row r . W;
  // batch-composition tests), and every per-row store goes to the clamped row's address: the duplicate lanes write the last row's own
  // bytes onto it.  So nothing below is predicated per lane on `row < ne` (no selects, no exec-mask branches around the epilogues' LDS
  // reads); the softmax walks sOff's edge ranges and never sees a tail row.  A tile without edges (`live` false, uniform) stores no edge row.
  const bool live = ne > 0;
  const int lrow = lane & 31, lh = lane >> 5;  // accumulator layout: this lane's rows lrow, lrow + 32; column runs 32 wave + 8 j + 4 lh
  const int cbase = 32 * wave + 4 * lh;
  // BLK (inference: the geometry tensor has no reader but the next layer's launch of this kernel on the SAME tile plan): a tile's geometry
  // rows are stored piece-major, [32 pieces of 4 columns][ne rows] x 16 B behind the tile's first row, instead of row-major: one
  // accumulator register of the wave (32 rows x 2 adjacent pieces) is then 2 runs of <= 512 contiguous bytes = 8-10 cache lines per load /
  // store instruction, not 32 lines of which 32 B each are used.  Piece of (wave, lh, j) = 8 wave + lh + 2 j.
  const int blk_jstride = 8 * ne;  // floats between a lane's pieces j and j + 1 (uniform: lands in the instruction's scalar base)
  const auto blk_off = [&](int rt) __attribute__((always_inline)) {
    return ((unsigned)eb * D + ((unsigned)(8 * wave + lh) * ne + min(lrow + 32 * rt, nem1)) * 4) * 4;
  };

  STAMP(a.stamps, 0);
  STAMP_IF(a.stamps, 6, threadIdx.x == 0 && eb >= 0);  // (diagnostic build) the tile descriptor has arrived
  STAMP_HWID(a.stamps, 14);
  STAMP_REAL(a.stamps, 12);  // 100 MHz reference clock at entry and exit: shader clock = cycles / ticks * 100 MHz
  // ---- prologue: every load is issued UNCONDITIONALLY from clamped rows and selected afterwards (a load under a per-thread
  // guard compiles to branch + load + s_waitcnt vmcnt(0): one full memory round trip per guard) -------------------------------
  // one weight slab at a time, in two halves of 4 k-steps (A: k < 64, B: k >= 64): W2 (base branch: Wf, 2 k-steps in A), later Wk
  WRegs<EX> wr;
  f16x8 fth[2], ftl[2];  // base branch: the K = 20 filter (split form in every instantiation)
  if (GUPD) {
    if (!FB) {  // (FB: requested after the basis products, whose operands and accumulators need the registers first)
      // the first half now -- it does not wait for the tile descriptor --, the second BEHIND the tile's own rows in the memory pipeline:
      // the rows still have to be split and staged before the product can start, the weights go straight to operand registers
      // (both halves first: 70.0 us per 10-batch launch; this order: 69.1; both behind the rows: 69.9)
      load_whalf<EX>(wr, a.p.W2h, wave, lane, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    load_wsplit<2>(a.p.Wfh, wave, lane, fth, ftl);
  }
  unsigned nboff[RT];  // byte offset of (neighbour atom row, this lane's first column) in an [n_atom,128] tensor
  int ctr[RT];         // tile-local centre atom of this lane's two edge rows
  float ewgt[RT] = {};
  // (a tile without edges reads word 0 of the offsets table instead -- valid, ignored -- so that no load here sits under a branch)
  const int32_t* const ecol = live ? a.edge_col : a.edge_offset;
  const int32_t* const erow = live ? a.edge_row : a.edge_offset;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const unsigned e4 = live ? (unsigned)(eb + min(lrow + 32 * rt, nem1)) * 4u : 0u;
    const int nbr = ld1i(ecol, e4), crw = ld1i(erow, e4);
    int nb = live ? nbr : 0;
    if (FB && a.species) nb = ld1i(a.species, (unsigned)nb * 4u);  // row of the per-species tables
    nboff[rt] = ((unsigned)nb * D + cbase) * 4;
    ctr[rt] = live ? crw - tile.atom_begin : 0;
    if (!GUPD) {
      const float wv = ld1f(live ? a.edge_weight : reinterpret_cast<const float*>(a.edge_offset), e4);
      ewgt[rt] = live ? wv : 0.f;
    }
  }
  const int voff = ld1i(a.edge_offset, (unsigned)(tile.atom_begin + min(tid, natom)) * 4u);
  // BLK: the tile's atoms need not be a contiguous range of the batch (the filled plan, EdgeArgs::tile_atom): slot tid of the tile's
  // tables, parked in LDS (sRow, sCen, sE0) for the query loads, the context store and the caller's edge numbers.  Addressed by the
  // tile's number: these loads, and the P1 rows' below, do not wait for the descriptor
  const unsigned slot4 = ((unsigned)tix * TQ + min(tid, TQ - 1)) * 4u;
  int trow = 0, tcen = 0, te0 = 0;
  if constexpr (BLK) {
    trow = ld1i(a.tile_atom, slot4);
    if (FB) tcen = ld1i(a.tile_cen, slot4);
    if (ATTN || MC) te0 = ld1i(a.tile_edge0, slot4);
  }
  STAMP_IF(a.stamps, 10, threadIdx.x == 0 && nboff[0] != 0xfffffff1u);  // (diagnostic build) the neighbour indices have arrived
  const float bkc = a.p.bk[tid & (D - 1)];
  const float par0 = GUPD ? (tid < D ? a.p.lng_g : a.p.lng_b)[tid & (D - 1)] : a.p.bfg[tid & (D - 1)];
  const float par1 = (tid < D ? a.p.ln_g : a.p.ln_b)[tid & (D - 1)];
  float4 greg[RT][4];
  {
    const int r = tid >> 2, sub = tid & 3;  // staging map of the base branch: 4 threads per edge row
    const int rs = r < ne ? r : nem1;
    if (GUPD) {
      float4 p1reg[3];  // centre thirds P1 = c_i W1 + bg of the tile's atoms
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int idx = tid + 256 * i, c4 = idx & 31;
        [[maybe_unused]] const int la = min(idx >> 5, natom - 1);
        int arow;
        if constexpr (BLK) arow = ld1i(a.tile_cen, ((unsigned)tix * TQ + (idx >> 5)) * 4u);  // (idx >> 5 < TQ; slots >= natom repeat the last atom)
        else arow = FB && a.species ? a.species[tile.atom_begin + la] : tile.atom_begin + la;
        p1reg[i] = ld4(a.P1, ((unsigned)arow * 32 + c4) * 16);
      }
      // geometry rows G of the tile's edges in the ACCUMULATOR layout, straight into registers: they stay there, exact fp32,
      // for the residual (attention.py:153); a tile without edges reads (and ignores) a valid row
      if (FB) {
        // geom0 rows of the tile = swish(Gauss(dist) Wd + bd) * swish(Gauss(weight) Ww + bw) (scann_model.py:378-389): basis_kernel's
        // instruction sequence on this tile's rows (a row's result does not depend on where in a tile it sits), the basis planes
        // staged in the plane buffer the geometry rows take over afterwards
        _Float16* const bH = reinterpret_cast<_Float16*>(sTile);
        _Float16* const bL = bH + TEK * BASIS_STRIDE;
        f16x8 bdh[2], bdl[2], bwh[2], bwl[2];
        load_wsplit<2>(a.basis.Wdh, wave, lane, bdh, bdl);
        load_wsplit<2>(a.basis.Wwh, wave, lane, bwh, bwl);
        {
          const float xd = ne > 0 ? a.dist[eb + rs] : 0.f, xw = ne > 0 ? a.edge_weight[eb + rs] : 0.f;
          // the 20 + 20 Gaussian centres: ONE coalesced load per wave and table, handed to the lanes by ds_bpermute (the sixteen
          // per-lane table loads of basis_kernel were a fifth of this kernel's vector-memory instructions); the same values
          const float cd_l = a.basis.cd[min(lane, NG - 1)], cw_l = a.basis.cw[min(lane, NG - 1)];
          f16x8 gh[2], gl[2];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int k = 8 * sub + i;
            const float cdk = __shfl(cd_l, k), cwk = __shfl(cw_l, k);
            const float vd = k < NG ? gauss_fast(xd, cdk) : 0.f, vw = k < NG ? gauss_fast(xw, cwk) : 0.f;
            gh[0][i] = (_Float16)vd; gl[0][i] = (_Float16)(vd - (float)gh[0][i]);
            gh[1][i] = (_Float16)vw; gl[1][i] = (_Float16)(vw - (float)gh[1][i]);
          }
          if (RT == 2 || r < TEK) {  // (32-row tiles: the upper half of the staging threads has no row)
            *reinterpret_cast<f16x8*>(bH + r * BASIS_STRIDE + 8 * sub) = gh[0];
            *reinterpret_cast<f16x8*>(bL + r * BASIS_STRIDE + 8 * sub) = gl[0];
            *reinterpret_cast<f16x8*>(bH + r * BASIS_STRIDE + 32 + 8 * sub) = gh[1];
            *reinterpret_cast<f16x8*>(bL + r * BASIS_STRIDE + 32 + 8 * sub) = gl[1];
          }
        }
        // the P1 rows (requested before the Gaussians) go to their LDS rows NOW: twelve registers less across the basis products
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int idx = tid + 256 * i;
          *reinterpret_cast<float4*>(&sQ[(idx >> 5) * LDS_STRIDE + 4 * (idx & 31)]) = p1reg[i];
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        f32x16 accd[RT], accw[RT];
        mma_split<2, true, BASIS_STRIDE, RT>(bH, bL, bdh, bdl, lane, accd);
        mma_split<2, true, BASIS_STRIDE, RT>(bH + 32, bL + 32, bwh, bwl, lane, accw);
        __builtin_amdgcn_sched_barrier(0);
        // W2 in halves, each requested once a row tile's accumulators are free (all of it at once: 28 B of scratch per lane)
        constexpr float WINV0 = 1.0f / WSCALE;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 bd = *reinterpret_cast<const float4*>(a.basis.bd + cbase + 8 * j);
            const float4 bw = *reinterpret_cast<const float4*>(a.basis.bw + cbase + 8 * j);
            const float4 sd = f4swish(make_float4(fmaf(accd[rt][4 * j], WINV0, bd.x), fmaf(accd[rt][4 * j + 1], WINV0, bd.y),
                                                  fmaf(accd[rt][4 * j + 2], WINV0, bd.z), fmaf(accd[rt][4 * j + 3], WINV0, bd.w)));
            const float4 sw = f4swish(make_float4(fmaf(accw[rt][4 * j], WINV0, bw.x), fmaf(accw[rt][4 * j + 1], WINV0, bw.y),
                                                  fmaf(accw[rt][4 * j + 2], WINV0, bw.z), fmaf(accw[rt][4 * j + 3], WINV0, bw.w)));
            greg[rt][j] = f4mul(sd, sw);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (rt == 0) load_whalf<EX>(wr, a.p.W2h, wave, lane, 0);
          if (rt == RT - 1) load_whalf<EX>(wr, a.p.W2h, wave, lane, 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every wave is done reading the basis planes: the geometry planes may overwrite them
      } else {
        const float* gsrc = ne > 0 ? a.geom : a.P1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (BLK) {
            const unsigned goff = ne > 0 ? blk_off(rt) : (unsigned)tile.atom_begin * (D * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) greg[rt][j] = ld4(gsrc + j * blk_jstride, goff);
          } else {
            const unsigned goff = ((ne > 0 ? (unsigned)(eb + min(lrow + 32 * rt, nem1)) : (unsigned)tile.atom_begin) * D + cbase) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) greg[rt][j] = ld4(gsrc, goff + 32 * j);
          }
        }
      }
      if (!FB) {
        __builtin_amdgcn_sched_barrier(0);
        load_whalf<EX>(wr, a.p.W2h, wave, lane, 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (!FB) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int idx = tid + 256 * i;
          *reinterpret_cast<float4*>(&sQ[(idx >> 5) * LDS_STRIDE + 4 * (idx & 31)]) = p1reg[i];  // rows >= natom: unused copies
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int row = lrow + 32 * rt;
#pragma unroll
        for (int j = 0; j < 4; j += 2) tile_store2<EX, TEK>(sTile, row, cbase + 8 * j, greg[rt][j], greg[rt][j + 1]);
      }
    } else {
      // base SCANN (attention.py:155): the raw distance basis gd[e][0..20) of the tile's edges, zero-padded to K = 32
      float4 gv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c4 = sub + 4 * i;  // float4 piece 0..7 of the 32-wide row; pieces 5..7 are padding
        gv[i] = ne > 0 ? ld4(a.gd, (unsigned)(eb + rs) * (NG * 4) + min(c4, 4) * 16) : ld4(a.q, (unsigned)tile.atom_begin * (D * 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c4 = sub + 4 * i;
        if (c4 > 4) gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        f16x4 h, l;
        split4(gv[i], h, l);
        if (r < TEK) {  // (32-row tiles: the upper half of the staging threads has no row)
          *reinterpret_cast<f16x4*>(sH + r * PLANE_STRIDE + 4 * c4) = h;
          *reinterpret_cast<f16x4*>(sL + r * PLANE_STRIDE + 4 * c4) = l;
        }
      }
    }
  }
  STAMP_IF(a.stamps, 11, threadIdx.x == 0 && (!GUPD || __float_as_uint(greg[RT - 1][3].w) != 0x7fc12345u));  // (diagnostic build) rows arrived, split, staged
  if (tid <= natom) sOff[tid] = part >= 0 ? (tid == 0 ? 0 : ne) : voff - eb;  // a chunk tile holds edges [0, ne) of its single atom
  if constexpr (BLK) {
    if (tid < TQ) {
      sRow[tid] = trow;
      if (FB) sCen[tid] = tcen;
      if (ATTN || MC) sE0[tid] = te0;
    }
  }
  sPar[tid] = par0;            // g_update: gamma | beta of layer_norm_g; base: filter bias (both halves)
  sPar[2 * D + tid] = par1;    // gamma | beta of layer_norm
  if (tid < D) sPar[4 * D + tid] = bkc;
  __syncthreads();
  STAMP(a.stamps, 1);

  float4 p3r[RT][4];
  f32x16 acc[RT];
  if (GUPD) {
    mma_half<EX, TEK, RT>(sTile, wr, lane, acc, 0);
    __builtin_amdgcn_sched_barrier(0);
    // gathered neighbour thirds P3[j] = c_j W3 (into the registers the first weight half leaves): in flight over the second half
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) p3r[rt][j] = ld4(a.P3, nboff[rt] + 32 * j);
    __builtin_amdgcn_sched_barrier(0);
    mma_half<EX, TEK, RT>(sTile, wr, lane, acc, 1);
  } else {
    mma_split<2, true, PLANE_STRIDE, RT>(sH, sL, fth, ftl, lane, acc);
  }
  STAMP(a.stamps, 2);
  __builtin_amdgcn_sched_barrier(0);

  constexpr float WINV = EX ? 1.0f : 1.0f / WSCALE;     // the 128x128 kernels (exact images are unscaled)
  constexpr float WINVF = 1.0f / WSCALE;                // the base branch's K = 20 filter: always the split form
  const int qa = tid >> 5;  // query rows qa, qa + 8, qa + 16 of the tile go through this thread
  const unsigned qoff = (tid & 31) * 16;
  // byte offset of the row of tile-local atom la (clamped by the caller) in an [n_atom,128] tensor / the per-species table
  const auto arow_off = [&](int la) __attribute__((always_inline)) {
    if constexpr (BLK) return qoff + (unsigned)(FB ? sCen : sRow)[la] * (D * 4);
    else return qoff + (unsigned)(FB && a.species ? a.species[tile.atom_begin + la] : tile.atom_begin + la) * (D * 4);
  };
  float4 q0, q1, q2;
  float4 cn[RT][4];
  unsigned eoff[RT];  // (edge row, first column) bytes
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) eoff[rt] = ((unsigned)(eb + min(lrow + 32 * rt, nem1)) * D + cbase) * 4;  // clamped: see `live`
  float* const gout = a.geom_out ? a.geom_out : a.geom;
  if (GUPD) {
    // geometry update (attention.py:141-153) on the accumulators: T = swish(U + P1[i] + P3[j]) + G
    float mean32[RT], m2[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const float* p1 = sQ + ctr[rt] * LDS_STRIDE + cbase;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 p1v = *reinterpret_cast<const float4*>(p1 + 8 * j);
        const float4 g = greg[rt][j];
        float4 v;
        v.x = fmaf(acc[rt][4 * j], WINV, p1v.x) + p3r[rt][j].x;
        v.y = fmaf(acc[rt][4 * j + 1], WINV, p1v.y) + p3r[rt][j].y;
        v.z = fmaf(acc[rt][4 * j + 2], WINV, p1v.z) + p3r[rt][j].z;
        v.w = fmaf(acc[rt][4 * j + 3], WINV, p1v.w) + p3r[rt][j].w;
        const float4 t = f4swish_plus(v, g);
        acc[rt][4 * j] = t.x; acc[rt][4 * j + 1] = t.y; acc[rt][4 * j + 2] = t.z; acc[rt][4 * j + 3] = t.w;
        s += f4sum(t);
        if (KEEP && a.keep_V && live) {  // training forward: the backward reads these instead of recomputing them
          // (no keep_T: the fused backward forms T again from V and G -- then T lands in V's slot and V over it, same lane, program
          // order: a select instead of a branch, which cost the 168-VGPR inference instantiation 8 bytes of scratch)
          st4(a.keep_T ? a.keep_T : a.keep_V, eoff[rt] + 32 * j, t);
          st4(a.keep_V, eoff[rt] + 32 * j, v);
        }
      }
      // LayerNorm_g statistics of the row: its 128 columns sit in 2 lanes x 4 waves.  Pairwise (Chan) combination of
      // (mean, sum of squared deviations) of the eight 16-column pieces: as accurate as the two-pass form.
      mean32[rt] = xor32(s) * (1.0f / 32.0f);
      float v2 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = acc[rt][i] - mean32[rt];
        v2 = fmaf(d, d, v2);
      }
      m2[rt] = xor32(v2);
      __builtin_amdgcn_sched_barrier(0);  // one row tile at a time: hoisting both tiles' LDS reads costs 40 VGPRs (spills)
    }
    // (statistics as [wave][row] pairs, logits below as [head][row + pad]: the 16 / 32 lanes one LDS cycle serves hold CONSECUTIVE rows,
    // and [row][8] put them 32 bytes apart -- a four-way bank conflict on this store, two-way on the reads behind the barrier, eight-way
    // on the logit stores, all of them between a barrier and the dependent arithmetic; SQ_LDS_BANK_CONFLICT: profiles/r06_notes.md)
    if (lh == 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) *reinterpret_cast<float2*>(&sE[SE_STAT(wave, lrow + 32 * rt)]) = make_float2(mean32[rt], m2[rt]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the P3 registers are free: neighbour centre rows c[j] (attention.py:136) and the key weights land over the barrier
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) cn[rt][j] = ld4(a.c, nboff[rt] + 32 * j);
    load_whalf<EX>(wr, a.p.Wkh, wave, lane, 0);  // first half of the key weights; the second half is requested at the GEMM
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // statistics complete; every wave is done with the G planes and the P1 rows
    STAMP(a.stamps, 3);
    // where this lane's geometry rows go (piece-major tiles), from a lane id read afresh (v_mbcnt): carried from the prologue, the
    // row index is one more value alive across both products in a kernel that sits at its register limit
    unsigned eoffb[RT];
    if (BLK) {
      const int lane2 = FB ? __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : lane;  // (only the fused first layer is that short)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        eoffb[rt] = ((unsigned)eb * D + ((unsigned)(8 * wave + (lane2 >> 5)) * ne + min((lane2 & 31) + 32 * rt, nem1)) * 4) * 4;
        // a tile without edges has no row of its own: its (meaningless) rows go to the spare row behind the batch's last edge, so
        // that the stores below stand in straight-line code instead of one uniform branch each
        if (!live) eoffb[rt] = ((unsigned)a.n_edge * D + cbase) * 4;
      }
    }
    // query rows of the tile's atoms: requested now, parked in sQ (the P1 rows are dead) before the key GEMM
    q0 = ld4(a.q, arow_off(min(qa, natom - 1)));
    q1 = ld4(a.q, arow_off(min(qa + 8, natom - 1)));
    q2 = ld4(a.q, arow_off(min(qa + 16, natom - 1)));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = lrow + 32 * rt;
      const float2 p0 = *reinterpret_cast<const float2*>(&sE[SE_STAT(0, row)]), p1 = *reinterpret_cast<const float2*>(&sE[SE_STAT(1, row)]);
      const float2 p2 = *reinterpret_cast<const float2*>(&sE[SE_STAT(2, row)]), p3 = *reinterpret_cast<const float2*>(&sE[SE_STAT(3, row)]);
      const float mean = ((p0.x + p1.x) + (p2.x + p3.x)) * 0.25f;
      const float d0 = p0.x - mean, d1 = p1.x - mean, d2 = p2.x - mean, d3 = p3.x - mean;
      const float var = (((p0.y + p1.y) + (p2.y + p3.y)) + 32.0f * ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3))) * (1.0f / D);
      const float rstd = ln_rstd(var), nmr = -mean * rstd;
      if (!EX && !(var < RANGE_FINITE) && live) flag_range(a.range_flag, 1, a.layer);  // an operand of the geometry update overflowed fp16
      float4 ang2[2];  // the gated rows of two neighbouring pieces go to the planes together (tile_store2)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 g = *reinterpret_cast<const float4*>(&sPar[cbase + 8 * j]);
        const float4 be = *reinterpret_cast<const float4*>(&sPar[D + cbase + 8 * j]);
        const float4 y = make_float4(ln_apply(acc[rt][4 * j], rstd, nmr, g.x, be.x), ln_apply(acc[rt][4 * j + 1], rstd, nmr, g.y, be.y),
                                     ln_apply(acc[rt][4 * j + 2], rstd, nmr, g.z, be.z), ln_apply(acc[rt][4 * j + 3], rstd, nmr, g.w, be.w));
        const float4 ang = f4mul(cn[rt][j], y);  // attention.py:157
        // threaded to the next layer (scann_model.py:415)
        if (BLK && !DEAD) st4(gout + j * blk_jstride, eoffb[rt], y);  // (a tile without edges: into the spare row, see eoffb)
        if (!BLK && !DEAD && live) st4(gout, eoff[rt] + 32 * j, y);
        if (KEEP && live && a.keep_ang) st4(a.keep_ang, eoff[rt] + 32 * j, ang);
        ang2[j & 1] = ang;
        if (j & 1) tile_store2<EX, TEK, TILE_B64_EPI>(sTile, row, cbase + 8 * (j - 1), ang2[0], ang2[1]);
      }
      __builtin_amdgcn_sched_barrier(0);  // one row tile at a time (register pressure)
    }
  } else {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) cn[rt][j] = ld4(a.c, nboff[rt] + 32 * j);
    load_whalf<EX>(wr, a.p.Wkh, wave, lane, 0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // every wave is done reading the basis planes
    STAMP(a.stamps, 3);
    // query rows of the tile's atoms: requested now, parked in sQ (the P1 rows are dead) before the key GEMM
    q0 = ld4(a.q, arow_off(min(qa, natom - 1)));
    q1 = ld4(a.q, arow_off(min(qa + 8, natom - 1)));
    q2 = ld4(a.q, arow_off(min(qa + 16, natom - 1)));
    __builtin_amdgcn_sched_barrier(0);
    // base SCANN: geomL = swish(gd Wf + bf) * weight (attention.py:155); ang = c[j] * geomL
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = lrow + 32 * rt;
      float4 ang2[2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bf = *reinterpret_cast<const float4*>(&sPar[cbase + 8 * j]);
        float4 y = f4swish(make_float4(fmaf(acc[rt][4 * j], WINVF, bf.x), fmaf(acc[rt][4 * j + 1], WINVF, bf.y),
                                       fmaf(acc[rt][4 * j + 2], WINVF, bf.z), fmaf(acc[rt][4 * j + 3], WINVF, bf.w)));
        y.x *= ewgt[rt]; y.y *= ewgt[rt]; y.z *= ewgt[rt]; y.w *= ewgt[rt];
        const float4 ang = f4mul(cn[rt][j], y);
        if (KEEP && a.keep_ang && live) {  // training forward: geomL (in the V slot) and the gated rows, kept for the backward
          st4(a.keep_V, eoff[rt] + 32 * j, y);
          st4(a.keep_ang, eoff[rt] + 32 * j, ang);
        }
        ang2[j & 1] = ang;
        if (j & 1) tile_store2<EX, TEK, TILE_B64_EPI>(sTile, row, cbase + 8 * (j - 1), ang2[0], ang2[1]);
      }
    }
  }
  // query rows: the P1 rows are dead (barrier above)
  *reinterpret_cast<float4*>(&sQ[qa * LDS_STRIDE + 4 * (tid & 31)]) = q0;
  *reinterpret_cast<float4*>(&sQ[(qa + 8) * LDS_STRIDE + 4 * (tid & 31)]) = q1;
  *reinterpret_cast<float4*>(&sQ[(qa + 16) * LDS_STRIDE + 4 * (tid & 31)]) = q2;
  __syncthreads();  // ang planes and query rows complete
  STAMP(a.stamps, 4);

  // K = ang . Wk + bk (attention.py:163); the second half of Wk arrives under the first half's MFMAs
  load_whalf<EX>(wr, a.p.Wkh, wave, lane, 1);
  __builtin_amdgcn_sched_barrier(0);
  mma_half<EX, TEK, RT>(sTile, wr, lane, acc, 0);
  mma_half<EX, TEK, RT>(sTile, wr, lane, acc, 1);
  STAMP(a.stamps, 5);
  // logits e[n, h] = (q[i, h, :] * 16^-0.5) . K[n, h, :] (attention.py:180-183) from the accumulators: this lane holds 8 of the
  // 16 columns of heads 2 wave (j = 0, 1) and 2 wave + 1 (j = 2, 3) of its rows; its partner lane (^32) holds the other 8
  float lg[RT][2];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const float* qrow = sQ + ctr[rt] * LDS_STRIDE + cbase;
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
      float e = 0.f;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * hp + jj;
        const float4 bk = *reinterpret_cast<const float4*>(&sPar[4 * D + cbase + 8 * j]);
        const float4 q4 = *reinterpret_cast<const float4*>(qrow + 8 * j);
        const float k0 = fmaf(acc[rt][4 * j], WINV, bk.x), k1 = fmaf(acc[rt][4 * j + 1], WINV, bk.y);
        const float k2 = fmaf(acc[rt][4 * j + 2], WINV, bk.z), k3 = fmaf(acc[rt][4 * j + 3], WINV, bk.w);
        acc[rt][4 * j] = k0; acc[rt][4 * j + 1] = k1; acc[rt][4 * j + 2] = k2; acc[rt][4 * j + 3] = k3;
        e = fmaf(q4.x, k0, e); e = fmaf(q4.y, k1, e); e = fmaf(q4.z, k2, e); e = fmaf(q4.w, k3, e);
      }
      // the query's 16^-0.5 (attention.py:180) on the SUM: a power of two scales every product and partial sum exactly, so
      // 0.25 (q . k) has the bits of (0.25 q) . k at a quarter ... a thirty-second of the multiplications
      lg[rt][hp] = xor32(e) * 0.25f;
    }
  }
  __syncthreads();  // every wave is done reading the ang planes: K may overwrite them
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = lrow + 32 * rt;
    // (two predicated stores, not `lh ? lg[rt][1] : lg[rt][0]`: hipcc makes a private array of lg for the select in the base kernel)
    if (lh == 0) sE[SE_LOGIT(row, 2 * wave)] = lg[rt][0];
    else sE[SE_LOGIT(row, 2 * wave + 1)] = lg[rt][1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 k4 = make_float4(acc[rt][4 * j], acc[rt][4 * j + 1], acc[rt][4 * j + 2], acc[rt][4 * j + 3]);
      *reinterpret_cast<float4*>(&sK[row * LDS_STRIDE + cbase + 8 * j]) = k4;
      if (KEEP && a.keep_K && live) st4(a.keep_K, eoff[rt] + 32 * j, k4);
    }
  }
  __syncthreads();
  STAMP(a.stamps, 8);
  // softmax over each atom's edges + context + unscaled-query residual (attention.py:186-212).
  // Packed edges are all unmasked: the additive -1e9 and the multiplicative mask are the identity; an atom without edges
  // yields q (then LayerNorm), which is what the reference's fully-masked row gives.
  {
    const int lgp = tid >> 5, c4 = tid & 31, h = c4 >> 2;
    for (int la = lgp; la < natom; la += 8) {
      const int e0 = sOff[la], e1 = sOff[la + 1];
      unsigned long long mcs = 0;  // MC: the atom's structure seed, and its first edge's structure-local index minus the tile's first edge
      size_t mce = 0;
      // the caller's number of the tile's edge n is ce + n: the attention maps and the Monte Carlo masks are keyed by it, whatever
      // order the plan puts the atoms in (a chunk tile's plan is the identity: eb is the chunk's first edge, sE0 the atom's)
      [[maybe_unused]] int ce = eb;
      if constexpr (BLK && (ATTN || MC)) ce = part >= 0 ? eb : sE0[la] - e0;
      if constexpr (MC) {
        const McRow mr = a.mc_rows[BLK ? sRow[la] : tile.atom_begin + la];
        mcs = mc_seed(a.attn_drop_seed, a.mc_t, mr.key);
        mce = (size_t)(long long)(ce - mr.e0);  // (ce + n >= mr.e0 for the atom's own edges n >= e0: the sums below do not wrap)
      }
      // row maximum first (logits only), then one exp per edge: no running-maximum rescaling in the accumulation loop
      float m = -INFINITY;
      for (int n = e0; n < e1; n += 4) {
        const float v0 = sE[SE_LOGIT(n, h)], v1 = sE[SE_LOGIT(min(n + 1, e1 - 1), h)];
        const float v2 = sE[SE_LOGIT(min(n + 2, e1 - 1), h)], v3 = sE[SE_LOGIT(min(n + 3, e1 - 1), h)];
        m = fmaxf(fmaxf(m, fmaxf(v0, v1)), fmaxf(v2, v3));
      }
      float ssum = 0.f;
      float4 cx = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int n = e0; n < e1; n += 2) {
        const bool two = n + 1 < e1;
        const int n1 = two ? n + 1 : n;
        const float4 ka = *reinterpret_cast<const float4*>(&sK[n * LDS_STRIDE + 4 * c4]);
        const float4 kb = *reinterpret_cast<const float4*>(&sK[n1 * LDS_STRIDE + 4 * c4]);
        float pa = fast_exp(sE[SE_LOGIT(n, h)] - m), pb = two ? fast_exp(sE[SE_LOGIT(n1, h)] - m) : 0.f;
        ssum += pa + pb;
        if (KEEP && a.attn_drop_p > 0.f) {  // training with use_drop: Dropout(0.05) on the attention weights (attention.py:116,191)
          pa *= drop_scale(a.attn_drop_seed, a.attn_drop_tag, (size_t)(eb + n) * NHEAD + h, a.attn_drop_p);
          pb *= drop_scale(a.attn_drop_seed, a.attn_drop_tag, (size_t)(eb + n1) * NHEAD + h, a.attn_drop_p);
        }
        if constexpr (MC) {  // Monte Carlo dropout on the attention weights, structure-local edge index
          pa *= drop_scale(mcs, a.attn_drop_tag, (mce + n) * NHEAD + h, a.attn_drop_p);
          pb *= drop_scale(mcs, a.attn_drop_tag, (mce + n1) * NHEAD + h, a.attn_drop_p);
        }
        cx.x = fmaf(pa, ka.x, fmaf(pb, kb.x, cx.x));
        cx.y = fmaf(pa, ka.y, fmaf(pb, kb.y, cx.y));
        cx.z = fmaf(pa, ka.z, fmaf(pb, kb.z, cx.z));
        cx.w = fmaf(pa, ka.w, fmaf(pb, kb.w, cx.w));
      }
      if (ATTN) {  // inference outputs: the weights of the context sum (attention.py:189), a second pass over the logits still in sE --
                   // the head's four lanes take every fourth edge: one writer per (edge, head), 4 edges x 8 heads = 128 contiguous bytes
                   // per 32 lanes.  A chunk tile knows its own chunk's maximum and sum only: exp(e - m_chunk), finished by attn_merge_kernel
        const float rn = part >= 0 ? 1.f : __builtin_amdgcn_rcpf(ssum);
        for (int n = e0 + (c4 & 3); n < e1; n += 4) a.attn_out[(size_t)(ce + n) * NHEAD + h] = fast_exp(sE[SE_LOGIT(n, h)] - m) * rn;
      }
      if (part >= 0) {  // chunk tile: leave the softmax state of this chunk for edge_merge_kernel
        float* pb = a.part_buf + (size_t)part * 3 * D + 4 * c4;
        *reinterpret_cast<float4*>(pb) = make_float4(m, m, m, m);
        *reinterpret_cast<float4*>(pb + D) = make_float4(ssum, ssum, ssum, ssum);
        *reinterpret_cast<float4*>(pb + 2 * D) = cx;
      } else {
        const float rs = e1 > e0 ? __builtin_amdgcn_rcpf(ssum) : 0.f;
        float4* qp = reinterpret_cast<float4*>(&sQ[la * LDS_STRIDE + 4 * c4]);
        const float4 q4 = *qp;
        *qp = make_float4(fmaf(cx.x, rs, q4.x), fmaf(cx.y, rs, q4.y), fmaf(cx.z, rs, q4.z), fmaf(cx.w, rs, q4.w));
      }
    }
  }
  __syncthreads();
  STAMP(a.stamps, 9);
  // LayerNorm of the context rows (attention.py:214): 8 threads per atom row
  {
    const int rr = tid >> 3, sb = tid & 7;
    if (rr < natom && part < 0) {
      float4 t[4];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        t[i] = *reinterpret_cast<const float4*>(&sQ[rr * LDS_STRIDE + 4 * (sb + 8 * i)]);
        s += f4sum(t[i]);
      }
      s = sum8(s);
      const float mean = s * (1.0f / D);
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dx = t[i].x - mean, dy = t[i].y - mean, dz = t[i].z - mean, dw = t[i].w - mean;
        v += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
      v = sum8(v);
      if (!EX && !(v < RANGE_FINITE)) flag_range(a.range_flag, 2, a.layer);  // the gated rows or the keys overflowed fp16
      const float rstd = ln_rstd(v * (1.0f / D)), nmr = -mean * rstd;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c4 = sb + 8 * i;
        const float4 g = *reinterpret_cast<const float4*>(&sPar[2 * D + 4 * c4]);
        const float4 be = *reinterpret_cast<const float4*>(&sPar[3 * D + 4 * c4]);
        const float4 y = make_float4(ln_apply(t[i].x, rstd, nmr, g.x, be.x), ln_apply(t[i].y, rstd, nmr, g.y, be.y),
                                     ln_apply(t[i].z, rstd, nmr, g.z, be.z), ln_apply(t[i].w, rstd, nmr, g.w, be.w));
        st4(a.ctx, ((unsigned)(BLK ? sRow[rr] : tile.atom_begin + rr) * 32 + c4) * 16, y);
      }
    }
  }
  STAMP(a.stamps, 7);
  STAMP_REAL(a.stamps, 13);

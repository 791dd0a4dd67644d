// The body of atom_kernel<FFN, MODE, RT, EX, KEEP, ZOUT, MC> (scann_kernels.hip) as text (a file of its own like scann_edge_body.inc; round 4's
// layer launches included both).
// Expects in scope: FFN, MODE, RT, EX, KEEP (training forward: Dropout and the keep_* stores exist), ZOUT (mode 2, inference outputs:
// after_Lc is stored), MC (Monte Carlo dropout: the Dropout layers with structure-local masks, scann_predict_mc), TAR; `a` (AtomArgs); LDS sTile [2 TAR PLANE_STRIDE halfs], sRed [TAR 8], sPar [7 D];
// SCANN_ATOM_BIX = the atom tile of this workgroup.
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane & 31, lh = lane >> 5, cbase = 32 * wave + 4 * lh;
  const int row0 = (SCANN_ATOM_BIX) * TAR;
  const int nrows = min(TAR, a.n_atom - row0);
  constexpr float WINV = EX ? 1.0f : 1.0f / WSCALE;  // (exact images are unscaled)
  // first projection after the (optional) ResidualNorm: W1 (mode 0), Wq (mode 1), after_Lc (mode 2)
  const _Float16* const firstW = MODE == 1 ? a.WCh : a.WAh;

  STAMP(a.stamps, 0);
  WRegs<EX> wr;
  load_whalf<EX>(wr, FFN ? a.Wf1h : firstW, wave, lane, 0);
  load_whalf<EX>(wr, FFN ? a.Wf1h : firstW, wave, lane, 1);
  {  // bias / LayerNorm rows -> sPar (absent ones read a valid dummy row and are never used)
    const float* const tab[7] = {FFN ? a.bf1 : a.bC, FFN ? a.bf2 : a.bC, FFN ? a.lnr_g : a.bC, FFN ? a.lnr_b : a.bC,
                                 MODE != 1 ? a.bA : a.bC, a.bC, MODE == 2 ? a.bD : a.bC};
    float pv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i] = (tid < D ? tab[2 * i] : tab[2 * i + 1 < 7 ? 2 * i + 1 : 6])[tid & (D - 1)];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (256 * i + tid < 7 * D) sPar[256 * i + tid] = pv[i];
  }
  // x rows of the tile in the accumulator layout, straight into registers (they stay there for the residual).  Ragged tail (the last
  // tile of a launch): rows past the last atom are DUPLICATES of the last real row -- loaded from the clamped row, computed like any row
  // (a row's result depends on nothing but that row), stored to the clamped row's address, i.e. the last row's own bytes onto it.
  // Nothing below is predicated per lane on `row < nrows` (edge_kernel's rule, scann_edge_body.inc).
  float4 xr[RT][4];
  unsigned ooff[RT];  // byte offset of (output row, this lane's first column) in an [n_atom,128] tensor
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int rc = row0 + min(lrow + 32 * rt, nrows - 1);
    const int src = a.x_index ? a.x_index[rc] : rc;
    ooff[rt] = ((unsigned)rc * D + cbase) * 4;
    const unsigned soff = ((unsigned)src * D + cbase) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[rt][j] = ld4(a.x, soff + 32 * j);
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = lrow + 32 * rt;
    unsigned long long mcs = 0;  // MC: this row's structure seed and the structure-local index of its first element
    size_t mce = 0;
    if constexpr (MC && !FFN) mc_row_key(a, row0 + min(row, nrows - 1), mcs, mce);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float4 v = xr[rt][j];
      if (!FFN) {
        if constexpr (MC) v = mc_drop4(mcs, a.drop_tag, mce + cbase + 8 * j, a.drop_p, v);  // Monte Carlo dropout after dense_embed
        if (KEEP && a.drop_p > 0.f) {  // training: Dropout after dense_embed (scann_model.py:374)
          const size_t e = (size_t)(row0 + min(row, nrows - 1)) * D + cbase + 8 * j;
          v.x *= drop_scale(a.drop_seed, a.drop_tag, e, a.drop_p);
          v.y *= drop_scale(a.drop_seed, a.drop_tag, e + 1, a.drop_p);
          v.z *= drop_scale(a.drop_seed, a.drop_tag, e + 2, a.drop_p);
          v.w *= drop_scale(a.drop_seed, a.drop_tag, e + 3, a.drop_p);
        }
        st4(a.c, ooff[rt] + 32 * j, v);  // centres = staged rows (layer 0 / no ResidualNorm)
      }
      xr[rt][j] = v;
      if constexpr (KEEP) tile_store<EX, TAR>(sTile, row, cbase + 8 * j, v);  // (training instantiations: round 5's stores -- at their register limit the paired form spills)
      else if (j & 1) tile_store2<EX, TAR>(sTile, row, cbase + 8 * (j - 1), xr[rt][j - 1], v);
    }
  }
  // MC with a ResidualNorm: this lane's 16 keep bits per row, hashed here -- beside the accumulators and x of the dropout site the hash's
  // 64-bit temporaries spill
  uint32_t mcm[RT] = {};
  if constexpr (MC && FFN) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      unsigned long long sd;
      size_t e;
      mc_row_key(a, row0 + min(lrow + 32 * rt, nrows - 1), sd, e);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (drop_scale(sd, a.drop_tag, e + cbase + 8 * j + k, a.drop_p) != 0.f) mcm[rt] |= 1u << (4 * j + k);
    }
  }
  __syncthreads();
  STAMP(a.stamps, 1);

  f32x16 acc[RT];
  if (FFN) {
    // ResidualNorm (attention.py:37-40): h = swish(x W1 + b1)
    gemm_tile_x<EX, true, TAR, RT>(sTile, wr, a.Wf2h, wave, lane, acc);
    STAMP(a.stamps, 2);
    __syncthreads();  // every wave is done reading the x planes
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = lrow + 32 * rt;
      float4 pair2[2];  // two neighbouring pieces go to the planes together (tile_store2)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(&sPar[cbase + 8 * j]);
        const float4 pre = make_float4(fmaf(acc[rt][4 * j], WINV, bv.x), fmaf(acc[rt][4 * j + 1], WINV, bv.y),
                                       fmaf(acc[rt][4 * j + 2], WINV, bv.z), fmaf(acc[rt][4 * j + 3], WINV, bv.w));
        const float4 hh = f4swish(pre);
        if (KEEP && a.keep_pre1) {  // training forward: kept for the backward
          st4(a.keep_pre1, ooff[rt] + 32 * j, pre);
          st4(a.keep_H1, ooff[rt] + 32 * j, hh);
        }
        if constexpr (KEEP) tile_store<EX, TAR>(sTile, row, cbase + 8 * j, hh);
        else {
          pair2[j & 1] = hh;
          if (j & 1) tile_store2<EX, TAR>(sTile, row, cbase + 8 * (j - 1), pair2[0], pair2[1]);
        }
      }
    }
    __syncthreads();
    STAMP(a.stamps, 3);
    // y = h W2 + b2 ; t = x + drop(y)
    gemm_tile_x<EX, true, TAR, RT>(sTile, wr, firstW, wave, lane, acc);
    STAMP(a.stamps, 4);
    float mean32[RT], m2[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = lrow + 32 * rt;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(&sPar[D + cbase + 8 * j]);
        float4 y = make_float4(fmaf(acc[rt][4 * j], WINV, bv.x), fmaf(acc[rt][4 * j + 1], WINV, bv.y),
                               fmaf(acc[rt][4 * j + 2], WINV, bv.z), fmaf(acc[rt][4 * j + 3], WINV, bv.w));
        if constexpr (MC) y = mc_keep4(mcm[rt] >> (4 * j), a.drop_p, y);  // Monte Carlo dropout, attention.py:29
        if (KEEP && a.drop_p > 0.f) {  // attention.py:29 (training)
          const size_t e = (size_t)(row0 + min(row, nrows - 1)) * D + cbase + 8 * j;
          y.x *= drop_scale(a.drop_seed, a.drop_tag, e, a.drop_p);
          y.y *= drop_scale(a.drop_seed, a.drop_tag, e + 1, a.drop_p);
          y.z *= drop_scale(a.drop_seed, a.drop_tag, e + 2, a.drop_p);
          y.w *= drop_scale(a.drop_seed, a.drop_tag, e + 3, a.drop_p);
        }
        const float4 t2 = f4add(xr[rt][j], y);
        acc[rt][4 * j] = t2.x; acc[rt][4 * j + 1] = t2.y; acc[rt][4 * j + 2] = t2.z; acc[rt][4 * j + 3] = t2.w;
        s += f4sum(t2);
        if (KEEP && a.keep_T2) st4(a.keep_T2, ooff[rt] + 32 * j, t2);
      }
      // LayerNorm statistics: pairwise combination of the eight 16-column pieces of the row (see edge_kernel)
      mean32[rt] = xor32(s) * (1.0f / 32.0f);
      float v2 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = acc[rt][i] - mean32[rt];
        v2 = fmaf(d, d, v2);
      }
      m2[rt] = xor32(v2);
    }
    // (the lane id is re-derived HERE, from the hardware (v_mbcnt): the address and the predicate of this store, and the row of the
    // statistics read behind the barrier, were otherwise computed at the top of the kernel and carried -- at the register limit,
    // spilled -- across both products)
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    {
      const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (and the wave index as a scalar, for the same reason)
      if ((ln >> 5) == 0) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) *reinterpret_cast<float2*>(&sRed[SR_STAT(wv, (ln & 31) + 32 * rt)]) = make_float2(mean32[rt], m2[rt]);
      }
    }
    __syncthreads();  // statistics complete; every wave is done reading the hidden planes
    STAMP(a.stamps, 5);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = (ln & 31) + 32 * rt;
      // ([wave][row] pairs: the lanes one LDS cycle serves hold consecutive rows -- see edge_kernel's sE)
      const float2 p0 = *reinterpret_cast<const float2*>(&sRed[SR_STAT(0, row)]), p1 = *reinterpret_cast<const float2*>(&sRed[SR_STAT(1, row)]);
      const float2 p2 = *reinterpret_cast<const float2*>(&sRed[SR_STAT(2, row)]), p3 = *reinterpret_cast<const float2*>(&sRed[SR_STAT(3, row)]);
      const float mean = ((p0.x + p1.x) + (p2.x + p3.x)) * 0.25f;
      const float d0 = p0.x - mean, d1 = p1.x - mean, d2 = p2.x - mean, d3 = p3.x - mean;
      const float var = (((p0.y + p1.y) + (p2.y + p3.y)) + 32.0f * ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3))) * (1.0f / D);
      const float rstd = ln_rstd(var), nmr = -mean * rstd;
      if (!EX && !(var < RANGE_FINITE)) flag_range(a.range_flag, 3, a.layer - 1);  // an operand of the ResidualNorm overflowed fp16
      float4 pair2[2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 g = *reinterpret_cast<const float4*>(&sPar[2 * D + cbase + 8 * j]);
        const float4 be = *reinterpret_cast<const float4*>(&sPar[3 * D + cbase + 8 * j]);
        const float4 y = make_float4(ln_apply(acc[rt][4 * j], rstd, nmr, g.x, be.x), ln_apply(acc[rt][4 * j + 1], rstd, nmr, g.y, be.y),
                                     ln_apply(acc[rt][4 * j + 2], rstd, nmr, g.z, be.z), ln_apply(acc[rt][4 * j + 3], rstd, nmr, g.w, be.w));
        st4(a.c, ooff[rt] + 32 * j, y);
        if constexpr (KEEP) tile_store<EX, TAR>(sTile, row, cbase + 8 * j, y);
        else {
          pair2[j & 1] = y;
          if (j & 1) tile_store2<EX, TAR>(sTile, row, cbase + 8 * (j - 1), pair2[0], pair2[1]);
        }
      }
    }
    __syncthreads();
    STAMP(a.stamps, 6);
  }

  if (MODE == 0) {  // P1 = c W1 + bg ; P3 = c W3 ; q = c Wq + bq (attention.py:142-151 thirds, :160)
    gemm_tile_x<EX, true, TAR, RT>(sTile, wr, a.WBh, wave, lane, acc);
    STAMP(a.stamps, 7);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bg = *reinterpret_cast<const float4*>(&sPar[4 * D + cbase + 8 * j]);
        st4(a.oA, ooff[rt] + 32 * j, make_float4(fmaf(acc[rt][4 * j], WINV, bg.x), fmaf(acc[rt][4 * j + 1], WINV, bg.y),
                                                   fmaf(acc[rt][4 * j + 2], WINV, bg.z), fmaf(acc[rt][4 * j + 3], WINV, bg.w)));
      }
    gemm_tile_x<EX, true, TAR, RT>(sTile, wr, a.WCh, wave, lane, acc);
    STAMP(a.stamps, 9);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        st4(a.oB, ooff[rt] + 32 * j, make_float4(acc[rt][4 * j] * WINV, acc[rt][4 * j + 1] * WINV, acc[rt][4 * j + 2] * WINV, acc[rt][4 * j + 3] * WINV));
  }
  if (MODE == 0 || MODE == 1) {  // q = c Wq + bq (attention.py:160)
    STAMP(a.stamps, 10);
    gemm_tile_x<EX, false, TAR, RT>(sTile, wr, nullptr, wave, lane, acc);
    STAMP(a.stamps, 11);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bq = *reinterpret_cast<const float4*>(&sPar[5 * D + cbase + 8 * j]);
        st4(a.oC, ooff[rt] + 32 * j, make_float4(fmaf(acc[rt][4 * j], WINV, bq.x), fmaf(acc[rt][4 * j + 1], WINV, bq.y),
                                                   fmaf(acc[rt][4 * j + 2], WINV, bq.z), fmaf(acc[rt][4 * j + 3], WINV, bq.w)));
      }
    STAMP(a.stamps, 12);
  }
  if (MODE == 2) {  // z = swish(c Wa + ba) (scann_model.py:424); gq = z Wgq + b ; gk = z Wgk + b (attention.py:269-272)
    gemm_tile_x<EX, true, TAR, RT>(sTile, wr, a.WCh, wave, lane, acc);
    __syncthreads();  // every wave is done reading the centre planes
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = lrow + 32 * rt;
      float4 pair2[2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(&sPar[4 * D + cbase + 8 * j]);
        const float4 pre = make_float4(fmaf(acc[rt][4 * j], WINV, bv.x), fmaf(acc[rt][4 * j + 1], WINV, bv.y),
                                       fmaf(acc[rt][4 * j + 2], WINV, bv.z), fmaf(acc[rt][4 * j + 3], WINV, bv.w));
        const float4 z = f4swish(pre);
        // no LayerNorm follows this activation: test it directly (its hi part feeds the GlobalAttention projections)
        if (!EX && !(fmaxf(fmaxf(fabsf(z.x), fabsf(z.y)), fmaxf(fabsf(z.z), fabsf(z.w))) < 65504.f)) flag_range(a.range_flag, 4, a.layer);
        if (KEEP && a.keep_preA) {  // training forward: after_Lc pre-activation and output, kept for the backward
          st4(a.keep_preA, ooff[rt] + 32 * j, pre);
          st4(a.keep_z, ooff[rt] + 32 * j, z);
        }
        if constexpr (ZOUT) st4(a.out_z, ooff[rt] + 32 * j, z);  // inference outputs: after_Lc, stored the way keep_z is
        if constexpr (KEEP) tile_store<EX, TAR>(sTile, row, cbase + 8 * j, z);
        else {
          pair2[j & 1] = z;
          if (j & 1) tile_store2<EX, TAR>(sTile, row, cbase + 8 * (j - 1), pair2[0], pair2[1]);
        }
      }
    }
    __syncthreads();
    gemm_tile_x<EX, true, TAR, RT>(sTile, wr, a.WDh, wave, lane, acc);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bq = *reinterpret_cast<const float4*>(&sPar[5 * D + cbase + 8 * j]);
        st4(a.oC, ooff[rt] + 32 * j, make_float4(fmaf(acc[rt][4 * j], WINV, bq.x), fmaf(acc[rt][4 * j + 1], WINV, bq.y),
                                                   fmaf(acc[rt][4 * j + 2], WINV, bq.z), fmaf(acc[rt][4 * j + 3], WINV, bq.w)));
      }
    gemm_tile_x<EX, false, TAR, RT>(sTile, wr, nullptr, wave, lane, acc);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bk = *reinterpret_cast<const float4*>(&sPar[6 * D + cbase + 8 * j]);
        st4(a.oB, ooff[rt] + 32 * j, make_float4(fmaf(acc[rt][4 * j], WINV, bk.x), fmaf(acc[rt][4 * j + 1], WINV, bk.y),
                                                   fmaf(acc[rt][4 * j + 2], WINV, bk.z), fmaf(acc[rt][4 * j + 3], WINV, bk.w)));
      }
  }

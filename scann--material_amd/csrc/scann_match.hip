// Nearest structures of a latent-space index by matching local structures (scann_index_match, include/scann_hip.h): a query structure
// and an index segment are compared as sets of after_Lc rows.  With D[i][j] the dist2 chain of scann_knn.hip,
//   f_i = min_j D[i][j],  g_j = min_i D[i][j]   (a NaN never counts; +inf if nothing does)
//   F = (fp64 sum of f_i, i ascending) / n,  G = (fp64 sum of g_j, j ascending) / m,  Fmax = max f_i,  Gmax = max g_j
// and the score is (float)(F + G), max(Fmax, Gmax) or (float) F.  The k best segments are the first k under (score, segment number).
//
// match_tile_kernel: the tile and the slab pipeline of scann_tile.h, difference form.  A workgroup's query rows are whole structures
// (the host plans the tiles), its index rows a range that begins and ends on segment boundaries (the host plans the ranges from the
// segment table), each row read from its own storage chunk.
// When a tile's 128 x 64 distances are complete they go to LDS and three short passes reduce them:
//   g pass  lane (row r, wave w) takes the structures w, w + 4, ... and the min of D[.][r] over each one's atoms        -> gbuf[r][s]
//   f pass  lane i < 128 walks its query atom's 64 distances in position order with the running f_i of the current segment (a
//           register that lives across tiles) and, where a segment ends, leaves f_i in the tile in place of D[i][r]
//   s pass  lane s < 32 walks its structure's g values in position order, adding them in fp64; where a segment ends it adds the f_i in
//           atom order, forms the score and brings its sorted list of the k best, [place][structure] in LDS, up to date
// Where segments end in a tile is one 64-bit ballot per wave (a row whose successor carries another id), tested with scalar instructions;
// the f and s passes read eight rows ahead of their walk, so that their LDS reads do not wait for one another.
// min and max are exact, so their order is free; the two fp64 sums have the one order of the definition.  No atomics, no dependence on
// the tiling or the ranges: knn_merge_kernel merges the ranges' lists under (score, segment).  The distance block never leaves LDS.
//
// match_pair_kernel: for the k winning segments of every structure the distances are formed once more, one workgroup per pair, and
// reduced to the four parts and to every query atom's witness (the least position that attains f_i) -- k pairs per structure, a
// vanishing share of the work.
#include "scann_match.h"

#include <algorithm>

namespace scann {

namespace {

constexpr int MT = TILE_LANES;  // lanes of match_tile_kernel
constexpr int MP = 128;    // lanes of match_pair_kernel: one per query atom
constexpr int MP_TR = 32;  // segment rows per step of match_pair_kernel
constexpr int MP_LD = MP + 1;

__device__ __forceinline__ float match_score(int measure, double F, double G, float Fmax, float Gmax) {
  return measure == 0 ? (float)(F + G) : measure == 1 ? (Fmax > Gmax ? Fmax : Gmax) : (float)F;
}

__global__ __launch_bounds__(MT) void match_tile_kernel(MatchArgs a) {
  extern __shared__ float4 match_smem[];
  float* sm = reinterpret_cast<float*>(match_smem);
  float* qs = sm;                                  // the query slab ...
  float* rs = sm + tile_slab_floats(TILE_TQ);      // ... and the row slab (tile_stage)
  float* tile = sm;                                // [64][MT_LD]  distances of the tile, over the slabs
  float* gbuf = sm + MT_UNION;                     // [64][SL + 1] g of (row, structure)
  const int SL = a.sets_ld, GLD = SL + 1;          // structures the per-structure arrays have room for (16 or 32: the host's choice)
  float* ld = gbuf + TILE_TR * GLD;                  // [k][SL]      per structure: the k least scores so far, ascending ...
  int32_t* lp = reinterpret_cast<int32_t*>(ld + a.k * SL);          // ... and their segments
  int32_t* qoff = lp + a.k * SL;                   // [SL + 1] first atom of every structure of the tile, relative to the tile's first
  long long* idt = reinterpret_cast<long long*>(qoff + SL + 2);     // [65] ids of the tile's rows and of the one behind them
  const int t = threadIdx.x, qg = t & 15, rg = t >> 4;
  const int set_begin = a.tiles[2 * blockIdx.y], n_set = a.tiles[2 * blockIdx.y + 1] - set_begin;
  const int q0 = a.q_first[set_begin], n_q = a.q_first[set_begin + n_set] - q0;
  const int r_begin = a.ranges[3 * blockIdx.x], r_end = a.ranges[3 * blockIdx.x + 1];
  int seg = a.ranges[3 * blockIdx.x + 2];  // (lanes of the s pass: the segment their walk is in)
  const int k = a.k, stride = a.stride, chunk_rows = a.chunk_rows;
  if (t <= n_set) qoff[t] = a.q_first[set_begin + t] - q0;
  const bool owner = t < n_set;  // lane t keeps the list of structure set_begin + t
  const bool has_qid = a.qid != nullptr;
  const long long my_id = owner && has_qid ? a.qid[set_begin + t] : 0;
  int cnt = 0;
  float f_run = __builtin_inff();                 // f pass: f_i of the current segment so far
  double g_sum = 0.0;                             // s pass: the fp64 sum of g_j, j ascending, ...
  float g_max = -__builtin_inff();                // ... their max ...
  int m_run = 0;                                  // ... and the rows of the current segment so far
  const int n_slab = (stride + TILE_SLAB - 1) / TILE_SLAB;
  const int n_step = ((r_end - r_begin + TILE_TR - 1) / TILE_TR) * n_slab;
  float4 gq[4], gr[2];
  auto fetch = [&](int step) {
    const int tile0 = r_begin + (step / n_slab) * TILE_TR, c0 = (step % n_slab) * TILE_SLAB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + MT * i, item = e >> 3, col = c0 + 4 * (e & 7);
      gq[i] = item < n_q && col < stride ? *reinterpret_cast<const float4*>(a.q + (size_t)(q0 + item) * stride + col) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = t + MT * i, pos = tile0 + (e >> 3), col = c0 + 4 * (e & 7);
      gr[i] = float4{0.f, 0.f, 0.f, 0.f};
      // every row from its own chunk: a range may lie across a chunk boundary
      if (pos < r_end && col < stride) gr[i] = *reinterpret_cast<const float4*>(tile_row(a.rows, pos, chunk_rows, stride) + col);
    }
  };
  f2 acc[8][2];
  tile_clear(acc);
  if (n_step > 0) fetch(0);
  for (int step = 0; step < n_step; ++step) {
    const int tile0 = r_begin + (step / n_slab) * TILE_TR;
    __syncthreads();  // the previous slab's reads, or the previous tile's passes, are over
    tile_stage<MT, 4, TILE_TQ>(qs, gq, t);
    tile_stage<MT, 2, TILE_TR>(rs, gr, t);
    __syncthreads();
    if (step + 1 < n_step) fetch(step + 1);
    tile_slab<TileForm::DIFF>(qs, rs, qg, rg, acc, TILE_SLAB);
    if (step % n_slab != n_slab - 1) continue;
    // the tile's last slab: its 128 x 64 distances go to LDS
    __syncthreads();  // every lane has read its last slab
    tile_write<MT_LD>(tile, acc, qg, rg);
    tile_clear(acc);
    const int n = min(TILE_TR, r_end - tile0);
    if (t <= n) {  // the ids of the tile's rows and of the row behind them: a row ends its segment if it is the range's last or the next id is another
      const int pos = tile0 + t;
      idt[t] = pos < r_end ? *tile_row(a.ids, pos, chunk_rows, 1) : 0;
    }
    __syncthreads();
    // bit r: row r ends its segment (the same 64 bits in every wave)
    const int lane = t & (TILE_TR - 1);
    const unsigned long long ends = __ballot(lane < n && (tile0 + lane + 1 == r_end || idt[lane] != idt[lane + 1]));
    {  // g pass
      const int r = lane;
      if (r < n)
        for (int s = t >> 6; s < n_set; s += MT / TILE_TR) {
          float g = __builtin_inff();
          for (int i = qoff[s]; i < qoff[s + 1]; ++i) {
            const float d = tile[r * MT_LD + i];
            if (d < g) g = d;  // a NaN never counts
          }
          gbuf[r * GLD + s] = g;
        }
    }
    __syncthreads();
    if (t < n_q)  // f pass (eight rows are read ahead of the walk: the store at a segment's end would hold the later reads back)
      for (int r0 = 0; r0 < n; r0 += 8) {
        float d8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) d8[u] = tile[(r0 + u) * MT_LD + t];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u;
          if (r >= n) break;
          if (d8[u] < f_run) f_run = d8[u];
          if ((ends >> r) & 1) {
            tile[r * MT_LD + t] = f_run;
            f_run = __builtin_inff();
          }
        }
      }
    __syncthreads();
    if (owner)  // s pass
      for (int r0 = 0; r0 < n; r0 += 8) {
        float g8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) g8[u] = gbuf[(r0 + u) * GLD + t];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u;
          if (r >= n) break;
          const float g = g8[u];
          g_sum += (double)g;
          if (g > g_max) g_max = g;
          ++m_run;
          if (!((ends >> r) & 1)) continue;
          double f_sum = 0.0;
          float f_max = -__builtin_inff();
          for (int i = qoff[t]; i < qoff[t + 1]; ++i) {
            const float f = tile[r * MT_LD + i];
            f_sum += (double)f;
            if (f > f_max) f_max = f;
          }
          const float d = match_score(a.measure, f_sum / (double)(qoff[t + 1] - qoff[t]), g_sum / (double)m_run, f_max, g_max);
          const int sg = seg++;
          g_sum = 0.0; g_max = -__builtin_inff(); m_run = 0;
          if (has_qid && idt[r] == my_id) continue;
          if (cnt == k && !(d < ld[(k - 1) * SL + t])) continue;  // segments ascending: among equal scores the earlier is in the list
          int j = cnt < k ? cnt : k - 1;
          for (; j > 0 && ld[(j - 1) * SL + t] > d; --j) {
            ld[j * SL + t] = ld[(j - 1) * SL + t];
            lp[j * SL + t] = lp[(j - 1) * SL + t];
          }
          ld[j * SL + t] = d;
          lp[j * SL + t] = sg;
          if (cnt < k) ++cnt;
        }
      }
  }
  if (owner) {
    const size_t o = ((size_t)(set_begin - a.set_base + t) * a.n_range + blockIdx.x) * k;
    for (int j = 0; j < k; ++j) {
      a.part_d[o + j] = j < cnt ? ld[j * SL + t] : __builtin_inff();
      a.part_p[o + j] = j < cnt ? lp[j * SL + t] : -1;
    }
  }
}

__global__ __launch_bounds__(MP) void match_pair_kernel(MatchPairArgs a) {
  __shared__ float db[MP_TR * MP_LD];  // [32][129] distances of this step: D[i][j] at [j][i]
  __shared__ float gl[MP_TR];          // g of the step's rows
  __shared__ float fs[MP];             // f of the query atoms
  const int t = threadIdx.x;
  const int pair = blockIdx.x, set = pair / a.k, place = pair - set * a.k;
  const int first = a.seg_first[pair], m = a.seg_count[pair];
  if (m <= 0) return;  // no segment at this place: the host has written the tail
  const int q0 = a.q_first[set], n = a.q_first[set + 1] - q0;
  const int stride = a.stride, chunk_rows = a.chunk_rows;
  const bool active = t < n;
  const float* __restrict__ qrow = a.q + (size_t)(q0 + (active ? t : 0)) * stride;
  float f = __builtin_inff();
  int w = -1;
  double g_sum = 0.0;
  float g_max = -__builtin_inff();
  for (int j0 = 0; j0 < m; j0 += MP_TR) {
    const int nj = min(MP_TR, m - j0);
    if (active)
      for (int jj = 0; jj < nj; ++jj) {
        const int pos = first + j0 + jj;
        const float* __restrict__ row = tile_row(a.rows, pos, chunk_rows, stride);
        float acc = 0.f;
        for (int c = 0; c < stride; c += 4) {  // the chain of the definition, columns ascending (the padding adds fmaf(0, 0, acc) = acc)
          const float4 x = *reinterpret_cast<const float4*>(qrow + c), y = *reinterpret_cast<const float4*>(row + c);
          float d = x.x - y.x;
          acc = __builtin_fmaf(d, d, acc);
          d = x.y - y.y;
          acc = __builtin_fmaf(d, d, acc);
          d = x.z - y.z;
          acc = __builtin_fmaf(d, d, acc);
          d = x.w - y.w;
          acc = __builtin_fmaf(d, d, acc);
        }
        db[jj * MP_LD + t] = acc;
        if (acc == acc && (w < 0 || acc < f)) f = acc, w = pos;  // positions ascending: the least position that attains f
      }
    __syncthreads();
    if (t < nj) {
      float g = __builtin_inff();
      for (int i = 0; i < n; ++i) {
        const float d = db[t * MP_LD + i];
        if (d < g) g = d;
      }
      gl[t] = g;
    }
    __syncthreads();
    if (t == 0)
      for (int jj = 0; jj < nj; ++jj) {
        g_sum += (double)gl[jj];
        if (gl[jj] > g_max) g_max = gl[jj];
      }
  }
  if (active) {
    fs[t] = f;
    a.match_pos[(size_t)(q0 + t) * a.k + place] = w;
    a.match_d[(size_t)(q0 + t) * a.k + place] = f;
  }
  __syncthreads();
  if (t == 0) {
    double f_sum = 0.0;
    float f_max = -__builtin_inff();
    for (int i = 0; i < n; ++i) {
      f_sum += (double)fs[i];
      if (fs[i] > f_max) f_max = fs[i];
    }
    float* o = a.parts + (size_t)pair * 4;
    o[0] = (float)(f_sum / (double)n);
    o[1] = (float)(g_sum / (double)m);
    o[2] = f_max;
    o[3] = g_max;
  }
}

}  // namespace

size_t match_lds_bytes(int k, int sets_ld) {
  return (size_t)MT_UNION * 4 + (size_t)TILE_TR * (sets_ld + 1) * 4 + (size_t)k * sets_ld * 8 + (sets_ld + 2) * 4 + (TILE_TR + 1) * 8;
}

hipError_t launch_match_tile(const MatchArgs& a, hipStream_t s) {
  if (a.n_tile <= 0 || a.n_range <= 0) return hipSuccess;
  const size_t lds = match_lds_bytes(a.k, a.sets_ld);
  if (lds > 48 * 1024) {  // above the default dynamic-LDS allowance a kernel has to be told
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(match_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(match_tile_kernel, dim3((unsigned)a.n_range, (unsigned)a.n_tile), dim3(MT), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_match_pair(const MatchPairArgs& a, hipStream_t s) {
  if (a.n_sets <= 0) return hipSuccess;
  hipLaunchKernelGGL(match_pair_kernel, dim3((unsigned)((size_t)a.n_sets * a.k)), dim3(MP), 0, s, a);
  return hipGetLastError();
}

}  // namespace scann

// Handle of libscann_hip.so's C ABI (include/scann_hip.h): device-block cache, weight container and its device images, creation,
// destruction and the handle's queries.  Host side only -- all arithmetic is in the .hip files.
#include "scann_runtime.h"

#include <mutex>

namespace {

// Per-device cache of freed device blocks: resident batches, their keep/debug buffers and training workspaces are
// allocated per batch, and pipelines (predict_dataset, the training loop) create and drop one per step -- reusing a
// block of similar size avoids a hipMalloc/hipFree pair (hundreds of microseconds, and an implicit device sync) each time.
struct BlockCache {
  std::multimap<size_t, void*> free_blocks;
  std::map<void*, size_t> size_of;
  size_t cached_bytes = 0;
};
std::map<int, BlockCache> g_block_cache;
std::mutex g_block_mu;
constexpr size_t BLOCK_CACHE_LIMIT = (size_t)16 << 30;  // per device
thread_local std::string g_create_error;

// Canonical tensor list; mirrors create_model (scann_model.py:329-453) and the layer constructors
// (attention.py:25-35, 95-113, 260-262).  Must stay in step with oracle/scann_oracle.py:weight_shapes.
std::vector<WeightSpec> build_specs(const scann_config_t& c) {
  std::vector<WeightSpec> s;
  const int64_t d = c.local_dim, dg = c.global_dim, dout = c.dense_out, emb = c.embedding_dim;
  if (c.feature_cgcnn) {
    s.push_back({"embed_atom/kernel", 92, emb});
    s.push_back({"embed_atom/bias", emb, 0});
  } else {
    s.push_back({"embed_atom/embeddings", c.n_atoms, emb});
  }
  int64_t cin = emb;
  if (c.use_ring) {
    s.push_back({"extra_embed/kernel", 2, 10});
    s.push_back({"extra_embed/bias", 10, 0});
    cin += 10;
  }
  s.push_back({"dense_embed/kernel", cin, d});
  s.push_back({"dense_embed/bias", d, 0});
  if (c.g_update) {
    s.push_back({"neighbor_d/kernel", c.n_gauss, d});
    s.push_back({"neighbor_d/bias", d, 0});
    s.push_back({"neighbor_w/kernel", c.n_gauss, d});
    s.push_back({"neighbor_w/bias", d, 0});
  }
  for (int i = 0; i < c.n_attention; ++i) {
    const std::string p = "local_attention_" + std::to_string(i) + "/";
    s.push_back({p + "query/kernel", d, d});
    s.push_back({p + "query/bias", d, 0});
    s.push_back({p + "key/kernel", d, d});
    s.push_back({p + "key/bias", d, 0});
    s.push_back({p + "filter_geo/kernel", c.g_update ? 3 * d : (int64_t)c.n_gauss, d});
    s.push_back({p + "filter_geo/bias", d, 0});
    s.push_back({p + "layer_norm/gamma", d, 0});
    s.push_back({p + "layer_norm/beta", d, 0});
    if (c.g_update) {
      s.push_back({p + "layer_norm_g/gamma", d, 0});
      s.push_back({p + "layer_norm_g/beta", d, 0});
    }
    if (c.use_attn_norm) {
      const std::string r = "residual_norm_" + std::to_string(i) + "/";
      s.push_back({r + "dense_1/kernel", d, d});
      s.push_back({r + "dense_1/bias", d, 0});
      s.push_back({r + "dense_2/kernel", d, d});
      s.push_back({r + "dense_2/bias", d, 0});
      s.push_back({r + "layer_norm/gamma", d, 0});
      s.push_back({r + "layer_norm/beta", d, 0});
    }
  }
  s.push_back({"after_Lc/kernel", d, dg});
  s.push_back({"after_Lc/bias", dg, 0});
  s.push_back({"global_attention/query/kernel", dg, dg});
  s.push_back({"global_attention/query/bias", dg, 0});
  s.push_back({"global_attention/key/kernel", dg, dg});
  s.push_back({"global_attention/key/bias", dg, 0});
  s.push_back({"bf_property/kernel", dg, dout});
  s.push_back({"bf_property/bias", dout, 0});
  s.push_back({"predict_property/kernel", dout, 1});
  s.push_back({"predict_property/bias", 1, 0});
  return s;
}

// np.linspace(0, stop, 20, dtype="float32") (scann_model.py:378,384): computed in double, cast once.
void linspace20(double stop, float* out) {
  const double step = stop / (NG - 1);
  for (int i = 0; i < NG; ++i) out[i] = (float)(i * step);
  out[NG - 1] = (float)stop;
}

}  // namespace

namespace scann {

hipError_t cached_malloc(void** p, size_t bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t gran = bytes >= ((size_t)1 << 20) ? ((size_t)1 << 20) : ((size_t)64 << 10);
  const size_t want = (std::max<size_t>(bytes, 1) + gran - 1) / gran * gran;
  {
    std::lock_guard<std::mutex> lk(g_block_mu);
    BlockCache& c = g_block_cache[dev];
    auto it = c.free_blocks.lower_bound(want);
    if (it != c.free_blocks.end() && it->first <= 2 * want) {
      *p = it->second;
      c.cached_bytes -= it->first;
      c.free_blocks.erase(it);
      return hipSuccess;
    }
  }
  const hipError_t e = hipMalloc(p, want);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_block_mu);
    g_block_cache[dev].size_of[*p] = want;
  }
  return e;
}

// The caller guarantees no kernel still uses the block (scann_batch_free synchronises first).
void cached_free(void* p) {
  if (!p) return;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(g_block_mu);
  BlockCache& c = g_block_cache[dev];
  auto it = c.size_of.find(p);
  if (it == c.size_of.end()) {
    (void)hipFree(p);
    return;
  }
  if (c.cached_bytes + it->second > BLOCK_CACHE_LIMIT) {
    c.size_of.erase(it);
    (void)hipFree(p);
    return;
  }
  c.free_blocks.emplace(it->second, p);
  c.cached_bytes += it->second;
}

void cache_release(int dev) {  // at handle destruction: give the idle blocks of this device back
  std::lock_guard<std::mutex> lk(g_block_mu);
  BlockCache& c = g_block_cache[dev];
  for (auto& kv : c.free_blocks) {
    c.size_of.erase(kv.second);
    (void)hipFree(kv.second);
  }
  c.free_blocks.clear();
  c.cached_bytes = 0;
}

int fail(scann_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  else g_create_error = msg;
  return code;
}

// After a synchronisation: did a kernel of the finished work trip the range guard (flag_range)?  The word is cleared, so the handle
// stays usable once the caller has dealt with the cause.
// One word per stream slot: with two launch groups in flight, the download of the group on stream A must not consume (and clear) a
// report raised by the kernels of the group on stream B.
int check_range(scann_handle* h, const char* where, int slot) {
  if (!h->range_flag) return SCANN_OK;
  const int32_t code = *reinterpret_cast<volatile int32_t*>(h->range_flag + slot);
  if (!code) return SCANN_OK;
  h->range_flag[slot] = 0;
  const int site = code >> 8, layer = (code & 0xff) - 1;
  static const char* const names[] = {"?", "layer_norm_g statistics (geometry update)", "layer_norm statistics (attention context)",
                                      "ResidualNorm statistics", "after_Lc activation", "a weight after the optimiser step"};
  std::string m = std::string(where) + ": value outside the range of the split-fp16 projections (|activation| < 65504, |weight| < 255.9): " +
                  (site >= 1 && site <= 5 ? names[site] : names[0]);
  if (site != 5) m += layer >= h->cfg.n_attention ? ", readout" : ", local_attention_" + std::to_string(layer);
  m += "; the results of this call are not valid";
  return fail(h, SCANN_ERR_RANGE, m);
}

// Fragment order consumed by gemm128 (scann_kernels.hip): element ((w*16 + t)*64 + lane)*4 + i holds
// W[8t + 4(lane>>5) + i][32w + (lane&31)].
void pack_weight(const float* W, int ld, float* Wp) {
  for (int w = 0; w < 4; ++w)
    for (int t = 0; t < 16; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i)
          Wp[((size_t)(w * 16 + t) * 64 + lane) * 4 + i] = W[(size_t)(8 * t + 4 * (lane >> 5) + i) * ld + 32 * w + (lane & 31)];
}

// fp32 -> fp16 bits, round to nearest even, subnormals kept (host twin of the device's v_cvt_f16_f32)
static uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7FFFFFFFu;
  if (x >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (x > 0x7F800000u ? 0x200u : 0));  // inf / nan
  if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                                    // rounds to >= 65520: inf
  if (x < 0x33000001u) return (uint16_t)sign;                                                  // <= 2^-25: zero
  const int e = (int)(x >> 23) - 127;
  uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
  int shift = 13;
  uint32_t base;
  if (e < -14) {  // subnormal result
    shift += -14 - e;
    base = 0;
  } else {
    base = (uint32_t)(e + 15) << 10;
    m &= 0x7FFFFFu;
  }
  const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
  uint32_t r = base + q;  // a mantissa carry runs into the exponent field, which is the right result
  if (rem > halfway || (rem == halfway && (q & 1))) ++r;
  return (uint16_t)(sign | r);
}
static float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31, m = h & 0x3FFu;
  float out;
  if (e == 0) {
    out = std::ldexp((float)m, -24);
  } else if (e == 31) {
    uint32_t x = 0x7F800000u | (m << 13);
    memcpy(&out, &x, 4);
  } else {
    out = std::ldexp((float)(m | 0x400u), (int)e - 25);
  }
  uint32_t x;
  memcpy(&x, &out, 4);
  x |= sign;
  memcpy(&out, &x, 4);
  return out;
}
void pack_weight_f16(const float* W, int ld, int k_real, int ks, uint16_t* out) {
  for (int w = 0; w < 4; ++w)
    for (int s = 0; s < ks; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * s + 8 * (lane >> 5) + j;
          const float x = k < k_real ? WSCALE * W[(size_t)k * ld + 32 * w + (lane & 31)] : 0.f;
          const uint16_t hi = f32_to_f16_bits(x);
          const uint16_t lo = f32_to_f16_bits(x - f16_bits_to_f32(hi));
          const size_t base = ((size_t)(w * ks + s) * 2) * 64 * 8 + (size_t)lane * 8 + j;
          out[base] = hi;
          out[base + 64 * 8] = lo;
        }
}

// The low end of the split-fp16 range.  A pair hi + lo holds 22 significant bits only while lo is a normal fp16 number; below that it
// has an absolute quantum (rounding error <= 2^-25), so an operand row whose LARGEST element is m carries a relative error of about
// 2^-25 / m, and so does a column of a kernel (times 2^8) whose largest element is m.  Below m = SMALL_OPERAND = 2^-8 that is more than
// 2^-17 = 7.6e-6 per operand -- a decade above fp32's own 2^-24 and within a factor 13 of the 1e-4 the forward promises, which two
// attention layers and the readout easily spend -- and the checkpoint runs on the exact-fp32 kernels instead, like one with |w| >= 255.9.
// What the projections will see is known at load time, operand by operand:
//   the columns of the seven kernels per layer and the three of the readout;
//   the rows a LayerNorm hands on (centres and geometry from the second layer on, every context): x = gamma n + beta with n of zero mean
//     and unit variance, component c of size sqrt(gamma_c^2 + beta_c^2);
//   the first layer's centres, swish(dense_embed(embedding)): one row per table entry, computed here (first_centres);
//   the first layer's geometry, swish(neighbor_d(.)) * swish(neighbor_w(.)): a K = 20 filter is a function of ONE scalar, so each
//     component's largest value over the distances / angles is computed here (filter_size) -- a row can only be smaller;
//   the key projection's operand, which is a PRODUCT, component by component: centres x the layer's new geometry (base branch: x the
//     filtered Gaussians, times a neighbour weight that is 1 for an atom's widest neighbour) -- two factors of 2^-6 are a row of 2^-12;
//   the two swish rows behind a Dense layer of a LayerNorm output -- the ResidualNorm's hidden row and after_Lc's output, z = x . W + b,
//     of root mean square sqrt(sum_k gamma_k^2 W_kj^2 + (sum_k beta_k W_kj + b_j)^2) in column j, and swish(z) ~ z / 2 where it matters.
// A row's size is the largest of its components' sizes.  Not classified: cgcnn features enter the first centres as an upper bound only
// (features in [0, 1]: a row that is certainly small is found, another may not be); rows that are small for the DATA's sake under
// ordinary weights (a structure whose after_Lc or ResidualNorm hidden rows happen to be tiny); and a checkpoint that becomes small
// under training -- the rule runs in scann_load_weights, not after an optimiser step (site 5 of flag_range watches |w| >= 255.9 only).  Exact zeros are representable and never count: a kernel column or a LayerNorm that is zero
// throughout is skipped, and a row's largest element decides, not its smallest.  Returns the cause, naming the tensor, or "".
// (tests/split_ref.py restates the rule in NumPy: the suite's emulation of the scheme shows what it lets through.)
constexpr double SMALL_OPERAND = 1.0 / 256.0;
static std::string small_operand_reason(const scann_config_t& c, std::map<std::string, const float*>& src) {
  const int L = c.n_attention;
  auto col_small = [&](const std::string& name, int row0) {
    const float* W = src[name] + (size_t)row0 * D;
    double least = INFINITY;
    for (int j = 0; j < D; ++j) {
      double m = 0.0;
      for (int k = 0; k < D; ++k) m = std::max(m, (double)std::fabs(W[(size_t)k * D + j]));
      if (m > 0.0) least = std::min(least, m);
    }
    return least * (double)WSCALE < SMALL_OPERAND;
  };
  typedef std::vector<double> Row;  // one size per component
  auto top = [](const Row& r) { return *std::max_element(r.begin(), r.end()); };
  auto small = [&](const Row& r) { return top(r) > 0.0 && top(r) < SMALL_OPERAND; };
  auto swish = [](double z) { return z / (1.0 + std::exp(-z)); };
  auto ln_size = [&](const std::string& prefix) {  // the rows a LayerNorm hands on: sqrt(gamma_c^2 + beta_c^2)
    const float *g = src[prefix + "/gamma"], *b = src[prefix + "/beta"];
    Row r(D);
    for (int k = 0; k < D; ++k) r[k] = std::sqrt((double)g[k] * g[k] + (double)b[k] * b[k]);
    return r;
  };
  auto ln_small = [&](const std::string& prefix) { return small(ln_size(prefix)); };
  // a K = 20 filter is a function of one scalar: the largest |swish(gaussians(x) . W + b)| of each component over x = 0 .. top in 64 steps
  auto filter_size = [&](const std::string& prefix, double x_top) {
    const float *W = src[prefix + "/kernel"], *b = src[prefix + "/bias"];
    Row r(D, 0.0);
    for (int i = 0; i <= 64; ++i) {
      double g[NG];
      for (int k = 0; k < NG; ++k) {
        const double d = i * (x_top / 64.0) - k * (x_top / (NG - 1));
        g[k] = std::exp(-d * d / 0.25);
      }
      for (int j = 0; j < D; ++j) {
        double z = b[j];
        for (int k = 0; k < NG; ++k) z += g[k] * W[(size_t)k * D + j];
        r[j] = std::max(r[j], std::fabs(swish(z)));
      }
    }
    return r;
  };
  // The first layer's centres, swish(dense_embed(.)): no LayerNorm precedes them, but the loaded tensors fix them.  Exact for the atomic
  // embedding -- one row per table row from 1 on (row 0 is the padding index), with use_ring times the four ring-feature combinations;
  // for cgcnn features an upper bound of every row, taking the features in [0, 1]: only rows that are CERTAINLY small are classified.
  // Returns the size of each component (largest over the rows); *least = the smallest of the rows' largest elements that is not 0.
  auto first_centres = [&](double* least) {
    const int E = c.embedding_dim, cin = E + (c.use_ring ? 10 : 0);
    const float *We = src["dense_embed/kernel"], *be = src["dense_embed/bias"];
    std::vector<Row> in;
    const bool bound = c.feature_cgcnn != 0;
    if (bound) {
      Row e(cin, 0.0);
      const float *Wc = src["embed_atom/kernel"], *bc = src["embed_atom/bias"];
      for (int k = 0; k < E; ++k) {
        e[k] = std::fabs(bc[k]);
        for (int f = 0; f < 92; ++f) e[k] += std::fabs(Wc[(size_t)f * E + k]);
      }
      if (c.use_ring)
        for (int k = 0; k < 10; ++k) e[E + k] = std::fabs(src["extra_embed/bias"][k]) + std::fabs(src["extra_embed/kernel"][k]) + std::fabs(src["extra_embed/kernel"][10 + k]);
      in.push_back(e);
    } else {
      const float* T = src["embed_atom/embeddings"];
      for (int s = 1; s < c.n_atoms; ++s)
        for (int rc = 0; rc < (c.use_ring ? 4 : 1); ++rc) {
          Row e(cin);
          for (int k = 0; k < E; ++k) e[k] = T[(size_t)s * E + k];
          if (c.use_ring)
            for (int k = 0; k < 10; ++k) e[E + k] = (rc >> 1) * (double)src["extra_embed/kernel"][k] + (rc & 1) * (double)src["extra_embed/kernel"][10 + k] + src["extra_embed/bias"][k];
          in.push_back(e);
        }
    }
    Row size(D, 0.0);
    *least = INFINITY;
    for (const Row& e : in) {
      double m = 0.0;
      for (int j = 0; j < D; ++j) {
        double z = bound ? std::fabs(be[j]) : be[j];
        for (int k = 0; k < cin; ++k) z += e[k] * (bound ? std::fabs(We[(size_t)k * D + j]) : We[(size_t)k * D + j]);
        const double v = bound ? z : std::fabs(swish(z));  // |swish(z)| <= |z|
        size[j] = std::max(size[j], v);
        m = std::max(m, v);
      }
      if (m > 0.0) *least = std::min(*least, m);
    }
    return size;
  };
  auto swish_small = [&](const std::string& ln, const std::string& dense) {
    const float *g = src[ln + "/gamma"], *b = src[ln + "/beta"], *W = src[dense + "/kernel"], *bias = src[dense + "/bias"];
    double r = 0.0;
    for (int j = 0; j < D; ++j) {
      double var = 0.0, mean = bias[j];
      for (int k = 0; k < D; ++k) {
        const double w = W[(size_t)k * D + j];
        var += (double)g[k] * g[k] * w * w;
        mean += (double)b[k] * w;
      }
      r = std::max(r, std::sqrt(var + mean * mean));
    }
    return r > 0.0 && 0.5 * r < SMALL_OPERAND;
  };
  const std::string column = ": a column of the kernel is below 2^-16 throughout (its split-fp16 image keeps too few bits)";
  const std::string few = " stay below 2^-8, where a split-fp16 operand keeps too few bits";
  double least = 0.0;
  Row cen = first_centres(&least);
  if (least < SMALL_OPERAND) return "dense_embed: its swish output rows (the first layer's centres)" + few;
  if (c.g_update && L > 0) {
    Row g = filter_size("neighbor_d", (double)c.gaussian_d);
    const Row gw = filter_size("neighbor_w", 2.0 * M_PI);
    for (int k = 0; k < D; ++k) g[k] *= gw[k];
    if (small(g)) return "neighbor_d, neighbor_w: the products of their swish outputs (the first layer's geometry)" + few;
  }
  for (int i = 0; i < L; ++i) {
    const std::string p = "local_attention_" + std::to_string(i) + "/", r = "residual_norm_" + std::to_string(i) + "/";
    {  // the key projection's operand is a PRODUCT, component by component: centres x this layer's new geometry (base branch: x the filtered
       // Gaussians at their largest over the distances, times a neighbour weight that is 1 for an atom's widest neighbour)
      Row ang = c.g_update ? ln_size(p + "layer_norm_g") : filter_size(p + "filter_geo", (double)c.gaussian_d);
      for (int k = 0; k < D; ++k) ang[k] *= cen[k];
      if (small(ang)) return p + "key: its operand rows (centres x geometry, component by component)" + few;
      cen = ln_size((c.use_attn_norm ? r : p) + "layer_norm");
    }
    std::vector<std::string> names = {p + "query/kernel", p + "key/kernel"};
    if (c.use_attn_norm) names.insert(names.end(), {r + "dense_1/kernel", r + "dense_2/kernel"});
    for (const std::string& n : names)
      if (col_small(n, 0)) return n + column;
    if (c.g_update) {
      for (int j = 0; j < 3; ++j)
        if (col_small(p + "filter_geo/kernel", j * D)) return p + "filter_geo/kernel, rows " + std::to_string(j * D) + ".." + std::to_string(j * D + D - 1) + column;
      if (ln_small(p + "layer_norm_g")) return p + "layer_norm_g: its output rows (the geometry) stay below 2^-8, where a split-fp16 operand keeps too few bits";
    }
    if (ln_small(p + "layer_norm")) return p + "layer_norm: its output rows (the context) stay below 2^-8, where a split-fp16 operand keeps too few bits";
    if (c.use_attn_norm) {
      if (ln_small(r + "layer_norm")) return r + "layer_norm: its output rows (the centres) stay below 2^-8, where a split-fp16 operand keeps too few bits";
      if (swish_small(p + "layer_norm", r + "dense_1"))
        return r + "dense_1: its swish output rows (the operand of dense_2) stay below 2^-8, where a split-fp16 operand keeps too few bits";
    }
  }
  for (const char* n : {"after_Lc/kernel", "global_attention/query/kernel", "global_attention/key/kernel"})
    if (col_small(n, 0)) return n + column;
  if (L > 0 && swish_small((c.use_attn_norm ? "residual_norm_" : "local_attention_") + std::to_string(L - 1) + "/layer_norm", "after_Lc"))
    return "after_Lc: its swish output rows (the operand of global_attention/query and key) stay below 2^-8, where a split-fp16 operand keeps too few bits";
  return "";
}

}  // namespace scann

extern "C" {

int scann_abi_version(void) { return SCANN_ABI_VERSION; }

int scann_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* scann_last_error(const scann_handle_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int scann_create(const scann_config_t* cfg, int device_id, scann_handle_t** out) {
  if (!cfg || !out) return fail(nullptr, SCANN_ERR_INVALID, "scann_create: null argument");
  *out = nullptr;
  if (cfg->n_gauss != NG) return fail(nullptr, SCANN_ERR_UNSUPPORTED, "scann_create: 20 Gaussians (custom_layers.py:39-53 as called by scann_model.py:378,384)");
  // every shipped reference config is 128 / 8 / 128 / 128: the MFMA kernels; any other widths the reference accepts
  // (scann_model.py:330-434): the plain-fp32 forward of scann_generic.hip, inference only
  const bool generic = cfg->local_dim != D || cfg->global_dim != D || cfg->dense_out != D || cfg->num_head != NHEAD ||
                       (getenv("SCANN_GENERIC") && atoi(getenv("SCANN_GENERIC")));
  if (generic) {
    if (cfg->local_dim <= 0 || cfg->num_head <= 0 || cfg->global_dim <= 0 || cfg->dense_out <= 0 || cfg->local_dim % cfg->num_head != 0)
      return fail(nullptr, SCANN_ERR_INVALID, "scann_create: local_dim must be a positive multiple of num_head (attention.py:170-173), global_dim and dense_out positive");
    if (cfg->local_dim > 1024 || cfg->global_dim > 1024 || cfg->dense_out > 1024 || cfg->embedding_dim > 1024)
      return fail(nullptr, SCANN_ERR_UNSUPPORTED, "scann_create: widths above 1024 are not implemented");
  } else if (cfg->embedding_dim + (cfg->use_ring ? 10 : 0) > 160) {
    return fail(nullptr, SCANN_ERR_UNSUPPORTED, "scann_create: embedding_dim (+10 ring features) must be <= 160");
  }
  if (cfg->n_atoms <= 0 || cfg->embedding_dim <= 0 || cfg->n_attention < 0 || !(cfg->gaussian_d > 0))
    return fail(nullptr, SCANN_ERR_INVALID, "scann_create: bad hyper-parameter");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, SCANN_ERR_NO_DEVICE, "scann_create: no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, SCANN_ERR_NO_DEVICE, "scann_create: device_id out of range");
  scann_handle* h = new scann_handle();
  h->cfg = *cfg;
  h->generic = generic;
  h->device = device_id;
  h->specs = build_specs(*cfg);
  if (const char* xr = getenv("SCANN_XCD_REMAP")) h->xcd_remap = atoi(xr) != 0;
  if (const char* ar = getenv("SCANN_ATOM_ROWS")) h->atom_rows = atoi(ar);
  if (const char* fb = getenv("SCANN_FUSE_BASIS")) h->fuse_basis = atoi(fb) != 0;
  if (const char* tf = getenv("SCANN_TILE_FILL")) h->tile_fill = atoi(tf) != 0;
  if (const char* st = getenv("SCANN_SPECIES_TABLES")) h->species_tables = atoi(st) != 0;
  if (const char* sg = getenv("SCANN_STRICT_RANGE")) h->strict_range = atoi(sg) != 0;
  if (const char* fe = getenv("SCANN_EXACT")) h->force_exact = atoi(fe) != 0;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) h->n_cu = prop.multiProcessorCount;
  }
  if (const char* ns = getenv("SCANN_STREAMS")) h->nstream = std::min(MAX_STREAM, std::max(1, atoi(ns)));
  if (hipSetDevice(device_id) != hipSuccess) {
    delete h;
    return fail(nullptr, SCANN_ERR_HIP, "scann_create: hipSetDevice failed");
  }
  if (hipHostMalloc((void**)&h->range_flag, 128, hipHostMallocDefault) != hipSuccess) {  // [0, 16): range guard per stream
    delete h;
    return fail(nullptr, SCANN_ERR_HIP, "scann_create: hipHostMalloc failed");
  }
  for (int i = 0; i < 32; ++i) h->range_flag[i] = 0;  // one range-guard word per stream slot
  for (int i = 0; i < h->nstream; ++i) {
    if (hipStreamCreateWithFlags(&h->streams[i], hipStreamNonBlocking) != hipSuccess) {
      delete h;
      return fail(nullptr, SCANN_ERR_HIP, "scann_create: hipStreamCreate failed");
    }
  }
  *out = h;
  return SCANN_OK;
}

void scann_destroy(scann_handle_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < MAX_STREAM; ++i)
    if (h->streams[i]) (void)hipStreamDestroy(h->streams[i]);
  if (h->d_weights) (void)hipFree(h->d_weights);
  for (scann_handle::DlStage& st : h->dl_stage)
    if (st.p) (void)hipHostFree(st.p);
  if (h->g_weights) (void)hipFree(h->g_weights);
  if (h->g_centres) (void)hipFree(h->g_centres);
  if (h->g_WT) (void)hipFree(h->g_WT);
  if (h->d_gt_descs) (void)hipFree(h->d_gt_descs);
  if (h->sp_c) (void)hipFree(h->sp_c);
  for (scann_handle::Stage& st : h->stage) {
    if (st.p) (void)hipHostFree(st.p);
    if (st.ev) (void)hipEventDestroy(st.ev);
  }
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  for (void* q : {(void*)h->t_master, (void*)h->t_grad, (void*)h->t_m, (void*)h->t_v, (void*)h->t_l2, (void*)h->t_lrs, (void*)h->t_descs, (void*)h->ig_grad})
    if (q) (void)hipFree(q);
  if (h->comm) ncclCommDestroy(h->comm);
  if (h->train_aux && !h->train_aux_borrowed) (void)hipStreamDestroy(h->train_aux);
  if (h->h_stat) (void)hipHostFree(h->h_stat);
  if (h->range_flag) (void)hipHostFree(h->range_flag);
  for (float* t : h->h_targets)
    if (t) (void)hipHostFree(t);
  for (hipEvent_t e : h->step_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->train_aux2) (void)hipStreamDestroy(h->train_aux2);
  for (hipEvent_t e : h->train_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->time_ev) (void)hipEventDestroy(e);
  free_models(h->models);
  if (h->sc_db) free_batch(h->sc_db);  // (its arena is the handle's scratch, freed below)
  if (h->sc_arena) (void)hipFree(h->sc_arena);
  if (h->pp_dev) (void)hipFree(h->pp_dev);
  if (h->pp_host) (void)hipHostFree(h->pp_host);
  if (h->sc_host) (void)hipHostFree(h->sc_host);
  cache_release(h->device);
  delete h;
}

int scann_num_streams(const scann_handle_t* h) { return h ? h->nstream : 0; }

int scann_weight_count(const scann_handle_t* h) { return h ? (int)h->specs.size() : SCANN_ERR_INVALID; }

int scann_weight_name(const scann_handle_t* h, int index, const char** name, int64_t* rows, int64_t* cols) {
  if (!h || index < 0 || index >= (int)h->specs.size()) return SCANN_ERR_INVALID;
  if (name) *name = h->specs[index].name.c_str();
  if (rows) *rows = h->specs[index].rows;
  if (cols) *cols = h->specs[index].cols;
  return SCANN_OK;
}

int64_t scann_param_count(const scann_handle_t* h) {
  if (!h) return SCANN_ERR_INVALID;
  int64_t n = 0;
  for (const WeightSpec& s : h->specs) n += s.numel();
  return n;
}

int scann_load_weights(scann_handle_t* h, const float* blob, const scann_tensor_desc_t* manifest, int n) {
  return scann::load_weights(h, blob, manifest, n, nullptr, nullptr);
}

}  // extern "C"

namespace scann {

int load_weights(scann_handle* h, const float* blob, const scann_tensor_desc_t* manifest, int n, float* at, size_t* need) {
  if (!h || !blob || !manifest || n <= 0) return fail(h, SCANN_ERR_INVALID, "scann_load_weights: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  std::map<std::string, const scann_tensor_desc_t*> by_name;
  for (int i = 0; i < n; ++i)
    if (manifest[i].name) by_name[manifest[i].name] = &manifest[i];
  // canonical flat parameter vector: the tensors in spec order
  std::map<std::string, const float*> src;
  {
    size_t total = 0;
    for (const WeightSpec& s : h->specs) {
      auto it = by_name.find(s.name);
      if (it == by_name.end()) return fail(h, SCANN_ERR_WEIGHTS, "scann_load_weights: missing tensor " + s.name);
      if (it->second->numel != s.numel() || it->second->offset < 0)
        return fail(h, SCANN_ERR_WEIGHTS, "scann_load_weights: wrong size for tensor " + s.name);
      total += (size_t)s.numel();
    }
    h->host_master.resize(total);
    h->spec_off.clear();
    size_t off = 0;
    for (const WeightSpec& s : h->specs) {
      memcpy(h->host_master.data() + off, blob + by_name[s.name]->offset, (size_t)s.numel() * sizeof(float));
      src[s.name] = h->host_master.data() + off;
      h->spec_off.push_back((int64_t)off);
      off += (size_t)s.numel();
    }
  }
  if (h->generic) {  // the plain-fp32 forward reads the Keras tensors as they are
    for (float v : h->host_master)
      if (!std::isfinite(v)) return fail(h, SCANN_ERR_WEIGHTS, "scann_load_weights: a parameter is not finite");
    if (h->g_weights) (void)hipFree(h->g_weights);
    h->g_weights = nullptr;
    HIPCHK(h, hipMalloc((void**)&h->g_weights, h->host_master.size() * sizeof(float)));
    HIPCHK(h, hipMemcpy(h->g_weights, h->host_master.data(), h->host_master.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!h->g_centres) {
      float cen[2 * NG];
      linspace20((double)h->cfg.gaussian_d, cen);
      linspace20(M_PI * 2.0, cen + NG);
      HIPCHK(h, hipMalloc((void**)&h->g_centres, sizeof(cen)));
      HIPCHK(h, hipMemcpy(h->g_centres, cen, sizeof(cen), hipMemcpyHostToDevice));
    }
    h->g_off.clear();
    for (size_t i = 0; i < h->specs.size(); ++i) h->g_off[h->specs[i].name] = h->spec_off[i];
    h->loaded = true;
    return SCANN_OK;
  }
  h->descs.clear();
  const float* const mbase = h->host_master.data();
  const float* const mend = mbase + h->host_master.size();
  const scann_config_t& c = h->cfg;
  const int L = c.n_attention;
  // host image of the device arena
  std::vector<float> img;
  img.reserve((size_t)(L * 8 + 8) * WPACK);
  auto put_raw = [&](const float* p, size_t numel) {
    const size_t off = img.size();
    img.insert(img.end(), p, p + numel);
    while (img.size() % 64) img.push_back(0.f);  // keep every tensor 256-byte aligned
    if (p >= mbase && p < mend)                  // derived from a parameter: re-copied after every optimiser step
      for (size_t done = 0; done < numel; done += 16384)
        h->descs.push_back(RepackDesc{(int64_t)(p - mbase + done), (int64_t)(off + done), 0, (int32_t)std::min<size_t>(16384, numel - done)});
    return off;
  };
  auto put_packed = [&](const float* W) {  // W: row-major [128,128] slice, leading dim 128
    const size_t off = img.size();
    img.resize(off + WPACK);
    pack_weight(W, D, img.data() + off);
    h->descs.push_back(RepackDesc{(int64_t)(W - mbase), (int64_t)off, 0, 0});
    return off;
  };
  auto put_packedT = [&](const float* W) {  // fragment-order image of W^T (backward: dX = dY . W^T)
    const size_t off = img.size();
    img.resize(off + WPACK);
    std::vector<float> wt((size_t)D * D);
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) wt[(size_t)j * D + i] = W[(size_t)i * D + j];
    pack_weight(wt.data(), D, img.data() + off);
    h->descs.push_back(RepackDesc{(int64_t)(W - mbase), (int64_t)off, 1, 0});
    return off;
  };
  auto put_f16 = [&](const float* W, int k_real, int ks) {  // split-fp16 image (edge_kernel); ks * 2048 floats' worth of bytes
    const size_t off = img.size();
    img.resize(off + (size_t)ks * 2048);
    pack_weight_f16(W, D, k_real, ks, reinterpret_cast<uint16_t*>(img.data() + off));
    h->descs.push_back(RepackDesc{(int64_t)(W - mbase), (int64_t)off, 0, ks == 8 ? -1 : -2});
    return off;
  };
  auto put_f16T = [&](const float* W) {  // split-fp16 image of W^T ([128,128]; fused backward kernels: dX = dY . W^T)
    const size_t off = img.size();
    img.resize(off + (size_t)8 * 2048);
    std::vector<float> wt((size_t)D * D);
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) wt[(size_t)j * D + i] = W[(size_t)i * D + j];
    pack_weight_f16(wt.data(), D, D, 8, reinterpret_cast<uint16_t*>(img.data() + off));
    h->descs.push_back(RepackDesc{(int64_t)(W - mbase), (int64_t)off, 1, -1});
    return off;
  };
  // The fp16 hi part of a split weight holds |w| * 2^8 < 65504.  A 128x128 kernel beyond that (the reference loads any fp32
  // checkpoint, scann_model.py:79) sends every inference forward of the handle to the exact-fp32 kernels; the K = 20 filters exist
  // in the split form only, and nothing can be done with a value that is not finite.
  h->weights_exact = false;
  for (const WeightSpec& sp : h->specs)
    if (sp.cols) {
      const float* wp = src[sp.name];
      const bool split_only = sp.name == "neighbor_d/kernel" || sp.name == "neighbor_w/kernel" ||
                              (!c.g_update && sp.name.size() > 17 && sp.name.compare(sp.name.size() - 17, 17, "filter_geo/kernel") == 0);
      const bool projection = sp.rows == D * (sp.name.find("filter_geo") != std::string::npos ? 3 : 1) && sp.cols == D &&
                              sp.name != "bf_property/kernel" && sp.name != "dense_embed/kernel";
      for (int64_t i = 0; i < sp.numel(); ++i)
        if (!(std::fabs(wp[i]) < WMAX)) {
          if (std::isfinite(wp[i]) && projection && !split_only) {
            h->weights_exact = true;
            break;
          }
          if (!std::isfinite(wp[i]) || split_only)
            return fail(h, SCANN_ERR_UNSUPPORTED, "scann_load_weights: |" + sp.name + "| reaches " + std::to_string(std::fabs(wp[i])) +
                                                      (split_only ? "; this kernel is multiplied in split-fp16 form only, which needs |w| < 255.9"
                                                                  : "; the value is not finite"));
          break;  // an fp32-only tensor (embedding, dense_embed, bf_property, head): any finite value
        }
    }
  h->small_operands = false;
  h->exact_reason = h->weights_exact ? "a 128x128 kernel has |w| >= 255.9" : "";
  if (!h->weights_exact) {
    const std::string why = small_operand_reason(c, src);
    if (!why.empty()) {
      h->weights_exact = h->small_operands = true;
      h->exact_reason = why;
    }
  }
  struct LTOff { size_t W1T, W2T, W3T, WqT, WkT, Wf1T, Wf2T, W1Th, W2Th, W3Th, WqTh, WkTh, Wf1Th, Wf2Th; };
  std::vector<LTOff> lto(L);
  struct LOff {
    size_t bg, bq, bk, lng_g, lng_b, ln_g, ln_b, Wfg, bfg, bf1, bf2, lnr_g, lnr_b;
    size_t W2h, Wkh, Wfh, W1h, W3h, Wqh, Wf1h, Wf2h;
    size_t W1p, W2p, W3p, Wqp, Wkp, Wf1p, Wf2p;  // fp32 fragment-order images: the exact-fp32 fallback of the forward
  };
  std::vector<LOff> lo(L);
  const size_t NONE = (size_t)-1;
  for (int i = 0; i < L; ++i) {
    const std::string p = "local_attention_" + std::to_string(i) + "/";
    LOff& o = lo[i];
    o = LOff{NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE,
             NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE};
    const float* fg = src[p + "filter_geo/kernel"];
    lto[i] = LTOff{NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE};
    if (c.g_update) {  // concat order [centre, geometry, neighbour] (attention.py:143-149)
      o.W1h = put_f16(fg, D, 8);
      o.W3h = put_f16(fg + (size_t)2 * D * D, D, 8);
      o.W2h = put_f16(fg + (size_t)D * D, D, 8);
      o.W1p = put_packed(fg);
      o.W2p = put_packed(fg + (size_t)D * D);
      o.W3p = put_packed(fg + (size_t)2 * D * D);
      lto[i].W1T = put_packedT(fg);
      lto[i].W2T = put_packedT(fg + (size_t)D * D);
      lto[i].W3T = put_packedT(fg + (size_t)2 * D * D);
      lto[i].W1Th = put_f16T(fg);
      lto[i].W2Th = put_f16T(fg + (size_t)D * D);
      lto[i].W3Th = put_f16T(fg + (size_t)2 * D * D);
      o.bg = put_raw(src[p + "filter_geo/bias"], D);
      o.lng_g = put_raw(src[p + "layer_norm_g/gamma"], D);
      o.lng_b = put_raw(src[p + "layer_norm_g/beta"], D);
    } else {
      o.Wfg = put_raw(fg, (size_t)NG * D);
      o.Wfh = put_f16(fg, NG, 2);
      o.bfg = put_raw(src[p + "filter_geo/bias"], D);
    }
    o.Wqh = put_f16(src[p + "query/kernel"], D, 8);
    o.Wqp = put_packed(src[p + "query/kernel"]);
    o.Wkp = put_packed(src[p + "key/kernel"]);
    lto[i].WqT = put_packedT(src[p + "query/kernel"]);
    lto[i].WkT = put_packedT(src[p + "key/kernel"]);
    lto[i].WqTh = put_f16T(src[p + "query/kernel"]);
    lto[i].WkTh = put_f16T(src[p + "key/kernel"]);
    o.bq = put_raw(src[p + "query/bias"], D);
    o.Wkh = put_f16(src[p + "key/kernel"], D, 8);
    o.bk = put_raw(src[p + "key/bias"], D);
    o.ln_g = put_raw(src[p + "layer_norm/gamma"], D);
    o.ln_b = put_raw(src[p + "layer_norm/beta"], D);
    if (c.use_attn_norm) {
      const std::string r = "residual_norm_" + std::to_string(i) + "/";
      lto[i].Wf1T = put_packedT(src[r + "dense_1/kernel"]);
      lto[i].Wf2T = put_packedT(src[r + "dense_2/kernel"]);
      lto[i].Wf1Th = put_f16T(src[r + "dense_1/kernel"]);
      lto[i].Wf2Th = put_f16T(src[r + "dense_2/kernel"]);
      o.Wf1h = put_f16(src[r + "dense_1/kernel"], D, 8);
      o.Wf2h = put_f16(src[r + "dense_2/kernel"], D, 8);
      o.Wf1p = put_packed(src[r + "dense_1/kernel"]);
      o.Wf2p = put_packed(src[r + "dense_2/kernel"]);
      o.bf1 = put_raw(src[r + "dense_1/bias"], D);
      o.bf2 = put_raw(src[r + "dense_2/bias"], D);
      o.lnr_g = put_raw(src[r + "layer_norm/gamma"], D);
      o.lnr_b = put_raw(src[r + "layer_norm/beta"], D);
    }
  }
  const size_t oWaTh = put_f16T(src["after_Lc/kernel"]);
  const size_t oWaT = put_packedT(src["after_Lc/kernel"]), oWgqT = put_packedT(src["global_attention/query/kernel"]),
               oWgkT = put_packedT(src["global_attention/key/kernel"]);
  const size_t oWah = put_f16(src["after_Lc/kernel"], D, 8), oWgqh = put_f16(src["global_attention/query/kernel"], D, 8),
               oWgkh = put_f16(src["global_attention/key/kernel"], D, 8);
  const size_t oWa = put_packed(src["after_Lc/kernel"]), oba = put_raw(src["after_Lc/bias"], D);
  const size_t oWgq = put_packed(src["global_attention/query/kernel"]), obgq = put_raw(src["global_attention/query/bias"], D);
  const size_t oWgk = put_packed(src["global_attention/key/kernel"]), obgk = put_raw(src["global_attention/key/bias"], D);
  const size_t oWb = put_raw(src["bf_property/kernel"], (size_t)D * D), obb = put_raw(src["bf_property/bias"], D);
  const size_t owo = put_raw(src["predict_property/kernel"], D), obo = put_raw(src["predict_property/bias"], 1);
  size_t oWd = NONE, obd = NONE, oWw = NONE, obw = NONE, oWdh = NONE, oWwh = NONE;
  if (c.g_update) {
    oWdh = put_f16(src["neighbor_d/kernel"], NG, 2);
    oWwh = put_f16(src["neighbor_w/kernel"], NG, 2);
    oWd = put_raw(src["neighbor_d/kernel"], (size_t)NG * D);
    obd = put_raw(src["neighbor_d/bias"], D);
    oWw = put_raw(src["neighbor_w/kernel"], (size_t)NG * D);
    obw = put_raw(src["neighbor_w/bias"], D);
  }
  float cen[2 * NG];
  linspace20((double)c.gaussian_d, cen);
  linspace20(M_PI * 2.0, cen + NG);
  const size_t ocd = put_raw(cen, NG), ocw = put_raw(cen + NG, NG);
  const bool general_embed = c.use_ring || c.feature_cgcnn;
  const int64_t cin = c.embedding_dim + (c.use_ring ? 10 : 0);
  size_t oemb = NONE, oWc = NONE, obc = NONE, oWr = NONE, obr = NONE;
  if (c.feature_cgcnn) {
    oWc = put_raw(src["embed_atom/kernel"], (size_t)92 * c.embedding_dim);
    obc = put_raw(src["embed_atom/bias"], c.embedding_dim);
  } else {
    oemb = put_raw(src["embed_atom/embeddings"], (size_t)c.n_atoms * c.embedding_dim);
  }
  if (c.use_ring) {
    oWr = put_raw(src["extra_embed/kernel"], 20);
    obr = put_raw(src["extra_embed/bias"], 10);
  }
  const size_t oWe = put_raw(src["dense_embed/kernel"], (size_t)cin * D);
  const size_t obe = put_raw(src["dense_embed/bias"], D);
  const size_t olut = img.size();
  img.resize(olut + (size_t)c.n_atoms * D, 0.f);
  // per-species tables of the first layer (c | P1 | P3 | q) behind the arena when it is placed (a model set's block)
  const size_t sp_tab = (!general_embed && c.g_update) ? (size_t)c.n_atoms * D : 0, o_sp = (img.size() + 63) & ~(size_t)63;
  if (need) {  // validated: the floats the arena and the tables take at a placement
    *need = o_sp + 4 * sp_tab;
    return SCANN_OK;
  }
  if (at) {
    h->d_weights = at;
    if (sp_tab) {
      h->sp_c = at + o_sp;
      h->sp_P1 = h->sp_c + sp_tab; h->sp_P3 = h->sp_c + 2 * sp_tab; h->sp_q = h->sp_c + 3 * sp_tab;
    }
  } else if (h->d_weights) {
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipFree(h->d_weights));
    h->d_weights = nullptr;
    h->loaded = false;
  }
  if (!at) HIPCHK(h, hipMalloc((void**)&h->d_weights, img.size() * sizeof(float)));
  HIPCHK(h, hipMemcpy(h->d_weights, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  const float* base = h->d_weights;
  auto P = [&](size_t off) -> const float* { return off == NONE ? nullptr : base + off; };
  h->layers.assign(L, LayerParams{});
  for (int i = 0; i < L; ++i) {
    const LOff& o = lo[i];
    LayerParams& lp = h->layers[i];
    lp.bg = P(o.bg); lp.bq = P(o.bq); lp.bk = P(o.bk);
    lp.lng_g = P(o.lng_g); lp.lng_b = P(o.lng_b); lp.ln_g = P(o.ln_g); lp.ln_b = P(o.ln_b);
    lp.Wfg = P(o.Wfg); lp.bfg = P(o.bfg);
    lp.W2h = reinterpret_cast<const _Float16*>(P(o.W2h)); lp.Wkh = reinterpret_cast<const _Float16*>(P(o.Wkh));
    lp.Wfh = reinterpret_cast<const _Float16*>(P(o.Wfh));
    lp.W1h = reinterpret_cast<const _Float16*>(P(o.W1h)); lp.W3h = reinterpret_cast<const _Float16*>(P(o.W3h));
    lp.Wqh = reinterpret_cast<const _Float16*>(P(o.Wqh)); lp.Wf1h = reinterpret_cast<const _Float16*>(P(o.Wf1h));
    lp.Wf2h = reinterpret_cast<const _Float16*>(P(o.Wf2h));
    lp.bf1 = P(o.bf1); lp.bf2 = P(o.bf2);
    lp.lnr_g = P(o.lnr_g); lp.lnr_b = P(o.lnr_b);
    lp.W1p = P(o.W1p); lp.W2p = P(o.W2p); lp.W3p = P(o.W3p); lp.Wqp = P(o.Wqp); lp.Wkp = P(o.Wkp); lp.Wf1p = P(o.Wf1p); lp.Wf2p = P(o.Wf2p);
  }
  h->layersT.assign(L, scann_handle::LayerT{});
  for (int i = 0; i < L; ++i) {
    auto PH = [&](size_t o) { return reinterpret_cast<const _Float16*>(P(o)); };
    h->layersT[i] = scann_handle::LayerT{P(lto[i].W1T), P(lto[i].W2T), P(lto[i].W3T), P(lto[i].WqT), P(lto[i].WkT), P(lto[i].Wf1T), P(lto[i].Wf2T),
                                         PH(lto[i].W1Th), PH(lto[i].W2Th), PH(lto[i].W3Th), PH(lto[i].WqTh), PH(lto[i].WkTh), PH(lto[i].Wf1Th),
                                         PH(lto[i].Wf2Th)};
  }
  h->WaT = P(oWaT); h->WgqT = P(oWgqT); h->WgkT = P(oWgkT);
  h->WaTh = reinterpret_cast<const _Float16*>(P(oWaTh));
  h->arena_floats = img.size(); h->o_lut = olut; h->o_emb = oemb; h->o_Wde = oWe; h->o_bde = obe;
  h->head = HeadParams{P(oWa), P(oba), P(oWgq), P(obgq), P(oWgk), P(obgk),
                       reinterpret_cast<const _Float16*>(P(oWah)), reinterpret_cast<const _Float16*>(P(oWgqh)),
                       reinterpret_cast<const _Float16*>(P(oWgkh)), P(oWb), P(obb), P(owo), P(obo)};
  h->basis = BasisParams{P(oWd), P(obd), P(oWw), P(obw), P(ocd), P(ocw), reinterpret_cast<const _Float16*>(P(oWdh)),
                         reinterpret_cast<const _Float16*>(P(oWwh))};
  h->cd = P(ocd);
  h->lut = P(olut);
  h->embed = EmbedArgs{};
  h->embed.emb_dim = c.embedding_dim;
  h->embed.emb = P(oemb); h->embed.We = P(oWc); h->embed.be = P(obc); h->embed.Wr = P(oWr); h->embed.br = P(obr);
  h->embed.Wde = P(oWe); h->embed.bde = P(obe);
  h->sp_dirty = true;
  if (!general_embed && !h->sp_c && c.g_update) {  // c | P1 | P3 | q tables of the first layer, one allocation
    const size_t tab = (size_t)c.n_atoms * D;
    HIPCHK(h, hipMalloc((void**)&h->sp_c, 4 * tab * sizeof(float)));
    h->sp_P1 = h->sp_c + tab; h->sp_P3 = h->sp_c + 2 * tab; h->sp_q = h->sp_c + 3 * tab;
  }
  if (!general_embed) {
    // Embedding + dense_embed folded into a per-species table, computed on the device.
    launch_embed_lut(P(oemb), P(oWe), P(obe), c.n_atoms, c.embedding_dim, h->d_weights + olut, h->streams[0]);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->streams[0]));
  }
  h->loaded = true;
  return SCANN_OK;
}

}  // namespace scann

extern "C" {

int scann_set_debug(scann_handle_t* h, int on) {
  if (!h) return SCANN_ERR_INVALID;
  if (on && h->generic) return fail(h, SCANN_ERR_UNSUPPORTED, "scann_set_debug: per-layer intermediates exist for the 128-wide kernels only");
  h->debug = on != 0;
  return SCANN_OK;
}

int scann_sync(scann_handle_t* h) {
  if (!h) return SCANN_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  for (int i = 0; i < h->nstream; ++i) HIPCHK(h, hipStreamSynchronize(h->streams[i]));
  return SCANN_OK;
}

}  // extern "C"

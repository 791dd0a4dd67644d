// Plan of a training backward under a per-tensor learning-rate scale (scann_set_lr_scale), host only and without a handle
// (scann_plan_check.cpp includes it without a device): the stage of a tensor, the floor of a scale vector, which stages of
// backward_impl's schedule run and which weight-gradient jobs are queued.  A pure function of the layer count, the tensor names and the
// scales; backward_impl asks it and launches accordingly.  Definitions: include/scann_hip.h ("fine-tuning").  Internal.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace scann {

// Stage of a tensor of a model with L LocalAttention layers: 0 the leaves (embedding, basis MLP), l + 1 layer l (LocalAttention with the
// base branch's per-layer filter_geo, ResidualNorm), L + 1 after_Lc and GlobalAttention, L + 2 the property head.  -1: no such tensor.
inline int tensor_stage(const char* name, int L) {
  if (!name || L < 0) return -1;
  const char* slash = strchr(name, '/');
  if (!slash || slash == name || !slash[1]) return -1;
  const std::string top(name, (size_t)(slash - name));
  for (const char* leaf : {"embed_atom", "extra_embed", "dense_embed", "neighbor_d", "neighbor_w"})
    if (top == leaf) return 0;
  for (const char* pre : {"local_attention_", "residual_norm_"}) {
    const size_t n = strlen(pre);
    if (top.compare(0, n, pre) != 0) continue;
    const std::string num = top.substr(n);
    if (num.empty() || num.size() > 6 || (num.size() > 1 && num[0] == '0')) return -1;
    for (char ch : num)
      if (ch < '0' || ch > '9') return -1;
    const long l = strtol(num.c_str(), nullptr, 10);
    return l < L ? (int)l + 1 : -1;
  }
  if (top == "after_Lc" || top == "global_attention") return L + 1;
  if (top == "bf_property" || top == "predict_property") return L + 2;
  return -1;
}

struct TrainPlan {
  int L = 0;
  int floor = 0;           // the lowest stage that holds a tensor with scale > 0 (no scale set: 0)
  std::vector<char> live;  // per tensor, scann_weight_name order: scale > 0.  Empty: no scale set, every tensor is live

  // ---- which stages run ----
  bool leaves() const { return floor == 0; }                // bwd_basis_leaf, bwd_embed_leaf and the Pend::flush into them
  bool layer(int l) const { return l + 1 >= floor; }        // ResidualNorm, attention, geometry / base branch, gradient launch, reduction
  int lowest_layer() const { return floor > 0 ? floor - 1 : 0; }  // the layer loop runs l = L - 1 .. lowest_layer()
  // the data gradients leaving layer l (d centres, d geometry) have a consumer: a launch whose only output they are is dropped otherwise
  bool feeds_below(int l) const { return l + 1 > floor; }
  bool readout_body() const { return floor <= L + 1; }      // after_Lc / GlobalAttention: their data gradient and weight gradients
  // ---- which jobs are kept ----
  bool tensor_live(int i) const { return live.empty() || (i >= 0 && (size_t)i < live.size() && live[(size_t)i]); }
  // a weight-gradient job writes a kernel and (bias >= 0) a bias: queued while either is trained
  bool keep_job(int kernel, int bias) const { return tensor_live(kernel) || (bias >= 0 && tensor_live(bias)); }
  uint64_t stage_bits() const {  // the stages a backward under this plan enters
    uint64_t m = 0;
    for (int s = floor; s <= L + 2 && s < 64; ++s) m |= (uint64_t)1 << s;
    return m;
  }
};

// scale: one factor per name, or null for "no scale set".  Names of no stage (none in a handle's list) count as leaves.
inline TrainPlan train_plan(int L, const std::vector<std::string>& names, const float* scale) {
  TrainPlan p;
  p.L = L;
  if (!scale) return p;
  p.live.resize(names.size());
  p.floor = L + 2;
  for (size_t i = 0; i < names.size(); ++i) {
    p.live[i] = scale[i] > 0.f;
    if (!p.live[i]) continue;
    const int st = tensor_stage(names[i].c_str(), L);
    p.floor = std::min(p.floor, st < 0 ? 0 : st);
  }
  return p;
}

}  // namespace scann

// Stand-alone check of the fine-tuning backward's plan (scann_train_plan.h) for the sanitizers: `make asan-plan` compiles it under
// AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  It builds the tensor list of both branches (with ring +
// cgcnn, with and without ResidualNorm) at L = 0, 1, 2 and 7 with each tensor's stage known by construction, and compares, for every
// floor and for scale vectors with frozen holes above the floor, every answer of the plan against a brute-force restatement: a stage
// runs iff some tensor at or below it is trained; a data gradient has a consumer iff some tensor strictly below is trained.
#include "scann_train_plan.h"

#include "scann_check.h"

namespace {

using namespace scann;

struct Named {
  std::string name;
  int stage;
};

std::vector<Named> tensors(int L, bool g_update, bool general, bool attn_norm) {
  std::vector<Named> t;
  auto dense = [&](const std::string& p, int st) {
    t.push_back({p + "/kernel", st});
    t.push_back({p + "/bias", st});
  };
  auto norm = [&](const std::string& p, int st) {
    t.push_back({p + "/gamma", st});
    t.push_back({p + "/beta", st});
  };
  if (general) {
    dense("embed_atom", 0);
    dense("extra_embed", 0);
  } else {
    t.push_back({"embed_atom/embeddings", 0});
  }
  dense("dense_embed", 0);
  if (g_update) {
    dense("neighbor_d", 0);
    dense("neighbor_w", 0);
  }
  for (int l = 0; l < L; ++l) {
    const std::string la = "local_attention_" + std::to_string(l), rn = "residual_norm_" + std::to_string(l);
    dense(la + "/query", l + 1);
    dense(la + "/key", l + 1);
    dense(la + "/filter_geo", l + 1);
    norm(la + "/layer_norm", l + 1);
    if (g_update) norm(la + "/layer_norm_g", l + 1);
    if (attn_norm) {
      dense(rn + "/dense_1", l + 1);
      dense(rn + "/dense_2", l + 1);
      norm(rn + "/layer_norm", l + 1);
    }
  }
  dense("after_Lc", L + 1);
  dense("global_attention/query", L + 1);
  dense("global_attention/key", L + 1);
  dense("bf_property", L + 2);
  dense("predict_property", L + 2);
  return t;
}

// some tensor of a stage <= `stage` is trained
bool trained_at_or_below(const std::vector<Named>& t, const std::vector<float>& s, int stage) {
  for (size_t i = 0; i < t.size(); ++i)
    if (s[i] > 0.f && t[i].stage <= stage) return true;
  return false;
}

void check_one(int L, const std::vector<Named>& t, const std::vector<float>& s) {
  std::vector<std::string> names;
  for (const Named& n : t) names.push_back(n.name);
  const TrainPlan p = train_plan(L, names, s.data());
  int floor = -1;
  for (int st = 0; st <= L + 2 && floor < 0; ++st)
    if (trained_at_or_below(t, s, st)) floor = st;
  EXPECT(floor >= 0 && p.floor == floor && p.L == L);
  EXPECT(p.leaves() == trained_at_or_below(t, s, 0));
  EXPECT(p.readout_body() == trained_at_or_below(t, s, L + 1));
  int lowest = L;
  for (int l = 0; l < L; ++l) {
    EXPECT(p.layer(l) == trained_at_or_below(t, s, l + 1));
    EXPECT(p.feeds_below(l) == trained_at_or_below(t, s, l));
    if (p.layer(l)) lowest = std::min(lowest, l);
  }
  // the layer loop l = L - 1 .. lowest_layer() visits exactly the layers that run
  for (int l = 0; l < L; ++l) EXPECT((l >= p.lowest_layer()) == p.layer(l));
  if (lowest < L) EXPECT(p.lowest_layer() == lowest);
  else EXPECT(p.lowest_layer() >= L);
  uint64_t bits = 0;
  for (int st = 0; st <= L + 2; ++st)
    if (trained_at_or_below(t, s, st)) bits |= (uint64_t)1 << st;
  EXPECT(p.stage_bits() == bits);
  for (size_t i = 0; i < t.size(); ++i) {
    EXPECT(p.tensor_live((int)i) == (s[i] > 0.f));
    EXPECT(p.keep_job((int)i, -1) == (s[i] > 0.f));
    if (i + 1 < t.size()) EXPECT(p.keep_job((int)i, (int)i + 1) == (s[i] > 0.f || s[i + 1] > 0.f));
  }
  EXPECT(!p.tensor_live(-1) && !p.tensor_live((int)t.size()));
}

void check_plans() {
  for (int L : {0, 1, 2, 7})
    for (int v = 0; v < 8; ++v) {
      const bool g_update = v & 1, general = v & 2, attn_norm = v & 4;
      const std::vector<Named> t = tensors(L, g_update, general, attn_norm);
      for (const Named& n : t) EXPECT(tensor_stage(n.name.c_str(), L) == n.stage);
      {  // no scale set: everything runs, every job is kept
        std::vector<std::string> names;
        for (const Named& n : t) names.push_back(n.name);
        const TrainPlan p = train_plan(L, names, nullptr);
        EXPECT(p.floor == 0 && p.leaves() && p.readout_body() && p.lowest_layer() == 0 && p.live.empty());
        EXPECT(p.stage_bits() == (((uint64_t)1 << (L + 3)) - 1));
        for (size_t i = 0; i < t.size(); ++i) EXPECT(p.tensor_live((int)i) && p.keep_job((int)i, -1));
        for (int l = 0; l < L; ++l) EXPECT(p.layer(l) && p.feeds_below(l));
      }
      for (int f = 0; f <= L + 2; ++f) {
        std::vector<float> s(t.size());
        for (size_t i = 0; i < t.size(); ++i) s[i] = t[i].stage >= f ? 1.0f : 0.f;
        check_one(L, t, s);
        // frozen holes above the floor, fractional rates: one tensor of stage f alone, then every third tensor at or above it
        size_t first = t.size();
        for (size_t i = 0; i < t.size() && first == t.size(); ++i)
          if (t[i].stage == f) first = i;
        EXPECT(first < t.size());
        std::vector<float> one(t.size(), 0.f);
        one[first] = 0.25f;
        check_one(L, t, one);
        std::vector<float> holes(t.size(), 0.f);
        holes[first] = 1e-30f;
        for (size_t i = first; i < t.size(); i += 3)
          if (t[i].stage >= f) holes[i] = 0.1f;
        check_one(L, t, holes);
      }
    }
}

void check_names() {
  for (int L : {0, 2, 7}) {
    for (const char* bad : {"", "/", "after_Lc", "after_Lc/", "/kernel", "bogus/kernel", "local_attention_/query/kernel",
                            "local_attention_x/query/kernel", "local_attention_-1/query/kernel", "local_attention_01/query/kernel",
                            "local_attention_7/query/kernel", "residual_norm_7/dense_1/kernel", "residual_norm_9999999999/dense_1/kernel",
                            "local_attention/query/kernel", "Embed_atom/embeddings"})
      EXPECT(tensor_stage(bad, L) == -1);
    EXPECT(tensor_stage(nullptr, L) == -1);
    EXPECT(tensor_stage("embed_atom/embeddings", L) == 0 && tensor_stage("global_attention/key/bias", L) == L + 1 &&
           tensor_stage("predict_property/bias", L) == L + 2);
  }
  EXPECT(tensor_stage("local_attention_6/query/kernel", 7) == 7 && tensor_stage("local_attention_0/key/bias", 0) == -1);
  EXPECT(tensor_stage("after_Lc/kernel", -1) == -1);
}

}  // namespace

int main() {
  check_plans();
  check_names();
  return finish("scann_plan_check");
}

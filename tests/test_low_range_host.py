"""Host: the low end of the split-fp16 projections, on the NumPy emulation of the scheme (tests/split_ref.py) -- what keeps
tests/test_gpu_low_range.py honest.  For every case and k of the GPU tests:

1. the fp32 oracle alone is far inside the acceptance bound, so the bound max(1e-4, 2 x the fp32 oracle's error) IS 1e-4 and a
   failure of the GPU is the GPU's;
2. the emulated UNGUARDED scheme leaves it at k = 14 for cases A, B, D and E (P: at k = 6 and 10), so the GPU tests fail on a forward that does nothing
   about small operands.  Case W does not leave it (measured: after_Lc 3.0e-5, context_2 2.5e-5 at k = 14, 2.9e-5 / 3.2e-5 at
   k = 18, bound 1e-4): with key and query kernels AND biases at 2^-14 the layer's context has a variance of 7e-9 per row, below
   LayerNorm's epsilon of 1e-6, which divides the error by ~12 before anybody reads it.  What W does break is the claim
   test_split_fp16_projections_reach_fp32_accuracy states -- within max(2 x the fp32 oracle's error, 2e-6) of fp64 -- by a factor of
   ten; that is what is asserted for W here, and the GPU tests keep W as a regression case under the one acceptance rule;
3. the guarded scheme -- the exact-fp32 kernels (= the fp32 oracle) where the load-time rule fires, the split elsewhere -- meets
   the bound at every k, with the largest error among the checkpoints the rule lets through printed;
4. the rule raises no false alarm: the default checkpoints, k = 0 of every case, the mixed rows of case M at every k, and exact zeros.
"""
import numpy as np
import pytest

import scann_oracle as so
import split_ref as sr

VARIANTS = [(c, {}) for c in sr.CASES] + [("A", dict(g_update=False)), ("A_no_attn_norm", dict(use_attn_norm=False)), ("E", dict(g_update=False))]
IDS = ["%s%s" % (c, "".join("-%s=%s" % kv for kv in m.items())) for c, m in VARIANTS]


@pytest.fixture(scope="module")
def sweep():
    """(case, model overrides as a sorted tuple, k) -> dict(reason, rows of the fp32 oracle / the unguarded split / the guarded scheme),
    computed on first use"""
    store = {}

    def get(case, model, k):
        key = (case, tuple(sorted(model.items())), k)
        if key not in store:
            cfg = sr.config(**model)
            w = sr.scaled(so.init_weights(cfg, 1234, perturb=True), case, k)
            de, dn = so.synth_dataset(8, 0)
            inputs, _ = so.pad_batch(de, dn, cfg["model"]["g_update"])
            r32, r64 = sr.references(cfg, w, inputs)
            reason = sr.small_operands(cfg, w)
            split = sr.outputs_of(cfg, inputs, lambda it: sr.forward_split(cfg, w, inputs, it))
            store[key] = dict(reason=reason, e32={n: sr.rel_err(r32[n], r64[n]) for n in r64}, split=sr.judge(split, r32, r64),
                              guarded=sr.judge(r32 if reason else split, r32, r64))
        return store[key]

    return get


def test_split_matmul_is_the_scheme():
    """the emulation against the issue's own table: error / sum |a b| of one 128 x 128 product at operand magnitude s -- 22 bits
    at s = 1, an absolute quantum below (the error grows as 1 / s) -- and the cases that fix the rounding: a value whose lo part is
    an fp16 subnormal keeps it (gradual underflow), one below 2^-25 is lost, one beyond 65504 is inf"""
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-1, 1, (128, 128)).astype(np.float32), rng.uniform(-1, 1, (128, 128)).astype(np.float32)
    err = {}
    for s in (1.0, 1e-2, 1e-3, 1e-4, 1e-5):
        x, y = (a * np.float32(s)).astype(np.float32), (b * np.float32(s)).astype(np.float32)
        ref = x.astype(np.float64) @ y.astype(np.float64)
        err[s] = float(np.max(np.abs(sr.split_matmul(x, y) - ref) / (np.abs(x).astype(np.float64) @ np.abs(y).astype(np.float64))))
    print(err)
    assert err[1.0] <= 2e-7 and err[1e-2] <= 5e-6  # fp32 grade while lo is normal (the issue: 5e-8, 9e-7)
    assert err[1e-5] > 50 * err[1e-3] > 50 * 50 * err[1.0] * 0.01  # ~1 / s below
    assert 2e-5 < err[1e-4] < 1e-3 and 2e-4 < err[1e-5] < 1e-2  # the issue's 1e-4 and 9e-4, within a factor of 5 either way
    hi, lo = sr.split(np.float32([2.0 ** -10 + 2.0 ** -23, 2.0 ** -26, 1.0 + 2.0 ** -20, 70000.0]))
    assert hi[0] == 2.0 ** -10 and lo[0] == 2.0 ** -23  # a subnormal lo is kept ...
    assert hi[1] == 0 and lo[1] == 0  # ... a value below half the smallest subnormal is not
    assert hi[2] == 1.0 and lo[2] == 2.0 ** -20 and np.isinf(hi[3])


@pytest.mark.parametrize("case,model", VARIANTS, ids=IDS)
def test_the_fp32_oracle_alone_is_far_inside_the_bound(sweep, case, model):
    for k in sr.KS:
        e32 = sweep(case, model, k)["e32"]
        print(case, model, k, "fp32 oracle worst %.1e (%s)" % (max(e32.values()), max(e32, key=e32.get)))
        assert max(e32.values()) <= sr.RTOL / 10, (k, e32)


def test_a_product_of_two_moderately_small_rows_leaves_the_bound(sweep):
    """case P: the key projection's operand is centres x geometry.  At k = 6 each factor alone is harmless (cases A and B stay at
    5e-6) and above the rule's 2^-8, their product is at 2^-12: the unguarded scheme is at 1.7e-4 (k = 6) and 4e-4 (k = 10)"""
    for k in (6, 10):
        r = sweep("P", {}, k)
        print("P", k, "unguarded, outside the bound:", [(n, "%.1e" % e) for n, e, _ in sr.failures(r["split"])])
        assert sr.failures(r["split"]) and r["reason"] is not None, (k, r["reason"])
    assert "key: its operand rows" in sweep("P", {}, 6)["reason"]  # (at k = 10 the centres alone are below 2^-8, which is found first)
    assert not sr.failures(sweep("A", {}, 6)["split"]) and not sr.failures(sweep("B", {}, 6)["split"])
    assert sweep("A", {}, 6)["reason"] is None and sweep("B", {}, 6)["reason"] is None


@pytest.mark.parametrize("case", ["A", "B", "D", "E"])
def test_the_unguarded_scheme_leaves_the_bound_at_k14(sweep, case):
    for k in (14, 18):
        r = sweep(case, {}, k)
        public = sr.failures([row for row in r["split"] if row[0] in sr.output_names(sr.config())])
        print(case, k, "unguarded, outside the bound:", [(n, "%.1e" % e) for n, e, _ in sr.failures(r["split"])])
        assert public, (case, k, r["split"])  # at least one tensor of the public API
    assert not sr.failures(sweep(case, {}, 0)["split"]) and not sr.failures(sweep(case, {}, 6)["split"])


def test_small_kernels_cost_the_split_its_fp32_accuracy(sweep):
    """case W (module docstring): inside 1e-4 because LayerNorm's epsilon dilutes it, but ten times the fp32 oracle's error"""
    for k in (14, 18):
        r = sweep("W", {}, k)
        worst = {row[0]: row[1] for row in r["split"]}
        print("W", k, {n: "%.1e (fp32 %.1e)" % (worst[n], r["e32"][n]) for n in ("context_2", "centers_2", "after_Lc")})
        assert not sr.failures(r["split"])
        for n in ("context_2", "after_Lc"):
            assert worst[n] > 10 * max(r["e32"][n], 1e-6), (n, worst[n], r["e32"][n])
    worst = {row[0]: row[1] for row in sweep("W", {}, 0)["split"]}
    assert all(worst[n] <= max(2 * sweep("W", {}, 0)["e32"][n], 2e-6) for n in worst), worst


@pytest.mark.parametrize("case,model", VARIANTS, ids=IDS)
def test_the_guarded_scheme_meets_the_bound_at_every_k(sweep, case, model):
    for k in sr.KS:
        r = sweep(case, model, k)
        worst = max(r["guarded"], key=lambda row: row[1] / row[2])
        print(case, model, k, "exact:" if r["reason"] else "split:", "%s %.1e of %.1e" % worst[:3], "|", r["reason"])
        assert not sr.failures(r["guarded"]), (k, r["reason"], sr.failures(r["guarded"]))
        if k == 0 or case == "M":
            assert r["reason"] is None, (k, r["reason"])  # a row's largest element decides its precision, not its smallest
        if k >= 14 and case != "M":
            assert r["reason"] is not None, (case, k)
        if case == "E" and k >= 6:
            assert r["reason"].startswith("dense_embed"), r["reason"]


def test_the_rule_lets_every_split_checkpoint_through_with_room(sweep):
    """the threshold was derived (2^-25 against a largest element of 2^-8 is 2^-17 per operand), not fitted: what it lets through
    sits at most at a quarter of the bound in the emulation, and what it sends to the exact kernels includes every checkpoint of the
    sweep beyond that"""
    for case, model in VARIANTS:
        for k in sr.KS:
            r = sweep(case, model, k)
            if r["reason"] is None:
                assert max(row[1] / row[2] for row in r["split"]) <= 0.25, (case, model, k, r["split"])


def test_ordinary_checkpoints_and_exact_zeros_are_no_false_alarm():
    for label, cfg, w, _ in sr.ordinary_checkpoints():
        assert sr.small_operands(cfg, w) is None, label
    cfg = sr.config()
    w = so.init_weights(cfg, 1234, perturb=True)
    z = dict(w)  # exact zeros are representable: a pruned column, a LayerNorm switched off, zero biases
    z["local_attention_1/key/kernel"] = w["local_attention_1/key/kernel"].copy()
    z["local_attention_1/key/kernel"][:, 5] = 0
    z["local_attention_0/filter_geo/kernel"] = w["local_attention_0/filter_geo/kernel"].copy()
    z["local_attention_0/filter_geo/kernel"][128:256] = 0
    for n in ("local_attention_1/layer_norm_g/gamma", "local_attention_1/layer_norm_g/beta", "after_Lc/bias"):
        z[n] = np.zeros_like(w[n])
    assert sr.small_operands(cfg, z) is None
    # every branch of the rule names the tensor that trips it
    for name, want in (("local_attention_0/filter_geo/kernel", "filter_geo"), ("global_attention/key/kernel", "global_attention/key"),
                       ("local_attention_0/layer_norm/gamma+beta", "local_attention_0/layer_norm"), ("residual_norm_1/dense_2/kernel", "dense_2")):
        s = dict(w)
        for n in ([name] if "+" not in name else [name.split("/gamma")[0] + "/gamma", name.split("/gamma")[0] + "/beta"]):
            s[n] = (w[n] * np.float32(2.0 ** -15)).astype(np.float32)
        assert want in (sr.small_operands(cfg, s) or ""), (name, sr.small_operands(cfg, s))
    # the generic widths run plain fp32: nothing to classify
    g = sr.config(local_dim=64, num_head=4)
    assert sr.small_operands(g, {}) is None


def test_far_edges_keep_the_k20_filters_in_range():
    """case G: neighbor_distance 1 A and 2 A beyond the last Gaussian centre makes every Gaussian of the row tiny (exp(-4), exp(-16)
    at best) -- but those are operands of the K = 20 filters, whose inputs live in [0, 1] against a bias of O(0.1): an absolute
    quantum of 2^-25 is harmless there, and the emulation (which leaves those filters in fp32) and the fp32 oracle agree with fp64"""
    for g_update in (True, False):
        cfg = sr.config(g_update=g_update)
        w = so.init_weights(cfg, 1234, perturb=True)
        de, dn = so.synth_dataset(8, 0)
        inputs = sr.far_edges(so.pad_batch(de, dn, g_update)[0], cfg)
        far = inputs["neighbor_distance"][inputs["neighbor_mask"]] > cfg["model"]["gaussian_d"]
        assert 0.2 < far.mean() < 0.3
        r32, r64 = sr.references(cfg, w, inputs)
        split = sr.outputs_of(cfg, inputs, lambda it: sr.forward_split(cfg, w, inputs, it))
        assert not sr.failures(sr.judge(split, r32, r64)) and max(sr.rel_err(r32[n], r64[n]) for n in r64) <= sr.RTOL / 10
